"""Checking the ZeRO-1 gather waits.

Under ZeRO-1 (parallel/zero.py) the updated bf16 weights are all-gathered in
place, bucket by bucket, while the next forward already runs.  What keeps a
kernel from reading a weight whose bucket is still mid-gather is a
convention: the forward pre-hooks of train/llm.py ``_install_param_waits``
wait for a module's buckets, so a read that does not go through the owning
module's call reads half-gathered weights, silently and only when the gather
happens to be late.  Two opt-in instruments turn that into an invariant:

* the host check (``TOA_ZERO_CHECK=1``): :class:`zero.ParamGather` tags the
  parameters of its buckets, and every place that hands a weight to a kernel
  calls :func:`reading` while the ``Parameter`` is still the object in hand;
  a read of a bucket launched and not yet waited raises
  :class:`ZeroGatherError` naming the parameter, the op and the bucket;
* the device proof (``TOA_ZERO_POISON=1``, ``TOA_ZERO_AG_DELAY_US=n``): the
  shards a rank does not own are overwritten with NaN before their gather
  starts and the gather is held back (csrc/hip/comm.hip ``toa_zero_poison``,
  ``toa_delay_us``), so ANY unwaited read gives a non-finite loss, also one
  that nobody instrumented.

With the switches unset no parameter carries the tag and :func:`reading`
costs one ``getattr``.
"""
from __future__ import annotations

import os
import weakref

AG_DELAY_CAP_US = 100000  # csrc/hip/comm.hip TOA_DELAY_CAP_US: toa_delay_us refuses more


class ZeroGatherError(RuntimeError):
    """A weight was handed to a kernel while its bucket's all-gather was in flight."""


def check_from_env() -> bool:
    return os.environ.get("TOA_ZERO_CHECK", "0") == "1"


def poison_from_env() -> bool:
    return os.environ.get("TOA_ZERO_POISON", "0") == "1"


def ag_delay_us_from_env() -> int:
    return int(os.environ.get("TOA_ZERO_AG_DELAY_US", "0") or 0)


def validate_delay_us(us) -> int:
    us = int(us)
    if not 0 <= us <= AG_DELAY_CAP_US:
        raise ValueError(f"zero_ag_delay_us / TOA_ZERO_AG_DELAY_US = {us}: must be 0 .. {AG_DELAY_CAP_US}")
    return us


def tag(gather, params_per_bucket, names):
    """Link every parameter of `gather`'s buckets to it (a weak reference:
    the gather holds the flat buffers that hold the parameters)."""
    ref = weakref.ref(gather)
    for b, ps in enumerate(params_per_bucket):
        for p in ps:
            p._toa_gather = ref
            p._toa_bucket = b  # what the bucketer set already when the buckets are its own
            p._toa_name = names.get(id(p), "?")


def reading(param, op: str):
    """`param` is about to be read by `op`: raise if its bucket's all-gather
    was launched and not waited for.  Anything but a tagged parameter passes."""
    ref = getattr(param, "_toa_gather", None)
    if ref is None:
        return
    gather = ref()
    if gather is None:
        return
    b = param._toa_bucket
    if gather.works[b] is not None:
        lo, hi = gather.ranges[b]
        raise ZeroGatherError(
            f"{op} reads {param._toa_name} while the all-gather of its bucket {b} (flat [{lo}, {hi})) is in "
            "flight: no ParamGather.wait ran for it (a read outside its owning module's call skips the "
            "forward pre-hook that waits, train/llm.py _install_param_waits)")
