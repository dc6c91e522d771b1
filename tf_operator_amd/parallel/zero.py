"""Sharded optimizer data parallelism (ZeRO stage 1) on the flat buffers.

Plain DP (:class:`GradBucketer` with all-reduce) has every rank run the
full AdamW: 28 B of HBM traffic per parameter, 43 ms per step at
Llama-3-8B on one MI355X, whatever the world size.  Here each gradient
bucket is split into ``world`` equal contiguous shards and

1. backward: as a bucket's gradients complete, ``reduce_scatter`` (RCCL,
   in place on the flat gradient buffer) leaves rank r the SUM of its
   shard r -- half the bytes an all-reduce moves, issued at the same time;
2. optimizer: each rank runs AdamW only over the shards it owns (the global
   gradient norm is the all-reduced sum of the per-shard squared norms), so
   the update costs 1/world of the replicated one;
3. the updated bf16 shards are ``all_gather``-ed in place, bucket by
   bucket in FORWARD order, on RCCL's stream; the next forward waits per
   bucket in module pre-hooks (:meth:`ParamGather.wait`), so the gathers of
   late layers run under the GEMMs of early ones.

RS + AG move exactly the bytes of one ring all-reduce, so the xGMI traffic
is unchanged; what shrinks is the optimizer (world x less HBM traffic) and
its exposure at the end of the step.  The fp32 master / m / v are kept
for the owned shards only (``FlatParams.shard_state``), packed: at
Llama-3-8B and world 8 that is 12 GB instead of 96 GB per GPU.  Checkpoints
stay world-size independent: each rank saves its shards with their flat
ranges (train/sharded_ckpt.py) and any other world size re-shards on load;
:func:`gather_full_state` assembles the full state where one is needed.

Shards must be a multiple of 8 elements (16-byte vectors in the AdamW
kernel): with 64-element parameter padding that holds for world 1/2/4/8;
other world sizes fall back to the all-reduce path (:func:`feasible`).

Reference parity: the reference's only collective is the payloads'
gradient all-reduce; sharding the update is the
MI355X-first way of running that same data-parallel step.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import zero_check


def feasible(buckets, world: int) -> bool:
    return world >= 1 and all((e - s) % (8 * world) == 0 for s, e, *_ in buckets)


def owned_ranges(buckets, world: int, rank: int):
    """[(lo, hi)] of the flat buffer this rank updates: shard `rank` of
    every bucket."""
    out = []
    for s, e, *_ in buckets:
        n = (e - s) // world
        out.append((s + rank * n, s + (rank + 1) * n))
    return out


def _is_nccl(group) -> bool:
    return dist.get_backend(group) == "nccl"


def reduce_scatter_(buf: torch.Tensor, rank: int, world: int, group=None, async_op=True):
    """buf[shard rank] <- sum over ranks of buf[shard rank] (in place on
    RCCL; gloo gets an out-of-place output copied back by the returned
    finisher).  Returns (work, finisher)."""
    n = buf.numel() // world
    shard = buf[rank * n:(rank + 1) * n]
    if _is_nccl(group):
        return dist.reduce_scatter_tensor(shard, buf, op=dist.ReduceOp.SUM, group=group, async_op=async_op), None
    out = torch.empty_like(shard)
    w = dist.reduce_scatter_tensor(out, buf, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    return w, (lambda: shard.copy_(out))


def all_gather_(buf: torch.Tensor, rank: int, world: int, group=None, async_op=True):
    """Every rank's shard of `buf` to every rank, in place."""
    n = buf.numel() // world
    return dist.all_gather_into_tensor(buf, buf[rank * n:(rank + 1) * n], group=group, async_op=async_op)


class ParamGather:
    """In-place all-gather of the updated bf16 weights after a sharded
    optimizer step, waited for per bucket by the next forward."""

    def __init__(self, flat, buckets, rank, world, group=None, on_gathered=None, emulator=None, pull=None,
                 check=False, poison=False, delay_us=0):
        """check / poison / delay_us: the instruments of parallel/zero_check.py
        (TOA_ZERO_CHECK, TOA_ZERO_POISON, TOA_ZERO_AG_DELAY_US), all off by default."""
        self.flat = flat
        self.emu = emulator  # parallel/emulate.CommEmulator: paced traffic instead of RCCL (world 1)
        self.pull = pull     # parallel/pull_gather.PullGather: copy-engine pulls instead of RCCL (TOA_ZERO_AG=sdma)
        self.ranges = [(b[0], b[1]) for b in buckets]
        self.rank, self.world, self.group = rank, world, group
        self.on_gathered = on_gathered  # fn(lo, hi) on the waiting stream (W^T refresh)
        self.works = [None] * len(self.ranges)
        self.check, self.poison, self.delay_us = bool(check), bool(poison), zero_check.validate_delay_us(delay_us)
        self._delay_stream = None  # carries the delayed RCCL gathers (never the compute stream)
        if self.check:  # reads of these parameters go through zero_check.reading
            per_bucket = [[] for _ in self.ranges]
            for seg in flat.segments:
                per_bucket[self._bucket_of(seg.offset)].append(seg.param)
            zero_check.tag(self, per_bucket, {id(seg.param): seg.name for seg in flat.segments})

    def _bucket_of(self, offset):
        return next(b for b, (lo, hi) in enumerate(self.ranges) if lo <= offset < hi)

    def _on_device(self):
        """The device instruments apply: real traffic into a GPU buffer."""
        return self.emu is None and self.flat.param.is_cuda

    def _poison_others(self, b):
        """NaN over the shards of bucket b this rank does not own, on the
        current stream: it has run this step's last reader of the old weights
        and this rank's update of its own shard, and the gather that refills
        them is ordered behind it."""
        from ..ops import _lib

        lo, hi = self.ranges[b]
        n = (hi - lo) // self.world
        _lib.call("toa_zero_poison", _lib.ptr(self.flat.param), lo, hi, lo + self.rank * n, lo + (self.rank + 1) * n,
                  _lib.stream(self.flat.param))

    def _delayed_all_gather(self, view):
        """The RCCL gather issued under a side stream that waits for the
        current one and then sits out the delay: the collective is ordered
        behind the delay, the compute stream is not.  work.wait() is unchanged."""
        import ctypes

        from ..ops import _lib

        if self._delay_stream is None:
            self._delay_stream = torch.cuda.Stream(device=view.device)
        side = self._delay_stream
        side.wait_stream(torch.cuda.current_stream(view.device))
        _lib.call("toa_delay_us", self.delay_us, ctypes.c_void_p(side.cuda_stream))
        with torch.cuda.stream(side):
            return all_gather_(view, self.rank, self.world, self.group)

    def order(self):
        """Forward-need order: flat order is backward order, so the forward
        needs the last bucket first."""
        return list(reversed(range(len(self.ranges))))

    def launch_one(self, b):
        """All-gather bucket b (its owned shard must be updated on the
        current stream already: the collective waits for that stream)."""
        lo, hi = self.ranges[b]
        device = self._on_device()
        if self.poison and device:
            self._poison_others(b)
        if self.pull is not None:
            if b == self.order()[0]:
                self.pull.new_step()   # one epoch per optimizer step, the same on every rank
            # the delay rides on the transport's copy stream, ahead of its flags wait
            self.works[b] = (self.pull.launch_one(b, delay_us=self.delay_us) if self.delay_us and device
                             else self.pull.launch_one(b))
        elif self.emu is not None:
            self.works[b] = self.emu.collective(self.flat.param[lo:hi], kind="all_gather")
        elif self.delay_us and device:
            self.works[b] = self._delayed_all_gather(self.flat.param[lo:hi])
        else:
            self.works[b] = all_gather_(self.flat.param[lo:hi], self.rank, self.world, self.group)

    def launch(self):
        for b in self.order():
            self.launch_one(b)

    def wait(self, b):
        w = self.works[b]
        if w is None:
            return
        self.works[b] = None
        w.wait()  # RCCL: the current stream waits, the host does not
        if self.on_gathered is not None:
            self.on_gathered(*self.ranges[b])

    def wait_all(self):
        for b in range(len(self.ranges)):
            self.wait(b)


@torch.no_grad()
def gather_full_state(flat, world, group=None):
    """{master, exp_avg, exp_avg_sq}: full-size tensors, each in its own dtype
    (fp32; bf16 moments stay bf16), assembled from every rank's compact
    shards.  Collective: every rank must call it (every rank holds equally
    many elements: 1/world of each bucket)."""
    out = {}
    ranges = torch.tensor([x for r in flat.state_ranges for x in r], dtype=torch.int64, device=flat.device)
    all_ranges = [torch.empty_like(ranges) for _ in range(world)]
    dist.all_gather(all_ranges, ranges, group=group)
    for k in ("master", "exp_avg", "exp_avg_sq"):
        t = getattr(flat, k)
        if t is None:
            continue
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t.contiguous(), group=group)
        full = torch.zeros(flat.numel, device=t.device, dtype=t.dtype)
        for r, (rg, part) in enumerate(zip(all_ranges, parts)):
            off = 0
            rg = rg.tolist()
            for lo, hi in zip(rg[0::2], rg[1::2]):
                full[lo:hi].copy_(part[off:off + hi - lo])
                off += hi - lo
        out[k] = full
    return out
