"""The ZeRO-1 gather-wait check on the host (parallel/zero_check.py,
``TOA_ZERO_CHECK``): a weight handed to a kernel while its bucket's
all-gather is launched and not waited for raises ``ZeroGatherError`` naming
the parameter; a correct trainer never raises and computes the same bits."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tf_operator_amd.parallel import zero, zero_check
from tf_operator_amd.parallel.flat import FlatParams
from tf_operator_amd.parallel.zero_check import ZeroGatherError, reading


class _Work:
    """Stand-in for a collective's work handle."""

    def __init__(self):
        self.waited = False

    def wait(self):
        self.waited = True


def _small_gather(monkeypatch, check):
    ps = [torch.nn.Parameter(torch.randn(16, 8)), torch.nn.Parameter(torch.randn(64)),
          torch.nn.Parameter(torch.randn(8, 16))]
    flat = FlatParams(ps, names={id(p): n for p, n in zip(ps, ("a.weight", "a.gain", "b.weight"))})
    buckets = [(0, 192), (192, 320)]   # a.weight + a.gain | b.weight, each a multiple of 8 x world
    assert zero.feasible(buckets, 2) and flat.numel == 320
    monkeypatch.setattr(zero, "all_gather_", lambda *a, **k: _Work())
    return ps, zero.ParamGather(flat, buckets, 0, 2, check=check)


def test_reading_raises_between_launch_and_wait(monkeypatch):
    ps, g = _small_gather(monkeypatch, check=True)
    for p in ps:
        reading(p, "before any gather")
    g.launch_one(1)
    reading(ps[0], "other bucket")
    reading(ps[1], "other bucket")
    with pytest.raises(ZeroGatherError) as e:
        reading(ps[2], "unit-op")
    assert "b.weight" in str(e.value) and "unit-op" in str(e.value) and "bucket 1" in str(e.value)
    g.launch_one(0)
    for p, name in ((ps[0], "a.weight"), (ps[1], "a.gain")):
        with pytest.raises(ZeroGatherError, match=name):
            reading(p, "unit-op")
    g.wait(1)
    reading(ps[2], "after wait")
    with pytest.raises(ZeroGatherError, match="a.gain"):
        reading(ps[1], "unit-op")
    g.wait_all()
    for p in ps:
        reading(p, "after wait_all")


def test_reading_never_raises_with_the_check_off(monkeypatch):
    ps, g = _small_gather(monkeypatch, check=False)
    assert not any(hasattr(p, "_toa_gather") for p in ps)
    g.launch()
    assert all(w is not None for w in g.works)
    for p in ps:
        reading(p, "check off")
    reading(torch.zeros(3), "a plain tensor")
    reading(None, "no tensor")


def test_delay_above_the_cap_is_a_value_error():
    from tf_operator_amd.train.llm import LlamaTrainer

    assert zero_check.AG_DELAY_CAP_US == 100000
    with pytest.raises(ValueError, match="100000"):
        LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=32, zero_ag_delay_us=100001)
    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=32, zero_ag_delay_us=100000)
    assert tr.zero_ag_delay_us == 100000 and not tr.zero_check and not tr.zero_poison


# ---------------------------------------------------------------- gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


STEPS = 3


def _run_arm(check, drop_hook):
    """One llama-tiny ZeRO-1 job: (losses of the steps that ran, error or None)."""
    from tf_operator_amd.train.llm import LlamaTrainer

    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=128, lr=1e-3, bucket_mb=0.25,
                      shard_optimizer=True, zero_check=check)
    assert tr.gather is not None and len(tr.bucketer.buckets) > 2
    assert sorted(tr._hook_by_module.values(), key=id) == sorted(tr._hooks, key=id)
    if drop_hook:
        tr._hook_by_module[drop_hook].remove()
    b = tr.synthetic_batch()
    losses, err = [], None
    try:
        for _ in range(STEPS):
            losses.append(float(tr.step([b])))
    except ZeroGatherError as e:   # raised on the host before the read: every rank stops at the same point
        err = str(e)
    tr.gather.wait_all()
    return losses, err


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {"off": _run_arm(False, None), "on": _run_arm(True, None),
               "no_final_norm_hook": _run_arm(True, "norm"),
               "no_block_norm_hook": _run_arm(True, "blocks.1.mlp_norm")}
        torch.save(res, f"{out}.{rank}")
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("zero_check") / "res")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]


def test_check_on_changes_no_bit_and_raises_nothing(arms):
    for r in arms:
        (l_off, e_off), (l_on, e_on) = r["off"], r["on"]
        assert e_off is None and e_on is None, (e_off, e_on)
        assert len(l_on) == STEPS and l_on == l_off, (l_on, l_off)
        assert l_on[-1] < l_on[0]


def test_removed_final_norm_hook_raises_on_every_rank(arms):
    """The round-6 incident: the final norm's hook carries the lm_head wait."""
    for r in arms:
        losses, err = r["no_final_norm_hook"]
        assert losses == r["on"][0][:1], losses   # step 0 ran (no gather before it) and step 1 raised
        assert err is not None and ("norm.weight" in err or "lm_head" in err), err


def test_removed_block_norm_hook_is_no_hazard(arms):
    """A block's norm weight shares its bucket with wo / wgu, which the
    block's own hook waits for first: no unwaited read, so no error."""
    for r in arms:
        losses, err = r["no_block_norm_hook"]
        assert err is None, err
        assert losses == r["on"][0]
