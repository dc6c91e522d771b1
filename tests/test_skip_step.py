"""Skipped steps on the host (ops/optim.py FlatAdamW skip_nonfinite /
skip_grad_norm, the CPU reference path): a step whose gradient norm is Inf,
NaN or above the limit leaves master, m, v and the weights untouched, counts
itself, and later steps take their bias corrections and rounding draws from
step - skipped; with ZeRO-1 over gloo every rank skips together."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tf_operator_amd.ops.optim import FlatAdamW
from tf_operator_amd.parallel.flat import FlatParams

DTYPES = [torch.float32, torch.bfloat16]


def _opt(state_dtype=torch.float32, **kw):
    """A small flat buffer: a 2-D weight (decayed) and a 1-D gain (not), so
    the update runs as two launches."""
    g = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(torch.randn(16, 24, generator=g)), torch.nn.Parameter(torch.randn(40, generator=g))]
    flat = FlatParams(ps)
    kw.setdefault("max_grad_norm", 1.0)
    opt = FlatAdamW(flat, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, state_dtype=state_dtype, seed=0x5EED, **kw)
    assert len(opt.runs) > 1
    return flat, opt


def _grad(flat, k, scale=1.0):
    """The gradient of step k: the same for every run that asks for step k."""
    g = torch.Generator().manual_seed(100 + k)
    return (torch.randn(flat.numel, generator=g) * scale).to(flat.grad.dtype)


def _take(flat, opt, g, **kw):
    flat.grad.copy_(g)
    opt.step(**kw)


def _state(flat):
    return [t.clone() for t in (flat.master, flat.exp_avg, flat.exp_avg_sq, flat.param)]


def _same(a, b):
    """Byte-equal: NaN payloads and signed zeros included."""
    return all(x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the guard alone changes no bit
@pytest.mark.parametrize("state_dtype", DTYPES)
def test_guard_on_with_finite_gradients_is_bit_identical(state_dtype):
    runs = []
    for guard in (False, True):
        flat, opt = _opt(state_dtype, skip_nonfinite=guard)
        for k in range(1, 5):
            _take(flat, opt, _grad(flat, k))
        assert opt.skipped_steps() == 0 and opt.step_count == 4
        runs.append(_state(flat))
    assert _same(*runs)
    assert float(runs[0][1].float().abs().max()) > 0


# ------------------------------------------------------------------ 2. one Inf element
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("state_dtype", DTYPES)
def test_nonfinite_step_is_skipped_and_leaves_no_trace(state_dtype, bad):
    flat, opt = _opt(state_dtype, skip_nonfinite=True)
    _take(flat, opt, _grad(flat, 1))
    after1 = _state(flat)
    g2 = _grad(flat, 2)
    g2[37] = bad                                  # a single element of the whole step
    _take(flat, opt, g2)
    assert _same(_state(flat), after1)
    assert opt.skipped_steps() == 1 and opt.step_count == 2
    _take(flat, opt, _grad(flat, 3))
    assert opt.skipped_steps() == 1
    got = _state(flat)
    assert not _same(got, after1)

    ref_flat, ref = _opt(state_dtype, skip_nonfinite=True)   # fed steps 1 and 3 only
    _take(ref_flat, ref, _grad(ref_flat, 1))
    _take(ref_flat, ref, _grad(ref_flat, 3))
    want = _state(ref_flat)
    assert _same(got[1:3], want[1:3])             # m, v: for bf16 moments the rounding key is that of step 2
    assert _same(got, want)                       # host arithmetic with st = step - skipped: the weights too


def test_unguarded_step_is_destroyed_by_the_same_gradient():
    """The control: without the guard one Inf element takes the whole state."""
    flat, opt = _opt(skip_nonfinite=False)
    _take(flat, opt, _grad(flat, 1))
    g2 = _grad(flat, 2)
    g2[37] = float("inf")
    _take(flat, opt, g2)
    assert not bool(torch.isfinite(flat.master).all())
    assert opt.skipped_steps() == 0


def test_guard_without_clipping_still_takes_the_norm():
    flat, opt = _opt(skip_nonfinite=True, max_grad_norm=0.0)
    _take(flat, opt, _grad(flat, 1))
    after1 = _state(flat)
    g2 = _grad(flat, 2)
    g2[0] = float("nan")
    _take(flat, opt, g2)
    assert _same(_state(flat), after1) and opt.skipped_steps() == 1
    # ... and no clip is applied: the step equals the unguarded, unclipped one
    a_flat, a = _opt(skip_nonfinite=True, max_grad_norm=0.0)
    b_flat, b = _opt(skip_nonfinite=False, max_grad_norm=0.0)
    for f, o in ((a_flat, a), (b_flat, b)):
        _take(f, o, _grad(f, 1, scale=50.0))
    assert _same(_state(a_flat), _state(b_flat))


# ------------------------------------------------------------------ 3. the norm limit
def test_skip_grad_norm_limit():
    flat, opt = _opt(skip_nonfinite=True)
    g = _grad(flat, 1)
    norm = float(g.float().pow(2).sum().sqrt())
    flat, opt = _opt(skip_nonfinite=True, skip_grad_norm=1.5 * norm)
    before = _state(flat)
    _take(flat, opt, g * 2)                       # finite, 2 norm > 1.5 norm: skipped
    assert _same(_state(flat), before) and opt.skipped_steps() == 1
    _take(flat, opt, g * 2, grad_scale=0.5)       # the limit is on the scaled norm: applied
    assert not _same(_state(flat), before) and opt.skipped_steps() == 1
    mid = _state(flat)
    _take(flat, opt, g)                           # below the limit: applied
    assert not _same(_state(flat), mid) and opt.skipped_steps() == 1
    _take(flat, opt, g, grad_scale=2.0)           # ... and above it through grad_scale: skipped
    assert opt.skipped_steps() == 2


# ------------------------------------------------------------------ 4. checkpoints
@pytest.mark.parametrize("state_dtype", DTYPES)
def test_state_dict_round_trip_continues_bit_for_bit(state_dtype):
    flat, opt = _opt(state_dtype, skip_nonfinite=True)
    _take(flat, opt, _grad(flat, 1))
    g2 = _grad(flat, 2)
    g2[5] = float("inf")
    _take(flat, opt, g2)
    sd = copy.deepcopy({"flat": flat.state_dict(), "opt": opt.state_dict()})
    assert sd["opt"]["skipped"] == 1 and sd["opt"]["step"] == 2

    flat2, opt2 = _opt(state_dtype, skip_nonfinite=True)
    flat2.load_state_dict(sd["flat"])
    opt2.load_state_dict(sd["opt"])
    assert opt2.skipped_steps() == 1 and opt2.step_count == 2
    for f, o in ((flat, opt), (flat2, opt2)):
        _take(f, o, _grad(f, 3))
        _take(f, o, _grad(f, 4))
    assert _same(_state(flat), _state(flat2))
    assert opt2.state_dict() == opt.state_dict()


def test_unguarded_state_dict_has_no_skipped_key():
    flat, opt = _opt(skip_nonfinite=False)
    _take(flat, opt, _grad(flat, 1))
    assert set(opt.state_dict()) == {"step", "lr", "seed", "state_dtype"}
    # an absent key means 0
    flat2, opt2 = _opt(skip_nonfinite=True)
    opt2.load_state_dict(opt.state_dict())
    assert opt2.skipped_steps() == 0 and opt2.step_count == 1


# ------------------------------------------------------------------ 6. arguments
def test_argument_errors():
    from tf_operator_amd.train.llm import LlamaTrainer

    with pytest.raises(ValueError, match="device-step"):
        _opt(skip_nonfinite=True, device_step=True)
    with pytest.raises(ValueError, match="skip_grad_norm"):
        _opt(skip_nonfinite=True, skip_grad_norm=-1.0)
    with pytest.raises(ValueError, match="skip_grad_norm"):
        _opt(skip_nonfinite=True, skip_grad_norm=float("inf"))
    with pytest.raises(ValueError, match="skip_nonfinite"):
        _opt(skip_nonfinite=False, skip_grad_norm=2.0)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="skip_grad_norm"):
        LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32, skip_nonfinite=True, skip_grad_norm=-0.5)
    with pytest.raises(ValueError, match="skip_grad_norm"):
        LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32, skip_nonfinite=True, skip_grad_norm=float("nan"))
    with pytest.raises(ValueError, match="skip_nonfinite"):
        LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32, skip_nonfinite=False, skip_grad_norm=3.0)


def test_trainer_reads_the_environment(monkeypatch):
    from tf_operator_amd.train.llm import LlamaTrainer

    cpu = torch.device("cpu")
    tr = LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32)
    assert not tr.skip_nonfinite and not tr.opt.skip_nonfinite and tr.skipped_steps() == 0
    assert "skipped" not in tr.opt.state_dict()
    monkeypatch.setenv("TOA_SKIP_NONFINITE", "1")
    monkeypatch.setenv("TOA_SKIP_GRAD_NORM", "7.5")
    tr = LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32)
    assert tr.opt.skip_nonfinite and tr.opt.skip_grad_norm == 7.5 and tr.skipped_steps() == 0
    monkeypatch.setenv("TOA_SKIP_NONFINITE", "0")
    with pytest.raises(ValueError, match="skip_nonfinite"):   # a limit with the guard off
        LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32)
    monkeypatch.setenv("TOA_SKIP_NONFINITE", "yes")
    with pytest.raises(ValueError, match="TOA_SKIP_NONFINITE"):
        LlamaTrainer("llama-tiny", cpu, micro_batch=1, seq_len=32)


# ------------------------------------------------------------------ 5. gloo world 2, ZeRO-1
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _zero_arm(rank, pipelined):
    """Three ZeRO-1 steps of llama-tiny; during step 2 rank 1 alone computes
    on NaN activations, so its whole gradient is NaN."""
    from tf_operator_amd.train.llm import LlamaTrainer

    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=128, lr=1e-3, bucket_mb=0.25,
                      shard_optimizer=True, skip_nonfinite=True)
    assert tr.gather is not None and len(tr.bucketer.buckets) > 2 and tr.opt.owned is not None
    tr.pipeline_tail = pipelined
    b = tr.synthetic_batch()
    f = tr.flat

    def snap():
        tr.gather.wait_all()
        return [f.param.detach().clone(), f.master.clone(), f.exp_avg.clone(), f.exp_avg_sq.clone()]

    losses = [float(tr.step([b]))]
    after1 = snap()
    hook = tr.model.embed.register_forward_hook(lambda mod, args, out: out * float("nan")) if rank == 1 else None
    losses.append(float(tr.step([b])))
    if hook is not None:
        hook.remove()
    after2 = snap()
    skipped2 = tr.skipped_steps()
    losses.append(float(tr.step([b])))
    after3 = snap()
    return {"losses": losses, "after1": after1, "after2": after2, "after3": after3, "skipped2": skipped2,
            "skipped3": tr.skipped_steps(), "step_idx": tr.step_idx, "sd": tr.opt.state_dict()}


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save({"pipelined": _zero_arm(rank, True), "whole": _zero_arm(rank, False)}, f"{out}.{rank}")
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def zero_runs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("skip_step") / "res")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]


@pytest.mark.parametrize("arm", ["pipelined", "whole"])
def test_zero1_every_rank_skips_when_one_rank_has_nan(zero_runs, arm):
    r0, r1 = (r[arm] for r in zero_runs)
    # the NaN was rank 1's alone: rank 0's own loss of that step is a number
    assert r0["losses"][1] == r0["losses"][1] and r1["losses"][1] != r1["losses"][1]
    for r in (r0, r1):
        assert r["skipped2"] == 1 and r["skipped3"] == 1 and r["step_idx"] == 3
        assert r["sd"]["skipped"] == 1 and r["sd"]["step"] == 3
        assert _same(r["after2"], r["after1"])                # weights and this rank's shards: untouched
        assert bool(torch.isfinite(r["after2"][0].float()).all())
        assert not _same(r["after3"][:1], r["after2"][:1])    # step 3 is taken
        assert r["losses"][2] == r["losses"][2]
        assert all(bool(torch.isfinite(t.float()).all()) for t in r["after3"])
    # the gathered weights agree between the ranks at every point
    for k in ("after1", "after2", "after3"):
        assert _same(r0[k][:1], r1[k][:1]), k
