"""Skipped steps on the MI355X (csrc/hip/optim.hip): the verdict kernel
toa_adamw_guard and the GUARD arms of the flat and W^T-writing AdamW kernels
(toa_adamw_flat[_bf16s]_guard, toa_adamw_wt[_bf16s]_guard), and the trainer
with skip_nonfinite through the real kernels and the real norm path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HIP_INVALID = 1   # hipErrorInvalidValue
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)
SEED = 0x5EED1234
PAD = 64          # sentinel elements behind every buffer: a write past the slice would show


def _L():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def _inputs(n, bf, grad_dtype=torch.bfloat16, seed=5):
    """(master, param, grad, m, v) of n + PAD elements; bf: bf16 moments."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = n + PAD
    master = torch.randn(k, device=DEV, generator=g)
    grad = torch.randn(k, device=DEV, generator=g).to(grad_dtype)
    mdt = torch.bfloat16 if bf else torch.float32
    m = (torch.randn(k, device=DEV, generator=g) * 0.01).to(mdt)
    v = (torch.rand(k, device=DEV, generator=g) * 0.01).to(mdt)
    return [master, master.to(torch.bfloat16), grad, m, v]


def _words(flag, skipped):
    return (torch.tensor([flag], device=DEV, dtype=torch.int32),
            torch.tensor([skipped], device=DEV, dtype=torch.int32))


def _flat(L, t, n, *, bf, step, zero=False, guard=None, nsq=None, max_norm=0.0, grad_scale=1.0, base=0, hp=HP,
          param=True):
    """toa_adamw_flat[_bf16s][_guard] over the first n elements of t; guard: (flag, skipped) tensors or
    ctypes pointers / None."""
    master, p, grad, m, v = t
    name = "toa_adamw_flat" + ("_bf16s" if bf else "") + ("_guard" if guard is not None else "")
    args = [L.ptr(master), L.ptr(p) if param else None, L.ptr(grad),
            int(grad.dtype == torch.bfloat16) | (2 if zero else 0), L.ptr(m), L.ptr(v), n, hp["lr"], hp["beta1"],
            hp["beta2"], hp["eps"], hp["weight_decay"], step, grad_scale, L.ptr(nsq), max_norm]
    if bf:
        args += [base, SEED]
    if guard is not None:
        args += [x if not isinstance(x, torch.Tensor) else L.ptr(x) for x in guard]
    return L.call_ret(name, *args, L.stream(master))


def _wt(L, t, wt, R, C, *, bf, step, zero=False, guard=None, nsq=None, max_norm=0.0, grad_scale=1.0, base=0, hp=HP):
    master, p, grad, m, v = t
    name = "toa_adamw_wt" + ("_bf16s" if bf else "") + ("_guard" if guard is not None else "")
    args = [L.ptr(master), L.ptr(p), L.ptr(grad), int(zero), L.ptr(m), L.ptr(v), L.ptr(wt), wt.stride(0), R, C,
            hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], step, grad_scale, L.ptr(nsq), max_norm]
    if bf:
        args += [base, SEED]
    if guard is not None:
        args += [x if not isinstance(x, torch.Tensor) else L.ptr(x) for x in guard]
    return L.call_ret(name, *args, L.stream(master))


def _bytes_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _wt_pattern(R, C):
    """A W^T buffer [C][R + 8] (row stride beyond R) that no update would write."""
    buf = (torch.arange(C * (R + 8), device=DEV) % 251).to(torch.bfloat16).view(C, R + 8)
    return buf, buf[:, :R]


# ------------------------------------------------------------------ 1. flat kernels, flag = 1
@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("n", [4096, 4096 + 8])
def test_flat_skipped_step_touches_nothing(n, bf, grad_dtype, zero):
    """flag = 1: master, param, m and v byte-equal; the gradient slice zeroed
    iff zero_grad, and not an element behind it.  n = 4096 + 8: the last
    workgroup is partial."""
    L = _L()
    t = _inputs(n, bf, grad_dtype)
    before = [x.clone() for x in t]
    nsq = torch.tensor([float("inf")], device=DEV)
    assert _flat(L, t, n, bf=bf, step=2, zero=zero, guard=_words(1, 1), nsq=nsq, max_norm=1.0, base=64) == 0
    torch.cuda.synchronize()
    for i in (0, 1, 3, 4):
        assert _bytes_equal(t[i], before[i]), i
    if zero:
        assert not bool(t[2][:n].any()) and _bytes_equal(t[2][n:], before[2][n:])
    else:
        assert _bytes_equal(t[2], before[2])


# ------------------------------------------------------------------ 2. W^T kernels, flag = 1
@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("R,C", [(128, 128), (256, 128)])
def test_wt_skipped_step_touches_nothing(R, C, bf, zero):
    L = _L()
    n = R * C
    t = _inputs(n, bf)
    before = [x.clone() for x in t]
    buf, wt = _wt_pattern(R, C)
    buf0 = buf.clone()
    nsq = torch.tensor([float("nan")], device=DEV)
    assert _wt(L, t, wt, R, C, bf=bf, step=2, zero=zero, guard=_words(1, 1), nsq=nsq, max_norm=1.0, base=64) == 0
    torch.cuda.synchronize()
    assert _bytes_equal(buf, buf0)
    for i in (0, 1, 3, 4):
        assert _bytes_equal(t[i], before[i]), i
    if zero:
        assert not bool(t[2][:n].any()) and _bytes_equal(t[2][n:], before[2][n:])
    else:
        assert _bytes_equal(t[2], before[2])


# ------------------------------------------------------------------ 3. flag = 0, skipped = 0: the unguarded bits
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("n", [4096, 4096 + 8])
def test_flat_guard_that_never_skips_is_bit_identical(n, bf):
    L = _L()
    from tf_operator_amd.ops.optim import grad_norm_sq

    a, b = _inputs(n, bf), _inputs(n, bf)
    nsq = grad_norm_sq(a[2][:n])
    words = _words(0, 0)
    for step in (1, 2, 3):
        assert _flat(L, a, n, bf=bf, step=step, nsq=nsq, max_norm=1.0, grad_scale=0.5, base=64) == 0
        assert _flat(L, b, n, bf=bf, step=step, nsq=nsq, max_norm=1.0, grad_scale=0.5, base=64, guard=words) == 0
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert _bytes_equal(x, y)
    assert not _bytes_equal(a[0], _inputs(n, bf)[0])
    assert words[0].item() == 0 and words[1].item() == 0


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("R,C", [(128, 128), (256, 128)])
def test_wt_guard_that_never_skips_is_bit_identical(R, C, bf):
    L = _L()
    from tf_operator_amd.ops.optim import grad_norm_sq

    n = R * C
    a, b = _inputs(n, bf), _inputs(n, bf)
    (abuf, awt), (bbuf, bwt) = _wt_pattern(R, C), _wt_pattern(R, C)
    nsq = grad_norm_sq(a[2][:n])
    words = _words(0, 0)
    for step in (1, 2, 3):
        assert _wt(L, a, awt, R, C, bf=bf, step=step, nsq=nsq, max_norm=1.0, grad_scale=0.5, base=64) == 0
        assert _wt(L, b, bwt, R, C, bf=bf, step=step, nsq=nsq, max_norm=1.0, grad_scale=0.5, base=64,
                   guard=words) == 0
    torch.cuda.synchronize()
    for x, y in zip(a + [abuf], b + [bbuf]):
        assert _bytes_equal(x, y)
    assert torch.equal(bwt, b[1][:n].view(R, C).t())


# ------------------------------------------------------------------ 4. skipped = 1: the step before
# the inputs of tests/test_ops_gpu.py test_adamw_device_step_matches_host_step
DS_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def _ds_inputs(n, bf, grad_dtype):
    torch.manual_seed(3)
    master = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV).to(grad_dtype)
    mdt = torch.bfloat16 if bf else torch.float32
    return [master, master.to(torch.bfloat16), g, torch.zeros(n, device=DEV, dtype=mdt),
            torch.zeros(n, device=DEV, dtype=mdt)]


@pytest.mark.parametrize("bf", [False, True])
def test_flat_one_skipped_step_shifts_the_step(bf):
    """Guarded at host step k + 1 with skipped = 1 against unguarded at step
    k, 5 steps: m and v bit for bit (bf16 moments: the rounding key is that
    of step k), master within 1e-6 (bias corrections by powf on the device
    against the host's)."""
    L = _L()
    n = 4096
    a, b = _ds_inputs(n, bf, torch.float32), _ds_inputs(n, bf, torch.float32)
    words = _words(0, 1)
    for k in range(1, 6):
        assert _flat(L, a, n, bf=bf, step=k, hp=DS_HP, param=bf) == 0
        assert _flat(L, b, n, bf=bf, step=k + 1, hp=DS_HP, param=bf, guard=words) == 0
    torch.cuda.synchronize()
    assert _bytes_equal(a[3], b[3]) and _bytes_equal(a[4], b[4])
    assert float(a[3].float().abs().max()) > 0
    err = float((a[0] - b[0]).abs().max())
    print(f"master: max abs difference {err:.3e}")
    assert err < 1e-6
    if bf:   # ... and the key matters: the same update keyed by step k + 1 rounds differently
        c = _ds_inputs(n, bf, torch.float32)
        assert _flat(L, c, n, bf=bf, step=2, hp=DS_HP, guard=_words(0, 0)) == 0
        d = _ds_inputs(n, bf, torch.float32)
        assert _flat(L, d, n, bf=bf, step=2, hp=DS_HP, guard=_words(0, 1)) == 0
        torch.cuda.synchronize()
        assert not _bytes_equal(c[4], d[4])


@pytest.mark.parametrize("bf", [False, True])
def test_wt_one_skipped_step_shifts_the_step(bf):
    L = _L()
    R = C = 128
    n = R * C
    a, b = _ds_inputs(n, bf, torch.bfloat16), _ds_inputs(n, bf, torch.bfloat16)
    (_, awt), (_, bwt) = _wt_pattern(R, C), _wt_pattern(R, C)
    words = _words(0, 1)
    for k in range(1, 6):
        assert _wt(L, a, awt, R, C, bf=bf, step=k, hp=DS_HP) == 0
        assert _wt(L, b, bwt, R, C, bf=bf, step=k + 1, hp=DS_HP, guard=words) == 0
    torch.cuda.synchronize()
    assert _bytes_equal(a[3], b[3]) and _bytes_equal(a[4], b[4])
    err = float((a[0] - b[0]).abs().max())
    print(f"master: max abs difference {err:.3e}")
    assert err < 1e-6
    assert torch.equal(bwt, b[1].view(R, C).t())


# ------------------------------------------------------------------ 5. the verdict kernel
def test_guard_verdict_and_running_count():
    L = _L()
    inf, nan = float("inf"), float("nan")
    #        norm_sq grad_scale limit  flag
    cases = [(1.0, 1.0, 0.0, 0),
             (inf, 1.0, 0.0, 1),
             (nan, 1.0, 0.0, 1),
             (4.0, 1.0, 1.9, 1),      # norm 2 above the limit
             (4.0, 1.0, 2.1, 0),      # ... and below it
             (4.0, 0.5, 1.1, 0),      # the limit is on norm x grad_scale = 1
             (4.0, 0.5, 0.9, 1),
             (4.0, 2.0, 3.9, 1),
             (inf, 1.0, 5.0, 1),
             (nan, 1.0, 5.0, 1),
             (0.0, 1.0, 5.0, 0),
             (1e30, 1.0, 0.0, 0)]     # huge and finite, no limit: applied
    flag, skipped = _words(7, 0)       # a stale flag is overwritten
    nsq = torch.zeros(1, device=DEV)
    total = 0
    for ns, gs, limit, want in cases:
        nsq.fill_(ns)
        assert L.call_ret("toa_adamw_guard", L.ptr(nsq), gs, limit, L.ptr(flag), L.ptr(skipped), L.stream(nsq)) == 0
        total += want
        assert (int(flag.item()), int(skipped.item())) == (want, total), (ns, gs, limit)
    assert total == 7


def test_null_pointers_are_refused_without_a_launch():
    L = _L()
    nsq = torch.ones(1, device=DEV)
    flag, skipped = _words(0, 3)
    s = L.stream(nsq)
    assert L.call_ret("toa_adamw_guard", None, 1.0, 0.0, L.ptr(flag), L.ptr(skipped), s) == HIP_INVALID
    assert L.call_ret("toa_adamw_guard", L.ptr(nsq), 1.0, 0.0, None, L.ptr(skipped), s) == HIP_INVALID
    assert L.call_ret("toa_adamw_guard", L.ptr(nsq), 1.0, 0.0, L.ptr(flag), None, s) == HIP_INVALID
    R = C = 128
    n = R * C
    for bf in (False, True):
        t = _inputs(n, bf)
        before = [x.clone() for x in t]
        buf, wt = _wt_pattern(R, C)
        buf0 = buf.clone()
        for guard in ((None, skipped), (flag, None)):
            assert _flat(L, t, n, bf=bf, step=1, guard=guard) == HIP_INVALID
            assert _wt(L, t, wt, R, C, bf=bf, step=1, guard=guard) == HIP_INVALID
        torch.cuda.synchronize()
        for x, y in zip(t + [buf], before + [buf0]):
            assert _bytes_equal(x, y)
    assert int(flag.item()) == 0 and int(skipped.item()) == 3


# ------------------------------------------------------------------ 6. the trainer
def _train3(adam_state, guard, seq_len=256):
    """Three steps of llama-tiny128 at world 1; step 2 computes on NaN
    activations (the embedding's output times NaN), so the non-finite values
    reach the update through the real kernels and the real norm."""
    from tf_operator_amd.train.llm import LlamaTrainer

    tr = LlamaTrainer("llama-tiny128", torch.device(DEV), micro_batch=2, seq_len=seq_len, seed=0,
                      adam_state=adam_state, skip_nonfinite=guard)
    assert tr.opt.skip_nonfinite == guard
    assert tr.opt.sumsq is not None                                   # the fused clipping norm stays on
    assert tr.wt is not None and len(tr.opt._fused_items()) == 2 * 4 + 1   # ... and the W^T-writing update
    f = tr.flat
    b = tr.synthetic_batch()

    def snap():
        torch.cuda.synchronize()
        return ([f.master.clone(), f.param.detach().clone(), f.exp_avg.clone(), f.exp_avg_sq.clone()]
                + [view.clone() for _, _, _, view in tr.wt.items])

    losses = [float(tr.step([b]))]
    after1 = snap()
    hook = tr.model.embed.register_forward_hook(lambda mod, args, out: out * float("nan"))
    losses.append(float(tr.step([b])))
    hook.remove()
    after2 = snap()
    skipped2 = tr.skipped_steps()
    losses.append(float(tr.step([b])))
    after3 = snap()
    return tr, losses, after1, after2, after3, skipped2


@pytest.mark.parametrize("adam_state,seq_len", [("fp32", 256), ("bf16", 256), ("fp32", 512)])
def test_trainer_skips_the_nan_step_and_trains_on(adam_state, seq_len):
    """2 x 512 tokens: the token count from which the weight-gradient
    kernels' partials are the clipping norm, so the NaN reaches the verdict
    through them (toa_sum_f32) and not through the pass over the gradient."""
    _L()
    tr, losses, after1, after2, after3, skipped2 = _train3(adam_state, True, seq_len)
    if seq_len == 512:
        assert tr.opt.sumsq.hits == 3, "a step fell back to the full pass"
    assert tr.flat.exp_avg.dtype == (torch.bfloat16 if adam_state == "bf16" else torch.float32)
    assert losses[1] != losses[1]                         # the bad step's loss is still returned
    for i, (x, y) in enumerate(zip(after2, after1)):
        assert _bytes_equal(x, y), i                      # master, weights, m, v and every W^T view
    assert skipped2 == 1 and tr.skipped_steps() == 1 and tr.step_idx == 3
    assert tr.opt.state_dict()["skipped"] == 1
    assert losses[2] == losses[2] and losses[2] < losses[0]
    assert all(bool(torch.isfinite(x.float()).all()) for x in after3)
    assert not _bytes_equal(after3[0], after2[0])         # step 3 is applied
    for _, _, p, view in tr.wt.items:
        assert torch.equal(view, p.data.t())

    # the control: the same three steps without the guard destroy the master weights
    tr0, losses0, _, _, ctl3, _ = _train3(adam_state, False, seq_len)
    assert losses0[0] == losses[0]
    assert not bool(torch.isfinite(ctl3[0]).all())
    assert tr0.skipped_steps() == 0 and "skipped" not in tr0.opt.state_dict()
