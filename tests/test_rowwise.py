"""The per-row checker of the row kernels (tests/rowwise_numerics.py) on the
CPU: the model the tolerance rests on is a sane one at every shape of the GPU
tests, the explicit fp64 reference agrees with torch autograd in fp64, and
planted errors that the whole-tensor measure of tests/test_ops_gpu.py accepts
are rejected."""
import functools

import pytest
import torch
import torch.nn.functional as F

import rowwise_numerics as rn
from rowwise_numerics import BF16, FP32
from tf_operator_amd.ops import llm

DTS = [BF16, FP32]
_dt = lambda d: "bf16" if d == BF16 else "fp32"


def _model_is_sane(name, model, ref, mag, n, dtype):
    """The rule is 3 x the model's own row error: the model must be within 2
    units per row, and within the limit the rule makes of it."""
    e = rn.row_err(model, ref, mag)[0]
    print(f"model {name}: {e / rn.unit(dtype):.3f} u")
    assert e <= 2 * rn.unit(dtype), (name, e / rn.unit(dtype))
    assert e <= rn.row_tol(e, n, dtype, name)


# ---------------------------------------------------------------------------
# the model at the GPU tests' shapes
# ---------------------------------------------------------------------------
_NORM_CASES = [(rows, cols, dtype, rms, res) for rows, cols in rn.NORM_WAVE_TALL + rn.NORM_WAVE_SHORT
               for dtype in DTS for rms in (True, False) for res in (False, True)] + \
              [(rows, cols, BF16, True, res) for rows, cols in rn.NORM_ROW for res in (False, True)]


@pytest.mark.parametrize("rows,cols,dtype,rms,res", _NORM_CASES,
                         ids=lambda x: _dt(x) if isinstance(x, torch.dtype) else str(x))
def test_norm_model(rows, cols, dtype, rms, res):
    case = rn.NormCase(rows, cols, dtype, rms, res)
    for name in case.names:
        n, dt = case.n_dtype(name)
        _model_is_sane(name, getattr(case.model, name), getattr(case.ref, name),
                       getattr(case.ref, rn.NORM_OUT[name]), n, dt)


@pytest.mark.parametrize("rep", ["gqa", 1])
@pytest.mark.parametrize("shape", rn.ROPE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rope_model(shape, rep):
    B, S, Hq, Hkv, D = shape
    rep = Hq // Hkv if rep == "gqa" else 1
    cos, sin = llm.rope_tables(S, D)
    ref = rn.rope_ref64(*rn.rope_inputs(*shape, rep), cos, sin, *shape, rep)
    for name in ("q", "k", "v", "dqkv"):
        r = getattr(ref, name)
        _model_is_sane(name, rn.rnd(r, BF16), r, getattr(ref, "mag_" + name), rep + 2, BF16)


@pytest.mark.parametrize("T,Fd", rn.SWIGLU_SHAPES)
def test_swiglu_model(T, Fd):
    gu, d = rn.swiglu_inputs(T, Fd)
    assert all(bool((gu[:, :Fd] == s).any()) for s in rn.SWIGLU_SPECIAL)
    ref = rn.swiglu_ref64(gu, d)
    g = gu[:, :Fd].double()
    # where exp(-g) saturates or overflows, silu is g or 0 in the output's precision
    assert bool((rn.rnd(F.silu(g[g >= 20]), BF16) == g[g >= 20]).all())
    assert bool((F.silu(g[g <= -20]).abs() < 1e-7).all())
    for name in ("out", "du", "dg"):
        r = getattr(ref, name)
        assert bool(torch.isfinite(r).all())
        _model_is_sane(name, rn.rnd(r, BF16), r, getattr(ref, "mag_" + name), 2, BF16)


@pytest.mark.parametrize("dtype", DTS, ids=_dt)
@pytest.mark.parametrize("V", rn.XENT_V)
def test_xent_model(V, dtype):
    x, t = rn.xent_inputs(V, dtype)
    ref = rn.xent_ref64(x, t, 0.37)
    model = rn.rnd(ref.grad, dtype)
    for part, (m, r, a) in zip(("softmax", "target"), zip(*(rn.xent_split(z, ref) for z in (model, ref.grad,
                                                                                          ref.mag_grad)))):
        _model_is_sane(part, m, r, a, V, dtype)
    for name in ("lse", "loss"):
        r = getattr(ref, name)
        _model_is_sane(name, rn.rnd(r, FP32), r, getattr(ref, "mag_" + name), V, FP32)
    assert rn.xent_grad_ok(model, ref, dtype) == (True, True)


def test_xent_loop_arithmetic():
    """V = 8200 is 1025 chunks of 8: with 512 threads and unroll 2 every thread
    makes exactly one full round and chunk 1024 is left to the remainder loop;
    8203 is no multiple of 8 (the scalar path)."""
    nb, unroll = rn.XENT_BLOCK, 2
    v8 = 8200 // 8
    assert 8200 % 8 == 0 and v8 == 1025
    rounds = [len(range(i, v8 - (unroll - 1) * nb, unroll * nb)) for i in range(nb)]
    assert rounds == [1] * nb
    left = [c for i in range(nb) for c in range(i + unroll * nb * rounds[i], v8, nb)]
    assert left == [1024]
    assert rn.xent_inputs(8200, BF16)[1][2] // 8 == 1024
    assert 8203 % 8 != 0


@pytest.mark.parametrize("gdtype", DTS, ids=_dt)
@pytest.mark.parametrize("dim", rn.EMBED_DIMS)
@pytest.mark.parametrize("kind", ["one", "run", "distinct"])
def test_embed_model(kind, dim, gdtype):
    base, idx, dy = rn.embed_inputs(kind, dim, gdtype)
    ref = rn.embed_ref64(base, idx, dy)
    srt = torch.sort(idx).values
    if kind == "run":
        assert int((srt == srt[-1]).sum()) == 5 and int(idx[-1]) == int(srt[-1])
    if kind == "distinct":
        assert ref.n == 2
    _model_is_sane("grad", ref.model, ref.grad, ref.mag, ref.n, gdtype)


# ---------------------------------------------------------------------------
# the reference against torch autograd in fp64
# ---------------------------------------------------------------------------
def _close(a, b, what):
    d = float((a.double() - b.double()).abs().max())
    assert d <= 1e-10 * max(1.0, float(b.abs().max())), (what, d)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
def test_norm_reference_is_autograd(rms, res):
    rows, cols, eps = 37, 520, 1e-5
    i = rn.norm_inputs(rows, cols, BF16)
    x, r, w, b = (t.double().requires_grad_() for t in (i.x, i.r, i.w, i.b))
    h = x + r if res else x
    if rms:
        y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w
    else:
        y = F.layer_norm(h, (cols,), w, b, eps)
    outs, grads = ([h, y], [i.dh.double(), i.dy.double()]) if res else ([y], [i.dy.double()])
    torch.autograd.backward(outs, grads)
    ref = rn.norm_ref64(i.x, i.r if res else None, i.w, None if rms else i.b, i.dy, i.dh if res else None, eps, rms)
    _close(ref.y, y.detach(), "y")
    _close(ref.dx, x.grad, "dx")
    _close(ref.dw[:, 0], w.grad, "dw")
    if not rms:
        _close(ref.db[:, 0], b.grad, "db")
        _close(ref.mean[:, 0], h.detach().mean(-1), "mean")
    if res:
        _close(ref.dx, r.grad, "dr")
    assert bool((ref.mag_dx >= ref.dx.abs() * (1 - 1e-12)).all()) and bool((ref.mag_y >= ref.y.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("rep", [2, 1])
def test_rope_reference_is_autograd(rep):
    B, S, Hq, Hkv, D = 2, 5, 4, 2, 16
    cos, sin = llm.rope_tables(S, D)
    qkv, dq, dk, dv = rn.rope_inputs(B, S, Hq, Hkv, D, rep)
    ref = rn.rope_ref64(qkv, dq, dk, dv, cos, sin, B, S, Hq, Hkv, D, rep)
    # the project's own CPU path (fp32 inside) agrees to fp32 rounding, and its autograd gives the backward
    xin = qkv.double().requires_grad_()
    x = xin.view(B, S, Hq + 2 * Hkv, D).transpose(1, 2)
    d2 = D // 2
    c, s = cos.double(), sin.double()
    rot = lambda t: torch.cat([t[..., :d2] * c - t[..., d2:] * s, t[..., d2:] * c + t[..., :d2] * s], -1)
    q, k = rot(x[:, :Hq]), rot(x[:, Hq:Hq + Hkv]).repeat_interleave(rep, 1)
    v = x[:, Hq + Hkv:].repeat_interleave(rep, 1)
    for name, t in (("q", q), ("k", k), ("v", v)):
        _close(getattr(ref, name), t.detach(), name)
    torch.autograd.backward([q, k, v], [dq.double(), dk.double(), dv.double()])
    _close(ref.dqkv.transpose(1, 2).reshape(B * S, -1), xin.grad, "dqkv")
    q32, k32, v32 = llm.rope_qkv(qkv.float(), cos, sin, B, S, Hq, Hkv, D, rep)
    assert float((q32.double() - ref.q).abs().max()) < 1e-5 and float((k32.double() - ref.k).abs().max()) < 1e-5


def test_swiglu_reference_is_autograd():
    gu, d = rn.swiglu_inputs(64, 8)
    ref = rn.swiglu_ref64(gu, d)
    g = gu.double().requires_grad_()
    out = F.silu(g[:, :8]) * g[:, 8:]
    out.backward(d.double())
    _close(ref.out, out.detach(), "out")
    _close(torch.cat([ref.dg, ref.du], -1), g.grad, "dgu")


@pytest.mark.parametrize("V", [10, 8203])
def test_xent_reference_is_autograd(V):
    x, t = rn.xent_inputs(V, BF16)
    ref = rn.xent_ref64(x, t, 0.37)
    xr = x.double().requires_grad_()
    per_row = F.cross_entropy(xr, t, ignore_index=-100, reduction="none")
    _close(ref.loss[:, 0], per_row.detach(), "loss")
    (0.37 * F.cross_entropy(xr, t, ignore_index=-100)).backward()
    _close(ref.grad, xr.grad, "grad")
    soft, tgt = rn.xent_split(ref.grad, ref)
    _close(soft + torch.zeros_like(soft).scatter_(1, ref.tc, tgt), ref.grad, "split")
    # masked columns: the reference stays finite
    xm = x.clone()
    xm[:, V // 2:] = float("-inf")
    refm = rn.xent_ref64(xm, t.clamp(max=V // 2 - 1), 1.0)
    assert bool(torch.isfinite(refm.loss).all()) and bool(torch.isfinite(refm.grad).all())
    _close(refm.loss[:, 0], F.cross_entropy(xm.double(), t.clamp(max=V // 2 - 1), reduction="none"), "masked loss")


def test_embed_reference_is_autograd():
    base, idx, dy = rn.embed_inputs("run", 16, FP32)
    w = base.double().requires_grad_()
    F.embedding(idx, w).backward(dy.double())
    _close(rn.embed_ref64(base, idx, dy).grad, base.double() + w.grad, "grad")


# ---------------------------------------------------------------------------
# planted errors: rejected per row, accepted by the whole-tensor measure
# ---------------------------------------------------------------------------
OLD_TOL = 1e-2   # the whole-tensor limit of test_rmsnorm_fwd_bwd / test_cross_entropy / test_swiglu


@functools.lru_cache(maxsize=None)
def _norm_case():
    return rn.NormCase(777, 4104, BF16, True, False)


def _rejected_but_old_accepts(what, new_ok, bad, ref):
    old = rn.rel(bad, ref)
    print(f"{what}: whole-tensor rel {old:.2e} (limit {OLD_TOL})")
    assert not new_ok, f"{what}: the per-row check accepted the planted error"
    assert old < OLD_TOL, f"{what}: the whole-tensor measure was meant to accept this ({old:.2e})"


def test_planted_rstd_off_by_5_percent():
    """One row of 777 normalised with an rstd 5 % too large: 0.05 / sqrt(777) of the whole tensor."""
    case = _norm_case()
    assert case.ok("y", case.model.y) and case.ok("rstd", case.model.rstd)
    y, rstd = case.model.y.clone(), case.model.rstd.clone()
    y[401] = rn.rnd(y[401] * 1.05, BF16)
    rstd[401] *= 1.05
    with pytest.raises(AssertionError):
        case.check("y", y, "planted")
    _rejected_but_old_accepts("rstd x 1.05: y", case.ok("y", y), y, case.ref.y)
    _rejected_but_old_accepts("rstd x 1.05: rstd", case.ok("rstd", rstd), rstd, case.ref.rstd)


def test_planted_row_tail_zeroed():
    """The last 8 of 4104 columns of one row left zero (a tail chunk not written), in y and in dx."""
    case = _norm_case()
    for name in ("y", "dx"):
        assert case.ok(name, getattr(case.model, name))
        bad = getattr(case.model, name).clone()
        bad[776, -8:] = 0
        _rejected_but_old_accepts(f"tail of {name}", case.ok(name, bad), bad, getattr(case.ref, name))


def test_planted_softmax_part_zeroed():
    """The softmax part of one row of 65 zero over 4096 columns, the target
    entry intact: the one-hot entries carry the whole-tensor norm."""
    V = 8200
    x, t = rn.xent_inputs(V, BF16, rows=65)
    ref = rn.xent_ref64(x, t)
    good = rn.rnd(ref.grad, BF16)
    assert rn.xent_grad_ok(good, ref, BF16) == (True, True)
    bad = good.clone()
    row, tcol = 9, int(t[9])
    keep = bad[row, tcol].clone()
    lo = 0 if tcol >= 4096 + 2048 or tcol < 2048 else 4096   # an aligned block of 4096 columns
    bad[row, lo:lo + 4096] = 0
    bad[row, tcol] = keep
    soft_ok, tgt_ok = rn.xent_grad_ok(bad, ref, BF16)
    assert tgt_ok
    with pytest.raises(AssertionError):
        rn.xent_check_grad("planted", bad, ref, BF16)
    _rejected_but_old_accepts("softmax part zeroed", soft_ok, bad, ref.grad)


@pytest.mark.parametrize("dtype", DTS, ids=_dt)
@pytest.mark.parametrize("V,drop", [(8200, 8), (8203, 3)])
def test_planted_lse_misses_its_tail(V, drop, dtype):
    """lse (and with it the loss) summed without the last chunk of 8 columns
    (V = 8200: the remainder loop's chunk) or without the 3 columns after the
    last whole chunk (V = 8203): 2e-3 and 4e-5 absolute, which a mean loss to
    1e-3 accepts, and in a bf16 gradient invisible.  The per-row lse and loss
    checks must reject both."""
    x, t = rn.xent_inputs(V, dtype)
    t[1] = 5                                    # no target in the dropped columns
    ref = rn.xent_ref64(x, t)
    short = torch.logsumexp(x.double()[:, :V - drop], -1, keepdim=True)
    for name, good, bad in (("lse", ref.lse, short), ("loss", ref.loss, ref.loss - (ref.lse - short) * ref.valid[:, None])):
        mag, model = getattr(ref, "mag_" + name), rn.rnd(good, FP32)
        assert rn.rows_ok(name, model, good, mag, model, V, FP32)
        bad = rn.rnd(bad, FP32)
        e = rn.row_err(bad, good, mag)[0]
        print(f"{name} without the last {drop} of {V} columns: {e / rn.U32:.1f} units (limit {rn.row_tol(0.5 * rn.U32, V, FP32, name) / rn.U32:.1f})")
        assert not rn.rows_ok(name, bad, good, mag, model, V, FP32), f"{name}: accepted"
        with pytest.raises(AssertionError):
            rn.check_rows("planted", name, bad, good, mag, model, V, FP32)
    assert abs(float(ref.loss.sum() - (ref.loss - (ref.lse - short) * ref.valid[:, None]).sum())) / 5 < 1e-3


def test_planted_embedding_second_pass_missing():
    """One vocabulary row's columns 2048.. (the second pass of 256 x 8 columns) left un-added."""
    base, idx, dy = rn.embed_inputs("run", 2056, BF16)
    ref = rn.embed_ref64(base, idx, dy)
    assert rn.rows_ok("grad", ref.model, ref.grad, ref.mag, ref.model, ref.n, BF16)
    bad = ref.model.clone()
    tok = int(idx[0])
    bad[tok, 2048:] = base.double()[tok, 2048:]
    ok = rn.rows_ok("grad", bad, ref.grad, ref.mag, ref.model, ref.n, BF16)
    _rejected_but_old_accepts("embedding columns 2048..", ok, bad, ref.grad)


def test_ignored_row_must_be_exactly_zero():
    x, t = rn.xent_inputs(10, FP32)
    ref = rn.xent_ref64(x, t)
    bad = ref.grad.clone()
    bad[3, 4] = 1e-30
    with pytest.raises(AssertionError, match="ignored"):
        rn.xent_check_grad("planted", bad, ref, FP32)
