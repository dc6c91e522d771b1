"""The attention kernels row by row (tests/attn_numerics.py): every row of
O, dQ, dK, dV within min(3 x the bf16 model's own error, 8 u) of the fp64
reference, relative to the magnitude of what was summed into the row; lse per
row; and causality bit for bit -- nothing at a key position > i changes row i,
nothing at a query position < j changes key row j.  Every kernel form: the
register-staged HIP forward and the split backward (ragged S), the LDS-DMA and
assembly forwards, the dS-through-HBM backward with the HIP and the assembly
dK/dV kernel, the fused RoPE backward, the document-mask pair.

Outputs are pre-filled with NaN and the workspace with 0xFF, so an unwritten
row fails.  The largest ratios seen on an MI355X are in docs/kernels.md
("Per-row attention tolerances").

With them, per element: cross entropy's loss / lse / gradient rows and its
unroll switch, and SwiGLU past the 4096-workgroup grid cap."""
import contextlib
import functools
import math

import pytest
import torch

import attn_numerics as an
from attn_numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def _id(shape):
    return "-".join(str(int(x)) if isinstance(x, bool) else str(x) for x in shape)


@contextlib.contextmanager
def _forms(L, fwd=-1, bwd=-1, dkdv=-1):
    """Pin the forward / backward / dK-dV kernel forms; back to the defaults on the way out."""
    try:
        L.call("toa_attn_set_fwd_variant", fwd)
        L.call("toa_attn_set_bwd_variant", bwd)
        L.call("toa_attn_set_dkdv_variant", dkdv)
        yield
    finally:
        L.call("toa_attn_set_fwd_variant", -1)
        L.call("toa_attn_set_bwd_variant", -1)
        L.call("toa_attn_set_dkdv_variant", -1)


@functools.lru_cache(maxsize=None)
def _case(shape, doc=False):
    """Inputs on the GPU, fp64 reference, model and tolerances of one shape:
    computed once, read-only for every test that uses the shape."""
    q, k, v, do = an.make_inputs(*shape, device=DEV)
    if doc:
        from tf_operator_amd.ops import llm

        S = shape[3]
        assert shape[0] == 2
        doc = llm.doc_bounds_from_lengths([an.doc_lengths(S), an.doc_lengths(S, (64, 256))], S, device=DEV)
    return an.Case(q, k, v, do, doc=doc or None)


def _bhsd(t, bshd):
    return t.transpose(1, 2) if bshd else t


def _fwd(L, q, k, v, bshd, doc=None):
    """(O in the kernel's layout, lse) of toa_attn_fwd / toa_attn_fwd_doc into NaN-filled outputs."""
    B, H, S, D = q.shape
    Hk = k.shape[1]
    P = L.ptr
    o = torch.full((B, S, H, D) if bshd else (B, H, S, D), NAN, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, S), NAN, device=DEV, dtype=torch.float32)
    flags = 1 | (2 if bshd else 0)
    scale = 1.0 / math.sqrt(D)
    if doc is None:
        L.call("toa_attn_fwd", P(q), P(k), P(v), P(o), P(lse), B, H, Hk, S, D, flags, scale, L.stream(q))
    else:
        L.call("toa_attn_fwd_doc", P(q), P(k), P(v), P(o), P(lse), P(doc[0]), B, H, Hk, S, D, flags, scale,
               L.stream(q))
    torch.cuda.synchronize()
    return o, lse


def _bwd(L, q, k, v, o, lse, do, bshd, doc=None):
    """(dq, dk, dv) of toa_attn_bwd / toa_attn_bwd_doc: NaN-filled outputs,
    0xFF-filled workspace; o in the kernel's layout, do as [B, H, S, D]."""
    B, H, S, D = q.shape
    Hk = k.shape[1]
    P = L.ptr
    do = _bhsd(do, bshd).contiguous()
    dq, dk, dv = (torch.full_like(t, NAN) for t in (q, k, v))
    delta = torch.full((B, H, S), NAN, device=DEV, dtype=torch.float32)
    flags = 1 | (2 if bshd else 0)
    scale = 1.0 / math.sqrt(D)
    if doc is None:
        nws = L.call_ret("toa_attn_bwd_ws_bytes", B, H, S, D)
        ws = torch.full((nws,), 0xFF, device=DEV, dtype=torch.uint8) if nws else None
        L.call("toa_attn_bwd", P(q), P(k), P(v), P(o), P(do), P(lse), P(delta), P(ws), P(dq), P(dk), P(dv), B, H, Hk,
               S, D, flags, scale, L.stream(q))
    else:
        L.call("toa_attn_bwd_doc", P(q), P(k), P(v), P(o), P(do), P(lse), P(delta), P(doc[0]), P(doc[1]), P(dq),
               P(dk), P(dv), B, H, Hk, S, D, flags, scale, L.stream(q))
    torch.cuda.synchronize()
    return dq, dk, dv


def _check_fwd_bwd(L, case, bshd, what, doc=None):
    o, lse = _fwd(L, case.q, case.k, case.v, bshd, doc)
    case.check("o", _bhsd(o, bshd), what)
    case.check_lse(lse, what)
    for name, got in zip(("dq", "dk", "dv"), _bwd(L, case.q, case.k, case.v, o, lse, case.do, bshd, doc)):
        case.check(name, got, what)


# ---------------------------------------------------------------------------
# per-row bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("shape", an.RAGGED_SHAPES, ids=_id)
def test_ragged_rows(shape, bshd):
    """Ragged S: the register-staged HIP forward and the split backward."""
    L = _lib()
    _check_fwd_bwd(L, _case(shape), bshd, f"ragged {_id(shape)} bshd{int(bshd)}")


def _fwd_forms(D):
    return (0, 1, 2) if D == 128 else (0, 1)


def _bwd_forms(D):
    """(backward variant, dK/dV variant): split; dS form with the HIP dK/dV kernel; with the assembly one."""
    return ((0, -1), (1, 0), (1, 1)) if D == 128 else ((0, -1), (1, 0))


@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("shape,form", [(s, f) for s in an.BLOCK_SHAPES for f in _fwd_forms(s[4])],
                         ids=lambda x: _id(x) if isinstance(x, tuple) else f"fwd{x}")
def test_block_forward_rows(shape, form, bshd):
    """S % 256 == 0: the register-staged (0), LDS-DMA (1) and assembly (2) forwards."""
    L = _lib()
    case = _case(shape)
    what = f"fwd{form} {_id(shape)} bshd{int(bshd)}"
    with _forms(L, fwd=form):
        o, lse = _fwd(L, case.q, case.k, case.v, bshd)
    case.check("o", _bhsd(o, bshd), what)
    case.check_lse(lse, what)


@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("shape,form", [(s, f) for s in an.BLOCK_SHAPES for f in _bwd_forms(s[4])],
                         ids=lambda x: _id(x) if isinstance(x, tuple) and len(x) > 2 else f"bwd{x[0]}dkdv{x[1]}")
def test_block_backward_rows(shape, form, bshd):
    """S % 256 == 0: the split backward, and the dS-through-HBM one with each
    dK/dV kernel; O and lse from the default forward."""
    L = _lib()
    case = _case(shape)
    what = f"bwd{form[0]}dkdv{form[1]} {_id(shape)} bshd{int(bshd)}"
    o, lse = _fwd(L, case.q, case.k, case.v, bshd)
    with _forms(L, bwd=form[0], dkdv=form[1]):
        grads = _bwd(L, case.q, case.k, case.v, o, lse, case.do, bshd)
    for name, got in zip(("dq", "dk", "dv"), grads):
        case.check(name, got, what)


@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("D,dkdv", [(128, 1), (128, 0), (64, 0)])
@pytest.mark.parametrize("shape", an.ROPE_SHAPES, ids=_id)
def test_rope_backward_rows(shape, D, dkdv, bshd):
    """toa_attn_bwd_rope: the d(qkv) rows against the fp64 dq / dk rotated
    back in fp64 (dv as it is), each part's magnitude rotated by |cos| + |sin|;
    the model's dq / dk are rotated before their rounding, as the epilogues do."""
    L = _lib()
    from tf_operator_amd.ops import llm

    B, H, Hk, S = shape
    case = _case((B, H, Hk, S, D, False))
    cos, sin = llm.rope_tables(S, D, device=DEV)
    P = L.ptr
    flags = 1 | (2 if bshd else 0)
    o, lse = _fwd(L, case.q, case.k, case.v, bshd)
    do = _bhsd(case.do, bshd).contiguous()
    H3 = H + 2 * Hk
    with _forms(L, bwd=1, dkdv=dkdv):
        nws = L.call_ret("toa_attn_bwd_ws_bytes", B, H, S, D)
        assert nws > 0
        ws = torch.full((nws,), 0xFF, device=DEV, dtype=torch.uint8)
        delta = torch.full((B, H, S), NAN, device=DEV, dtype=torch.float32)
        dqkv = torch.full((B * S, H3 * D), NAN, device=DEV, dtype=torch.bfloat16)
        L.call("toa_attn_bwd_rope", P(case.q), P(case.k), P(case.v), P(o), P(do), P(lse), P(delta), P(ws), P(cos),
               P(sin), P(dqkv), B, H, Hk, S, D, flags, case.scale, L.stream(do))
        torch.cuda.synchronize()
    got = dqkv.view(B, S, H3, D).transpose(1, 2)   # [B, H3, S, D]
    c64, s64 = cos.double(), sin.double()
    ref, model = case.ref, case.model
    parts = (("dq", slice(0, H), an.rope_back(ref.dq, c64, s64), an.rope_mag(ref.mag_q, c64, s64),
              an.rope_back(model.dq_raw, c64, s64)),
             ("dk", slice(H, H + Hk), an.rope_back(ref.dk, c64, s64), an.rope_mag(ref.mag_k, c64, s64),
              an.rope_back(model.dk_raw, c64, s64)),
             ("dv", slice(H + Hk, H3), ref.dv, ref.mag_v, model.dv_raw))
    what = f"rope dkdv{dkdv} {_id(shape)}-{D} bshd{int(bshd)}"
    for name, cols, r, mag, m in parts:
        an.check_rows(what, name, got[:, cols], r, mag, m.to(torch.bfloat16), S, D)


@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("S", [257, 512])
@pytest.mark.parametrize("D", [64, 128])
def test_doc_rows(D, S, bshd):
    """toa_attn_fwd_doc / toa_attn_bwd_doc: document boundaries at 1, 64, 255,
    256, 257 (those < S) in batch row 0, at 64 and 256 in row 1."""
    L = _lib()
    case = _case((2, 4, 2, S, D, False), doc=True)
    _check_fwd_bwd(L, case, bshd, f"doc 2-4-2-{S}-{D} bshd{int(bshd)}", case.doc)


# ---------------------------------------------------------------------------
# causality, bit for bit
# ---------------------------------------------------------------------------
CUTS = (1, 64, 65, 256, 257)
# (shape, forward form, bshd): one ragged shape per head dim, one S = 512 shape per forward form
_CAUSAL_FWD = [((1, 4, 2, 300, D, False), -1, False) for D in (64, 128)] + \
              [((1, 4, 2, 512, D, False), f, True) for D in (128, 64) for f in _fwd_forms(D)]
# (shape, (backward, dK/dV) form, bshd)
_CAUSAL_BWD = [((1, 4, 2, 300, D, False), (-1, -1), False) for D in (64, 128)] + \
              [((1, 4, 2, 512, D, False), f, True) for D in (128, 64) for f in _bwd_forms(D)]


def _later_keys_changed(case, t):
    """k and v with everything at key positions >= t changed: keys x 8, values
    1e30 (finite: a correctly masked p = 0 gives exactly 0)."""
    k, v = case.k.clone(), case.v.clone()
    k[:, :, t:] *= 8.0
    v[:, :, t:] = 1e30
    return k, v


@pytest.mark.parametrize("shape,form,bshd", _CAUSAL_FWD, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_forward_rows_ignore_later_keys(shape, form, bshd):
    """O and lse of rows < t are bit for bit the same whatever stands at key
    positions >= t."""
    L = _lib()
    case = _case(shape)
    with _forms(L, fwd=form):
        o0, lse0 = _fwd(L, case.q, case.k, case.v, bshd)
        for t in (c for c in CUTS if c < case.S):
            k, v = _later_keys_changed(case, t)
            o1, lse1 = _fwd(L, case.q, k, v, bshd)
            assert torch.isfinite(lse1).all()
            assert torch.equal(_bhsd(o0, bshd)[:, :, :t], _bhsd(o1, bshd)[:, :, :t]), f"O rows < {t} changed"
            assert torch.equal(lse0[:, :, :t], lse1[:, :, :t]), f"lse rows < {t} changed"
            assert not torch.equal(lse0[:, :, t:], lse1[:, :, t:])   # the change itself arrived


@pytest.mark.parametrize("shape,form,bshd", _CAUSAL_FWD, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_forward_rows_under_changed_earlier_queries(shape, form, bshd):
    """Rows >= t of O and lse when the query rows < t change (q x -8).  They
    are not bit-stable, and not by a leak: the rescale of O and l is decided
    per wave of 32 query rows (see test_backward_rows_ignore_the_masked_side),
    so they move by rounding; they must stay within the per-row bound."""
    L = _lib()
    case = _case(shape)
    with _forms(L, fwd=form):
        for t in (c for c in CUTS if c < case.S):
            q2 = case.q.clone()
            q2[:, :, :t] *= -8.0
            o, lse = _fwd(L, q2, case.k, case.v, bshd)
            e, row = an.row_err(_bhsd(o, bshd)[:, :, t:], case.ref.o[:, :, t:], case.ref.mag_o[:, :, t:])
            dl = float((lse[:, :, t:].double() - case.ref.lse[:, :, t:]).abs().max())
            print(f"rows q < {t} changed, fwd{form} {_id(shape)} o: {e / U:.3f} u at {row}; lse {dl:.3e}")
            assert e <= case.tol["o"] and dl <= case.lse_tol, (t, e / U, dl)


@pytest.mark.parametrize("shape,form,bshd", _CAUSAL_BWD, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_backward_rows_ignore_the_masked_side(shape, form, bshd):
    """dQ rows < t are bit for bit the same whatever stands at key positions
    >= t (O and lse recomputed by the forward from the changed k, v); dK and
    dV rows >= t whatever stands at query positions < t (q x -8 and dO = 1e20
    there).

    For the second half O and lse of the rows < t are recomputed by the
    forward from the changed q, but the rows >= t are the unchanged run's,
    because the forward's own rows >= t are not bit-stable under a change to
    another query row, and that is not a leak: every forward kernel decides
    per wave (32 query rows), not per row, whether a tile's new maximum is
    worth a rescale of O and l (attention.hip, `__any(mx > m_run +
    RESCALE_THR)`), so the rows of a wave steer which maximum their
    neighbours' P is rounded against.  Measured on an MI355X with row 256
    changed: rows 257-287 of O move in their last bf16 bit, lse by up to
    1.6e-4, and dK / dV from such O / lse in their last bit too.  With O
    and lse recomputed for every row, dK and dV rows >= t therefore answer to
    the per-row bound instead (against the unchanged inputs' reference, which
    is exact for these rows)."""
    L = _lib()
    case = _case(shape)
    q, k, v, do = case.q, case.k, case.v, case.do

    def bwd(q, k, v, o, lse, do):
        with _forms(L, bwd=form[0], dkdv=form[1]):
            return _bwd(L, q, k, v, o, lse, do, bshd)

    o0, lse0 = _fwd(L, q, k, v, bshd)
    dq0, dk0, dv0 = bwd(q, k, v, o0, lse0, do)
    assert all(bool(torch.isfinite(x.float()).all()) for x in (dq0, dk0, dv0))
    for t in (c for c in CUTS if c < case.S):
        k1, v1 = _later_keys_changed(case, t)
        dq1, dk1, _ = bwd(q, k1, v1, *_fwd(L, q, k1, v1, bshd), do)
        assert torch.equal(dq0[:, :, :t], dq1[:, :, :t]), f"dQ rows < {t} changed"
        assert not torch.equal(dk0[:, :, t:], dk1[:, :, t:])
        q2, do2 = q.clone(), do.clone()
        q2[:, :, :t] *= -8.0
        do2[:, :, :t] = 1e20
        o2, lse2 = _fwd(L, q2, k, v, bshd)
        _, dk2, dv2 = bwd(q2, k, v, o2, lse2, do2)
        what = f"q < {t} changed, bwd{form[0]}dkdv{form[1]} {_id(shape)}"
        for name, got in (("dk", dk2), ("dv", dv2)):
            e, row = an.row_err(got[:, :, t:], getattr(case.ref, name)[:, :, t:],
                                getattr(case.ref, case.NAMES[name])[:, :, t:])
            print(f"rows {what} {name}: {e / U:.3f} u at {row} (limit {case.tol[name] / U:.3f} u)")
            assert e <= case.tol[name], f"{what}: {name} rows >= {t} off by {e / U:.2f} u"
        _bhsd(o2, bshd)[:, :, t:] = _bhsd(o0, bshd)[:, :, t:]
        lse2[:, :, t:] = lse0[:, :, t:]
        _, dk3, dv3 = bwd(q2, k, v, o2, lse2, do2)
        assert torch.equal(dk0[:, :, t:], dk3[:, :, t:]), f"dK rows >= {t} changed"
        assert torch.equal(dv0[:, :, t:], dv3[:, :, t:]), f"dV rows >= {t} changed"
        assert not torch.equal(dv0[:, :, :t], dv3[:, :, :t])


# ---------------------------------------------------------------------------
# cross entropy and SwiGLU, per element
# ---------------------------------------------------------------------------
def _xent(L, x, t, ldx, grad=True):
    """(loss, lse, dx buffer [rows, ldx]) of toa_xent_fwd / toa_xent_bwd on a
    row-strided x; outputs NaN-filled, so the dx buffer's pad columns must
    still be NaN afterwards."""
    rows, V = x.shape
    P = L.ptr
    loss = torch.full((rows,), NAN, device=DEV, dtype=torch.float32)
    lse = torch.full((rows,), NAN, device=DEV, dtype=torch.float32)
    L.call("toa_xent_fwd", L.dtype_code(x), P(x), P(t), P(loss), P(lse), rows, V, ldx, -100, L.stream(x))
    dbuf = torch.full((rows, ldx), NAN, device=DEV, dtype=x.dtype)
    if grad:
        go = torch.ones(1, device=DEV)
        nv = (t != -100).sum().float().reshape(1)
        L.call("toa_xent_bwd", L.dtype_code(x), P(x), P(t), P(lse), P(go), P(nv), P(dbuf), rows, V, ldx, -100,
               L.stream(x))
    torch.cuda.synchronize()
    return loss, lse, dbuf


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [10, 1000, 4104])
def test_cross_entropy_rows(V, dt):
    """loss, lse and the gradient of every row against fp64, the row stride
    V + 8; 4104 = 513 chunks of 8: the unroll-2 main loop (thread 0) and its
    remainder loop.

    Bounds.  lse and loss are fp32 sums of fast exp2 / log2 at arguments up
    to 2^5: the argument's rounding (2^5 x 1.44 x 2^-24) and a 2 ulp exp give
    each term, so the sum, a relative 2^-18; the logarithm and the fp32 lse
    itself (2^5 x 2^-24) stay below that: 2^-15 absolute leaves a factor 4.
    The gradient: |got - ref| <= 3 u (p + onehot) / n_valid per element for
    bf16 logits (one rounding of the result is u); for fp32 logits p carries
    the relative 2^-18 of its exponent's argument and the same of lse: 2^-15."""
    L = _lib()
    g = torch.Generator().manual_seed(V)
    rows, ldx = 5, V + 8
    buf = (3 * torch.randn(rows, ldx, generator=g)).to(dt).to(DEV)
    x = buf[:, :V]
    t = torch.randint(0, V, (rows,), generator=g).to(DEV)
    t[2] = -100
    valid = t != -100
    n = int(valid.sum())
    x64 = x.double()
    lse_ref = torch.logsumexp(x64, -1)
    tc = t.clamp(min=0)
    loss_ref = torch.where(valid, lse_ref - x64.gather(1, tc[:, None]).squeeze(1), torch.zeros_like(lse_ref))
    onehot = torch.zeros_like(x64).scatter_(1, tc[:, None], 1.0) * valid[:, None]
    p = torch.softmax(x64, -1)
    grad_ref = (p - onehot) * valid[:, None] / n
    loss, lse, dbuf = _xent(L, x, t, ldx)
    dlse, dloss = float((lse - lse_ref).abs().max()), float((loss - loss_ref).abs().max())
    print(f"xent V={V} {dt}: lse dev {dlse:.2e}, loss dev {dloss:.2e}")
    assert dlse <= 2.0 ** -15 and dloss <= 2.0 ** -15, (dlse, dloss)
    assert float(loss[2]) == 0.0
    dx = dbuf[:, :V]
    assert torch.isnan(dbuf[:, V:]).all(), "the backward wrote past a row's V columns"
    assert torch.isfinite(dx).all()
    assert bool((dx[2] == 0).all()), "an ignored row's gradient is exactly zero"
    eps = 3 * U if dt == torch.bfloat16 else 2.0 ** -15
    excess = ((dx.double() - grad_ref).abs() - eps * (p + onehot) / n).max()
    print(f"xent V={V} {dt}: worst gradient error / bound "
          f"{float(((dx.double() - grad_ref).abs() / (eps * (p + onehot) / n)).max()):.3f}")
    assert float(excess) <= 0.0
    # the unroll switch changes nothing, bit for bit
    try:
        for u in (1, 4, 2):
            L.call("toa_xent_set_unroll", u)
            assert torch.equal(_xent(L, x, t, ldx)[2][:, :V], dx), f"unroll {u}"
    finally:
        L.call("toa_xent_set_unroll", 2)
    # all rows ignored: loss 0, gradient zero, nothing NaN
    none = torch.full_like(t, -100)
    loss0, lse0, dbuf0 = _xent(L, x, none, ldx)
    assert bool((loss0 == 0).all()) and float((lse0 - lse_ref).abs().max()) <= 2.0 ** -15
    assert bool((dbuf0[:, :V] == 0).all())
    from tf_operator_amd.ops.llm import cross_entropy

    xa = x.detach().clone().requires_grad_()
    la = cross_entropy(xa, none)
    la.backward()
    assert float(la.detach()) == 0.0 and bool((xa.grad == 0).all())


def test_swiglu_past_the_grid_cap():
    """The row kernels launch at most 4096 workgroups and stride beyond:
    T = 4100 rows, F = 8.  Per element against fp64, <= 2 u (the result's
    rounding and fp32 arithmetic with a fast exp) of |silu(g) u| forward, of
    |d silu(g)| and |d u| sig(g) (1 + |g| (1 - sig(g))) backward."""
    L = _lib()
    from tf_operator_amd.ops import llm

    T, F = 4100, 8
    gen = torch.Generator().manual_seed(8)
    gu = torch.randn(T, 2 * F, generator=gen).to(torch.bfloat16).to(DEV)
    d = torch.randn(T, F, generator=gen).to(torch.bfloat16).to(DEV)
    out = llm.swiglu(gu)
    dgu = llm.swiglu_bwd(d, gu)
    torch.cuda.synchronize()
    g, up, dd = gu[:, :F].double(), gu[:, F:].double(), d.double()
    sg = torch.sigmoid(g)
    ref = g * sg * up
    assert bool(((out.double() - ref).abs() <= 2 * U * ref.abs()).all()), \
        int(((out.double() - ref).abs() > 2 * U * ref.abs()).nonzero()[0, 0])
    du_ref = dd * g * sg
    dg_ref = dd * up * sg * (1 + g * (1 - sg))
    dg_mag = (dd * up).abs() * sg * (1 + g.abs() * (1 - sg))
    bad = ((dgu[:, F:].double() - du_ref).abs() > 2 * U * du_ref.abs()) | \
          ((dgu[:, :F].double() - dg_ref).abs() > 2 * U * dg_mag)
    assert not bool(bad.any()), int(bad.nonzero()[0, 0])
