"""The row kernels of the Llama step row by row (tests/rowwise_numerics.py):
RMSNorm / LayerNorm, RoPE, SwiGLU, cross entropy and the embedding backward,
every output row within min(3 x the model's own error + the fp32 floor, cap)
of the fp64 reference, relative to the magnitude of what was summed into it,
at the smallest shapes that reach each path: a second row per wave in
norm_bwd_kernel, a second unit per thread in rope_bwd_kernel, rows past the
SwiGLU grid cap, the unrolled main loop, remainder loop and scalar tail of
the cross-entropy kernels, a second column pass in embed_bwd_kernel.

Outputs are pre-filled with NaN where the launcher is called directly, so an
unwritten row fails.  The largest ratios seen on an MI355X are in
docs/kernels.md ("Per-row tolerances of the row kernels")."""
import pytest
import torch

import rowwise_numerics as rn
from rowwise_numerics import BF16, FP32

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DTS = [BF16, FP32]
_dt = lambda d: "bf16" if d == BF16 else "fp32"
_ids = lambda x: _dt(x) if isinstance(x, torch.dtype) else str(x)


def _lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def _nan(*shape, dtype):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


# ---------------------------------------------------------------------------
# RMSNorm / LayerNorm
# ---------------------------------------------------------------------------
def _norm_case(rows, cols, dtype, rms, res):
    return rn.NormCase(rows, cols, dtype, rms, res, device=DEV)


def _norm_fwd(L, case):
    """{h, y, rstd, mean} of toa_rmsnorm_fwd / toa_layernorm_fwd into NaN-filled outputs."""
    i, rows, cols, dt = case.inp, case.rows, case.cols, case.dtype
    P, code, s = L.ptr, L.dtype_code(case.inp.x), L.stream(case.inp.x)
    out = {"y": _nan(rows, cols, dtype=dt), "rstd": _nan(rows, dtype=FP32)}
    r = i.r if case.res else None
    h = out["h"] = _nan(rows, cols, dtype=dt) if case.res else None
    if case.rms:
        L.call("toa_rmsnorm_fwd", code, P(i.x), P(r), P(h), P(i.w), P(out["y"]), P(out["rstd"]), rows, cols,
               case.eps, s)
    else:
        out["mean"] = _nan(rows, dtype=FP32)
        L.call("toa_layernorm_fwd", code, P(i.x), P(r), P(h), P(i.w), P(i.b), P(out["y"]), P(out["mean"]),
               P(out["rstd"]), rows, cols, case.eps, s)
    torch.cuda.synchronize()
    return out


def _norm_bwd(L, case, fwd):
    """{dx, dw, db} of toa_rmsnorm_bwd / toa_layernorm_bwd from the forward's
    own h, rstd and mean: NaN-filled outputs and partial workspace, fp32 dw /
    db, overwritten (not accumulated)."""
    i, rows, cols, dt = case.inp, case.rows, case.cols, case.dtype
    P, code, s = L.ptr, L.dtype_code(case.inp.x), L.stream(case.inp.x)
    h = fwd["h"] if case.res else i.x
    dadd = i.dh if case.res else None
    nb = L.call_ret("toa_norm_bwd_blocks", rows, cols)
    partial = _nan(nb * cols * (1 if case.rms else 2), dtype=FP32)
    out = {"dx": _nan(rows, cols, dtype=dt), "dw": _nan(cols, dtype=FP32)}
    if case.rms:
        L.call("toa_rmsnorm_bwd", code, P(i.dy), P(h), P(i.w), P(fwd["rstd"]), P(dadd), P(out["dx"]), P(partial),
               P(out["dw"]), 0, 0, rows, cols, s)
    else:
        out["db"] = _nan(cols, dtype=FP32)
        L.call("toa_layernorm_bwd", code, P(i.dy), P(h), P(i.w), P(fwd["mean"]), P(fwd["rstd"]), P(dadd),
               P(out["dx"]), P(partial), P(out["dw"]), 0, P(out["db"]), 0, 0, rows, cols, s)
    torch.cuda.synchronize()
    return out


def _check_norm(L, case, what):
    fwd = _norm_fwd(L, case)
    got = {**fwd, **_norm_bwd(L, case, fwd)}
    for name in case.names:
        case.check(name, got[name], what)


_WAVE = [(rows, cols, dtype, rms, res) for rows, cols in rn.NORM_WAVE_TALL + rn.NORM_WAVE_SHORT for dtype in DTS
         for rms in (True, False) for res in (False, True)]


@pytest.mark.parametrize("rows,cols,dtype,rms,res", _WAVE, ids=_ids)
def test_norm_wave_form_rows(rows, cols, dtype, rms, res):
    """The one-row-per-wave kernels: a second row per wave with the dW / db
    accumulators carried over (tall cases; 4104 columns re-read the row), a
    partly filled last chunk group, fewer rows than a workgroup's four waves."""
    L = _lib()
    assert cols % 2048 != 0
    if (rows, cols) in rn.NORM_WAVE_TALL:
        assert L.call_ret("toa_norm_bwd_blocks", rows, cols) * 4 < rows, "no wave takes a second row any more"
    kind = ("rms" if rms else "ln") + ("+res" if res else "")
    _check_norm(L, _norm_case(rows, cols, dtype, rms, res), f"wave {kind} {rows}x{cols} {_dt(dtype)}")


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("rows,cols", rn.NORM_ROW, ids=_ids)
def test_norm_row_form_rows(rows, cols, res):
    """The one-row-per-workgroup RMSNorm kernels (bf16, cols % 2048 == 0): one
    row, three rows in one workgroup of the backward, 301."""
    L = _lib()
    _check_norm(L, _norm_case(rows, cols, BF16, True, res), f"row rms{'+res' if res else ''} {rows}x{cols}")


@pytest.mark.parametrize("cols", [2048, 6144])
def test_norm_row_form_grid_stride_is_bit_identical(cols):
    """rms_fwd_row_kernel with its grid capped at 3 workgroups for 10 rows
    (four rows through the double-buffered LDS slot): h, y, rstd bit for bit
    those of the uncapped run."""
    L = _lib()
    case = _norm_case(10, cols, BF16, True, True)
    free = _norm_fwd(L, case)
    try:
        L.call("toa_norm_set_fwd_cap", 3)
        capped = _norm_fwd(L, case)
    finally:
        L.call("toa_norm_set_fwd_cap", 0)
    for name in ("h", "y", "rstd"):
        assert torch.isfinite(free[name].float()).all()
        assert torch.equal(capped[name], free[name]), name
        case.check(name, capped[name], f"row capped 10x{cols}")


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rep", ["gqa", 1])
@pytest.mark.parametrize("shape", rn.ROPE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rope_rows(shape, rep):
    """toa_rope_fwd / toa_rope_bwd: every head row of q, k, v and of dqkv (the
    replica sum in dk / dv included).  The large shape has more units than the
    backward's 2048 x 256 threads: a second unit per thread."""
    L = _lib()
    from tf_operator_amd.ops import llm

    B, S, Hq, Hkv, D = shape
    rep = Hq // Hkv if rep == "gqa" else 1
    H3 = Hq + 2 * Hkv
    if S > 1:
        assert B * S * H3 * (D // 16) > 2048 * 256
    cos, sin = llm.rope_tables(S, D, device=DEV)
    qkv, dq, dk, dv = rn.rope_inputs(B, S, Hq, Hkv, D, rep, device=DEV)
    ref = rn.rope_ref64(qkv, dq, dk, dv, cos, sin, B, S, Hq, Hkv, D, rep)
    P = L.ptr
    q = _nan(B, Hq, S, D, dtype=BF16)
    k, v = _nan(B, Hkv * rep, S, D, dtype=BF16), _nan(B, Hkv * rep, S, D, dtype=BF16)
    L.call("toa_rope_fwd", P(qkv), P(cos), P(sin), P(q), P(k), P(v), B, S, Hq, Hkv, D, rep, L.stream(qkv))
    dqkv = _nan(B * S, H3 * D, dtype=BF16)
    L.call("toa_rope_bwd", P(dq), P(dk), P(dv), P(cos), P(sin), P(dqkv), B, S, Hq, Hkv, D, rep, L.stream(qkv))
    torch.cuda.synchronize()
    what = f"rope {'-'.join(map(str, shape))} rep{rep}"
    got = {"q": q, "k": k, "v": v, "dqkv": dqkv.view(B, S, H3, D).transpose(1, 2)}
    for name, g in got.items():
        r = getattr(ref, name)
        rn.check_rows(what, name, g, r, getattr(ref, "mag_" + name), rn.rnd(r, BF16), rep + 2, BF16)
    assert torch.equal(v.double(), ref.v), "v is a copy"


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,F", rn.SWIGLU_SHAPES)
def test_swiglu_rows(T, F):
    """T = 4133 rows: the row forms launch at most 4096 workgroups and stride
    beyond.  Gates at +-20 and +-90 (exp(-g) saturates / overflows fp32): the
    result is silu -> g or 0, never NaN.  The flat forms are bit-identical."""
    L = _lib()
    assert T > 4096
    gu, d = rn.swiglu_inputs(T, F, device=DEV)
    ref = rn.swiglu_ref64(gu, d)

    def run():
        """(out, dgu) of toa_swiglu_fwd / toa_swiglu_bwd, the launchers themselves, into NaN-filled outputs."""
        out, dgu = _nan(T, F, dtype=BF16), _nan(T, 2 * F, dtype=BF16)
        L.call("toa_swiglu_fwd", L.ptr(gu), L.ptr(out), T, F, L.stream(gu))
        L.call("toa_swiglu_bwd", L.ptr(d), L.ptr(gu), L.ptr(dgu), T, F, L.stream(gu))
        return out, dgu

    out, dgu = run()
    old = L.lib().toa_set_stream_variant(0)
    try:
        out_flat, dgu_flat = run()
    finally:
        L.lib().toa_set_stream_variant(old)
    torch.cuda.synchronize()
    assert old & 2, "row-structured SwiGLU is the default"
    assert torch.isfinite(out.float()).all() and torch.isfinite(dgu.float()).all()
    assert torch.equal(out_flat, out) and torch.equal(dgu_flat, dgu)
    what = f"swiglu {T}x{F}"
    for name, g in (("out", out), ("dg", dgu[:, :F]), ("du", dgu[:, F:])):
        r = getattr(ref, name)
        rn.check_rows(what, name, g, r, getattr(ref, "mag_" + name), rn.rnd(r, BF16), 2, BF16)


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
def _xent(L, x, t, grad_out=1.0):
    """(loss, lse, dx) of toa_xent_fwd / toa_xent_bwd on contiguous logits, NaN-filled outputs."""
    rows, V = x.shape
    assert x.is_contiguous()
    P = L.ptr
    loss, lse = _nan(rows, dtype=FP32), _nan(rows, dtype=FP32)
    L.call("toa_xent_fwd", L.dtype_code(x), P(x), P(t), P(loss), P(lse), rows, V, V, -100, L.stream(x))
    dx = _nan(rows, V, dtype=x.dtype)
    go = torch.full((1,), grad_out, device=DEV)
    nv = (t != -100).sum().float().reshape(1)
    L.call("toa_xent_bwd", L.dtype_code(x), P(x), P(t), P(lse), P(go), P(nv), P(dx), rows, V, V, -100, L.stream(x))
    torch.cuda.synchronize()
    return loss, lse, dx


def _check_xent(what, x, t, loss, lse, dx, grad_out):
    V, dt = x.shape[1], x.dtype
    ref = rn.xent_ref64(x, t, grad_out)
    assert torch.isfinite(ref.loss).all() and torch.isfinite(loss).all() and torch.isfinite(lse).all()
    for name, got in (("lse", lse), ("loss", loss)):
        r = getattr(ref, name)
        rn.check_rows(what, name, got[:, None], r, getattr(ref, "mag_" + name), rn.rnd(r, FP32), V, FP32)
    assert bool((loss[~ref.valid] == 0).all()), "the loss of an ignored row is exactly 0"
    rn.xent_check_grad(what, dx, ref, dt)
    return ref


@pytest.mark.parametrize("dtype", DTS, ids=_dt)
@pytest.mark.parametrize("V", rn.XENT_V)
def test_xent_rows(V, dtype):
    """loss and lse per row and the gradient in two parts (softmax part,
    target entry) with grad_out = 0.37; targets in the first, the last and a
    remainder-loop column, one row ignored.  8200 = 1025 chunks of 8: one full
    unroll-2 round per thread and chunk 1024 in the remainder loop; 8203: the
    scalar path; 10: fewer columns than one chunk.  All targets ignored: loss
    0, gradient exactly 0.  The unroll switch exists for bf16 logits only (fp32
    logits always run xent_bwd_kernel<float, 1>, whose one loop takes every
    chunk): the unroll-2 arithmetic and "every unroll setting bit for bit" are
    asserted for bf16 alone."""
    L = _lib()
    if V == 8200 and dtype == BF16:
        nb, unroll, v8 = rn.XENT_BLOCK, 2, V // 8
        assert V % 8 == 0 and v8 == 2 * nb + 1                      # one full round of U = 2 for every thread ...
        assert (nb - 1) + (unroll - 1) * nb < v8 <= unroll * nb + 1  # ... and exactly chunk 1024 left for thread 0
    if V == 8203:
        assert V % 8 != 0
    x, t = rn.xent_inputs(V, dtype, device=DEV)
    what = f"xent V={V} {_dt(dtype)}"
    loss, lse, dx = _xent(L, x, t, 0.37)
    _check_xent(what, x, t, loss, lse, dx, 0.37)
    if dtype == BF16:
        try:
            for u in (1, 4, 2):
                L.call("toa_xent_set_unroll", u)
                assert torch.equal(_xent(L, x, t, 0.37)[2], dx), f"unroll {u}"
        finally:
            L.call("toa_xent_set_unroll", 2)
    none = torch.full_like(t, -100)
    loss0, lse0, dx0 = _xent(L, x, none, 0.37)
    assert bool((loss0 == 0).all()) and bool((dx0 == 0).all()) and torch.equal(lse0, lse)


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("dtype", DTS, ids=_dt)
@pytest.mark.parametrize("V", [8200, 10])
def test_xent_column_sliced_logits(V, dtype, inplace):
    """Logits that are a column slice of a wider buffer (row stride V + 8)
    through ops.llm.cross_entropy: loss and gradient equal those of the
    contiguous copy, bit for bit; the parent's 8 padding columns are untouched,
    and its logits too unless the gradient is written in place."""
    _lib()
    from tf_operator_amd.ops.llm import cross_entropy

    x, t = rn.xent_inputs(V, dtype, device=DEV)
    rows = x.shape[0]
    parent = torch.full((rows, V + 8), 7.0, device=DEV, dtype=dtype)
    parent[:, :V] = x
    xc = x.clone().requires_grad_()
    lc = cross_entropy(xc, t)
    lc.backward()
    xv = parent[:, :V].detach().requires_grad_()
    assert xv.stride() == (V + 8, 1) and xv.data_ptr() == parent.data_ptr()
    lv = cross_entropy(xv, t, inplace_grad=inplace)
    lv.backward()
    torch.cuda.synchronize()
    assert float(lv.detach()) == float(lc.detach())
    assert xv.grad.shape == (rows, V) and torch.equal(xv.grad, xc.grad)
    assert bool((parent[:, V:] == 7.0).all()), "the padding columns were written"
    assert torch.equal(parent[:, :V], xc.grad if inplace else x)
    ref = rn.xent_ref64(x, t)
    rn.xent_check_grad(f"xent view V={V} {_dt(dtype)} inplace{int(inplace)}", xv.grad, ref, dtype)


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
def test_xent_expanded_row_is_copied(inplace):
    """Logits whose rows overlap (one row expanded to four, row stride 0)
    cannot be walked with a row stride: cross_entropy copies them, so loss and
    gradient are those of the contiguous copy and the one stored row is left
    alone, also with inplace_grad."""
    _lib()
    from tf_operator_amd.ops.llm import cross_entropy

    V = 1000
    row = rn.xent_inputs(V, BF16, device=DEV)[0][:1].clone()
    keep = row.clone()
    t = torch.tensor([0, V - 1, 17, -100], device=DEV)
    xe = row.expand(4, V).detach().requires_grad_()
    assert xe.stride() == (0, 1)
    xc = row.repeat(4, 1).requires_grad_()
    le, lc = cross_entropy(xe, t, inplace_grad=inplace), cross_entropy(xc, t)
    le.backward()
    lc.backward()
    torch.cuda.synchronize()
    assert float(le.detach()) == float(lc.detach())
    assert xe.grad.shape == (4, V) and torch.equal(xe.grad, xc.grad)
    assert torch.equal(row, keep)
    rn.xent_check_grad(f"xent expanded inplace{int(inplace)}", xe.grad, rn.xent_ref64(xc.detach(), t), BF16)


@pytest.mark.parametrize("half", ["upper", "lower"])
@pytest.mark.parametrize("dtype", DTS, ids=_dt)
@pytest.mark.parametrize("V", [8200, 8203, 1000, 10])
def test_xent_masked_vocabulary(V, dtype, half):
    """Half the columns -inf (a masked or padded vocabulary), the targets in
    the other half: finite loss and lse equal to the reference, gradient 0 in
    the masked columns.  Threads whose first chunk (V = 1000 upper, 8200
    lower) or first column (V = 10, 8203 lower) is -inf start from m = -inf."""
    L = _lib()
    x, t = rn.xent_inputs(V, dtype, device=DEV)
    h = V // 2
    if half == "upper":
        x[:, h:] = float("-inf")
        t = torch.where(t >= 0, t % h, t)
    else:
        x[:, :h] = float("-inf")
        t = torch.where(t >= 0, h + t % (V - h), t)
    loss, lse, dx = _xent(L, x, t)
    _check_xent(f"xent masked {half} V={V} {_dt(dtype)}", x, t, loss, lse, dx, 1.0)
    assert bool((dx[:, h:] if half == "upper" else dx[:, :h]).eq(0).all())


# ---------------------------------------------------------------------------
# embedding backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gdtype", DTS, ids=_dt)
@pytest.mark.parametrize("dim", rn.EMBED_DIMS)
@pytest.mark.parametrize("kind", ["one", "run", "distinct"])
def test_embedding_backward_rows(kind, dim, gdtype):
    """embed_bwd_kernel per vocabulary row at dim > 2048 (a second pass of
    256 x 8 columns): one token; repeated ids with a run that ends the sorted
    list; every id distinct.  Rows of absent ids stay as they were; two runs
    are bit-identical.  toa_embed_bwd itself is called, with the stable sort
    ops.embedding._scatter_rows makes, so no torch path can stand in."""
    L = _lib()
    assert dim > 256 * 8
    base, idx, dy = rn.embed_inputs(kind, dim, gdtype, device=DEV)
    ref = rn.embed_ref64(base, idx, dy)
    outs = []
    for _ in range(2):
        g = base.clone()
        srt, perm = torch.sort(idx.long(), stable=True)
        L.call("toa_embed_bwd", L.ptr(srt), L.ptr(perm), L.ptr(dy), L.ptr(g), int(gdtype == FP32), idx.numel(), dim,
               L.stream(dy))
        outs.append(g)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    absent = torch.ones(base.shape[0], dtype=torch.bool, device=DEV)
    absent[idx] = False
    assert torch.equal(outs[0][absent], base[absent])
    rn.check_rows(f"embed {kind} dim={dim} {_dt(gdtype)}", "grad", outs[0], ref.grad, ref.mag, ref.model, ref.n,
                  gdtype)
