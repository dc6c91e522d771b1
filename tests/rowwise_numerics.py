"""Per-row numerics of the row kernels of the Llama step: RMSNorm / LayerNorm
(csrc/hip/norm.hip), RoPE, SwiGLU, cross entropy and the embedding backward
(csrc/hip/llm.hip).  For each operation: an explicit fp64 reference (forward
and backward, no autograd) on the inputs' values with the magnitude of every
output (the same sums over absolute values), and a model: the fp64 result with
only the roundings a correct kernel must make (the output to its dtype; h to
its dtype before the statistics in add + norm; one rounding of old + sum in the
embedding gradient).

Why per row: one norm row wrong by 10 % in 777 moves the whole-tensor
||a - b|| / ||b|| by 0.4 %, and the one-hot entry of a cross-entropy gradient
row carries almost all of that row's norm at a large vocabulary, so the
softmax part can be wrong over thousands of columns unnoticed.

The tolerance is the attention rule (tests/attn_numerics.py): a row passes at
min(FACTOR x the model's row_err on the same inputs + floor, cap), floor = the
length of the longest fp32 sum (columns, vocabulary, run of equal ids) x 2^-24.
For bf16 outputs cap = CAP = 8 u (u = 2^-9); for fp32 outputs (fp32 tensors,
rstd, mean, dW, db, loss, lse) the same rule in the fp32 unit, cap = 8 x 2^-24.
There the floor is mostly larger than the cap, so the cap is what binds: a
correct kernel's tree-shaped sums stay within a few units, and an lse that
misses its last chunk of 8 columns at V = 8200 is 2 285 units off.  One output
needs more than 8 units, see CAPS.

A plain helper module: no fixtures, imported by tests/test_rowwise.py (CPU)
and tests/test_rowwise_gpu.py.
"""
from types import SimpleNamespace as NS

import torch

import attn_numerics as an
from attn_numerics import CAP, FACTOR, U, row_err

U32 = 2.0 ** -24         # half an fp32 ulp
BF16, FP32 = torch.bfloat16, torch.float32
# per-output factors above 3, where a correct kernel needed one (docs/kernels.md, "Per-row tolerances of the row kernels")
FACTORS = {}
# per-output caps above 8 units, keyed (name, dtype).  The softmax part of the cross-entropy gradient with fp32 logits:
# p = exp(x - lse) takes the absolute error of the stored fp32 lse as a relative error of the whole row, and half an ulp
# of an lse in [8, 16) (V = 8200, logits 3 randn: lse 13.5) is 2^-21 = 8 units before any rounding of p itself: 8 + 8.
# Measured on an MI355X: 10.0 units at V = 8203, 4.6 at V = 10 (docs/kernels.md).
CAPS = {("dx softmax part", torch.float32): 16 * 2.0 ** -24}

# ---------------------------------------------------------------------------
# the shapes of the GPU tests; tests/test_rowwise.py checks the model at the same inputs
# ---------------------------------------------------------------------------
# one-row-per-wave norm kernels.  Tall: a wave takes a second row (toa_norm_bwd_blocks(rows, cols) * 4 < rows);
# 520 and 4104 columns: a partly filled last chunk group per lane; 1, 2, 3, 5 rows: less than / just over a workgroup
NORM_WAVE_TALL = [(3077, 64), (3077, 520), (1029, 4104)]
NORM_WAVE_SHORT = [(1, 520), (2, 520), (3, 520), (5, 520)]
# one-row-per-workgroup RMSNorm kernels (bf16, cols % 2048 == 0)
NORM_ROW = [(rows, cols) for cols in (2048, 6144) for rows in (1, 3, 301)]
# (B, S, Hq, Hkv, D): 655 360 units, more than the backward's 2048 x 256 threads; one chunk per half head at S = 1
ROPE_SHAPES = [(2, 1024, 32, 4, 128), (2, 1, 4, 2, 16)]
SWIGLU_SHAPES = [(4133, 8), (4133, 264)]     # T past the 4096-workgroup cap of the row forms
XENT_V = [8200, 8203, 10]                    # unrolled main loop + remainder; scalar path; fewer columns than a chunk
XENT_BLOCK = 512                             # threads per row of the cross-entropy kernels
EMBED_DIMS = [2056, 4096]                    # a second pass of 256 x 8 columns, partly and wholly filled


def unit(dtype):
    return U if dtype == BF16 else U32


def rnd(x, dtype):
    """x (fp64) rounded to dtype, back in fp64."""
    return x.to(dtype).to(torch.float64)


def fp32_floor(n):
    """What an fp32 sum of n terms can add that the model (fp64 between its
    roundings) does not have: a worst-case 2^-24 per term."""
    return n * 2.0 ** -24


def row_tol(model_err, n, dtype, name=None):
    """min(3 x the model's row_err + floor(n), cap), cap = 8 units of dtype (module docstring)."""
    cap = CAPS.get((name, dtype), CAP if dtype == BF16 else 8 * U32)
    return min(FACTORS.get(name, FACTOR) * model_err + fp32_floor(n), cap)


def check_rows(what, name, got, ref, mag, model, n, dtype):
    """Assert row_err(got) <= row_tol(row_err(model)) against the same
    reference and magnitude (a row is the last dimension; a quantity with one
    number per row is passed as [..., 1]).  n: the longest fp32 sum; dtype:
    the output's.  Prints and returns row_err in units of unit(dtype)."""
    u = unit(dtype)
    me = row_err(model, ref, mag)[0]
    tol = row_tol(me, n, dtype, name)
    e, row = row_err(got, ref, mag)
    print(f"rows {what} {name}: {e / u:.3f} u at {row} (model {me / u:.3f} u, limit {tol / u:.3f} u)")
    assert e <= tol, (f"{what} {name}: row {row} is off by {e / u:.2f} u of its magnitude, limit {tol / u:.2f} u "
                      f"(model {me / u:.2f} u)")
    return e / u


def rows_ok(name, got, ref, mag, model, n, dtype):
    return row_err(got, ref, mag)[0] <= row_tol(row_err(model, ref, mag)[0], n, dtype, name)


def rel(a, b):
    """The whole-tensor measure of tests/test_ops_gpu.py."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-12))


# ---------------------------------------------------------------------------
# RMSNorm / LayerNorm (+ residual add)
# ---------------------------------------------------------------------------
def norm_inputs(rows, cols, dtype, seed=0, device="cpu"):
    """x, r, w, b, dy, dh from a CPU generator (the same values on every
    device).  The rows of x differ in scale and are shifted, so every row has
    its own rstd and a mean that matters."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + cols)
    scale = 0.5 + (torch.arange(rows) % 5).double()[:, None]
    x = (torch.randn(rows, cols, generator=g, dtype=torch.float64) * scale + 0.25).to(dtype)
    r, dy, dh = (torch.randn(rows, cols, generator=g).to(dtype) for _ in range(3))
    w = (1 + 0.1 * torch.randn(cols, generator=g)).to(dtype)
    b = (0.1 * torch.randn(cols, generator=g)).to(dtype)
    return NS(**{k: v.to(device) for k, v in dict(x=x, r=r, w=w, b=b, dy=dy, dh=dh).items()})


NORM_OUT = {"h": "mag_h", "y": "mag_y", "dx": "mag_dx", "rstd": "mag_rstd", "mean": "mag_mean", "dw": "mag_dw",
            "db": "mag_db"}


def norm_ref64(x, r, w, b, dy, dh, eps, rms, hround=None):
    """Explicit fp64 forward and backward of y = norm(h) w (+ b), h = x (+ r),
    dx = d norm + dh, with every output's magnitude.  r / b / dh may be None.
    hround: round h to this dtype before the statistics and the backward (the
    model: what a kernel stores and reads back).  rstd, mean, dw, db come as
    [rows, 1] / [cols, 1]: one number per row / column."""
    x, w, dy = x.double(), w.double(), dy.double()
    h = x if r is None else x + r.double()
    mag_h = x.abs() if r is None else x.abs() + r.double().abs()
    if hround is not None and r is not None:
        h = rnd(h, hround)
    mean = torch.zeros_like(h[:, :1]) if rms else h.mean(-1, keepdim=True)
    hc = h - mean
    rstd = torch.rsqrt((hc * hc).mean(-1, keepdim=True) + eps)
    xh = hc * rstd
    axh = (h.abs() + mean.abs()) * rstd
    y, mag_y = xh * w, axh * w.abs()
    if b is not None:
        y, mag_y = y + b.double(), mag_y + b.double().abs()
    g = dy * w
    ag = g.abs()
    s1 = (g * xh).mean(-1, keepdim=True)
    a1 = (ag * axh).mean(-1, keepdim=True)
    s2 = 0.0 if rms else g.mean(-1, keepdim=True)
    a2 = 0.0 if rms else ag.mean(-1, keepdim=True)
    dx, mag_dx = (g - s2 - xh * s1) * rstd, (ag + a2 + axh * a1) * rstd
    if dh is not None:
        dx, mag_dx = dx + dh.double(), mag_dx + dh.double().abs()
    return NS(h=h, y=y, dx=dx, rstd=rstd, mean=mean, dw=(dy * xh).sum(0)[:, None], db=dy.sum(0)[:, None],
              mag_h=mag_h, mag_y=mag_y, mag_dx=mag_dx, mag_rstd=rstd, mag_mean=h.abs().mean(-1, keepdim=True),
              mag_dw=(dy.abs() * axh).sum(0)[:, None], mag_db=dy.abs().sum(0)[:, None])


def norm_model(x, r, w, b, dy, dh, eps, rms, dtype, wdtype=FP32):
    """norm_ref64 with a kernel's roundings: h to dtype before anything reads
    it, y and dx to dtype, rstd and mean to fp32, dw and db to wdtype."""
    m = norm_ref64(x, r, w, b, dy, dh, eps, rms, hround=dtype)
    return NS(h=m.h, y=rnd(m.y, dtype), dx=rnd(m.dx, dtype), rstd=rnd(m.rstd, FP32), mean=rnd(m.mean, FP32),
              dw=rnd(m.dw, wdtype), db=rnd(m.db, wdtype))


class NormCase:
    """Inputs, reference, model and what the outputs are called, for one
    (rows, cols, dtype, rms, res): computed once, read-only afterwards."""

    def __init__(self, rows, cols, dtype, rms, res, eps=1e-5, device="cpu", wdtype=FP32):
        self.rows, self.cols, self.dtype, self.rms, self.res, self.eps = rows, cols, dtype, rms, res, eps
        self.inp = i = norm_inputs(rows, cols, dtype, device=device)
        args = (i.x, i.r if res else None, i.w, None if rms else i.b, i.dy, i.dh if res else None, eps, rms)
        self.ref = norm_ref64(*args)
        self.model = norm_model(*args, dtype, wdtype)
        self.wdtype = wdtype
        if res:
            # h and y answer to the exact sum x + r (the model rounds h before the statistics).  The saved statistics
            # are those of the stored, rounded h, and the backward's input is that stored h: rstd, mean, dx, dw, db
            # answer to fp64 on the stored h's values, not to the unrounded sum (1 u of bf16 off in h)
            hr = norm_ref64(*args, hround=dtype)
            for n in ("rstd", "mean", "dx", "dw", "db"):
                setattr(self.ref, n, getattr(hr, n))
                setattr(self.ref, NORM_OUT[n], getattr(hr, NORM_OUT[n]))
        self.names = [n for n in NORM_OUT if not (n == "h" and not res) and not (n in ("mean", "db") and rms)]

    def n_dtype(self, name):
        """(longest fp32 sum, output dtype) of output `name`."""
        if name in ("dw", "db"):
            return self.rows, self.wdtype
        return self.cols, (FP32 if name in ("rstd", "mean") else self.dtype)

    def check(self, name, got, what=""):
        n, dt = self.n_dtype(name)
        got = got.reshape(getattr(self.ref, name).shape)
        return check_rows(what, name, got, getattr(self.ref, name), getattr(self.ref, NORM_OUT[name]),
                          getattr(self.model, name), n, dt)

    def ok(self, name, got):
        n, dt = self.n_dtype(name)
        return rows_ok(name, got.reshape(getattr(self.ref, name).shape), getattr(self.ref, name),
                       getattr(self.ref, NORM_OUT[name]), getattr(self.model, name), n, dt)


# ---------------------------------------------------------------------------
# RoPE: qkv [B S, (Hq + 2 Hkv) D] <-> q [B, Hq, S, D], k / v [B, Hkv rep, S, D]
# ---------------------------------------------------------------------------
def rope_inputs(B, S, Hq, Hkv, D, rep, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(1000 * seed + S + D + rep)
    H3 = Hq + 2 * Hkv
    qkv = torch.randn(B * S, H3 * D, generator=g).to(BF16)
    dq = torch.randn(B, Hq, S, D, generator=g).to(BF16)
    dk, dv = (torch.randn(B, Hkv * rep, S, D, generator=g).to(BF16) for _ in range(2))
    return tuple(t.to(device) for t in (qkv, dq, dk, dv))


def rope_ref64(qkv, dq, dk, dv, cos, sin, B, S, Hq, Hkv, D, rep):
    """fp64 forward (q, k, v) and backward (dqkv as [B, H3, S, D]: the
    replicas of dk / dv summed, dq / dk rotated back) with magnitudes."""
    H3 = Hq + 2 * Hkv
    c, s = cos.double(), sin.double()
    x = qkv.double().view(B, S, H3, D).transpose(1, 2)
    xq, xk, xv = x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]
    rot = lambda t: an.rope_back(t, c, -s)   # the forward rotation is the inverse one by -theta
    mag = lambda t: an.rope_mag(t.abs(), c, s)
    rp = lambda t: t.repeat_interleave(rep, 1)
    gsum = lambda t: t.double().view(B, Hkv, rep, S, D).sum(2)
    dks, dvs = gsum(dk), gsum(dv)
    mks, mvs = gsum(dk.double().abs()), gsum(dv.double().abs())
    return NS(q=rot(xq), k=rp(rot(xk)), v=rp(xv), mag_q=mag(xq), mag_k=rp(mag(xk)), mag_v=rp(xv.abs()),
              dqkv=torch.cat([an.rope_back(dq.double(), c, s), an.rope_back(dks, c, s), dvs], 1),
              mag_dqkv=torch.cat([mag(dq.double()), an.rope_mag(mks, c, s), mvs], 1))


# ---------------------------------------------------------------------------
# SwiGLU: gu [T, 2F] (gate | up) -> out = silu(gate) up
# ---------------------------------------------------------------------------
SWIGLU_SPECIAL = (20.0, -20.0, 90.0, -90.0)   # exp(-g) saturates (20) and overflows fp32 (-90)


def swiglu_inputs(T, F, seed=0, device="cpu"):
    """bf16 randn gu and dout; gate (t, t % F) of rows t = 0, 5, 10, ... is one
    of SWIGLU_SPECIAL in turn, so such a row keeps ordinary values next to it."""
    g = torch.Generator().manual_seed(1000 * seed + T + F)
    gu = torch.randn(T, 2 * F, generator=g).to(BF16)
    d = torch.randn(T, F, generator=g).to(BF16)
    rows = torch.arange(0, T, 5)
    gu[rows, rows % F] = torch.tensor(SWIGLU_SPECIAL, dtype=BF16)[(rows // 5) % 4]
    return gu.to(device), d.to(device)


def swiglu_ref64(gu, d):
    F = gu.shape[-1] // 2
    g, up, d = gu[:, :F].double(), gu[:, F:].double(), d.double()
    sg = torch.sigmoid(g)
    out = g * sg * up
    du = d * g * sg
    dg = d * up * sg * (1 + g * (1 - sg))
    return NS(out=out, du=du, dg=dg, mag_out=out.abs(), mag_du=du.abs(),
              mag_dg=(d * up).abs() * sg * (1 + g.abs() * (1 - sg)))


# ---------------------------------------------------------------------------
# cross entropy: loss and lse per row, dx = (softmax - onehot) grad_out / n_valid
# ---------------------------------------------------------------------------
def xent_inputs(V, dtype, rows=6, seed=0, device="cpu"):
    """logits 3 randn, and targets: the first column, the last, one in the
    unroll-2 kernel's remainder chunk (V = 8200: chunk 1024), an ignored row,
    two random ones."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    x = (3 * torch.randn(rows, V, generator=g)).to(dtype)
    t = torch.randint(0, V, (rows,), generator=g)
    t[0], t[1], t[2], t[3] = 0, V - 1, (8195 if V == 8200 else V // 2), -100
    return x.to(device), t.to(device)


def xent_ref64(x, t, grad_out=1.0, ignore_index=-100):
    """fp64 loss / lse per row ([rows, 1]) and gradient, with magnitudes; the
    gradient split into the softmax part (every column but the target) and the
    target entry ([rows, 1]), so the one-hot entry cannot hide the rest."""
    x = x.double()
    rows, V = x.shape
    valid = ((t != ignore_index) & (t >= 0) & (t < V))[:, None]
    tc = t.clamp(0, V - 1)[:, None]
    lse = torch.logsumexp(x, -1, keepdim=True)
    xt = x.gather(1, tc)
    p = torch.exp(x - lse)
    onehot = torch.zeros_like(x, dtype=torch.bool).scatter_(1, tc, True) & valid
    scale = grad_out / max(int(valid.sum()), 1)
    grad = (p - onehot.double()) * valid * scale
    mag = (p + onehot.double()) * valid * abs(scale)
    return NS(lse=lse, loss=torch.where(valid, lse - xt, torch.zeros_like(lse)), mag_lse=1 + lse.abs(),
              mag_loss=torch.where(valid, 1 + lse.abs() + xt.abs(), torch.zeros_like(lse)), p=p, onehot=onehot,
              valid=valid.squeeze(1), tc=tc, grad=grad, mag_grad=mag)


def xent_split(g, ref):
    """(softmax part: g with the target entries zeroed, target entries [rows, 1])."""
    g = g.double()
    return g.masked_fill(ref.onehot, 0.0), g.gather(1, ref.tc) * ref.onehot.any(1, keepdim=True)


def xent_check_grad(what, got, ref, dtype):
    """The gradient in two parts against the reference, rows with an ignored
    target exactly 0; the model is the reference rounded to dtype.  Returns
    (softmax part, target entry) row_err in units."""
    V = got.shape[1]
    assert bool((got[~ref.valid] == 0).all()), f"{what}: the gradient of an ignored row is not exactly 0"
    assert float(ref.lse.abs().max()) < 16, "CAPS rests on half an ulp of an fp32 lse below 16"
    model = rnd(ref.grad, dtype)
    (gs, gt), (rs, rt), (ms, mt), (as_, at) = (xent_split(z, ref) for z in (got, ref.grad, model, ref.mag_grad))
    return (check_rows(what, "dx softmax part", gs, rs, as_, ms, V, dtype),
            check_rows(what, "dx target entry", gt, rt, at, mt, V, dtype))


def xent_grad_ok(got, ref, dtype):
    V = got.shape[1]
    model = rnd(ref.grad, dtype)
    (gs, gt), (rs, rt), (ms, mt), (as_, at) = (xent_split(z, ref) for z in (got, ref.grad, model, ref.mag_grad))
    return (rows_ok("dx softmax part", gs, rs, as_, ms, V, dtype), rows_ok("dx target entry", gt, rt, at, mt, V, dtype))


# ---------------------------------------------------------------------------
# embedding backward: grad[idx[i]] += dy[i]
# ---------------------------------------------------------------------------
def embed_inputs(kind, dim, gdtype, seed=0, device="cpu"):
    """(base [V, dim] gdtype, idx [n], dy [n, dim] bf16).  kind: 'one' (n = 1),
    'run' (ids with repeats; the largest id five times, once at the last
    position, so its run ends the sorted list), 'distinct' (every id once)."""
    g = torch.Generator().manual_seed(1000 * seed + dim + len(kind))
    V = 24
    if kind == "one":
        idx = torch.tensor([5])
    elif kind == "run":
        idx = torch.randint(0, V - 1, (40,), generator=g)
        idx[[3, 11, 12, 30, 39]] = V - 1
        idx[15:24] = 2
    else:
        idx = torch.randperm(V, generator=g)[:17]
    base = torch.randn(V, dim, generator=g).to(gdtype)
    dy = torch.randn(idx.numel(), dim, generator=g).to(BF16)
    return base.to(device), idx.to(device), dy.to(device)


def embed_ref64(base, idx, dy):
    """fp64 base + the sum of each id's rows, the magnitude, the model (one
    rounding of old + sum to the gradient's dtype), and the longest run + 1."""
    b, d = base.double(), dy.double()
    ref = b.index_add(0, idx, d)
    return NS(grad=ref, mag=b.abs().index_add(0, idx, d.abs()), model=rnd(ref, base.dtype),
              n=int(torch.bincount(idx.cpu(), minlength=base.shape[0]).max()) + 1)
