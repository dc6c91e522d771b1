"""Per-row numerics of causal attention: an fp64 reference with magnitudes, a
model of a flash kernel's bf16 roundings, and a per-row error measure.

Why per row: row i of O averages i + 1 value rows, so its norm falls like
1 / sqrt(i + 1) and a whole-tensor ||a - b|| / ||b|| is dominated by the first
few dozen rows; the last rows of every head (and, mirrored, the last key rows
of dK / dV) can be wrong without moving it.  row_err measures every row (the
last dimension) on its own, against the magnitude of what was summed to make
it, so cancellation in the exact value (dK at S = 1 is exactly 0) does not
enter.

A plain helper module: no fixtures, imported by tests/test_attn_rows.py (CPU)
and tests/test_attn_rows_gpu.py.  Tensors are [B, H, S, D] (q, dO, O, dQ) and
[B, Hk, S, D] (k, v, dK, dV); lse is [B, H, S]; doc is the (doc_start,
doc_end) pair of ops.llm.doc_bounds (query i sees key j iff
doc_start[i] <= j <= i).
"""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -9            # half a bf16 ulp: the relative error of one rounding to bf16
FACTOR = 3.0             # a kernel may round in another place or order than the model
CAP = 8.0 * U            # worst-case sum of the roundings along the path (output, P, normaliser, dS, delta, inputs)
# per-output factors above 3, where a correct kernel needed one (docs/kernels.md, "Per-row attention tolerances")
FACTORS = {}


# (B, H, Hk, S, D, spike) of the GPU tests; tests/test_attn_rows.py checks the model at the same inputs.
# Ragged S (register-staged HIP forward, split backward): around the 64-key tile and the 256-row block, one row,
# a tail of 44; every S at both head dims, every head layout at least twice.
_LAYOUTS = ((1, 2, 2), (2, 4, 1), (1, 4, 2))
RAGGED_SHAPES = [(*_LAYOUTS[(i + j) % 3], S, D, False)
                 for j, D in enumerate((64, 128)) for i, S in enumerate((1, 63, 65, 255, 257, 300))]
RAGGED_SHAPES.append((1, 4, 2, 300, 128, True))
# S % 256 == 0 (LDS-DMA and assembly forwards, dS-through-HBM backward): one, two and three 256-row blocks (three:
# the odd count of the heaviest-first order), B Hk % 8 == 0 (the XCD-grouped order), one spike
BLOCK_SHAPES = [(B, H, Hk, S, D, False) for D in (128, 64)
                for B, H, Hk, S in ((1, 2, 2, 256), (2, 4, 1, 512), (1, 4, 2, 768), (2, 8, 4, 256))]
BLOCK_SHAPES.append((1, 4, 2, 512, 128, True))
ROPE_SHAPES = [(1, 4, 2, 256), (2, 8, 2, 512)]
DOC_BOUNDARIES = (1, 64, 255, 256, 257)


def make_inputs(B, H, Hk, S, D, spike=False, seed=0, device="cpu"):
    """bf16 randn q, k, v, dO from a CPU generator (the same values on every
    device).  spike: late keys x 6 and one key aligned with a query, so the
    running maximum moves late in the row (the deferred-rescale branch)."""
    g = torch.Generator().manual_seed(1000 * seed + S + D)
    q, k, v, do = (torch.randn(B, h, S, D, generator=g).to(torch.bfloat16) for h in (H, Hk, Hk, H))
    if spike:
        k[:, :, S // 2:] *= 6.0
        k[:, :, S - 37] = 4.0 * q[0, 0, S - 20]
    return tuple(t.to(device) for t in (q, k, v, do))


def doc_lengths(S, boundaries=DOC_BOUNDARIES):
    """Document lengths of a row with a boundary at each of `boundaries` below S."""
    cuts = [0] + [b for b in boundaries if b < S] + [S]
    return [b - a for a, b in zip(cuts, cuts[1:])]


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _mask(S, device, doc):
    """[1 or B, 1, S, S] bool: key j visible to query i."""
    i = torch.arange(S, device=device)
    m = (i[None, :] <= i[:, None])[None, None]
    if doc is not None:
        ds = doc[0].to(device=device, dtype=torch.int64)
        m = m & (i[None, None, None, :] >= ds[:, None, :, None])
    return m


def _expand(x, rep):
    return x.repeat_interleave(rep, 1) if rep > 1 else x


def _group_sum(x, Hk):
    B, H, S, D = x.shape
    return x.view(B, Hk, H // Hk, S, D).sum(2)


def _scores(q, k, v, do, scale, doc):
    q, k, v, do = (t.to(torch.float64) for t in (q, k, v, do))
    Hk = k.shape[1]
    rep = q.shape[1] // Hk
    ke, ve = _expand(k, rep), _expand(v, rep)
    s = torch.matmul(q, ke.transpose(-1, -2)) * scale
    s = s.masked_fill(~_mask(q.shape[2], q.device, doc), float("-inf"))
    return q, ke, ve, do, Hk, s


def attn_ref64(q, k, v, do, scale, doc=None):
    """Explicit fp64 forward and backward of causal attention (no autograd)
    on the inputs' values, with the magnitude of every output: the same
    contractions over absolute values.  dK / dV (and their magnitudes) are
    summed over the H / Hk query heads of a group."""
    q, ke, ve, do, Hk, s = _scores(q, k, v, do, scale, doc)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.matmul(p, ve)
    dp = torch.matmul(do, ve.transpose(-1, -2))
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
    mag_s = p * (dp.abs() + (do.abs() * o.abs()).sum(-1, keepdim=True))
    return SimpleNamespace(
        o=o, lse=lse,
        dq=scale * torch.matmul(ds, ke),
        dk=scale * _group_sum(torch.matmul(dst, q), Hk),
        dv=_group_sum(torch.matmul(pt, do), Hk),
        mag_o=torch.matmul(p, ve.abs()),
        mag_q=scale * torch.matmul(mag_s, ke.abs()),
        mag_k=scale * _group_sum(torch.matmul(mag_s.transpose(-1, -2), q.abs()), Hk),
        mag_v=_group_sum(torch.matmul(pt, do.abs()), Hk))


def bf16_model(q, k, v, do, scale, doc=None):
    """The same computation with the roundings a flash kernel makes, fp64
    otherwise: P relative to the row maximum rounded to bf16, the normaliser
    summed from the rounded P, O rounded to bf16, delta from the rounded O, P
    of the backward (relative to lse) rounded to bf16 where it is a matrix
    operand (dV), dS rounded to bf16, the outputs rounded to bf16.  A
    reference for how large honest rounding error is, not the code under
    test.  o / dq / dk / dv are the rounded outputs; *_raw are the values
    before that last rounding (what an epilogue that rotates them sees)."""
    q, ke, ve, do, Hk, s = _scores(q, k, v, do, scale, doc)
    m = s.max(-1, keepdim=True).values
    pr = _bf(torch.exp(s - m))
    l = pr.sum(-1, keepdim=True)
    o_raw = torch.matmul(pr, ve) / l
    o = _bf(o_raw)
    lse = (m + torch.log(l)).squeeze(-1)
    p = torch.exp(s - lse[..., None])
    dp = torch.matmul(do, ve.transpose(-1, -2))
    delta = (do * o).sum(-1, keepdim=True)
    ds = _bf(p * (dp - delta))
    dq_raw = scale * torch.matmul(ds, ke)
    dk_raw = scale * _group_sum(torch.matmul(ds.transpose(-1, -2), q), Hk)
    dv_raw = _group_sum(torch.matmul(_bf(p).transpose(-1, -2), do), Hk)
    return SimpleNamespace(o=o, lse=lse, dq=_bf(dq_raw), dk=_bf(dk_raw), dv=_bf(dv_raw),
                           o_raw=o_raw, dq_raw=dq_raw, dk_raw=dk_raw, dv_raw=dv_raw)


def row_err(got, ref, mag):
    """(max over rows of ||got_row - ref_row|| / ||mag_row||, index of that
    row); a row is the last dimension.  A row that is not finite counts as
    infinitely wrong."""
    d = (got.to(torch.float64) - ref.to(torch.float64)).norm(dim=-1)
    m = mag.to(torch.float64).norm(dim=-1)
    r = torch.where(m > 0, d / m, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    r = torch.nan_to_num(r, nan=float("inf"))
    i = int(r.flatten().argmax())
    return float(r.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))


def fp32_floor(S, D):
    """What fp32 accumulation can add that the model (fp64 between its bf16
    roundings) does not have: a worst-case 2^-24 per term of the longest
    contractions, S keys and D columns.  It is what is left of the bound
    where the model's own error is exactly 0: at S = 1 the model's O, dV and
    lse are exact and its dS is exactly 0, while a kernel's dP and delta are
    two fp32 sums that differ in their last bits.  2.7e-2 u at S = 768."""
    return (S + D) * 2.0 ** -24


def row_tol(model_err, S, D, name=None):
    """min(3 x the model's row_err on the same inputs, 8 u) (+ fp32_floor)."""
    return min(FACTORS.get(name, FACTOR) * model_err + fp32_floor(S, D), CAP)


def check_rows(what, name, got, ref, mag, model, S, D):
    """Assert row_err(got) <= row_tol(row_err(model)) against the same
    reference and magnitude; prints and returns row_err / u."""
    me = row_err(model, ref, mag)[0]
    tol = row_tol(me, S, D, name)
    e, row = row_err(got, ref, mag)
    print(f"rows {what} {name}: {e / U:.3f} u at {row} (model {me / U:.3f} u, limit {tol / U:.3f} u)")
    assert e <= tol, (f"{what} {name}: row {row} is off by {e / U:.2f} u of its magnitude, limit {tol / U:.2f} u "
                      f"(model {me / U:.2f} u)")
    return e / U


class Case:
    """Inputs, the fp64 reference, the bf16 model and the tolerances that
    follow from them; computed once, shared by the tests that use the inputs.
    The tensors kept are output-sized ([B, H, S, D]); the S x S intermediates
    are dropped."""

    NAMES = {"o": "mag_o", "dq": "mag_q", "dk": "mag_k", "dv": "mag_v"}

    def __init__(self, q, k, v, do, scale=None, doc=None):
        self.q, self.k, self.v, self.do, self.doc = q, k, v, do, doc
        self.S, self.D = q.shape[2], q.shape[3]
        self.scale = 1.0 / math.sqrt(self.D) if scale is None else scale
        self.ref = attn_ref64(q, k, v, do, self.scale, doc)
        self.model = bf16_model(q, k, v, do, self.scale, doc)
        self.model_err = {n: row_err(getattr(self.model, n), getattr(self.ref, n), getattr(self.ref, m))[0]
                          for n, m in self.NAMES.items()}
        self.tol = {n: row_tol(e, self.S, self.D, n) for n, e in self.model_err.items()}
        self.model_lse_dev = float((self.model.lse - self.ref.lse).abs().max())
        # lse is stored as fp32 and made of fp32 sums in the log2 domain: 16 fp32 ulps of it on top of the model's
        # deviation, which is exactly 0 at S = 1
        self.lse_tol = FACTOR * self.model_lse_dev + 2.0 ** -20 * max(1.0, float(self.ref.lse.abs().max()))

    def err(self, name, got):
        return row_err(got, getattr(self.ref, name), getattr(self.ref, self.NAMES[name]))

    def ok(self, name, got):
        return self.err(name, got)[0] <= self.tol[name]

    def check(self, name, got, what=""):
        """Assert the per-row bound for output `name`; prints and returns row_err / u."""
        e, row = self.err(name, got)
        print(f"rows {what} {name}: {e / U:.3f} u at {row} (model {self.model_err[name] / U:.3f} u, "
              f"limit {self.tol[name] / U:.3f} u)")
        assert e <= self.tol[name], (f"{what} {name}: row {row} is off by {e / U:.2f} u of its magnitude, limit "
                                     f"{self.tol[name] / U:.2f} u (model {self.model_err[name] / U:.2f} u)")
        return e / U

    def check_lse(self, got, what=""):
        d = (got.to(torch.float64) - self.ref.lse).abs()
        d = torch.nan_to_num(d, nan=float("inf"))
        i = int(d.flatten().argmax())
        row = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), d.shape))
        e = float(d.flatten()[i])
        print(f"rows {what} lse: {e:.3e} at {row} (model {self.model_lse_dev:.3e}, limit {self.lse_tol:.3e})")
        assert e <= self.lse_tol, f"{what} lse: row {row} deviates by {e:.3e}, limit {self.lse_tol:.3e}"
        return e


def rope_back(x, cos, sin):
    """The inverse rotation of ops.llm._rope_ref (rotation by -theta) in the
    dtype of x; cos / sin [S, D / 2], x [..., S, D]."""
    d2 = x.shape[-1] // 2
    x1, x2 = x[..., :d2], x[..., d2:]
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)


def rope_mag(mag, cos, sin):
    """The magnitude of a rotated row: mag rotated by |cos| + |sin|."""
    d2 = mag.shape[-1] // 2
    m1, m2 = mag[..., :d2], mag[..., d2:]
    c, s = cos.to(mag.dtype).abs(), sin.to(mag.dtype).abs()
    return torch.cat([m1 * c + m2 * s, m2 * c + m1 * s], -1)
