"""KV-cache decoding ops: the cache, RoPE + append of one token per row, and
one query row per head against the cached keys.

HIP kernels: csrc/hip/decode.hip (``toa_decode_rope_append``,
``toa_attn_decode``: split over keys, fp32 partials, a merge kernel) and, for
T tokens per row at once (chunked prefill, continuation), csrc/hip/extend.hip
(``toa_extend_rope_append``, ``toa_attn_extend``: the same split on the MFMA);
RoPE + append and the merge are one kernel each for both
(csrc/hip/kv_cache.hip); n samples per prompt on one copy of the prompt's keys
are csrc/hip/decode_shared.hip (SharedKVCache, ``toa_shared_rope_append``,
``toa_attn_decode_shared``).  CPU tensors take a plain PyTorch reference (fp32
math, the result in the tensor's dtype), row by row, so the CPU tier runs the
whole feature; decoding is its T = 1.

Cache layout: K and V are [B, Hkv, C, D] per layer, C the capacity, K stored
rotated.  Row b attends slots 0 .. len[b]-1; slots at or beyond len[b] are
never read into a result.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib
from . import gemm as _gemm
from .linear import linear
from .llm import swiglu_mlp

HEAD_DIMS = (64, 128)     # the kernels' head-dim instantiations (csrc/hip/decode.hip)
E4M3 = torch.float8_e4m3fn   # the fp8 KV cache's bytes (csrc/hip/kv_cache_q8.hip; docs/kernels.md "fp8 KV cache")
# keys per workgroup of toa_attn_decode.  Chosen for long caches: 4096 keys x 8 KV heads x 8 rows are 1024
# workgroups (4 per CU) of 128 KB of K + V each at head_dim 128
SPLIT_KEYS_DEFAULT = 256


GEMMS = ("tile", "skinny", "stream", "wide")   # what runs a decode step's projections (docs/kernels.md "Decoding")
# Under ``skinny``, a projection whose training GEMM already has a 256 x 256 tile per CU or more stays on it: at the
# Llama-3-8B head (128256 x 4096, 501 tiles) the tile kernel measured 6 to 48 % faster than the skinny one at 1, 8 and
# 16 rows on the same box; at the forms of 16 to 112 tiles it is 1.3 to 7.9 x slower (docs/kernels.md "Decoding").
TILE_KEEPS_FROM = 256 * 256   # rows of W


def check_gemm(gemm) -> str:
    """gemm (None: TOA_DECODE_GEMM, default ``tile``) as one of GEMMS, else ValueError."""
    g = os.environ.get("TOA_DECODE_GEMM", "tile") if gemm is None else gemm
    if g not in GEMMS:
        raise ValueError(f"{'TOA_DECODE_GEMM' if gemm is None else 'gemm'}={g!r}: expected one of {GEMMS}")
    return g


def _w8(x, pair, swiglu, gemm):
    """The fp8 kernel that serves these rows on the pair (q, scale) of a weights
    snapshot: "skinny" (1 to 16 rows), "stream" (17 to 64 rows under
    gemm="stream" or "wide"), "wide" (65 to 128 rows under gemm="wide") or ""
    for none.  One check is asked per projection, the one whose rows these are
    (ops.gemm.skinny_w8_refusal, stream_w8_refusal or wide_w8_refusal: the
    launcher's own).  Refused operands -- more than 128 rows, more than 64
    under gemm="stream", or more than 16 under gemm="skinny" -- are counted
    (ops.gemm.fallbacks, warned once per shape) and the caller goes on with
    the block's bf16 weight by `gemm`.  An MXFP4 pair (q uint8, scale uint8)
    has the one kernel "skinny_w4" for 1 to 16 rows under every
    weight-streaming `gemm`; more rows are counted as ``decode-fp4`` and run on
    the bf16 weight."""
    if pair is None:
        return ""
    if gemm == "tile":
        raise ValueError('a weights snapshot needs gemm="skinny" or "stream": the tile GEMMs read the bf16 weights')
    rows = x.shape[0] if x.dim() == 2 else 0
    if pair[0].dtype == torch.uint8:   # an MXFP4 pair (ops.gemm.quantize_w4): one kernel, for 1 to 16 rows
        why = _gemm.skinny_w4_refusal(x, pair[0], pair[1], swiglu)
        if why:
            _gemm._fallback("decode-fp4", (x.shape[0], pair[0].shape[0], x.shape[1]), f"bf16 {gemm}", why)
        return "" if why else "skinny_w4"
    kind = "wide" if gemm == "wide" and rows > 64 else "stream" if gemm in ("stream", "wide") and rows > 16 else "skinny"
    why = _W8_REFUSAL[kind](x, pair[0], pair[1], swiglu)
    if why:
        _gemm._fallback("decode-fp8", (x.shape[0], pair[0].shape[0], x.shape[1]), f"bf16 {gemm}", why)
    return "" if why else kind


# the fp8 kernels by the rows they serve: the launcher's check, the plain form, the SwiGLU form
_W8_REFUSAL = {"skinny": _gemm.skinny_w8_refusal, "stream": _gemm.stream_w8_refusal, "wide": _gemm.wide_w8_refusal}
_W8_LINEAR = {"skinny": _gemm.linear_skinny_w8, "stream": _gemm.linear_stream_w8, "wide": _gemm.linear_wide_w8,
              "skinny_w4": _gemm.linear_skinny_w4}
_W8_SWIGLU = {"skinny": _gemm.swiglu_skinny_w8, "stream": _gemm.swiglu_stream_w8, "wide": _gemm.swiglu_wide_w8,
              "skinny_w4": _gemm.swiglu_skinny_w4}


def project(x, w, gemm="tile", w8=None):
    """x [B, K] w [N, K]^T of a decode step.  ``tile``: ops.linear.linear, the
    training GEMMs.  ``skinny``: ops.gemm.linear_skinny, except from
    TILE_KEEPS_FROM rows of W on where the assembly GEMM takes the operands
    (the head of a large vocabulary: the tile kernel measured faster there);
    operands the skinny check refuses (more than 16 rows, a non-bf16 GPU
    model) take the tile path and are counted (ops.gemm.fallbacks, warned
    once per shape).  ``stream``: as ``skinny``, and operands of 17 to 64 rows
    take ops.gemm.linear_stream; only what both checks refuse takes the tile
    path and is counted.  ``wide``: as ``stream``, and operands of 65 to 128
    rows take ops.gemm.linear_wide; only what all three checks refuse takes
    the tile path and is counted.  w8: w's fp8 pair (q, scale) of a weights snapshot
    (Llama.quantize_projections); operands its check takes run on
    ops.gemm.linear_skinny_w8, at 17 to 64 rows under ``stream`` or ``wide``
    ops.gemm.linear_stream_w8, at 65 to 128 rows under ``wide``
    ops.gemm.linear_wide_w8, and w is not read; there is no fp8 kernel above
    128 rows (above 64 under ``stream``), so those rows are counted
    (``decode-fp8 ... -> bf16 wide``, ``-> bf16 stream``) and run on w.  An
    MXFP4 pair (fmt="fp4") runs on ops.gemm.linear_skinny_w4 at 1 to 16 rows;
    more rows are counted (``decode-fp4 ... -> bf16 <gemm>``) and run on w."""
    kind = _w8(x, w8, False, gemm)
    if kind:
        return _W8_LINEAR[kind](x, *w8, checked=True)
    if gemm != "tile":
        if w.shape[0] >= TILE_KEEPS_FROM and _gemm.asm_takes(x, w):
            return linear(x, w)   # the measured dispatch, not a fallback
        why = _gemm.skinny_refusal(x, w)
        if not why:
            return _gemm.linear_skinny(x, w)
        if gemm in ("stream", "wide"):
            why = _gemm.stream_refusal(x, w)
            if not why:
                return _gemm.linear_stream(x, w)
        if gemm == "wide":
            why = _gemm.wide_refusal(x, w)
            if not why:
                return _gemm.linear_wide(x, w)
        _gemm._fallback("decode", (x.shape[0], w.shape[0], x.shape[1]), "tile", why)
    return linear(x, w)


def mlp(x, wgu, wd, gemm="tile", w8gu=None, w8d=None):
    """The Llama MLP of a decode step, x [B, H] -> [B, H].  ``skinny``: the
    SwiGLU in the gate|up GEMM (ops.gemm.swiglu_skinny: one launch, no
    [B, 2F] round trip), then the down projection; refused operands as in
    :func:`project`.  ``stream``: the same, with ops.gemm.swiglu_stream for
    17 to 64 rows.  ``wide``: the same, with ops.gemm.swiglu_wide for 65 to
    128 rows.  w8gu, w8d: the fp8 pairs of wgu and wd, as in
    :func:`project` (ops.gemm.swiglu_skinny_w8, swiglu_stream_w8,
    swiglu_wide_w8)."""
    kind = _w8(x, w8gu, True, gemm)
    if kind:
        s = _W8_SWIGLU[kind](x, *w8gu, checked=True)
        return project(s, wd, gemm, w8d)
    if gemm != "tile":
        why = _gemm.skinny_refusal(x, wgu, swiglu=True)
        if not why:
            return project(_gemm.swiglu_skinny(x, wgu), wd, gemm, w8d)
        if gemm in ("stream", "wide"):
            why = _gemm.stream_refusal(x, wgu, swiglu=True)
            if not why:
                return project(_gemm.swiglu_stream(x, wgu), wd, gemm, w8d)
        if gemm == "wide":
            why = _gemm.wide_refusal(x, wgu, swiglu=True)
            if not why:
                return project(_gemm.swiglu_wide(x, wgu), wd, gemm, w8d)
        _gemm._fallback("decode", (x.shape[0], wgu.shape[0], x.shape[1]), "tile", why)
    return swiglu_mlp(x, wgu, wd)


def check_split_keys(split_keys) -> int:
    """split_keys (None: the default) as the launcher takes it: a power of two >= 64."""
    s = SPLIT_KEYS_DEFAULT if split_keys is None else split_keys
    if not isinstance(s, int) or isinstance(s, bool) or s < 64 or s & (s - 1):
        raise ValueError(f"split_keys must be a power of two >= 64, not {split_keys!r}")
    return s


def _check_heads(Hq, Hkv, D):
    if D not in HEAD_DIMS:
        raise ValueError(f"head_dim {D} not in {HEAD_DIMS}")
    if Hq < 1 or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"query heads {Hq} not a multiple of kv heads {Hkv}")


class KVCache:
    """K and V of every layer, [batch, kv_heads, capacity, head_dim] each, and
    the rows' lengths.  The lengths live on the host (they are known there:
    the prompt lengths, plus one per step) and are mirrored on the device for
    the kernels; ``append`` advances both without a synchronisation."""

    def __init__(self, layers, batch, kv_heads, capacity, head_dim, device, dtype=torch.bfloat16):
        if min(layers, batch, kv_heads, capacity) < 1:
            raise ValueError(f"KVCache needs positive sizes (layers {layers}, batch {batch}, kv_heads {kv_heads}, "
                             f"capacity {capacity})")
        if head_dim not in HEAD_DIMS:
            raise ValueError(f"head_dim {head_dim} not in {HEAD_DIMS}")
        if not (dtype.is_floating_point and (dtype.itemsize > 1 or dtype == E4M3)):
            raise ValueError(f"KVCache dtype {dtype}: a float type of 2 bytes or more, or {E4M3}")
        self.layers, self.batch, self.kv_heads, self.capacity, self.head_dim = layers, batch, kv_heads, capacity, head_dim
        self.device, self.dtype = torch.device(device), dtype
        shape = (batch, kv_heads, capacity, head_dim)
        self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)]
        # the fp8 cache: one power-of-two scale per (row, kv head, slot) beside the e4m3 bytes; None otherwise
        self.k_scale = self.v_scale = None
        if dtype == E4M3:
            self.k_scale = [torch.ones(shape[:3], device=device, dtype=torch.float32) for _ in range(layers)]
            self.v_scale = [torch.ones(shape[:3], device=device, dtype=torch.float32) for _ in range(layers)]
        self.host_lengths = [0] * batch
        # row 0: the last filled slot of each row (the position the newest token was appended at),
        # row 1: the lengths.  One tensor, so one in-place add advances both.
        self._state = torch.zeros(2, batch, device=device, dtype=torch.int32)
        self._state[0] -= 1

    @property
    def positions(self):
        """int32 [B] on the device: the slot of each row's newest token (len - 1)."""
        return self._state[0]

    @property
    def lengths(self):
        """int32 [B] on the device."""
        return self._state[1]

    @property
    def max_len(self) -> int:
        return max(self.host_lengths)

    def scales(self, layer) -> dict:
        """The k_scale= / v_scale= arguments of the ops for this layer: the fp8 cache's scales, else None."""
        if self.k_scale is None:
            return dict(k_scale=None, v_scale=None)
        return dict(k_scale=self.k_scale[layer], v_scale=self.v_scale[layer])

    def nbytes(self) -> int:
        """Bytes of the cache's tensors, the scales included."""
        ts = self.k + self.v + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in ts)

    def set_lengths(self, lengths):
        """The rows' lengths after a prefill (host ints); raises before anything is written."""
        lengths = [int(n) for n in lengths]
        if len(lengths) != self.batch:
            raise ValueError(f"{len(lengths)} lengths for a batch of {self.batch}")
        if min(lengths) < 0 or max(lengths) > self.capacity:
            raise ValueError(f"lengths {lengths} outside 0 .. capacity {self.capacity}")
        self.host_lengths = lengths
        n = torch.tensor(lengths, dtype=torch.int32)
        self._state.copy_(torch.stack([n - 1, n]))

    def append(self, n=1):
        """Every row grows by n slots.  Past the capacity: ValueError, before
        any launch and with nothing changed."""
        if n < 1:
            raise ValueError(f"append of {n} slots")
        if self.max_len + n > self.capacity:
            raise ValueError(f"KV cache overflow: length {self.max_len} + {n} exceeds the capacity {self.capacity}")
        self.host_lengths = [x + n for x in self.host_lengths]
        self._state += n

    def extend(self, counts):
        """Row b grows by counts[b] slots (host ints >= 0, not all zero).  Past
        the capacity: ValueError, before any launch and with nothing changed.
        Advances the host and the device lengths and returns (start, count),
        int32 [B] on the device, start the lengths before the call.  The device
        update is queued like set_lengths' copy; nothing waits for the device."""
        counts = [int(n) for n in counts]
        if len(counts) != self.batch:
            raise ValueError(f"{len(counts)} counts for a batch of {self.batch}")
        if min(counts) < 0 or max(counts) < 1:
            raise ValueError(f"extend by {counts}: counts must be >= 0 and not all zero")
        new = [a + n for a, n in zip(self.host_lengths, counts)]
        if max(new) > self.capacity:
            raise ValueError(f"KV cache overflow: lengths {self.host_lengths} + {counts} exceed the capacity "
                             f"{self.capacity}")
        sc = torch.tensor([self.host_lengths, counts], dtype=torch.int32).to(self.device)
        n = torch.tensor(new, dtype=torch.int32)
        self.host_lengths = new
        self._state.copy_(torch.stack([n - 1, n]))
        return sc[0], sc[1]


def _check_cache(k_cache, v_cache, B, Hkv, D, like, k_scale=None, v_scale=None):
    """The caches against the tensor they serve (`like`: qkv or q), and the
    pair of scales: required exactly when the caches are e4m3, fp32
    [B, Hkv, C] each.  Returns True for the fp8 cache."""
    q8 = k_cache.dtype == E4M3
    want = E4M3 if q8 else like.dtype
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dim() != 4 or t.shape[0] != B or t.shape[1] != Hkv or t.shape[3] != D:
            raise ValueError(f"{name} {tuple(t.shape)} is not [B={B}, Hkv={Hkv}, C, D={D}]")
        if t.dtype != want or t.device != like.device or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous {want} on {like.device}")
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} differ")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if not q8:
            if t is not None:
                raise ValueError(f"{name} given with {k_cache.dtype} caches: the scales belong to {E4M3} caches")
        elif t is None:
            raise ValueError(f"{E4M3} caches need k_scale and v_scale, fp32 {tuple(k_cache.shape[:3])}")
        elif (t.dtype != torch.float32 or t.shape != k_cache.shape[:3] or t.device != like.device
              or not t.is_contiguous()):
            raise ValueError(f"{name} must be contiguous fp32 {tuple(k_cache.shape[:3])} on {like.device} (got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device})")
    return q8


Q8_OPS = ("append", "fill", "decode", "extend")   # kv_cache_q8_shapes.h's enum Op, in its order


def _q8_call(name, args, op, k_cache, v_cache, k_scale, v_scale, B, T, Hq, Hkv, D, limit, split_keys=0):
    """Launcher `name` of the fp8 cache.  It refuses operands its check (kv_cache_q8_shapes.h) does not take before
    any launch; the same check, asked through toa_kv_q8_check only then, names the reason: ValueError in its words.
    A decode step is bound by the host's launches, so nothing is asked beforehand."""
    rc = _lib.call_ret(name, *args)
    if rc == _gemm.HIP_ERROR_INVALID_VALUE:
        r = _lib.call_ret("toa_kv_q8_check", Q8_OPS.index(op), _lib.ptr(k_cache), _lib.ptr(v_cache),
                          _lib.ptr(k_scale), _lib.ptr(v_scale), B, T, Hq, Hkv, D, k_cache.shape[2], limit, split_keys)
        raise ValueError(f"{name}: {_lib._fn('toa_kv_q8_why')(r).decode() if r else 'refused'}")
    if rc:
        raise RuntimeError(f"{name} failed with hipError {rc}")


def _quant_rows(x):
    """x [..., D] -> (e4m3 [..., D], fp32 [...]): ops.gemm's quantiser formula on every D-wide row."""
    q, scale = _gemm._quantize_ref(x.reshape(-1, x.shape[-1]))
    return q.view(x.shape), scale.view(x.shape[:-1])


def dequantize_cache(cache, scale, dtype=torch.bfloat16):
    """scale * e4m3 [B, Hkv, C, D] in `dtype`: exact in bf16 for the quantiser's power-of-two scales."""
    return (cache.float() * scale[..., None]).to(dtype)


def _check_rows(name, t, B, device):
    if t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != device:
        raise ValueError(f"{name} must be an int32 [{B}] tensor on {device} (got {t.dtype} {tuple(t.shape)} on "
                         f"{t.device})")
    return t.contiguous()


def _need_bf16(fn, t):
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"HIP {fn} needs bf16 (got {t.dtype})")


def _check_rope(qkv, many, cos, sin, rows, k_cache, v_cache, Hq, Hkv, D, k_scale=None, v_scale=None):
    """The arguments of rope_append (qkv [B, W]) and, many, of rope_append_many
    (qkv [B, T, W]); rows: the int32 [B] tensors by name, returned contiguous."""
    _check_heads(Hq, Hkv, D)
    width = (Hq + 2 * Hkv) * D
    if qkv.dim() != 2 + many or (many and qkv.shape[1] < 1) or qkv.shape[-1] != width:
        raise ValueError(f"qkv {tuple(qkv.shape)} is not [B,{' T >= 1,' if many else ''} (Hq + 2 Hkv) D = {width}]")
    B = qkv.shape[0]
    _check_cache(k_cache, v_cache, B, Hkv, D, qkv, k_scale, v_scale)
    rows = [_check_rows(name, t, B, qkv.device) for name, t in rows.items()]
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != D // 2 or cos.dtype != torch.float32:
        raise ValueError(f"cos / sin {tuple(cos.shape)} {cos.dtype} are not fp32 [rows, D/2 = {D // 2}]")
    return rows


def _check_attn(q, many, k_cache, v_cache, rows, max_len, scale, k_scale=None, v_scale=None):
    """The arguments of attn_decode (q [B, Hq, D]) and, many, of attn_extend
    (q [B, T, Hq, D]); rows as in _check_rope.  Returns (rows, max_len, scale)
    with the defaults filled in."""
    if q.dim() != 3 + many or (many and q.shape[1] < 1):
        raise ValueError(f"q {tuple(q.shape)} is not [B,{' T >= 1,' if many else ''} Hq, D]")
    B, Hq, D = q.shape[0], q.shape[-2], q.shape[-1]
    if k_cache.dim() != 4:
        raise ValueError(f"k_cache {tuple(k_cache.shape)} is not [B, Hkv, C, D]")
    Hkv, C = k_cache.shape[1], k_cache.shape[2]
    _check_heads(Hq, Hkv, D)
    _check_cache(k_cache, v_cache, B, Hkv, D, q, k_scale, v_scale)
    rows = [_check_rows(name, t, B, q.device) for name, t in rows.items()]
    max_len = C if max_len is None else int(max_len)
    if not 1 <= max_len <= C:
        raise ValueError(f"max_len {max_len} outside 1 .. capacity {C}")
    return rows, max_len, 1.0 / math.sqrt(D) if scale is None else float(scale)


def _put(cache, scale, b, s, n, rows):
    """rows [n, Hkv, D] into slots s .. s + n - 1 of row b; quantised where the cache has scales."""
    rows = rows.transpose(0, 1)
    if scale is None:
        cache[b, :, s:s + n] = rows
    else:
        cache[b, :, s:s + n], scale[b, :, s:s + n] = _quant_rows(rows)


def _rope_ref(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D, k_scale=None, v_scale=None):
    """The CPU reference of both rope-appends, qkv [B, T, W]; count None: T
    each.  A token that is not there (t >= count, a position outside the cache
    or the table) is skipped: nothing appended, a zero q row.  With scales the
    caches are e4m3: the rows the plain cache would hold, quantised."""
    B, T = qkv.shape[:2]
    C = k_cache.shape[2]
    q = torch.zeros(B, T, Hq, D, dtype=qkv.dtype)
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    d2 = D // 2
    for b, (s, n) in enumerate(zip(start.tolist(), [T] * B if count is None else count.tolist())):
        n = min(n, T, C - s, cos.shape[0] - s) if s >= 0 else 0
        if n < 1:
            continue
        xb = x[b, :n]
        x1, x2 = xb[:, :Hq + Hkv, :d2].float(), xb[:, :Hq + Hkv, d2:].float()
        c, sn = cos[s:s + n, None], sin[s:s + n, None]
        r = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn], -1).to(qkv.dtype)     # [n, Hq + Hkv, D]
        q[b, :n] = r[:, :Hq]
        _put(k_cache, k_scale, b, s, n, r[:, Hq:])
        _put(v_cache, v_scale, b, s, n, xb[:, Hq + Hkv:])
    return q


def _attn_ref(q, k_cache, v_cache, start, count, max_len, scale):
    """The CPU reference of both attentions, q [B, T, Hq, D]: token t < count[b]
    (None: T each) of row b attends keys 0 .. start[b] + t below max_len;
    zeros for a token that is not there."""
    B, T, Hq, D = q.shape
    C = k_cache.shape[2]
    rep = Hq // k_cache.shape[1]
    out = torch.zeros(B, T, Hq, D, dtype=q.dtype)
    for b, (s, cnt) in enumerate(zip(start.tolist(), [T] * B if count is None else count.tolist())):
        if s < 0:
            continue
        kb = k_cache[b].float().repeat_interleave(rep, 0)     # [Hq, C, D]
        vb = v_cache[b].float().repeat_interleave(rep, 0)
        for t in range(min(cnt, T, C - s)):
            n = min(s + t + 1, max_len)
            sc = torch.matmul(kb[:, :n], q[b, t].float()[:, :, None]).squeeze(-1) * scale
            out[b, t] = torch.matmul(torch.softmax(sc, -1)[:, None], vb[:, :n]).squeeze(1).to(q.dtype)
    return out


def rope_append(qkv, cos, sin, pos, k_cache, v_cache, Hq, Hkv, D, k_scale=None, v_scale=None):
    """k_scale, v_scale: fp32 [B, Hkv, C], required exactly when the caches
    are float8_e4m3fn (KVCache(dtype=torch.float8_e4m3fn)): the slot then
    holds the bf16 row quantised by ops.gemm.quantize_w8's rule and its scale
    (toa_decode_rope_append_q8); q is the same bits either way.

    One token per row: qkv [B, (Hq + 2 Hkv) D] (the fused projection's
    output), cos / sin [rows, D/2] fp32 (ops.llm.rope_tables), pos int32 [B]
    on the device.  Rotates q and k at position pos[b] with the convention
    and the roundings of ops.llm.rope_qkv, returns q [B, Hq, D] and stores k
    and v into slot pos[b] of the caches [B, Hkv, C, D]; no other slot is
    written.  Positions are the caller's (KVCache.positions, which never
    leaves the cache): a position outside the cache or the table writes
    nothing to the caches and a zero q row, as in rope_append_many."""
    (pos,) = _check_rope(qkv, False, cos, sin, {"pos": pos}, k_cache, v_cache, Hq, Hkv, D, k_scale, v_scale)
    B, C = qkv.shape[0], k_cache.shape[2]
    if _lib.use_hip(qkv):
        _need_bf16("rope_append", qkv)
        qkv, cos, sin = qkv.contiguous(), cos.contiguous(), sin.contiguous()
        q = torch.empty(B, Hq, D, device=qkv.device, dtype=qkv.dtype)
        if k_scale is not None:
            _q8_call("toa_decode_rope_append_q8",
                     (_lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(pos), _lib.ptr(q), _lib.ptr(k_cache),
                      _lib.ptr(v_cache), _lib.ptr(k_scale), _lib.ptr(v_scale), B, Hq, Hkv, D, C, cos.shape[0],
                      _lib.stream(qkv)), "append", k_cache, v_cache, k_scale, v_scale, B, 1, Hq, Hkv, D, cos.shape[0])
            return q
        _lib.call("toa_decode_rope_append", _lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(pos), _lib.ptr(q),
                  _lib.ptr(k_cache), _lib.ptr(v_cache), B, Hq, Hkv, D, C, cos.shape[0], _lib.stream(qkv))
        return q
    return _rope_ref(qkv[:, None], cos, sin, pos, None, k_cache, v_cache, Hq, Hkv, D, k_scale, v_scale)[:, 0]


def decode_ws_floats(B, Hq, D, max_len, split_keys) -> int:
    """fp32 words of toa_attn_decode's workspace: per (row, head, split) D of
    unnormalised output, the running maximum and the normaliser."""
    return B * Hq * -(-max_len // split_keys) * (D + 2)


def attn_decode(q, k_cache, v_cache, lengths, scale=None, split_keys=None, max_len=None, k_scale=None, v_scale=None):
    """q [B, Hq, D] against the caches [B, Hkv, C, D]: row b attends keys
    0 .. lengths[b]-1 (int32 [B] on the device); returns O [B, Hq, D].
    k_scale, v_scale: as in rope_append; on float8_e4m3fn caches the GPU runs
    toa_attn_decode_q8, which reads half the bytes and computes what the bf16
    kernel computes on the dequantised cache.

    On the GPU: toa_attn_decode, split_keys keys per workgroup (a power of
    two >= 64; None: SPLIT_KEYS_DEFAULT) and a merge kernel.  max_len: a
    host-side bound of the lengths (KVCache.max_len; None: the capacity) that
    sizes the grid -- nothing is read back from the device.  A row's result
    depends on that row's q, cache, length and split_keys only."""
    split = check_split_keys(split_keys)
    (lengths,), max_len, scale = _check_attn(q, False, k_cache, v_cache, {"lengths": lengths}, max_len, scale,
                                             k_scale, v_scale)
    B, Hq, D = q.shape
    Hkv, C = k_cache.shape[1], k_cache.shape[2]
    if _lib.use_hip(q):
        _need_bf16("attn_decode", q)
        q = q.contiguous()
        ws = torch.empty(decode_ws_floats(B, Hq, D, max_len, split), device=q.device, dtype=torch.float32)
        o = torch.empty_like(q)
        if k_scale is not None:
            _q8_call("toa_attn_decode_q8",
                     (_lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(k_scale), _lib.ptr(v_scale),
                      _lib.ptr(lengths), _lib.ptr(ws), _lib.ptr(o), B, Hq, Hkv, C, D, max_len, split, scale,
                      _lib.stream(q)), "decode", k_cache, v_cache, k_scale, v_scale, B, 1, Hq, Hkv, D, max_len, split)
            return o
        _lib.call("toa_attn_decode", _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(lengths),
                  _lib.ptr(ws), _lib.ptr(o), B, Hq, Hkv, C, D, max_len, split, scale, _lib.stream(q))
        return o
    if k_scale is not None:
        k_cache, v_cache = dequantize_cache(k_cache, k_scale, q.dtype), dequantize_cache(v_cache, v_scale, q.dtype)
    # one token per row at the last of its keys, the lengths cut to the cache as the kernel cuts them
    return _attn_ref(q[:, None], k_cache, v_cache, lengths.clamp(max=C) - 1, None, max_len, scale)[:, 0]


# ---- extending the cache by T tokens per row (csrc/hip/extend.hip; docs/kernels.md "Extending the cache")
EXTEND_QUERY_ROWS = 64    # query rows (token x head of a GQA group) per workgroup of toa_attn_extend
# Below this many workgroups the keys are split as well (SPLIT_KEYS_DEFAULT), from it on they are not: one
# workgroup per CU of an MI355X.  A guess: the crossover was not measured (docs/kernels.md "Extending the cache").
EXTEND_FILLS_FROM = 256


def check_extend_split(split_keys) -> int:
    """split_keys as toa_attn_extend takes it: 0 (one split over all keys) or a power of two >= 64."""
    s = split_keys
    if not isinstance(s, int) or isinstance(s, bool) or (s != 0 and (s < 64 or s & (s - 1))):
        raise ValueError(f"split_keys must be 0 or a power of two >= 64, not {split_keys!r}")
    return s


def extend_split(B, T, Hq, Hkv, max_len) -> int:
    """The default split_keys of attn_extend: SPLIT_KEYS_DEFAULT while the
    query tiles x KV heads x rows are fewer than EXTEND_FILLS_FROM workgroups,
    0 (no split) from there on."""
    tiles = -(-T * (Hq // Hkv) // EXTEND_QUERY_ROWS)
    return SPLIT_KEYS_DEFAULT if tiles * Hkv * B < EXTEND_FILLS_FROM else 0


def extend_ws_floats(B, T, Hq, D, max_len, split_keys) -> int:
    """fp32 words of toa_attn_extend's workspace: per (row, token, head, split)
    D of unnormalised output, the running maximum and the normaliser."""
    return B * T * Hq * (-(-max_len // split_keys) if split_keys else 1) * (D + 2)


def rope_append_many(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D, k_scale=None, v_scale=None):
    """k_scale, v_scale: as in rope_append (toa_extend_rope_append_q8).

    T tokens per row: qkv [B, T, (Hq + 2 Hkv) D], cos / sin [rows, D/2]
    fp32, start and count int32 [B] on the device (KVCache.extend).  Token t
    of row b sits at position start[b] + t if t < count[b]: q and k are
    rotated there with rope_append's expressions, k and v stored into that
    slot of the caches [B, Hkv, C, D]; returns q [B, T, Hq, D].  A token with
    t >= count[b], or whose position is outside the cache or the table, writes
    nothing to the caches and a zero q row."""
    start, count = _check_rope(qkv, True, cos, sin, {"start": start, "count": count}, k_cache, v_cache, Hq, Hkv, D,
                               k_scale, v_scale)
    B, T = qkv.shape[:2]
    C = k_cache.shape[2]
    if _lib.use_hip(qkv):
        _need_bf16("rope_append_many", qkv)
        qkv, cos, sin = qkv.contiguous(), cos.contiguous(), sin.contiguous()
        q = torch.empty(B, T, Hq, D, device=qkv.device, dtype=qkv.dtype)
        if k_scale is not None:
            _q8_call("toa_extend_rope_append_q8",
                     (_lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(start), _lib.ptr(count), _lib.ptr(q),
                      _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(k_scale), _lib.ptr(v_scale), B, T, Hq, Hkv, D, C,
                      cos.shape[0], _lib.stream(qkv)), "append", k_cache, v_cache, k_scale, v_scale, B, T, Hq, Hkv, D,
                     cos.shape[0])
            return q
        _lib.call("toa_extend_rope_append", _lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(start),
                  _lib.ptr(count), _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), B, T, Hq, Hkv, D, C,
                  cos.shape[0], _lib.stream(qkv))
        return q
    return _rope_ref(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D, k_scale, v_scale)


def fill_cache(k, v, k_cache, v_cache, k_scale, v_scale):
    """A whole prompt's rotated k and v [B, Hkv, P, D] into slots 0 .. P - 1
    of the fp8 cache [B, Hkv, C, D] and its scales [B, Hkv, C]: every D-wide
    row quantised as rope_append quantises it.  Slots at or beyond P are not
    touched.  On the GPU: toa_kv_quant_rows, one row per D / 8 lanes."""
    if k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
        raise ValueError(f"k {tuple(k.shape)} {k.dtype} and v {tuple(v.shape)} {v.dtype} are not one [B, Hkv, P, D]")
    B, Hkv, P, D = k.shape
    if D not in HEAD_DIMS:
        raise ValueError(f"head_dim {D} not in {HEAD_DIMS}")
    if not _check_cache(k_cache, v_cache, B, Hkv, D, k, k_scale, v_scale):
        raise ValueError(f"fill_cache fills {E4M3} caches, not {k_cache.dtype} (a plain cache takes a slice assignment)")
    if not 1 <= P <= k_cache.shape[2]:
        raise ValueError(f"KV cache overflow: {P} rows for a capacity of {k_cache.shape[2]}")
    if _lib.use_hip(k):
        _need_bf16("fill_cache", k)
        k, v = k.contiguous(), v.contiguous()
        _q8_call("toa_kv_quant_rows",
                 (_lib.ptr(k), _lib.ptr(v), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(k_scale), _lib.ptr(v_scale),
                  B, Hkv, P, D, k_cache.shape[2], _lib.stream(k)), "fill", k_cache, v_cache, k_scale, v_scale, B, P, 0,
                 Hkv, D, 0)
        return
    k_cache[:, :, :P], k_scale[:, :, :P] = _quant_rows(k)
    v_cache[:, :, :P], v_scale[:, :, :P] = _quant_rows(v)


def attn_extend(q, k_cache, v_cache, start, count, scale=None, split_keys=None, max_len=None, workspace=None,
                k_scale=None, v_scale=None):
    """k_scale, v_scale: as in rope_append; on float8_e4m3fn caches the GPU
    runs toa_attn_extend_q8, the same kernel with a staging that dequantises
    into the LDS image: bit for bit the result on the dequantised cache.

    q [B, T, Hq, D] against the caches [B, Hkv, C, D]: query (b, t, h),
    t < count[b], attends keys 0 .. start[b] + t of KV head h / (Hq / Hkv) --
    its own key is in the cache already, rope_append_many ran first; returns
    O [B, T, Hq, D], rows of zeros for tokens with t >= count[b].

    On the GPU: toa_attn_extend, both products on the MFMA, split_keys keys
    per workgroup (0: one split; a power of two >= 64; None: extend_split)
    and a merge kernel.  max_len: a host-side bound of start + count
    (KVCache.max_len; None: the capacity) that sizes the grid -- nothing is
    read back from the device.  workspace: fp32, at least extend_ws_floats
    words (None: torch.empty).  At a fixed split_keys a token's result
    depends on its q row, its cache row's keys 0 .. position, the position
    and split_keys only -- not on T, its index in the call, count, max_len or
    the batch."""
    (start, count), max_len, scale = _check_attn(q, True, k_cache, v_cache, {"start": start, "count": count}, max_len,
                                                 scale, k_scale, v_scale)
    B, T, Hq, D = q.shape
    Hkv, C = k_cache.shape[1], k_cache.shape[2]
    split = check_extend_split(extend_split(B, T, Hq, Hkv, max_len) if split_keys is None else split_keys)
    words = extend_ws_floats(B, T, Hq, D, max_len, split)
    if workspace is not None:
        if (workspace.dtype != torch.float32 or workspace.device != q.device or not workspace.is_contiguous()
                or workspace.numel() < words or workspace.data_ptr() % 16):
            raise ValueError(f"workspace must be a contiguous, 16-byte aligned fp32 tensor of at least {words} words "
                             f"on {q.device} (got {workspace.dtype} x {workspace.numel()} on {workspace.device})")
    if _lib.use_hip(q):
        _need_bf16("attn_extend", q)
        q = q.contiguous()
        ws = torch.empty(words, device=q.device, dtype=torch.float32) if workspace is None else workspace
        o = torch.empty_like(q)
        if k_scale is not None:
            _q8_call("toa_attn_extend_q8",
                     (_lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(k_scale), _lib.ptr(v_scale),
                      _lib.ptr(start), _lib.ptr(count), _lib.ptr(ws), _lib.ptr(o), B, T, Hq, Hkv, C, D, max_len, split,
                      scale, _lib.stream(q)), "extend", k_cache, v_cache, k_scale, v_scale, B, T, Hq, Hkv, D, max_len,
                     split)
            return o
        _lib.call("toa_attn_extend", _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(start),
                  _lib.ptr(count), _lib.ptr(ws), _lib.ptr(o), B, T, Hq, Hkv, C, D, max_len, split, scale,
                  _lib.stream(q))
        return o
    if k_scale is not None:
        k_cache, v_cache = dequantize_cache(k_cache, k_scale, q.dtype), dequantize_cache(v_cache, v_scale, q.dtype)
    return _attn_ref(q, k_cache, v_cache, start, count, max_len, scale)


# ---- n samples per prompt on one prefix cache (csrc/hip/decode_shared.hip; docs/kernels.md "Shared prompts")
class SharedKVCache:
    """The cache of `samples` completions per prompt: ``prefix``, a KVCache of
    `groups` rows (one per prompt, filled by Llama.prefill and read-only
    afterwards), and ``suffix``, a KVCache of groups x samples rows that holds
    only what was generated after the prompt; row g samples + j is sample j
    of prompt g.  A decode step reads each prompt's keys once for all its
    samples (ops.decode.attn_decode_shared).  The model's dtype only: the fp8
    cache (float8_e4m3fn) is refused."""

    def __init__(self, layers, groups, samples, kv_heads, prefix_capacity, capacity, head_dim, device,
                 dtype=torch.bfloat16):
        if dtype.itemsize < 2:
            raise ValueError(f"SharedKVCache dtype {dtype}: the shared-prompt kernels read a cache of the model's dtype, "
                             "not an fp8 one")
        if min(groups, samples) < 1:
            raise ValueError(f"SharedKVCache needs positive sizes (groups {groups}, samples {samples})")
        self.prefix = KVCache(layers, groups, kv_heads, prefix_capacity, head_dim, device, dtype)
        self.suffix = KVCache(layers, groups * samples, kv_heads, capacity, head_dim, device, dtype)
        self.layers, self.groups, self.samples, self.batch = layers, groups, samples, groups * samples
        self.kv_heads, self.head_dim, self.device, self.dtype = kv_heads, head_dim, self.prefix.device, dtype

    def append(self, n=1):
        """Every row's suffix grows by n slots; past its capacity: ValueError,
        before any launch and with nothing changed."""
        self.suffix.append(n)

    def nbytes(self) -> int:
        return self.prefix.nbytes() + self.suffix.nbytes()


def _shared_call(name, args, B, groups, samples, Hq, Hkv, D, Cp, Cs, max_plen=0, max_slen=0, split=64):
    """Launcher `name` of decode_shared.hip.  It refuses operands its check (decode_shared_shapes.h) does not take
    before any launch; the same check, asked only then, names the reason: ValueError in its words."""
    rc = _lib.call_ret(name, *args)
    if rc == _gemm.HIP_ERROR_INVALID_VALUE:
        r = _lib.call_ret("toa_decode_shared_check", B, groups, samples, Hq, Hkv, D, Cp, Cs, max_plen, max_slen, split)
        raise ValueError(f"{name}: {_lib._fn('toa_decode_shared_why')(r).decode() if r else 'refused'}")
    if rc:
        raise RuntimeError(f"{name} failed with hipError {rc}")


def _check_samples(samples, B):
    if not isinstance(samples, int) or isinstance(samples, bool) or samples < 1 or B % samples:
        raise ValueError(f"samples {samples!r}: a positive int that divides the {B} rows")
    return B // samples


def rope_append_shared(qkv, cos, sin, base, pos, k_cache, v_cache, samples, Hq, Hkv, D):
    """rope_append with the rotation and the slot apart: qkv [B, (Hq + 2 Hkv) D],
    B = groups x samples rows; base int32 [groups] (the prompts' lengths) and
    pos int32 [B] (the slots of the suffix cache), both on the device.  Row b
    rotates q and k at the absolute position base[b // samples] + pos[b] --
    the bits rope_append gives at that position -- returns q [B, Hq, D] and
    stores k and v into slot pos[b] of the suffix caches [B, Hkv, C, D]; no
    other slot is written.  A slot outside the cache or a position outside
    the table writes nothing to the caches and a zero q row."""
    (pos,) = _check_rope(qkv, False, cos, sin, {"pos": pos}, k_cache, v_cache, Hq, Hkv, D)
    B, C = qkv.shape[0], k_cache.shape[2]
    groups = _check_samples(samples, B)
    base = _check_rows("base", base, groups, qkv.device)
    if _lib.use_hip(qkv):
        _need_bf16("rope_append_shared", qkv)
        qkv, cos, sin = qkv.contiguous(), cos.contiguous(), sin.contiguous()
        q = torch.empty(B, Hq, D, device=qkv.device, dtype=qkv.dtype)
        _shared_call("toa_shared_rope_append",
                     (_lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(base), _lib.ptr(pos), _lib.ptr(q),
                      _lib.ptr(k_cache), _lib.ptr(v_cache), B, samples, Hq, Hkv, D, C, cos.shape[0], _lib.stream(qkv)),
                     B, groups, samples, Hq, Hkv, D, 1, C)
        return q
    # the plain reference at the absolute position, then the new rows moved to their slots: row by row, each on a
    # one-slot view, so nothing else of the cache is touched
    q = torch.zeros(B, 1, Hq, D, dtype=qkv.dtype)
    for b, (s, bs) in enumerate(zip(pos.tolist(), base.repeat_interleave(samples).tolist())):
        if not (0 <= s < C and bs >= 0 and bs + s < cos.shape[0]):
            continue
        one = torch.tensor([0], dtype=torch.int32)
        q[b] = _rope_ref(qkv[b:b + 1, None], cos[bs + s:bs + s + 1], sin[bs + s:bs + s + 1], one, None,
                         k_cache[b:b + 1, :, s:s + 1], v_cache[b:b + 1, :, s:s + 1], Hq, Hkv, D)[0]
    return q[:, 0]


def shared_ws_floats(B, Hq, D, max_plen, max_slen, split_keys) -> int:
    """fp32 words of toa_attn_decode_shared's workspace: per (row, head) the partials of the prefix's and of the
    suffix's splits, D + 2 words each."""
    return B * Hq * (-(-max_plen // split_keys) + -(-max_slen // split_keys)) * (D + 2)


def attn_decode_shared(q, prefix_k, prefix_v, prefix_lengths, k_cache, v_cache, lengths, samples, scale=None,
                       split_keys=None, max_prefix_len=None, max_len=None, workspace=None):
    """q [B, Hq, D], B = groups x samples, against the prompts' caches
    prefix_k / prefix_v [groups, Hkv, Cp, D] and the rows' own k_cache /
    v_cache [B, Hkv, Cs, D]: row b attends prefix keys
    0 .. prefix_lengths[b // samples] - 1 and then its suffix keys
    0 .. lengths[b] - 1 (int32 [groups] and [B] on the device) -- what
    attn_decode computes on a cache holding the concatenation; returns
    O [B, Hq, D].  An empty prefix or suffix contributes nothing; a row with
    neither is zeros.

    On the GPU: toa_attn_decode_shared.  The prefix runs on the MFMA, the
    samples x (Hq / Hkv) query rows of a prompt and KV head against its keys,
    split_keys keys per workgroup (a power of two >= 64; None:
    SPLIT_KEYS_DEFAULT), every K / V byte read once per prompt; the suffix
    runs attn_decode's kernel; one merge kernel.  max_prefix_len, max_len:
    host-side bounds of the two lengths (None: the capacities) that size the
    grids.  workspace: fp32, at least shared_ws_floats words (None:
    torch.empty).  A row's result depends on its q, its prefix, its suffix,
    the two lengths and split_keys only -- not on samples, its place in the
    group or the other rows."""
    split = check_split_keys(split_keys)
    (lengths,), max_len, scale = _check_attn(q, False, k_cache, v_cache, {"lengths": lengths}, max_len, scale)
    B, Hq, D = q.shape
    Hkv, Cs = k_cache.shape[1], k_cache.shape[2]
    groups = _check_samples(samples, B)
    if prefix_k.dim() != 4:
        raise ValueError(f"prefix_k {tuple(prefix_k.shape)} is not [groups, Hkv, Cp, D]")
    _check_cache(prefix_k, prefix_v, groups, Hkv, D, q)
    Cp = prefix_k.shape[2]
    plens = _check_rows("prefix_lengths", prefix_lengths, groups, q.device)
    max_plen = Cp if max_prefix_len is None else int(max_prefix_len)
    if not 0 <= max_plen <= Cp:
        raise ValueError(f"max_prefix_len {max_plen} outside 0 .. prefix capacity {Cp}")
    words = shared_ws_floats(B, Hq, D, max_plen, max_len, split)
    if workspace is not None:
        if (workspace.dtype != torch.float32 or workspace.device != q.device or not workspace.is_contiguous()
                or workspace.numel() < words or workspace.data_ptr() % 16):
            raise ValueError(f"workspace must be a contiguous, 16-byte aligned fp32 tensor of at least {words} words "
                             f"on {q.device} (got {workspace.dtype} x {workspace.numel()} on {workspace.device})")
    if _lib.use_hip(q):
        _need_bf16("attn_decode_shared", q)
        q = q.contiguous()
        ws = torch.empty(words, device=q.device, dtype=torch.float32) if workspace is None else workspace
        o = torch.empty_like(q)
        _shared_call("toa_attn_decode_shared",
                     (_lib.ptr(q), _lib.ptr(prefix_k), _lib.ptr(prefix_v), _lib.ptr(plens), _lib.ptr(k_cache),
                      _lib.ptr(v_cache), _lib.ptr(lengths), _lib.ptr(ws), _lib.ptr(o), B, groups, samples, Hq, Hkv, Cp,
                      Cs, D, max_plen, max_len, split, scale, _lib.stream(q)),
                     B, groups, samples, Hq, Hkv, D, Cp, Cs, max_plen, max_len, split)
        return o
    # row by row on the concatenation of its prefix and its suffix: attn_decode's reference on that cache
    out = torch.zeros_like(q)
    pl = plens.clamp(0, max_plen).tolist()
    for b, n in enumerate(lengths.clamp(0, max_len).tolist()):
        p = pl[b // samples]
        if p + n < 1:
            continue
        k = torch.cat([prefix_k[b // samples, :, :p], k_cache[b, :, :n]], 1)[None]
        v = torch.cat([prefix_v[b // samples, :, :p], v_cache[b, :, :n]], 1)[None]
        last = torch.tensor([p + n - 1], dtype=torch.int32)
        out[b] = _attn_ref(q[b:b + 1, None], k, v, last, None, p + n, scale)[0, 0]
    return out
