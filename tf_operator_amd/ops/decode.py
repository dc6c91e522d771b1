"""KV-cache decoding ops: the cache, RoPE + append of one token per row, and
one query row per head against the cached keys.

HIP kernels: csrc/hip/decode.hip (``toa_decode_rope_append``,
``toa_attn_decode``: split over keys, fp32 partials, a merge kernel) and, for
T tokens per row at once (chunked prefill, continuation), csrc/hip/extend.hip
(``toa_extend_rope_append``, ``toa_attn_extend``: the same split on the MFMA);
RoPE + append and the merge are one kernel each for both
(csrc/hip/kv_cache.hip).  CPU tensors take a plain PyTorch reference (fp32
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
# keys per workgroup of toa_attn_decode.  Chosen for long caches: 4096 keys x 8 KV heads x 8 rows are 1024
# workgroups (4 per CU) of 128 KB of K + V each at head_dim 128
SPLIT_KEYS_DEFAULT = 256


GEMMS = ("tile", "skinny")   # what runs a decode step's projections (docs/kernels.md "Decoding")
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


def project(x, w, gemm="tile"):
    """x [B, K] w [N, K]^T of a decode step.  ``tile``: ops.linear.linear, the
    training GEMMs.  ``skinny``: ops.gemm.linear_skinny, except from
    TILE_KEEPS_FROM rows of W on where the assembly GEMM takes the operands
    (the head of a large vocabulary: the tile kernel measured faster there);
    operands the skinny check refuses (more than 16 rows, a non-bf16 GPU
    model) take the tile path and are counted (ops.gemm.fallbacks, warned
    once per shape)."""
    if gemm == "skinny":
        if w.shape[0] >= TILE_KEEPS_FROM and _gemm.asm_takes(x, w):
            return linear(x, w)   # the measured dispatch, not a fallback
        why = _gemm.skinny_refusal(x, w)
        if not why:
            return _gemm.linear_skinny(x, w)
        _gemm._fallback("decode", (x.shape[0], w.shape[0], x.shape[1]), "tile", why)
    return linear(x, w)


def mlp(x, wgu, wd, gemm="tile"):
    """The Llama MLP of a decode step, x [B, H] -> [B, H].  ``skinny``: the
    SwiGLU in the gate|up GEMM (ops.gemm.swiglu_skinny: one launch, no
    [B, 2F] round trip), then the down projection; refused operands as in
    :func:`project`."""
    if gemm == "skinny":
        why = _gemm.skinny_refusal(x, wgu, swiglu=True)
        if not why:
            return project(_gemm.swiglu_skinny(x, wgu), wd, gemm)
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
        self.layers, self.batch, self.kv_heads, self.capacity, self.head_dim = layers, batch, kv_heads, capacity, head_dim
        self.device, self.dtype = torch.device(device), dtype
        shape = (batch, kv_heads, capacity, head_dim)
        self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)]
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


def _check_cache(k_cache, v_cache, B, Hkv, D, like):
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dim() != 4 or t.shape[0] != B or t.shape[1] != Hkv or t.shape[3] != D:
            raise ValueError(f"{name} {tuple(t.shape)} is not [B={B}, Hkv={Hkv}, C, D={D}]")
        if t.dtype != like.dtype or t.device != like.device or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous {like.dtype} on {like.device}")
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} differ")


def _check_rows(name, t, B, device):
    if t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != device:
        raise ValueError(f"{name} must be an int32 [{B}] tensor on {device} (got {t.dtype} {tuple(t.shape)} on "
                         f"{t.device})")
    return t.contiguous()


def _need_bf16(fn, t):
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"HIP {fn} needs bf16 (got {t.dtype})")


def _check_rope(qkv, many, cos, sin, rows, k_cache, v_cache, Hq, Hkv, D):
    """The arguments of rope_append (qkv [B, W]) and, many, of rope_append_many
    (qkv [B, T, W]); rows: the int32 [B] tensors by name, returned contiguous."""
    _check_heads(Hq, Hkv, D)
    width = (Hq + 2 * Hkv) * D
    if qkv.dim() != 2 + many or (many and qkv.shape[1] < 1) or qkv.shape[-1] != width:
        raise ValueError(f"qkv {tuple(qkv.shape)} is not [B,{' T >= 1,' if many else ''} (Hq + 2 Hkv) D = {width}]")
    B = qkv.shape[0]
    _check_cache(k_cache, v_cache, B, Hkv, D, qkv)
    rows = [_check_rows(name, t, B, qkv.device) for name, t in rows.items()]
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != D // 2 or cos.dtype != torch.float32:
        raise ValueError(f"cos / sin {tuple(cos.shape)} {cos.dtype} are not fp32 [rows, D/2 = {D // 2}]")
    return rows


def _check_attn(q, many, k_cache, v_cache, rows, max_len, scale):
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
    _check_cache(k_cache, v_cache, B, Hkv, D, q)
    rows = [_check_rows(name, t, B, q.device) for name, t in rows.items()]
    max_len = C if max_len is None else int(max_len)
    if not 1 <= max_len <= C:
        raise ValueError(f"max_len {max_len} outside 1 .. capacity {C}")
    return rows, max_len, 1.0 / math.sqrt(D) if scale is None else float(scale)


def _rope_ref(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D):
    """The CPU reference of both rope-appends, qkv [B, T, W]; count None: T
    each.  A token that is not there (t >= count, a position outside the cache
    or the table) is skipped: nothing appended, a zero q row."""
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
        k_cache[b, :, s:s + n] = r[:, Hq:].transpose(0, 1)
        v_cache[b, :, s:s + n] = xb[:, Hq + Hkv:].transpose(0, 1)
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


def rope_append(qkv, cos, sin, pos, k_cache, v_cache, Hq, Hkv, D):
    """One token per row: qkv [B, (Hq + 2 Hkv) D] (the fused projection's
    output), cos / sin [rows, D/2] fp32 (ops.llm.rope_tables), pos int32 [B]
    on the device.  Rotates q and k at position pos[b] with the convention
    and the roundings of ops.llm.rope_qkv, returns q [B, Hq, D] and stores k
    and v into slot pos[b] of the caches [B, Hkv, C, D]; no other slot is
    written.  Positions are the caller's (KVCache.positions, which never
    leaves the cache): a position outside the cache or the table writes
    nothing to the caches and a zero q row, as in rope_append_many."""
    (pos,) = _check_rope(qkv, False, cos, sin, {"pos": pos}, k_cache, v_cache, Hq, Hkv, D)
    B, C = qkv.shape[0], k_cache.shape[2]
    if _lib.use_hip(qkv):
        _need_bf16("rope_append", qkv)
        qkv, cos, sin = qkv.contiguous(), cos.contiguous(), sin.contiguous()
        q = torch.empty(B, Hq, D, device=qkv.device, dtype=qkv.dtype)
        _lib.call("toa_decode_rope_append", _lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(pos), _lib.ptr(q),
                  _lib.ptr(k_cache), _lib.ptr(v_cache), B, Hq, Hkv, D, C, cos.shape[0], _lib.stream(qkv))
        return q
    return _rope_ref(qkv[:, None], cos, sin, pos, None, k_cache, v_cache, Hq, Hkv, D)[:, 0]


def decode_ws_floats(B, Hq, D, max_len, split_keys) -> int:
    """fp32 words of toa_attn_decode's workspace: per (row, head, split) D of
    unnormalised output, the running maximum and the normaliser."""
    return B * Hq * -(-max_len // split_keys) * (D + 2)


def attn_decode(q, k_cache, v_cache, lengths, scale=None, split_keys=None, max_len=None):
    """q [B, Hq, D] against the caches [B, Hkv, C, D]: row b attends keys
    0 .. lengths[b]-1 (int32 [B] on the device); returns O [B, Hq, D].

    On the GPU: toa_attn_decode, split_keys keys per workgroup (a power of
    two >= 64; None: SPLIT_KEYS_DEFAULT) and a merge kernel.  max_len: a
    host-side bound of the lengths (KVCache.max_len; None: the capacity) that
    sizes the grid -- nothing is read back from the device.  A row's result
    depends on that row's q, cache, length and split_keys only."""
    split = check_split_keys(split_keys)
    (lengths,), max_len, scale = _check_attn(q, False, k_cache, v_cache, {"lengths": lengths}, max_len, scale)
    B, Hq, D = q.shape
    Hkv, C = k_cache.shape[1], k_cache.shape[2]
    if _lib.use_hip(q):
        _need_bf16("attn_decode", q)
        q = q.contiguous()
        ws = torch.empty(decode_ws_floats(B, Hq, D, max_len, split), device=q.device, dtype=torch.float32)
        o = torch.empty_like(q)
        _lib.call("toa_attn_decode", _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(lengths),
                  _lib.ptr(ws), _lib.ptr(o), B, Hq, Hkv, C, D, max_len, split, scale, _lib.stream(q))
        return o
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


def rope_append_many(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D):
    """T tokens per row: qkv [B, T, (Hq + 2 Hkv) D], cos / sin [rows, D/2]
    fp32, start and count int32 [B] on the device (KVCache.extend).  Token t
    of row b sits at position start[b] + t if t < count[b]: q and k are
    rotated there with rope_append's expressions, k and v stored into that
    slot of the caches [B, Hkv, C, D]; returns q [B, T, Hq, D].  A token with
    t >= count[b], or whose position is outside the cache or the table, writes
    nothing to the caches and a zero q row."""
    start, count = _check_rope(qkv, True, cos, sin, {"start": start, "count": count}, k_cache, v_cache, Hq, Hkv, D)
    B, T = qkv.shape[:2]
    C = k_cache.shape[2]
    if _lib.use_hip(qkv):
        _need_bf16("rope_append_many", qkv)
        qkv, cos, sin = qkv.contiguous(), cos.contiguous(), sin.contiguous()
        q = torch.empty(B, T, Hq, D, device=qkv.device, dtype=qkv.dtype)
        _lib.call("toa_extend_rope_append", _lib.ptr(qkv), _lib.ptr(cos), _lib.ptr(sin), _lib.ptr(start),
                  _lib.ptr(count), _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), B, T, Hq, Hkv, D, C,
                  cos.shape[0], _lib.stream(qkv))
        return q
    return _rope_ref(qkv, cos, sin, start, count, k_cache, v_cache, Hq, Hkv, D)


def attn_extend(q, k_cache, v_cache, start, count, scale=None, split_keys=None, max_len=None, workspace=None):
    """q [B, T, Hq, D] against the caches [B, Hkv, C, D]: query (b, t, h),
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
                                                 scale)
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
        _lib.call("toa_attn_extend", _lib.ptr(q), _lib.ptr(k_cache), _lib.ptr(v_cache), _lib.ptr(start),
                  _lib.ptr(count), _lib.ptr(ws), _lib.ptr(o), B, T, Hq, Hkv, C, D, max_len, split, scale,
                  _lib.stream(q))
        return o
    return _attn_ref(q, k_cache, v_cache, start, count, max_len, scale)
