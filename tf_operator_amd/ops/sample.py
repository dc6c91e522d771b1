"""Token sampling: temperature, top-k, top-p (nucleus) and min-p per row, with
a counter-hash draw, so a row's token is a pure function of (its logits, its
parameters, seed, its stream id, its position) -- not of the batch around it.

HIP kernel: csrc/hip/sample.hip (``toa_sample_tokens``, one workgroup per
row).  CPU tensors run the references below, which are the normative
definition (docs/kernels.md "Sampling"):

* :func:`draw_reference`     the 64-bit draw, in Python ints;
* :func:`weights_reference`  the float stage: each token's integer weight q;
* :func:`pick_reference`     the integer stage: filters and draw, pure ints.

Weights: with m the row maximum (NaN counts as -inf, -0 as +0), a token with
x == m weighs exactly 2^32, one with x == -inf weighs 0, every other one
q = min(rint(2^32 * exp2((x - m) * (log2e / T))), 2^32 - 1) in fp32.  A token
whose q is 0 -- below 2^-33 of the mode's probability -- is never drawn.  All
masses are exact integer sums of q.

Order: logit descending, index ascending among equal logits.  top-k keeps the
first k tokens of it; top-p the shortest prefix whose mass reaches
t = max(1, ceil(P * Z_k / 2^32)), P = floor(p * 2^32) and Z_k the top-k
prefix's mass; min-p the tokens with q >= ceil(min_p * 2^32).  The kept set is
their intersection.  The token is the first index whose cumulative kept mass,
in index order, exceeds r = (h64 * Z_kept) >> 64.
"""
from __future__ import annotations

import math

import torch

from . import _lib

MAX_VOCAB = 1 << 20
_U32 = 0xFFFFFFFF
_ONE = 1 << 32                      # the mode's weight
LOG2E = 1.44269504                  # rounded to fp32 where it is used
DRAW_CONSTANTS = (0x9E3779B9, 0x7F4A7C15)


def _mix32(h: int) -> int:
    """murmur3's finaliser (csrc/hip/optim.hip mix32) on a Python int."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _U32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _U32
    return h ^ (h >> 16)


def draw_reference(seed: int, stream: int, pos: int) -> int:
    """The 64-bit draw of (seed, stream id, position): two 32-bit chains of
    mix32 that differ in a constant, the first one the high half."""
    seed, stream, pos = int(seed) & _U32, int(stream) & 0xFFFFFFFFFFFFFFFF, int(pos) & _U32
    out = 0
    for c in DRAW_CONSTANTS:
        a = _mix32((seed + c) & _U32)
        b = _mix32(((stream >> 32) + a) & _U32)
        out = (out << 32) | _mix32(pos ^ _mix32((stream & _U32) ^ b))
    return out


def _canonical(logits: torch.Tensor) -> torch.Tensor:
    """fp32, NaN as -inf and -0 as +0."""
    x = logits.detach().to("cpu", torch.float32)
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    return x + 0.0


def order_keys(logits: torch.Tensor) -> torch.Tensor:
    """The order-preserving integer image of each logit (int64, in [0, 2^32)):
    a larger logit has a larger key, equal logits equal keys."""
    u = _canonical(logits).contiguous().view(torch.int32).to(torch.int64) & _U32
    return torch.where((u >> 31) != 0, ~u & _U32, u | 0x80000000)


def weights_reference(logits: torch.Tensor, T) -> torch.Tensor:
    """q of each token of one row [V] (or of rows [.., V] sharing T) as int64:
    2^32 at the maximum, else the fp32 expression of the module docstring."""
    x = _canonical(logits)
    m = x.max(-1, keepdim=True).values
    c = torch.tensor(LOG2E, dtype=torch.float32) / torch.as_tensor(T, dtype=torch.float32)
    w = torch.exp2((x - m) * c) * 4294967296.0
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)     # 0 * inf at the maximum, decided below
    sat = w >= 4294967296.0
    q = torch.where(sat, torch.zeros_like(w), torch.round(w)).to(torch.int64)
    q = torch.where(sat, torch.full_like(q, _U32), q)
    q = torch.where(x == float("-inf"), torch.zeros_like(q), q)
    return torch.where(x == m, torch.full_like(q, _ONE), q)


def pick_reference(order_keys, q, k: int, P: int, minq: int, h64: int) -> int:
    """The integer stage.  order_keys, q: per-token ints (q up to 2^32);
    k: top-k (0 or >= V: off); P = floor(top_p * 2^32) (>= 2^32: off);
    minq = ceil(min_p * 2^32) (0: off); h64: the draw.  Thresholds as the
    kernel finds them: a key and how many of its tokens, in index order, enter."""
    keys, q = [int(a) for a in order_keys], [int(a) for a in q]
    V = len(keys)
    ties: dict[int, list[int]] = {}
    for i, key in enumerate(keys):
        ties.setdefault(key, []).append(i)
    distinct = sorted(ties, reverse=True)
    k_on, p_on = 0 < k < V, P < _ONE
    kst, ntie, zk = None, 0, 0          # kst None: every token is in the prefix
    if k_on:
        rem = k
        for key in distinct:
            if rem <= len(ties[key]):
                break
            rem -= len(ties[key])
            zk += sum(q[i] for i in ties[key])
        kst, ntie = key, rem
        zk += sum(q[i] for i in ties[key][:rem])
    elif p_on:
        zk = sum(q)
    if p_on:
        rem = max(1, (P * zk + _ONE - 1) >> 32)
        for key in distinct:
            mass = sum(q[i] for i in ties[key])
            if rem <= mass:
                break
            rem -= mass
        kst, ntie, acc = key, 0, 0
        for i in ties[key]:
            ntie += 1
            acc += q[i]
            if acc >= rem:
                break
    last = V if kst is None else ties[kst][min(ntie, len(ties[kst])) - 1]
    kept = [(kst is None or keys[i] > kst or (keys[i] == kst and i <= last)) and min(q[i], _U32) >= minq
            for i in range(V)]
    z = sum(q[i] for i in range(V) if kept[i])
    r = (h64 * z) >> 64
    acc = 0
    for i in range(V):
        if kept[i]:
            acc += q[i]
            if acc > r:
                return i
    return ties[distinct[0]][0]


def filter_ints(top_p: float, min_p: float):
    """(P, minq) of fp32 top_p and min_p, as the kernel rounds them."""
    p32 = torch.tensor(float(top_p), dtype=torch.float32).item()
    m32 = torch.tensor(float(min_p), dtype=torch.float32).item()
    P = math.floor(max(p32, 0.0) * _ONE) if p32 < 1.0 else _ONE
    minq = 0 if not m32 > 0.0 else (math.ceil(m32 * _ONE) if m32 < 1.0 else _U32)
    return P, minq


def _sample_row_reference(row, T: float, k: int, top_p: float, min_p: float, seed: int, stream: int, pos: int):
    """One row on the CPU: (token, q saturated to 32 bits)."""
    keys, x = order_keys(row), _canonical(row)
    sat = torch.clamp(weights_reference(row, T), max=_U32)      # temperature 0: log2e / T is inf, the rest weighs 0
    if not bool(torch.isfinite(x).any()):
        return 0, sat
    if not T > 0.0:
        return int((keys == keys.max()).nonzero()[0]), sat
    P, minq = filter_ints(top_p, min_p)
    q = torch.where(keys == keys.max(), torch.full_like(sat, _ONE), sat)
    return pick_reference(keys.tolist(), q.tolist(), int(k), P, minq, draw_reference(seed, stream, pos)), sat


def _is_scalar(v) -> bool:
    return not isinstance(v, torch.Tensor) or v.dim() == 0


_CHECKS = {
    "temperature": (lambda v: v >= 0.0 and math.isfinite(v), "must be finite and not negative"),
    "top_k": (lambda v: v >= 0, "must not be negative"),
    "top_p": (lambda v: 0.0 < v <= 1.0, "must be in (0, 1]"),
    "min_p": (lambda v: 0.0 <= v < 1.0, "must be in [0, 1)"),
}


def row_parameter(name: str, v, B: int, device, dtype=None) -> torch.Tensor:
    """A sampling parameter as its per-row array on `device`: a Python scalar
    (or 0-d tensor) is broadcast, a [B] tensor taken.  Values that the host
    can see (scalars, CPU tensors) are checked against the parameter's range;
    a tensor already on a GPU is checked for shape, dtype and device only --
    nothing is read back."""
    dtype = dtype or (torch.int32 if name == "top_k" else torch.float32)
    ok, why = _CHECKS[name]
    device = torch.device(device)
    if _is_scalar(v):
        v = v.item() if isinstance(v, torch.Tensor) else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or (name == "top_k" and not isinstance(v, int)):
            raise ValueError(f"{name}={v!r}: expected a number or a [{B}] tensor")
        if not ok(v):
            raise ValueError(f"{name}={v!r} {why}")
        return torch.full((B,), v, dtype=dtype, device=device)
    if tuple(v.shape) != (B,):
        raise ValueError(f"{name} {tuple(v.shape)} is not [{B}]")
    if v.dtype.is_floating_point != dtype.is_floating_point or v.dtype == torch.bool:
        raise ValueError(f"{name} has dtype {v.dtype}: expected {dtype}")
    if v.device.type == "cpu":
        for e in v.tolist():
            if not ok(e):
                raise ValueError(f"{name}={e!r} {why}")
    elif v.device != device:
        raise ValueError(f"{name} is on {v.device}, the logits on {device}")
    return v.to(device=device, dtype=dtype).contiguous()


def _row_ints(name: str, v, B: int, device, dtype) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.dtype == torch.bool or tuple(v.shape) != (B,):
            raise ValueError(f"{name} must be an integer [{B}] tensor (got {v.dtype} {tuple(v.shape)})")
        if v.device.type != "cpu" and v.device != torch.device(device):
            raise ValueError(f"{name} is on {v.device}, the logits on {device}")
        return v.to(device=device, dtype=dtype).contiguous()
    if isinstance(v, int) and not isinstance(v, bool):
        return torch.full((B,), v, dtype=dtype, device=device)
    if isinstance(v, (list, tuple)) and len(v) == B and all(isinstance(e, int) for e in v):
        return torch.tensor(list(v), dtype=dtype, device=device)
    raise ValueError(f"{name}={v!r}: expected an int or {B} of them")


def sample_tokens(logits, *, temperature, top_k=0, top_p=1.0, min_p=0.0, seed=0, stream_ids=None, positions,
                  return_weights=False):
    """logits [B, V] (bf16 or fp32, unit stride along V) -> tokens int64 [B].

    temperature, top_k, top_p, min_p: a Python scalar or a [B] tensor each
    (row_parameter).  temperature 0: that row's argmax, lowest index among
    ties, filters ignored.  top_k 0, top_p 1 and min_p 0 turn a filter off.
    A row without a finite logit gives token 0.  stream_ids (int64 [B],
    default arange(B)) and positions (int32 [B], required) select the draw
    with `seed`: the same (logits, parameters, seed, stream id, position)
    give the same token in any batch, at any row, on any call.

    return_weights: also each token's q as int64 [B, V], saturated at
    2^32 - 1 (a token at the row maximum weighs 2^32 and shows as 2^32 - 1).
    ValueError for bad arguments, before any launch."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"logits must be a [B, V] tensor (got {getattr(logits, 'shape', type(logits))})")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"logits must be bf16 or fp32 (got {logits.dtype})")
    B, V = logits.shape
    if B < 1 or not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"logits {tuple(logits.shape)}: need B >= 1 and 1 <= V <= {MAX_VOCAB}")
    dev = logits.device
    seed = int(seed)
    if not 0 <= seed <= _U32:
        raise ValueError(f"seed {seed} outside 0 .. 2^32 - 1")
    T = row_parameter("temperature", temperature, B, dev)
    K = row_parameter("top_k", top_k, B, dev)
    Pp = row_parameter("top_p", top_p, B, dev)
    Mp = row_parameter("min_p", min_p, B, dev)
    sid = torch.arange(B, dtype=torch.int64, device=dev) if stream_ids is None else \
        _row_ints("stream_ids", stream_ids, B, dev, torch.int64)
    pos = _row_ints("positions", positions, B, dev, torch.int32)
    if _lib.use_hip(logits):
        if logits.stride(1) != 1 or logits.stride(0) < V:
            logits = logits.contiguous()
        tokens = torch.empty(B, dtype=torch.int64, device=dev)
        w = torch.empty(B, V, dtype=torch.int32, device=dev) if return_weights else None
        _lib.call("toa_sample_tokens", _lib.dtype_code(logits), _lib.ptr(logits), logits.stride(0), B, V, _lib.ptr(T),
                  _lib.ptr(K), _lib.ptr(Pp), _lib.ptr(Mp), _lib.ptr(sid), _lib.ptr(pos), seed, _lib.ptr(tokens),
                  _lib.ptr(w), _lib.stream(logits))
        return (tokens, w.to(torch.int64) & _U32) if return_weights else tokens
    rows = [_sample_row_reference(logits[b], t, k, p, mp, seed, s, n) for b, (t, k, p, mp, s, n) in
            enumerate(zip(T.tolist(), K.tolist(), Pp.tolist(), Mp.tolist(), sid.tolist(), pos.tolist()))]
    tokens = torch.tensor([r[0] for r in rows], dtype=torch.int64)
    return (tokens, torch.stack([r[1] for r in rows])) if return_weights else tokens
