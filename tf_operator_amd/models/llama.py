"""Llama-3 family decoder (random init, bf16) built on the fused HIP ops.

This is the BASELINE.json config-#3 model (TFJob Worker=8 all-reduce
Llama-3-8B bf16).  Per layer the forward is:

    (h, x) = add_rms_norm(h_prev, delta_prev)      HIP, residual add fused
    qkv    = x @ Wqkv^T                             hipBLASLt (fused Q|K|V weight)
    o      = rope_attention(qkv)                    HIP RoPE + head-major relayout, flash attention
                                                    (packed GQA); backward writes d(qkv) directly
    a      = o^T @ Wo^T                             hipBLASLt
    (h, x) = add_rms_norm(h, a)                     HIP
    gu     = x @ Wgu^T                              hipBLASLt (fused gate|up weight)
    delta  = swiglu(gu) @ Wd^T                      HIP SwiGLU, recomputed in bwd
final norm -> lm_head -> fused cross entropy (HIP, in-place logit gradient).

Every weight gradient is accumulated by the op straight into the flat
gradient buffer (``main_grad``), in backward order, so bucket all-reduces
start during backward.
"""
from __future__ import annotations

import dataclasses
import math

import torch

from ..ops.decode import KVCache, attn_decode, check_gemm, check_split_keys, rope_append
from ..ops import decode as _dec
from ..ops.embedding import Embedding
from ..ops.linear import linear
from ..ops.llm import (attention_block, causal_attention, cross_entropy, rope_cossin, rope_qkv, rope_tables, swiglu_mlp,
                       swiglu_mlp_resadd_ok)
from ..ops.norm import RMSNorm
from ..parallel.zero_check import reading


@dataclasses.dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    ffn: int = 14336
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    max_seq: int = 8192
    tie_embeddings: bool = False
    init_std: float = 0.02
    # "expand" materialises K/V per query head (kept for A/B runs); the HIP
    # flash-attention kernel (and the CPU reference) read packed GQA K/V directly.
    kv_layout: str = "auto"

    @property
    def head_dim(self):
        return self.hidden // self.heads

    def num_params(self):
        h, f, v, L = self.hidden, self.ffn, self.vocab_size, self.layers
        d = self.head_dim
        per_layer = h * (self.heads + 2 * self.kv_heads) * d + self.heads * d * h + 2 * f * h + f * h + 2 * h
        emb = v * h * (1 if self.tie_embeddings else 2)
        return L * per_layer + emb + h

    def flops_per_token(self, seq):
        """Training FLOPs/token (6N + causal attention 6*L*S*H... per Megatron)."""
        n = self.num_params() - self.vocab_size * self.hidden  # embedding lookup is not a GEMM
        attn = 6 * self.layers * seq * self.hidden  # 12*L*S*H/2 (causal)
        return 6 * n + attn


PRESETS = {
    "llama3-8b": LlamaConfig(),
    "llama3-1b": LlamaConfig(vocab_size=128256, hidden=2048, layers=16, heads=32, kv_heads=8, ffn=8192,
                             tie_embeddings=True),
    "llama-tiny": LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4, kv_heads=2, ffn=512, max_seq=512),
    # head_dim 128 like Llama-3-8B: the smoke model runs the same attention kernel as the flagship
    "llama-tiny128": LlamaConfig(vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, max_seq=1024),
}


# a block's second output when its down projection already added the residual (the next norm is presummed)
PRESUMMED = object()


class LlamaBlock(torch.nn.Module):
    def __init__(self, cfg: LlamaConfig, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        d = cfg.head_dim
        qkv_out = (cfg.heads + 2 * cfg.kv_heads) * d
        self.attn_norm = RMSNorm(cfg.hidden, cfg.norm_eps, dtype=dtype, device=device)
        self.wqkv = torch.nn.Parameter(torch.empty(qkv_out, cfg.hidden, dtype=dtype, device=device))
        self.wo = torch.nn.Parameter(torch.empty(cfg.hidden, cfg.heads * d, dtype=dtype, device=device))
        self.mlp_norm = RMSNorm(cfg.hidden, cfg.norm_eps, dtype=dtype, device=device)
        self.wgu = torch.nn.Parameter(torch.empty(2 * cfg.ffn, cfg.hidden, dtype=dtype, device=device))
        self.wd = torch.nn.Parameter(torch.empty(cfg.hidden, cfg.ffn, dtype=dtype, device=device))

    def params_backward_order(self):
        return [self.wd, self.wgu, self.mlp_norm.weight, self.wo, self.wqkv, self.attn_norm.weight]

    def forward(self, h, delta, cos, sin, B, S, cossin=None, doc=None):
        cfg = self.cfg
        if delta is None:
            x = self.attn_norm(h)
        elif delta is PRESUMMED:   # the previous block's down projection added the residual already
            h, x = self.attn_norm.presummed(h)
        else:
            h, x = self.attn_norm(h, delta)
        a, summed = attention_block(x, self.wqkv, self.wo, cos, sin, B, S, cfg.heads, cfg.kv_heads, cfg.head_dim,
                                    residual=h, kv_layout=cfg.kv_layout, cossin=cossin, doc=doc)
        # summed: the output projection's epilogue added the residual; the norm then reads the sum once
        h, x = self.mlp_norm.presummed(a) if summed else self.mlp_norm(h, a)
        if swiglu_mlp_resadd_ok(x, self.wd, h):
            # + the residual in the down projection's epilogue: the next norm reads the sum once
            return swiglu_mlp(x, self.wgu, self.wd, residual=h), PRESUMMED
        delta = swiglu_mlp(x, self.wgu, self.wd)  # SwiGLU in the GEMMs' epilogues under the asm GEMM policy
        return h, delta


class Llama(torch.nn.Module):
    def __init__(self, cfg: LlamaConfig, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.embed = Embedding(cfg.vocab_size, cfg.hidden, dtype=dtype, device=device)
        self.blocks = torch.nn.ModuleList([LlamaBlock(cfg, device, dtype) for _ in range(cfg.layers)])
        self.norm = RMSNorm(cfg.hidden, cfg.norm_eps, dtype=dtype, device=device)
        if not cfg.tie_embeddings:
            self.lm_head = torch.nn.Parameter(torch.empty(cfg.vocab_size, cfg.hidden, dtype=dtype, device=device))
        self._rope_cache = {}

    @torch.no_grad()
    def init_weights(self, seed=0):
        g = torch.Generator(device=self.embed.weight.device)
        g.manual_seed(seed)
        std = self.cfg.init_std
        out_std = std / math.sqrt(2 * self.cfg.layers)
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0)
            elif name.endswith("wo") or name.endswith("wd"):
                p.normal_(0.0, out_std, generator=g)
            else:
                p.normal_(0.0, std, generator=g)

    def head_weight(self):
        return self.embed.weight if self.cfg.tie_embeddings else self.lm_head

    def params_backward_order(self):
        ps = []
        if not self.cfg.tie_embeddings:
            ps.append(self.lm_head)
        ps.append(self.norm.weight)
        for b in reversed(self.blocks):
            ps.extend(b.params_backward_order())
        ps.append(self.embed.weight)
        return ps

    def no_decay(self, p):
        return p.dim() == 1

    def rope(self, S, device):
        """(cos, sin [S, D/2], cos | sin stacked [2, S, D/2]) fp32 of this
        model's rope_theta, built once per (S, device): the stacked copy is
        the table the fused QKV + RoPE GEMM reads."""
        key = (S, str(device))
        if key not in self._rope_cache:
            cos, sin = rope_tables(S, self.cfg.head_dim, self.cfg.rope_theta, device=device)
            self._rope_cache[key] = (cos, sin, rope_cossin(cos, sin))
        return self._rope_cache[key]

    def forward(self, tokens, targets=None, doc=None):
        """doc: the (doc_start, doc_end) pair of ops.llm.doc_bounds for these
        tokens; every block's attention then stays inside each document
        (RoPE positions stay the row's).  None: plain causal attention."""
        B, S = tokens.shape
        cos, sin, cossin = self.rope(S, tokens.device)
        h = self.embed(tokens).view(B * S, self.cfg.hidden)
        delta = None
        for blk in self.blocks:
            h, delta = blk(h, delta, cos, sin, B, S, cossin, doc)
        _, x = self.norm.presummed(h) if delta is PRESUMMED else self.norm(h, delta)
        head = self.head_weight()
        reading(head, "lm_head")   # waited for by the final norm's hook (train/llm.py _install_param_waits)
        logits = linear(x, head)
        if targets is None:
            return logits.view(B, S, -1)
        return cross_entropy(logits, targets.reshape(-1), inplace_grad=True)

    # ---- KV-cache decoding (ops/decode.py; docs/kernels.md "Decoding").  Additions: forward is as it was.
    def new_cache(self, batch, capacity, device=None, dtype=None):
        """An empty KVCache of this model's layers, KV heads and head dim."""
        w = self.embed.weight
        return KVCache(self.cfg.layers, batch, self.cfg.kv_heads, capacity, self.cfg.head_dim,
                       w.device if device is None else device, w.dtype if dtype is None else dtype)

    def _check_cache(self, cache, B):
        cfg = self.cfg
        if (cache.layers, cache.kv_heads, cache.head_dim) != (cfg.layers, cfg.kv_heads, cfg.head_dim):
            raise ValueError(f"KV cache of {cache.layers} layers x {cache.kv_heads} kv heads x head dim "
                             f"{cache.head_dim} for a model of {cfg.layers} x {cfg.kv_heads} x {cfg.head_dim}")
        if cache.batch != B:
            raise ValueError(f"KV cache of {cache.batch} rows for a batch of {B}")

    def _logits_of(self, h, delta, rows=None, gemm="tile"):
        """Final norm and head of the residual stream h (+ delta); rows: an index into the tokens;
        gemm: what runs the head GEMM (ops.decode.project)."""
        _, x = self.norm(h, delta)
        if rows is not None:
            x = x[rows]
        head = self.head_weight()
        reading(head, "lm_head")
        return _dec.project(x, head, gemm)

    def _cached_blocks(self, h, attend, gemm):
        """The blocks over the rows h [n, hidden] for prefill, extend and
        decode_step, projections by `gemm` (ops.decode.project / mlp; ``tile``
        is linear / swiglu_mlp).  attend(layer index, qkv [n, (Hq + 2 Hkv) D])
        rotates, fills the layer's cache and returns the attention output
        [n, Hq D].  Returns the residual stream and the last delta."""
        delta = None
        for i, blk in enumerate(self.blocks):
            if delta is None:
                x = blk.attn_norm(h)
            else:
                h, x = blk.attn_norm(h, delta)
            o = attend(i, _dec.project(x, blk.wqkv, gemm))
            h, x = blk.mlp_norm(h, _dec.project(o, blk.wo, gemm))
            delta = _dec.mlp(x, blk.wgu, blk.wd, gemm)
        return h, delta

    @torch.no_grad()
    def prefill(self, tokens, cache, lengths=None, gemm=None, chunk=None):
        """Run the prompts tokens [B, P] (ragged ones right-padded; lengths:
        host ints, default P each) through the training ops, copy every
        layer's rotated K and V into the cache and return the logits [B, V] of
        position lengths[b]-1.  Causality keeps the pads out of every valid
        position, and cache slots at or beyond lengths[b] are never read.
        gemm: as in decode_step; here only the head GEMM on the B last
        positions' rows changes.

        chunk=n >= 1: the prompts go through :meth:`extend` n tokens at a
        time instead (every projection by `gemm`), so the intermediates are
        those of B n rows, not B P; no pad is written into the cache (slots
        at or beyond lengths[b] stay as they were) and chunks in which no row
        has a token left are skipped."""
        cfg = self.cfg
        B, P = tokens.shape
        gemm = check_gemm(gemm)
        self._check_cache(cache, B)
        lengths = [P] * B if lengths is None else [int(n) for n in lengths]
        if len(lengths) != B or min(lengths) < 1 or max(lengths) > P:
            raise ValueError(f"prompt lengths {lengths} outside 1 .. {P} for a batch of {B}")
        if P > cache.capacity:
            raise ValueError(f"KV cache overflow: a prompt of {P} tokens exceeds the capacity {cache.capacity}")
        if chunk is not None:
            if not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1:
                raise ValueError(f"chunk must be an int >= 1, not {chunk!r}")
            cache.set_lengths([0] * B)
            logits = None
            for c0 in range(0, max(lengths), chunk):
                counts = [min(max(n - c0, 0), chunk) for n in lengths]
                lg = self.extend(tokens[:, c0:c0 + chunk], cache, counts, gemm=gemm)
                if logits is None:
                    logits = lg
                else:   # a row's logits come from the chunk that holds its last token
                    here = torch.tensor([n > 0 for n in counts], device=lg.device)
                    logits = torch.where(here[:, None], lg, logits)
            return logits
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        cos, sin, _ = self.rope(cache.capacity, tokens.device)
        cos, sin = cos[:P], sin[:P]

        def attend(i, qkv):
            q, k, v = rope_qkv(qkv, cos, sin, B, P, Hq, Hkv, D, 1)
            cache.k[i][:, :, :P] = k
            cache.v[i][:, :, :P] = v
            return causal_attention(q, k, v, out_layout="bshd").reshape(B * P, Hq * D)

        h, delta = self._cached_blocks(self.embed(tokens).view(B * P, cfg.hidden), attend, "tile")
        cache.set_lengths(lengths)
        last = torch.tensor([b * P + n - 1 for b, n in enumerate(lengths)], device=tokens.device)
        return self._logits_of(h, delta, last, gemm)

    @torch.no_grad()
    def extend(self, tokens, cache, counts=None, split_keys=None, gemm=None, logits="last"):
        """Append counts[b] (host ints >= 0, not all zero; default T each) of
        the tokens [B, T] to row b of the cache at its current length: T = 1
        on a filled cache is a decode step, T = P on an empty one a prefill,
        anything between a chunk of a prompt, a second turn, or drafted tokens
        to verify.  Embedding, norms and projections run on the B T rows
        (ops.decode.project / mlp by `gemm`, as in decode_step: the skinny
        GEMM applies by its own check when B T <= 16, refused operands take
        ``tile`` and are counted), RoPE + append and the attention are
        ops.decode.rope_append_many / attn_extend (split_keys: None is
        ops.decode.extend_split's choice).

        logits="last": [B, V] at each row's last new token; only those B rows
        go through the final norm and the head.  "all": [B, T, V].  The
        logits of a row with count 0, and under "all" those of positions
        t >= counts[b], are finite but meaningless.  No host synchronisation;
        past the cache's capacity it raises ValueError before any launch."""
        cfg = self.cfg
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError(f"tokens {tuple(tokens.shape)} is not [B, T >= 1]")
        B, T = tokens.shape
        gemm = check_gemm(gemm)
        self._check_cache(cache, B)
        if logits not in ("last", "all"):
            raise ValueError(f"logits={logits!r}: expected 'last' or 'all'")
        if split_keys is not None:
            _dec.check_extend_split(split_keys)
        counts = [T] * B if counts is None else [int(n) for n in counts]
        if len(counts) != B or max(counts) > T:
            raise ValueError(f"counts {counts} for tokens {tuple(tokens.shape)}: one per row, at most {T}")
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        start, count = cache.extend(counts)
        max_len = cache.max_len
        cos, sin, _ = self.rope(cache.capacity, tokens.device)

        def attend(i, qkv):
            q = _dec.rope_append_many(qkv.view(B, T, -1), cos, sin, start, count, cache.k[i], cache.v[i], Hq, Hkv, D)
            o = _dec.attn_extend(q, cache.k[i], cache.v[i], start, count, split_keys=split_keys, max_len=max_len)
            return o.view(B * T, Hq * D)

        h, delta = self._cached_blocks(self.embed(tokens).view(B * T, cfg.hidden), attend, gemm)
        if logits == "all":
            return self._logits_of(h, delta, gemm=gemm).view(B, T, -1)
        last = torch.tensor([b * T + max(n, 1) - 1 for b, n in enumerate(counts)], device=tokens.device)
        return self._logits_of(h[last], delta[last], gemm=gemm)

    @torch.no_grad()
    def decode_step(self, tokens, cache, split_keys=None, gemm=None):
        """One new token per row, tokens [B], against the cache: appends the
        token's rotated K and V at each row's length and returns the logits
        [B, V] of that position.  No host synchronisation; past the cache's
        capacity it raises ValueError before any launch.

        gemm: what runs the seven projections per layer and the head.
        ``tile``: the training GEMMs (ops.linear.linear, swiglu_mlp);
        ``skinny``: the weight-streaming GEMM for 1 to 16 rows (ops.gemm
        linear_skinny / swiglu_skinny), the tile path for operands it
        refuses; None: TOA_DECODE_GEMM, default ``tile``.  Anything else
        raises ValueError before a launch."""
        cfg = self.cfg
        (B,) = tokens.shape
        gemm = check_gemm(gemm)
        self._check_cache(cache, B)
        split_keys = check_split_keys(split_keys)
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        cos, sin, _ = self.rope(cache.capacity, tokens.device)
        cache.append()
        pos, lens, max_len = cache.positions, cache.lengths, cache.max_len

        def attend(i, qkv):
            q = rope_append(qkv, cos, sin, pos, cache.k[i], cache.v[i], Hq, Hkv, D)
            o = attn_decode(q, cache.k[i], cache.v[i], lens, split_keys=split_keys, max_len=max_len)
            return o.view(B, Hq * D)

        h, delta = self._cached_blocks(self.embed(tokens), attend, gemm)
        return self._logits_of(h, delta, gemm=gemm)
