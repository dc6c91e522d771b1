"""Sampling from a Llama model through the KV cache (models/llama.py prefill /
decode_step, ops/decode.py): one prefill over the prompts, then one decode
step per new token -- O(S) attention work per token instead of a full forward
over the growing sequence."""
from __future__ import annotations

import os

import torch

from ..ops import sample as _sample
from ..ops.decode import check_gemm

SAMPLERS = ("torch", "device")   # what picks a token from the logits (docs/kernels.md "Sampling")
# what the blocks' projections read (docs/kernels.md "Decoding on fp8 weights", "Decoding on MXFP4 weights")
WEIGHTS = ("bf16", "fp8", "fp4")


def check_weights(weights):
    """weights (None: TOA_DECODE_WEIGHTS, default ``bf16``) as one of WEIGHTS
    or a snapshot (Llama.quantize_projections), else ValueError."""
    w = os.environ.get("TOA_DECODE_WEIGHTS", "bf16") if weights is None else weights
    if isinstance(w, str) and w not in WEIGHTS:
        raise ValueError(f"{'TOA_DECODE_WEIGHTS' if weights is None else 'weights'}={w!r}: expected one of {WEIGHTS} "
                         "or a snapshot")
    return w


KVS = ("bf16", "fp8")            # what the KV cache holds (docs/kernels.md "fp8 KV cache")


def check_kv(kv) -> str:
    """kv (None: TOA_DECODE_KV, default ``bf16``) as one of KVS, else ValueError."""
    k = os.environ.get("TOA_DECODE_KV", "bf16") if kv is None else kv
    if k not in KVS:
        raise ValueError(f"{'TOA_DECODE_KV' if kv is None else 'kv'}={k!r}: expected one of {KVS}")
    return k


def check_sampler(sampler) -> str:
    """sampler (None: TOA_SAMPLER, default ``torch``) as one of SAMPLERS, else ValueError."""
    s = os.environ.get("TOA_SAMPLER", "torch") if sampler is None else sampler
    if s not in SAMPLERS:
        raise ValueError(f"{'TOA_SAMPLER' if sampler is None else 'sampler'}={s!r}: expected one of {SAMPLERS}")
    return s


def _pick(logits, temperature, top_k, gen):
    """The next token of each row [B] from its logits [B, V]."""
    if temperature == 0.0 or top_k == 1:
        return logits.argmax(-1)
    x = logits.float() / temperature
    if top_k:
        kth = torch.topk(x, min(top_k, x.shape[-1]), dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    return torch.multinomial(torch.softmax(x, -1), 1, generator=gen).squeeze(1)


@torch.no_grad()
def generate(model, prompts, max_new_tokens, *, lengths=None, temperature=0.0, top_k=0, eos_id=None, seed=0,
             capacity=None, split_keys=None, gemm=None, prefill_chunk=None, top_p=1.0, min_p=0.0, sampler=None,
             stream_ids=None, weights=None, kv=None, samples=1):
    """prompts [B, P] token ids (ragged ones right-padded, lengths: host ints,
    default P each) -> (tokens [B, P + max_new_tokens], lengths int64 [B]):
    row b holds its prompt, then its max_new_tokens new tokens from position
    lengths[b] on, then padding (eos_id, or 0).

    Greedy at temperature 0 (or top_k 1); otherwise temperature / top-k
    sampling from a generator of its own seeded with `seed`: the process's
    RNG states are neither read nor advanced.  A row that has emitted eos_id
    keeps emitting it (a done mask on the device).  Nothing inside the loop
    synchronises with the host.  capacity: the KV cache's (default: P +
    max_new_tokens); too small a one raises ValueError before any launch.
    gemm: what runs the projections of the decode steps and the prefill's head
    (Llama.decode_step: ``tile``, ``skinny``, ``stream`` or ``wide``; None:
    TOA_DECODE_GEMM, default ``tile``).
    prefill_chunk: Llama.prefill's chunk (None: the whole prompt at once
    through the training ops; n >= 1: n tokens at a time through the
    cache-extend kernels).
    weights: ``bf16``, ``fp8``, ``fp4`` or a snapshot from
    Llama.quantize_projections (None: TOA_DECODE_WEIGHTS, default ``bf16``).
    ``fp8`` quantises the blocks' projections once at the start of this call
    -- so a trainer samples from its current weights -- and the decode steps
    and prefill chunks of up to 16 rows (``stream``: up to 64, ``wide``: up to
    128) read one byte per weight (Llama.decode_step weights=); it needs gemm
    ``skinny``, ``stream`` or ``wide``.  ``fp4`` is the same on MXFP4 weights:
    up to 16 rows read four bits per weight and a scale byte per 32, more rows
    the bf16 weights.
    kv: ``bf16`` or ``fp8`` (None: TOA_DECODE_KV, default ``bf16``): the KV
    cache in the model's dtype, or e4m3 keys and values with one power-of-two
    scale per token and KV head (Llama.new_cache(dtype=torch.float8_e4m3fn):
    half the cache's bytes and half of what a decode step streams from it).
    Independent of gemm and weights.

    sampler (None: TOA_SAMPLER, default ``torch``): ``torch`` is the path
    above.  ``device`` picks every token with ops.sample.sample_tokens: top_p
    and min_p join the filters, temperature, top_k, top_p and min_p may be
    [B] tensors (a row at temperature 0 is greedy), and the draw is a hash of
    (seed, stream_ids[b], the row's cache length) -- no generator exists, and
    a row's tokens do not depend on the rows around it.  stream_ids: int64
    [B], default arange(B).

    samples=n > 1: n completions per prompt on one copy of the prompt's keys
    and values (docs/kernels.md "Shared prompts").  The prompts [groups, P]
    are prefilled once into the prefix of an ops.decode.SharedKVCache, the
    logits repeated n times, and the steps decode groups x n rows; returns
    tokens [groups n, P + max_new_tokens], row g n + j sample j of prompt g,
    and their lengths -- the tokens of generate(prompts.repeat_interleave(n,
    0), ...) under the torch sampler.  Per-row parameters and stream_ids
    (default arange(groups n), so the samples draw differently) then have
    groups n rows; capacity sizes the suffixes (default max_new_tokens).
    kv="fp8" with samples > 1 raises ValueError."""
    if prompts.dim() != 2 or prompts.shape[1] < 1:
        raise ValueError(f"prompts {tuple(prompts.shape)} is not [B, P >= 1]")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens {max_new_tokens} < 1")
    if not isinstance(samples, int) or isinstance(samples, bool) or samples < 1:
        raise ValueError(f"samples {samples!r}: an int >= 1")
    groups, P = prompts.shape
    B = groups * samples
    dev = prompts.device
    sampler = check_sampler(sampler)
    if sampler == "device":
        # checked and made per-row arrays once; the steps pass them as they are
        rowp = {n: _sample.row_parameter(n, v, B, dev) for n, v in
                (("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("min_p", min_p))}
        stream_ids = torch.arange(B, device=dev) if stream_ids is None else \
            _sample._row_ints("stream_ids", stream_ids, B, dev, torch.int64)
        if not 0 <= int(seed) < 1 << 32:
            raise ValueError(f"seed {seed} outside 0 .. 2^32 - 1")
        greedy = not isinstance(temperature, torch.Tensor) and temperature == 0.0
        greedy = greedy or (not isinstance(top_k, torch.Tensor) and top_k == 1)
    else:
        if any(isinstance(v, torch.Tensor) for v in (temperature, top_k, top_p, min_p)) or stream_ids is not None:
            raise ValueError('per-row sampling parameters and stream_ids need sampler="device"')
        if top_p != 1.0 or min_p != 0.0:
            raise ValueError(f'top_p {top_p} / min_p {min_p}: these filters need sampler="device"')
        if temperature < 0.0 or top_k < 0:
            raise ValueError(f"temperature {temperature} and top_k {top_k} must not be negative")
        greedy = temperature == 0.0 or top_k == 1
    gemm = check_gemm(gemm)
    weights = check_weights(weights)
    kv = check_kv(kv)
    if samples > 1 and kv == "fp8":
        raise ValueError('samples > 1 needs kv="bf16": the shared-prompt kernels read a cache of the model\'s dtype')
    if weights in ("fp8", "fp4") and gemm == "tile":
        raise ValueError(f'weights="{weights}" needs gemm="skinny" or "stream": the tile GEMMs read the bf16 weights')
    lengths = [P] * groups if lengths is None else [int(n) for n in lengths]
    if len(lengths) != groups or min(lengths) < 1 or max(lengths) > P:
        raise ValueError(f"prompt lengths {lengths} outside 1 .. {P} for a batch of {groups}")
    need = max(P, max(lengths) + max_new_tokens - 1)   # the last new token is never appended
    if samples > 1:   # the suffixes hold the new tokens only
        need = max(max_new_tokens - 1, 1)
        capacity = max_new_tokens if capacity is None else int(capacity)
    else:
        capacity = P + max_new_tokens if capacity is None else int(capacity)
    if capacity < need:
        raise ValueError(f"KV cache overflow: capacity {capacity} < {need} slots for prompts of up to {max(lengths)} "
                         f"tokens (padded to {P}) + {max_new_tokens} new ones")
    if eos_id is not None and not 0 <= int(eos_id) < model.cfg.vocab_size:
        raise ValueError(f"eos_id {eos_id} is not a token id of a vocabulary of {model.cfg.vocab_size}")
    gen = None
    if sampler == "torch" and not greedy:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
    if isinstance(weights, str):
        weights = None if weights == "bf16" else model.quantize_projections(fmt=weights)
    if samples > 1:
        cache = model.new_shared_cache(groups, samples, P, capacity, device=dev)
        prompts, lengths = prompts.repeat_interleave(samples, 0), [n for n in lengths for _ in range(samples)]
    else:
        cache = model.new_cache(B, capacity, device=dev, dtype=torch.float8_e4m3fn if kv == "fp8" else None)
    pad = 0 if eos_id is None else int(eos_id)
    out = torch.full((B, P + max_new_tokens), pad, device=dev, dtype=prompts.dtype)
    cols = torch.arange(P + max_new_tokens, device=dev)
    at = torch.tensor(lengths, device=dev)                  # where each row's next token goes
    out[:, :P] = torch.where(cols[None, :P] < at[:, None], prompts, out[:, :P])
    rows = torch.arange(B, device=dev)
    done = torch.zeros(B, device=dev, dtype=torch.bool)
    if samples > 1:   # a row's length: its prompt's plus its suffix's
        plens = at.to(torch.int32)
        positions = lambda: plens + cache.suffix.lengths
    else:
        positions = lambda: cache.lengths
    if samples > 1:   # the prompts once, into the prefix; every sample starts from its prompt's logits
        logits = model.prefill(prompts[::samples], cache.prefix, lengths[::samples], gemm=gemm, chunk=prefill_chunk,
                               weights=weights).repeat_interleave(samples, 0)
    else:
        logits = model.prefill(prompts, cache, lengths, gemm=gemm, chunk=prefill_chunk, weights=weights)
    for t in range(max_new_tokens):
        if sampler == "torch":
            tok = _pick(logits, temperature, top_k, gen).to(prompts.dtype)
        elif greedy:
            tok = logits.argmax(-1).to(prompts.dtype)
        else:   # the cache's lengths: unique per row and step, on the device already
            tok = _sample.sample_tokens(logits, seed=seed, stream_ids=stream_ids, positions=positions(),
                                        **rowp).to(prompts.dtype)
        if eos_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad), tok)
            done = done | (tok == pad)
        out[rows, at + t] = tok
        if t + 1 < max_new_tokens:
            logits = model.decode_step(tok, cache, split_keys=split_keys, gemm=gemm, weights=weights)
    return out, at + max_new_tokens
