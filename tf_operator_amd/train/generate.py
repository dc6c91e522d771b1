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
             stream_ids=None):
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
    (Llama.decode_step; None: TOA_DECODE_GEMM, default ``tile``).
    prefill_chunk: Llama.prefill's chunk (None: the whole prompt at once
    through the training ops; n >= 1: n tokens at a time through the
    cache-extend kernels).

    sampler (None: TOA_SAMPLER, default ``torch``): ``torch`` is the path
    above.  ``device`` picks every token with ops.sample.sample_tokens: top_p
    and min_p join the filters, temperature, top_k, top_p and min_p may be
    [B] tensors (a row at temperature 0 is greedy), and the draw is a hash of
    (seed, stream_ids[b], the row's cache length) -- no generator exists, and
    a row's tokens do not depend on the rows around it.  stream_ids: int64
    [B], default arange(B)."""
    if prompts.dim() != 2 or prompts.shape[1] < 1:
        raise ValueError(f"prompts {tuple(prompts.shape)} is not [B, P >= 1]")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens {max_new_tokens} < 1")
    B, P = prompts.shape
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
    lengths = [P] * B if lengths is None else [int(n) for n in lengths]
    if len(lengths) != B or min(lengths) < 1 or max(lengths) > P:
        raise ValueError(f"prompt lengths {lengths} outside 1 .. {P} for a batch of {B}")
    need = max(P, max(lengths) + max_new_tokens - 1)   # the last new token is never appended
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
    cache = model.new_cache(B, capacity, device=dev)
    pad = 0 if eos_id is None else int(eos_id)
    out = torch.full((B, P + max_new_tokens), pad, device=dev, dtype=prompts.dtype)
    cols = torch.arange(P + max_new_tokens, device=dev)
    at = torch.tensor(lengths, device=dev)                  # where each row's next token goes
    out[:, :P] = torch.where(cols[None, :P] < at[:, None], prompts, out[:, :P])
    rows = torch.arange(B, device=dev)
    done = torch.zeros(B, device=dev, dtype=torch.bool)
    logits = model.prefill(prompts, cache, lengths, gemm=gemm, chunk=prefill_chunk)
    for t in range(max_new_tokens):
        if sampler == "torch":
            tok = _pick(logits, temperature, top_k, gen).to(prompts.dtype)
        elif greedy:
            tok = logits.argmax(-1).to(prompts.dtype)
        else:   # the cache's lengths: unique per row and step, on the device already
            tok = _sample.sample_tokens(logits, seed=seed, stream_ids=stream_ids, positions=cache.lengths,
                                        **rowp).to(prompts.dtype)
        if eos_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad), tok)
            done = done | (tok == pad)
        out[rows, at + t] = tok
        if t + 1 < max_new_tokens:
            logits = model.decode_step(tok, cache, split_keys=split_keys, gemm=gemm)
    return out, at + max_new_tokens
