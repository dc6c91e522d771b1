"""Sampling from a Llama model through the KV cache (models/llama.py prefill /
decode_step, ops/decode.py): one prefill over the prompts, then one decode
step per new token -- O(S) attention work per token instead of a full forward
over the growing sequence."""
from __future__ import annotations

import torch

from ..ops.decode import check_gemm


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
             capacity=None, split_keys=None, gemm=None, prefill_chunk=None):
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
    cache-extend kernels)."""
    if prompts.dim() != 2 or prompts.shape[1] < 1:
        raise ValueError(f"prompts {tuple(prompts.shape)} is not [B, P >= 1]")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens {max_new_tokens} < 1")
    if temperature < 0.0 or top_k < 0:
        raise ValueError(f"temperature {temperature} and top_k {top_k} must not be negative")
    B, P = prompts.shape
    dev = prompts.device
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
    if temperature != 0.0 and top_k != 1:
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
        tok = _pick(logits, temperature, top_k, gen).to(prompts.dtype)
        if eos_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad), tok)
            done = done | (tok == pad)
        out[rows, at + t] = tok
        if t + 1 < max_new_tokens:
            logits = model.decode_step(tok, cache, split_keys=split_keys, gemm=gemm)
    return out, at + max_new_tokens
