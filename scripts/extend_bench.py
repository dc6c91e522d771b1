#!/usr/bin/env python3
"""Time toa_attn_extend (csrc/hip/extend.hip) in the three places it is used.

(a) Small T: Hq 32, Hkv 8, D 128, B = 8 rows at length 4096, T in {1, 4, 8,
    16} new tokens per row.  One toa_attn_extend launch against T back-to-back
    toa_attn_decode launches and against a same-process device copy of the
    K + V bytes (extend reads them once, T decode steps read them T times).
(b) Prefill form: B = 1, 4096 tokens from an empty cache in chunks of 256, 512
    and 4096; the attention time summed over the chunks against the training
    causal_attention forward at S = 4096, B = 1, in the same process.
(c) Whole model: llama3-8b, random init, one prompt of 8192 tokens;
    torch.cuda.max_memory_allocated and the time of prefill(chunk=None)
    against prefill(chunk=512).

Method of scripts/decode_bench.py: device events around each sample, warm-up
first, the median (and range) over the samples, each sample a few back-to-back
repetitions so the host's launch cost does not sit between the events; one
process, one JSON line.

    python scripts/extend_bench.py [--parts a b c] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, warmup, iters, inner):
    """(median, min, max) ms per call of fn over `iters` samples of `inner` calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times), min(times), max(times)


def _us(t):
    med, lo, hi = t
    return {"median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2)}


def _randn(g, *shape):
    return torch.randn(*shape, device=g.device, generator=g).to(torch.bfloat16)


def part_a(a, dev):
    from tf_operator_amd.ops import decode

    B, Hq, Hkv, D, L = 8, 32, 8, 128, a.length
    g = torch.Generator(device=dev).manual_seed(0)
    kc, vc = _randn(g, B, Hkv, L, D), _randn(g, B, Hkv, L, D)
    n = torch.full((B,), L, dtype=torch.int32, device=dev)
    nbytes = 2 * kc.numel() * kc.element_size()
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    res = {"shape": {"B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "len": L}, "kv_bytes": nbytes,
           "copy": _us(_median_ms(lambda: dst.copy_(src), a.warmup, a.iters, 10)), "T": {}}
    q1 = _randn(g, B, Hq, D)
    for T in (1, 4, 8, 16):
        q = _randn(g, B, T, Hq, D)
        start = torch.full((B,), L - T, dtype=torch.int32, device=dev)
        count = torch.full((B,), T, dtype=torch.int32, device=dev)
        split = decode.extend_split(B, T, Hq, Hkv, L)

        def steps():
            for _ in range(T):
                decode.attn_decode(q1, kc, vc, n, max_len=L)

        row = {"extend_split_keys": split,
               "extend": _us(_median_ms(lambda: decode.attn_extend(q, kc, vc, start, count, max_len=L), a.warmup,
                                        a.iters, 10)),
               "decode_x_T": _us(_median_ms(steps, a.warmup, a.iters, max(1, 10 // T)))}
        row["extend_of_decode"] = round(row["extend"]["median_us"] / row["decode_x_T"]["median_us"], 3)
        row["extend_of_copy"] = round(row["extend"]["median_us"] / res["copy"]["median_us"], 3)
        res["T"][str(T)] = row
    res["copy_again"] = _us(_median_ms(lambda: dst.copy_(src), 2, a.iters, 10))
    return res


def part_b(a, dev):
    from tf_operator_amd.ops import decode
    from tf_operator_amd.ops.llm import causal_attention

    B, Hq, Hkv, D, L = 1, 32, 8, 128, a.length
    g = torch.Generator(device=dev).manual_seed(1)
    q = _randn(g, B, L, Hq, D)
    kc, vc = _randn(g, B, Hkv, L, D), _randn(g, B, Hkv, L, D)
    qh = q.transpose(1, 2).contiguous()   # [B, Hq, S, D], the training layout
    with torch.no_grad():
        train = _median_ms(lambda: causal_attention(qh, kc, vc, out_layout="bshd"), a.warmup, a.iters, 5)
    res = {"shape": {"B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "len": L}, "causal_attention": _us(train), "chunk": {}}
    for chunk in (256, 512, 4096):
        calls = []
        for c0 in range(0, L, chunk):
            T = min(chunk, L - c0)
            calls.append((q[:, c0:c0 + T].contiguous(), torch.full((B,), c0, dtype=torch.int32, device=dev),
                          torch.full((B,), T, dtype=torch.int32, device=dev), c0 + T))

        def sweep():
            for qc, st, n, ml in calls:
                decode.attn_extend(qc, kc, vc, st, n, max_len=ml)

        t = _median_ms(sweep, max(2, a.warmup // 3), a.iters, 2)
        row = _us(t)
        row["launches"] = len(calls)
        row["split_keys"] = sorted({decode.extend_split(B, c[0].shape[1], Hq, Hkv, c[3]) for c in calls})
        row["of_causal_attention"] = round(t[0] / train[0], 2)
        res["chunk"][str(chunk)] = row
    return res


def part_c(a, dev):
    from tf_operator_amd.models.llama import PRESETS, Llama

    P = a.prompt
    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    tokens = torch.randint(0, m.cfg.vocab_size, (1, P), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    cache = m.new_cache(1, P)
    torch.cuda.synchronize()
    res = {"model": "llama3-8b", "prompt": P, "resident_GiB": round(torch.cuda.memory_allocated(dev) / 2 ** 30, 2)}
    for name, chunk in (("chunk_512", 512), ("unchunked", None)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        try:
            t = _median_ms(lambda: m.prefill(tokens, cache, chunk=chunk), 1, 3, 1)
        except torch.OutOfMemoryError as e:   # the arm does not fit: say so
            res[name] = {"error": f"out of memory: {str(e)[:120]}"}
            continue
        res[name] = {"median_ms": round(t[0], 2), "min_ms": round(t[1], 2), "max_ms": round(t[2], 2),
                     "peak_GiB": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="*", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--len", type=int, default=4096, dest="length")
    ap.add_argument("--prompt", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("extend_bench needs a GPU: a CPU run says nothing about the kernel's rate")
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "iters": a.iters}
    for p, fn in (("a", part_a), ("b", part_b), ("c", part_c)):
        if p in a.parts:
            res[p] = fn(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
