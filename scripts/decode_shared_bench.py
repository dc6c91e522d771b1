#!/usr/bin/env python3
"""Time shared-prompt decoding (ops.decode.attn_decode_shared, Llama.decode_step
on a SharedKVCache, generate(samples=n)) against the plain path on the prompt
repeated n times.  scripts/decode_bench.py's method: device events around
samples of 10 back-to-back launches, warm-up first, median and min to max; one
process; one JSON line per arm.

  kernel  one prompt x n samples, Hq 32, Hkv 8, D 128, suffix 64: attn_decode_shared
          against attn_decode on a plain cache of the same total lengths, and a
          device copy of the bytes each of them reads.  Every launch takes the next
          of enough distinct copies of its operands (a GiB of them) that it does
          not re-read what a recent launch left in the 256 MB Infinity Cache.
  step    decode_step of --preset at n rows, gemm="skinny": shared against plain,
          ABBA, 8 rounds of 16 steps from the same lengths; mean +- standard error
          of the difference per step.
  call    generate(16 new tokens) on one prompt, samples=n against the prompt
          repeated: whole-call time and the cache's bytes.

    python scripts/decode_shared_bench.py kernel --prefix 4096 16384
    python scripts/decode_shared_bench.py step call --prefix 4096
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INNER = 10    # launches per timed sample, back to back
ROTATE = 1 << 30   # bytes of distinct operands a launch's successors run through before it is read again


def _samples_ms(fn, warmup, iters):
    """(median, min, max) ms per launch over `iters` samples of INNER launches each; fn(i) is launch i."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    times, k = [], warmup
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn(k)
            k += 1
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / INNER)
    return statistics.median(times), min(times), max(times)


def _us(t, nbytes=None):
    r = {"median_us": round(t[0] * 1e3, 2), "min_us": round(t[1] * 1e3, 2), "max_us": round(t[2] * 1e3, 2)}
    if nbytes:
        r["read_GBps"] = round(nbytes / t[0] / 1e6, 1)
    return r


def _rand(*shape, dev):
    return torch.randn(*shape, device=dev).to(torch.bfloat16)


def kernel_arm(a, dev, prefix):
    from tf_operator_amd.ops import decode

    n, Hq, Hkv, D, S = a.samples, 32, 8, 128, a.suffix
    row = 2 * Hkv * D * 2                              # bytes of K + V per key and cache row
    shared_bytes, plain_bytes = row * (prefix + n * S), row * n * (prefix + S)
    copies_s, copies_p = max(3, -(-ROTATE // shared_bytes)), max(3, -(-ROTATE // plain_bytes))
    q = _rand(n, Hq, D, dev=dev)
    pk = [(_rand(1, Hkv, prefix, D, dev=dev), _rand(1, Hkv, prefix, D, dev=dev)) for _ in range(copies_s)]
    sk = [(_rand(n, Hkv, S, D, dev=dev), _rand(n, Hkv, S, D, dev=dev)) for _ in range(copies_s)]
    plain = [(_rand(n, Hkv, prefix + S, D, dev=dev), _rand(n, Hkv, prefix + S, D, dev=dev)) for _ in range(copies_p)]
    plen = torch.full((1,), prefix, dtype=torch.int32, device=dev)
    slen = torch.full((n,), S, dtype=torch.int32, device=dev)
    tlen = torch.full((n,), prefix + S, dtype=torch.int32, device=dev)
    ws = torch.empty(decode.shared_ws_floats(n, Hq, D, prefix, S, a.split_keys), dtype=torch.float32, device=dev)

    def shared(i):
        (k, v), (k2, v2) = pk[i % copies_s], sk[i % copies_s]
        return decode.attn_decode_shared(q, k, v, plen, k2, v2, slen, n, split_keys=a.split_keys, max_prefix_len=prefix,
                                         max_len=S, workspace=ws)

    def plain_fn(i):
        k, v = plain[i % copies_p]
        return decode.attn_decode(q, k, v, tlen, split_keys=a.split_keys, max_len=prefix + S)

    # the same query rows on the same keys: the two arms agree to bf16 rounding before either is timed
    plain[0][0][:, :, :prefix], plain[0][1][:, :, :prefix] = pk[0][0], pk[0][1]
    plain[0][0][:, :, prefix:], plain[0][1][:, :, prefix:] = sk[0][0], sk[0][1]
    dev_max = float((shared(0).float() - plain_fn(0).float()).abs().max())
    assert dev_max < 2.0 ** -6, dev_max
    dst = torch.empty(plain_bytes, dtype=torch.uint8, device=dev)

    def copy_of(copies, nbytes):   # a device copy of the bytes of one launch's operands, rotating like the launches
        flat = [torch.cat([t.view(torch.uint8).flatten() for t in c]) for c in copies]
        return lambda i: dst[:nbytes].copy_(flat[i % len(flat)])

    res = {"arm": "kernel", "shape": {"samples": n, "Hq": Hq, "Hkv": Hkv, "D": D, "prefix": prefix, "suffix": S},
           "split_keys": a.split_keys, "max_abs_difference": dev_max,
           "shared": dict(_us(_samples_ms(shared, a.warmup, a.iters), shared_bytes), bytes=shared_bytes,
                          copies=copies_s),
           "plain": dict(_us(_samples_ms(plain_fn, a.warmup, a.iters), plain_bytes), bytes=plain_bytes, copies=copies_p)}
    res["shared_again"] = _us(_samples_ms(shared, a.warmup, a.iters), shared_bytes)
    res["copy_plain_bytes"] = _us(_samples_ms(copy_of(plain, plain_bytes), a.warmup, a.iters), plain_bytes)
    res["copy_shared_bytes"] = _us(_samples_ms(copy_of([pk[i] + sk[i] for i in range(copies_s)], shared_bytes), a.warmup,
                                               a.iters), shared_bytes)
    res["plain_over_shared"] = round(res["plain"]["median_us"] / res["shared"]["median_us"], 2)
    print(json.dumps(res), flush=True)


def _model(a, dev):
    from tf_operator_amd.models.llama import PRESETS, Llama

    m = Llama(PRESETS[a.preset], device=dev)
    m.init_weights(0)
    return m.eval()


def _fill(cache, length):
    for t in cache.k + cache.v:
        t.normal_()
    cache.set_lengths([length] * cache.batch)
    return cache


@torch.no_grad()
def step_arm(a, dev, prefix, m):
    n, steps, rounds = a.samples, 16, 8
    tok = torch.zeros(n, dtype=torch.int64, device=dev)
    plain = _fill(m.new_cache(n, prefix + steps), prefix)
    shared = m.new_shared_cache(1, n, prefix, steps)
    _fill(shared.prefix, prefix)

    def block(cache):
        """ms per step over `steps` steps from the prompt's length on; the reset is outside the clock."""
        if cache is plain:
            plain.set_lengths([prefix] * n)
        else:
            shared.suffix.set_lengths([0] * n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            m.decode_step(tok, cache, gemm="skinny")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for c in (plain, shared):   # warm up both
        block(c)
    ts, tp = [], []
    for r in range(rounds):     # ABBA
        order = (shared, plain, plain, shared) if r % 2 == 0 else (plain, shared, shared, plain)
        got = {id(shared): [], id(plain): []}
        for c in order:
            got[id(c)].append(block(c))
        ts.append(statistics.mean(got[id(shared)]))
        tp.append(statistics.mean(got[id(plain)]))
    diff = [p - s for p, s in zip(tp, ts)]
    print(json.dumps({"arm": "step", "preset": a.preset, "rows": n, "prefix": prefix, "gemm": "skinny",
                      "rounds": rounds, "steps": steps, "shared_ms_per_step": round(statistics.mean(ts), 4),
                      "plain_ms_per_step": round(statistics.mean(tp), 4),
                      "plain_minus_shared_ms": round(statistics.mean(diff), 4),
                      "standard_error_ms": round(statistics.stdev(diff) / len(diff) ** 0.5, 4)}), flush=True)


@torch.no_grad()
def call_arm(a, dev, prefix, m):
    from tf_operator_amd.train.generate import generate

    n, new = a.samples, 16
    prompt = torch.randint(0, m.cfg.vocab_size, (1, prefix), device=dev, generator=torch.Generator(dev).manual_seed(1))

    def calls(**kw):
        times = []
        for _ in range(1 + a.calls):   # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate(m, prompt if "samples" in kw else prompt.repeat_interleave(n, 0), new, gemm="skinny",
                     prefill_chunk=a.prefill_chunk, **kw)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(times[1:]), 2), "min_ms": round(min(times[1:]), 2),
                "max_ms": round(max(times[1:]), 2)}

    st, pt = calls(samples=n), calls()
    st["cache_bytes"] = m.new_shared_cache(1, n, prefix, new).nbytes()
    pt["cache_bytes"] = m.new_cache(n, prefix + new).nbytes()
    print(json.dumps({"arm": "call", "preset": a.preset, "samples": n, "prefix": prefix, "new_tokens": new,
                      "prefill_chunk": a.prefill_chunk, "calls": a.calls, "shared": st, "plain": pt}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("arms", nargs="+", choices=["kernel", "step", "call"])
    ap.add_argument("--prefix", type=int, nargs="+", default=[4096])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--suffix", type=int, default=64)
    ap.add_argument("--split-keys", type=int, default=256)
    ap.add_argument("--preset", default="llama3-8b")
    ap.add_argument("--prefill-chunk", type=int, default=None)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("decode_shared_bench needs a GPU: a CPU run says nothing about these times")
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = _model(a, dev) if set(a.arms) & {"step", "call"} else None
    for prefix in a.prefix:
        if "kernel" in a.arms:
            kernel_arm(a, dev, prefix)
            torch.cuda.empty_cache()
        if "step" in a.arms:
            step_arm(a, dev, prefix, m)
        if "call" in a.arms:
            call_arm(a, dev, prefix, m)


if __name__ == "__main__":
    main()
