#!/usr/bin/env python3
"""Time the decode step's projections, per form and as a whole step.

Per form: the five Llama-3-8B projection shapes at M = 1, 8 and 16 rows on the
weight-streaming GEMM (``skinny``: csrc/hip/gemm_skinny.hip) and on the
training GEMMs the decode step ran before it (``tile``: toa_gemm_asm_rows, and
toa_gemm_asm_swiglu for gate|up), against a device copy of W's bytes in the
same process.  Every arm, the copy included, rotates over distinct copies of W
-- enough that the rotation's footprint is at least 512 MB, twice the Infinity
Cache, and never fewer than two -- so consecutive launches never touch the same
bytes.  The launchers are called directly on preallocated outputs, so the
host's cost per launch is a ctypes call.  The method is scripts/decode_bench.py's:
device events around samples of 10 back-to-back launches, warm-up first, the
median with min and max over the samples.  ``skinny_nt`` is the skinny kernel
with non-temporal loads on the W stream instead of the default cache policy.

Whole step: llama3-8b, random init, every row at length 1024, B = 1 and 8:
``decode_step`` with ``tile`` and ``skinny`` alternated ABBA in one process,
rounds of 16 steps per arm visit, the difference per round as mean +- standard
error.  The step is timed by device events around its 16 steps and includes
whatever the host's launch cost leaves exposed.

One JSON line.

    python scripts/decode_step_bench.py [--iters 50] [--rounds 8] [--skip-step] [--skip-forms]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INNER = 10          # launches per timed sample, back to back
ROTATION_BYTES = 512 << 20
FORMS = (("qkv", 6144, 4096, False), ("attn_out", 4096, 4096, False), ("gate_up", 14336, 4096, True),
         ("down", 4096, 14336, False), ("head", 128256, 4096, False))   # (name, N or F, K, SwiGLU)
MS = (1, 8, 16)
STEPS = 16          # decode steps per arm visit of the whole-step ABBA


def _sample_ms(fn, warmup, iters):
    """(median, min, max) ms per launch over `iters` samples of INNER launches; fn(i) is launch number i."""
    n = 0
    for _ in range(warmup):
        fn(n)
        n += 1
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn(n)
            n += 1
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / INNER)
    return statistics.median(times), min(times), max(times)


def _row(med, lo, hi, nbytes, copy_med=None):
    r = {"median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2),
         "W_GBps": round(nbytes / med / 1e6, 1)}
    if copy_med is not None:
        r["of_copy"] = round(copy_med / med, 3)
    return r


def bench_forms(a, dev):
    from tf_operator_amd.ops import _lib, gemm

    P, st = _lib.ptr, _lib.stream()
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, swiglu in FORMS:
        rows = 2 * N if swiglu else N
        nbytes = rows * K * 2
        copies = max(2, -(-ROTATION_BYTES // nbytes))
        ws_ = [(torch.randn(rows, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        dst = torch.empty_like(ws_[0])
        res = {"N": N, "K": K, "swiglu": swiglu, "W_bytes": nbytes, "copies": copies,
               "split": _lib.call_ret("toa_gemm_skinny_split", N, K)}
        med, lo, hi = _sample_ms(lambda i: dst.copy_(ws_[i % copies]), a.warmup, a.iters)
        copy_med = med
        res["copy"] = _row(med, lo, hi, nbytes)
        ws_name = "toa_gemm_skinny_swiglu_ws_bytes" if swiglu else "toa_gemm_skinny_ws_bytes"
        wsb = int(_lib.call_ret(ws_name, N, K))
        ws = torch.empty(max(wsb, 16) // 4, device=dev, dtype=torch.float32)
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            gu = torch.empty(M, 2 * N, device=dev, dtype=torch.bfloat16) if swiglu else None
            wp = [P(w) for w in ws_]
            sk = "toa_gemm_skinny_swiglu" if swiglu else "toa_gemm_skinny"

            def skinny(i):
                _lib.call(sk, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(ws), st)

            def tile(i):
                if swiglu:
                    _lib.call("toa_gemm_asm_swiglu", P(x), K, wp[i % copies], K, P(gu), 2 * N, P(y), N, M, N, K, st)
                else:
                    _lib.call("toa_gemm_asm_rows", P(x), K, wp[i % copies], K, P(y), N, M, N, K, st)

            arms = {}
            for arm, fn, nt in (("skinny", skinny, 0), ("tile", tile, 0), ("skinny_nt", skinny, 1)):
                _lib.call("toa_gemm_skinny_set_nt", nt)
                med, lo, hi = _sample_ms(fn, a.warmup, a.iters)
                arms[arm] = _row(med, lo, hi, nbytes, copy_med)
            _lib.call("toa_gemm_skinny_set_nt", 0)
            arms["skinny_vs_tile"] = round(arms["tile"]["median_us"] / arms["skinny"]["median_us"], 3)
            res[f"M{M}"] = arms
        med, lo, hi = _sample_ms(lambda i: dst.copy_(ws_[i % copies]), 2, a.iters)
        res["copy_again"] = _row(med, lo, hi, nbytes)   # the spread between the two copy figures: this run's noise
        out[name] = res
        del ws_, dst
        torch.cuda.empty_cache()
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")]
    return out


def bench_step(a, dev):
    from tf_operator_amd.models.llama import PRESETS, Llama

    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    out = {"preset": "llama3-8b", "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds}
    for B in (1, 8):
        cache = m.new_cache(B, a.length + STEPS)
        tokens = torch.randint(0, m.cfg.vocab_size, (B,), device=dev)

        def visit(arm):
            cache.set_lengths([a.length] * B)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(STEPS):
                m.decode_step(tokens, cache, gemm=arm)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / STEPS

        for arm in ("tile", "skinny"):
            visit(arm)   # warm-up: code objects, workspaces, allocator
        t, s, d = [], [], []
        for _ in range(a.rounds):
            r = [visit(arm) for arm in ("tile", "skinny", "skinny", "tile")]
            t.append((r[0] + r[3]) / 2)
            s.append((r[1] + r[2]) / 2)
            d.append(t[-1] - s[-1])
        se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
        out[f"B{B}"] = {"tile_ms_per_step": round(statistics.mean(t), 4), "skinny_ms_per_step": round(statistics.mean(s), 4),
                        "tile_minus_skinny_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--len", type=int, default=1024, dest="length")
    ap.add_argument("--skip-forms", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args(argv)
    if a.iters < 50 or a.rounds < 8:
        ap.error("--iters must be at least 50 and --rounds at least 8")
    if not torch.cuda.is_available():
        raise SystemExit("decode_step_bench needs a GPU: a CPU run says nothing about the kernels' rates")
    from tf_operator_amd.ops import _lib, gemm

    assert _lib.available(), _lib.load_error()
    gemm.resolve_auto()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "gemm_mode": gemm.mode(), "iters": a.iters, "inner": INNER}
    if not a.skip_forms:
        res["forms"] = bench_forms(a, dev)
    if not a.skip_step:
        res["step"] = bench_step(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
