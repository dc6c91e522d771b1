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

``--fp4``: the 1-to-16-row GEMM on MXFP4 weights (csrc/hip/gemm_w4.hip) beside
the fp8 and bf16 ones per form, and the whole step on an fp4 snapshot against
an fp8 one (bench_fp4).  ``--fp8``: the 1-to-16-row GEMM on fp8 weights (csrc/hip/gemm_w8.hip) beside
``skinny`` and the 17-to-64-row one (csrc/hip/gemm_stream_w8.hip) beside
``stream``, per form against a copy of q's bytes, and as a whole step and a
whole extend call on a snapshot (bench_fp8).  With ``--only-stream``: the
17-to-64-row arms and the extend call alone.

    python scripts/decode_step_bench.py [--iters 50] [--rounds 8] [--skip-step] [--skip-forms] [--only-stream]
                                        [--extend] [--fp8] [--fp4] [--wide]

``--wide``: the 65-to-128-row GEMM (csrc/hip/gemm_wide.hip) per form at M = 65,
96 and 128 against ``tile``, ``stream`` at M = 64, the decode step of 128 rows
and a generate(samples=16) call on 8 prompts, ``wide`` against ``stream``
(bench_wide).  ``--wide --fp8``: the fp8 arm of that protocol alone, the
65-to-128-row GEMM on fp8 weights (csrc/hip/gemm_wide_w8.hip) per form at
M = 65, 96 and 128 against ``wide`` on the bf16 weights, and the decode step of
128 rows on a snapshot against the same on the bf16 weights (bench_wide_fp8).
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
STREAM_MS = (17, 32, 48, 64)   # the 17-to-64-row kernel (csrc/hip/gemm_stream.hip): the ``stream`` arm against ``tile``
STREAM_W8_MS = (17, 32, 64)    # the 17-to-64-row kernel on fp8 weights (csrc/hip/gemm_stream_w8.hip) against ``stream``
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
        st_wsb = int(_lib.call_ret(ws_name.replace("skinny", "stream"), N, K))
        st_ws = torch.empty(max(st_wsb, 16) // 4, device=dev, dtype=torch.float32)
        res["stream_split"] = _lib.call_ret("toa_gemm_stream_split", N, K)
        for M in STREAM_MS if name != "head" else ():   # the head stays on the tile kernel (ops.decode.TILE_KEEPS_FROM)
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            gu = torch.empty(M, 2 * N, device=dev, dtype=torch.bfloat16) if swiglu else None
            wp = [P(w) for w in ws_]
            sn_ = "toa_gemm_stream_swiglu" if swiglu else "toa_gemm_stream"

            def stream(i):
                _lib.call(sn_, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(st_ws), st)

            def tile_(i):
                if swiglu:
                    _lib.call("toa_gemm_asm_swiglu", P(x), K, wp[i % copies], K, P(gu), 2 * N, P(y), N, M, N, K, st)
                else:
                    _lib.call("toa_gemm_asm_rows", P(x), K, wp[i % copies], K, P(y), N, M, N, K, st)

            arms = {}
            for arm, fn in (("stream", stream), ("tile", tile_)):
                med, lo, hi = _sample_ms(fn, a.warmup, a.iters)
                arms[arm] = _row(med, lo, hi, nbytes, copy_med)
            arms["stream_vs_tile"] = round(arms["tile"]["median_us"] / arms["stream"]["median_us"], 3)
            res[f"M{M}"] = arms
        for M in MS if not a.only_stream else ():
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


def bench_fp8(a, dev):
    """The fp8 arm (csrc/hip/gemm_w8.hip) beside ``skinny``.  Per form, the four block projections at M = 1, 8 and
    16: the fp8 GEMM over rotating copies of q (at least ROTATION_BYTES of them), the bf16 skinny GEMM over as many
    copies of W, and a device copy of q's bytes as the yardstick.  Whole step: ``decode_step(gemm="skinny")`` on the
    bf16 weights against the same on a snapshot, ABBA as in bench_step; the time of quantize_projections and the
    snapshot's bytes.  The same at M = 17, 32 and 64 for the 17-to-64-row kernels: toa_gemm_stream_w8 against
    toa_gemm_stream, which is what ran these operands before it; and the whole call, Llama.extend of 8 rows x 4
    tokens under ``stream`` on the bf16 weights against the same on the snapshot, ABBA."""
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.ops import _lib, gemm

    P, st = _lib.ptr, _lib.stream()
    forms = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, swiglu in FORMS[:4]:
        rows = 2 * N if swiglu else N
        qbytes = rows * K
        copies = max(2, -(-ROTATION_BYTES // qbytes))
        ws_ = [(torch.randn(rows, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        pairs = [gemm.quantize_w8(w) for w in ws_]
        dst = torch.empty_like(pairs[0][0])
        res = {"N": N, "K": K, "swiglu": swiglu, "q_bytes": qbytes, "copies": copies,
               "split": _lib.call_ret("toa_gemm_skinny_w8_split", rows, K),
               "skinny_split": _lib.call_ret("toa_gemm_skinny_split", N, K)}
        copy_med, lo, hi = _sample_ms(lambda i: dst.copy_(pairs[i % copies][0]), a.warmup, a.iters)
        res["copy_q"] = _row(copy_med, lo, hi, qbytes)
        tail = "_swiglu" if swiglu else ""
        ws8 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_skinny_w8{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        ws16 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_skinny{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        wp, qp, sp = [P(w) for w in ws_], [P(q) for q, _ in pairs], [P(s) for _, s in pairs]
        res["stream_w8_split"] = _lib.call_ret("toa_gemm_stream_w8_split", rows, K)
        res["stream_split"] = _lib.call_ret("toa_gemm_stream_split", N, K)
        sws8 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_stream_w8{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        sws16 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_stream{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        for M in STREAM_W8_MS:
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def stream_fp8(i):
                _lib.call("toa_gemm_stream_w8" + tail, P(x), K, qp[i % copies], K, sp[i % copies], P(y), N, M, N, K,
                          P(sws8), st)

            def stream(i):
                _lib.call("toa_gemm_stream" + tail, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(sws16), st)

            arms = {"fp8": _row(*_sample_ms(stream_fp8, a.warmup, a.iters), qbytes, copy_med),
                    "stream": _row(*_sample_ms(stream, a.warmup, a.iters), 2 * qbytes)}
            arms["fp8_vs_stream"] = round(arms["stream"]["median_us"] / arms["fp8"]["median_us"], 3)
            res[f"M{M}"] = arms
        for M in MS if not a.only_stream else ():
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fp8(i):
                _lib.call("toa_gemm_skinny_w8" + tail, P(x), K, qp[i % copies], K, sp[i % copies], P(y), N, M, N, K,
                          P(ws8), st)

            def skinny(i):
                _lib.call("toa_gemm_skinny" + tail, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(ws16), st)

            arms = {"fp8": _row(*_sample_ms(fp8, a.warmup, a.iters), qbytes, copy_med),
                    "skinny": _row(*_sample_ms(skinny, a.warmup, a.iters), 2 * qbytes)}
            arms["fp8_vs_skinny"] = round(arms["skinny"]["median_us"] / arms["fp8"]["median_us"], 3)
            res[f"M{M}"] = arms
        forms[name] = res
        del ws_, pairs, dst
        torch.cuda.empty_cache()
    out = {"forms": forms}
    if a.skip_step:
        return out
    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    m.quantize_projections()   # warm-up
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    snap = m.quantize_projections()
    e.record()
    e.synchronize()
    step = {"preset": "llama3-8b", "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds,
            "quantize_projections_ms": round(s.elapsed_time(e), 3),
            "snapshot_bytes": sum(q.numel() + 4 * sc.numel() for b in snap for q, sc in b.values())}
    for B in (1, 8) if not a.only_stream else ():
        cache = m.new_cache(B, a.length + STEPS)
        tokens = torch.randint(0, m.cfg.vocab_size, (B,), device=dev)

        def visit(weights):
            cache.set_lengths([a.length] * B)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(STEPS):
                m.decode_step(tokens, cache, gemm="skinny", weights=weights)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / STEPS

        for w in (None, snap):
            visit(w)   # warm-up: code objects, workspaces, allocator
        t, f, d = [], [], []
        for _ in range(a.rounds):
            r = [visit(w) for w in (None, snap, snap, None)]
            t.append((r[0] + r[3]) / 2)
            f.append((r[1] + r[2]) / 2)
            d.append(t[-1] - f[-1])
        se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
        step[f"B{B}"] = {"skinny_ms_per_step": round(statistics.mean(t), 4), "fp8_ms_per_step": round(statistics.mean(f), 4),
                         "skinny_minus_fp8_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4)}
    B, T = 8, 4
    cache = m.new_cache(B, a.length + T)
    tokens = torch.randint(0, m.cfg.vocab_size, (B, T), device=dev)

    def call(weights):
        cache.set_lengths([a.length] * B)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        with torch.no_grad():
            m.extend(tokens, cache, gemm="stream", logits="last", weights=weights)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for w in (None, snap, None, snap):
        call(w)   # warm-up: code objects, workspaces, allocator
    t, f, d = [], [], []
    for _ in range(a.rounds):
        r = [call(w) for w in (None, snap, snap, None)]
        t.append((r[0] + r[3]) / 2)
        f.append((r[1] + r[2]) / 2)
        d.append(t[-1] - f[-1])
    se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
    out["extend"] = {"preset": "llama3-8b", "B": B, "T": T, "length": a.length, "rounds": a.rounds,
                     "stream_ms": round(statistics.mean(t), 4), "fp8_ms": round(statistics.mean(f), 4),
                     "stream_minus_fp8_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4)}
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    out["step"] = step
    return out


def bench_fp4(a, dev):
    """The MXFP4 arm (csrc/hip/gemm_w4.hip) beside the fp8 kernel, which is what ran these operands before it, and
    bf16 ``skinny``; bench_fp8's protocol.  Per form at M = 1, 8 and 16: the fp4 GEMM over rotating copies of q and
    its scales (at least ROTATION_BYTES of them), the fp8 and bf16 GEMMs over as many copies of theirs, and a device
    copy of the fp4 bytes as the yardstick.  Whole step: ``decode_step(gemm="skinny")`` on an fp8 snapshot against the
    same on an fp4 one, ABBA; the time of quantize_projections(fmt="fp4") and the snapshot's bytes."""
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.ops import _lib, gemm

    P, st = _lib.ptr, _lib.stream()
    forms = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, swiglu in FORMS[:4]:
        rows = 2 * N if swiglu else N
        qbytes = rows * (K // 2 + K // 32)
        copies = max(2, -(-ROTATION_BYTES // qbytes))
        ws_ = [(torch.randn(rows, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        p8, p4 = [gemm.quantize_w8(w) for w in ws_], [gemm.quantize_w4(w) for w in ws_]
        lds = p4[0][1].stride(0)
        src = [torch.empty(qbytes, device=dev, dtype=torch.uint8) for _ in range(copies)]   # q and scales, one buffer
        dst = torch.empty_like(src[0])
        res = {"N": N, "K": K, "swiglu": swiglu, "q_and_scale_bytes": qbytes, "copies": copies,
               "split": _lib.call_ret("toa_gemm_skinny_w4_split", rows, K),
               "fp8_split": _lib.call_ret("toa_gemm_skinny_w8_split", rows, K)}
        copy_med, lo, hi = _sample_ms(lambda i: dst.copy_(src[i % copies]), a.warmup, a.iters)
        res["copy"] = _row(copy_med, lo, hi, qbytes)
        tail = "_swiglu" if swiglu else ""
        ws4 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_skinny_w4{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        ws8 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_skinny_w8{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        ws16 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_skinny{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        wp = [P(w) for w in ws_]
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fp4(i):
                q, s = p4[i % copies]
                _lib.call("toa_gemm_skinny_w4" + tail, P(x), K, P(q), K // 2, P(s), lds, P(y), N, M, N, K, P(ws4), st)

            def fp8(i):
                q, s = p8[i % copies]
                _lib.call("toa_gemm_skinny_w8" + tail, P(x), K, P(q), K, P(s), P(y), N, M, N, K, P(ws8), st)

            def skinny(i):
                _lib.call("toa_gemm_skinny" + tail, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(ws16), st)

            arms = {"fp4": _row(*_sample_ms(fp4, a.warmup, a.iters), qbytes, copy_med),
                    "fp8": _row(*_sample_ms(fp8, a.warmup, a.iters), rows * K),
                    "skinny": _row(*_sample_ms(skinny, a.warmup, a.iters), 2 * rows * K)}
            arms["fp4_vs_fp8"] = round(arms["fp8"]["median_us"] / arms["fp4"]["median_us"], 3)
            arms["fp4_vs_skinny"] = round(arms["skinny"]["median_us"] / arms["fp4"]["median_us"], 3)
            res[f"M{M}"] = arms
        forms[name] = res
        del ws_, p8, p4, src, dst
        torch.cuda.empty_cache()
    out = {"forms": forms}
    if a.skip_step:
        return out
    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    m.quantize_projections(fmt="fp4")   # warm-up
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    snap4 = m.quantize_projections(fmt="fp4")
    e.record()
    e.synchronize()
    snap8 = m.quantize_projections()
    step = {"preset": "llama3-8b", "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds,
            "quantize_projections_fp4_ms": round(s.elapsed_time(e), 3),
            "fp4_snapshot_bytes": sum(q.numel() + sc.numel() for b in snap4 for q, sc in b.values()),
            "fp8_snapshot_bytes": sum(q.numel() + 4 * sc.numel() for b in snap8 for q, sc in b.values())}
    for B in (1, 8):
        cache = m.new_cache(B, a.length + STEPS)
        tokens = torch.randint(0, m.cfg.vocab_size, (B,), device=dev)

        def visit(weights):
            cache.set_lengths([a.length] * B)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(STEPS):
                m.decode_step(tokens, cache, gemm="skinny", weights=weights)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / STEPS

        for w in (snap8, snap4):
            visit(w)   # warm-up: code objects, workspaces, allocator
        t, f, d = [], [], []
        for _ in range(a.rounds):
            r = [visit(w) for w in (snap8, snap4, snap4, snap8)]
            t.append((r[0] + r[3]) / 2)
            f.append((r[1] + r[2]) / 2)
            d.append(t[-1] - f[-1])
        se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
        step[f"B{B}"] = {"fp8_ms_per_step": round(statistics.mean(t), 4), "fp4_ms_per_step": round(statistics.mean(f), 4),
                         "fp8_minus_fp4_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4)}
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    out["step"] = step
    return out


def bench_kv(a, dev):
    """The whole decode step on llama3-8b, ``skinny`` projections, B = 1 and 8 at cache length --len: the bf16 cache
    against the fp8 cache (csrc/hip/kv_cache_q8.hip), ABBA as in bench_step; ms per step and the caches' bytes."""
    from tf_operator_amd.models.llama import PRESETS, Llama

    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    out = {"preset": "llama3-8b", "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds}
    for B in (1, 8):
        caches = {"bf16": m.new_cache(B, a.length + STEPS), "fp8": m.new_cache(B, a.length + STEPS,
                                                                                 dtype=torch.float8_e4m3fn)}
        tokens = torch.randint(0, m.cfg.vocab_size, (B,), device=dev)

        def visit(kv):
            cache = caches[kv]
            cache.set_lengths([a.length] * B)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(STEPS):
                m.decode_step(tokens, cache, gemm="skinny")
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / STEPS

        for kv in ("bf16", "fp8"):
            visit(kv)   # warm-up: code objects, workspaces, allocator
        t, f, d = [], [], []
        for _ in range(a.rounds):
            r = [visit(kv) for kv in ("bf16", "fp8", "fp8", "bf16")]
            t.append((r[0] + r[3]) / 2)
            f.append((r[1] + r[2]) / 2)
            d.append(t[-1] - f[-1])
        se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
        out[f"B{B}"] = {"bf16_ms_per_step": round(statistics.mean(t), 4), "fp8_ms_per_step": round(statistics.mean(f), 4),
                        "bf16_minus_fp8_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4),
                        "cache_bytes": {k: c.nbytes() for k, c in caches.items()}}
        del caches
        torch.cuda.empty_cache()
    return out


def _abba(visit, a_arm, b_arm, rounds):
    """Arms a and b alternated ABBA: (mean a, mean b, mean of a - b per round, its standard error)."""
    for arm in (a_arm, b_arm):
        visit(arm)   # warm-up: code objects, workspaces, allocator
    ta, tb, d = [], [], []
    for _ in range(rounds):
        r = [visit(arm) for arm in (a_arm, b_arm, b_arm, a_arm)]
        ta.append((r[0] + r[3]) / 2)
        tb.append((r[1] + r[2]) / 2)
        d.append(ta[-1] - tb[-1])
    se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
    return (round(statistics.mean(ta), 4), round(statistics.mean(tb), 4), round(statistics.mean(d), 4), round(se, 4))


def bench_wide(a, dev):
    """The 65-to-128-row kernel (csrc/hip/gemm_wide.hip).  Per form, the four block projections at M = 65, 96 and
    128: ``wide`` against ``tile`` (what ran these rows before it) and a device copy of W's bytes, and ``stream`` at
    M = 64 for continuity; bench_forms' protocol.  Whole step: ``decode_step`` of 128 rows under ``wide`` against
    ``stream`` (whose projections fall to ``tile`` there), ABBA; and one generate(samples=16) call on 8 prompts."""
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.ops import _lib, gemm
    from tf_operator_amd.train.generate import generate

    P, st = _lib.ptr, _lib.stream()
    forms = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, swiglu in FORMS[:4] if not a.skip_forms else ():
        rows = 2 * N if swiglu else N
        nbytes = rows * K * 2
        copies = max(2, -(-ROTATION_BYTES // nbytes))
        ws_ = [(torch.randn(rows, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        dst = torch.empty_like(ws_[0])
        wp = [P(w) for w in ws_]
        tail = "_swiglu" if swiglu else ""
        res = {"N": N, "K": K, "swiglu": swiglu, "W_bytes": nbytes, "copies": copies,
               "wide_split": _lib.call_ret("toa_gemm_wide_split", rows, K)}
        copy_med, lo, hi = _sample_ms(lambda i: dst.copy_(ws_[i % copies]), a.warmup, a.iters)
        res["copy"] = _row(copy_med, lo, hi, nbytes)
        wsb = max(int(_lib.call_ret(f"toa_gemm_wide{tail}_ws_bytes", N, K)),
                  int(_lib.call_ret(f"toa_gemm_stream{tail}_ws_bytes", N, K)), 16)
        ws = torch.empty(wsb // 4, device=dev, dtype=torch.float32)
        for M in (64, 65, 96, 128):
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            gu = torch.empty(M, 2 * N, device=dev, dtype=torch.bfloat16) if swiglu else None
            kern = ("toa_gemm_stream" if M == 64 else "toa_gemm_wide") + tail

            def stream_or_wide(i):
                _lib.call(kern, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(ws), st)

            def tile(i):
                if swiglu:
                    _lib.call("toa_gemm_asm_swiglu", P(x), K, wp[i % copies], K, P(gu), 2 * N, P(y), N, M, N, K, st)
                else:
                    _lib.call("toa_gemm_asm_rows", P(x), K, wp[i % copies], K, P(y), N, M, N, K, st)

            arm = "stream" if M == 64 else "wide"
            arms = {arm: _row(*_sample_ms(stream_or_wide, a.warmup, a.iters), nbytes, copy_med),
                    "tile": _row(*_sample_ms(tile, a.warmup, a.iters), nbytes, copy_med)}
            arms[arm + "_vs_tile"] = round(arms["tile"]["median_us"] / arms[arm]["median_us"], 3)
            res[f"M{M}"] = arms
        forms[name] = res
        del ws_, dst
        torch.cuda.empty_cache()
    out = {"forms": forms}
    if a.skip_step:
        return out
    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    B = 128
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

    gemm.reset_fallbacks()
    visit("wide")
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    ts, tw, d, se = _abba(visit, "stream", "wide", a.rounds)
    out["step"] = {"preset": "llama3-8b", "rows": B, "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds,
                   "stream_ms_per_step": ts, "wide_ms_per_step": tw, "stream_minus_wide_ms": d, "stderr_ms": se}
    del cache
    torch.cuda.empty_cache()
    prompts = torch.randint(0, m.cfg.vocab_size, (8, a.length), device=dev)

    def sample(arm):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        generate(m, prompts, STEPS, gemm=arm, samples=16)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    ts, tw, d, se = _abba(sample, "stream", "wide", a.rounds)
    out["generate"] = {"prompts": 8, "samples": 16, "prompt_len": a.length, "new_tokens": STEPS, "rounds": a.rounds,
                       "stream_ms": ts, "wide_ms": tw, "stream_minus_wide_ms": d, "stderr_ms": se}
    return out


def bench_wide_fp8(a, dev):
    """The 65-to-128-row kernel on fp8 weights (csrc/hip/gemm_wide_w8.hip) against the bf16 ``wide`` kernel, which is
    what ran these operands before it.  Per form, the four block projections at M = 65, 96 and 128: toa_gemm_wide_w8
    over rotating copies of q (at least ROTATION_BYTES of them), toa_gemm_wide over as many copies of W, and a device
    copy of q's bytes; bench_fp8's protocol.  Whole step: ``decode_step`` of 128 rows under ``wide`` on the bf16
    weights against the same on a snapshot, ABBA."""
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.ops import _lib, gemm

    P, st = _lib.ptr, _lib.stream()
    forms = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, swiglu in FORMS[:4] if not a.skip_forms else ():
        rows = 2 * N if swiglu else N
        qbytes = rows * K
        copies = max(2, -(-ROTATION_BYTES // qbytes))
        ws_ = [(torch.randn(rows, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        pairs = [gemm.quantize_w8(w) for w in ws_]
        dst = torch.empty_like(pairs[0][0])
        tail = "_swiglu" if swiglu else ""
        res = {"N": N, "K": K, "swiglu": swiglu, "q_bytes": qbytes, "copies": copies,
               "wide_w8_split": _lib.call_ret("toa_gemm_wide_w8_split", rows, K),
               "wide_split": _lib.call_ret("toa_gemm_wide_split", rows, K)}
        copy_med, lo, hi = _sample_ms(lambda i: dst.copy_(pairs[i % copies][0]), a.warmup, a.iters)
        res["copy_q"] = _row(copy_med, lo, hi, qbytes)
        ws8 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_wide_w8{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        ws16 = torch.empty(max(int(_lib.call_ret(f"toa_gemm_wide{tail}_ws_bytes", N, K)), 16) // 4, device=dev)
        wp, qp, sp = [P(w) for w in ws_], [P(q) for q, _ in pairs], [P(s) for _, s in pairs]
        for M in (65, 96, 128):
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fp8(i):
                _lib.call("toa_gemm_wide_w8" + tail, P(x), K, qp[i % copies], K, sp[i % copies], P(y), N, M, N, K,
                          P(ws8), st)

            def wide(i):
                _lib.call("toa_gemm_wide" + tail, P(x), K, wp[i % copies], K, P(y), N, M, N, K, P(ws16), st)

            arms = {"fp8": _row(*_sample_ms(fp8, a.warmup, a.iters), qbytes, copy_med),
                    "wide": _row(*_sample_ms(wide, a.warmup, a.iters), 2 * qbytes)}
            arms["fp8_vs_wide"] = round(arms["wide"]["median_us"] / arms["fp8"]["median_us"], 3)
            res[f"M{M}"] = arms
        forms[name] = res
        del ws_, pairs, dst
        torch.cuda.empty_cache()
    out = {"forms": forms}
    if a.skip_step:
        return out
    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    snap = m.quantize_projections()
    B = 128
    cache = m.new_cache(B, a.length + STEPS)
    tokens = torch.randint(0, m.cfg.vocab_size, (B,), device=dev)

    def visit(weights):
        cache.set_lengths([a.length] * B)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(STEPS):
            m.decode_step(tokens, cache, gemm="wide", weights=weights)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / STEPS

    gemm.reset_fallbacks()
    tw, tf, d, se = _abba(visit, None, snap, a.rounds)
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    out["step"] = {"preset": "llama3-8b", "rows": B, "length": a.length, "steps_per_visit": STEPS, "rounds": a.rounds,
                   "wide_ms_per_step": tw, "fp8_ms_per_step": tf, "wide_minus_fp8_ms": d, "stderr_ms": se}
    return out


def bench_extend(a, dev):
    """Llama.extend of T = 4 tokens on B = 8 rows at cache length --len, logits="last": ``tile`` and ``stream``
    alternated ABBA, device events around each call; ms per call."""
    from tf_operator_amd.models.llama import PRESETS, Llama

    m = Llama(PRESETS["llama3-8b"], device=dev)
    m.init_weights(0)
    m.eval()
    B, T = 8, 4
    cache = m.new_cache(B, a.length + T)
    tokens = torch.randint(0, m.cfg.vocab_size, (B, T), device=dev)

    def visit(arm):
        cache.set_lengths([a.length] * B)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        with torch.no_grad():
            m.extend(tokens, cache, gemm=arm, logits="last")
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for arm in ("tile", "stream", "tile", "stream"):
        visit(arm)   # warm-up: code objects, workspaces, allocator
    t, s, d = [], [], []
    for _ in range(a.rounds):
        r = [visit(arm) for arm in ("tile", "stream", "stream", "tile")]
        t.append((r[0] + r[3]) / 2)
        s.append((r[1] + r[2]) / 2)
        d.append(t[-1] - s[-1])
    se = statistics.stdev(d) / len(d) ** 0.5 if len(d) > 1 else float("nan")
    return {"preset": "llama3-8b", "B": B, "T": T, "length": a.length, "rounds": a.rounds,
            "tile_ms": round(statistics.mean(t), 4), "stream_ms": round(statistics.mean(s), 4),
            "tile_minus_stream_ms": round(statistics.mean(d), 4), "stderr_ms": round(se, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--len", type=int, default=1024, dest="length")
    ap.add_argument("--skip-forms", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--only-stream", action="store_true", help="per form, only the 17-to-64-row arms")
    ap.add_argument("--extend", action="store_true", help="the whole extend call, tile against stream")
    ap.add_argument("--fp8", action="store_true",
                    help="only the fp8 arm beside skinny: per form, the whole step (unless --skip-step), the quantiser")
    ap.add_argument("--fp4", action="store_true",
                    help="only the MXFP4 arm beside fp8 and skinny: per form, the whole step against an fp8 snapshot "
                         "(unless --skip-step), the quantiser")
    ap.add_argument("--wide", action="store_true",
                    help="only the 65-to-128-row arm: per form wide against tile, the 128-row step and generate call")
    ap.add_argument("--kv", action="store_true", help="only the whole step on the bf16 cache against the fp8 cache")
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
    if a.fp8 and a.wide:
        res["wide_fp8"] = bench_wide_fp8(a, dev)
    elif a.fp8:
        res["fp8"] = bench_fp8(a, dev)
    elif a.wide:
        res["wide"] = bench_wide(a, dev)
    elif a.fp4:
        res["fp4"] = bench_fp4(a, dev)
    if a.kv:
        res["kv"] = bench_kv(a, dev)
    if not a.skip_forms and not a.fp8 and not a.kv and not a.wide and not a.fp4:
        res["forms"] = bench_forms(a, dev)
    if not a.skip_step and not a.fp8 and not a.kv and not a.wide and not a.fp4:
        res["step"] = bench_step(a, dev)
    if a.extend:
        res["extend"] = bench_extend(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
