#!/usr/bin/env python3
"""Time toa_sample_tokens (csrc/hip/sample.hip) against train/generate.py's
_pick, the library-call sampler, in the same process.

Shapes: B in {1, 8, 16} rows of V = 128256 bf16 logits (the Llama-3 head).
Cases: (T 0.8, top_k 50), (T 0.8, top_p 0.9), (T 0.8, min_p 0.05).  _pick has
no top-p or min-p filter: in those two cases it runs with the temperature
alone, which is the least it would have to do.

The kernel is timed as ops.sample.sample_tokens with its per-row arrays made
once (what generate(sampler="device") does per token) -- the launch, plus the
allocation of the token tensor.

Method of scripts/extend_bench.py: device events around each sample, warm-up
first, the median (and range) over the samples, each sample a few back-to-back
repetitions; one process, one JSON line.

    python scripts/sample_bench.py [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 128256
CASES = {"top_k_50": dict(top_k=50), "top_p_0.9": dict(top_p=0.9), "min_p_0.05": dict(min_p=0.05)}


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs a GPU: a CPU run says nothing about the kernel's rate")
    from tf_operator_amd.ops import _lib, sample
    from tf_operator_amd.train.generate import _pick

    assert _lib.available(), _lib.load_error()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "iters": a.iters, "V": V, "dtype": "bf16", "temperature": 0.8,
           "B": {}}
    for B in (1, 8, 16):
        g = torch.Generator(device=dev).manual_seed(B)
        logits = (torch.randn(B, V, device=dev, generator=g) * 2.5).to(torch.bfloat16)
        pos = torch.full((B,), 17, dtype=torch.int32, device=dev)
        sid = torch.arange(B, device=dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        rows = {}
        for name, kw in CASES.items():
            full = {"temperature": 0.8, "top_k": 0, "top_p": 1.0, "min_p": 0.0, **kw}
            rowp = {n: sample.row_parameter(n, v, B, dev) for n, v in full.items()}
            k = kw.get("top_k", 0)
            row = {"kernel": _us(_median_ms(lambda: sample.sample_tokens(logits, seed=1, stream_ids=sid, positions=pos,
                                                                         **rowp), a.warmup, a.iters, 10)),
                   "torch_pick": _us(_median_ms(lambda: _pick(logits, 0.8, k, gen), a.warmup, a.iters, 10)),
                   "torch_pick_filter": "top_k" if k else "none"}
            row["kernel_of_torch_pick"] = round(row["kernel"]["median_us"] / row["torch_pick"]["median_us"], 3)
            rows[name] = row
        res["B"][str(B)] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
