"""AdamW moments in fp32 against bf16 (FlatAdamW state_dtype, TOA_ADAM_STATE),
in ONE process, arms in ABBA order:

1. kernels: one Llama-3-8B layer's linear weights (qkv, o, gate_up, down: 218M
   parameters) through toa_adamw_flat / toa_adamw_flat_bf16s (one launch over
   the buffer) and through toa_adamw_wt / toa_adamw_wt_bf16s (one launch per
   weight, W^T written too): ms per pass and achieved GB/s per arm, counting
   28 / 20 B per parameter (+2 B for the W^T copy);
2. in-model (--model, default the bench shape): ms per LlamaTrainer step per
   arm in alternating windows, with torch.cuda.max_memory_allocated() of each
   arm's windows.  One trainer: between windows the moments are converted in
   place (FlatAdamW._convert_moments), so both arms share every other buffer.

    python scripts/adamw_state_ab.py [--rounds 4] [--iters 10] [--steps 3] [--skip-model]
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from tf_operator_amd.ops import _lib  # noqa: E402
from tf_operator_amd.ops.optim import FlatAdamW  # noqa: E402
from tf_operator_amd.ops.wt import TransposedWeights  # noqa: E402
from tf_operator_amd.parallel.flat import FlatParams  # noqa: E402

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def abba(arms, rounds):
    for r in range(rounds):
        yield from (arms if r % 2 == 0 else arms[::-1])


def summary(v):
    return {"mean": round(statistics.fmean(v), 4), "spread": round(statistics.pstdev(v), 4), "n": len(v)}


def kernels(a):
    torch.manual_seed(0)
    shapes = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]
    nparam = sum(r * c for r, c in shapes)
    opts = {}
    for st in DT:   # each arm its own buffers: 218M x (28 | 20) B, far beyond the caches either way
        ps = [torch.nn.Parameter(torch.randn(*s, device="cuda").to(torch.bfloat16) * 0.02) for s in shapes]
        flat = FlatParams(ps)
        flat.grad.copy_(torch.randn(flat.grad.numel(), device="cuda").to(flat.grad.dtype) * 1e-3)
        plain = FlatAdamW(flat, lr=1e-4, max_grad_norm=0.0, weight_decay=0.0, state_dtype=DT[st])
        fused = FlatAdamW(flat, lr=1e-4, max_grad_norm=0.0, weight_decay=0.0, state_dtype=DT[st])
        fused.fused_wt = TransposedWeights(flat, ps)
        assert len(fused._fused_items()) == len(shapes) and len(plain.runs) == 1
        opts[st] = {"flat": plain, "wt": fused}
    out = {}
    for form in ("flat", "wt"):
        times = {st: [] for st in DT}
        for st in abba(list(DT), a.rounds):
            o = opts[st][form]
            o.step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                o.step()
            e1.record()
            torch.cuda.synchronize()
            times[st].append(e0.elapsed_time(e1) / a.iters)
        for st, v in times.items():
            bpp = (28 if st == "fp32" else 20) + (2 if form == "wt" else 0)
            ms = statistics.fmean(v)
            out[f"{form}/{st}"] = {"ms": summary(v), "bytes_per_param": bpp,
                                   "GBps": round(nparam * bpp / ms / 1e6, 1)}
        out[f"{form}/bf16_vs_fp32_pct"] = round(100 * (statistics.fmean(times["bf16"]) /
                                                        statistics.fmean(times["fp32"]) - 1), 2)
    out["params"] = nparam
    print(json.dumps({"kernels": out}), flush=True)


def in_model(a):
    from tf_operator_amd.ops import gemm
    from tf_operator_amd.train.llm import LlamaTrainer

    dev = torch.device("cuda", 0)
    tr = LlamaTrainer(a.model, dev, micro_batch=a.micro_batch, seq_len=a.seq_len, adam_state="fp32")
    batch = [tr.synthetic_batch()]

    def switch(st):
        torch.cuda.synchronize()
        tr.opt.state_dtype = tr.flat.moment_dtype = DT[st]
        tr.opt._convert_moments()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    for st in DT:   # both arms warm
        switch(st)
        for _ in range(a.warmup):
            tr.step(batch)
    times, peak = {st: [] for st in DT}, {st: 0 for st in DT}
    for st in abba(list(DT), a.rounds):
        switch(st)
        tr.step(batch)   # one untimed step after the switch
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = tr.step(batch)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        times[st].append(ms)
        peak[st] = max(peak[st], torch.cuda.max_memory_allocated(dev))
        print(json.dumps({"arm": st, "ms_per_step": round(ms, 2), "loss": float(loss),
                          "peak_GiB": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}), flush=True)
    d = [y - x for x, y in zip(times["fp32"], times["bf16"])]   # paired by window index
    out = {"model": a.model, "micro_batch": a.micro_batch, "seq_len": a.seq_len,
           "ms_per_step": {st: summary(v) for st, v in times.items()},
           "bf16_minus_fp32_ms": summary(d), "peak_GiB": {st: round(p / 2**30, 2) for st, p in peak.items()},
           "gemm_fallbacks": sum(gemm.fallbacks().values())}
    print(json.dumps({"in_model": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--micro-batch", type=int, default=6)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    assert _lib.available(), _lib.load_error()
    torch.cuda.set_device(0)
    if not a.skip_kernels:
        kernels(a)
        torch.cuda.empty_cache()
    if not a.skip_model:
        in_model(a)


if __name__ == "__main__":
    main()
