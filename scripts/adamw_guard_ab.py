"""The skipped-step guard off against on (FlatAdamW skip_nonfinite,
TOA_SKIP_NONFINITE), in ONE process, arms in ABBA order, over the whole flat
buffer of --model (default Llama-3-8B) and its W^T-writing launches: ms per
optimizer step (the norm, with the guard the verdict kernel, every AdamW
launch) and per arm the median and range over the rounds.

Both arms are optimizers over the SAME trainer's buffers (weights, master,
moments, gradient, W^T copies), so they differ only in the guard.  Four arms:
    off / on          clipping on (max_grad_norm 1): both pay the norm pass
    off0 / on0        clipping off: the guard alone pays the norm pass
The gradient is finite, so no step is skipped: this is what a healthy run
pays.  --skip-rounds N then times N rounds of steps that ARE skipped (a NaN
gradient element): the early-out.

    python scripts/adamw_guard_ab.py [--rounds 6] [--iters 5] [--adam-state fp32]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from tf_operator_amd.ops import _lib  # noqa: E402
from tf_operator_amd.ops.optim import FlatAdamW  # noqa: E402


def abba(arms, rounds):
    for r in range(rounds):
        yield from (arms if r % 2 == 0 else arms[::-1])


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def timed(opt, iters):
    opt.step()   # one untimed step after the switch of arms
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-rounds", type=int, default=2)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--adam-state", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    assert _lib.available(), _lib.load_error()
    from tf_operator_amd.train.llm import LlamaTrainer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tr = LlamaTrainer(a.model, dev, micro_batch=1, seq_len=256, adam_state=a.adam_state, skip_nonfinite=False)
    flat = tr.flat
    g = torch.Generator(device=dev).manual_seed(0)
    for c in range(0, flat.numel, 1 << 26):   # a finite gradient of a plausible size, in bounded pieces
        piece = flat.grad[c:c + (1 << 26)]
        piece.copy_((torch.randn(piece.numel(), device=dev, generator=g) * 1e-3).to(piece.dtype))

    def make(guard, clip):
        o = FlatAdamW(flat, lr=1e-5, max_grad_norm=1.0 if clip else 0.0, post_update=tr.opt.post_update,
                      state_dtype=tr.opt.state_dtype, skip_nonfinite=guard)
        o.fused_wt = tr.opt.fused_wt
        return o

    arms = {"off": make(False, True), "on": make(True, True), "off0": make(False, False), "on0": make(True, False)}
    fused = len(arms["on"]._fused_items())
    assert fused == len(arms["off"]._fused_items()) and fused > 0, "the W^T-writing update is not in the measurement"
    times = {k: [] for k in arms}
    for k in abba(list(arms), a.rounds):
        ms = timed(arms[k], a.iters)
        times[k].append(ms)
        print(json.dumps({"arm": k, "ms_per_step": round(ms, 4)}), flush=True)
    assert arms["on"].skipped_steps() == 0 and arms["on0"].skipped_steps() == 0
    assert bool(torch.isfinite(flat.master[:1 << 20]).all())
    out = {"model": a.model, "params": flat.numel, "adam_state": a.adam_state, "wt_launches": fused,
           "iters": a.iters, "ms_per_step": {k: summary(v) for k, v in times.items()}}
    med = {k: statistics.median(v) for k, v in times.items()}
    out["on_minus_off_ms"] = round(med["on"] - med["off"], 4)
    out["on0_minus_off0_ms"] = round(med["on0"] - med["off0"], 4)
    if a.skip_rounds:
        flat.grad[12345] = float("nan")
        before = flat.master[:1 << 20].clone()
        sk = [timed(arms["on"], a.iters) for _ in range(a.skip_rounds)]
        assert arms["on"].skipped_steps() == a.skip_rounds * (a.iters + 1)
        assert torch.equal(flat.master[:1 << 20], before)
        out["skipped_step_ms"] = summary(sk)
    print(json.dumps({"adamw_guard_ab": out}), flush=True)


if __name__ == "__main__":
    main()
