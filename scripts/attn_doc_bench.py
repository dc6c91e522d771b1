"""Document-masked attention against the unmasked paths at the Llama-3-8B
bench shape (B=6, H=32, Hkv=8, S=4096, D=128, O / dO in [B,S,H,D]), one
process, interleaved rounds on random data (guide §5.4 rules 24/25):

    default  toa_attn_fwd / toa_attn_bwd as the step runs them (the assembly
             forward, the dS-form backward)
    hip      the general HIP kernels the mask is an arm of: the register-staged
             forward (toa_attn_set_fwd_variant(0)) and the two-kernel backward
             (toa_attn_set_bwd_variant(0), i.e. TOA_ATTN_BWD=sp)
    doc4096  toa_attn_fwd_doc / toa_attn_bwd_doc with one document per row
    doc1024  ... documents of 1024 tokens
    doc512   ... documents of 512 tokens

Prints forward and backward time per arm and the visible 64 x 64 tiles of
each mask relative to plain causal.

    python scripts/attn_doc_bench.py [--rounds 6] [--reps 5]
"""
import argparse
import json
import math
import statistics
import sys

import torch

sys.path.insert(0, ".")
from tf_operator_amd.ops import _lib, llm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=6)
    a = ap.parse_args()
    B, H, Hk, S, D = a.batch, 32, 8, 4096, 128
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda").to(torch.bfloat16)
    k = torch.randn(B, Hk, S, D, device="cuda").to(torch.bfloat16)
    v = torch.randn(B, Hk, S, D, device="cuda").to(torch.bfloat16)
    do = torch.randn(B, S, H, D, device="cuda").to(torch.bfloat16)
    docs = {f"doc{n}": llm.doc_bounds_from_lengths([[n] * (S // n)] * B, S, device="cuda") for n in (4096, 1024, 512)}
    arms = ["default", "hip"] + list(docs)

    def variants(arm):
        _lib.call("toa_attn_set_fwd_variant", 0 if arm == "hip" else -1)
        _lib.call("toa_attn_set_bwd_variant", 0 if arm == "hip" else -1)

    def fwd(arm):
        if arm in docs:
            return llm._attn_fwd_doc(q, k, v, docs[arm][0], scale, True)
        return llm._attn_fwd(q, k, v, scale, True)

    def bwd(arm, o, lse):
        if arm in docs:
            return llm._attn_bwd_doc(q, k, v, o, lse, do, docs[arm][0], docs[arm][1], scale, True)
        return llm._attn_bwd(q, k, v, o, lse, do, scale, True)

    saved = {}
    for arm in arms:
        variants(arm)
        saved[arm] = fwd(arm)
    torch.cuda.synchronize()
    same = {f"{arm}_vs_hip": bool(torch.equal(saved[arm][0], saved["hip"][0]) and
                                  torch.equal(saved[arm][1], saved["hip"][1])) for arm in ("default", "doc4096")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tb = {arm: [] for arm in arms}, {arm: [] for arm in arms}
    for _ in range(a.rounds):
        for arm in arms:
            variants(arm)
            o, lse = saved[arm]
            fwd(arm)
            bwd(arm, o, lse)
            ev[0].record()
            for _ in range(a.reps):
                fwd(arm)
            ev[1].record()
            for _ in range(a.reps):
                bwd(arm, o, lse)
            ev[2].record()
            torch.cuda.synchronize()
            tf[arm].append(ev[0].elapsed_time(ev[1]) / a.reps)
            tb[arm].append(ev[1].elapsed_time(ev[2]) / a.reps)
    variants("default")
    nt = S // 64
    causal_tiles = nt * (nt + 1) // 2
    res = {"shape": [B, H, Hk, S, D], "rounds": a.rounds, "reps": a.reps, "o_lse_bit_equal": same}
    for arm in arms:
        r = {}
        for name, t in (("fwd", tf[arm]), ("bwd", tb[arm])):
            r[name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                       "max_ms": round(max(t), 4)}
        if arm in docs:
            n = int(arm[3:]) // 64
            r["visible_tiles_vs_causal"] = round((S // int(arm[3:])) * (n * (n + 1) // 2) / causal_tiles, 4)
        res[arm] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
