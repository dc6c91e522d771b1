#!/usr/bin/env python3
"""Time toa_attn_decode alone against a plain device copy of the bytes it reads.

Default shape: B = 8 rows, Hq = 32, Hkv = 8, D = 128, every row at length
4096 (the Llama-3-8B head layout).  The kernel reads K and V once:
2 x B x Hkv x L x D x 2 bytes.  The yardstick is a device-to-device copy of
that many bytes in the same process (its rate counts the bytes read, as the
kernel's does; the copy also writes them).  Device events around each sample,
warm-up first, the median over the samples (10 back-to-back launches each, so
the host's launch cost does not sit between the events); one JSON line.

    python scripts/decode_bench.py [--iters 50] [--split-keys 256] [--len 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


INNER = 10   # launches per timed sample, back to back: the host's launch cost hides behind the queue


def _median_ms(fn, warmup, iters):
    """(median, min, max) ms per launch over `iters` samples of INNER launches each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / INNER)
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--len", type=int, default=4096, dest="length")
    ap.add_argument("--split-keys", type=int, nargs="*", default=None, help="default: ops.decode.SPLIT_KEYS_DEFAULT")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs a GPU: a CPU run says nothing about the kernel's rate")
    from tf_operator_amd.ops import _lib, decode

    assert _lib.available(), _lib.load_error()
    dev = torch.device("cuda", 0)
    B, Hq, Hkv, D, L = a.batch, a.heads, a.kv_heads, a.head_dim, a.length
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, Hq, D, device=dev, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
    n = torch.full((B,), L, dtype=torch.int32, device=dev)
    nbytes = 2 * kc.numel() * kc.element_size()
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    res = {"shape": {"B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "len": L}, "kv_bytes": nbytes, "iters": a.iters,
           "device": torch.cuda.get_device_name(dev)}
    med, lo, hi = _median_ms(lambda: dst.copy_(src), a.warmup, a.iters)
    res["copy"] = {"median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2),
                   "read_GBps": round(nbytes / med / 1e6, 1)}
    res["attn_decode"] = {}
    for split in (a.split_keys or [decode.SPLIT_KEYS_DEFAULT]):
        med, lo, hi = _median_ms(lambda: decode.attn_decode(q, kc, vc, n, split_keys=split, max_len=L), a.warmup, a.iters)
        res["attn_decode"][str(split)] = {"median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2),
                                          "max_us": round(hi * 1e3, 2), "read_GBps": round(nbytes / med / 1e6, 1),
                                          "of_copy": round(res["copy"]["median_us"] / (med * 1e3), 3)}
    # the copy again after the kernel runs: the spread between the two copy figures is the noise of this run
    med, lo, hi = _median_ms(lambda: dst.copy_(src), 2, a.iters)
    res["copy_again"] = {"median_us": round(med * 1e3, 2), "read_GBps": round(nbytes / med / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
