"""The 17-to-64-row GEMM on the CPU tier: what csrc/hip/gemm_stream_shapes.h
takes, asked through toa_gemm_stream_check as ops/gemm.py asks it, and the
model with ``gemm="stream"``."""
import pytest
import torch

import test_decode as td
from tf_operator_amd.ops import _lib, gemm
from tf_operator_amd.ops import decode as dec

BF16 = torch.bfloat16
KC, KG, SPC, KSTEP, WG_N, MIN_CHUNKS, MAX_M = (_lib.call_ret("toa_gemm_stream_constant", i) for i in range(7))
SPLIT_K = 2 * MIN_CHUNKS * KC - KC + 8     # the least K that splits at N = 16 (tests/test_gemm_stream_gpu.py)


def _z(*shape):
    return torch.zeros(*shape, dtype=BF16)


def test_the_header_check_through_python():
    w, wgu = _z(48, 520), _z(96, 520)
    for M, taken in ((16, False), (17, True), (64, True), (65, False)):
        for sw, ww in ((False, w), (True, wgu)):
            r = gemm.stream_reason(_z(M, 520), ww, sw)
            assert (r == 0) == taken, (M, sw, r)
            if not taken:
                assert gemm.stream_why(r) == "M (rows) outside 17 .. 64"
                assert gemm.stream_why(r) in gemm.stream_refusal(_z(M, 520), ww, sw)
                with pytest.raises(ValueError, match="toa_gemm_stream.*outside 17 .. 64"):
                    (gemm.swiglu_stream if sw else gemm.linear_stream)(_z(M, 520), ww)
    x = _z(20, 520)
    assert gemm.stream_refusal(x, w) == "" == gemm.stream_refusal(x, wgu, swiglu=True)
    assert not gemm.stream_takes(x, w)                    # CPU tensors: the reference, not the kernel
    cases = {
        "N (F) not a positive multiple of 16": (x, w[:8], False),
        "K not a positive multiple of 8": (x[:, :12], w[:, :12], False),
        "row stride under the row or not a multiple of 8": (_z(20, 12)[:, :8], _z(48, 8), False),
        "base address null or not 16-byte aligned": (_z(20 * 520 + 1)[1:].view(20, 520), w, False),
        "W has fewer than N rows (SwiGLU: not 2F rows)": (x, _z(97, 520), True),
    }
    for words, (xx, ww, sw) in cases.items():
        r = gemm.stream_reason(xx, ww, sw)
        assert r != 0 and gemm.stream_why(r) == words, (words, gemm.stream_why(r))
        assert gemm.stream_refusal(xx, ww, sw).startswith(words)          # the launcher's own words
    # a caller's misaligned workspace is refused where K splits, and only there
    xs, ws_ = _z(20, SPLIT_K), _z(16, SPLIT_K)
    bad = torch.zeros(1024, dtype=torch.float32)[1:]
    assert _lib.call_ret("toa_gemm_stream_split", 16, SPLIT_K) == 2 == 2 * _lib.call_ret("toa_gemm_stream_split", 16, SPLIT_K - KC)
    assert gemm.stream_reason(xs, ws_) == 0 == gemm.stream_reason(x, w, ws=bad)
    assert gemm.stream_why(gemm.stream_reason(xs, ws_, ws=bad)) == "split-K workspace null or not 16-byte aligned"
    assert _lib.call_ret("toa_gemm_stream_ws_bytes", 16, SPLIT_K) == 2 * MAX_M * 16 * 4
    assert _lib.call_ret("toa_gemm_stream_swiglu_ws_bytes", 16, SPLIT_K) == 2 * 2 * MAX_M * 16 * 4
    assert _lib.call_ret("toa_gemm_stream_ws_bytes", 16, SPLIT_K - KC) == 0


def _extend(m, tokens, name):
    gemm.reset_fallbacks()
    cache = m.new_cache(tokens.shape[0], 8)
    out = m.extend(tokens, cache, gemm=name, logits="all")
    counted = {k: v for k, v in gemm.fallbacks().items() if k.startswith("decode")}
    gemm.reset_fallbacks()
    return out, counted


def test_extend_of_twenty_rows_counts_no_fallback_and_matches_tile(monkeypatch):
    f = td._fixture()
    m = f["model"]
    tokens = torch.randint(0, m.cfg.vocab_size, (5, 4), generator=torch.Generator().manual_seed(11))
    tile, none = _extend(m, tokens, "tile")
    stream, counted = _extend(m, tokens, "stream")
    assert none == {} and counted == {}, counted
    e = td._row_dev(stream, tile, tile)
    print(f"stream extend vs tile: {e:.3e} of a row's norm (limit {f['tol']:.3e})")
    assert stream.shape == (5, 4, m.cfg.vocab_size) and e <= f["tol"]
    _, skinny = _extend(m, tokens, "skinny")
    assert skinny and all(k.startswith("decode 20x") and k.endswith("-> tile") for k in skinny), skinny
    monkeypatch.setenv("TOA_DECODE_GEMM", "stream")
    assert dec.check_gemm(None) == "stream"
    monkeypatch.setenv("TOA_DECODE_GEMM", "bogus")
    with pytest.raises(ValueError, match="TOA_DECODE_GEMM"):
        dec.check_gemm(None)
