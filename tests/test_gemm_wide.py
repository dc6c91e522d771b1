"""The 65-to-128-row GEMM on the CPU tier: what csrc/hip/gemm_wide_shapes.h
takes, asked through toa_gemm_wide_check as ops/gemm.py asks it, and the
model with ``gemm="wide"``."""
import pytest
import torch

import test_decode as td
from tf_operator_amd.ops import _lib, gemm

BF16 = torch.bfloat16
KC, KG, SPC, KSTEP, WG_ROWS, MIN_CHUNKS, MAX_M = (_lib.call_ret("toa_gemm_wide_constant", i) for i in range(7))
SPLIT_K = 2 * MIN_CHUNKS * KC - KC + 8     # the least K that splits at N = 16 (tests/test_gemm_wide_gpu.py)


def _z(*shape):
    return torch.zeros(*shape, dtype=BF16)


def test_the_header_check_through_python():
    w, wgu = _z(48, 520), _z(96, 520)
    for M, taken in ((64, False), (65, True), (128, True), (129, False)):
        for sw, ww in ((False, w), (True, wgu)):
            r = gemm.wide_reason(_z(M, 520), ww, sw)
            assert (r == 0) == taken, (M, sw, r)
            if not taken:
                assert gemm.wide_why(r) == "M (rows) outside 65 .. 128"
                assert gemm.wide_why(r) in gemm.wide_refusal(_z(M, 520), ww, sw)
                with pytest.raises(ValueError, match="toa_gemm_wide.*outside 65 .. 128"):
                    (gemm.swiglu_wide if sw else gemm.linear_wide)(_z(M, 520), ww)
    x = _z(80, 520)
    assert gemm.wide_refusal(x, w) == "" == gemm.wide_refusal(x, wgu, swiglu=True)
    assert not gemm.wide_takes(x, w)                      # CPU tensors: the reference, not the kernel
    cases = {
        "N (F) not a positive multiple of 16": (x, w[:8], False),
        "K not a positive multiple of 8": (x[:, :12], w[:, :12], False),
        "row stride under the row or not a multiple of 8": (_z(80, 12)[:, :8], _z(48, 8), False),
        "base address null or not 16-byte aligned": (_z(80 * 520 + 1)[1:].view(80, 520), w, False),
        "W has fewer than N rows (SwiGLU: not 2F rows)": (x, _z(97, 520), True),
    }
    for words, (xx, ww, sw) in cases.items():
        r = gemm.wide_reason(xx, ww, sw)
        assert r != 0 and gemm.wide_why(r) == words, (words, gemm.wide_why(r))
        assert gemm.wide_refusal(xx, ww, sw).startswith(words)            # the launcher's own words
    # a caller's misaligned workspace is refused where K splits, and only there
    xs, ws_ = _z(80, SPLIT_K), _z(16, SPLIT_K)
    bad = torch.zeros(1024, dtype=torch.float32)[1:]
    assert _lib.call_ret("toa_gemm_wide_split", 16, SPLIT_K) == 2 == 2 * _lib.call_ret("toa_gemm_wide_split", 16, SPLIT_K - KC)
    assert gemm.wide_reason(xs, ws_) == 0 == gemm.wide_reason(x, w, ws=bad)
    assert gemm.wide_why(gemm.wide_reason(xs, ws_, ws=bad)) == "split-K workspace null or not 16-byte aligned"
    assert _lib.call_ret("toa_gemm_wide_ws_bytes", 16, SPLIT_K) == 2 * MAX_M * 16 * 4
    assert _lib.call_ret("toa_gemm_wide_swiglu_ws_bytes", 16, SPLIT_K) == 2 * 2 * MAX_M * 16 * 4
    assert _lib.call_ret("toa_gemm_wide_ws_bytes", 16, SPLIT_K - KC) == 0


def _extend(m, tokens, name):
    gemm.reset_fallbacks()
    cache = m.new_cache(tokens.shape[0], tokens.shape[1])
    out = m.extend(tokens, cache, gemm=name, logits="all")
    counted = {k: v for k, v in gemm.fallbacks().items() if k.startswith("decode")}
    gemm.reset_fallbacks()
    return out, counted


def test_extend_of_eighty_rows_counts_no_fallback_and_matches_tile():
    f = td._fixture()
    m = f["model"]
    tokens = torch.randint(0, m.cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(11))
    tile, none = _extend(m, tokens, "tile")
    wide, counted = _extend(m, tokens, "wide")
    assert none == {} and counted == {}, counted
    e = td._row_dev(wide, tile, tile)
    print(f"wide extend vs tile: {e:.3e} of a row's norm (limit {f['tol']:.3e})")
    assert wide.shape == (2, 40, m.cfg.vocab_size) and e <= f["tol"]
    _, stream = _extend(m, tokens, "stream")
    assert stream and all(k.startswith("decode 80x") and k.endswith("-> tile") for k in stream), stream
