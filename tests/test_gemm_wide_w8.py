"""The 65-to-128-row GEMM on fp8 weights, the CPU tier (csrc/hip/gemm_wide_w8.hip
through ops/gemm.py linear_wide_w8 / swiglu_wide_w8 and Llama.extend on a
snapshot): what csrc/hip/gemm_wide_w8_shapes.h takes, the shapes of the GPU
tests against the launch plan, the reference inside the bound, the model.
tests/test_gemm_wide_w8_gpu.py imports SHAPES, MS and reference."""
import functools

import pytest
import torch

import rowwise_numerics as rn
import skinny_numerics as sn
import test_decode as td
import test_gemm_w8 as w8
from tf_operator_amd.ops import _lib, gemm

BF16, E4M3 = torch.bfloat16, torch.float8_e4m3fn
KC, KG, SPC, KSTEP, WG_ROWS, MIN_CHUNKS, MAX_M, MIN_M, TILE_N, TILES, CHUNK, MERGE_BLOCK = (
    _lib.call_ret("toa_gemm_wide_w8_constant", i) for i in range(12))
SPLIT_K = (2 * MIN_CHUNKS - 1) * KC + CHUNK   # the least K that splits across workgroups (up to 128 workgroups)
MS = (65, 80, 96, 97, 113, 128)               # every MT = 5 .. 8 (96 is the one of MT = 6) and both ends
# (N, K), F in N's place for SwiGLU; each the smallest that reaches its path, from gemm_wide_w8_shapes.h's constants
SHAPES = {
    # one row tile (plain: the wave's second tile is not there), the workgroup's other row groups idle at the
    # barriers; K of one 16-column piece, so K group 1 has no work
    "idle-groups": (TILE_N, CHUNK),
    # a whole workgroup and a partial one; two whole chunks, so both LDS buffers are rewritten, then a predicated tail
    "two-wgs": (WG_ROWS + TILE_N, 2 * KC + CHUNK),
    # K group 0 with SPC whole k-steps, K group 1 with one lane group's 16 columns
    "uneven-groups": (TILE_N, SPC * KSTEP + CHUNK),
    # the workspace and the merge kernel; three row tiles, so the plain form's last wave owns one tile
    "split": (3 * TILE_N, SPLIT_K),
    # pieces of 2 MIN_CHUNKS + 1 chunks: the unpredicated prologue and loop, then the predicated one
    "steady": (TILE_N, (8 * (2 * MIN_CHUNKS + 1) - 1) * KC + CHUNK),
}


@functools.lru_cache(maxsize=None)
def reference(name, swiglu, seed=0):
    """(x [128, K], q, scale, ref64, bound) on the CPU, read-only: x randn, q by the CPU formula of randn / sqrt(K),
    odd rows' scales x 1.25; tests/test_gemm_stream_w8.py reference's bound at 128 rows."""
    N, K = SHAPES[name]
    g = torch.Generator().manual_seed(100 * seed + 7 * N + K + int(swiglu))
    x = torch.randn(MAX_M, K, generator=g).to(BF16)
    q, scale, _ = w8.quant_ref((torch.randn((2 if swiglu else 1) * N, K, generator=g) / K ** 0.5).to(BF16))
    scale = scale.clone()
    scale[1::2] *= 1.25
    s64 = scale.double()
    y = (x.double() @ q.double().t()) * s64
    gamma = K * rn.U32 * (x.double().abs() @ q.double().abs().t()) * s64 + rn.U32 * y.abs()
    if not swiglu:
        return x, q, scale, y, 2.0 ** -8 * y.abs() + (1 + 2.0 ** -8) * gamma
    r = rn.swiglu_ref64(y, torch.ones(MAX_M, N, dtype=torch.float64))
    lin = r.dg.abs() * gamma[:, :N] + r.du.abs() * gamma[:, N:] + 8 * rn.U32 * r.mag_out
    return x, q, scale, r.out, 2.0 ** -8 * r.mag_out + (1 + 2.0 ** -8) * lin


def _operands(M, rows, K):
    return torch.zeros(M, K, dtype=BF16), torch.zeros(rows, K, dtype=torch.uint8).view(E4M3), torch.ones(rows)


def _reason(x, q, scale, sw, ws=None, scale_ptr=None):
    N = q.shape[0] // 2 if sw else q.shape[0]
    return _lib.call_ret("toa_gemm_wide_w8_check", int(sw), x.data_ptr(), q.data_ptr(), x.data_ptr(),
                         x.data_ptr() if ws is None else ws.data_ptr(), scale.data_ptr() if scale_ptr is None else
                         scale_ptr, x.stride(0), q.stride(0), N, q.shape[0], x.shape[0], N, x.shape[1])


def test_the_header_check_through_python():
    for M, taken in ((64, False), (65, True), (128, True), (129, False)):
        for sw in (False, True):
            x, q, scale = _operands(M, 96 if sw else 48, 528)
            why = gemm.wide_w8_refusal(x, q, scale, sw)
            assert (why == "") == taken, (M, sw, why)
            if not taken:
                assert why.startswith("M (rows) outside 65 .. 128") and why.startswith(gemm.wide_w8_why(_reason(x, q, scale, sw)))
                with pytest.raises(ValueError, match="toa_gemm_wide_w8.*outside 65 .. 128"):
                    (gemm.swiglu_wide_w8 if sw else gemm.linear_wide_w8)(x, q, scale)
    x, q, scale = _operands(80, 48, 528)
    flat = torch.zeros(48 * 528 + 16, dtype=torch.uint8).view(E4M3)
    cases = {
        "N (F) not a positive multiple of 16": (x, q[:8], scale[:8], False),
        "K not a positive multiple of 16": (x[:, :24], q[:, :24], scale, False),
        "row stride under the row, or not a multiple of 16 bytes": (torch.zeros(80, 20, dtype=BF16)[:, :16], q[:, :16].contiguous(), scale, False),
        "base address null or not 16-byte aligned": (x, flat[1:1 + 48 * 528].view(48, 528), scale, False),
        "q has fewer than N rows (SwiGLU: not 2F rows)": _operands(80, 97, 528) + (True,),
    }
    for words, (xx, qq, ss, sw) in cases.items():
        assert gemm.wide_w8_refusal(xx, qq, ss, sw).startswith(words), (words, gemm.wide_w8_refusal(xx, qq, ss, sw))
    assert gemm.wide_w8_why(_reason(x, q, scale, False, scale_ptr=0)) == "scale null or not 4-byte aligned"
    assert gemm.wide_w8_refusal(x, q, scale[:47], False).startswith("scale ")          # the tensors' kind
    # a caller's misaligned workspace is refused where K splits, and only there
    xs, qs, ss = _operands(80, 16, SPLIT_K)
    bad = torch.zeros(1024)[1:]
    assert _reason(xs, qs, ss, False) == 0 == _reason(x, q, scale, False, ws=bad)
    assert gemm.wide_w8_why(_reason(xs, qs, ss, False, ws=bad)) == "split-K workspace null or not 16-byte aligned"
    assert _lib.call_ret("toa_gemm_wide_w8_ws_bytes", 16, SPLIT_K) == 2 * MAX_M * 16 * 4
    assert _lib.call_ret("toa_gemm_wide_w8_swiglu_ws_bytes", 16, SPLIT_K) == 2 * MAX_M * 32 * 4
    assert _lib.call_ret("toa_gemm_wide_w8_ws_bytes", 16, SPLIT_K - KC) == 0


def test_the_shapes_reach_their_paths():
    plan = lambda rows, k: (_lib.call_ret("toa_gemm_wide_w8_split", rows, k), _lib.call_ret("toa_gemm_wide_w8_piece_chunks", rows, k))
    assert (KC, WG_ROWS, MIN_M, MAX_M) == (KG * SPC * KSTEP, 4 * TILES * TILE_N, 65, 128) and KSTEP == 4 * CHUNK
    assert sorted({(M + 15) // 16 for M in MS}) == [5, 6, 7, 8] and (MS[0], MS[-1]) == (MIN_M, MAX_M)
    for form in (1, 2):   # rows of q = form x N
        assert plan(form * SHAPES["idle-groups"][0], SHAPES["idle-groups"][1]) == (1, 1) and CHUNK < KSTEP
        n, k = SHAPES["two-wgs"]
        assert plan(form * n, k) == (1, 3) and WG_ROWS < form * n and (form * n) % WG_ROWS and k % KC == CHUNK
        n, k = SHAPES["uneven-groups"]
        assert plan(form * n, k) == (1, 1) and SPC * KSTEP < k < KC
        n, k = SHAPES["split"]
        assert plan(form * n, k) == (2, MIN_CHUNKS) and plan(form * n, k - KC)[0] == 1 and (n // TILE_N) % TILES
        n, k = SHAPES["steady"]
        assert plan(form * n, k) == (8, 2 * MIN_CHUNKS + 1)


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_cpu_reference_is_inside_the_bound(name, swiglu):
    x, q, scale, ref, bound = reference(name, swiglu)
    got = (gemm.swiglu_wide_w8 if swiglu else gemm.linear_wide_w8)(x, q, scale)
    assert got.shape == (MAX_M, SHAPES[name][0]) and got.dtype == BF16
    sn.check(f"cpu wide w8 {'swiglu' if swiglu else 'plain'} {name}", got, ref, bound)


def test_extend_of_eighty_rows_on_a_snapshot_runs_fp8_under_wide_only():
    m, tol = w8.snapped_model("llama-tiny", "cpu", torch.float32), td._fixture()["tol"]
    snap = m.quantize_projections()
    tokens = torch.randint(0, m.cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(11))
    out = {}
    for name, weights in (("wide", None), ("wide", snap), ("stream", snap)):
        gemm.reset_fallbacks()
        out[name, weights is not None] = m.extend(tokens, m.new_cache(2, 40), gemm=name, logits="all", weights=weights)
        counted = {k: v for k, v in gemm.fallbacks().items() if k.startswith("decode")}
        if name == "wide":
            assert counted == {}, counted
        else:   # refused and counted, as before: the 17-to-64-row kernel stops at 64
            assert any(k.startswith("decode-fp8 80x") and k.endswith("-> bf16 stream") for k in counted), counted
    gemm.reset_fallbacks()
    e = td._row_dev(out["wide", True], out["wide", False], out["wide", False])
    print(f"fp8 wide extend vs bf16 wide: {e:.3e} of a row's norm (limit {tol:.3e})")
    assert out["wide", True].shape == (2, 40, m.cfg.vocab_size) and e <= tol
