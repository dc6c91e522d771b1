"""Decode projections on fp8 weights, the CPU tier (csrc/hip/gemm_w8.hip through
ops/gemm.py quantize_w8 / linear_skinny_w8 / swiglu_skinny_w8 and
Llama.decode_step(weights=)): the quantiser's formula, the shapes of the GPU
tests against the launch plan, the reference inside the bound, the model on a
snapshot.  tests/test_gemm_w8_gpu.py imports the helpers."""
import math

import pytest
import torch

import decode_numerics as dn
import rowwise_numerics as rn
import skinny_numerics as sn
from tf_operator_amd.ops import _lib, gemm

BF16, E4M3 = torch.bfloat16, torch.float8_e4m3fn
KSTEP, CHUNK, WAVES, UNROLL, MAX_SPLIT, TILE_N, TILES, MERGE_BLOCK, QUANT_LDS_K, MAX_M = (
    _lib.call_ret("toa_gemm_skinny_w8_constant", i) for i in range(10))
# (N, K), F in N's place for SwiGLU; each the smallest that reaches its path, from gemm_w8_shapes.h's constants
SHAPES = {
    "a": (TILE_N, CHUNK),                    # K under one k-step; one tile in the plain form's only workgroup
    # (c) fewer k-steps than waves: six, the last of one chunk; (e) three row tiles: a pair and a single
    "c": (3 * TILE_N, 5 * KSTEP + CHUNK),
    # (b) every wave two whole passes and one k-step more, the last of one chunk; at N = 16 that many k-steps are
    #     split MAX_SPLIT ways (the split stops only there), so MAX_SPLIT WAVES slices of 2 UNROLL + 1 k-steps
    "b": (TILE_N, (MAX_SPLIT * WAVES * (2 * UNROLL + 1) - 1) * KSTEP + CHUNK),
    # (d) the least K that splits across workgroups: 2 WAVES UNROLL k-steps, the last of one chunk
    "d": (TILE_N, (2 * WAVES * UNROLL - 1) * KSTEP + CHUNK),
    # (e) five row tiles at (d)'s K: at M = 16 the merge runs a whole workgroup and a partial one
    "e": (5 * TILE_N, (2 * WAVES * UNROLL - 1) * KSTEP + CHUNK),
}


def exponent(amax: float) -> int:
    """The issue's rule: the least e with amax <= 448 * 2^e from amax = m 2^E, 1 <= m < 2; 0 for 0; clamped."""
    if amax == 0:
        return 0
    m, E = math.frexp(amax)     # amax = m 2^E, 0.5 <= m < 1
    return max(-100, min(100, E - 1 - 8 if 2 * m <= 1.75 else E - 1 - 7))


def quant_ref(w):
    """(q, scale, e) of w [N, K] by the CPU formula."""
    e = torch.tensor([exponent(float(a)) for a in w.float().abs().amax(1)])
    return (w.float() * (2.0 ** -e.double()).float()[:, None]).to(E4M3), (2.0 ** e.double()).float(), e


def planted(N, K, seed=0):
    """randn / sqrt(K) rows [N >= 5, K >= 16] bf16 with the issue's rows planted at 0 .. 4; (w, e of rows 0 .. 2)."""
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) / K ** 0.5).to(BF16)
    w[0] = 0
    w[1:3] = w[1:3].clamp(-1, 1)
    w[1, 3], w[2, 3] = 1.75 * 2.0 ** 3, 1.7578125 * 2.0 ** 3       # 1.75 2^E and the next bf16 above it, E = 3
    # amax 448, so e = 0: e4m3 subnormals (units of 2^-9), ties among them and among normals, both signs
    w[3, :16] = torch.tensor([448, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, -2.0 ** -10, -3 * 2.0 ** -10,
                              7 * 2.0 ** -10, 1.0625, 1.1875, -1.0625, 2.0 ** -11, 15 * 2.0 ** -10, 17 * 2.0 ** -10,
                              -2.0 ** -9, 0.0])
    w[3, 16:] = 0
    w[4] = (w[4].float() * 2.0 ** 40).to(BF16)
    return w, [0, 3 - 8, 3 - 7]


def w8_reference(N, K, swiglu):
    """(x, q, scale, ref64, bound) at 16 rows on sn.inputs: q by the CPU formula, odd rows' scales x 1.25.  The
    bound is skinny_numerics' with gamma scaled by |scale| and 2^-24 |y64| more for the fp32 multiply."""
    x, w = sn.inputs(N, K, swiglu)
    q, scale, _ = quant_ref(w)
    scale = scale.clone()
    scale[1::2] *= 1.25
    s64 = scale.double()
    y = (x.double() @ q.double().t()) * s64
    gamma = K * rn.U32 * (x.double().abs() @ q.double().abs().t()) * s64 + rn.U32 * y.abs()
    if not swiglu:
        return x, q, scale, y, 2.0 ** -8 * y.abs() + (1 + 2.0 ** -8) * gamma
    r = rn.swiglu_ref64(y, torch.ones(x.shape[0], N, dtype=torch.float64))
    lin = r.dg.abs() * gamma[:, :N] + r.du.abs() * gamma[:, N:] + 8 * rn.U32 * r.mag_out
    return x, q, scale, r.out, 2.0 ** -8 * r.mag_out + (1 + 2.0 ** -8) * lin


def snapped_model(preset, device, dtype):
    """The preset's model with each block's four projections replaced by their fp8 round trip: fp8 is lossless for it."""
    from tf_operator_amd.models.llama import PRESETS, W8_NAMES, Llama

    m = Llama(PRESETS[preset], device=device, dtype=dtype)
    m.init_weights(0)
    with torch.no_grad():
        for blk in m.blocks:
            for n in W8_NAMES:
                p = getattr(blk, n)
                p.copy_(gemm.dequantize_w8(*gemm.quantize_w8(p.to(BF16))))
    return m.eval()


def test_the_shapes_reach_their_paths():
    plan = lambda n, k: (_lib.call_ret("toa_gemm_skinny_w8_split", n, k), _lib.call_ret("toa_gemm_skinny_w8_slice_steps", n, k))
    assert plan(*SHAPES["a"]) == (1, 1) and plan(*SHAPES["c"]) == (1, 1) and -(-SHAPES["c"][1] // KSTEP) < WAVES
    assert plan(*SHAPES["b"]) == (MAX_SPLIT, 2 * UNROLL + 1)
    for rows in (SHAPES["d"][0], 2 * SHAPES["d"][0], SHAPES["e"][0]):
        assert plan(rows, SHAPES["d"][1]) == (2, UNROLL) and plan(rows, SHAPES["d"][1] - CHUNK)[0] == 1
    assert (MAX_M * SHAPES["e"][0] // 4) % MERGE_BLOCK not in (0, MAX_M * SHAPES["e"][0] // 4)
    assert all(k % KSTEP == CHUNK for _, k in SHAPES.values())


@pytest.mark.parametrize("K", [16, 48])
def test_quantize_on_the_cpu_is_the_formula(K):
    w, want_e = planted(9, K)
    q, scale = gemm.quantize_w8(w)
    q_ref, s_ref, e = quant_ref(w)
    assert e[:3].tolist() == want_e
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(scale, s_ref)
    assert q[3, :8].float().tolist() == [448, 2.0 ** -9, 0, 2.0 ** -8, 2.0 ** -8, 0, -2.0 ** -8, 2.0 ** -7]   # ties to even
    assert torch.equal(gemm.dequantize_w8(q, scale).float(), q.float() * scale[:, None])
    w[5, 1] = float("inf")
    assert torch.isnan(gemm.quantize_w8(w)[1]).tolist() == [i == 5 for i in range(9)]


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_cpu_reference_is_inside_the_bound(case, swiglu):
    N, K = SHAPES[case]
    x, q, scale, ref, bound = w8_reference(N, K, swiglu)
    got = (gemm.swiglu_skinny_w8 if swiglu else gemm.linear_skinny_w8)(x, q, scale)
    assert got.shape == (16, N) and got.dtype == BF16
    sn.check(f"cpu w8 {'swiglu' if swiglu else 'plain'} {case} N={N} K={K}", got, ref, bound)


def test_decode_step_on_a_snapshot_within_the_teacher_forcing_rule():
    f = dn.fixture(24)
    m, tokens = snapped_model("llama-tiny", "cpu", torch.float32), f["tokens"]
    snap = m.quantize_projections()
    with torch.no_grad():
        full, ref = m(tokens), dn.forward64(m, tokens)
        cache = m.new_cache(2, 24)
        gemm.reset_fallbacks()
        got = [m.prefill(tokens[:, :5], cache, gemm="skinny", weights=snap)]
        got += [m.decode_step(tokens[:, t], cache, gemm="skinny", weights=snap) for t in range(5, 24)]
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    e = dn.row_dev(torch.stack(got, 1), full[:, 4:], ref[:, 4:])
    print(f"fp8 decode on snapped weights vs full forward: {e:.3e} (limit {f['tol']:.3e})")
    assert e <= f["tol"]
    with pytest.raises(ValueError, match="tile"):
        m.decode_step(tokens[:, 0], cache, gemm="tile", weights=snap)
