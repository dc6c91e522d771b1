"""Decode projections on MXFP4 weights, the CPU tier (csrc/hip/gemm_w4.hip through ops/gemm.py and
Llama.decode_step(weights=)): the quantiser's formula against a scalar restatement, the GPU tests' shapes
against the launch plan, the reference inside the bound, the model on a snapshot."""
import math

import pytest
import torch

import decode_numerics as dn
import skinny_numerics as sn
from tf_operator_amd.ops import _lib, gemm

BF16 = torch.bfloat16
KSTEP, BLOCK, WAVES, UNROLL, MAX_SPLIT, TILE_N, TILES, MERGE_BLOCK, SCALE_ALIGN, MAX_M, TILES_FEW, MIN_WGS = (
    _lib.call_ret("toa_gemm_skinny_w4_constant", i) for i in range(12))
K_SPLITS = (2 * WAVES * UNROLL - 1) * KSTEP + BLOCK
# (N, K), F in N's place for SwiGLU; each the smallest that reaches its path, from gemm_w4_shapes.h's constants
SHAPES = {
    "a": (TILE_N, BLOCK),                    # K under one k-step; one tile of the only workgroup's two
    # (c) fewer k-steps than waves, the last of one block; five row tiles, two a workgroup: a short last workgroup
    "c": (5 * TILE_N, (WAVES - 3) * KSTEP + BLOCK),
    # (f) the least row count with four tiles a workgroup that leaves a short last workgroup in both forms
    "f": ((MIN_WGS * TILES + 1) * TILE_N, KSTEP + BLOCK),
    # (b) every wave two whole passes and one k-step more, the last of one block, at the largest split
    "b": (TILE_N, (MAX_SPLIT * WAVES * (2 * UNROLL + 1) - 1) * KSTEP + BLOCK),
    "d": (TILE_N, K_SPLITS),                 # the least K that splits across workgroups
    "e": (5 * TILE_N, K_SPLITS),             # at M = 16 the merge runs a whole workgroup and a partial one
}
MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# the block with amax 6: every tie in both signs, then 0.5 and -6, and the codes the rule gives them
TIES = [6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5, .5, -6]
TIE_CODES = [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 1, 15]


def quant_scalar(w):
    """(q, X) of w [N, K] by the issue's rule, one Python float at a time."""
    N, K = w.shape
    q, X = torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N, K // BLOCK, dtype=torch.uint8)
    for n in range(N):
        for b in range(K // BLOCK):
            vals = [float(v) for v in w[n, b * BLOCK:(b + 1) * BLOCK].float()]
            amax = max(abs(v) for v in vals)
            e = 0
            if amax > 0 and math.isfinite(amax):
                m, E = math.frexp(amax)     # amax = m 2^E, 0.5 <= m < 1
                e = max(-100, min(100, E - 3 if m <= 0.75 else E - 2))
            X[n, b] = e + 127 if math.isfinite(amax) else 0xff
            for i, v in enumerate(vals):
                a = abs(v) * 2.0 ** -e
                # the nearest magnitude, a tie to the even code, anything beyond 6 to 6
                code = 7 if a > 6 else min(range(8), key=lambda c: (abs(a - MAGS[c]), c % 2))
                q[n, (b * BLOCK + i) // 2] |= (code | (8 if math.copysign(1, v) < 0 else 0)) << (4 * (i % 2))
    return q, X


def planted(K, seed=0):
    """randn / sqrt(K) rows [9, K] bf16 with the issue's blocks planted in the first block of rows 0 .. 7."""
    w = (torch.randn(9, K, generator=torch.Generator().manual_seed(seed)) / K ** 0.5).to(BF16)
    w[0, :BLOCK] = 0
    w[1:3, :BLOCK] = w[1:3, :BLOCK].clamp(-1, 1)
    w[1, 3], w[2, 3] = 1.5 * 2.0 ** 3, 1.5078125 * 2.0 ** 3       # 1.5 2^E and the next bf16 above it, E = 3
    w[3, :BLOCK] = 0
    w[3, :len(TIES)] = torch.tensor(TIES)
    w[4] = (w[4].float() * 2.0 ** 40).to(BF16)
    w[5] = (w[5].float() * 2.0 ** 118).to(BF16)                   # e meets its clamp: the elements saturate
    w[6] = (w[6].float() * 2.0 ** -112).to(BF16)                  # and the other clamp
    w[7, 5] = float("inf")
    return w


def w4_reference(N, K, swiglu):
    """(x, q, scale, ref64, bound) at 16 rows on sn.inputs: q by the CPU formula, every other block's scale byte + 1,
    so a scale read from the wrong block is off by a factor of 2.  Reference and bound: skinny_numerics' on deq."""
    x, w = sn.inputs(N, K, swiglu)
    q, scale = gemm.quantize_w4(w)   # scale: this call's own, a view of rows padded to SCALE_ALIGN
    scale[:, 1::2] += 1
    deq = gemm.dequantize_w4(q, scale)
    return (x, q, scale) + (sn.swiglu_ref64(x, deq) if swiglu else sn.linear_ref64(x, deq))


def snapped_model(preset, device, dtype):
    """The preset's model with each block's four projections replaced by their fp4 round trip: fp4 is lossless for it."""
    from tf_operator_amd.models.llama import PRESETS, W8_NAMES, Llama

    m = Llama(PRESETS[preset], device=device, dtype=dtype)
    m.init_weights(0)
    with torch.no_grad():
        for blk in m.blocks:
            for n in W8_NAMES:
                p = getattr(blk, n)
                p.copy_(gemm.dequantize_w4(*gemm.quantize_w4(p.to(BF16))))
    return m.eval()


def test_the_shapes_reach_their_paths():
    plan = lambda n, k: (_lib.call_ret("toa_gemm_skinny_w4_split", n, k), _lib.call_ret("toa_gemm_skinny_w4_slice_steps", n, k))
    assert plan(*SHAPES["a"]) == (1, 1) and plan(*SHAPES["c"]) == (1, 1) and -(-SHAPES["c"][1] // KSTEP) < WAVES
    four = lambda rows: -(-(rows // TILE_N) // TILES) >= MIN_WGS    # gemm_w4_shapes.h tiles(rows) == TILES
    assert [c for c, (n, _) in SHAPES.items() if four(n)] == ["f"]
    assert (SHAPES["c"][0] // TILE_N) % TILES_FEW == 1 and (SHAPES["f"][0] // TILE_N) % TILES == 1
    assert plan(*SHAPES["b"]) == (MAX_SPLIT, 2 * UNROLL + 1)
    for rows in (SHAPES["d"][0], 2 * SHAPES["d"][0], SHAPES["e"][0], 2 * SHAPES["e"][0]):
        assert plan(rows, K_SPLITS) == (2, UNROLL) and plan(rows, K_SPLITS - BLOCK)[0] == 1
    assert (MAX_M * SHAPES["e"][0] // 4) % MERGE_BLOCK not in (0, MAX_M * SHAPES["e"][0] // 4)
    assert all(k % KSTEP == BLOCK for _, k in SHAPES.values())


@pytest.mark.parametrize("K", [32, 96])
def test_quantize_on_the_cpu_is_the_rule(K):
    w = planted(K)
    q, scale = gemm.quantize_w4(w)
    q_ref, x_ref = quant_scalar(w)
    assert q.shape == (9, K // 2) and scale.shape == (9, K // BLOCK) and scale.stride(0) % SCALE_ALIGN == 0
    assert torch.equal(scale, x_ref) and torch.equal(q, q_ref)
    assert scale[:8, 0].tolist() == [127, 128, 129, 127, int(scale[4, 0]), 227, 27, 0xff] and 160 <= scale[4, 0] <= 168
    assert (scale[7] == 0xff).tolist() == [True] + [False] * (K // BLOCK - 1)
    assert torch.stack((q[3] & 15, q[3] >> 4), 1).flatten()[:len(TIES)].tolist() == TIE_CODES
    assert set((q[5, :BLOCK // 2] & 7).tolist()) == {7}   # saturated at +-6
    deq = gemm.dequantize_w4(q, scale)
    assert deq[3, :len(TIES)].tolist() == [math.copysign(MAGS[c & 7], -1 if c & 8 else 1) for c in TIE_CODES]
    assert torch.isnan(deq[7, :BLOCK]).all() and torch.isfinite(deq[7, BLOCK:]).all() and torch.isfinite(deq[:7]).all()


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_cpu_reference_is_inside_the_bound(case, swiglu):
    N, K = SHAPES[case]
    x, q, scale, ref, bound = w4_reference(N, K, swiglu)
    got = (gemm.swiglu_skinny_w4 if swiglu else gemm.linear_skinny_w4)(x, q, scale)
    assert got.shape == (16, N) and got.dtype == BF16
    sn.check(f"cpu w4 {'swiglu' if swiglu else 'plain'} {case} N={N} K={K}", got, ref, bound)


def test_the_model_on_a_snapshot():
    from tf_operator_amd.train.generate import generate

    f = dn.fixture(24)
    m, tokens = snapped_model("llama-tiny", "cpu", torch.float32), f["tokens"]
    snap = m.quantize_projections(fmt="fp4")
    with torch.no_grad():
        full, ref = m(tokens), dn.forward64(m, tokens)
        cache = m.new_cache(2, 24)
        gemm.reset_fallbacks()
        got = [m.prefill(tokens[:, :5], cache, gemm="skinny", weights=snap)]
        got += [m.decode_step(tokens[:, t], cache, gemm="skinny", weights=snap) for t in range(5, 24)]
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    e = dn.row_dev(torch.stack(got, 1), full[:, 4:], ref[:, 4:])
    print(f"fp4 decode on snapped weights vs full forward: {e:.3e} (limit {f['tol']:.3e})")
    assert e <= f["tol"]
    a, _ = generate(m, tokens[:, :5], 6, gemm="skinny", weights="fp4")
    b, _ = generate(m, tokens[:, :5], 6, gemm="skinny", weights=snap)
    assert torch.equal(a, b)
    # 17 rows: no fp4 kernel yet, so they are counted and run on the bf16 weight
    out = {}
    for weights in (None, snap):
        gemm.reset_fallbacks()
        out[weights is None] = m.extend(tokens[:1, :17], m.new_cache(1, 17), gemm="stream", logits="all", weights=weights)
    counted = [k for k in gemm.fallbacks() if k.startswith("decode")]
    gemm.reset_fallbacks()
    assert counted and all(k.startswith("decode-fp4 17x") and k.endswith("-> bf16 stream") for k in counted), counted
    assert torch.equal(out[True], out[False])
