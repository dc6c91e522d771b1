"""Element-wise numerics of the 1-to-16-row GEMM (csrc/hip/gemm_skinny.hip
through ops/gemm.py linear_skinny / swiglu_skinny): inputs, the fp64
reference, the bound and the shapes of the GPU tests.  A plain helper module:
no fixtures, imported by tests/test_gemm_skinny.py (CPU) and
tests/test_gemm_skinny_gpu.py.

The bound, per element of y = x w^T with bf16 operands, fp32 accumulation and
one rounding to bf16:

* products of two bf16 values are exact in fp32;
* a sum of K fp32 terms in any order is within gamma = K 2^-24 sum_k |x_k w_k|
  of the exact sum, to first order;
* one rounding to bf16 adds 2^-8 |y|.

So an element passes at |y - y64| <= 2^-8 |y64| + (1 + 2^-8) gamma.

SwiGLU, s = silu(g) u with g = x wg^T, u = x wu^T taken from the fp32
accumulators: gamma_g and gamma_u go through ds/dg and ds/du evaluated in fp64
(tests/rowwise_numerics.py swiglu_ref64 with dout = 1: its dg and du ARE the
two derivatives), the fp32 evaluation of silu(g) u itself is given that
module's cap for an fp32 result, 8 units of 2^-24 of |s|, and the one
rounding to bf16 adds 2^-8 |s|:

    |s - s64| <= 2^-8 |s64| + (1 + 2^-8) (|ds/dg| gamma_g + |ds/du| gamma_u + 8 x 2^-24 |s64|)
"""
import functools

import torch

import rowwise_numerics as rn

# ---- the kernel's constants, restated from csrc/hip/gemm_skinny_shapes.h (tests/test_gemm_skinny.py holds them
# against the header's text)
MAX_M = 16     # rows of x
TILE_N = 16    # rows of W per workgroup (SwiGLU: a gate and an up tile)
KSTEP = 32     # k per MFMA
WAVES = 8      # waves per workgroup = K slices of its tile
UNROLL = 8     # k-steps per pass of the plain form (SwiGLU: UNROLL / 2)
MIN_WGS = 256  # fewer row tiles: K is split across workgroups, while every wave keeps UNROLL k-steps
MERGE_BLOCK = 256   # threads of the merge kernel, one per (row, four columns) (gemm_skinny.hip gemm_skinny_merge_kernel)

MS = (1, 2, 3, 7, 8, 9, 15, 16)

# (N, K); F takes N's place in the SwiGLU form.
BASE = [(16, 8), (16, 40), (48, 520)]
# (b) every wave's slice runs its loop at least twice, the last pass partial: WAVES slices of UNROLL + 1 k-steps
#     (plain: one whole pass and one k-step; SwiGLU, UNROLL / 2 steps a pass: two whole passes and one k-step), the
#     last k-step holding one 8-column chunk.  From WAVES, UNROLL, KSTEP; under 2 WAVES UNROLL k-steps, so no split.
CASE_B = (TILE_N, WAVES * (UNROLL + 1) * KSTEP - 24)                      # (16, 2280)
# (c) at least one wave with an empty slice: fewer k-steps than WAVES.  K = 40 of BASE has 2 k-steps (six empty
#     waves); K = 520 has 17, 3 a slice, so waves 6 and 7 are empty and wave 5 has 2.  From WAVES, KSTEP.
CASE_C = (TILE_N, 40)
# (d) a cross-workgroup split with more than one piece: under MIN_WGS row tiles and 2 WAVES UNROLL k-steps, the
#     least K that splits (two pieces, UNROLL k-steps a wave), again ending in one 8-column chunk.  From MIN_WGS,
#     WAVES, UNROLL, KSTEP.
CASE_D = (TILE_N, 2 * WAVES * UNROLL * KSTEP - 24)                        # (16, 4072)
# (a) a partial last workgroup.  The GEMM kernel has none: a workgroup is one whole row tile and TILE_N divides N.
#     The merge kernel of a split launch has one whenever M N / 4 is no multiple of MERGE_BLOCK: always at N = 16
#     (at most 64 threads of its only workgroup); N = 80 at M = 16 is 320 threads, a whole workgroup and a partial
#     one, and 5 row tiles.  From TILE_N, MERGE_BLOCK and (d)'s K.
CASE_A = (5 * TILE_N, CASE_D[1])                                          # (80, 4072)
SHAPES = BASE + [CASE_A, CASE_B, CASE_D]    # CASE_C is BASE[1]
INVARIANCE_SHAPES = [CASE_B, CASE_D]


def split_of(N, K):
    """gemm_skinny_shapes.h split(N, K), restated for the planted errors and the CPU tests."""
    ksteps = -(-K // KSTEP)
    s = 1
    while s < 8 and (N // TILE_N) * s < MIN_WGS and ksteps // (2 * s * WAVES) >= UNROLL:
        s *= 2
    return s


def slice_steps(N, K):
    slices = split_of(N, K) * WAVES
    ksteps = -(-K // KSTEP)
    return -(-ksteps // slices)


@functools.lru_cache(maxsize=None)
def inputs(N, K, swiglu=False, seed=0):
    """x [16, K] and w [N, K] (SwiGLU: gate | up [2N, K]) bf16 on the CPU: x
    randn, w randn / sqrt(K), so the results are of order one.  Read-only."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + K + int(swiglu))
    x = torch.randn(MAX_M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn((2 if swiglu else 1) * N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    return x, w


def linear_ref64(x, w):
    """(y64, bound) of y = x w^T, each [M, N] fp64."""
    y = x.double() @ w.double().t()
    gamma = x.shape[1] * rn.U32 * (x.double().abs() @ w.double().abs().t())
    return y, 2.0 ** -8 * y.abs() + (1 + 2.0 ** -8) * gamma


def swiglu_ref64(x, wgu):
    """(s64, bound) of s = silu(x wg^T) (x wu^T), each [M, F] fp64."""
    F = wgu.shape[0] // 2
    gu = x.double() @ wgu.double().t()
    gamma = x.shape[1] * rn.U32 * (x.double().abs() @ wgu.double().abs().t())
    r = rn.swiglu_ref64(gu, torch.ones(x.shape[0], F, dtype=torch.float64))   # dout = 1: dg = ds/dg, du = ds/du
    lin = r.dg.abs() * gamma[:, :F] + r.du.abs() * gamma[:, F:] + 8 * rn.U32 * r.mag_out
    return r.out, 2.0 ** -8 * r.mag_out + (1 + 2.0 ** -8) * lin


@functools.lru_cache(maxsize=None)
def reference(N, K, swiglu=False):
    """(x, w, ref64, bound) at 16 rows; a launch of M rows is held against the first M (a row depends on itself only)."""
    x, w = inputs(N, K, swiglu)
    return (x, w) + (swiglu_ref64(x, w) if swiglu else linear_ref64(x, w))


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound, and where; non-finite results count as infinitely off."""
    e = (got.double() - ref).abs() / bound
    e = torch.where(torch.isfinite(got.double()), e, torch.full_like(e, float("inf")))
    i = int(e.flatten().argmax())
    return float(e.flatten()[i]), (i // e.shape[1], i % e.shape[1])


def ok(got, ref, bound):
    return worst(got, ref, bound)[0] <= 1.0


def check(what, got, ref, bound):
    """Print the worst element's share of its bound, then assert every element is inside."""
    e, at = worst(got, ref, bound)
    print(f"skinny {what}: worst element at {e:.3f} of its bound, {at}")
    assert e <= 1.0, f"{what}: element {at} is at {e:.2f} x its bound"
    return e
