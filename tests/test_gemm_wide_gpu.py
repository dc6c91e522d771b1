"""The 65-to-128-row GEMM on an MI355X (csrc/hip/gemm_wide.hip through
ops/gemm.py linear_wide / swiglu_wide and Llama.extend(gemm="wide")).

Every element against fp64 under the bound of tests/skinny_numerics.py (it
holds for any summation order), on strided operands with NaN around them and
a sentinel around the result; a row's bits independent of M, of its index and
of the launch before; refusals that launch nothing; the model by the
teacher-forcing rule of tests/decode_numerics.py."""
import functools

import pytest
import torch

import decode_numerics as dn
import skinny_numerics as sn

pytestmark = pytest.mark.gpu

DEV = dn.DEV
NAN = float("nan")
INVALID_VALUE = 1   # hipErrorInvalidValue
SENTINEL = 0x1234
BF16 = torch.bfloat16
TOTAL = 140         # the sequence of tests/test_extend_gpu.py: one teacher per preset for all its users
ROWS = 128          # the header's MAX_M


def _shapes():
    """(N, K), each the smallest that reaches one path of the kernel, from the header's constants."""
    KC, KG, SPC, KSTEP, WG_ROWS, MIN_CHUNKS, MAX_M = (dn.lib().call_ret("toa_gemm_wide_constant", i) for i in range(7))
    assert MAX_M == ROWS
    return {
        # one wave pair with one (plain) or two (SwiGLU) live tiles, the other row groups idle at the barriers of the
        # chunks and of the two-step merge; one chunk of one 8-column piece, K group 1 without work
        "idle-groups": (16, 8),
        # a whole workgroup and one with a single tile (plain: the wave's second tile is not there); two whole
        # chunks, so both LDS buffers are written, then a predicated chunk of 8 columns
        "two-wgs": (WG_ROWS + 16, 2 * KC + 8),
        # K group 0 with SPC whole k-steps, K group 1 with one of 8 columns
        "uneven-groups": (16, SPC * KSTEP + 8),
        # the least K that splits across workgroups at N = 16 (2 MIN_CHUNKS chunks): the workspace and the merge
        # kernel, the last chunk again 8 columns
        "split": (16, (2 * MIN_CHUNKS - 1) * KC + 8),
    }


SHAPE_NAMES = ("idle-groups", "two-wgs", "uneven-groups", "split")
MS = (65, 80, 81, 113, 128)


@functools.lru_cache(maxsize=None)
def _reference(name, swiglu, seed=0):
    """(x [128, K], w, ref64, bound) on the CPU, read-only."""
    N, K = _shapes()[name]
    g = torch.Generator().manual_seed(100 * seed + 7 * N + K + int(swiglu))
    x = torch.randn(ROWS, K, generator=g).to(BF16)
    w = (torch.randn((2 if swiglu else 1) * N, K, generator=g) / K ** 0.5).to(BF16)
    return (x, w) + (sn.swiglu_ref64(x, w) if swiglu else sn.linear_ref64(x, w))


def _ws_bytes(swiglu, N, K):
    return dn.lib().call_ret("toa_gemm_wide_swiglu_ws_bytes" if swiglu else "toa_gemm_wide_ws_bytes", N, K)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_every_element_against_fp64_and_nothing_outside_the_operands(name, swiglu):
    from tf_operator_amd.ops import gemm

    L = dn.lib()
    N, K = _shapes()[name]
    x, w, ref, bound = _reference(name, swiglu)
    rows_w, ldx, ldw, ldy = w.shape[0], K + 8, K + 16, N + 8
    wb = torch.full((rows_w + 16, ldw), NAN, dtype=BF16, device=DEV)
    wb[:rows_w, :K] = w.to(DEV)
    nbytes = _ws_bytes(swiglu, N, K)
    assert (nbytes > 0) == (name == "split")
    for M in MS:
        xb = torch.full((ROWS, ldx), NAN, dtype=BF16, device=DEV)
        xb[:M, :K] = x[:M].to(DEV)
        yb = torch.full((ROWS, ldy), SENTINEL, dtype=torch.int16, device=DEV)
        ws = gemm._workspace(torch.device(DEV, torch.cuda.current_device()), nbytes).fill_(NAN) if nbytes else None
        L.call("toa_gemm_wide_swiglu" if swiglu else "toa_gemm_wide", L.ptr(xb), ldx, L.ptr(wb), ldw, L.ptr(yb), ldy,
               M, N, K, L.ptr(ws), L.stream(xb))
        torch.cuda.synchronize()
        sn.check(f"wide {'swiglu' if swiglu else 'plain'} {name} M={M} N={N} K={K}", yb.view(BF16)[:M, :N].cpu(),
                 ref[:M], bound[:M])
        yc = yb.cpu()
        assert bool((yc[M:] == SENTINEL).all()), "rows of y from M on were written"
        assert bool((yc[:, N:] == SENTINEL).all()), "columns of y from N on were written"


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("name", ["two-wgs", "split"])
def test_a_rows_bits_depend_on_that_row_alone(name, swiglu):
    from tf_operator_amd.ops import gemm

    f = gemm.swiglu_wide if swiglu else gemm.linear_wide
    N, K = _shapes()[name]
    x, w, _, _ = _reference(name, swiglu)
    xd, wd = x.to(DEV), w.to(DEV)
    assert gemm.wide_takes(xd, wd, swiglu)
    nbytes = _ws_bytes(swiglu, N, K)
    if nbytes:   # a partial read before this call wrote it would be a NaN
        gemm._workspace(xd.device, nbytes).fill_(NAN)
    full = f(xd, wd)
    assert torch.isfinite(full.float()).all()
    assert torch.equal(_bits(full)[:65], _bits(f(xd[:65], wd))), "rows 0 .. 64 differ between M = 128 and M = 65"
    perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(2))
    assert torch.equal(_bits(full)[perm], _bits(f(xd[perm.to(DEV)], wd))), "permuted rows of x, other rows of y"
    other_x, other_w = (t.to(DEV) for t in _reference(name, swiglu, seed=1)[:2])
    between = f(other_x[:90] * 3, other_w)
    assert torch.isfinite(between.float()).all() and not torch.equal(_bits(between), _bits(full)[:90])
    assert torch.equal(_bits(full), _bits(f(xd, wd))), "a second launch after an unrelated one differs"


def test_refusals_launch_nothing():
    L = dn.lib()
    P, st = L.ptr, L.stream()
    N, K = 48, 520
    x = torch.ones(144, K, dtype=BF16, device=DEV)
    w = torch.ones(2 * N, K, dtype=BF16, device=DEV)
    y = torch.full((144, N), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float32, device=DEV)
    for name in ("toa_gemm_wide", "toa_gemm_wide_swiglu"):
        for M in (64, 129):
            assert L.call_ret(name, P(x), K, P(w), K, P(y), N, M, N, K, P(ws), st) == INVALID_VALUE, (name, M)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


@pytest.mark.parametrize("T", [35, 64], ids=["70-rows", "128-rows"])
@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_extend_under_wide_within_the_teacher_forcing_bound(preset, T):
    from tf_operator_amd.ops import gemm

    m, _, tokens, ref, full = dn.teacher(preset, TOTAL)
    toks = tokens.to(DEV)
    gemm.reset_fallbacks()
    with torch.no_grad():
        cache = m.new_cache(2, TOTAL)
        got = [m.extend(toks[:, c0:c0 + T], cache, split_keys=64, logits="all", gemm="wide")
               for c0 in range(0, TOTAL, T)]
    got = torch.cat(got, 1).double().cpu()
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    dn.check_teacher(f"{preset} extend(all, {T}, wide)", got, ref, full, 0, m.cfg.head_dim, TOTAL)
