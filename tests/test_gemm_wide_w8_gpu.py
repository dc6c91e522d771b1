"""The 65-to-128-row GEMM on fp8 weights on an MI355X (csrc/hip/gemm_wide_w8.hip):
every element of both forms against fp64 on strided operands with NaN around
them, a row's bits independent of M and of its index, refusals that launch
nothing, the model on a lossless snapshot by the teacher-forcing rule.
Shapes, references and bounds: tests/test_gemm_wide_w8.py."""
import pytest
import torch

import decode_numerics as dn
import skinny_numerics as sn
import test_gemm_w8 as w8
import test_gemm_wide_w8 as ww8

pytestmark = pytest.mark.gpu

DEV, BF16, E4M3 = "cuda", torch.bfloat16, torch.float8_e4m3fn
NAN, SENTINEL, INVALID_VALUE = float("nan"), 0x1234, 1
T, TOTAL = 35, 140   # 2 x 35 = 70 rows a call; split_keys 64, the boundaries at 64 and 128 are crossed


def _gemm():
    from tf_operator_amd.ops import gemm

    dn.lib()
    return gemm


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("name", sorted(ww8.SHAPES))
def test_every_element_against_fp64_and_nothing_outside_the_operands(name, swiglu):
    gemm, L = _gemm(), dn.lib()
    N, K = ww8.SHAPES[name]
    x, q, scale, ref, bound = ww8.reference(name, swiglu)
    rows, tail = q.shape[0], "_swiglu" if swiglu else ""
    ldx, ldw, ldy = K + 8, K + 16, N + 8
    qb = torch.full((rows + 16, ldw), 0x7f, dtype=torch.uint8, device=DEV)   # e4m3 NaN beyond K and beyond the rows
    qb[:rows, :K] = q.view(torch.uint8).to(DEV)
    sb = torch.full((rows + 16,), NAN, device=DEV)
    sb[:rows] = scale.to(DEV)
    nbytes = L.call_ret(f"toa_gemm_wide_w8{tail}_ws_bytes", N, K)
    assert (nbytes > 0) == (name in ("split", "steady"))
    ws = gemm._workspace(torch.device(DEV, torch.cuda.current_device()), nbytes) if nbytes else None
    for M in ww8.MS:
        xb = torch.full((ww8.MAX_M, ldx), NAN, dtype=BF16, device=DEV)
        xb[:M, :K] = x[:M].to(DEV)
        yb = torch.full((ww8.MAX_M + 1, ldy), SENTINEL, dtype=torch.int16, device=DEV)
        if ws is not None:
            ws.fill_(NAN)
        L.call("toa_gemm_wide_w8" + tail, L.ptr(xb), ldx, L.ptr(qb), ldw, L.ptr(sb), L.ptr(yb), ldy, M, N, K,
               L.ptr(ws), L.stream(xb))
        yc = yb.cpu()
        sn.check(f"wide w8 {'swiglu' if swiglu else 'plain'} {name} M={M} N={N} K={K}", yc[:M, :N].view(BF16),
                 ref[:M], bound[:M])
        assert bool((yc[M:] == SENTINEL).all()) and bool((yc[:, N:] == SENTINEL).all()), "y written outside [M, N]"


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("name", ["two-wgs", "split"])
def test_a_rows_bits_depend_on_that_row_alone(name, swiglu):
    gemm = _gemm()
    f = gemm.swiglu_wide_w8 if swiglu else gemm.linear_wide_w8
    x, q, scale = (t.to(DEV) for t in ww8.reference(name, swiglu)[:3])
    bits = lambda t: t.contiguous().view(torch.int16).cpu()
    full = f(x, q, scale)
    assert torch.isfinite(full.float()).all()
    assert torch.equal(bits(full)[:65], bits(f(x[:65], q, scale))), "rows 0 .. 64 differ between M = 128 and M = 65"
    perm = torch.randperm(128, generator=torch.Generator().manual_seed(2))
    assert torch.equal(bits(full)[perm], bits(f(x[perm.to(DEV)], q, scale))), "permuted rows of x, other rows of y"


def test_refusals_launch_nothing():
    gemm, L = _gemm(), dn.lib()
    P, st = L.ptr, L.stream()
    x = torch.ones(144, 64, dtype=BF16, device=DEV)
    qflat = torch.full((64 * 64 + 16,), 0x38, dtype=torch.uint8, device=DEV).view(E4M3)   # ones
    q = qflat[:64 * 64].view(64, 64)
    scale = torch.ones(64, device=DEV)
    y = torch.full((144, 64), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    cases = {   # the wrapper's operands; (M, K, q) of the launcher
        "M = 64": ((x[:64], q, scale), (64, 64, q)),
        "M = 129": ((x[:129], q, scale), (129, 64, q)),
        "K = 24": ((x[:80, :24], q[:, :24], scale), (80, 24, q)),
        "a misaligned q": ((x[:80], qflat[1:1 + 64 * 64].view(64, 64), scale), (80, 64, qflat[1:])),
    }
    for what, (operands, (M, K, qq)) in cases.items():
        assert gemm.wide_w8_refusal(*operands), what
        for f, name in ((gemm.linear_wide_w8, "toa_gemm_wide_w8"), (gemm.swiglu_wide_w8, "toa_gemm_wide_w8_swiglu")):
            with pytest.raises(ValueError, match=name):
                f(*operands)
            N = 64 if f is gemm.linear_wide_w8 else 32
            assert L.call_ret(name, P(x), 64, P(qq), 64, P(scale), P(y), 64, M, N, K, P(ws), st) == INVALID_VALUE, what
    assert L.call_ret("toa_gemm_wide_w8", P(x), 64, P(q), 64, None, P(y), 64, 80, 64, 64, P(ws), st) == INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_teacher_forcing_on_a_lossless_snapshot(preset):
    from tf_operator_amd.models.llama import PRESETS, Llama

    gemm = _gemm()
    m = w8.snapped_model(preset, DEV, BF16)
    ref_m = Llama(PRESETS[preset], device="cpu", dtype=torch.float32).eval()
    ref_m.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    tokens = torch.randint(0, m.cfg.vocab_size, (2, TOTAL), generator=torch.Generator().manual_seed(5))
    snap, toks = m.quantize_projections(), tokens.to(DEV)
    gemm.reset_fallbacks()
    with torch.no_grad():
        ref, full = ref_m(tokens).double(), m(toks).double().cpu()
        cache = m.new_cache(2, TOTAL)
        got = [m.prefill(toks[:, :T], cache, gemm="wide", weights=snap)[:, None]]   # 70 rows, as every call below
        got += [m.extend(toks[:, c0:c0 + T], cache, split_keys=64, logits="all", gemm="wide", weights=snap)
                for c0 in range(T, TOTAL, T)]
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    dn.check_teacher(f"{preset} fp8 extend(all, {T}, wide)", torch.cat(got, 1).double().cpu(), ref, full, T - 1,
                     m.cfg.head_dim, TOTAL)
