"""Decode projections on MXFP4 weights on an MI355X (csrc/hip/gemm_w4.hip): the quantiser bit for bit, both GEMM
forms against fp64, untouched memory and row invariance, refusals, the model.  Shapes: tests/test_gemm_w4.py."""
import pytest
import torch

import decode_numerics as dn
import skinny_numerics as sn
import test_gemm_w4 as w4

pytestmark = pytest.mark.gpu

DEV, BF16, U8 = "cuda", torch.bfloat16, torch.uint8
NAN, SENTINEL, INVALID_VALUE = float("nan"), 0x1234, 1
PROMPT, TOTAL = 5, 44   # about 40 teacher-forced positions


def _gemm():
    from tf_operator_amd.ops import gemm
    dn.lib()
    return gemm


def strided(t, rows, ld, fill):
    """t in the corner of a [rows, ld] buffer of `fill` on the GPU, as a view of t's shape."""
    buf = torch.full((rows, ld), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return buf[:t.shape[0], :t.shape[1]]


def scales(scale, rows=None):
    """scale on the GPU in rows padded to SCALE_ALIGN, 0xff in the padding."""
    ld = -(-scale.shape[1] // w4.SCALE_ALIGN) * w4.SCALE_ALIGN
    return strided(scale, rows or scale.shape[0], ld, 0xff)


@pytest.mark.parametrize("K", [32, 96, 256 * w4.BLOCK + 32])   # the last: a thread of the quantiser takes two blocks
def test_quantiser_bit_for_bit(K):
    gemm = _gemm()
    w = w4.planted(K)
    q_ref, s_ref = gemm.quantize_w4(w)
    q, scale = gemm.quantize_w4(strided(w, 9, K + 8, NAN))      # ldw > K, NaN in the padding
    assert q.dtype == scale.dtype == U8 and torch.equal(scale.cpu(), s_ref), (scale.cpu(), s_ref)
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), [float(w[i, 2 * j]) for i, j in bad[:8].tolist()])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", sorted(w4.SHAPES))
def test_every_element_against_fp64(case, swiglu):
    gemm = _gemm()
    N, K = w4.SHAPES[case]
    x, q, scale, ref, bound = w4.w4_reference(N, K, swiglu)
    xd, qd, sd = x.to(DEV), q.to(DEV), scales(scale)
    f = gemm.swiglu_skinny_w4 if swiglu else gemm.linear_skinny_w4
    for M in sn.MS:
        got = f(xd[:M], qd, sd)
        sn.check(f"w4 {'swiglu' if swiglu else 'plain'} {case} M={M} N={N} K={K}", got.cpu(), ref[:M], bound[:M])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", ["b", "d"])
def test_nothing_else_is_touched_and_a_row_does_not_depend_on_its_batch(case, swiglu):
    gemm = _gemm()
    L = dn.lib()
    N, K = w4.SHAPES[case]
    x, q, scale, ref, bound = w4.w4_reference(N, K, swiglu)
    rows, tail = q.shape[0], "_swiglu" if swiglu else ""
    ldx, ldw, ldy = K + 8, K // 2 + 16, N + 8
    qb = strided(q, rows + 16, ldw, 0xff)      # -6 pairs beyond K and beyond the rows, under NaN scales
    sb = scales(scale, rows + 16)
    nbytes = L.call_ret(f"toa_gemm_skinny_w4{tail}_ws_bytes", N, K)
    assert nbytes > 0
    ws = gemm._workspace(torch.device(DEV, torch.cuda.current_device()), nbytes)
    out = {}
    for M in (1, 7, 16):
        xb = strided(x[:M], sn.MAX_M, ldx, NAN)
        yb = torch.full((sn.MAX_M + 1, ldy), SENTINEL, dtype=torch.int16, device=DEV)
        ws.fill_(NAN)
        L.call("toa_gemm_skinny_w4" + tail, L.ptr(xb), ldx, L.ptr(qb), ldw, L.ptr(sb), sb.stride(0), L.ptr(yb), ldy, M, N,
               K, L.ptr(ws), L.stream(xb))
        yc = yb.cpu()
        out[M] = yc[:M, :N]
        assert torch.isfinite(out[M].view(BF16).float()).all()
        sn.check(f"strided w4 {case} M={M}", out[M].view(BF16), ref[:M], bound[:M])
        assert bool((yc[M:] == SENTINEL).all()) and bool((yc[:, N:] == SENTINEL).all()), "y written outside [M, N]"
    assert torch.equal(out[1], out[16][:1]) and torch.equal(out[7], out[16][:7])


def test_refusals_launch_nothing():
    gemm = _gemm()
    L = dn.lib()
    P, st = L.ptr, L.stream()
    x = torch.ones(32, 128, dtype=BF16, device=DEV)
    qflat = torch.full((48 * 64 + 16,), 0x22, dtype=U8, device=DEV)   # ones
    q = qflat[:48 * 64].view(48, 64)
    scale = torch.full((48, 4), 127, dtype=U8, device=DEV)
    y = torch.full((32, 48), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    cases = {   # the wrapper's operands; (M, N, K, q) of the launcher
        "M = 17": ((x[:17], q, scale), (17, 48, 128, q)),
        "K = 48": ((x[:8, :48], q[:, :24], scale[:, :1]), (8, 48, 48, q)),
        "N = 24": ((x[:8], q[:24], scale[:24]), (8, 24, 128, q)),
        "a misaligned q": ((x[:8], qflat[1:1 + 48 * 64].view(48, 64), scale), (8, 48, 128, qflat[1:])),
        "scales of the wrong shape": ((x[:8], q, scale[:47]), None),
        "scales of one block too few": ((x[:8], q, scale[:, :3]), None),
        "scales of the wrong dtype": ((x[:8], q, scale.float()), None),
    }
    for what, (operands, raw) in cases.items():
        assert gemm.skinny_w4_refusal(*operands), what
        with pytest.raises(ValueError, match="toa_gemm_skinny_w4"):
            gemm.linear_skinny_w4(*operands)
        if raw is not None:
            M, N, K, qq = raw
            assert L.call_ret("toa_gemm_skinny_w4", P(x), 128, P(qq), 64, P(scale), 4, P(y), 48, M, N, K, P(ws), st) == \
                INVALID_VALUE, what
    for s, lds in ((None, 4), (scale, 2)):   # a null scale, scale rows the 4-byte loads cannot take
        assert L.call_ret("toa_gemm_skinny_w4", P(x), 128, P(q), 64, P(s), lds, P(y), 48, 8, 48, 128, P(ws), st) == \
            INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and not gemm.skinny_w4_refusal(x[:8], q, scale)


def test_the_model_on_a_lossless_snapshot():
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.train.generate import generate

    gemm = _gemm()
    m = w4.snapped_model("llama-tiny", DEV, BF16)
    ref_m = Llama(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32).eval()
    ref_m.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    tokens = torch.randint(0, m.cfg.vocab_size, (2, TOTAL), generator=torch.Generator().manual_seed(5))
    snap, toks = m.quantize_projections(fmt="fp4"), tokens.to(DEV)
    gemm.reset_fallbacks()
    with torch.no_grad():
        ref, full = ref_m(tokens).double(), m(toks).double().cpu()
        cache = m.new_cache(2, TOTAL)
        dec = [m.prefill(toks[:, :PROMPT], cache, gemm="skinny", weights=snap)]
        for t in range(PROMPT, TOTAL):
            dec.append(m.decode_step(toks[:, t], cache, split_keys=64, gemm="skinny", weights=snap))
        assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
        dn.check_teacher("llama-tiny fp4 decode", torch.stack(dec, 1).double().cpu(), ref, full, PROMPT - 1,
                         m.cfg.head_dim, TOTAL)
        with pytest.raises(ValueError, match="tile"):
            m.decode_step(toks[:, 0], m.new_cache(2, 8), gemm="tile", weights=snap)
        a, _ = generate(m, toks[:, :PROMPT], 6, gemm="skinny", weights="fp4")
        b, _ = generate(m, toks[:, :PROMPT], 6, gemm="skinny", weights=snap)
        assert torch.equal(a, b) and not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
        # 17 rows: counted, and the bf16 path's bits
        got = m.extend(toks[:1, :17], m.new_cache(1, 17), gemm="stream", logits="all", weights=snap)
        counted = [k for k in gemm.fallbacks() if k.startswith("decode")]
        gemm.reset_fallbacks()
        assert counted and all(k.startswith("decode-fp4 17x") and k.endswith("-> bf16 stream") for k in counted), counted
        assert torch.equal(got, m.extend(toks[:1, :17], m.new_cache(1, 17), gemm="stream", logits="all"))
