"""Decode projections on fp8 weights on an MI355X (csrc/hip/gemm_w8.hip): the
quantiser bit for bit against the CPU formula, every element of both GEMM
forms against fp64, untouched memory and row invariance, refusals that launch
nothing, the model on a lossless snapshot, and a trainer's fresh weights.
Shapes, references and bounds: tests/test_gemm_w8.py."""
import pytest
import torch

import decode_numerics as dn
import skinny_numerics as sn
import test_gemm_w8 as w8

pytestmark = pytest.mark.gpu

DEV, BF16, E4M3 = "cuda", torch.bfloat16, torch.float8_e4m3fn
NAN, SENTINEL, INVALID_VALUE = float("nan"), 0x1234, 1
PROMPT, TOTAL = 5, 140   # tests/test_decode_gpu.py's: split_keys 64, the boundaries at 64 and 128 are crossed


def _gemm():
    from tf_operator_amd.ops import gemm

    dn.lib()
    return gemm


@pytest.mark.parametrize("K", [16, 48, w8.QUANT_LDS_K + 16])
def test_quantiser_bit_for_bit(K):
    gemm = _gemm()
    w, want_e = w8.planted(9, K)
    q_ref, s_ref, e = w8.quant_ref(w)
    assert e[:3].tolist() == want_e
    wb = torch.full((9, K + 8), NAN, dtype=BF16, device=DEV)      # ldw > K, NaN in the padding
    wb[:, :K] = w.to(DEV)
    q, scale = gemm.quantize_w8(wb[:, :K])
    assert q.dtype == E4M3 and q.shape == (9, K)
    assert torch.equal(scale.cpu().view(torch.int32), s_ref.view(torch.int32)), (scale.cpu(), s_ref)
    bad = (q.cpu().view(torch.uint8) != q_ref.view(torch.uint8)).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), [float(w[i, j]) for i, j in bad[:8].tolist()])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", sorted(w8.SHAPES))
def test_every_element_against_fp64(case, swiglu):
    gemm = _gemm()
    N, K = w8.SHAPES[case]
    x, q, scale, ref, bound = w8.w8_reference(N, K, swiglu)
    xd, qd, sd = x.to(DEV), q.to(DEV), scale.to(DEV)
    f = gemm.swiglu_skinny_w8 if swiglu else gemm.linear_skinny_w8
    for M in sn.MS:
        got = f(xd[:M], qd, sd)
        assert got.shape == (M, N) and got.dtype == BF16
        sn.check(f"w8 {'swiglu' if swiglu else 'plain'} {case} M={M} N={N} K={K}", got.cpu(), ref[:M], bound[:M])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("case", ["b", "d"])
def test_nothing_else_is_touched_and_a_row_does_not_depend_on_its_batch(case, swiglu):
    gemm = _gemm()
    L = dn.lib()
    N, K = w8.SHAPES[case]
    x, q, scale, ref, bound = w8.w8_reference(N, K, swiglu)
    rows, tail = q.shape[0], "_swiglu" if swiglu else ""
    ldx, ldw, ldy = K + 8, K + 16, N + 8
    qb = torch.full((rows + 16, ldw), 0x7f, dtype=torch.uint8, device=DEV)   # e4m3 NaN beyond K and beyond the rows
    qb[:rows, :K] = q.view(torch.uint8).to(DEV)
    sb = torch.full((rows + 16,), NAN, device=DEV)
    sb[:rows] = scale.to(DEV)
    nbytes = L.call_ret(f"toa_gemm_skinny_w8{tail}_ws_bytes", N, K)
    assert nbytes > 0
    ws = gemm._workspace(torch.device(DEV, torch.cuda.current_device()), nbytes)
    out = {}
    for M in (1, 7, 16):
        xb = torch.full((sn.MAX_M, ldx), NAN, dtype=BF16, device=DEV)
        xb[:M, :K] = x[:M].to(DEV)
        yb = torch.full((sn.MAX_M + 1, ldy), SENTINEL, dtype=torch.int16, device=DEV)
        ws.fill_(NAN)
        L.call("toa_gemm_skinny_w8" + tail, L.ptr(xb), ldx, L.ptr(qb), ldw, L.ptr(sb), L.ptr(yb), ldy, M, N, K, L.ptr(ws),
               L.stream(xb))
        yc = yb.cpu()
        out[M] = yc[:M, :N]
        assert torch.isfinite(out[M].view(BF16).float()).all()
        sn.check(f"strided w8 {case} M={M}", out[M].view(BF16), ref[:M], bound[:M])
        assert bool((yc[M:] == SENTINEL).all()) and bool((yc[:, N:] == SENTINEL).all()), "y written outside [M, N]"
    assert torch.equal(out[1], out[16][:1]) and torch.equal(out[7], out[16][:7])


def test_refusals_launch_nothing():
    gemm = _gemm()
    L = dn.lib()
    P, st = L.ptr, L.stream()
    x = torch.ones(32, 64, dtype=BF16, device=DEV)
    qflat = torch.full((48 * 64 + 16,), 0x38, dtype=torch.uint8, device=DEV).view(E4M3)   # ones
    q = qflat[:48 * 64].view(48, 64)
    scale = torch.ones(48, device=DEV)
    y = torch.full((32, 48), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    cases = {   # the wrapper's operands; (M, N, K, q) of the launcher
        "M = 17": ((x[:17], q, scale), (17, 48, 64, q)),
        "K = 24": ((x[:8, :24], q[:, :24], scale), (8, 48, 24, q)),
        "N = 24": ((x[:8], q[:24], scale[:24]), (8, 24, 64, q)),
        "a misaligned q": ((x[:8], qflat[1:1 + 48 * 64].view(48, 64), scale), (8, 48, 64, qflat[1:])),
        "a scale of the wrong length": ((x[:8], q, scale[:47]), None),
        "a scale of the wrong dtype": ((x[:8], q, scale.to(BF16)), None),
    }
    for what, (operands, raw) in cases.items():
        assert gemm.skinny_w8_refusal(*operands), what
        with pytest.raises(ValueError, match="toa_gemm_skinny_w8"):
            gemm.linear_skinny_w8(*operands)
        if raw is not None:
            M, N, K, qq = raw
            assert L.call_ret("toa_gemm_skinny_w8", P(x), 64, P(qq), 64, P(scale), P(y), 48, M, N, K, P(ws), st) == \
                INVALID_VALUE, what
    assert L.call_ret("toa_gemm_skinny_w8", P(x), 64, P(q), 64, None, P(y), 48, 8, 48, 64, P(ws), st) == INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    m = w8.snapped_model("llama-tiny", DEV, BF16)
    cache = m.new_cache(2, 8)
    with pytest.raises(ValueError, match="tile"):
        m.decode_step(torch.zeros(2, dtype=torch.long, device=DEV), cache, gemm="tile", weights=m.quantize_projections())
    assert cache.host_lengths == [0, 0]


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_teacher_forcing_on_a_lossless_snapshot(preset):
    from tf_operator_amd.models.llama import PRESETS, Llama

    gemm = _gemm()
    m = w8.snapped_model(preset, DEV, BF16)
    ref_m = Llama(PRESETS[preset], device="cpu", dtype=torch.float32).eval()
    ref_m.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    tokens = torch.randint(0, m.cfg.vocab_size, (2, TOTAL), generator=torch.Generator().manual_seed(5))
    snap = m.quantize_projections()
    gemm.reset_fallbacks()
    with torch.no_grad():
        ref, full = ref_m(tokens).double(), m(tokens.to(DEV)).double().cpu()
        cache = m.new_cache(2, TOTAL)
        dec = [m.prefill(tokens[:, :PROMPT].to(DEV), cache, gemm="skinny", weights=snap)]
        for t in range(PROMPT, TOTAL):
            dec.append(m.decode_step(tokens[:, t].to(DEV), cache, split_keys=64, gemm="skinny", weights=snap))
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    dn.check_teacher(f"{preset} fp8 decode", torch.stack(dec, 1).double().cpu(), ref, full, PROMPT - 1, m.cfg.head_dim,
                     TOTAL)


def test_a_trainer_samples_from_its_current_weights():
    from tf_operator_amd.train.generate import generate
    from tf_operator_amd.train.llm import LlamaTrainer

    _gemm()
    tr = LlamaTrainer("llama-tiny", torch.device(DEV), micro_batch=2, seq_len=128, lr=1e-2)
    b = tr.synthetic_batch()
    p = b[0][:, :8]
    before = tr.model.quantize_projections()
    tr.step([b])
    got, _ = tr.generate(p, 8, gemm="skinny", weights="fp8")
    tr.model.eval()
    want, _ = generate(tr.model, p, 8, gemm="skinny", weights=tr.model.quantize_projections())
    assert torch.equal(got, want)
    after = tr.model.quantize_projections()
    assert not torch.equal(before[0]["wqkv"][0].view(torch.uint8), after[0]["wqkv"][0].view(torch.uint8))
