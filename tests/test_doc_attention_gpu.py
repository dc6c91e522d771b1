"""Document-masked causal attention on the GPU: the DOC arms of the
register-staged HIP kernels (toa_attn_fwd_doc / toa_attn_bwd_doc) against the
fp32 reference with the mask, and the opt-in path up to the trainer.

Tolerances are test_flash_attention_fwd_bwd's (tests/test_ops_gpu.py):
rel(o) < 2e-2, gradients < 3e-2."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, HK = 2, 4, 2
O_TOL, G_TOL = 2e-2, 3e-2


def _lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _lengths(starts, S):
    return [[b - a for a, b in zip(s, s[1:] + [S])] for s in starts]


def _inputs(S, D, seed, b=B):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, k, v = (torch.randn(b, h, S, D, device=DEV, generator=g).to(torch.bfloat16) for h in (H, HK, HK))
    do = torch.randn(b, H, S, D, device=DEV, generator=g).to(torch.bfloat16)
    return q, k, v, do


def _run(q, k, v, do, doc, bshd=False):
    """(o, dq, dk, dv) of causal_attention, o and do as [B, H, S, D] whatever the kernel's layout."""
    from tf_operator_amd.ops import llm

    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = llm.causal_attention(q, k, v, out_layout="bshd" if bshd else "bhsd", doc=doc)
    o.backward(do.transpose(1, 2).contiguous() if bshd else do)
    torch.cuda.synchronize()
    return (o.detach().transpose(1, 2) if bshd else o.detach()), q.grad, k.grad, v.grad


def _reference(q, k, v, do, doc):
    from tf_operator_amd.ops import llm

    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    o = llm._attention_reference(qr, kr, vr, 1.0 / math.sqrt(q.shape[-1]), doc)
    o.backward(do.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


# per batch row: a boundary inside a tile (10), on a 64-tile edge (128, 64) and on the 256-block edge (256), a
# length-1 document (80), documents starting in the ragged tail (293, 300); rows 64-95 are one wave whose rows
# start at 10 and at 80, in different 64-key tiles: its first computed tile is fully masked for the rows of 80
STARTS = [[0, 10, 80, 81, 128, 256, 293], [0, 64, 300]]


@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_doc_attention_numerics(D, bshd):
    _lib()
    from tf_operator_amd.ops import llm

    S = 320
    q, k, v, do = _inputs(S, D, 21)
    doc = llm.doc_bounds_from_lengths(_lengths(STARTS, S), S, device=DEV)
    got = _run(q, k, v, do, doc, bshd)
    ref = _reference(q, k, v, do, doc)
    errs = [rel(a, b) for a, b in zip(got, ref)]
    print("D", D, "bshd", bshd, "rel o dq dk dv", errs)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert errs[0] < O_TOL and max(errs[1:]) < G_TOL, errs


@pytest.mark.parametrize("S", [320, 100])
@pytest.mark.parametrize("D", [64, 128])
def test_one_document_is_plain_causal_bit_for_bit(S, D):
    """At these S the unmasked path runs the same ragged-S kernels; one
    document per row must change nothing."""
    _lib()
    from tf_operator_amd.ops import llm

    q, k, v, do = _inputs(S, D, 22)
    scale = 1.0 / math.sqrt(D)
    ds = torch.zeros(B, S, device=DEV, dtype=torch.int32)
    de = torch.full((B, S), S, device=DEV, dtype=torch.int32)
    o0, lse0 = llm._attn_fwd(q, k, v, scale, False)
    o1, lse1 = llm._attn_fwd_doc(q, k, v, ds, scale, False)
    g0 = llm._attn_bwd(q, k, v, o0, lse0, do, scale, False)
    g1 = llm._attn_bwd_doc(q, k, v, o1, lse1, do, ds, de, scale, False)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    for name, a, b in zip(("dq", "dk", "dv"), g0, g1):
        assert torch.equal(a, b), name
    assert float(g1[0].float().abs().sum()) > 0


def test_packed_equals_separate():
    _lib()
    from tf_operator_amd.ops import llm

    S, D, starts = 320, 128, [0, 100, 228]
    q, k, v, do = _inputs(S, D, 23)
    doc = llm.doc_bounds_from_lengths(_lengths([starts] * B, S), S, device=DEV)
    packed = _run(q, k, v, do, doc)
    for a, e in zip(starts, starts[1:] + [S]):
        alone = _run(*(t[:, :, a:e].contiguous() for t in (q, k, v, do)), None)
        errs = [rel(p[:, :, a:e], x) for p, x in zip(packed, alone)]
        print("document", a, e, "rel o dq dk dv", errs)
        assert errs[0] < O_TOL and max(errs[1:]) < G_TOL, (a, e, errs)


def test_foreign_tiles_are_skipped_not_masked():
    """NaN in every input of documents 0 and 2: a kernel that computed their
    tiles and masked afterwards would give 0 x NaN in document 1."""
    _lib()
    from tf_operator_amd.ops import llm

    S, D = 768, 128
    q, k, v, do = _inputs(S, D, 24)
    alone = _run(*(t[:, :, 256:512].contiguous() for t in (q, k, v, do)), None)
    for t in (q, k, v, do):
        t[:, :, :256] = float("nan")
        t[:, :, 512:] = float("nan")
    doc = llm.doc_bounds_from_lengths([[256, 256, 256]] * B, S, device=DEV)
    got = [t[:, :, 256:512] for t in _run(q, k, v, do, doc)]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    errs = [rel(a, b) for a, b in zip(got, alone)]
    print("document 1 rel o dq dk dv", errs)
    assert errs[0] < O_TOL and max(errs[1:]) < G_TOL, errs


@pytest.mark.parametrize("S", [320, 256])
def test_out_of_range_arrays_are_clamped(S):
    """doc_start past the row and doc_end before it: the kernels clamp both
    where they read them, so the calls complete; the values are unspecified."""
    _lib()
    from tf_operator_amd.ops import llm

    D = 128
    q, k, v, do = _inputs(S, D, 25)
    good = llm.doc_bounds_from_lengths([[S]] * B, S, device=DEV)
    for ds, de in ((torch.full_like(good[0], S + 5), good[1]), (good[0], torch.full_like(good[1], -3))):
        got = _run(q, k, v, do, (ds, de))
        torch.cuda.synchronize()
        assert all(t.shape == r.shape for t, r in zip(got, (q, q, k, v)))


def test_trainer_with_doc_eos():
    """llama-tiny128 at seq_len 320: 3 steps with finite, decreasing loss, and
    a first-step loss that matches the CPU trainer's on the same weights and
    tokens within what test_llama_tiny_gpu_matches_cpu_reference
    (tests/test_ops_gpu.py) allows between the GPU and the CPU model: 2e-2."""
    _lib()
    from tf_operator_amd.train.data import SyntheticTokens
    from tf_operator_amd.train.llm import LlamaTrainer

    tok, tgt = SyntheticTokens(2, 320, 1024, doc_len=(16, 120), eos_id=3).next()
    gpu = LlamaTrainer("llama-tiny128", torch.device(DEV), micro_batch=2, seq_len=320, seed=0, doc_eos=3)
    cpu = LlamaTrainer("llama-tiny128", torch.device("cpu"), micro_batch=2, seq_len=320, seed=0, doc_eos=3)
    cpu.model.load_state_dict({n: t.cpu() for n, t in gpu.model.state_dict().items()})
    batch = (tok.to(DEV), tgt.to(DEV))
    losses = [float(gpu.step([batch])) for _ in range(3)]
    first_cpu = float(cpu.step([(tok, tgt)]))
    print("gpu losses", losses, "cpu first", first_cpu)
    assert all(math.isfinite(x) for x in losses), losses
    assert losses[2] < losses[1] < losses[0], losses
    assert abs(losses[0] - first_cpu) < 2e-2, (losses[0], first_cpu)


def test_unmasked_block_is_untouched(monkeypatch):
    """doc=None: attention_block launches what it launched before -- the
    fused QKV + RoPE GEMM, the attention forward, the fused RoPE backward with
    the delta rows from the output projection's GEMM -- and no _doc entry
    point; two calls agree bit for bit."""
    L = _lib()
    from tf_operator_amd.ops import gemm, llm

    names = []
    real_call, real_ret = L.call, L.call_ret
    monkeypatch.setattr(L, "call", lambda n, *a: (names.append(n), real_call(n, *a))[1])
    monkeypatch.setattr(L, "call_ret", lambda n, *a: (names.append(n), real_ret(n, *a))[1])
    old = gemm.mode()
    gemm.set_mode("asm")
    try:
        S, D, Hd = 256, 128, 512
        g = torch.Generator(device=DEV).manual_seed(26)
        x0, h0, dy = (torch.randn(B * S, Hd, device=DEV, generator=g).to(torch.bfloat16) for _ in range(3))
        cos, sin = llm.rope_tables(S, D, device=DEV)
        res, seqs = [], []
        for _ in range(2):
            ws = []
            for n, kk in (((H + 2 * HK) * D, Hd), (Hd, H * D)):
                w = torch.nn.Parameter((torch.randn(n, kk, device=DEV,
                                                    generator=torch.Generator(device=DEV).manual_seed(n)) / kk ** 0.5
                                        ).to(torch.bfloat16))
                w.main_grad = torch.zeros_like(w)
                w._toa_wt = w.data.t().contiguous()
                ws.append(w)
            x, h = x0.clone().requires_grad_(), h0.clone().requires_grad_()
            del names[:]
            out, _ = llm.attention_block(x, ws[0], ws[1], cos, sin, B, S, H, HK, D, residual=h)
            out.backward(dy)
            torch.cuda.synchronize()
            seqs.append(list(names))
            res.append((out.detach(), x.grad, h.grad, ws[0].main_grad, ws[1].main_grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)
        assert seqs[0] == seqs[1]
        called = set(seqs[0])
        assert not [n for n in called if n.endswith("_doc")], called
        assert {"toa_gemm_asm_rope", "toa_attn_fwd", "toa_gemm_asm_delta", "toa_attn_bwd_rope"} <= called, called
        assert not called & {"toa_rope_fwd", "toa_rope_bwd", "toa_attn_bwd"}, called
        # the same block with a mask takes the entry points of its own
        del names[:]
        doc = llm.doc_bounds_from_lengths([[100, 156]] * B, S, device=DEV)
        out, _ = llm.attention_block(x0.clone().requires_grad_(), ws[0], ws[1], cos, sin, B, S, H, HK, D, residual=h0,
                                     doc=doc)
        out.backward(dy)
        torch.cuda.synchronize()
        assert {"toa_rope_fwd", "toa_attn_fwd_doc", "toa_attn_bwd_doc", "toa_rope_bwd"} <= set(names), names
        assert not set(names) & {"toa_attn_fwd", "toa_attn_bwd_rope", "toa_gemm_asm_rope", "toa_gemm_asm_delta"}, names
    finally:
        gemm.set_mode(old)
