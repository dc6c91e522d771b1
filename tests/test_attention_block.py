"""The attention sub-block's glue (ops/llm.attention_block): the per-call
delta link between its two autograd nodes, the model-owned cos | sin table of
the fused QKV + RoPE GEMM, and the predicates that mirror the assembly GEMM
launcher's checks."""
import dataclasses

import pytest
import torch

DEV = "cuda"


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _asm_lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()


def test_rope_table_belongs_to_the_model():
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.ops.llm import rope_tables

    tabs = []
    for theta in (500000.0, 10000.0):
        cfg = dataclasses.replace(PRESETS["llama-tiny128"], rope_theta=theta)
        m = Llama(cfg, device="cpu")
        cos, sin, cossin = m.rope(256, "cpu")
        rc, rs = rope_tables(256, cfg.head_dim, theta, device="cpu")
        assert torch.equal(cos, rc) and torch.equal(sin, rs)
        assert cossin.dtype == torch.float32 and torch.equal(cossin, torch.stack([rc, rs]))
        assert m.rope(256, "cpu")[2] is cossin
        tabs.append(cossin)
    assert not torch.equal(tabs[0], tabs[1])


def _weights(Hq, Hkv, D, Hd, seed):
    """wqkv, wo as a trainer holds them: a flat-buffer gradient and the W^T copy."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ws = []
    for n, k in (((Hq + 2 * Hkv) * D, Hd), (Hd, Hq * D)):
        w = torch.nn.Parameter((torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).to(torch.bfloat16))
        w.main_grad = torch.zeros_like(w)
        w._toa_wt = w.data.t().contiguous()
        ws.append(w)
    return ws


@pytest.mark.gpu
def test_qkv_rope_two_thetas_in_one_process():
    """Two models' tables at the same S, one after the other with the first
    freed: each fused output follows its own tables (a table kept by address
    would serve the second theta the first one's rotation)."""
    from tf_operator_amd.ops import gemm, llm
    from tf_operator_amd.ops.linear import linear

    _asm_lib()
    old = gemm.mode()
    gemm.set_mode("asm")
    try:
        B, S, Hq, Hkv, D, Hd = 1, 256, 4, 2, 128, 512
        torch.manual_seed(0)
        x0 = torch.randn(B * S, Hd, device=DEV).to(torch.bfloat16)
        w0 = (torch.randn((Hq + 2 * Hkv) * D, Hd, device=DEV) / Hd ** 0.5).to(torch.bfloat16)
        dout = torch.randn(B, S, Hq, D, device=DEV).to(torch.bfloat16)
        fused_out = []
        for theta in (500000.0, 10000.0):
            cos, sin = llm.rope_tables(S, D, theta, device=DEV)
            res = []
            for fused in (True, False):
                x = x0.clone().requires_grad_()
                w = torch.nn.Parameter(w0.clone())
                w.main_grad = torch.zeros_like(w)
                assert llm.qkv_rope_attention_ok(x, w, S, Hq, Hkv, D)
                o = (llm.qkv_rope_attention(x, w, cos, sin, B, S, Hq, Hkv, D) if fused
                     else llm.rope_attention(linear(x, w), cos, sin, B, S, Hq, Hkv, D))
                o.backward(dout)
                torch.cuda.synchronize()
                res.append((o.detach().float(), x.grad.float(), w.main_grad.float()))
            for a, b in zip(*res):
                print("theta", theta, "fused vs two nodes rel", rel(a, b))
                assert rel(a, b) < 2e-2, (theta, rel(a, b))
            fused_out.append(res[0][0])
            del cos, sin, res
        print("theta 500000 vs 10000 rel", rel(fused_out[0], fused_out[1]))
        assert rel(fused_out[0], fused_out[1]) > 0.2
    finally:
        gemm.set_mode(old)


@pytest.mark.gpu
def test_delta_link_does_not_outlive_its_graph():
    """An output projection's backward whose attention backward never runs
    fills only its own link: a later, unrelated attention backward computes
    what it computed before."""
    from tf_operator_amd.ops import gemm, llm

    _asm_lib()
    assert not hasattr(llm, "_PENDING_DELTA") and not hasattr(llm, "_COSSIN")
    old = gemm.mode()
    gemm.set_mode("asm")
    try:
        B, S, H, D = 2, 512, 4, 128
        torch.manual_seed(3)
        qkv0 = torch.randn(B * S, 3 * H * D, device=DEV).to(torch.bfloat16)
        cos, sin = llm.rope_tables(S, D, device=DEV)
        do = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)

        def attention_alone():
            qkv = qkv0.clone().requires_grad_()
            llm.rope_attention(qkv, cos, sin, B, S, H, H, D).backward(do)
            torch.cuda.synchronize()
            return qkv.grad

        first = attention_alone()
        o = torch.randn(B * S, H * D, device=DEV).to(torch.bfloat16).requires_grad_()   # a leaf: no attention node
        _, wo = _weights(H, H, D, H * D, 4)
        link = llm._DeltaLink()
        llm.attn_out_proj(o, wo, B, S, H, link=link).backward(do.view(B * S, H * D))
        torch.cuda.synchronize()
        assert link.ndelta is not None   # filled, and nobody took it
        del o
        assert torch.equal(attention_alone(), first)
    finally:
        gemm.set_mode(old)


@pytest.mark.gpu
def test_attention_block_equals_its_parts():
    """attention_block against qkv_rope_attention -> attn_out_proj wired with
    a link by hand: the same kernels in the same order, so bit for bit."""
    from tf_operator_amd.ops import gemm, llm

    _asm_lib()
    old = gemm.mode()
    gemm.set_mode("asm")
    try:
        B, S, Hq, Hkv, D, Hd = 2, 512, 4, 2, 128, 512
        torch.manual_seed(5)
        x0 = torch.randn(B * S, Hd, device=DEV).to(torch.bfloat16)
        h0 = torch.randn(B * S, Hd, device=DEV).to(torch.bfloat16)
        dy = torch.randn(B * S, Hd, device=DEV).to(torch.bfloat16)
        cos, sin = llm.rope_tables(S, D, device=DEV)
        res = []
        for whole in (True, False):
            x, h = x0.clone().requires_grad_(), h0.clone().requires_grad_()
            wqkv, wo = _weights(Hq, Hkv, D, Hd, 6)
            if whole:
                out, summed = llm.attention_block(x, wqkv, wo, cos, sin, B, S, Hq, Hkv, D, residual=h)
                assert summed
            else:
                link = llm._DeltaLink()
                o = llm.qkv_rope_attention(x, wqkv, cos, sin, B, S, Hq, Hkv, D, link=link)
                out = llm.attn_out_proj(o.reshape(B * S, Hq * D), wo, B, S, Hq, residual=h, link=link)
            out.backward(dy)
            torch.cuda.synchronize()
            if not whole:
                assert link.ndelta is None   # filled by the projection's backward, taken by the attention's
            res.append((out.detach(), x.grad, h.grad, wqkv.main_grad, wo.main_grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)
        assert float(res[0][0].float().abs().sum()) > 0 and float(res[0][3].float().abs().sum()) > 0
    finally:
        gemm.set_mode(old)


@pytest.mark.gpu
def test_fused_predicates_mirror_the_launcher():
    """Shapes the assembly launchers refuse (csrc/hip/gemm_asm.hip) fail the
    predicates, and the callers then complete on the unfused path."""
    from tf_operator_amd.ops import gemm, llm

    _asm_lib()
    old = gemm.mode()
    gemm.set_mode("asm")
    try:
        torch.manual_seed(7)
        bf = dict(device=DEV, dtype=torch.bfloat16)
        # K = 64 < 128 in the down projection
        x = torch.randn(256, 64, **bf)
        wgu = torch.randn(128, 64, **bf) / 8
        wd = torch.randn(256, 64, **bf) / 8
        assert not llm.swiglu_mlp_resadd_ok(x, wd, torch.zeros(256, 256, **bf))
        out = llm.swiglu_mlp(x, wgu, wd)
        gu = x.float() @ wgu.float().t()
        ref = (torch.nn.functional.silu(gu[:, :64]) * gu[:, 64:]) @ wd.float().t()
        assert rel(out, ref) < 2e-2
        # a residual one element into its buffer: contiguous, data_ptr % 16 == 2
        B, S, Hq, Hkv, D, Hd = 1, 256, 4, 2, 128, 512
        xa = torch.randn(B * S, Hd, **bf)
        wqkv, wo = _weights(Hq, Hkv, D, Hd, 8)
        cos, sin = llm.rope_tables(S, D, device=DEV)
        r = torch.randn(B * S * Hd + 8, **bf)[1:1 + B * S * Hd].view(B * S, Hd)
        o = torch.randn(B * S, Hq * D, **bf)
        assert r.is_contiguous() and r.data_ptr() % 16 == 2
        assert llm.attn_out_proj_resadd_ok(o, wo, r.clone()) and not llm.attn_out_proj_resadd_ok(o, wo, r)
        with torch.no_grad():
            a, summed = llm.attention_block(xa, wqkv, wo, cos, sin, B, S, Hq, Hkv, D, residual=r)
            plain, _ = llm.attention_block(xa, wqkv, wo, cos, sin, B, S, Hq, Hkv, D)
        assert not summed and torch.equal(a, plain)
        # the RoPE launcher's 32-bit output offsets: M N 2 bytes < 2^32
        M = 524288
        xb = torch.empty(M, 128, **bf)
        wb = torch.empty((16 + 2 * 8) * 128, 128, **bf)
        assert M * wb.shape[0] * 2 == 2 ** 32
        assert not llm.qkv_rope_attention_ok(xb, wb, 256, 16, 8, 128)
        assert llm.qkv_rope_attention_ok(xb[:M - 256], wb, 256, 16, 8, 128)
    finally:
        gemm.set_mode(old)
