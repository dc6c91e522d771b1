"""The assembly GEMMs at token counts that are no multiple of their tiles
(MI355X): the TN kernels' M tail (forward / data gradient, the residual-add
and fused SwiGLU epilogues) and the NT weight-gradient kernel's T tail, vs
fp32 torch with the tolerances tests/test_ops_gpu.py uses for the same
kernels, and one training step at 600 tokens with no library fallback.

The launcher tests write into views of larger tensors: guard rows after row
M must stay untouched (the dead rows' stores are dropped by the buffer
resources' range check).  The weight-gradient operands are views of
NaN-padded tensors: the rows of the last 64-row tile past T must read as 0
through the LDS-DMA -- the measurement docs/kernels.md records."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_TAIL = 300          # two tile rows, 44 live rows in the second
GUARD = 8             # guard rows past the end of the last tile row


def _lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def guarded(rows, cols):
    """(the live [rows, cols] view, the guard rows after it) of one tensor
    that covers the whole last tile row and GUARD rows more: a dead row's
    store that is not dropped shows up in the guard, inside this tensor."""
    t = torch.full((-(-rows // 256) * 256 + GUARD, cols), 7.0, device=DEV, dtype=torch.bfloat16)
    return t[:rows], t[rows:]


@pytest.fixture
def asm_mode():
    from tf_operator_amd.ops import gemm

    _lib()
    old = gemm.mode()
    gemm.set_mode("asm")
    yield gemm
    gemm.set_mode(old)


def test_linear_fwd_m_tail(asm_mode):
    gemm, L = asm_mode, _lib()
    torch.manual_seed(1)
    M, N, K = M_TAIL, 512, 192
    x = bf(M, K)                                  # exactly M rows
    w = bf(N, K, scale=0.5)
    ref = x.float() @ w.float().t()
    out, guard = guarded(M, N)
    L.call("toa_gemm_asm_rows", L.ptr(x), K, L.ptr(w), K, L.ptr(out), N, M, N, K, L.stream(x))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    assert rel(out, ref) < 1e-2, rel(out, ref)
    # the strict entry keeps refusing a partial tile row (before any launch)
    assert L.call_ret("toa_gemm_asm", L.ptr(x), K, L.ptr(w), K, L.ptr(out), N, M, N, K, L.stream(x)) != 0
    gemm.reset_fallbacks()
    assert gemm.asm_takes(x, w)
    y = gemm.linear_fwd(x, w)
    assert torch.equal(out, y)
    assert gemm.fallbacks() == {}


def test_linear_resadd_m_tail(asm_mode):
    gemm, L = asm_mode, _lib()
    from tf_operator_amd.ops import llm

    torch.manual_seed(2)
    M, N, K = M_TAIL, 256, 256
    x, w, r = bf(M, K), bf(N, K, scale=0.2), bf(M, N)
    ref = x.float() @ w.float().t() + r.float()
    out, guard = guarded(M, N)
    L.call("toa_gemm_asm_resadd", L.ptr(x), K, L.ptr(w), K, L.ptr(out), N, L.ptr(r), M, N, K, L.stream(x))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    assert rel(out, ref) < 1e-2, rel(out, ref)
    assert llm.attn_out_proj_resadd_ok(x, w, r)
    y = gemm.linear_resadd(x, w, r)
    assert torch.equal(out, y)


def test_swiglu_launchers_m_tail_leave_guard_rows(asm_mode):
    gemm, L = asm_mode, _lib()
    from tf_operator_amd.ops import llm

    torch.manual_seed(3)
    M, F, K = M_TAIL, 256, 128
    x = bf(M, K)
    wgu = bf(2 * F, K, scale=K ** -0.5)
    gu, ggu = guarded(M, 2 * F)
    s, gs = guarded(M, F)
    L.call("toa_gemm_asm_swiglu", L.ptr(x), K, L.ptr(wgu), K, L.ptr(gu), 2 * F, L.ptr(s), F, M, F, K, L.stream(x))
    ref_gu = x.float() @ wgu.float().t()
    assert rel(gu, ref_gu) < 1e-2
    g, u = gu[:, :F].float(), gu[:, F:].float()
    assert rel(s, torch.nn.functional.silu(g) * u) < 1e-2
    wdt = bf(F, K, scale=F ** -0.5)               # W_down^T [F, K]: the kernel's operand
    d2 = bf(M, K)
    dgu, gdgu = guarded(M, 2 * F)
    L.call("toa_gemm_asm_swiglu_bwd", L.ptr(d2), K, L.ptr(wdt), K, L.ptr(gu), 2 * F, L.ptr(dgu), 2 * F, M, F, K,
           L.stream(x))
    torch.cuda.synchronize()
    ds = (d2.float() @ wdt.float().t()).to(torch.bfloat16)
    ref = llm.swiglu_bwd(ds, gu.contiguous())
    assert rel(dgu, ref) < 2e-2, rel(dgu, ref)
    for guard in (ggu, gs, gdgu):
        assert bool((guard == 7.0).all())


def test_swiglu_mlp_fwd_bwd_m_tail(asm_mode):
    """The fused MLP (gate|up GEMM with the SwiGLU epilogue, the down
    projection, its data gradient with the SwiGLU backward, the plain data
    gradient and both weight gradients) at 300 tokens vs fp32 autograd."""
    gemm = asm_mode
    from tf_operator_amd.ops import llm

    torch.manual_seed(4)
    M, H, F = M_TAIL, 256, 512
    x = bf(M, H).requires_grad_()
    wgu = bf(2 * F, H, scale=H ** -0.5).requires_grad_()
    wd = bf(H, F, scale=F ** -0.5).requires_grad_()
    for p in (wgu, wd):                           # the transposed copies the data gradients run on
        p._toa_wt = p.detach().t().contiguous()
    dout = bf(M, H)
    gemm.reset_fallbacks()
    out = llm.swiglu_mlp(x, wgu, wd)
    out.backward(dout)
    torch.cuda.synchronize()
    assert gemm.fallbacks() == {}, gemm.fallbacks()
    xf, wguf, wdf = (t.detach().float().requires_grad_() for t in (x, wgu, wd))
    guf = xf @ wguf.t()
    outf = (torch.nn.functional.silu(guf[:, :F]) * guf[:, F:]) @ wdf.t()
    outf.backward(dout.float())
    assert rel(out.detach(), outf.detach()) < 2e-2, rel(out.detach(), outf.detach())
    assert rel(x.grad, xf.grad) < 2e-2, rel(x.grad, xf.grad)
    assert rel(wgu.grad, wguf.grad) < 2e-2, rel(wgu.grad, wguf.grad)
    assert rel(wd.grad, wdf.grad) < 2e-2, rel(wd.grad, wdf.grad)


@pytest.mark.parametrize("T,beta,split", [(200, 0, None), (129, 1, None), (200, 0, 2)])
def test_wgrad_asm_t_tail_nan_padded(T, beta, split):
    """dW = dy[:T]^T x[:T] with NaN rows behind both operands: the dead rows
    of the last k-tile must add exactly 0 (LDS-DMA lanes past num_records
    write 0 into LDS)."""
    L = _lib()
    from tf_operator_amd.ops import gemm

    if gemm.wgrad_kernel() != "asm":
        pytest.fail("the assembly weight-gradient kernel is not the selected one")
    torch.manual_seed(T)
    N, K = 256, 512
    nan = float("nan")
    dyb = torch.full((T + 70, N + 256), nan, device=DEV, dtype=torch.bfloat16)
    xb = torch.full((T + 70, K), nan, device=DEV, dtype=torch.bfloat16)
    dyb[:T] = (torch.rand(T, N + 256, device=DEV) * 2 - 1).to(torch.bfloat16)
    xb[:T] = (torch.rand(T, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    dy, x = dyb[:T, 128:128 + N], xb[:T]
    g0 = (torch.rand(N, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    ref = dy.float().t() @ x.float() + (g0.float() if beta else 0)
    assert gemm.wgrad_hip_ok(g0, dy, x)
    outs = []
    for _ in range(2):
        g = g0.clone()
        gemm.wgrad_hip_(g, dy, x, beta=float(beta), split=split)
        outs.append(g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all())
    err = (outs[0].float() - ref).abs().max() / ref.abs().max()
    assert err < 1e-2, float(err)
    assert torch.equal(outs[0], outs[1])
    # under 65 tokens (one k-tile) the kernel's pipeline has nothing to run on: refused
    assert L.call_ret("toa_wgrad_asm", L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), L.ptr(g0), K, None, N, K, 64, 0,
                      0, L.stream(g0)) != 0


def test_trainer_step_at_600_tokens_has_no_gemm_fallback(monkeypatch):
    """llama-tiny128 at micro-batch 3 x seq 200: every GEMM of the step runs
    on the assembly kernels (the attention itself takes the HIP kernels at
    S % 256 != 0), and the loss follows the library policy's."""
    from tf_operator_amd.ops import gemm
    from tf_operator_amd.train.llm import LlamaTrainer

    _lib()
    # the library policy's trainer starts the process-wide plan prewarm
    # (gemm.prewarm); it is this test's own and gone with it, so a later
    # prewarm in this process starts from scratch
    monkeypatch.setattr(gemm, "_prewarm_thread", None)
    monkeypatch.setattr(gemm, "_prewarm_dev", None)
    losses = {}
    for mode in ("nosk", "asm"):
        monkeypatch.setattr(gemm, "_MODE", mode)
        monkeypatch.setattr(gemm, "_installed", False)
        gemm.reset_fallbacks()
        tr = LlamaTrainer("llama-tiny128", torch.device(DEV), micro_batch=3, seq_len=200, seed=0)
        b = tr.synthetic_batch()
        losses[mode] = [float(tr.step([b])) for _ in range(2)]
        del tr
        if gemm._prewarm_thread is not None:
            gemm._prewarm_thread.join(60)
            assert not gemm._prewarm_thread.is_alive()
        if mode == "asm":
            assert gemm.fallbacks() == {}, gemm.fallbacks()
    for a, b in zip(losses["nosk"], losses["asm"]):
        assert abs(a - b) < 2e-2 * abs(a), losses
