"""toa_gemm_shape_check and the launchers give one answer (MI355X): per
product form the smallest operands it takes and one refused neighbour --
the query is 0 exactly when the launcher returns 0, a refusal is
hipErrorInvalidValue before any launch, and what was launched matches fp32
torch at the tolerances tests/test_gemm_tails_gpu.py uses for these kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
INVALID_VALUE = 1


@pytest.fixture(scope="module")
def L():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf(rows, cols, scale=1.0, off=0):
    """[rows, cols] bf16; off: elements into its buffer (4 = 8 bytes: contiguous, misaligned)."""
    t = (torch.randn(rows * cols + 8, device=DEV) * scale).to(torch.bfloat16)
    return t[off:off + rows * cols].view(rows, cols)


def agree(L, form, fn, tensors, lds, dims, args, taken, **extra):
    """The query's answer, the launcher's, and that they are the expected one."""
    reason = L.shape_check(form, tensors, lds, *dims, **extra)
    rc = L.call_ret(fn, *args, L.stream(tensors[0]))
    torch.cuda.synchronize()
    assert (reason == 0) == (rc == 0), (form, fn, reason, L.shape_why(reason), rc)
    assert rc == (0 if taken else INVALID_VALUE), (form, fn, rc, L.shape_why(reason))
    assert (reason == 0) == taken, L.shape_why(reason)


@pytest.mark.parametrize("form,fn,M,N,K,off,taken", [
    ("tn", "toa_gemm_asm", 256, 256, 128, 0, True), ("tn", "toa_gemm_asm", 257, 256, 128, 0, False),
    ("tn", "toa_gemm_asm", 256, 384, 128, 0, False),
    ("tn_rows", "toa_gemm_asm_rows", 256, 256, 128, 0, True), ("tn_rows", "toa_gemm_asm_rows", 257, 256, 128, 0, True),
    ("tn_rows", "toa_gemm_asm_rows", 257, 256, 160, 0, False),
    ("tn_resadd", "toa_gemm_asm_resadd", 256, 256, 128, 0, True),
    ("tn_resadd", "toa_gemm_asm_resadd", 257, 256, 128, 0, True),
    ("tn_resadd", "toa_gemm_asm_resadd", 257, 256, 128, 4, False),
    ("nn", "toa_gemm_nn_asm", 256, 256, 128, 0, True), ("nn", "toa_gemm_nn_asm", 257, 256, 128, 0, True),
    ("nn", "toa_gemm_nn_asm", 257, 384, 128, 0, False)])
def test_plain_forms(L, form, fn, M, N, K, off, taken):
    """off: the residual 8 bytes into its buffer."""
    torch.manual_seed(M + N + K)
    x = bf(M, K)
    w = bf(K, N, 0.5) if form == "nn" else bf(N, K, 0.5)
    r = bf(M, N, off=off) if form == "tn_resadd" else None
    y = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
    res = (L.ptr(r),) if r is not None else ()
    agree(L, form, fn, (x, w, y, r), (x.stride(0), w.stride(0), N), (M, N, K),
          (L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(y), N, *res, M, N, K), taken)
    if not taken:
        assert bool((y == 7.0).all())
        return
    ref = x.float() @ (w.float() if form == "nn" else w.float().t()) + (r.float() if r is not None else 0)
    assert rel(y, ref) < 1e-2, rel(y, ref)


@pytest.mark.parametrize("M,F,K,off,taken", [(256, 128, 128, 0, True), (257, 128, 128, 0, True), (256, 128, 128, 4, False)])
def test_swiglu_forward(L, M, F, K, off, taken):
    """off: x 8 bytes into its buffer."""
    torch.manual_seed(F)
    x, wgu = bf(M, K, off=off), bf(2 * F, K, K ** -0.5)
    gu = torch.full((M, 2 * F), 7.0, device=DEV, dtype=torch.bfloat16)
    s = torch.full((M, F), 7.0, device=DEV, dtype=torch.bfloat16)
    agree(L, "tn_swiglu_fwd", "toa_gemm_asm_swiglu", (x, wgu, gu, s), (K, K, 2 * F, F), (M, F, K),
          (L.ptr(x), K, L.ptr(wgu), K, L.ptr(gu), 2 * F, L.ptr(s), F, M, F, K), taken)
    if not taken:
        assert bool((gu == 7.0).all()) and bool((s == 7.0).all())
        return
    assert rel(gu, x.float() @ wgu.float().t()) < 1e-2
    g, u = gu[:, :F].float(), gu[:, F:].float()
    assert rel(s, torch.nn.functional.silu(g) * u) < 1e-2


@pytest.mark.parametrize("form,fn,M,F,K,off,taken", [
    ("tn_swiglu_bwd", "toa_gemm_asm_swiglu_bwd", 256, 256, 128, 0, True),
    ("tn_swiglu_bwd", "toa_gemm_asm_swiglu_bwd", 256, 256, 160, 0, False),
    ("nn_swiglu_bwd", "toa_gemm_nn_asm_swiglu_bwd", 256, 256, 128, 0, True),
    ("nn_swiglu_bwd", "toa_gemm_nn_asm_swiglu_bwd", 256, 256, 128, 4, False)])
def test_swiglu_backward(L, form, fn, M, F, K, off, taken):
    """dgu from dY [M, K] and W_down^T [F, K] (TN) or W_down [K, F] (NN); off: gu 8 bytes into its buffer."""
    from tf_operator_amd.ops import llm

    torch.manual_seed(F + K)
    d2 = bf(M, K)
    w = bf(K, F, F ** -0.5) if form.startswith("nn") else bf(F, K, F ** -0.5)
    gu = bf(M, 2 * F, off=off)
    dgu = torch.full((M, 2 * F), 7.0, device=DEV, dtype=torch.bfloat16)
    agree(L, form, fn, (d2, w, dgu, gu), (K, w.stride(0), 2 * F, 2 * F), (M, F, K),
          (L.ptr(d2), K, L.ptr(w), w.stride(0), L.ptr(gu), 2 * F, L.ptr(dgu), 2 * F, M, F, K), taken)
    if not taken:
        assert bool((dgu == 7.0).all())
        return
    ds = (d2.float() @ (w.float() if form.startswith("nn") else w.float().t())).to(torch.bfloat16)
    ref = llm.swiglu_bwd(ds, gu.contiguous())
    assert rel(dgu, ref) < 2e-2, rel(dgu, ref)


@pytest.mark.parametrize("S,taken", [(256, True), (128, False)])
def test_rope(L, S, taken):
    from tf_operator_amd.ops import llm

    torch.manual_seed(S)
    M, K, Hq, Hkv, D = 256, 128, 2, 1, 128
    B, N = M // S, (Hq + 2 * Hkv) * D
    x, w = bf(M, K), bf(N, K, K ** -0.5)
    cos, sin = llm.rope_tables(S, D, device=DEV)
    cossin = llm.rope_cossin(cos, sin)
    out = torch.full((M * N,), 7.0, device=DEV, dtype=torch.bfloat16)
    agree(L, "tn_rope", "toa_gemm_asm_rope", (x, w, out, cossin), (K, K), (M, 0, K),
          (L.ptr(x), K, L.ptr(w), K, L.ptr(out), L.ptr(cossin), M, K, S, Hq, Hkv), taken, S=S, Hq=Hq, Hkv=Hkv)
    if not taken:
        assert bool((out == 7.0).all())
        return
    qkv = (x.float() @ w.float().t()).view(B, S, Hq + 2 * Hkv, D).transpose(1, 2)
    ref = torch.cat([llm._rope_ref(qkv[:, :Hq], cos, sin).flatten(), llm._rope_ref(qkv[:, Hq:Hq + Hkv], cos, sin).flatten(),
                     qkv[:, Hq + Hkv:].flatten()])
    assert rel(out, ref) < 1e-2, rel(out, ref)


@pytest.mark.parametrize("form,fn", [("tn_delta", "toa_gemm_asm_delta"), ("nn_delta", "toa_gemm_nn_asm_delta")])
@pytest.mark.parametrize("S,taken", [(256, True), (128, False)])
def test_delta(L, form, fn, S, taken):
    torch.manual_seed(S + len(form))
    M, N, K, H = 256, 256, 128, 2
    B = M // S
    dy = bf(M, K)
    w = bf(K, N, K ** -0.5) if form == "nn_delta" else bf(N, K, K ** -0.5)
    o = bf(M, N)
    dx = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
    nd = torch.full((B * H * S,), 7.0, device=DEV, dtype=torch.float32)
    agree(L, form, fn, (dy, w, dx, o, nd), (K, w.stride(0), N), (M, N, K),
          (L.ptr(dy), K, L.ptr(w), w.stride(0), L.ptr(dx), N, L.ptr(o), L.ptr(nd), M, N, K, S, H), taken, S=S, H=H)
    if not taken:
        assert bool((dx == 7.0).all()) and bool((nd == 7.0).all())
        return
    assert rel(dx, dy.float() @ (w.float() if form == "nn_delta" else w.float().t())) < 1e-2
    ref = -(dx.float() * o.float()).view(B, S, H, 128).sum(-1).permute(0, 2, 1).reshape(-1)
    assert rel(nd, ref) < 1e-2, rel(nd, ref)


@pytest.mark.parametrize("form,fn,ws_fn,T,off,taken", [
    ("wgrad_asm", "toa_wgrad_asm", "toa_wgrad_asm_workspace", 65, 0, True),
    ("wgrad_asm", "toa_wgrad_asm", "toa_wgrad_asm_workspace", 1024, 0, True),
    ("wgrad_asm", "toa_wgrad_asm", "toa_wgrad_asm_workspace", 64, 0, False),
    ("wgrad_hip", "toa_wgrad", "toa_wgrad_workspace", 1024, 0, True),
    ("wgrad_hip", "toa_wgrad", "toa_wgrad_workspace", 64, 0, False),
    ("wgrad_hip", "toa_wgrad", "toa_wgrad_workspace", 1024, 4, False)])
def test_weight_gradient(L, form, fn, ws_fn, T, off, taken):
    """off: x 8 bytes into its buffer."""
    torch.manual_seed(T)
    N = K = 256
    dy, x = bf(T, N), bf(T, K, off=off)
    g = torch.full((N, K), 7.0, device=DEV, dtype=torch.bfloat16)
    nbytes = int(L.call_ret(ws_fn, N, K, T, 0))
    ws = torch.empty(nbytes // 4, device=DEV, dtype=torch.float32) if nbytes else None
    agree(L, form, fn, (dy, x, g, ws), (N, K, K), (N, K, T), (L.ptr(dy), N, L.ptr(x), K, L.ptr(g), K, L.ptr(ws), N, K, T, 0, 0),
          taken)
    if not taken:
        assert bool((g == 7.0).all())
        return
    ref = dy.float().t() @ x.float()
    err = (g.float() - ref).abs().max() / ref.abs().max()
    assert err < 1e-2, float(err)
