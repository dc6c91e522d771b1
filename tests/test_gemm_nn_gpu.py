"""The NN-form assembly GEMMs on an MI355X (csrc/asm/gemm_gen.py kernel_nn,
csrc/hip/gemm_asm.hip toa_gemm_nn_asm*): the data gradient dX = dY W read
from the weight as stored, the ``TOA_DGRAD=nn`` switch of ops/gemm.py and the
trainer without transposed weight copies.

Tolerances are the project's own for the same kernels in the TN form
(tests/test_ops_gpu.py): rel < 1e-2 against fp32 torch for a plain GEMM, 2e-2
for the fused SwiGLU backward, 1e-4 for the delta rows, 2e-2 between the loss
trajectories of two trainers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8


def _lib():
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    return _lib


def rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def guarded(rows, cols):
    """(the live [rows, cols] view, the guard rows after it) of one tensor
    that covers the whole last tile row and GUARD rows more (as in
    tests/test_gemm_tails_gpu.py)."""
    t = torch.full((-(-rows // 256) * 256 + GUARD, cols), 7.0, device=DEV, dtype=torch.bfloat16)
    return t[:rows], t[rows:]


def nn(L, x, w, y, M, N, K):
    return L.call_ret("toa_gemm_nn_asm", L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(y), y.stride(0), M, N, K,
                      L.stream(y))


@pytest.fixture
def nn_form():
    """The asm policy with the NN data-gradient form; both restored."""
    from tf_operator_amd.ops import gemm

    _lib()
    old_mode, old_form = gemm.mode(), gemm.dgrad_form()
    gemm.set_mode("asm")
    gemm.set_dgrad_form("nn")
    gemm.reset_fallbacks()
    yield gemm
    gemm.set_mode(old_mode)
    gemm.set_dgrad_form(old_form)
    gemm.reset_fallbacks()


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 384), (768, 512, 256), (1024, 1536, 1152)])
def test_gemm_nn_asm_matches_fp32(M, N, K):
    """y = x w with w [K, N] as stored, padded strides on all three operands,
    C a column window of a larger tensor whose other columns keep their fill."""
    L = _lib()
    torch.manual_seed(M + N + K)
    xb = torch.randn(M, K + 64, device=DEV).to(torch.bfloat16)[:, :K]
    wb = (torch.randn(K, N + 40, device=DEV) * 0.5 + torch.arange(K, device=DEV)[:, None] / K).to(torch.bfloat16)
    w = wb[:, :N]
    yb = torch.full((M, N + 256), 7.0, device=DEV, dtype=torch.bfloat16)
    y = yb[:, 128:128 + N]
    assert nn(L, xb, w, y, M, N, K) == 0
    ref = xb.float() @ w.float()
    torch.cuda.synchronize()
    assert rel(y, ref) < 1e-2, rel(y, ref)
    assert bool((yb[:, :128] == 7.0).all()) and bool((yb[:, 128 + N:] == 7.0).all())  # nothing outside C


def test_gemm_nn_asm_m_tail():
    L = _lib()
    M, N, K = 300, 512, 192
    torch.manual_seed(5)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = torch.randn(K, N, device=DEV).to(torch.bfloat16)
    y, guard = guarded(M, N)
    assert nn(L, x, w, y, M, N, K) == 0
    torch.cuda.synchronize()
    assert rel(y, x.float() @ w.float()) < 1e-2
    assert bool((guard == 7.0).all())


@pytest.mark.parametrize("M,N,K", [(512, 512, 128), (768, 1280, 640)])
def test_gemm_nn_asm_repeatable_bit_for_bit(M, N, K):
    """Eleven launches agree bit for bit (a staging race would differ)."""
    L = _lib()
    torch.manual_seed(K)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = torch.randn(K, N, device=DEV).to(torch.bfloat16)
    ys = []
    for _ in range(11):
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        assert nn(L, x, w, y, M, N, K) == 0
        ys.append(y)
    torch.cuda.synchronize()
    assert rel(ys[0], x.float() @ w.float()) < 1e-2
    for y in ys[1:]:
        assert torch.equal(ys[0], y)


def test_gemm_nn_asm_refusals():
    """N = 200, K = 96, K = 64 and an unaligned base: rc != 0, output untouched."""
    L = _lib()
    x = torch.randn(256, 136, device=DEV).to(torch.bfloat16)
    w = torch.randn(128, 264, device=DEV).to(torch.bfloat16)
    y = torch.full((256, 256), 7.0, device=DEV, dtype=torch.bfloat16)
    for M, N, K in ((256, 200, 128), (256, 256, 96), (256, 256, 64)):
        assert nn(L, x, w, y, M, N, K) != 0, (M, N, K)
    for xs, ws in ((x[:, 1:129], w[:, :256]), (x[:, :128], w[:, 1:257])):     # bases 2 bytes off
        assert nn(L, xs, ws, y, 256, 256, 128) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert nn(L, x[:, :128], w[:, :256], y, 256, 256, 128) == 0                # the same operands, aligned: taken
    torch.cuda.synchronize()
    assert rel(y, x[:, :128].float() @ w[:, :256].float()) < 1e-2


def test_linear_dgrad_nn_form(nn_form):
    gemm = nn_form
    L = _lib()
    torch.manual_seed(9)
    w = torch.nn.Parameter(torch.randn(768, 512, device=DEV).to(torch.bfloat16))
    dy = torch.randn(2048, 768, device=DEV).to(torch.bfloat16)
    ref = dy.float() @ w.float()
    assert gemm.nn_takes(dy, w)
    got = gemm.linear_dgrad(dy, w)
    assert (got.float() - ref).abs().max() <= 1e-2 * ref.abs().max()
    direct = torch.empty_like(got)
    assert nn(L, dy, w.data, direct, 2048, 512, 768) == 0
    torch.cuda.synchronize()
    assert torch.equal(got, direct)
    assert gemm.fallbacks() == {}
    # a weight the NN kernel refuses: the counted fallback names the failed check
    w_odd = torch.randn(768, 200, device=DEV).to(torch.bfloat16)
    assert not gemm.nn_takes(dy, w_odd)
    gemm.linear_dgrad(dy, w_odd)
    (key,) = gemm.fallbacks()
    assert key.startswith("dgrad 2048x200x768")
    # the default form: the same call still counts its fallback
    gemm.reset_fallbacks()
    gemm.set_dgrad_form("wt")
    got_wt = gemm.linear_dgrad(dy, w)
    assert list(gemm.fallbacks()) and all(k.startswith("dgrad 2048x512x768") for k in gemm.fallbacks())
    assert (got_wt.float() - ref).abs().max() <= 1e-2 * ref.abs().max()
    with pytest.raises(ValueError):
        gemm.set_dgrad_form("tn")


@pytest.mark.parametrize("M,F,K", [(256, 128, 128), (512, 384, 256), (1024, 1024, 1024), (300, 512, 256)])
def test_swiglu_mlp_nn_form(nn_form, M, F, K):
    """swiglu_mlp forward + backward with no ``_toa_wt`` on any weight (the
    shapes of test_gemm_asm_swiglu_epilogues, and one that the fused NN kernel
    takes with a token tail, M = 300): where the kernels take them (F
    and K multiples of 256) the down projection's data gradient runs the
    fused NN kernel on wd [K, F] and nothing falls back; elsewhere the node
    takes the unfused pass, as it does today without a W^T copy."""
    from tf_operator_amd.ops import llm

    gemm = nn_form
    torch.manual_seed(3)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16).requires_grad_()
    wgu = torch.nn.Parameter((torch.randn(2 * F, K, device=DEV) / K ** 0.5).to(torch.bfloat16))
    wd = torch.nn.Parameter((torch.randn(K, F, device=DEV) / F ** 0.5).to(torch.bfloat16))
    for p in (wgu, wd):
        p.main_grad = torch.zeros_like(p)
        assert not hasattr(p, "_toa_wt")
    # the fused kernel itself against the unfused formula
    gu, s = gemm.swiglu_gate_up(x.detach(), wgu)
    d2 = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    dgu = gemm.swiglu_down_dgrad(d2, wd, gu)
    ds = (d2.float() @ wd.float()).to(torch.bfloat16)
    assert (dgu is not None) == (F % 256 == 0)
    if dgu is not None:
        assert rel(dgu, llm.swiglu_bwd(ds, gu)) < 2e-2
    # the whole node against fp32 autograd
    out = llm.swiglu_mlp(x, wgu, wd)
    out.backward(d2)
    xr = x.detach().float().requires_grad_()
    gur = xr @ wgu.float().t()
    outr = (torch.nn.functional.silu(gur[:, :F]) * gur[:, F:]) @ wd.float().t()
    outr.backward(d2.float())
    torch.cuda.synchronize()
    assert rel(out, outr) < 2e-2 and rel(x.grad, xr.grad) < 2e-2
    if F % 256 == 0 and K % 256 == 0:
        assert not any(k.startswith("dgrad") for k in gemm.fallbacks()), gemm.fallbacks()


def test_attn_out_proj_delta_rows_nn_form(nn_form):
    """_AttnOutProj without a W^T copy: toa_gemm_nn_asm_delta's dX equals the
    plain NN data gradient bit for bit and leaves -rowsum(dO * O) per head."""
    from tf_operator_amd.ops import llm

    gemm = nn_form
    torch.manual_seed(8)
    B, S, H, D = 2, 512, 4, 128
    o = torch.randn(B * S, H * D, device=DEV).to(torch.bfloat16).requires_grad_()
    wo = torch.nn.Parameter((torch.randn(H * D, H * D, device=DEV) / (H * D) ** 0.5).to(torch.bfloat16))
    wo.main_grad = torch.zeros_like(wo)
    dy = torch.randn(B * S, H * D, device=DEV).to(torch.bfloat16)
    link = llm._DeltaLink()
    llm.attn_out_proj(o, wo, B, S, H, link=link).backward(dy)
    torch.cuda.synchronize()
    assert not hasattr(wo, "_toa_wt")
    assert link.ndelta is not None and link.do_ptr == o.grad.data_ptr() and link.numel == o.grad.numel()
    assert torch.equal(o.grad, gemm.linear_dgrad(dy, wo))
    assert rel(o.grad, dy.float() @ wo.float()) < 1e-2
    ref = -(o.grad.float() * o.detach().float()).view(B, S, H, D).sum(-1).permute(0, 2, 1).reshape(-1)
    assert rel(link.ndelta, ref) < 1e-4
    assert gemm.fallbacks() == {}


_TRAINER_CHILD = """
import gc, json, torch
from tf_operator_amd.models.llama import PRESETS
from tf_operator_amd.ops import gemm
from tf_operator_amd.train.llm import LlamaTrainer

gemm.set_mode("asm")
out = {}
for form in ("wt", "nn"):
    gemm.set_dgrad_form(form)
    gemm.reset_fallbacks()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    tr = LlamaTrainer(PRESETS["llama-tiny"], torch.device("cuda"), micro_batch=2, seq_len=128, lr=1e-3,
                      bucket_mb=0.25)
    b = tr.synthetic_batch()
    losses = [float(tr.step([b])) for _ in range(4)]
    tr.opt.wait_all()
    torch.cuda.synchronize()
    out[form] = {"losses": losses, "peak": torch.cuda.max_memory_allocated(), "wt_is_none": tr.wt is None,
                 "wt_nbytes": tr.wt.nbytes if tr.wt else 0, "fused_wt": getattr(tr.opt, "fused_wt", None) is not None,
                 "fallbacks": sorted(gemm.fallbacks())}
    del tr, b
print("RESULT " + json.dumps(out))
"""


def test_trainer_nn_form_has_no_transposed_weights():
    """llama-tiny, 4 steps (the preset and step count of
    test_trainer_transposed_weights_refresh), once with the W^T copies and
    once with the NN data gradient: the same loss trajectory to bf16 GEMM
    rounding, no W^T buffer, no data-gradient fallback, and
    torch.cuda.max_memory_allocated lower by at least the copies' bytes.

    In a child process: max_memory_allocated counts the caching allocator's
    blocks, and which cached block serves a request depends on everything the
    process allocated before -- after the other tests of a session the two
    peaks move by up to a MiB each (measured: 30140928 / 28288000 bytes in
    this session against 31174144 / 27519488 in a fresh process, the copies
    being 2621440), in a fresh one they repeat to the byte."""
    import json
    import os
    import subprocess
    import sys

    _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("TOA_DGRAD", None)
    r = subprocess.run([sys.executable, "-c", _TRAINER_CHILD], cwd=root, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    runs = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    print("nn-form trainer:", runs)
    wt, nn_ = runs["wt"], runs["nn"]
    assert nn_["wt_is_none"] and not nn_["fused_wt"] and not wt["wt_is_none"] and wt["wt_nbytes"] > 0
    for r_ in (wt, nn_):
        assert not any(k.startswith("dgrad") for k in r_["fallbacks"]), r_["fallbacks"]
    assert max(abs(a - c) for a, c in zip(nn_["losses"], wt["losses"])) < 2e-2, runs
    assert nn_["peak"] <= wt["peak"] - wt["wt_nbytes"], runs
