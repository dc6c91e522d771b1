"""The 1-to-16-row GEMM on the CPU tier: the bound of tests/skinny_numerics.py
against the CPU reference and against planted errors, the Python predicates
against the header's reasons (csrc/hip/gemm_skinny_shapes.h), the boundary
table (csrc/hip/tests/gemm_skinny_selftest.cc, built alone under ASan + UBSan
and run as its own process), and the model with ``gemm="skinny"``."""
import os
import re
import subprocess

import pytest
import torch

import skinny_numerics as sn
import test_decode as td
from tf_operator_amd.ops import _lib, gemm
from tf_operator_amd.ops import decode as dec
from tf_operator_amd.train.generate import generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "csrc", "hip")
BF16 = torch.bfloat16


def _header():
    with open(os.path.join(HIP, "gemm_skinny_shapes.h")) as f:
        return f.read()


def _reasons():
    body = re.search(r"enum Reason \{(.*?)\};", _header(), re.S).group(1)
    names = re.findall(r"^\s*(R_\w+)", body, re.M)
    assert names[0] == "R_OK" and names[-1] == "R_COUNT"
    return {n: i for i, n in enumerate(names[:-1])}


def test_selftest_asan_ubsan(tmp_path):
    exe = str(tmp_path / "gemm_skinny_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(HIP, "tests", "gemm_skinny_selftest.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "gemm skinny selftest OK" in r.stdout


def test_restated_constants_and_plan_follow_the_header():
    text = _header()
    for name in ("MAX_M", "TILE_N", "KSTEP", "WAVES", "UNROLL", "MIN_WGS"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) == getattr(sn, name), name
    with open(os.path.join(HIP, "gemm_skinny.hip")) as f:
        assert f"gemm_skinny_merge_kernel<SWIGLU>), dim3((unsigned)((units + {sn.MERGE_BLOCK - 1}) / {sn.MERGE_BLOCK}))" \
            in f.read()
    assert _lib.available(), _lib.load_error()
    for N, K in sn.SHAPES + [(4096, 4096), (2048, 8192), (128256, 4096)]:
        assert _lib.call_ret("toa_gemm_skinny_split", N, K) == sn.split_of(N, K), (N, K)
        assert _lib.call_ret("toa_gemm_skinny_slice_steps", N, K) == sn.slice_steps(N, K), (N, K)
    # the paths the GPU cases are named for
    assert sn.split_of(*sn.CASE_B) == 1 and sn.slice_steps(*sn.CASE_B) == sn.UNROLL + 1
    assert -(-sn.CASE_B[1] // sn.KSTEP) == sn.WAVES * (sn.UNROLL + 1) and sn.CASE_B[1] % sn.KSTEP == 8
    assert -(-sn.CASE_C[1] // sn.KSTEP) < sn.WAVES
    assert sn.split_of(*sn.CASE_D) == 2 and sn.split_of(sn.CASE_D[0], sn.CASE_D[1] - sn.KSTEP) == 1
    assert sn.split_of(*sn.CASE_A) == 2 and (sn.MAX_M * sn.CASE_A[0] // 4) % sn.MERGE_BLOCK not in (0, sn.MAX_M * sn.CASE_A[0] // 4)
    ws = _lib.call_ret("toa_gemm_skinny_ws_bytes", *sn.CASE_D)
    assert ws == 2 * sn.MAX_M * sn.CASE_D[0] * 4 and _lib.call_ret("toa_gemm_skinny_swiglu_ws_bytes", *sn.CASE_D) == 2 * ws
    assert _lib.call_ret("toa_gemm_skinny_ws_bytes", *sn.CASE_B) == 0


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", sn.SHAPES, ids=lambda v: str(v))
def test_cpu_reference_is_inside_the_bound(N, K, swiglu):
    x, w, ref, bound = sn.reference(N, K, swiglu)
    f = gemm.swiglu_skinny if swiglu else gemm.linear_skinny
    for M in sn.MS:
        got = f(x[:M], w)
        assert got.shape == (M, N) and got.dtype == BF16
        sn.check(f"cpu {'swiglu' if swiglu else 'plain'} M={M} N={N} K={K}", got, ref[:M], bound[:M])


@pytest.mark.parametrize("N,K", [(48, 520), sn.CASE_B, sn.CASE_D], ids=lambda v: str(v))
def test_planted_errors_are_rejected(N, K):
    x, w, ref, bound = sn.reference(N, K)
    xd, wd = x.double(), w.double()
    good = ref.to(BF16)
    assert sn.ok(good, ref, bound)
    # the last 8-element K chunk of one row dropped
    y = ref.clone()
    y[5] = xd[5, :K - 8] @ wd[:, :K - 8].t()
    assert not sn.ok(y.to(BF16), ref, bound), "a dropped last chunk of 8 columns passed"
    # one K slice's partial left out of the merge: the last non-empty wave slice of the plan
    per = sn.slice_steps(N, K) * sn.KSTEP
    last = (-(-K // per) - 1) * per
    y = xd[:, :last] @ wd[:, :last].t()
    assert not sn.ok(y.to(BF16), ref, bound), "a missing slice passed"
    # row m answered with row m - 1's x
    y = ref.clone()
    y[3] = ref[2]
    assert not sn.ok(y.to(BF16), ref, bound), "row 3 from row 2's x passed"
    # gate and up swapped
    xs, wgu, sref, sbound = sn.reference(N, K, True)
    assert sn.ok(sref.to(BF16), sref, sbound)
    swapped, _ = sn.swiglu_ref64(xs, torch.cat([wgu[N:], wgu[:N]]))
    assert not sn.ok(swapped.to(BF16), sref, sbound), "gate and up swapped passed"
    # and a NaN is no pass
    y = good.clone()
    y[0, 0] = float("nan")
    assert not sn.ok(y, ref, bound)


def test_every_reason_is_reachable_from_python():
    R = _reasons()
    x = torch.zeros(8, 520, dtype=BF16)
    w = torch.zeros(48, 520, dtype=BF16)
    wgu = torch.zeros(96, 520, dtype=BF16)
    seen = {}

    def hit(name, reason, refusal):
        assert reason == R[name], (name, reason, gemm.skinny_why(reason))
        assert gemm.skinny_why(reason) in refusal, (name, refusal)
        seen[name] = refusal

    assert gemm.skinny_reason(x, w) == 0 == gemm.skinny_reason(x, wgu, swiglu=True)
    assert gemm.skinny_refusal(x, w) == "" == gemm.skinny_refusal(x, wgu, swiglu=True)
    assert not gemm.skinny_takes(x, w)                 # CPU tensors: the reference, not the kernel
    for xx, ww, name in ((torch.zeros(0, 520, dtype=BF16), w, "R_M"), (torch.zeros(17, 520, dtype=BF16), w, "R_M"),
                         (x, w[:8], "R_N"), (x[:, :12], w[:, :12], "R_K"),
                         (torch.zeros(8, 12, dtype=BF16)[:, :8], torch.zeros(48, 8, dtype=BF16), "R_LD"),
                         (torch.zeros(8 * 520 + 1, dtype=BF16)[1:].view(8, 520), w, "R_ALIGN")):
        for sw, wt in ((False, ww), (True, torch.cat([ww, ww]) if ww.is_contiguous() else ww)):
            if sw and not wt.is_contiguous():
                continue
            hit(name, gemm.skinny_reason(xx, wt, sw), gemm.skinny_refusal(xx, wt, sw))
            with pytest.raises(ValueError, match="toa_gemm_skinny"):
                (gemm.swiglu_skinny if sw else gemm.linear_skinny)(xx, wt)
    odd = torch.zeros(97, 520, dtype=BF16)             # F = 48 and one row more: not gate | up
    hit("R_W_ROWS", gemm.skinny_reason(x, odd, swiglu=True), gemm.skinny_refusal(x, odd, swiglu=True))
    # the workspace is the wrappers' own (ops.gemm._workspace): a caller's misaligned one, where K is split
    xd, wd = torch.zeros(8, sn.CASE_D[1], dtype=BF16), torch.zeros(sn.CASE_D[0], sn.CASE_D[1], dtype=BF16)
    bad_ws = torch.zeros(1024, dtype=torch.float32)[1:]
    assert gemm.skinny_reason(xd, wd) == 0 and gemm.skinny_reason(x, w, ws=bad_ws) == 0
    r = gemm.skinny_reason(xd, wd, ws=bad_ws)
    hit("R_WORKSPACE", r, gemm.skinny_why(r))
    r = _lib.call_ret("toa_gemm_skinny_check", 2, x.data_ptr(), w.data_ptr(), x.data_ptr(), None, 520, 520, 48, 48, 8, 48,
                      520)
    hit("R_FORM", r, gemm.skinny_why(r))
    assert set(seen) == set(R) - {"R_OK"}, sorted(set(R) - set(seen))
    # what the launchers cannot see: the tensors' kind
    assert "column stride" in gemm.skinny_refusal(x.t().contiguous().t(), w)
    assert "columns against" in gemm.skinny_refusal(x, torch.zeros(48, 512, dtype=BF16))
    assert "matrix" in gemm.skinny_refusal(x[0], w)
    assert "differ" in gemm.skinny_refusal(x, w.float())
    assert gemm.skinny_refusal(x.float(), w.float()) == ""        # CPU: any float dtype takes the reference


# ------------------------------------------------------------------ the model on the CPU
def test_decode_step_skinny_within_the_teacher_forcing_rule():
    f = td._fixture()
    m, tokens, full = f["model"], f["tokens"], f["full"]
    gemm.reset_fallbacks()
    cache = m.new_cache(2, td.TOTAL)
    worst = 0.0
    logits = m.prefill(tokens[:, :td.PROMPT], cache, gemm="skinny")
    for t in range(td.PROMPT - 1, td.TOTAL):
        if t >= td.PROMPT:
            logits = m.decode_step(tokens[:, t], cache, gemm="skinny")
        assert logits.shape == (2, m.cfg.vocab_size)
        e = td._row_dev(logits, full[:, t], f["ref"][:, t])
        worst = max(worst, e)
        assert e <= f["tol"], f"position {t}: skinny decode logits off by {e:.3e} of the row's norm, limit {f['tol']:.3e}"
    print(f"skinny decode vs full forward: {worst:.3e} (limit {f['tol']:.3e})")
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()


def test_generate_skinny_shapes_and_bad_names(monkeypatch):
    f = td._fixture()
    m, prompts = f["model"], f["tokens"][:, :td.PROMPT]
    out, lengths = generate(m, prompts, 6, gemm="skinny")
    assert out.shape == (2, td.PROMPT + 6) and lengths.tolist() == [td.PROMPT + 6] * 2
    assert torch.equal(out[:, :td.PROMPT], prompts)
    cache = m.new_cache(2, 8)
    m.prefill(prompts, cache)
    snap = [t.clone() for t in cache.k + cache.v]
    for call in (lambda: m.decode_step(prompts[:, 0], cache, gemm="bogus"),
                 lambda: m.prefill(prompts, m.new_cache(2, 8), gemm="bogus"),
                 lambda: generate(m, prompts, 2, gemm="bogus")):
        with pytest.raises(ValueError, match="bogus"):
            call()
    monkeypatch.setenv("TOA_DECODE_GEMM", "bogus")
    with pytest.raises(ValueError, match="TOA_DECODE_GEMM"):
        m.decode_step(prompts[:, 0], cache)
    assert cache.host_lengths == [td.PROMPT] * 2 and all(torch.equal(a, b) for a, b in zip(snap, cache.k + cache.v))
    monkeypatch.setenv("TOA_DECODE_GEMM", "skinny")
    assert dec.check_gemm(None) == "skinny" and dec.check_gemm("tile") == "tile"
    monkeypatch.delenv("TOA_DECODE_GEMM")
    assert dec.check_gemm(None) == "tile"


def test_seventeen_rows_take_tile_and_count_one_key_per_shape():
    m = td._fixture()["model"]
    cfg = m.cfg
    tokens = torch.randint(0, cfg.vocab_size, (17, 4), generator=torch.Generator().manual_seed(3))
    gemm.reset_fallbacks()
    ca, cb = m.new_cache(17, 8), m.new_cache(17, 8)
    a = [m.prefill(tokens[:, :2], ca, gemm="skinny")] + [m.decode_step(tokens[:, t], ca, gemm="skinny") for t in (2, 3)]
    counted = {k: v for k, v in gemm.fallbacks().items() if k.startswith("decode")}
    b = [m.prefill(tokens[:, :2], cb, gemm="tile")] + [m.decode_step(tokens[:, t], cb, gemm="tile") for t in (2, 3)]
    for x, y in zip(a, b):
        assert torch.equal(x, y)                        # the tile path itself
    qkv = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
    want = {}   # keyed by shape: at llama-tiny the head [512, 256] has the qkv projection's shape
    for N, K, n in ((qkv, cfg.hidden, 2 * cfg.layers), (cfg.hidden, cfg.heads * cfg.head_dim, 2 * cfg.layers),
                    (2 * cfg.ffn, cfg.hidden, 2 * cfg.layers), (cfg.vocab_size, cfg.hidden, 3)):
        key = f"decode 17x{N}x{K} -> tile"
        want[key] = want.get(key, 0) + n
    assert counted == want, counted
    gemm.reset_fallbacks()
