"""The 1-to-16-row GEMM on an MI355X (csrc/hip/gemm_skinny.hip through
ops/gemm.py linear_skinny / swiglu_skinny, Llama.decode_step(gemm="skinny")).

Every element against fp64 under the bound of tests/skinny_numerics.py at the
shapes listed there (each path of the kernel, derived from its constants);
NaN around strided operands and a sentinel around the result; batch invariance
and determinism bit for bit; refusals that launch nothing; teacher forcing,
greedy generation and a ZeRO-1 trainer with the weight-read check on, by the
rules and helpers of tests/test_decode_gpu.py."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

import attn_numerics as an
import decode_numerics as dn
import skinny_numerics as sn
import test_decode_gpu as tdg

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INVALID_VALUE = 1   # hipErrorInvalidValue
SENTINEL = 0x1234
BF16 = torch.bfloat16


def _gemm():
    from tf_operator_amd.ops import gemm

    tdg._lib()
    return gemm


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", sn.SHAPES, ids=lambda v: str(v))
def test_every_element_against_fp64(N, K, swiglu):
    gemm = _gemm()
    x, w, ref, bound = sn.reference(N, K, swiglu)
    xd, wd = x.to(DEV), w.to(DEV)
    assert gemm.skinny_takes(xd, wd, swiglu)
    f = gemm.swiglu_skinny if swiglu else gemm.linear_skinny
    for M in sn.MS:
        got = f(xd[:M], wd)
        assert got.shape == (M, N) and got.dtype == BF16
        sn.check(f"{'swiglu' if swiglu else 'plain'} M={M} N={N} K={K}", got.cpu(), ref[:M], bound[:M])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", [(48, 520), sn.CASE_A], ids=lambda v: str(v))
def test_nothing_outside_the_operands_is_touched(N, K, swiglu):
    gemm = _gemm()
    L = tdg._lib()
    x, w, ref, bound = sn.reference(N, K, swiglu)
    rows_w = w.shape[0]
    ldx, ldw, ldy = K + 8, K + 16, N + 8
    for M in (1, 5, 16):
        xb = torch.full((sn.MAX_M, ldx), NAN, dtype=BF16, device=DEV)
        xb[:M, :K] = x[:M].to(DEV)
        wb = torch.full((rows_w + 16, ldw), NAN, dtype=BF16, device=DEV)
        wb[:rows_w, :K] = w.to(DEV)
        yb = torch.full((sn.MAX_M, ldy), SENTINEL, dtype=torch.int16, device=DEV)
        nbytes = L.call_ret("toa_gemm_skinny_swiglu_ws_bytes" if swiglu else "toa_gemm_skinny_ws_bytes", N, K)
        ws = gemm._workspace(torch.device(DEV, torch.cuda.current_device()), nbytes).fill_(NAN) if nbytes else None
        L.call("toa_gemm_skinny_swiglu" if swiglu else "toa_gemm_skinny", L.ptr(xb), ldx, L.ptr(wb), ldw, L.ptr(yb), ldy,
               M, N, K, L.ptr(ws), L.stream(xb))
        torch.cuda.synchronize()
        got = yb.view(BF16)[:M, :N].cpu()
        assert torch.isfinite(got.float()).all()
        sn.check(f"strided {'swiglu' if swiglu else 'plain'} M={M} N={N} K={K}", got, ref[:M], bound[:M])
        yc = yb.cpu()
        assert bool((yc[M:] == SENTINEL).all()), "rows of y from M on were written"
        assert bool((yc[:, N:] == SENTINEL).all()), "columns of y from N on were written"


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", sn.INVARIANCE_SHAPES, ids=lambda v: str(v))
def test_a_row_does_not_depend_on_its_batch(N, K, swiglu):
    gemm = _gemm()
    x, w, _, _ = sn.reference(N, K, swiglu)
    xd, wd = x.to(DEV), w.to(DEV)
    f = gemm.swiglu_skinny if swiglu else gemm.linear_skinny
    full = _bits(f(xd, wd))
    for m in (0, 7, 15):
        alone = _bits(f(xd[m:m + 1], wd))
        assert torch.equal(full[m], alone[0]), f"row {m} alone differs from its row in the M = 16 launch"
        five = torch.stack([xd[(m + 3) % 16], xd[(m + 9) % 16], xd[m], xd[(m + 1) % 16], xd[(m + 5) % 16]])
        assert torch.equal(full[m], _bits(f(five, wd))[2]), f"row {m} in an M = 5 launch differs from the M = 16 launch"


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", sn.INVARIANCE_SHAPES, ids=lambda v: str(v))
def test_two_launches_are_bit_identical_with_another_in_between(N, K, swiglu):
    gemm = _gemm()
    L = tdg._lib()
    x, w, _, _ = sn.reference(N, K, swiglu)
    xd, wd = x.to(DEV), w.to(DEV)
    other_x, other_w = (t.to(DEV) for t in sn.inputs(N, K, swiglu, seed=1))
    f = gemm.swiglu_skinny if swiglu else gemm.linear_skinny
    nbytes = L.call_ret("toa_gemm_skinny_swiglu_ws_bytes" if swiglu else "toa_gemm_skinny_ws_bytes", N, K)
    if nbytes:   # a partial read before it is written would be a NaN
        gemm._workspace(xd.device, nbytes).fill_(NAN)
    first = f(xd, wd)
    between = f(other_x * 3, other_w)
    second = f(xd, wd)
    assert torch.isfinite(first.float()).all() and torch.isfinite(between.float()).all()
    assert not torch.equal(_bits(first), _bits(between))
    assert torch.equal(_bits(first), _bits(second))


def test_refusals_launch_nothing():
    L = tdg._lib()
    P, st = L.ptr, L.stream()
    N, K = 48, 520
    x = torch.ones(16, K, dtype=BF16, device=DEV)
    w = torch.ones(2 * N, K, dtype=BF16, device=DEV)
    y = torch.full((16, N), SENTINEL, dtype=torch.int16, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float32, device=DEV)
    off = lambda t, nbytes: __import__("ctypes").c_void_p(t.data_ptr() + nbytes)   # noqa: E731
    Nd, Kd = sn.CASE_D
    xd = torch.ones(16, Kd, dtype=BF16, device=DEV)
    wdd = torch.ones(2 * Nd, Kd, dtype=BF16, device=DEV)
    # (x, ldx, w, ldw, y, ldy, M, N, K, ws)
    cases = {
        "M = 0": (P(x), K, P(w), K, P(y), N, 0, N, K, P(ws)),
        "M = 17": (P(x), K, P(w), K, P(y), N, 17, N, K, P(ws)),
        "N = 8": (P(x), K, P(w), K, P(y), N, 8, 8, K, P(ws)),
        "K = 12": (P(x), K, P(w), K, P(y), N, 8, N, 12, P(ws)),
        "x off by 2 bytes": (off(x, 2), K, P(w), K, P(y), N, 8, N, K - 8, P(ws)),
        "w off by 2 bytes": (P(x), K, off(w, 2), K, P(y), N, 8, N, K - 8, P(ws)),
        "y off by 2 bytes": (P(x), K, P(w), K, off(y, 2), N, 8, N - 16, K, P(ws)),
        "ldw < K": (P(x), K, P(w), K - 8, P(y), N, 8, N, K, P(ws)),
        "a null workspace where K is split": (P(xd), Kd, P(wdd), Kd, P(y), N, 8, Nd, Kd, None),
    }
    for name in ("toa_gemm_skinny", "toa_gemm_skinny_swiglu"):
        for what, a in cases.items():
            assert L.call_ret(name, *a, st) == INVALID_VALUE, (name, what)
        # the last one is taken with a workspace: the refusal was the workspace's
        assert L.call_ret(name, *cases["a null workspace where K is split"][:-1], P(ws), st) == 0
        torch.cuda.synchronize()
        assert bool((y[8:] == SENTINEL).all()) and bool((y[:8, Nd:] == SENTINEL).all()) and not bool(
            (y[:8, :Nd] == SENTINEL).any())
        y.fill_(SENTINEL)
    for name in ("toa_gemm_skinny", "toa_gemm_skinny_swiglu"):
        for what, a in cases.items():
            assert L.call_ret(name, *a, st) == INVALID_VALUE, (name, what)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and not ws.isnan().any()


# ------------------------------------------------------------------ the model
def _decode_skinny(m, preset):
    tokens = torch.randint(0, m.cfg.vocab_size, (2, tdg.TOTAL), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        cache = m.new_cache(2, tdg.TOTAL)
        dec = [m.prefill(tokens[:, :tdg.PROMPT].to(DEV), cache, gemm="skinny")]
        for t in range(tdg.PROMPT, tdg.TOTAL):
            dec.append(m.decode_step(tokens[:, t].to(DEV), cache, split_keys=64, gemm="skinny"))
    return torch.stack(dec, 1).double().cpu()


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_teacher_forcing_within_three_times_the_full_forwards_error(preset):
    gemm = _gemm()
    m, ref, full, tile = tdg._teacher(preset)      # the same tokens (seed 5), positions and split_keys
    gemm.reset_fallbacks()
    dec = _decode_skinny(m, preset)
    assert not [k for k in gemm.fallbacks() if k.startswith("decode")], gemm.fallbacks()
    e_full, e_dec, e_tile = dn.row_rel(full, ref), dn.row_rel(dec, ref), dn.row_rel(tile, ref)
    floor = an.fp32_floor(tdg.TOTAL, m.cfg.head_dim)
    limit = 3.0 * e_full + floor
    ratio = e_dec / limit
    i = int(ratio.flatten().argmax())
    b, t = i // ratio.shape[1], i % ratio.shape[1]
    print(f"{preset}: worst skinny decode / limit {float(ratio.max()):.3f} at row {b} position {tdg.PROMPT - 1 + t}; "
          f"worst tile decode / limit {float((e_tile / limit).max()):.3f}")
    assert torch.isfinite(dec).all()
    assert bool((e_dec <= limit).all()), (b, tdg.PROMPT - 1 + t, float(e_dec[b, t]), float(e_full[b, t]))


def test_greedy_generate_follows_the_full_forward_argmax():
    """The rule of tests/test_decode_gpu.py's test of the same name, with
    ``gemm="skinny"``: a step is left out when the bf16 full forward's two
    best logits are closer than twice its largest single-logit error; at most
    10 % of the steps (the share belongs to the reference: 7 of 80 at prompt
    seed 8, that test's docstring)."""
    from tf_operator_amd.train.generate import generate

    m, ref, full, _ = tdg._teacher("llama-tiny")
    thr = 2.0 * float((full - ref).abs().max())
    new = 40
    prompts = torch.randint(0, m.cfg.vocab_size, (2, tdg.PROMPT), generator=torch.Generator().manual_seed(8)).to(DEV)
    out, lengths = generate(m, prompts, new, split_keys=64, gemm="skinny")
    assert out.shape == (2, tdg.PROMPT + new) and lengths.tolist() == [tdg.PROMPT + new] * 2
    left_out, wrong = 0, []
    with torch.no_grad():
        for t in range(new):
            lg = m(out[:, :tdg.PROMPT + t])[:, -1].float()
            top = torch.topk(lg, 2, dim=-1).values
            close = (top[:, 0] - top[:, 1]) < thr
            left_out += int(close.sum())
            if not bool((close | (out[:, tdg.PROMPT + t] == lg.argmax(-1))).all()):
                wrong.append(t)
    print(f"gap threshold {thr:.4e}; left out {left_out} of {2 * new} steps; wrong at {wrong}")
    assert not wrong
    assert left_out <= 0.1 * 2 * new


def _zero_worker(port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    try:
        from tf_operator_amd.ops import gemm
        from tf_operator_amd.train.llm import LlamaTrainer

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        tr = LlamaTrainer("llama-tiny", dev, micro_batch=2, seq_len=128, lr=1e-3, bucket_mb=0.25, zero_check=True,
                          force_collectives=True, shard_optimizer=True)
        assert tr.gather is not None and tr.gather.check
        b = tr.synthetic_batch()
        l0 = float(tr.step([b]))
        toks, _ = tr.generate(b[0][:, :8], 6, gemm="skinny")   # right after the step: its gathers are still outstanding
        l1 = float(tr.step([b]))
        tr.gather.wait_all()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        torch.save({"losses": [l0, l1], "tokens": toks.cpu(),
                    "fallbacks": [k for k in gemm.fallbacks() if k.startswith("decode")]}, out)
    except Exception:  # pragma: no cover - reported to the parent
        import traceback

        torch.save({"err": traceback.format_exc()}, out)


@pytest.mark.timeout(300)
def test_generate_right_after_a_zero1_step_passes_the_weight_read_check(tmp_path):
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "zero.pt")
    p = ctx.Process(target=_zero_worker, args=(tdg._port(), out))
    p.start()
    p.join(timeout=280)
    if p.is_alive():
        p.kill()
        pytest.fail("the worker was still running after 280 s")
    res = torch.load(out, weights_only=True)
    assert "err" not in res, res["err"]
    assert res["tokens"].shape == (2, 14) and all(math.isfinite(x) for x in res["losses"])
    assert res["fallbacks"] == [], res["fallbacks"]
