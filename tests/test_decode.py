"""KV-cache decoding on the CPU tier (ops/decode.py's torch references,
Llama.prefill / decode_step, train/generate.py, LlamaTrainer.generate, the
payload's --sample-every): decoding one token at a time gives what the
existing full forward gives for the same position.

The yardstick is ``model(tokens)``, not the code under test.  The teacher-
forcing and greedy tests run in fp32, the widest dtype the CPU fallbacks
compute in (they take fp64 tensors too, but do their arithmetic in fp32);
the tolerance is 3 x the deviation of that fp32 full forward from the same
model evaluated in fp64 by the plain formulas (decode_numerics.forward64)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from decode_numerics import fixture, model as _model, row_dev as _row_dev
from tf_operator_amd.ops import decode as dec
from tf_operator_amd.ops.llm import rope_tables
from tf_operator_amd.train.generate import generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT, TOTAL = 5, 45    # prefill 5 tokens, decode the next 40
# 3 x the fp32 full forward's deviation from fp64, per row relative to the row's norm, is computed from the model
# at hand (decode_numerics.fixture).  Observed on the development machine (llama-tiny, seed 0, 2 x 45 tokens): full
# forward vs fp64 <= 4.7e-7 of a row's norm, so a tolerance of 1.4e-6; decode vs full forward <= 5.6e-7.
_fixture = functools.partial(fixture, TOTAL)


def test_teacher_forcing_matches_the_full_forward():
    f = _fixture()
    m, tokens, full = f["model"], f["tokens"], f["full"]
    cache = m.new_cache(2, TOTAL)
    worst = 0.0
    logits = m.prefill(tokens[:, :PROMPT], cache)
    for t in range(PROMPT - 1, TOTAL):
        if t >= PROMPT:
            logits = m.decode_step(tokens[:, t], cache)
        assert logits.shape == (2, m.cfg.vocab_size)
        e = _row_dev(logits, full[:, t], f["ref"][:, t])
        worst = max(worst, e)
        assert e <= f["tol"], f"position {t}: decode logits off by {e:.3e} of the row's norm, limit {f['tol']:.3e}"
    assert cache.host_lengths == [TOTAL, TOTAL] and cache.lengths.tolist() == [TOTAL, TOTAL]
    assert cache.positions.tolist() == [TOTAL - 1, TOTAL - 1]
    print(f"decode vs full forward: {worst:.3e} (limit {f['tol']:.3e})")


def test_ragged_prompts_each_row_as_if_alone_and_nan_beyond_the_lengths():
    """bf16, the model's own dtype, with the CPU GEMM pinned to ATen's loop
    nest (no oneDNN): its sums do not depend on the row count, so 'bit for
    bit' is a statement about this code (fp32 library GEMMs pick their kernel
    by the row count: 5e-7 apart between a batch of 3 and a batch of 1)."""
    m = _model(torch.bfloat16)
    g = torch.Generator().manual_seed(7)
    P, lens, steps, cap = 7, [1, 3, 7], 4, 16
    prompts = torch.randint(0, m.cfg.vocab_size, (3, P), generator=g)
    nxt = torch.randint(0, m.cfg.vocab_size, (3, steps), generator=g)

    def poison(cache, lengths):
        for t in cache.k + cache.v:
            for b, n in enumerate(lengths):
                t[b, :, n:] = float("nan")

    with torch.backends.mkldnn.flags(enabled=False):
        c3 = m.new_cache(3, cap)
        got = [m.prefill(prompts, c3, lens)]
        poison(c3, lens)
        got += [m.decode_step(nxt[:, t], c3) for t in range(steps)]
        for lg in got:
            assert torch.isfinite(lg.float()).all()
        for b, n in enumerate(lens):
            c1 = m.new_cache(1, cap)
            alone = [m.prefill(prompts[b:b + 1, :n], c1)]
            poison(c1, [n])
            alone += [m.decode_step(nxt[b:b + 1, t], c1) for t in range(steps)]
            for t, (a, bt) in enumerate(zip(alone, got)):
                assert torch.equal(a[0], bt[b]), f"row {b} (length {n}), step {t}: logits differ from the row alone"
            end = n + steps
            for i in range(m.cfg.layers):
                assert torch.equal(c1.k[i][0, :, :end], c3.k[i][b, :, :end]), (b, i)
                assert torch.equal(c1.v[i][0, :, :end], c3.v[i][b, :, :end]), (b, i)
                assert torch.isnan(c3.k[i][b, :, end:].float()).all() and torch.isnan(c3.v[i][b, :, end:].float()).all()
        assert c3.host_lengths == [n + steps for n in lens] == c3.lengths.tolist()


def test_greedy_generate_follows_the_full_forward_argmax():
    """Steps where the full forward's top two logits are closer than the
    teacher-forcing tolerance (of the row's norm) are left out: at most 10 %.
    Observed: 0 of 80 steps left out in fp32 (seed 5 prompts, llama-tiny seed 0)."""
    f = _fixture()
    m = f["model"]
    new = 40
    prompts = f["tokens"][:, :PROMPT]
    out, lengths = generate(m, prompts, new)
    assert out.shape == (2, PROMPT + new) and lengths.tolist() == [PROMPT + new] * 2
    assert torch.equal(out[:, :PROMPT], prompts)
    left_out = 0
    with torch.no_grad():
        for t in range(new):
            ref = m(out[:, :PROMPT + t])[:, -1]
            top = torch.topk(ref, 2, dim=-1).values
            close = (top[:, 0] - top[:, 1]) < f["tol"] * ref.norm(dim=-1)
            left_out += int(close.sum())
            ok = close | (out[:, PROMPT + t] == ref.argmax(-1))
            assert ok.all(), f"step {t}: generate chose {out[:, PROMPT + t].tolist()}, the full forward {ref.argmax(-1).tolist()}"
    print(f"left out: {left_out} of {2 * new} steps")
    assert left_out <= 0.1 * 2 * new


def test_sampling_reproduces_itself_topk1_is_greedy_and_eos_sticks():
    m = _fixture()["model"]
    prompts = _fixture()["tokens"][:, :PROMPT]
    state = torch.get_rng_state()
    a, _ = generate(m, prompts, 12, temperature=0.9, top_k=20, seed=3)
    b, _ = generate(m, prompts, 12, temperature=0.9, top_k=20, seed=3)
    c, _ = generate(m, prompts, 12, temperature=0.9, top_k=20, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(torch.get_rng_state(), state)       # a generator of its own
    greedy, _ = generate(m, prompts, 12)
    k1, _ = generate(m, prompts, 12, temperature=0.7, top_k=1, seed=9)
    assert torch.equal(greedy, k1)
    # top-k: every sampled token is among the k best of the full forward at its position
    with torch.no_grad():
        for t in range(12):
            best = torch.topk(m(a[:, :PROMPT + t])[:, -1], 20, dim=-1).indices
            assert (best == a[:, PROMPT + t, None]).any(-1).all(), t
    # the third greedy token of row 0 as the EOS: from there on the row stays at it, the other row goes on
    eos = int(greedy[0, PROMPT + 2])
    e, _ = generate(m, prompts, 12, eos_id=eos)
    first = int((e[0, PROMPT:] == eos).nonzero()[0])
    assert first <= 2 and torch.equal(e[0, PROMPT:PROMPT + first], greedy[0, PROMPT:PROMPT + first])
    assert (e[0, PROMPT + first:] == eos).all()
    row1 = e[1, PROMPT:]
    hit = (row1 == eos).nonzero()
    stop = int(hit[0]) if len(hit) else 12
    assert torch.equal(row1[:stop], greedy[1, PROMPT:PROMPT + stop]) and (row1[stop:] == eos).all()


def test_errors_are_value_errors_before_anything_runs():
    m = _fixture()["model"]
    tokens = _fixture()["tokens"]
    cache = m.new_cache(2, 6)
    m.prefill(tokens[:, :5], cache)
    m.decode_step(tokens[:, 5], cache)
    snap = [t.clone() for t in cache.k + cache.v]
    with pytest.raises(ValueError, match="overflow"):
        m.decode_step(tokens[:, 6], cache)                       # a seventh slot
    assert cache.host_lengths == [6, 6] and cache.lengths.tolist() == [6, 6]
    assert all(torch.equal(a, b) for a, b in zip(snap, cache.k + cache.v))
    with pytest.raises(ValueError, match="overflow"):
        m.prefill(tokens[:, :7], m.new_cache(2, 6))
    with pytest.raises(ValueError, match="overflow"):
        generate(m, tokens[:, :5], 4, capacity=7)
    for bad in (0, 32, 96, 63, -64, 64.0, True):
        with pytest.raises(ValueError, match="split_keys"):
            m.decode_step(tokens[:, 6], m.new_cache(2, 8), split_keys=bad)
    q = torch.zeros(2, 4, 64)
    kc, vc = torch.zeros(2, 2, 8, 64), torch.zeros(2, 2, 8, 64)
    n = torch.ones(2, dtype=torch.int32)
    assert dec.attn_decode(q, kc, vc, n, split_keys=64).shape == (2, 4, 64)
    with pytest.raises(ValueError, match="split_keys"):
        dec.attn_decode(q, kc, vc, n, split_keys=48)
    with pytest.raises(ValueError, match="head_dim"):
        dec.attn_decode(torch.zeros(2, 4, 32), torch.zeros(2, 2, 8, 32), torch.zeros(2, 2, 8, 32), n)
    with pytest.raises(ValueError, match="multiple"):
        dec.attn_decode(torch.zeros(2, 3, 64), kc, vc, n)
    with pytest.raises(ValueError):
        dec.attn_decode(q, kc, torch.zeros(2, 2, 8, 128), n)     # K and V caches disagree
    with pytest.raises(ValueError, match="lengths"):
        dec.attn_decode(q, kc, vc, n.long())
    with pytest.raises(ValueError, match="max_len"):
        dec.attn_decode(q, kc, vc, n, max_len=9)
    cos, sin = rope_tables(8, 64)
    pos = torch.zeros(2, dtype=torch.int32)
    assert dec.rope_append(torch.zeros(2, 8 * 64), cos, sin, pos, kc, vc, 4, 2, 64).shape == (2, 4, 64)
    with pytest.raises(ValueError, match="multiple"):
        dec.rope_append(torch.zeros(2, 7 * 64), cos, sin, pos, kc, vc, 3, 2, 64)
    with pytest.raises(ValueError, match="head_dim"):
        dec.rope_append(torch.zeros(2, 8 * 32), cos, sin, pos, kc, vc, 4, 2, 32)
    with pytest.raises(ValueError, match="qkv"):
        dec.rope_append(torch.zeros(2, 6 * 64), cos, sin, pos, kc, vc, 4, 2, 64)
    with pytest.raises(ValueError):
        dec.KVCache(2, 2, 2, 8, 96, "cpu")
    with pytest.raises(ValueError, match="KV cache"):
        m.decode_step(tokens[:, 0], dec.KVCache(2, 2, 4, 8, 64, "cpu", torch.float32))   # 4 kv heads, the model has 2
    assert dec.SPLIT_KEYS_DEFAULT >= 64 and dec.SPLIT_KEYS_DEFAULT & (dec.SPLIT_KEYS_DEFAULT - 1) == 0


def test_generate_between_steps_leaves_the_training_run_bit_identical():
    from tf_operator_amd.train.llm import LlamaTrainer

    def run(sample):
        torch.manual_seed(11)
        tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, lr=1e-3)
        batch = tr.synthetic_batch()
        losses, samples = [], []
        for i in range(4):
            losses.append(float(tr.step([batch])))
            if sample and i in (0, 2):   # after steps 1 and 3
                samples.append(tr.generate(batch[0][:, :6], 5, temperature=0.8, top_k=8, seed=i)[0])
        assert tr.step_idx == 4 and tr.model.training
        return (losses, tr.flat.master.clone(), tr.flat.exp_avg.clone(), tr.flat.exp_avg_sq.clone(), tr.flat.param.clone(),
                tr.flat.grad.clone(), torch.get_rng_state(), samples)

    a, b = run(False), run(True)
    assert len(b[-1]) == 2 and all(s.shape == (2, 11) for s in b[-1])
    assert a[0] == b[0], (a[0], b[0])
    for x, y, name in zip(a[1:7], b[1:7], ("master", "exp_avg", "exp_avg_sq", "param", "grad", "rng")):
        assert torch.equal(x, y), name


def _payload(*args):
    env = dict(os.environ, TOA_NO_GPU="1", OMP_NUM_THREADS="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TOA_CHECKPOINT_DIR", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tf_operator_amd.examples.llama_train", "--steps", "4", "--seq-len", "32",
                        *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"sample"')], r.stdout


def test_payload_prints_sample_lines_only_when_asked():
    samples, out = _payload("--sample-every", "2", "--sample-tokens", "4")
    assert [s["sample"]["step"] for s in samples] == [2, 4], out
    for s in samples:
        toks = s["sample"]["tokens"]
        assert set(s) == {"sample"} and set(s["sample"]) == {"step", "tokens"}
        assert len(toks) == 4 and all(isinstance(t, int) and 0 <= t < 512 for t in toks), toks
    samples, out = _payload()
    assert samples == [] and "sample" not in out, out
