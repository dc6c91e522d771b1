"""Token sampling on the CPU tier (ops/sample.py's references, which CPU
tensors run; train/generate.py's sampler="device"; the payload's --sample-*
flags).

The yardstick of the integer stage is a brute-force sort in Python ints
(`_brute`), written from the prose of the contract, not from pick_reference:
sort by (logit descending, index ascending), cut the prefixes, intersect with
min-p, scan the kept tokens in index order."""
import math
import os
import random
import subprocess
import sys
import json

import pytest
import torch

from tf_operator_amd.models.llama import PRESETS, Llama
from tf_operator_amd.ops import sample as S
from tf_operator_amd.train.generate import generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32
INF, NAN = float("inf"), float("nan")


def _brute(keys, q, k, P, minq, h64):
    """(token, kept indices) from the definitions."""
    V = len(keys)
    order = sorted(range(V), key=lambda i: (-keys[i], i))
    pre = order[:k] if 0 < k < V else order
    if P < ONE:
        zk = sum(q[i] for i in pre)
        t = max(1, -(-(P * zk) // ONE))
        acc, n = 0, 0
        for i in pre:
            acc, n = acc + q[i], n + 1
            if acc >= t:
                break
        pre = pre[:n]
    kept = sorted(i for i in pre if min(q[i], ONE - 1) >= minq)
    z = sum(q[i] for i in kept)
    r = (h64 * z) >> 64
    acc = 0
    for i in kept:
        acc += q[i]
        if acc > r:
            return i, kept
    raise AssertionError("the kept mass does not exceed r")


def _kq(logits, T=1.0):
    x = torch.tensor(logits, dtype=torch.float32)
    return S.order_keys(x).tolist(), S.weights_reference(x, T).tolist()


# ------------------------------------------------------------------ the hash
def test_draw_is_a_pure_function_of_its_arguments_and_its_values_are_pinned():
    assert S._mix32(0) == 0 and S._mix32(1) == 0x514E28B7      # murmur3's fmix32
    pinned = {(0, 0, 0): 0x37DD7702CEBE33FA, (1, 2, 3): 0x38C0E03E02DD554B, (0, 1 << 40, 7): 0x035F571E2DE28DCA,
              (0xFFFFFFFF, -1, 0x7FFFFFFF): 0x4FF2D76ABE5387B2, (5, 0, 1): 0xB582810EAC18B25B,
              (5, 1, 0): 0xFA7EDFE410680E33}
    for args, want in pinned.items():
        assert S.draw_reference(*args) == want, args
        random.seed(1)                      # no hidden state: not the process's generators, not an earlier call
        torch.manual_seed(1)
        assert S.draw_reference(*args) == want
    # every argument counts, and so does each half of the stream id
    base = S.draw_reference(9, 9, 9)
    assert len({base, S.draw_reference(10, 9, 9), S.draw_reference(9, 10, 9), S.draw_reference(9, 9, 10),
                S.draw_reference(9, 9 + (1 << 32), 9)}) == 5


# ------------------------------------------------------- the integer stage
VALUES = (-INF, NAN, -3.0, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, 2.0)     # few values: heavy ties


def test_pick_reference_against_a_brute_force_sort():
    rng = random.Random(0)
    for V in range(1, 41):
        for _ in range(12):
            logits = [rng.choice(VALUES) for _ in range(V)]
            keys, q = _kq(logits, rng.choice((0.3, 1.0, 5.0)))
            if not any(math.isfinite(v) for v in logits):
                continue
            k = rng.choice((0, 1, 2, 5, V - 1, V, V + 3))
            P = rng.choice((ONE, ONE, 1, ONE // 2, int(0.9 * ONE), ONE - 1))
            minq = rng.choice((0, 0, 1, ONE // 20, ONE // 2, ONE - 256))
            for h64 in (0, (1 << 64) - 1, rng.getrandbits(64), rng.getrandbits(64)):
                tok, kept = _brute(keys, q, max(k, 0), P, minq, h64)
                assert S.pick_reference(keys, q, max(k, 0), P, minq, h64) == tok, (logits, k, P, minq, h64)
                assert q[tok] > 0 and math.isfinite(logits[tok])


def _support(keys, q, k, P, minq, draws=400):
    rng = random.Random(1)
    return {S.pick_reference(keys, q, k, P, minq, h) for h in [0, (1 << 64) - 1] + [rng.getrandbits(64)
                                                                                    for _ in range(draws)]}


def test_ties_enter_in_index_order():
    keys, q = _kq([1.5] * 12)
    assert q == [ONE] * 12
    assert _support(keys, q, 5, ONE, 0) == {0, 1, 2, 3, 4}                  # all equal, top_k 5
    keys, q = _kq([0.25] * 10)
    assert _support(keys, q, 0, ONE // 2, 0) == {0, 1, 2, 3, 4}             # ten equal, top_p 0.5
    keys, q = _kq([0.0, 2.0, -0.0, 2.0, 0.0, 2.0])                          # -0 ties with +0
    assert _support(keys, q, 4, ONE, 0) == {0, 1, 3, 5}


def test_filters_off_topk_beyond_v_minp_mode_only_and_non_finite_logits():
    logits = [0.0, -INF, 1.0, NAN, 0.5, -2.0, NAN, 0.75]
    keys, q = _kq(logits)
    assert q[1] == q[3] == q[6] == 0 and q[2] == ONE
    live = {0, 2, 4, 5, 7}
    assert _support(keys, q, 0, ONE, 0) == live                             # every filter off
    assert _support(keys, q, 8, ONE, 0) == live and _support(keys, q, 99, ONE, 0) == live
    assert _support(keys, q, 7, ONE, 0) == live                             # the last of the order weighs 0 anyway
    assert _support(keys, q, 2, ONE, 0) == {2, 7}
    assert _support(keys, q, 0, ONE, ONE - 256) == {2}                      # a min_p that keeps the mode alone
    assert _support(keys, q, 0, 1, 0) == {2}                                # the smallest top_p: t = 1


def test_special_rows_through_sample_tokens():
    pos = torch.arange(4, dtype=torch.int32)
    rows = torch.tensor([[NAN, -INF, -INF, NAN], [-1.0, 3.0, 3.0, NAN], [INF, 0.0, INF, -INF], [0.0, -0.0, -5.0, -0.0]])
    for T in (0.0, 1e-30, 1e-39):       # log2e / 1e-39 is inf in fp32
        tok, w = S.sample_tokens(rows, temperature=T, positions=pos, return_weights=True)
        maxima = ({0}, {1, 2}, {0, 2}, {0, 1, 3})
        assert tok.tolist() == [0, 1, 0, 0] if T == 0.0 else all(t in s for t, s in zip(tok.tolist(), maxima)), T
        assert w[1].tolist() == [0, ONE - 1, ONE - 1, 0] and w[2].tolist() == [ONE - 1, 0, ONE - 1, 0]
    # temperature 0 ignores the filters; a tiny temperature draws among the maxima only
    assert S.sample_tokens(rows, temperature=0.0, top_k=3, top_p=0.5, min_p=0.5, positions=pos).tolist() == [0, 1, 0, 0]
    seen = {tuple(S.sample_tokens(rows, temperature=1e-30, seed=s, positions=pos).tolist()) for s in range(40)}
    assert {t[0] for t in seen} == {0} and {t[1] for t in seen} == {1, 2} and {t[2] for t in seen} == {0, 2}
    assert {t[3] for t in seen} == {0, 1, 3}
    # per-row parameters: a greedy row next to sampled ones
    tok = S.sample_tokens(rows[1:], temperature=torch.tensor([0.0, 1.0, 1.0]), top_k=torch.tensor([0, 1, 0]),
                          positions=pos[:3])
    assert tok[0] == 1 and tok[1] == 0


# ------------------------------------------------------------ distribution
DIST_V, DIST_ROWS, DIST_SEED, DIST_POS = 37, 4096, 20240, 11
DIST_CASES = {"none": {}, "top_k": {"top_k": 8}, "top_p": {"top_p": 0.7}, "min_p": {"min_p": 0.1}}


def dist_logits():
    """37 distinct fp32 logits in a scrambled order, 0.17 apart."""
    return torch.tensor([-0.17 * ((i * 7) % DIST_V) for i in range(DIST_V)], dtype=torch.float32)


def dist_expectation(case):
    """(kept indices, their fp64 probabilities): the kept set from the brute
    force on the reference weights, after checking that no prefix mass is
    within 1e-3 of top_p, so that the set does not hang on a rounding."""
    x = dist_logits()
    keys, q = S.order_keys(x).tolist(), S.weights_reference(x, 1.0).tolist()
    kw = DIST_CASES[case]
    P, minq = S.filter_ints(kw.get("top_p", 1.0), kw.get("min_p", 0.0))
    _, kept = _brute(keys, q, kw.get("top_k", 0), P, minq, 0)
    p64 = torch.softmax(x.double(), 0)
    order = sorted(range(DIST_V), key=lambda i: (-keys[i], i))
    pre = order[:kw["top_k"]] if "top_k" in kw else order
    cum = torch.cumsum(p64[pre] / p64[pre].sum(), 0)
    assert float((cum - kw.get("top_p", 1.0)).abs().min()) >= 1e-3 or "top_p" not in kw
    if "min_p" in kw:
        assert float(((p64 / p64.max()) - kw["min_p"]).abs().min()) >= 1e-3
    pk = p64[kept] / p64[kept].sum()
    return kept, pk


def chi_square_check(tokens, case):
    """The drawn tokens [DIST_ROWS] against the case's expectation: none
    outside the kept set, chi2 <= dof + 5 sqrt(2 dof) with cells of
    expectation < 5 pooled."""
    kept, pk = dist_expectation(case)
    counts = torch.bincount(tokens.cpu(), minlength=DIST_V)
    assert int(counts[kept].sum()) == DIST_ROWS, f"{case}: tokens outside the kept set {kept}: {counts.tolist()}"
    exp = pk * DIST_ROWS
    obs = counts[kept].double()
    small = exp < 5
    cells = [(float(o), float(e)) for o, e in zip(obs[~small], exp[~small])]
    if bool(small.any()):
        cells.append((float(obs[small].sum()), float(exp[small].sum())))
    chi2 = sum((o - e) ** 2 / e for o, e in cells)
    dof = len(cells) - 1
    limit = dof + 5.0 * math.sqrt(2.0 * dof) if dof else 0.0
    print(f"{case}: kept {len(kept)} tokens, {len(cells)} cells, chi2 {chi2:.2f} vs limit {limit:.2f}")
    assert chi2 <= limit, (case, chi2, limit)


@pytest.mark.parametrize("case", list(DIST_CASES))
def test_distribution_of_4096_streams_at_one_position(case):
    logits = dist_logits().expand(DIST_ROWS, DIST_V)
    tok = S.sample_tokens(logits, temperature=1.0, seed=DIST_SEED, positions=DIST_POS, **DIST_CASES[case])
    chi_square_check(tok, case)


# ---------------------------------------------------------------- generate
def _model():
    m = Llama(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32)
    m.init_weights(0)
    return m.eval()


def test_generate_with_the_device_sampler():
    m = _model()
    prompts = torch.randint(0, m.cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(2))
    kw = dict(temperature=0.9, top_k=20, top_p=0.95, min_p=0.01, sampler="device")
    state = torch.get_rng_state()
    a, _ = generate(m, prompts, 10, seed=3, **kw)
    b, _ = generate(m, prompts, 10, seed=3, **kw)
    c, _ = generate(m, prompts, 10, seed=4, **kw)
    assert torch.equal(torch.get_rng_state(), state)            # the process's generator was neither read nor advanced
    assert torch.equal(a, b) and not torch.equal(a, c)
    greedy, _ = generate(m, prompts, 10)
    k1, _ = generate(m, prompts, 10, temperature=0.7, top_k=1, seed=9, sampler="device")
    t0, _ = generate(m, prompts, 10, temperature=0.0, top_p=0.5, sampler="device")
    assert torch.equal(k1, greedy) and torch.equal(t0, greedy)
    # per-row temperatures: row 0 greedy, row 1 sampled
    mixed, _ = generate(m, prompts, 10, temperature=torch.tensor([0.0, 0.8]), seed=3, sampler="device")
    assert torch.equal(mixed[0], greedy[0]) and not torch.equal(mixed[1], greedy[1])
    # a row alone, and as row 2 of a batch of 3 under the same stream id
    alone, _ = generate(m, prompts[1:], 10, seed=3, stream_ids=torch.tensor([7]), **kw)
    other = torch.randint(0, m.cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(6))
    batch, _ = generate(m, torch.cat([other, prompts[1:]]), 10, seed=3, stream_ids=torch.tensor([0, 1, 7]), **kw)
    assert torch.equal(batch[2], alone[0])
    moved, _ = generate(m, prompts[1:], 10, seed=3, stream_ids=torch.tensor([8]), **kw)
    assert not torch.equal(moved, alone)


def test_generate_refuses_what_the_torch_sampler_cannot_do(monkeypatch):
    m = _model()
    prompts = torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match='sampler="device"'):
        generate(m, prompts, 2, temperature=0.8, top_p=0.9, sampler="torch")
    with pytest.raises(ValueError, match='sampler="device"'):
        generate(m, prompts, 2, temperature=0.8, min_p=0.1)
    with pytest.raises(ValueError, match='sampler="device"'):
        generate(m, prompts, 2, temperature=torch.tensor([0.8]))
    with pytest.raises(ValueError, match="sampler"):
        generate(m, prompts, 2, sampler="cpu")
    monkeypatch.setenv("TOA_SAMPLER", "gpu")
    with pytest.raises(ValueError, match="TOA_SAMPLER"):
        generate(m, prompts, 2)
    monkeypatch.setenv("TOA_SAMPLER", "device")
    a, _ = generate(m, prompts, 4, temperature=0.8, top_p=0.9, seed=1)
    monkeypatch.delenv("TOA_SAMPLER")
    b, _ = generate(m, prompts, 4, temperature=0.8, top_p=0.9, seed=1, sampler="device")
    assert torch.equal(a, b)
    for bad in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=1.0),
                dict(min_p=-0.1), dict(temperature=torch.tensor([0.5, 0.5])), dict(seed=-1)):
        with pytest.raises(ValueError):
            generate(m, prompts, 2, sampler="device", **{"temperature": 0.8, **bad})


# ---------------------------------------------------------------- refusals
def test_sample_tokens_refuses_bad_arguments_before_anything_runs():
    x = torch.zeros(2, 5)
    ok = dict(temperature=1.0, positions=0)
    assert S.sample_tokens(x, **ok).shape == (2,)
    for logits in (torch.zeros(5), torch.zeros(0, 5), torch.zeros(2, 0), torch.zeros(1, (1 << 20) + 1),
                   torch.zeros(2, 5, dtype=torch.float16), torch.zeros(2, 5, dtype=torch.float64), [[0.0]]):
        with pytest.raises(ValueError):
            S.sample_tokens(logits, **ok)
    assert S.sample_tokens(torch.zeros(1, 1 << 20, dtype=torch.bfloat16), temperature=0.0, positions=0).tolist() == [0]
    for bad in (dict(temperature=-0.5), dict(temperature=INF), dict(temperature=NAN), dict(temperature="1"),
                dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=NAN),
                dict(min_p=-0.01), dict(min_p=1.0), dict(seed=1 << 32), dict(seed=-1),
                dict(temperature=torch.ones(3)), dict(temperature=torch.ones(2, 1)),
                dict(temperature=torch.tensor([1.0, -1.0])), dict(top_k=torch.tensor([1.0, 2.0])),
                dict(top_k=torch.tensor([1, -2])), dict(top_p=torch.tensor([0.5, 0.0])),
                dict(min_p=torch.tensor([0.5, 1.0])), dict(temperature=torch.tensor([1, 1])),
                dict(stream_ids=torch.zeros(3, dtype=torch.int64)), dict(stream_ids=torch.zeros(2)),
                dict(positions=torch.zeros(3, dtype=torch.int32)), dict(positions=1.5), dict(positions=None)):
        with pytest.raises(ValueError):
            S.sample_tokens(x, **{**ok, **bad})
    with pytest.raises(TypeError):
        S.sample_tokens(x, temperature=1.0)     # positions are required


# ------------------------------------------------------------- the payload
@pytest.mark.parametrize("flags", [("--sample-temperature", "-1"), ("--sample-temperature", "inf"),
                                   ("--sample-top-k", "-2"), ("--sample-top-k", "1.5"), ("--sample-top-p", "0"),
                                   ("--sample-top-p", "1.2"), ("--sample-min-p", "1"), ("--sample-min-p", "-0.1"),
                                   ("--sample-seed", "-1"), ("--sample-seed", str(1 << 32)),
                                   ("--sample-sampler", "cpu"),
                                   ("--sample-top-p", "0.9", "--sample-sampler", "torch"),
                                   ("--sample-min-p", "0.1", "--sample-sampler", "torch")],
                         ids=lambda f: " ".join(f))
def test_payload_refuses_bad_sampling_flags(flags, capsys):
    from tf_operator_amd.examples.llama_train import main

    with pytest.raises(SystemExit) as e:
        main(["--steps", "1", *flags])
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_payload_samples_with_the_device_sampler():
    env = dict(os.environ, TOA_NO_GPU="1", OMP_NUM_THREADS="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TOA_CHECKPOINT_DIR", "TF_CONFIG", "TOA_SAMPLER"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tf_operator_amd.examples.llama_train", "--steps", "2", "--seq-len", "32",
                        "--sample-every", "1", "--sample-tokens", "4", "--sample-temperature", "0.8",
                        "--sample-top-p", "0.9", "--sample-min-p", "0.02", "--sample-seed", "5",
                        "--sample-sampler", "device"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout
    samples = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"sample"')]
    assert [s["sample"]["step"] for s in samples] == [1, 2], r.stdout
    assert all(len(s["sample"]["tokens"]) == 4 and all(0 <= t < 512 for t in s["sample"]["tokens"]) for s in samples)
