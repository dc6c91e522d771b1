"""Extending the KV cache on the CPU tier (ops/decode.py rope_append_many /
attn_extend torch references, KVCache.extend, Llama.extend, prefill(chunk=),
generate(prefill_chunk=), the payload's --sample-prefill-chunk): T tokens per
row appended to a cache give what the existing full forward gives at those
positions.

The yardstick is ``model(tokens)``; the fp32 tolerance is the one of
tests/test_decode.py's teacher-forcing test, 3 x the deviation of the fp32 full
forward from the same model in fp64 (decode_numerics.forward64), per row
relative to the row's norm, computed here from the model at hand."""
import functools

import pytest
import torch

from decode_numerics import fixture, model as _model, row_dev as _row_dev
from tf_operator_amd.ops import decode as dec
from tf_operator_amd.ops.llm import rope_tables
from tf_operator_amd.train.generate import generate

TOTAL = 140     # the sequence; chunks of 48 cross 64 and 128
PROMPT = 70     # prefilled by chunks of 1, 7, 64 (one whole chunk and a tail of 6) and 70, then 10 decode steps
STEPS = 10
_fixture = functools.partial(fixture, TOTAL)


@pytest.mark.parametrize("chunk", [1, 7, 64, PROMPT])
def test_chunked_prefill_then_decode_steps_match_the_full_forward(chunk):
    f = _fixture()
    m, tokens, full = f["model"], f["tokens"], f["full"]
    cache = m.new_cache(2, PROMPT + STEPS)
    logits = m.prefill(tokens[:, :PROMPT], cache, chunk=chunk)
    assert cache.host_lengths == [PROMPT] * 2 == cache.lengths.tolist()
    worst = 0.0
    for t in range(PROMPT - 1, PROMPT + STEPS):
        if t >= PROMPT:
            logits = m.decode_step(tokens[:, t], cache)
        assert logits.shape == (2, m.cfg.vocab_size)
        e = _row_dev(logits, full[:, t], f["ref"][:, t])
        worst = max(worst, e)
        assert e <= f["tol"], f"chunk {chunk}, position {t}: off by {e:.3e} of the row's norm, limit {f['tol']:.3e}"
    print(f"prefill(chunk={chunk}) + decode vs full forward: {worst:.3e} (limit {f['tol']:.3e})")


def test_extend_all_logits_in_chunks_of_48_match_the_full_forward():
    f = _fixture()
    m, tokens, full = f["model"], f["tokens"], f["full"]
    cache = m.new_cache(2, TOTAL)
    worst = 0.0
    for c0 in range(0, TOTAL, 48):
        lg = m.extend(tokens[:, c0:c0 + 48], cache, logits="all")
        n = lg.shape[1]
        assert lg.shape == (2, min(48, TOTAL - c0), m.cfg.vocab_size)
        for t in range(n):
            e = _row_dev(lg[:, t], full[:, c0 + t], f["ref"][:, c0 + t])
            worst = max(worst, e)
            assert e <= f["tol"], f"position {c0 + t}: off by {e:.3e} of the row's norm, limit {f['tol']:.3e}"
    assert cache.host_lengths == [TOTAL] * 2 == cache.lengths.tolist()
    assert cache.positions.tolist() == [TOTAL - 1] * 2
    print(f"extend(all) vs full forward: {worst:.3e} (limit {f['tol']:.3e})")


def test_continuation_after_prefill_and_decode_steps():
    f = _fixture()
    m, tokens, full = f["model"], f["tokens"], f["full"]
    cache = m.new_cache(2, 64)
    m.prefill(tokens[:, :40], cache)
    for t in range(40, 43):
        m.decode_step(tokens[:, t], cache)
    logits = m.extend(tokens[:, 43:63], cache)
    assert cache.host_lengths == [63, 63]
    e = _row_dev(logits, full[:, 62], f["ref"][:, 62])
    print(f"continuation vs full forward: {e:.3e} (limit {f['tol']:.3e})")
    assert e <= f["tol"]


SENTINEL = 7.0


def test_ragged_prompts_by_chunks_each_row_as_if_alone_and_no_pad_is_written():
    """bf16 with the CPU GEMM pinned to ATen's loop nest (no oneDNN), the
    setting of tests/test_decode.py's ragged test and for its reason: its
    sums do not depend on the row count, so 'bit for bit' is a statement
    about this code.  Unlike prefill(chunk=None), which writes the pads' K
    and V, nothing at or beyond a row's length is touched."""
    m = _model(torch.bfloat16)
    lens, P, cap = [5, 70, 129], 129, 136
    prompts = torch.randint(0, m.cfg.vocab_size, (3, P), generator=torch.Generator().manual_seed(7))
    with torch.backends.mkldnn.flags(enabled=False):
        c3 = m.new_cache(3, cap)
        for t in c3.k + c3.v:
            t.fill_(SENTINEL)
        got = m.prefill(prompts, c3, lens, chunk=64)
        assert torch.isfinite(got.float()).all() and c3.host_lengths == lens == c3.lengths.tolist()
        for b, n in enumerate(lens):
            c1 = m.new_cache(1, cap)
            alone = m.prefill(prompts[b:b + 1, :n], c1, chunk=64)
            assert torch.equal(alone[0], got[b]), f"row {b} (length {n}): logits differ from the row alone"
            for i in range(m.cfg.layers):
                assert torch.equal(c1.k[i][0, :, :n], c3.k[i][b, :, :n]), (b, i)
                assert torch.equal(c1.v[i][0, :, :n], c3.v[i][b, :, :n]), (b, i)
                assert bool((c3.k[i][b, :, n:] == SENTINEL).all()) and bool((c3.v[i][b, :, n:] == SENTINEL).all()), (b, i)


def test_greedy_generate_with_a_chunked_prefill_emits_the_same_tokens():
    m = _model(torch.bfloat16)
    prompts = torch.randint(0, m.cfg.vocab_size, (2, 8), generator=torch.Generator().manual_seed(8))
    with torch.backends.mkldnn.flags(enabled=False):
        a, la = generate(m, prompts, 12)
        b, lb = generate(m, prompts, 12, prefill_chunk=3)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_kvcache_extend_advances_per_row_and_refuses_before_anything_changes():
    c = dec.KVCache(1, 3, 2, 16, 64, "cpu", torch.float32)
    start, count = c.extend([4, 0, 9])
    assert start.dtype == count.dtype == torch.int32
    assert start.tolist() == [0, 0, 0] and count.tolist() == [4, 0, 9]
    assert c.host_lengths == [4, 0, 9] == c.lengths.tolist() and c.positions.tolist() == [3, -1, 8]
    start, count = c.extend([1, 2, 7])
    assert start.tolist() == [4, 0, 9] and count.tolist() == [1, 2, 7]
    assert c.host_lengths == [5, 2, 16] == c.lengths.tolist() and c.max_len == 16
    for bad in ([0, 0, 0], [1, -1, 0], [0, 0, 1], [1, 1], [12, 1, 0]):
        with pytest.raises(ValueError):
            c.extend(bad)
        assert c.host_lengths == [5, 2, 16] == c.lengths.tolist() and c.positions.tolist() == [4, 1, 15]


def test_errors_are_value_errors_before_anything_runs():
    f = _fixture()
    m, tokens = f["model"], f["tokens"]
    cache = m.new_cache(2, 16)
    m.prefill(tokens[:, :5], cache)
    snap = [t.clone() for t in cache.k + cache.v]

    def unchanged():
        return cache.host_lengths == [5, 5] == cache.lengths.tolist() and all(
            torch.equal(a, b) for a, b in zip(snap, cache.k + cache.v))

    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="chunk"):
            m.prefill(tokens[:, :5], m.new_cache(2, 16), chunk=bad)
        with pytest.raises(ValueError, match="chunk"):
            generate(m, tokens[:, :5], 4, prefill_chunk=bad)
    with pytest.raises(ValueError, match="logits"):
        m.extend(tokens[:, 5:8], cache, logits="some")
    with pytest.raises(ValueError, match="counts"):
        m.extend(tokens[:, 5:8], cache, counts=[3])
    with pytest.raises(ValueError, match="counts"):
        m.extend(tokens[:, 5:8], cache, counts=[4, 1])          # more than T
    with pytest.raises(ValueError):
        m.extend(tokens[:, 5:8], cache, counts=[0, 0])
    with pytest.raises(ValueError):
        m.extend(tokens[:, 5:8], cache, counts=[-1, 2])
    with pytest.raises(ValueError, match="overflow"):
        m.extend(tokens[:, 5:17], cache)                        # 5 + 12 slots of 16
    for bad in (96, 32, -64, 64.0, True):
        with pytest.raises(ValueError, match="split_keys"):
            m.extend(tokens[:, 5:8], cache, split_keys=bad)
    assert unchanged()

    q = torch.zeros(2, 3, 4, 64)
    kc, vc = torch.zeros(2, 2, 8, 64), torch.zeros(2, 2, 8, 64)
    st, n = torch.zeros(2, dtype=torch.int32), torch.full((2,), 3, dtype=torch.int32)
    assert dec.attn_extend(q, kc, vc, st, n, split_keys=64).shape == (2, 3, 4, 64)
    assert dec.attn_extend(q, kc, vc, st, n, split_keys=0).shape == (2, 3, 4, 64)
    words = dec.extend_ws_floats(2, 3, 4, 64, 8, 64)
    assert words == 2 * 3 * 4 * 1 * 66 and dec.extend_ws_floats(2, 3, 4, 64, 130, 64) == 3 * words
    assert dec.extend_ws_floats(2, 3, 4, 64, 130, 0) == words
    assert dec.attn_extend(q, kc, vc, st, n, split_keys=64, workspace=torch.zeros(words)).shape == (2, 3, 4, 64)
    with pytest.raises(ValueError, match="split_keys"):
        dec.attn_extend(q, kc, vc, st, n, split_keys=96)
    with pytest.raises(ValueError, match="workspace"):
        dec.attn_extend(q, kc, vc, st, n, split_keys=64, workspace=torch.zeros(words - 1))
    with pytest.raises(ValueError, match="workspace"):
        dec.attn_extend(q, kc, vc, st, n, split_keys=64, workspace=torch.zeros(words, dtype=torch.float64))
    with pytest.raises(ValueError, match="head_dim"):
        dec.attn_extend(torch.zeros(2, 3, 4, 32), torch.zeros(2, 2, 8, 32), torch.zeros(2, 2, 8, 32), st, n)
    with pytest.raises(ValueError, match="multiple"):
        dec.attn_extend(torch.zeros(2, 3, 3, 64), kc, vc, st, n)
    with pytest.raises(ValueError, match="count"):
        dec.attn_extend(q, kc, vc, st, n.long())
    with pytest.raises(ValueError, match="start"):
        dec.attn_extend(q, kc, vc, st[:1], n)
    with pytest.raises(ValueError, match="max_len"):
        dec.attn_extend(q, kc, vc, st, n, max_len=9)
    with pytest.raises(ValueError, match="q "):
        dec.attn_extend(q[:, 0], kc, vc, st, n)
    cos, sin = rope_tables(8, 64)
    assert dec.rope_append_many(torch.zeros(2, 3, 8 * 64), cos, sin, st, n, kc, vc, 4, 2, 64).shape == (2, 3, 4, 64)
    with pytest.raises(ValueError, match="qkv"):
        dec.rope_append_many(torch.zeros(2, 8 * 64), cos, sin, st, n, kc, vc, 4, 2, 64)
    with pytest.raises(ValueError, match="multiple"):
        dec.rope_append_many(torch.zeros(2, 3, 7 * 64), cos, sin, st, n, kc, vc, 3, 2, 64)
    with pytest.raises(ValueError, match="count"):
        dec.rope_append_many(torch.zeros(2, 3, 8 * 64), cos, sin, st, n.long(), kc, vc, 4, 2, 64)
    # the default split: the keys are split while the query tiles are too few to fill the device
    assert dec.extend_split(8, 4, 32, 8, 4096) == dec.SPLIT_KEYS_DEFAULT
    assert dec.extend_split(1, 4096, 32, 8, 4096) == 0

    from tf_operator_amd.examples.llama_train import main

    with pytest.raises(SystemExit) as e:
        main(["--sample-every", "2", "--sample-prefill-chunk", "0"])
    assert e.value.code == 2


def test_reference_masks_later_tokens_and_zeroes_absent_ones():
    """The torch references themselves: a token sees keys 0 .. start + t and
    nothing later (NaN there), tokens at or beyond count write nothing and
    get zero rows."""
    g = torch.Generator().manual_seed(3)
    B, T, Hq, Hkv, D, C = 2, 4, 4, 2, 64, 12
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g)
    cos, sin = rope_tables(C, D)
    kc = torch.full((B, Hkv, C, D), SENTINEL)
    vc = torch.full((B, Hkv, C, D), SENTINEL)
    start = torch.tensor([3, 8], dtype=torch.int32)
    count = torch.tensor([2, 4], dtype=torch.int32)
    q = dec.rope_append_many(qkv, cos, sin, start, count, kc, vc, Hq, Hkv, D)
    pos = torch.tensor([0, 0], dtype=torch.int32)
    for b, (s, n) in enumerate(((3, 2), (8, 4))):
        for t in range(T):
            k1, v1 = torch.zeros(B, Hkv, C, D), torch.zeros(B, Hkv, C, D)
            pos[:] = s + t
            q1 = dec.rope_append(qkv[:, t], cos, sin, pos, k1, v1, Hq, Hkv, D)
            if t < n:
                assert torch.equal(q[b, t], q1[b]) and torch.equal(kc[b, :, s + t], k1[b, :, s + t])
                assert torch.equal(vc[b, :, s + t], v1[b, :, s + t])
            else:
                assert not q[b, t].any()
        written = torch.zeros(C, dtype=torch.bool)
        written[s:s + n] = True
        assert bool((kc[b][:, ~written] == SENTINEL).all()) and bool((vc[b][:, ~written] == SENTINEL).all())
    # attention: row 0's slots 0 .. 2 hold the sentinel (finite), everything beyond a token's position is NaN-proof
    kc[0, :, 5:] = float("nan")
    vc[0, :, 5:] = float("nan")
    o = dec.attn_extend(q, kc, vc, start, count, max_len=12)
    assert torch.isfinite(o).all() and not o[0, 2:].any()
    for t in range(2):
        one = dec.attn_decode(q[:1, t], kc[:1], vc[:1], torch.tensor([3 + t + 1], dtype=torch.int32))
        assert torch.equal(o[0, t], one[0])
