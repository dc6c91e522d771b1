"""Extending the KV cache on an MI355X (csrc/hip/extend.hip through
ops/decode.py, Llama.extend / prefill(chunk=)).

rope_append_many bit for bit against the training path's RoPE; attn_extend
row by row against the fp64 reference of tests/attn_numerics.py (T tokens from
position `start` are rows start .. start + T - 1 of causal attention over
S = start + T) with the causal diagonal across the split boundaries inside one
call, NaN beyond what a row may see and in the workspace; the invariance
contract bit for bit (one call = two calls = T calls = the row inside a batch);
chunked prefill and extend(logits="all") against the fp32 reference within
the teacher-forcing bound of tests/test_decode_gpu.py."""
import functools
import math

import pytest
import torch

import attn_numerics as an
import decode_numerics as dn
from attn_numerics import U
from decode_numerics import DEV, lib as _lib, row_rel as _row_rel

pytestmark = pytest.mark.gpu

NAN = float("nan")
INVALID_VALUE = 1   # hipErrorInvalidValue
LAYOUTS = ((2, 2), (4, 1), (4, 2))   # (Hq, Hkv): G = 1, 4, 2
CAP = 320


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ rope_append_many
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", LAYOUTS)
def test_rope_append_many_bits_of_the_training_rope_and_no_other_slot(Hq, Hkv, D):
    from tf_operator_amd.ops import decode as dec
    from tf_operator_amd.ops.llm import rope_qkv, rope_tables

    _lib()
    B, T, C = 3, 5, CAP
    starts, counts = [0, 17, C - 5], [5, 2, 5]
    g = torch.Generator().manual_seed(D + Hq)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(DEV)
    cos, sin = rope_tables(C, D, device=DEV)
    sentinel = torch.tensor(0x1234, dtype=torch.int16)
    kc = torch.full((B, Hkv, C, D), 0x1234, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    vc = kc.clone()
    q = dec.rope_append_many(qkv, cos, sin, _i32(starts), _i32(counts), kc, vc, Hq, Hkv, D)
    # the same rows placed at those positions of a [B, C] block through the training path
    block = torch.zeros(B, C, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16, device=DEV)
    for b, (s, n) in enumerate(zip(starts, counts)):
        block[b, s:s + n] = qkv[b, :n]
    with torch.no_grad():
        qr, kr, vr = rope_qkv(block.view(B * C, -1), cos, sin, B, C, Hq, Hkv, D, 1)
    torch.cuda.synchronize()
    assert q.shape == (B, T, Hq, D)
    for b, (s, n) in enumerate(zip(starts, counts)):
        others = torch.ones(C, dtype=torch.bool)
        for t in range(T):
            p = s + t
            if t >= n:
                assert not _bits(q[b, t]).any(), (b, t)     # a token that is not there: a zero q row
                continue
            others[p] = False
            assert torch.equal(_bits(q[b, t]), _bits(qr[b, :, p])), (b, t)
            assert torch.equal(_bits(kc[b, :, p]), _bits(kr[b, :, p])), (b, t)
            assert torch.equal(_bits(vc[b, :, p]), _bits(vr[b, :, p])), (b, t)
            assert torch.equal(_bits(vc[b, :, p]), _bits(qkv[b, t].view(Hq + 2 * Hkv, D)[Hq + Hkv:])), (b, t)
        for cache in (kc, vc):   # slots start + 2 .. start + 4 of the row with count 2 among them
            assert bool((_bits(cache[b])[:, others] == sentinel).all()), b


# ------------------------------------------------------------------ attn_extend against fp64
@functools.lru_cache(maxsize=None)
def _case(H, Hk, start, T, D, spike):
    """Causal attention over S = start + T and what its last T rows must be:
    (q [T, H, D], k, v [Hk, S, D] on the GPU; ref, mag, model rows [H, T, D] fp64)."""
    S = start + T
    q, k, v, do = an.make_inputs(1, H, Hk, S, D, spike)
    scale = 1.0 / math.sqrt(D)
    ref = an.attn_ref64(q, k, v, do, scale)
    model = an.bf16_model(q, k, v, do, scale)
    return (q[0, :, start:].transpose(0, 1).contiguous().to(DEV), k[0].to(DEV), v[0].to(DEV), ref.o[0, :, start:],
            ref.mag_o[0, :, start:], model.o[0, :, start:])


def _caches(B, Hk, D):
    kc = torch.full((B, Hk, CAP, D), NAN, dtype=torch.bfloat16, device=DEV)
    return kc, torch.full_like(kc, NAN)


# T G crosses 16 and 32; (60, 9), (63, 2) and (128, 33) put the causal diagonal across the split boundaries at 64
# and 128 inside one call, so early tokens have empty later splits
SPANS = ((0, 1), (0, 16), (0, 17), (1, 3), (60, 9), (63, 2), (64, 5), (128, 33), (197, 4))
CASES = [(Hq, Hkv, D, st, T, False, 64) for D in (64, 128) for Hq, Hkv in LAYOUTS for st, T in SPANS]
CASES.append((4, 2, 128, 128, 33, True, 64))   # late keys x 6: a late split dominates the merge
CASES += [(4, 2, D, st, T, False, sk) for D in (64, 128) for st, T in ((0, 17), (128, 33)) for sk in (0, None)]


@pytest.mark.parametrize("Hq,Hkv,D,start,T,spike,split", CASES, ids=lambda x: str(x))
def test_attn_extend_rows_against_fp64(Hq, Hkv, D, start, T, spike, split):
    from tf_operator_amd.ops import decode as dec

    _lib()
    S = start + T
    q, k, v, ref, mag, model = _case(Hq, Hkv, start, T, D, spike)
    kc, vc = _caches(1, Hkv, D)
    kc[0, :, :S], vc[0, :, :S] = k, v
    o = dec.attn_extend(q[None], kc, vc, _i32([start]), _i32([T]), split_keys=split, max_len=S)
    torch.cuda.synchronize()
    assert o.shape == (1, T, Hq, D)
    an.check_rows(f"extend start={start} T={T} D={D} {Hq}/{Hkv} split={split}", "o", o[0].transpose(0, 1).cpu(), ref,
                  mag, model, S, D)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", LAYOUTS)
def test_attn_extend_mixed_batch_absent_tokens_and_a_nan_workspace(Hq, Hkv, D):
    """Rows of different start with counts (T, 0, T - 1), the workspace and
    every cache slot at or beyond start + count NaN: everything is finite, the
    count-0 row and the token beyond count are exactly zero, the rest within
    bound."""
    from tf_operator_amd.ops import decode as dec

    _lib()
    T = 9
    starts, counts = (60, 128, 197), (T, 0, T - 1)
    cases = [_case(Hq, Hkv, st, T, D, False) for st in starts]
    kc, vc = _caches(3, Hkv, D)
    for b, (st, n, c) in enumerate(zip(starts, counts, cases)):
        kc[b, :, :st + n], vc[b, :, :st + n] = c[1][:, :st + n], c[2][:, :st + n]
    q = torch.stack([c[0] for c in cases])
    max_len = max(s + n for s, n in zip(starts, counts))
    ws = torch.full((dec.extend_ws_floats(3, T, Hq, D, max_len, 64),), NAN, dtype=torch.float32, device=DEV)
    o = dec.attn_extend(q, kc, vc, _i32(starts), _i32(counts), split_keys=64, max_len=max_len, workspace=ws)
    torch.cuda.synchronize()
    o = o.cpu()
    assert torch.isfinite(o.float()).all()
    assert not _bits(o[1]).any() and not _bits(o[2, T - 1]).any()
    for b, n in ((0, T), (2, T - 1)):
        _, _, _, ref, mag, model = cases[b]
        an.check_rows(f"extend batch row {b} D={D} {Hq}/{Hkv}", "o", o[b, :n].transpose(0, 1), ref[:, :n], mag[:, :n],
                      model[:, :n], starts[b] + T, D)


# ------------------------------------------------------------------ the invariance contract
@pytest.mark.parametrize("split", [64, 0])
@pytest.mark.parametrize("D", [64, 128])
def test_one_call_two_calls_sixty_calls_and_a_row_in_a_batch_give_the_same_bits(D, split):
    from tf_operator_amd.ops import decode as dec

    _lib()
    Hq, Hkv, start, T = 4, 2, 170, 60      # keys 0 .. 229: the chunk crosses 192
    q, k, v, _, _, _ = _case(Hq, Hkv, start, T, D, False)
    kc, vc = _caches(1, Hkv, D)
    kc[0, :, :start + T], vc[0, :, :start + T] = k, v
    q = q[None]

    def run(t0, t1, max_len=None):
        return dec.attn_extend(q[:, t0:t1].contiguous(), kc, vc, _i32([start + t0]), _i32([t1 - t0]), split_keys=split,
                               max_len=start + t1 if max_len is None else max_len)

    one = _bits(run(0, T))
    for t1 in (1, 7, 22):
        two = torch.cat([_bits(run(0, t1)), _bits(run(t1, T))], 1)
        assert torch.equal(one, two), f"calls of ({t1}, {T - t1}) tokens differ from one call of {T}"
    each = torch.cat([_bits(run(t, t + 1)) for t in range(T)], 1)
    assert torch.equal(one, each), "60 calls of one token differ from one call of 60"
    # the same row between two others with other starts, a larger max_len
    g = torch.Generator().manual_seed(D)
    k3, v3 = _caches(3, Hkv, D)
    k3[1], v3[1] = kc[0], vc[0]
    for b, st in ((0, 5), (2, 250)):
        k3[b, :, :st + T] = torch.randn(Hkv, st + T, D, generator=g).to(torch.bfloat16).to(DEV)
        v3[b, :, :st + T] = torch.randn(Hkv, st + T, D, generator=g).to(torch.bfloat16).to(DEV)
    q3 = torch.randn(3, T, Hq, D, generator=g).to(torch.bfloat16).to(DEV)
    q3[1] = q[0]
    o3 = dec.attn_extend(q3, k3, v3, _i32([5, start, 250]), _i32([T, T, T]), split_keys=split, max_len=250 + T)
    torch.cuda.synchronize()
    assert torch.isfinite(o3.float()).all()
    assert torch.equal(one[0], _bits(o3[1])), "the row inside a batch of three differs from the row alone"


def test_launchers_refuse_bad_shapes_and_launch_nothing():
    L = _lib()
    P, st = L.ptr, L.stream()
    q = torch.full((2, 3, 4, 64), NAN, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    o = torch.full_like(q, NAN)
    s0 = torch.zeros(2, dtype=torch.int32, device=DEV)
    n = torch.full((2,), 3, dtype=torch.int32, device=DEV)
    ws = torch.zeros(8192, dtype=torch.float32, device=DEV)
    # (B, T, Hq, Hkv, C, D, max_len, split_keys); the last three: grid dimensions past 65535
    for a in ((2, 3, 4, 2, 64, 96, 64, 64), (2, 3, 3, 2, 64, 64, 64, 64), (2, 3, 4, 2, 64, 64, 64, 48),
              (2, 3, 4, 2, 64, 64, 64, 32), (2, 3, 4, 2, 64, 64, 64, 96), (2, 0, 4, 2, 64, 64, 64, 64),
              (2, -1, 4, 2, 64, 64, 64, 0), (2, 3, 4, 2, 64, 64, 65, 64), (2, 3, 4, 2, 64, 64, 0, 64),
              (2, 3, 4, 0, 64, 64, 64, 64), (65536, 3, 4, 2, 64, 64, 64, 64), (2, 2_100_000, 4, 2, 64, 64, 64, 64),
              (2, 3, 4, 2, 1 << 23, 64, 1 << 23, 64)):
        assert L.call_ret("toa_attn_extend", P(q), P(kc), P(vc), P(s0), P(n), P(ws), P(o), *a, 0.125, st) \
            == INVALID_VALUE, a
    cos = torch.ones(64, 32, dtype=torch.float32, device=DEV)
    qkv = torch.ones(2, 3, 8 * 64, dtype=torch.bfloat16, device=DEV)
    # (B, T, Hq, Hkv, D, C, table rows)
    for a in ((2, 3, 4, 2, 96, 64, 64), (2, 3, 3, 2, 64, 64, 64), (2, 3, 4, 0, 64, 64, 64), (2, 0, 4, 2, 64, 64, 64),
              (0, 3, 4, 2, 64, 64, 64)):
        assert L.call_ret("toa_extend_rope_append", P(qkv), P(cos), P(cos), P(s0), P(n), P(q), P(kc), P(vc), *a, st) \
            == INVALID_VALUE, a
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all() and torch.isnan(q.float()).all()
    assert not kc.any() and not vc.any() and not ws.any()


# ------------------------------------------------------------------ the model
PROMPT, TOTAL = 70, 140   # chunks of 7 and 64 (a tail of 6), then decode steps across 128


def _teacher(preset):
    return dn.teacher(preset, TOTAL)


def _check_teacher(what, got, ref, full, first, D):
    dn.check_teacher(what, got, ref, full, first, D, TOTAL)


@pytest.mark.parametrize("chunk,gemm", [(7, "tile"), (64, "tile"), (7, "skinny")])
@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_chunked_prefill_then_decode_steps_within_the_teacher_forcing_bound(preset, chunk, gemm):
    """skinny at B = 2, chunk 7: 14 rows, inside the skinny GEMM's window."""
    m, _, tokens, ref, full = _teacher(preset)
    toks = tokens.to(DEV)
    with torch.no_grad():
        cache = m.new_cache(2, TOTAL)
        got = [m.prefill(toks[:, :PROMPT], cache, chunk=chunk, gemm=gemm)]
        for t in range(PROMPT, TOTAL):
            got.append(m.decode_step(toks[:, t], cache, split_keys=64, gemm=gemm))
    got = torch.stack(got, 1).double().cpu()
    assert cache.host_lengths == [TOTAL] * 2 == cache.lengths.tolist()
    _check_teacher(f"{preset} prefill(chunk={chunk}, {gemm}) + decode", got, ref, full, PROMPT - 1, m.cfg.head_dim)


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_extend_all_logits_in_chunks_of_48_within_the_teacher_forcing_bound(preset):
    m, _, tokens, ref, full = _teacher(preset)
    toks = tokens.to(DEV)
    with torch.no_grad():
        cache = m.new_cache(2, TOTAL)
        got = [m.extend(toks[:, c0:c0 + 48], cache, split_keys=64, logits="all", gemm="tile")
               for c0 in range(0, TOTAL, 48)]
    got = torch.cat(got, 1).double().cpu()
    assert got.shape[:2] == (2, TOTAL)
    _check_teacher(f"{preset} extend(all, 48)", got, ref, full, 0, m.cfg.head_dim)


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_ragged_prompts_by_chunks_write_no_pad_and_stay_within_bound(preset):
    m, ref_m, _, _, _ = _teacher(preset)
    lens, P = [5, 70, 129], 129
    prompts = torch.randint(0, m.cfg.vocab_size, (3, P), generator=torch.Generator().manual_seed(7))
    sentinel = torch.tensor(0x1234, dtype=torch.int16)
    with torch.no_grad():
        ref = ref_m(prompts).double()
        full = m(prompts.to(DEV)).double().cpu()
        cache = m.new_cache(3, CAP)
        for t in cache.k + cache.v:
            t.view(torch.int16).fill_(0x1234)
        got = m.prefill(prompts.to(DEV), cache, lens, chunk=64).double().cpu()
    assert cache.host_lengths == lens == cache.lengths.tolist()
    for b, n in enumerate(lens):
        for t in cache.k + cache.v:
            assert bool((_bits(t[b, :, n:]) == sentinel).all()), (b, n)
            assert bool((_bits(t[b, :, :n]) != sentinel).any()), (b, n)
        r, f = ref[b, n - 1], full[b, n - 1]
        e_full, e = float(_row_rel(f, r)), float(_row_rel(got[b], r))
        limit = 3.0 * e_full + an.fp32_floor(P, m.cfg.head_dim)
        print(f"{preset} ragged row {b} (length {n}): {e / U:.3f} u, full forward {e_full / U:.3f} u, "
              f"worst / limit {e / limit:.3f}")
        assert e <= limit, (b, n, e, e_full)
