"""Shared-prompt decoding on an MI355X (csrc/hip/decode_shared.hip through
ops/decode.py and Llama.decode_step on a SharedKVCache).

rope_append_shared bit for bit against rope_append at the same absolute
position; attn_decode_shared row by row against the fp64 reference of
tests/attn_numerics.py (a row with a prefix of P and a suffix of s keys is row
P + s - 1 of causal attention over the concatenation), NaN beyond every length
and in the workspace; the invariance contract bit for bit; the launchers'
refusals; the model within the teacher-forcing bound of the plain decode tests."""
import functools
import itertools
import math

import pytest
import torch

import attn_numerics as an
import decode_numerics as dn
from decode_numerics import DEV, lib as _lib
from test_extend_gpu import INVALID_VALUE, LAYOUTS, NAN, _bits, _i32

pytestmark = pytest.mark.gpu

CP, CS = 200, 80   # capacities of the prefix and the suffix caches


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ------------------------------------------------------------------ rope_append_shared
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", LAYOUTS)
def test_rope_append_shared_bits_of_rope_append_and_no_other_slot(Hq, Hkv, D):
    from tf_operator_amd.ops import decode as dec
    from tf_operator_amd.ops.llm import rope_tables

    _lib()
    n, base, pos = 3, [5, 140], [0, 3, CS - 1, 1, 0, CS]   # the last row's slot is outside the cache
    B = len(pos)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=torch.Generator().manual_seed(D + Hq)).to(torch.bfloat16).to(DEV)
    cos, sin = rope_tables(CP + CS, D, device=DEV)
    kc, vc, prefix = _nan(B, Hkv, CS, D), _nan(B, Hkv, CS, D), _nan(2, Hkv, CP, D)
    q = dec.rope_append_shared(qkv, cos, sin, _i32(base), _i32(pos), kc, vc, n, Hq, Hkv, D)
    absolute = [base[b // n] + s for b, s in enumerate(pos)]
    pk, pv = _nan(B, Hkv, CP + CS, D), _nan(B, Hkv, CP + CS, D)
    qr = dec.rope_append(qkv[:-1], cos, sin, _i32(absolute[:-1]), pk[:-1], pv[:-1], Hq, Hkv, D)
    torch.cuda.synchronize()
    assert torch.equal(_bits(q[:-1]), _bits(qr)) and not _bits(q[-1]).any()
    written = torch.zeros(B, CS, dtype=torch.bool)
    for b in range(B - 1):
        written[b, pos[b]] = True
        assert torch.equal(_bits(kc[b, :, pos[b]]), _bits(pk[b, :, absolute[b]])), b
        assert torch.equal(_bits(vc[b, :, pos[b]]), _bits(pv[b, :, absolute[b]])), b
    for cache in (kc, vc):
        nan = torch.isnan(cache.float()).all(-1).all(1).cpu()   # [B, CS]: the slot is as it was
        assert torch.equal(nan, ~written)
    assert torch.isnan(prefix.float()).all()


# ------------------------------------------------------------------ attn_decode_shared against fp64
@functools.lru_cache(maxsize=None)
def _group(Hq, Hkv, D, plen, slens, spike=False):
    """One prompt of plen keys and a sample per entry of slens with that many
    keys of its own: q [n, Hq, D], the prompt's k, v [Hkv, plen, D], the
    samples' k, v [n, Hkv, max slen, D] on the GPU, and what each row must be:
    ref, mag, model [n, Hq, D] fp64, S."""
    n, S = len(slens), plen + max(max(slens), 1)
    q, k, v, do = an.make_inputs(n, Hq, Hkv, S, D, spike)
    k[:, :, :plen], v[:, :, :plen] = k[:1, :, :plen].clone(), v[:1, :, :plen].clone()
    scale = 1.0 / math.sqrt(D)
    ref, model = an.attn_ref64(q, k, v, do, scale), an.bf16_model(q, k, v, do, scale)
    rows, last = torch.arange(n), torch.tensor([plen + s - 1 for s in slens])
    return ([q[rows, :, last].to(DEV)] + [t.contiguous().to(DEV) for t in (k[0, :, :plen], v[0, :, :plen], k[:, :, plen:],
                                                                         v[:, :, plen:])]
            + [t[rows, :, last] for t in (ref.o, ref.mag_o, model.o)] + [S])


def _attend(groups, plens, slens, split, rows=None):
    """attn_decode_shared on these _group()s (all of one sample count), every
    slot beyond a length and the workspace NaN; rows: only these rows, each
    as a group of its own."""
    from tf_operator_amd.ops import decode as dec

    n = len(slens) // len(groups)
    Hkv, D = groups[0][1].shape[0], groups[0][1].shape[2]
    pk, pv, sk, sv = _nan(len(groups), Hkv, CP, D), _nan(len(groups), Hkv, CP, D), _nan(len(slens), Hkv, CS, D), \
        _nan(len(slens), Hkv, CS, D)
    for g, (grp, p) in enumerate(zip(groups, plens)):
        pk[g, :, :p], pv[g, :, :p] = grp[1], grp[2]
        for j in range(n):
            s = slens[g * n + j]
            sk[g * n + j, :, :s], sv[g * n + j, :, :s] = grp[3][j, :, :s], grp[4][j, :, :s]
    q = torch.cat([grp[0] for grp in groups])

    def call(q, pk, pv, plens, sk, sv, slens, n):
        ws = _nan(dec.shared_ws_floats(q.shape[0], q.shape[1], D, max(plens), max(max(slens), 1), split or 256),
                  dtype=torch.float32)
        return dec.attn_decode_shared(q, pk, pv, _i32(plens), sk, sv, _i32(slens), n, split_keys=split,
                                      max_prefix_len=max(plens), max_len=max(max(slens), 1), workspace=ws)

    if rows is None:
        return call(q, pk, pv, plens, sk, sv, slens, n)
    return torch.cat([call(q[b:b + 1], pk[b // n:b // n + 1], pv[b // n:b // n + 1], plens[b // n:b // n + 1],
                           sk[b:b + 1], sv[b:b + 1], slens[b:b + 1], 1) for b in rows])


def _check(what, o, groups):
    torch.cuda.synchronize()
    ref, mag, model = (torch.cat([grp[i] for grp in groups]) for i in (5, 6, 7))
    an.check_rows(what, "o", o.cpu(), ref, mag, model, max(grp[8] for grp in groups), groups[0][1].shape[2])


HEADS = ((2, 2), (4, 1), (4, 2), (8, 1))   # G = 1, 4, 2, 8
SAMPLES = (1, 3, 5, 17)    # rows n G: under a tile, no multiple of 16, across two tiles, beyond 64 (a second chunk)
PLENS, SLENS = (1, 63, 64, 65, 197), (1, 2, 64, 65)
# every (D, heads, samples) at two of the prefix lengths, the suffix lengths cycling from another start each time
CASES = [(Hq, Hkv, D, n, PLENS[(i + o) % 5], tuple(SLENS[(i + j) % 4] for j in range(n)), False)
         for i, (D, (Hq, Hkv), n) in enumerate(itertools.product((64, 128), HEADS, SAMPLES)) for o in (0, 2)]
CASES.append((4, 2, 128, 5, 197, (65, 1, 2, 64, 65), True))    # late keys x 6: a late split dominates the merge
CASES.append((4, 1, 64, 3, 65, (2, 0, 64), False))             # a row without a suffix


@pytest.mark.parametrize("Hq,Hkv,D,n,plen,slens,spike", CASES, ids=lambda x: str(x).replace(" ", ""))
def test_attn_decode_shared_rows_against_fp64(Hq, Hkv, D, n, plen, slens, spike):
    _lib()
    grp = _group(Hq, Hkv, D, plen, slens, spike)
    o = _attend([grp], [plen], list(slens), 64)
    assert o.shape == (n, Hq, D)
    _check(f"shared {Hq}/{Hkv} D={D} n={n} prefix={plen} suffixes={slens}", o, [grp])


TWO = ((197, (1, 2, 64, 65, 1)), (65, (64, 65, 0, 2, 64)))   # two prompts x 5 samples, one row without a suffix


@pytest.mark.parametrize("split", [64, None])
@pytest.mark.parametrize("D", [64, 128])
def test_two_prompts_in_one_call_and_every_row_alone_give_the_same_bits(D, split):
    """(4, 1): 20 query rows per prompt and KV head, two tiles; alone a row is 4 rows of one tile, under grids
    bounded by its own lengths."""
    _lib()
    groups = [_group(4, 1, D, p, s) for p, s in TWO]
    plens, slens = [p for p, _ in TWO], [x for _, s in TWO for x in s]
    o = _attend(groups, plens, slens, split)
    _check(f"shared two prompts D={D} split={split}", o, groups)
    alone = _attend(groups, plens, slens, split, rows=range(len(slens)))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(alone))


def test_launchers_refuse_bad_shapes_and_launch_nothing():
    L = _lib()
    P, st = L.ptr, L.stream()
    q, o = _nan(6, 4, 64), _nan(6, 4, 64)
    pk, sk = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(6, 2, 64, 64, dtype=torch.bfloat16,
                                                                                      device=DEV)
    n2, n6, ws = _i32([64] * 2), _i32([64] * 6), torch.zeros(8192, dtype=torch.float32, device=DEV)
    # (B, groups, samples, Hq, Hkv, Cp, Cs, D, max_plen, max_slen, split_keys)
    for a in ((6, 2, 3, 4, 2, 64, 64, 96, 64, 64, 64), (6, 2, 3, 3, 2, 64, 64, 64, 64, 64, 64),
              (6, 2, 0, 4, 2, 64, 64, 64, 64, 64, 64), (6, 2, 2, 4, 2, 64, 64, 64, 64, 64, 64),
              (6, 2, 3, 4, 2, 64, 64, 64, 64, 64, 48), (6, 2, 3, 4, 2, 64, 64, 64, 64, 64, 32),
              (6, 2, 3, 4, 2, 64, 64, 64, 64, 64, 96), (0, 0, 3, 4, 2, 64, 64, 64, 64, 64, 64),
              (6, 2, 3, 4, 2, 0, 64, 64, 0, 64, 64), (6, 2, 3, 4, 2, 64, 0, 64, 64, 0, 64),
              (6, 2, 3, 4, 0, 64, 64, 64, 64, 64, 64), (6, 2, 3, 4, 2, 64, 64, 64, 65, 64, 64),
              (-6, 2, -3, 4, 2, 64, 64, 64, 64, 64, 64)):
        assert L.call_ret("toa_attn_decode_shared", P(q), P(pk), P(pk), P(n2), P(sk), P(sk), P(n6), P(ws), P(o), *a,
                          0.125, st) == INVALID_VALUE, a
    cos = torch.ones(128, 32, dtype=torch.float32, device=DEV)
    qkv = torch.ones(6, 8 * 64, dtype=torch.bfloat16, device=DEV)
    # (B, samples, Hq, Hkv, D, C, table rows)
    for a in ((6, 3, 4, 2, 96, 64, 128), (6, 3, 3, 2, 64, 64, 128), (6, 0, 4, 2, 64, 64, 128), (6, 4, 4, 2, 64, 64, 128),
              (6, 3, 4, 2, 64, 0, 128), (6, 3, 4, 2, 64, 64, 0), (0, 3, 4, 2, 64, 64, 128)):
        assert L.call_ret("toa_shared_rope_append", P(qkv), P(cos), P(cos), P(n2), P(n6), P(q), P(sk), P(sk), *a, st) \
            == INVALID_VALUE, a
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all() and torch.isnan(q.float()).all()
    assert not sk.any() and not ws.any()


# ------------------------------------------------------------------ the model
PROMPT, TOTAL = 6, 76   # 70 decode steps: the suffixes cross the split boundary at 64


@functools.lru_cache(maxsize=None)
def _continuations(preset):
    """One prompt with three different continuations [3, TOTAL]; their fp32 reference and bf16 full-forward logits."""
    m, ref_m, tokens, _, _ = dn.teacher(preset, 140)
    seqs = torch.stack([tokens[0, :TOTAL], tokens[1, :TOTAL], tokens[1, -TOTAL:]])
    seqs[:, :PROMPT] = tokens[0, :PROMPT]
    with torch.no_grad():
        return m, seqs, ref_m(seqs).double(), m(seqs.to(DEV)).double().cpu()


@pytest.mark.parametrize("preset,gemm", [("llama-tiny", "tile"), ("llama-tiny128", "tile"), ("llama-tiny", "skinny")])
def test_three_samples_of_one_prompt_within_the_teacher_forcing_bound(preset, gemm):
    m, seqs, ref, full = _continuations(preset)
    toks = seqs.to(DEV)
    with torch.no_grad():
        cache = m.new_shared_cache(1, 3, PROMPT, TOTAL - PROMPT)
        got = [m.prefill(toks[:1, :PROMPT], cache.prefix, gemm=gemm).expand(3, -1)]
        for t in range(PROMPT, TOTAL):
            got.append(m.decode_step(toks[:, t], cache, split_keys=64, gemm=gemm))
    got = torch.stack(got, 1).double().cpu()
    assert cache.prefix.host_lengths == [PROMPT] and cache.suffix.lengths.tolist() == [TOTAL - PROMPT] * 3
    dn.check_teacher(f"{preset} shared x 3 ({gemm})", got, ref, full, PROMPT - 1, m.cfg.head_dim, TOTAL)
