"""toa_sample_tokens on the GPU (csrc/hip/sample.hip) in two stages, as the
kernel's optional `weights` output allows:

* the float stage: each token's integer weight q against 2^32 * exp2 in fp64,
  within a per-element bound derived below;
* the integer stage, bit for bit: ops.sample.pick_reference, fed the kernel's
  own weights and the logits' order keys, must name the kernel's token.

Then invariance (a row's token depends on that row's logits, parameters,
seed, stream id and position only), the distribution, the launcher's
refusals and generate(sampler="device") on the tiny model."""
import itertools
import math

import pytest
import torch

from test_sample import DIST_CASES, DIST_POS, DIST_ROWS, DIST_SEED, DIST_V, chi_square_check, dist_logits
from tf_operator_amd.ops import sample as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
INVALID_VALUE = 1   # hipErrorInvalidValue
ONE = 1 << 32
INF, NAN = float("inf"), float("nan")
# 2053 = two sweeps of the 1024-thread workgroup and a tail of 5; each wave's segment is 129 tokens: two full
# 64-wide steps and a third of one lane
VS = (1, 7, 257, 4099, 2 * 1024 + 5)
DTYPES = (torch.bfloat16, torch.float32)

# The float stage's bound.  The kernel computes arg = fl(fl(x - m) * fl(fl(log2e) / T)): four roundings of at most
# 2^-24 relative each (the subtraction, the constant, the division, the product), so |arg - exact| <= ROUNDINGS *
# 2^-24 * |arg| to first order, which moves 2^arg by a relative ln2 times that.  v_exp_f32 is documented to 1 ulp,
# at most 2^-23 of its result.  The scaling by 2^32 is exact; rint and the comparison's own fp64 value add 1.
ROUNDINGS = 4.0
EXP2_ULP = 2.0 ** -23


def _lib():
    from tf_operator_amd.ops import _lib as L

    assert L.available(), L.load_error()
    return L


def _logits(B, V, dtype, seed, scale=3.0):
    """Random rows, rounded to bf16 first (ties, and the same values in
    either dtype); row 1 ends in -inf, row 2 holds NaNs, row 3 +inf."""
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()
    if B > 1:
        x[1, V // 2 + 1:] = -INF
    if B > 2:
        x[2, ::3] = NAN
    if B > 3:
        x[3, V // 3] = INF
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", VS)
def test_weights_against_fp64(V, dtype):
    worst = 0.0
    for T in (0.3, 1.0, 5.0):
        x = _logits(5, V, dtype, seed=V)
        _, w = S.sample_tokens(x.to(DEV), temperature=T, positions=0, return_weights=True)
        w = w.cpu().double()
        x64 = S._canonical(x).double()
        m = x64.max(-1, keepdim=True).values
        T32 = float(torch.tensor(T, dtype=torch.float32))
        arg = torch.where(x64 == m, torch.zeros_like(x64), (x64 - m) * (math.log2(math.e) / T32))
        arg = torch.where(torch.isnan(arg), torch.full_like(arg, -INF), arg)        # -inf - -inf: weight 0
        exact = torch.clamp(torch.exp2(arg) * ONE, max=ONE - 1)
        bound = exact * (ROUNDINGS * 2.0 ** -24 * math.log(2.0) * arg.abs().clamp(max=200.0) + EXP2_ULP) + 1.0
        bound = torch.where(x64 == m, torch.zeros_like(bound), bound)               # the maximum: 2^32 - 1 exactly
        bound = torch.where(x64 == -INF, torch.zeros_like(bound), bound)            # -inf and NaN: 0 exactly
        err = (w - exact).abs()
        ratio = float((err / bound.clamp(min=1.0)).max())
        worst = max(worst, ratio)
        bad = (err > bound).nonzero()
        assert bad.numel() == 0, (T, bad[0].tolist(), float(err[tuple(bad[0])]), float(bound[tuple(bad[0])]))
    print(f"V {V} {dtype}: worst |q - exact| / bound {worst:.3f}")


def _expected(x, w, T, k, p, mp, seed, sid, pos):
    """pick_reference per row on the kernel's weights w [B, V] (int64, CPU)."""
    out = []
    for b in range(x.shape[0]):
        keys = S.order_keys(x[b])
        if not bool(torch.isfinite(S._canonical(x[b])).any()):
            out.append(0)
        elif not T[b] > 0.0:
            out.append(int((keys == keys.max()).nonzero()[0]))
        else:
            q = torch.where(keys == keys.max(), torch.full_like(w[b], ONE), w[b])
            P, minq = S.filter_ints(p[b], mp[b])
            out.append(S.pick_reference(keys.tolist(), q.tolist(), k[b], P, minq,
                                        S.draw_reference(seed, sid[b], pos[b])))
    return out


def _cycle(values, n, skip=0):
    return list(itertools.islice(itertools.cycle(values), skip, skip + n))


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", VS)
def test_tokens_bit_for_bit_against_pick_reference(V, dtype):
    B, seed = 64, 77
    x = _logits(B, V, dtype, seed=100 + V)
    x[5] = NAN                                                   # no finite logit: token 0
    x[7] = x[7, 0]                                               # one value: every token ties
    T = _cycle((0.3, 1.0, 5.0, 0.8, 1e-30), B)
    T[6] = 0.0                                                   # a greedy row
    k = _cycle((0, 1, 5, max(V // 2, 1), V, V + 7, 50), B)
    p = _cycle((1.0, 0.9, 0.5, 0.05, 1.0, 0.999), B, 1)
    mp = _cycle((0.0, 0.05, 0.5, 0.0), B, 2)
    sid = [(1 << 33) * b + 3 * b for b in range(B)]
    pos = [1000 - b for b in range(B)]
    tok, w = S.sample_tokens(x.to(DEV), temperature=torch.tensor(T), top_k=torch.tensor(k), top_p=torch.tensor(p),
                             min_p=torch.tensor(mp), seed=seed, stream_ids=torch.tensor(sid),
                             positions=torch.tensor(pos, dtype=torch.int32), return_weights=True)
    T32, p32, mp32 = (torch.tensor(v, dtype=torch.float32).tolist() for v in (T, p, mp))
    want = _expected(x, w.cpu(), T32, k, p32, mp32, seed, sid, pos)
    assert tok.tolist() == want
    assert tok[5] == 0 and tok[6] == int(S.order_keys(x[6]).argmax())
    # the weights output changes nothing
    again = S.sample_tokens(x.to(DEV), temperature=torch.tensor(T), top_k=torch.tensor(k), top_p=torch.tensor(p),
                            min_p=torch.tensor(mp), seed=seed, stream_ids=torch.tensor(sid),
                            positions=torch.tensor(pos, dtype=torch.int32))
    assert torch.equal(again, tok)


def test_real_vocabulary_bit_for_bit():
    B, V, seed = 8, 128256, 9
    x = _logits(B, V, torch.bfloat16, seed=4, scale=2.5)
    xd = x.to(DEV)
    for kw in (dict(top_k=50), dict(top_p=0.9), dict(min_p=0.05)):
        pos = list(range(40, 40 + B))
        tok, w = S.sample_tokens(xd, temperature=0.8, seed=seed, positions=torch.tensor(pos, dtype=torch.int32),
                                 return_weights=True, **kw)
        T32, p32, mp32 = (float(torch.tensor(v, dtype=torch.float32)) for v in
                          (0.8, kw.get("top_p", 1.0), kw.get("min_p", 0.0)))
        want = _expected(x, w.cpu(), [T32] * B, [kw.get("top_k", 0)] * B, [p32] * B, [mp32] * B, seed, list(range(B)),
                         pos)
        assert tok.tolist() == want, kw


def test_a_rows_token_depends_on_that_row_only():
    V, n = 4099, 16
    x = _logits(n, V, torch.bfloat16, seed=21).to(DEV)
    kw = dict(temperature=0.9, top_k=50, top_p=0.9, seed=12)
    sid = torch.arange(100, 100 + n, device=DEV)
    pos = torch.arange(30, 30 + n, dtype=torch.int32, device=DEV)
    base = S.sample_tokens(x, stream_ids=sid, positions=pos, **kw)
    alone = torch.cat([S.sample_tokens(x[b:b + 1], stream_ids=sid[b:b + 1], positions=pos[b:b + 1], **kw)
                       for b in range(n)])
    assert torch.equal(alone, base)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(DEV)      # another index, other neighbours
    assert torch.equal(S.sample_tokens(x[perm], stream_ids=sid[perm], positions=pos[perm], **kw), base[perm])
    wide = torch.full((n, V + 13), 50.0, dtype=torch.bfloat16, device=DEV)            # a row stride above V
    wide[:, :V] = x
    assert wide[:, :V].stride(0) == V + 13
    assert torch.equal(S.sample_tokens(wide[:, :V], stream_ids=sid, positions=pos, **kw), base)
    other = torch.cat([_logits(3, V, torch.bfloat16, seed=5).to(DEV), x[4:5]])        # among rows it never met
    got = S.sample_tokens(other, stream_ids=torch.cat([sid[:3], sid[4:5]]), positions=torch.cat([pos[:3], pos[4:5]]),
                          temperature=torch.tensor([0.0, 5.0, 1.0, 0.9]), top_k=torch.tensor([0, 3, 0, 50]),
                          top_p=torch.tensor([1.0, 0.5, 1.0, 0.9]), seed=12)
    assert got[3] == base[4]


def test_position_and_stream_id_change_the_draw():
    n, V = 256, 257
    flat = torch.zeros(n, V, dtype=torch.float32, device=DEV)
    sid = torch.arange(n, device=DEV)
    a = S.sample_tokens(flat, temperature=1.0, seed=1, stream_ids=sid, positions=3)
    assert torch.equal(S.sample_tokens(flat, temperature=1.0, seed=1, stream_ids=sid, positions=3), a)
    for kw in (dict(stream_ids=sid, positions=4), dict(stream_ids=sid + 1000, positions=3),
               dict(stream_ids=sid + (1 << 32), positions=3)):
        b = S.sample_tokens(flat, temperature=1.0, seed=1, **kw)
        assert int((a != b).sum()) > n // 2, kw
    assert int((S.sample_tokens(flat, temperature=1.0, seed=2, stream_ids=sid, positions=3) != a).sum()) > n // 2


@pytest.mark.parametrize("case", list(DIST_CASES))
def test_distribution_of_4096_streams_at_one_position(case):
    logits = dist_logits().repeat(DIST_ROWS, 1).to(DEV)
    tok = S.sample_tokens(logits, temperature=1.0, seed=DIST_SEED, positions=DIST_POS, **DIST_CASES[case])
    assert tok.shape == (DIST_ROWS,) and int(tok.max()) < DIST_V
    chi_square_check(tok, case)


def test_launcher_refuses_bad_sizes_and_launches_nothing():
    L = _lib()
    P, st = L.ptr, L.stream()
    B, V = 2, 16
    x = torch.zeros(B, V, dtype=torch.float32, device=DEV)
    f = torch.ones(B, dtype=torch.float32, device=DEV)
    i32 = torch.zeros(B, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(B, dtype=torch.int64, device=DEV)
    tok = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    w = torch.full((B, V), -1, dtype=torch.int32, device=DEV)

    def call(dtype, ld, b, v):
        return L.call_ret("toa_sample_tokens", dtype, P(x), ld, b, v, P(f), P(i32), P(f), P(f), P(i64), P(i32), 0,
                          P(tok), P(w), st)

    # (dtype, ld, B, V)
    for a in ((1, V, 0, V), (1, V, -1, V), (1, V, B, 0), (1, (1 << 20) + 1, B, (1 << 20) + 1), (1, V - 1, B, V),
              (2, V, B, V), (-1, V, B, V)):
        assert call(*a) == INVALID_VALUE, a
    torch.cuda.synchronize()
    assert bool((tok == -1).all()) and bool((w == -1).all())
    assert call(1, V, B, V) == 0
    torch.cuda.synchronize()
    assert tok.tolist() == [0, 0] or bool(((tok >= 0) & (tok < V)).all())
    assert bool((w.to(torch.int64) & 0xFFFFFFFF == ONE - 1).all())      # all logits equal: every token at the maximum


def test_generate_with_the_device_sampler_on_the_tiny_model():
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.train.generate import generate

    m = Llama(PRESETS["llama-tiny"], device=DEV)
    m.init_weights(0)
    m.eval()
    prompts = torch.randint(0, m.cfg.vocab_size, (3, 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    kw = dict(temperature=0.9, top_k=40, top_p=0.95, min_p=0.01, seed=3, sampler="device", split_keys=64)
    sid = torch.tensor([0, 1, 7], device=DEV)
    state = torch.cuda.get_rng_state()
    a, _ = generate(m, prompts, 12, stream_ids=sid, **kw)
    b, _ = generate(m, prompts, 12, stream_ids=sid, **kw)
    assert torch.equal(a, b)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    alone, _ = generate(m, prompts[2:], 12, stream_ids=sid[2:], **kw)
    assert torch.equal(alone[0], a[2])
    c, _ = generate(m, prompts, 12, stream_ids=sid, **{**kw, "seed": 4})
    assert not torch.equal(a, c)
    greedy, _ = generate(m, prompts, 12, split_keys=64)
    k1, _ = generate(m, prompts, 12, temperature=0.7, top_k=1, seed=9, sampler="device", split_keys=64)
    assert torch.equal(k1, greedy)
    mixed, _ = generate(m, prompts, 12, temperature=torch.tensor([0.0, 0.8, 0.0]), seed=3, sampler="device",
                        split_keys=64)
    assert torch.equal(mixed[0], greedy[0]) and torch.equal(mixed[2], greedy[2])
