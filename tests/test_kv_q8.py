"""The fp8 KV cache, the CPU tier (csrc/hip/kv_cache_q8.hip through
ops/decode.py and Llama / generate): append and fill against the quantiser's
formula (test_gemm_w8.quant_ref), attention against _attn_ref on the
dequantised cache, the argument checks.  tests/test_kv_q8_gpu.py runs the same
cases on the device through the helpers here."""
import pytest
import torch

import decode_numerics as dn
from test_gemm_w8 import quant_ref
from tf_operator_amd.ops import decode as dec
from tf_operator_amd.ops.llm import rope_tables

BF16, E4M3, NAN = torch.bfloat16, torch.float8_e4m3fn, float("nan")
LAYOUTS = ((2, 2), (4, 1), (4, 2))   # tests/test_decode_gpu.py's (Hq, Hkv)
bits = lambda t: t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()  # noqa: E731


def expect(rows):
    """(bytes uint8 [..., D], scale fp32 [...]) of rows [..., D] by quant_ref.  A row with a non-finite element has
    scale NaN, the issue's rule; its bytes are set to 0 here and are not compared (slots_are)."""
    flat = rows.reshape(-1, rows.shape[-1]).cpu()
    q, s, _ = quant_ref(flat)
    bad = ~torch.isfinite(flat.float()).all(1)
    q, s = q.view(torch.uint8).clone(), s.clone()
    q[bad], s[bad] = 0, NAN
    return q.view(rows.shape), s.view(rows.shape[:-1])


def slots_are(name, c8, sc, rows, w):
    """Where w [B, Hkv, n]: bytes and scale bits equal expect(rows); elsewhere the sentinels."""
    want_q, want_s = expect(rows)
    fin = w & ~torch.isnan(want_s)
    assert torch.equal(bits(c8)[fin], want_q[fin]), name
    assert torch.equal(bits(sc)[w], bits(want_s)[w]), name
    assert bool((bits(c8)[~w] == 0x7f).all()) and bool(torch.isnan(sc.cpu()[~w]).all()), name


def dequant(q8, scale):
    return (q8.view(E4M3).float() * scale[..., None]).to(BF16)


def empty_q8(B, Hkv, C, D, dev):
    """Sentinels everywhere: bytes 0x7f (e4m3 NaN), scales NaN."""
    k8 = torch.full((B, Hkv, C, D), 0x7f, dtype=torch.uint8, device=dev).view(E4M3)
    ks = torch.full((B, Hkv, C), NAN, device=dev)
    return k8, k8.clone(), ks, ks.clone()


def append_case(dev, Hq, Hkv, D, T):
    """The bf16 and the fp8 append on the same qkv: q bit for bit, the written slots quant_ref of the bf16 cache's
    rows, every other slot its sentinel.  T = 1: rope_append; T = 3: rope_append_many with counts (3, 1, 0)."""
    B, C = 3, 32
    start, count = ([0, 17, C - 1], [1, 1, 1]) if T == 1 else ([5, 0, 9], [3, 1, 0])
    there = [(b, t) for b in range(B) for t in range(count[b])]
    x = torch.randn(B, T, Hq + 2 * Hkv, D, generator=torch.Generator().manual_seed(D + Hq + T)).to(BF16)
    v = x[:, :, Hq + Hkv:]                       # the exponent rule's edges, in V (unrotated)
    v[there[0]] = 0
    v[there[1]] = v[there[1]].clamp(-1, 1)
    v[there[2]] = v[there[2]].clamp(-1, 1)
    v[there[1]][:, 3], v[there[2]][:, 3] = 1.75 * 2.0 ** 3, 1.7578125 * 2.0 ** 3   # amax = 448 2^-5; just above 1.75
    x[there[-1]][Hq, 5] = float("inf")           # one non-finite element in a K row
    qkv = x.view(B, T, -1).to(dev)
    cos, sin = rope_tables(C, D, device=dev)
    st, cn = (torch.tensor(a, dtype=torch.int32, device=dev) for a in (start, count))
    kc = torch.full((B, Hkv, C, D), 0x1234, dtype=torch.int16, device=dev).view(BF16)
    vc = kc.clone()
    k8, v8, ks, vs = empty_q8(B, Hkv, C, D, dev)
    if T == 1:
        q = dec.rope_append(qkv[:, 0], cos, sin, st, kc, vc, Hq, Hkv, D)
        q8 = dec.rope_append(qkv[:, 0], cos, sin, st, k8, v8, Hq, Hkv, D, k_scale=ks, v_scale=vs)
    else:
        q = dec.rope_append_many(qkv, cos, sin, st, cn, kc, vc, Hq, Hkv, D)
        q8 = dec.rope_append_many(qkv, cos, sin, st, cn, k8, v8, Hq, Hkv, D, k_scale=ks, v_scale=vs)
    assert torch.equal(bits(q), bits(q8))
    written = torch.zeros(B, C, dtype=torch.bool)
    for b, t in there:
        written[b, start[b] + t] = True
    for name, c16, c8, sc in (("k", kc, k8, ks), ("v", vc, v8, vs)):
        slots_are(name, c8, sc, c16, written[:, None].expand(B, Hkv, C))
    s_v = vs.cpu()
    assert [float(s_v[b, 0, start[b] + t]) for b, t in there[:3]] == [1.0, 2.0 ** -5, 2.0 ** -4]
    b, t = there[-1]
    assert bool(torch.isnan(ks.cpu()[b, 0, start[b] + t]))


def fill_case(dev, P, D):
    B, Hkv, C = 2, 2, 80
    k, v = (torch.randn(B, Hkv, P, D, generator=torch.Generator().manual_seed(P + i)).to(BF16) for i in (0, 1))
    k[0, 0, 0], v[1, 1, P - 1, 7] = 0, float("inf")
    k8, v8, ks, vs = empty_q8(B, Hkv, C, D, dev)
    dec.fill_cache(k.to(dev), v.to(dev), k8, v8, ks, vs)
    w = (torch.arange(C) < P).expand(B, Hkv, C)
    for name, src, c8, sc in (("k", k, k8, ks), ("v", v, v8, vs)):
        rows = torch.zeros(B, Hkv, C, D, dtype=BF16)
        rows[:, :, :P] = src
        slots_are(name, c8, sc, rows, w)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", LAYOUTS)
def test_append_on_the_cpu_is_quant_ref_of_the_bf16_cache(Hq, Hkv, D, T):
    append_case("cpu", Hq, Hkv, D, T)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [1, 70])
def test_fill_cache_on_the_cpu_is_quant_ref(P, D):
    fill_case("cpu", P, D)


def test_attention_on_the_cpu_is_the_reference_on_the_dequantised_cache():
    B, T, Hq, Hkv, C, D = 2, 5, 4, 2, 40, 64
    g = torch.Generator().manual_seed(3)
    k8, ks = expect(torch.randn(B, Hkv, C, D, generator=g).to(BF16))
    v8, vs = expect(torch.randn(B, Hkv, C, D, generator=g).to(BF16))
    k8, v8 = k8.view(E4M3), v8.view(E4M3)
    q = torch.randn(B, T, Hq, D, generator=g).to(BF16)
    start, count = torch.tensor([30, 7], dtype=torch.int32), torch.tensor([5, 3], dtype=torch.int32)
    kd, vd = dequant(k8, ks), dequant(v8, vs)
    got = dec.attn_extend(q, k8, v8, start, count, k_scale=ks, v_scale=vs)
    assert torch.equal(bits(got), bits(dec._attn_ref(q, kd, vd, start, count, C, D ** -0.5)))
    n = start + count
    got = dec.attn_decode(q[:, 0], k8, v8, n, k_scale=ks, v_scale=vs)
    assert torch.equal(bits(got), bits(dec.attn_decode(q[:, 0], kd, vd, n)))


def refusal_case(dev):
    """e4m3 caches without scales, scales of the wrong shape or dtype, scales with bf16 caches, D = 96: ValueError
    before anything runs."""
    B, Hq, Hkv, C, D = 2, 4, 2, 16, 64
    k8, v8, ks, vs = empty_q8(B, Hkv, C, D, dev)
    kc = torch.zeros(B, Hkv, C, D, dtype=BF16, device=dev)
    q = torch.zeros(B, Hq, D, dtype=BF16, device=dev)
    n = torch.ones(B, dtype=torch.int32, device=dev)
    for kw in (dict(), dict(k_scale=ks), dict(k_scale=ks[:, :, 1:], v_scale=vs), dict(k_scale=ks.double(), v_scale=vs)):
        with pytest.raises(ValueError, match="scale"):
            dec.attn_decode(q, k8, v8, n, **kw)
        with pytest.raises(ValueError, match="scale"):
            dec.attn_extend(q[:, None], k8, v8, n, n, **kw)
    with pytest.raises(ValueError, match="scale"):
        dec.attn_decode(q, kc, kc.clone(), n, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="scale"):
        dec.fill_cache(kc[:, :, :4], kc[:, :, :4], k8, v8, ks, None)
    q96, c96 = torch.zeros(B, Hq, 96, dtype=BF16, device=dev), empty_q8(B, Hkv, C, 96, dev)
    with pytest.raises(ValueError, match="head_dim"):
        dec.attn_decode(q96, c96[0], c96[1], n, k_scale=c96[2], v_scale=c96[3])
    with pytest.raises(ValueError, match="head_dim"):
        dec.fill_cache(torch.zeros(B, Hkv, 4, 96, dtype=BF16, device=dev), torch.zeros(B, Hkv, 4, 96, dtype=BF16, device=dev), *c96)
    assert bool((bits(k8) == 0x7f).all()) and bool(torch.isnan(ks).all())


def test_refusals_on_the_cpu():
    refusal_case("cpu")


def test_cache_model_and_generate_arguments(monkeypatch):
    from tf_operator_amd.train.generate import generate

    c = dec.KVCache(2, 3, 2, 16, 64, "cpu", dtype=E4M3)
    assert c.k[0].dtype == E4M3 and c.k_scale[1].shape == (3, 2, 16) and c.scales(1)["v_scale"] is c.v_scale[1]
    plain = dec.KVCache(2, 3, 2, 16, 64, "cpu")
    assert plain.scales(0) == dict(k_scale=None, v_scale=None)
    assert c.nbytes() * 2 * 64 == plain.nbytes() * (64 + 4)   # D bytes and one fp32 scale against 2 D bytes a row
    with pytest.raises(ValueError, match="dtype"):
        dec.KVCache(2, 3, 2, 16, 64, "cpu", dtype=torch.float8_e5m2)
    m = dn.model()
    prompts = torch.randint(0, m.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(1))
    out, _ = generate(m, prompts, 4, kv="fp8")
    assert out.shape == (2, 10)
    with pytest.raises(ValueError, match="kv"):
        generate(m, prompts, 4, kv="e5m2")
    monkeypatch.setenv("TOA_DECODE_KV", "int8")
    with pytest.raises(ValueError, match="TOA_DECODE_KV"):
        generate(m, prompts, 4)


def test_model_on_the_cpu_fills_the_cache_with_quant_ref_of_the_plain_one():
    m = dn.model()
    tokens = dn.fixture(24)["tokens"]
    with torch.no_grad():
        plain, q8 = m.new_cache(2, 24), m.new_cache(2, 24, dtype=E4M3)
        assert torch.equal(m.prefill(tokens[:, :9], plain), m.prefill(tokens[:, :9], q8))
        for i in range(m.cfg.layers):
            want_q, want_s = expect(plain.k[i][:, :, :9])
            assert torch.equal(bits(q8.k[i])[:, :, :9], want_q) and torch.equal(q8.k_scale[i][:, :, :9], want_s)
        lg = [m.decode_step(tokens[:, t], q8) for t in range(9, 12)] + [m.extend(tokens[:, 12:15], q8)]
    assert all(bool(torch.isfinite(x).all()) for x in lg) and q8.host_lengths == [15, 15]
