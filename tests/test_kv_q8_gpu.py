"""The fp8 KV cache on an MI355X (csrc/hip/kv_cache_q8.hip, extend.hip's e4m3
staging): append and fill bit for bit against the quantiser's formula, decode
row by row against the fp64 reference on the values the cache holds (the
bf16 kernel's bound, unchanged), batch invariance and the extend kernel bit
for bit, the refusals, the model."""
import functools
import math

import pytest
import torch

import attn_numerics as an
import test_kv_q8 as cpu
from decode_numerics import DEV, lib as _lib
from test_decode_gpu import CAP, CASES, LAYOUTS
from test_kv_q8 import BF16, E4M3, NAN, bits, dequant, expect

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", LAYOUTS)
def test_append_is_quant_ref_of_the_bf16_cache_and_q_is_the_bf16_paths(Hq, Hkv, D, T):
    _lib()
    cpu.append_case(DEV, Hq, Hkv, D, T)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [1, 70])
def test_fill_cache_is_quant_ref_and_leaves_the_other_slots(P, D):
    _lib()
    cpu.fill_case(DEV, P, D)


# ------------------------------------------------------------------ decode against fp64
@functools.lru_cache(maxsize=None)
def _row(H, Hk, L, D, spike):
    """test_decode_gpu._row with k and v snapped by quantise -> dequantise, so the reference sees exactly the cache's
    values: (q [H, D]; bytes [Hk, L, D] and scales [Hk, L] of k and v on the GPU; ref, mag, model rows [H, D] fp64)."""
    q, k, v, do = an.make_inputs(1, H, Hk, L, D, spike)
    (k8, ks), (v8, vs) = expect(k), expect(v)
    k, v = dequant(k8, ks), dequant(v8, vs)
    scale = 1.0 / math.sqrt(D)
    ref, model = an.attn_ref64(q, k, v, do, scale), an.bf16_model(q, k, v, do, scale)
    return (q[0, :, L - 1].to(DEV), [t[0].to(DEV) for t in (k8, v8, ks, vs)], ref.o[0, :, L - 1],
            ref.mag_o[0, :, L - 1], model.o[0, :, L - 1])


def _batch(H, Hk, D, lengths, spike=False):
    """q [B, H, D], the fp8 cache [B, Hk, CAP, ...] with 0x7f / NaN beyond each row's length, lengths int32 [B]."""
    rows = [_row(H, Hk, L, D, spike) for L in lengths]
    cache = cpu.empty_q8(len(lengths), Hk, CAP, D, DEV)
    for b, (L, r) in enumerate(zip(lengths, rows)):
        for dst, src in zip(cache, r[1]):
            dst[b, :, :L] = src.view(dst.dtype)
    return torch.stack([r[0] for r in rows]), cache, torch.tensor(lengths, dtype=torch.int32, device=DEV), rows


# test_decode_gpu's cases at split_keys 64, and (70, 197, 300) at the default split: a full unrolled pass and a
# predicated tail
Q8_CASES = [c + (64,) for c in CASES] + [(Hq, Hkv, D, (70, 197, 300), False, None)
                                         for D in (64, 128) for Hq, Hkv in LAYOUTS]


@pytest.mark.parametrize("Hq,Hkv,D,lengths,spike,split", Q8_CASES,
                         ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_attn_decode_rows_against_fp64_on_the_caches_values(Hq, Hkv, D, lengths, spike, split):
    from tf_operator_amd.ops import decode as dec

    _lib()
    q, (k8, v8, ks, vs), n, rows = _batch(Hq, Hkv, D, lengths, spike)
    o = dec.attn_decode(q, k8, v8, n, split_keys=split, max_len=max(lengths), k_scale=ks, v_scale=vs).cpu()
    for b, (L, r) in enumerate(zip(lengths, rows)):
        an.check_rows(f"fp8 decode L={L} D={D} {Hq}/{Hkv}", "o", o[b], r[2], r[3], r[4], L, D)


@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_row_does_not_depend_on_its_batch(D):
    from tf_operator_amd.ops import decode as dec

    _lib()
    q, cache, n, _ = _batch(4, 2, D, (70, 197, 300))
    k8, v8, ks, vs = (t[1:2].contiguous() for t in cache)
    for split in (64, None):
        full = dec.attn_decode(q, cache[0], cache[1], n, split_keys=split, max_len=300, k_scale=cache[2],
                               v_scale=cache[3])
        alone = dec.attn_decode(q[1:2].contiguous(), k8, v8, n[1:2].contiguous(), split_keys=split, max_len=197,
                                k_scale=ks, v_scale=vs)
        assert torch.isfinite(full.float()).all()
        assert torch.equal(bits(full[1]), bits(alone[0])), split


# ------------------------------------------------------------------ extend
@pytest.mark.parametrize("split", [64, 0])
@pytest.mark.parametrize("D", [64, 128])
def test_attn_extend_on_the_fp8_cache_is_attn_extend_on_the_dequantised_one(D, split):
    from tf_operator_amd.ops import decode as dec

    _lib()
    B, T, Hq, Hkv, C = 2, 5, 4, 2, 192
    starts, counts = (60, 130), (5, 3)        # a 64-key block and a split boundary are crossed
    g = torch.Generator().manual_seed(D)
    k8, v8, ks, vs = cpu.empty_q8(B, Hkv, C, D, DEV)
    kd = torch.full((B, Hkv, C, D), NAN, dtype=BF16, device=DEV)
    vd = kd.clone()
    for b, L in enumerate(s + c for s, c in zip(starts, counts)):
        for c8, sc, cd in ((k8, ks, kd), (v8, vs, vd)):
            q8, s = expect(torch.randn(Hkv, L, D, generator=g).to(BF16))
            c8[b, :, :L], sc[b, :, :L], cd[b, :, :L] = q8.view(E4M3).to(DEV), s.to(DEV), dequant(q8, s).to(DEV)
    q = torch.randn(B, T, Hq, D, generator=g).to(BF16).to(DEV)
    st, cn = (torch.tensor(a, dtype=torch.int32, device=DEV) for a in (starts, counts))
    got = dec.attn_extend(q, k8, v8, st, cn, split_keys=split, max_len=133, k_scale=ks, v_scale=vs)
    want = dec.attn_extend(q, kd, vd, st, cn, split_keys=split, max_len=133)
    assert torch.isfinite(want.float()).all() and bool(want[0].any())
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    L = _lib()
    cpu.refusal_case(DEV)
    P, st = L.ptr, L.stream()
    k8, v8, ks, vs = cpu.empty_q8(2, 2, 16, 96, DEV)
    q = torch.full((2, 4, 96), NAN, dtype=BF16, device=DEV)
    o, ws = torch.full_like(q, NAN), torch.zeros(4096, device=DEV)
    n = torch.ones(2, dtype=torch.int32, device=DEV)
    assert L.call_ret("toa_attn_decode_q8", P(q), P(k8), P(v8), P(ks), P(vs), P(n), P(ws), P(o), 2, 4, 2, 16, 96, 16,
                      64, 0.125, st) == 1
    assert L.call_ret("toa_kv_quant_rows", P(q), P(q), P(k8), P(v8), P(ks), P(vs), 2, 2, 2, 96, 16, st) == 1
    assert L.call_ret("toa_attn_decode_q8", P(q), P(k8), P(v8), None, P(vs), P(n), P(ws), P(o), 2, 4, 2, 16, 64, 16,
                      64, 0.125, st) == 1
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all() and not ws.any() and bool((bits(k8) == 0x7f).all()) and torch.isnan(ks).all()


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("preset", ["llama-tiny", "llama-tiny128"])
def test_model_prefill_fills_quant_ref_and_a_row_decodes_as_if_alone(preset):
    from tf_operator_amd.models.llama import PRESETS, Llama
    from tf_operator_amd.train.generate import generate

    _lib()
    m = Llama(PRESETS[preset], device=DEV)
    m.init_weights(0)
    m.eval()
    P, lengths = 9, [9, 6, 3]
    tokens = torch.randint(0, m.cfg.vocab_size, (3, 16), generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        plain, q8 = m.new_cache(3, 16), m.new_cache(3, 16, dtype=E4M3)
        assert torch.equal(bits(m.prefill(tokens[:, :P], plain)), bits(m.prefill(tokens[:, :P], q8)))
        w = (torch.arange(16) < P).expand(3, m.cfg.kv_heads, 16)
        for i in range(m.cfg.layers):
            for c8, sc, c16 in ((q8.k[i], q8.k_scale[i], plain.k[i]), (q8.v[i], q8.v_scale[i], plain.v[i])):
                want_q, want_s = expect(c16)
                assert torch.equal(bits(c8)[w], want_q[w]) and torch.equal(bits(sc)[w], bits(want_s)[w]), i

        def run(rows):
            """Ragged rows: a chunked prefill, three decode steps and an extend by two, on the row-invariant GEMM."""
            t, c = tokens[rows], m.new_cache(len(rows), 16, dtype=E4M3)
            lg = [m.prefill(t[:, :P], c, [lengths[b] for b in rows], gemm="skinny", chunk=4)]
            lg += [m.decode_step(t[:, P + s], c, gemm="skinny") for s in range(3)]
            return torch.stack(lg + [m.extend(t[:, 12:14], c, gemm="skinny")])

        full, alone = run([0, 1, 2]), run([1])
    assert torch.isfinite(full.float()).all()
    assert torch.equal(bits(full[:, 1]), bits(alone[:, 0]))
    out, n = generate(m, tokens[:2, :5], 6, kv="fp8")
    assert out.shape == (2, 11) and n.tolist() == [11, 11]
