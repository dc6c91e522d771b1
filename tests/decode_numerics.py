"""What the KV-cache tests share (test_decode.py and test_extend.py on the CPU
tier, test_decode_gpu.py and test_extend_gpu.py on the GPU): the llama-tiny
model, its forward in fp64 from the plain formulas, the fixture and the
tolerance that follows from it, and the teacher-forcing bound of the GPU tests.

The yardstick is always the existing full forward, ``model(tokens)``, never the
code under test."""
import functools

import torch

import attn_numerics as an
from attn_numerics import U
from tf_operator_amd.models.llama import PRESETS, Llama
from tf_operator_amd.ops.llm import rope_tables

DEV = "cuda"
FACTOR = 3.0   # the CPU tolerance: FACTOR x the fp32 full forward's deviation from fp64


def model(dtype=torch.float32):
    m = Llama(PRESETS["llama-tiny"], device="cpu", dtype=dtype)
    m.init_weights(0)
    return m.eval()


def forward64(model, tokens):
    """The model's forward in fp64 from the plain formulas: logits [B, S, V]."""
    cfg = model.cfg
    B, S = tokens.shape
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    cos, sin = (t.double() for t in rope_tables(S, D, cfg.rope_theta))   # the model's own (fp32) table values

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.norm_eps) * w.double()

    def rope(x):   # [B, H, S, D]
        x1, x2 = x[..., :D // 2], x[..., D // 2:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)

    h = model.embed.weight.double()[tokens]
    mask = torch.ones(S, S, dtype=torch.bool).triu(1)
    for blk in model.blocks:
        x = rms(h, blk.attn_norm.weight)
        qkv = (x @ blk.wqkv.double().t()).view(B, S, Hq + 2 * Hkv, D).transpose(1, 2)
        q, k, v = rope(qkv[:, :Hq]), rope(qkv[:, Hq:Hq + Hkv]), qkv[:, Hq + Hkv:]
        k, v = (t.repeat_interleave(Hq // Hkv, 1) for t in (k, v))
        s = (q @ k.transpose(-1, -2) / D ** 0.5).masked_fill(mask, float("-inf"))
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, Hq * D)
        h = h + o @ blk.wo.double().t()
        x = rms(h, blk.mlp_norm.weight)
        gu = x @ blk.wgu.double().t()
        h = h + (torch.nn.functional.silu(gu[..., :cfg.ffn]) * gu[..., cfg.ffn:]) @ blk.wd.double().t()
    return rms(h, model.norm.weight) @ model.head_weight().double().t()


def row_dev(a, b, ref):
    """max over rows of ||a - b|| / ||ref||, rows = the last dimension."""
    return float(((a.double() - b.double()).norm(dim=-1) / ref.double().norm(dim=-1)).max())


@functools.lru_cache(maxsize=None)
def fixture(total):
    """The fp32 model, a fixed random sequence [2, total], its full-forward
    logits, the fp64 reference and the tolerance that follows; computed once
    per length, read-only."""
    m = model()
    tokens = torch.randint(0, m.cfg.vocab_size, (2, total), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        full = m(tokens)
        ref = forward64(m, tokens)
    dev = row_dev(full, ref, ref)
    print(f"fp32 full forward vs fp64: {dev:.3e} of a row's norm -> tolerance {FACTOR * dev:.3e}")
    assert 0 < dev < 1e-5, dev   # fp32 rounding, nothing else
    return dict(model=m, tokens=tokens, full=full, ref=ref, tol=FACTOR * dev)


# ------------------------------------------------------------------ the GPU tests
def lib():
    from tf_operator_amd.ops import _lib as L

    assert L.available(), L.load_error()
    return L


@functools.lru_cache(maxsize=None)
def teacher(preset, total):
    """bf16 model on the GPU, the same weights in fp32 on the CPU (the torch
    fallbacks), a fixed random sequence [2, total]; the fp32 reference logits
    and the bf16 full forward's, [2, total, V] fp64 on the CPU."""
    m = Llama(PRESETS[preset], device=DEV)
    m.init_weights(0)
    m.eval()
    ref_m = Llama(PRESETS[preset], device="cpu", dtype=torch.float32).eval()
    ref_m.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    tokens = torch.randint(0, m.cfg.vocab_size, (2, total), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = ref_m(tokens).double()
        full = m(tokens.to(DEV)).double().cpu()
    return m, ref_m, tokens, ref, full


def row_rel(a, ref):
    return (a - ref).norm(dim=-1) / ref.norm(dim=-1)


def check_teacher(what, got, ref, full, first, D, total):
    """got [B, n, V] at positions first .. first + n - 1 of `total` within 3 x the full forward's error + the fp32
    floor."""
    n = got.shape[1]
    ref, full = ref[:, first:first + n], full[:, first:first + n]
    e_full, e = row_rel(full, ref), row_rel(got, ref)
    limit = 3.0 * e_full + an.fp32_floor(total, D)
    ratio = e / limit
    i = int(ratio.flatten().argmax())
    b, t = i // n, i % n
    print(f"{what}: full forward {float(e_full.max()) / U:.3f} u max, {float(e_full.mean()) / U:.3f} u mean; "
          f"{float(e.max()) / U:.3f} u max, {float(e.mean()) / U:.3f} u mean; worst / limit {float(ratio.max()):.3f} at "
          f"row {b} position {first + t} ({float(e[b, t]) / U:.3f} u, full {float(e_full[b, t]) / U:.3f} u)")
    assert torch.isfinite(got).all()
    assert bool((e <= limit).all()), (what, b, first + t, float(e[b, t]), float(e_full[b, t]))
