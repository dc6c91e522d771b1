"""The per-row attention checker (tests/attn_numerics.py) on the CPU: the
torch fallback of causal_attention passes it, seeded faults that the
whole-tensor measure of tests/test_ops_gpu.py accepts do not, and the bf16
model the tolerance rests on stays within 2 u at the GPU tests' inputs."""
import math

import pytest
import torch

import attn_numerics as an
from attn_numerics import U
from tf_operator_amd.ops import llm

O_TOL, G_TOL = 2e-2, 3e-2   # the whole-tensor limits of test_flash_attention_fwd_bwd


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _cpu_attention(q, k, v, do, doc=None):
    """(o, dq, dk, dv) of causal_attention on CPU tensors (ops.llm._attention_reference)."""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = llm.causal_attention(q, k, v, doc=doc)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,H,Hk,S,D,doc", [(1, 4, 2, 257, 64, False), (2, 4, 1, 129, 128, False),
                                            (1, 2, 2, 1, 64, False), (2, 4, 2, 257, 64, True),
                                            (2, 2, 1, 300, 128, True)])
def test_cpu_attention_passes_the_row_check(B, H, Hk, S, D, doc):
    q, k, v, do = an.make_inputs(B, H, Hk, S, D, seed=3)
    if doc:
        doc = llm.doc_bounds_from_lengths([an.doc_lengths(S), an.doc_lengths(S, (64, 256))][:B], S)
    case = an.Case(q, k, v, do, doc=doc or None)
    for name, got in zip(("o", "dq", "dk", "dv"), _cpu_attention(q, k, v, do, doc or None)):
        case.check(name, got, "cpu")


@pytest.fixture(scope="module")
def passing():
    """B=1, H=4, Hk=2, S=257, D=64 with key 256 aligned with query 255 of head
    0 (weight 0.06 of that key if row 255 saw it; an unaligned key's 0.002
    moves the row by less than the rounding allowance, which is what the
    bit-for-bit causality tests on the GPU are for), the reference, and the
    CPU path's result, which passes."""
    B, H, Hk, S, D = 1, 4, 2, 257, 64
    q, k, v, do = an.make_inputs(B, H, Hk, S, D, seed=4)
    k[0, 0, 256] = 0.375 * q[0, 0, 255]
    case = an.Case(q, k, v, do)
    got = dict(zip(("o", "dq", "dk", "dv"), _cpu_attention(q, k, v, do)))
    for name, t in got.items():
        case.check(name, t, "passing")
        assert rel(t, getattr(case.ref, name)) < (O_TOL if name == "o" else G_TOL)
    return case, got


def _rejected_but_old_accepts(case, name, bad, old_tol):
    e, row = case.err(name, bad)
    old = rel(bad, getattr(case.ref, name))
    print(f"fault in {name}: row_err {e / U:.2f} u at {row} (limit {case.tol[name] / U:.2f} u); whole-tensor rel "
          f"{old:.2e} (limit {old_tol})")
    assert not case.ok(name, bad), f"the per-row check accepted the fault ({e / U:.2f} u)"
    with pytest.raises(AssertionError):
        case.check(name, bad)
    assert old < old_tol, f"the whole-tensor measure was meant to accept this fault ({old:.2e})"


def test_fault_last_o_row_scaled(passing):
    """(a) the last O row of one head x 0.9: 2e-3 of the whole tensor."""
    case, got = passing
    bad = got["o"].clone()
    bad[0, 2, 256] = (bad[0, 2, 256].float() * 0.9).to(bad.dtype)
    _rejected_but_old_accepts(case, "o", bad, O_TOL)


def test_fault_row_sees_one_key_too_many(passing):
    """(b) the mask loosened by one at one row: row 255, the last of the
    first 256-row block, also sees key 256 (257 keys), in every head."""
    case, got = passing
    q, k, v = (t.double() for t in (case.q, case.k, case.v))
    rep = q.shape[1] // k.shape[1]
    ke, ve = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    p = torch.softmax(torch.einsum("bhd,bhjd->bhj", q[:, :, 255], ke[:, :, :257]) * case.scale, -1)
    print("leaked weight per head", p[0, :, 256].tolist())
    bad = got["o"].clone()
    bad[:, :, 255] = torch.einsum("bhj,bhjd->bhd", p, ve[:, :, :257]).to(bad.dtype)
    _rejected_but_old_accepts(case, "o", bad, O_TOL)


def test_fault_dk_misses_a_head_of_the_group(passing):
    """(c) dK of kv head 0 without its second query head, for key rows >= 250."""
    case, got = passing
    rep = case.q.shape[1] // case.k.shape[1]
    per_head = an.attn_ref64(case.q, case.k.repeat_interleave(rep, 1), case.v.repeat_interleave(rep, 1), case.do,
                             case.scale).dk
    bad = got["dk"].clone()
    bad[0, 0, 250:] = (bad[0, 0, 250:].double() - per_head[0, 1, 250:]).to(bad.dtype)
    _rejected_but_old_accepts(case, "dk", bad, G_TOL)


def test_fault_dv_tail_rows_zero(passing):
    """(d) dV rows >= 255 are zero."""
    case, got = passing
    bad = got["dv"].clone()
    bad[:, :, 255:] = 0
    _rejected_but_old_accepts(case, "dv", bad, G_TOL)


@pytest.mark.parametrize("shape", an.RAGGED_SHAPES + an.BLOCK_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_model_within_two_u(shape):
    """The tolerance rule is 3 x the model's own row error: the model must be
    a sane one, <= 2 u per row (and its lse within 2e-3), at the inputs of
    the GPU tests."""
    case = an.Case(*an.make_inputs(*shape))
    print(shape, {n: round(e / U, 2) for n, e in case.model_err.items()}, case.model_lse_dev)
    assert max(case.model_err.values()) <= 2 * U, case.model_err
    assert case.model_lse_dev <= 2e-3
    assert all(t <= an.CAP for t in case.tol.values())


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [257, 512])
def test_model_within_two_u_doc(S, D):
    q, k, v, do = an.make_inputs(2, 4, 2, S, D)
    doc = llm.doc_bounds_from_lengths([an.doc_lengths(S), an.doc_lengths(S, (64, 256))], S)
    case = an.Case(q, k, v, do, doc=doc)
    assert max(case.model_err.values()) <= 2 * U, case.model_err
    assert case.model_lse_dev <= 2e-3


def test_row_err_and_rope_helpers():
    """row_err: the worst row and its index, NaN counts as wrong, a zero
    magnitude row with a zero difference is 0; rope_back inverts _rope_ref."""
    ref = torch.zeros(2, 3, 4, dtype=torch.float64)
    mag = torch.ones(2, 3, 4, dtype=torch.float64)
    got = ref.clone()
    got[1, 2, 0] = 0.5
    assert an.row_err(got, ref, mag) == (0.25, (1, 2))
    got[0, 1, 3] = float("nan")
    assert an.row_err(got, ref, mag) == (float("inf"), (0, 1))
    mag[0, 0] = 0
    assert an.row_err(ref, ref, mag)[0] == 0.0
    cos, sin = llm.rope_tables(5, 8)
    x = torch.randn(1, 2, 5, 8, dtype=torch.float64)
    back = an.rope_back(llm._rope_ref(x.float(), cos, sin).double(), cos, sin)
    assert float((back - x).abs().max()) < 1e-6
    assert math.isclose(an.fp32_floor(768, 128), 896 * 2.0 ** -24)
