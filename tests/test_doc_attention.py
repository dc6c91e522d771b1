"""Document-masked causal attention, the parts that need no GPU: the boundary
arrays (ops/llm.doc_bounds, doc_bounds_from_lengths), the masked reference,
the synthetic document stream and the CPU trainer with doc_eos."""
import math

import pytest
import torch

EOS = 9


def _rows():
    """Hand-written rows of S = 8 and their documents' lengths: EOS at 0,
    EOS at S - 1, two adjacent EOS (a length-1 document), no EOS at all."""
    return [([EOS, 1, 2, 3, 4, 5, 6, 7], [1, 7]),
            ([1, 2, 3, 4, 5, 6, 7, EOS], [8]),
            ([1, 2, EOS, EOS, 3, 4, EOS, 5], [3, 1, 3, 1]),
            ([1, 2, 3, 4, 5, 6, 7, 8], [8])]


def test_doc_bounds_hand_written_rows():
    from tf_operator_amd.ops.llm import doc_bounds

    tok = torch.tensor([r for r, _ in _rows()])
    ds, de = doc_bounds(tok, EOS)
    assert ds.dtype == torch.int32 and de.dtype == torch.int32 and ds.shape == de.shape == (4, 8)
    assert ds.tolist() == [[0, 1, 1, 1, 1, 1, 1, 1],     # the EOS at 0 is a document of its own
                           [0, 0, 0, 0, 0, 0, 0, 0],     # an EOS at S - 1 ends the row's only document
                           [0, 0, 0, 3, 4, 4, 4, 7],     # the second of two adjacent EOS: length 1
                           [0, 0, 0, 0, 0, 0, 0, 0]]
    assert de.tolist() == [[1, 8, 8, 8, 8, 8, 8, 8],
                           [8, 8, 8, 8, 8, 8, 8, 8],
                           [3, 3, 3, 4, 7, 7, 7, 8],
                           [8, 8, 8, 8, 8, 8, 8, 8]]


def test_doc_bounds_from_lengths_agrees():
    from tf_operator_amd.ops.llm import doc_bounds, doc_bounds_from_lengths

    tok = torch.tensor([r for r, _ in _rows()])
    ds, de = doc_bounds(tok, EOS)
    ls, le = doc_bounds_from_lengths([n for _, n in _rows()], 8)
    assert ls.dtype == torch.int32 and le.dtype == torch.int32
    assert torch.equal(ds, ls) and torch.equal(de, le)
    with pytest.raises(ValueError):
        doc_bounds_from_lengths([[3, 4]], 8)


# the GPU numerics test's rows: a boundary inside a tile, on tile and block edges, a length-1 document
STARTS = [[0, 10, 80, 81, 128, 256, 293], [0, 64, 300]]


def _lengths(starts, S):
    return [[b - a for a, b in zip(s, s[1:] + [S])] for s in starts]


def test_masked_reference_is_each_document_alone():
    """Exactly, in fp32, forward and gradients; and against the dense
    predicate doc_start[i] <= j <= i written out here, to fp32 rounding."""
    from tf_operator_amd.ops.llm import _attention_reference, doc_bounds_from_lengths

    torch.manual_seed(0)
    B, H, Hk, S, D = 2, 4, 2, 320, 64
    scale = 1.0 / math.sqrt(D)
    q, k, v = (torch.randn(B, h, S, D, requires_grad=True) for h in (H, Hk, Hk))
    doc = doc_bounds_from_lengths(_lengths(STARTS, S), S)
    o = _attention_reference(q, k, v, scale, doc)
    do = torch.randn_like(o)
    g = torch.autograd.grad(o, (q, k, v), do)
    for b, starts in enumerate(STARTS):
        for a, e in zip(starts, starts[1:] + [S]):
            qa, ka, va = (t[b:b + 1, :, a:e].detach().clone().requires_grad_() for t in (q, k, v))
            oa = _attention_reference(qa, ka, va, scale)
            assert torch.equal(oa, o[b:b + 1, :, a:e]), (b, a, e)
            ga = torch.autograd.grad(oa, (qa, ka, va), do[b:b + 1, :, a:e])
            for x, y in zip(ga, g):
                assert torch.equal(x, y[b:b + 1, :, a:e]), (b, a, e)
    with torch.no_grad():
        kf, vf = k.repeat_interleave(H // Hk, 1), v.repeat_interleave(H // Hk, 1)
        s = torch.matmul(q, kf.transpose(-1, -2)) * scale
        i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
        seen = (j <= i)[None] & (j[None] >= doc[0].long()[:, :, None])
        dense = torch.matmul(torch.softmax(s.masked_fill(~seen[:, None], float("-inf")), -1), vf)
    assert float((dense - o.detach()).abs().max()) < 1e-5
    assert float((o - _attention_reference(q, k, v, scale)).detach().abs().max()) > 1e-2   # the mask does something


def test_causal_attention_cpu_takes_doc():
    from tf_operator_amd.ops.llm import _attention_reference, causal_attention, doc_bounds_from_lengths

    torch.manual_seed(1)
    q, k, v = (torch.randn(1, h, 16, 64) for h in (2, 1, 1))
    doc = doc_bounds_from_lengths([[5, 11]], 16)
    o = causal_attention(q, k, v, out_layout="bshd", doc=doc)
    assert torch.equal(o, _attention_reference(q, k, v, 0.125, doc).transpose(1, 2))


def test_synthetic_tokens_documents_are_a_pure_function():
    from tf_operator_amd.ops.llm import doc_bounds
    from tf_operator_amd.train.data import SyntheticTokens

    mk = lambda **kw: SyntheticTokens(2, 256, 512, rank=1, seed=5, doc_len=(8, 40), eos_id=3, **kw)
    a, b = mk(), mk()
    first = [a.next() for _ in range(3)]
    for x, y in zip(first, [b.next() for _ in range(3)]):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert not torch.equal(first[0][0], first[1][0])
    c = mk()
    c.load_state_dict(a.state_dict())       # the cursor is still the whole state
    assert a.state_dict() == {"cursor": 3, "seed": 5, "rank": 1}
    na, nc = a.next(), c.next()
    assert torch.equal(na[0], nc[0]) and torch.equal(na[1], nc[1])
    tok, tgt = first[0]
    assert torch.equal(tok[:, 1:], tgt[:, :-1])
    ds, de = doc_bounds(tok, 3)
    lens = (de - ds)[tok == 3]               # every EOS closes a document of lo..hi tokens
    assert lens.numel() >= 2 * (256 // 40) and int(lens.min()) >= 8 and int(lens.max()) <= 40
    # without doc_len the stream is what it was
    plain = SyntheticTokens(2, 256, 512, rank=1, seed=5).next()[0]
    g = torch.Generator().manual_seed((5 * 1000003 + 1) * 1000003)
    assert torch.equal(plain, torch.randint(0, 512, (2, 257), generator=g)[:, :-1])
    with pytest.raises(ValueError):
        SyntheticTokens(2, 256, 512, doc_len=(8, 40))


def test_cpu_trainer_with_doc_eos():
    """llama-tiny on the CPU: 3 steps with finite, decreasing loss, and a
    first-step loss that is not the unmasked trainer's on the same tokens."""
    from tf_operator_amd.train.data import SyntheticTokens
    from tf_operator_amd.train.llm import LlamaTrainer

    batch = SyntheticTokens(2, 96, 512, doc_len=(8, 40), eos_id=3).next()
    masked = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=96, lr=1e-3, doc_eos=3)
    losses = [float(masked.step([batch])) for _ in range(3)]
    assert all(math.isfinite(x) for x in losses), losses
    assert losses[2] < losses[1] < losses[0], losses
    plain = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=96, lr=1e-3)
    first = float(plain.step([batch]))
    assert math.isfinite(first) and first != losses[0], (first, losses[0])
    with pytest.raises(ValueError):
        LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=96, doc_eos=512)
