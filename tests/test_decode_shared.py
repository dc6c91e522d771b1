"""Shared-prompt decoding on the CPU tier (ops/decode.py SharedKVCache,
rope_append_shared, attn_decode_shared; train/generate.py samples=): n samples
per prompt on one prefix cache give the tokens of the prompt repeated n times
on a plain cache, and the cache refuses what it cannot hold before anything is
written."""
import pytest
import torch

from decode_numerics import model as _model
from tf_operator_amd.ops import decode as dec
from tf_operator_amd.train.generate import generate


@pytest.mark.parametrize("temperature", [0.0, 0.8])
@pytest.mark.parametrize("n", [1, 3])
def test_samples_give_the_tokens_of_the_repeated_prompt(n, temperature):
    m = _model()
    prompts = torch.randint(0, m.cfg.vocab_size, (2, 9), generator=torch.Generator().manual_seed(11))
    lens = [9, 4]   # ragged: the second row is padded
    kw = dict(temperature=temperature, top_k=12, seed=5, split_keys=64)
    got, gl = generate(m, prompts, 7, lengths=lens, samples=n, **kw)
    want, wl = generate(m, prompts.repeat_interleave(n, 0), 7, lengths=[x for x in lens for _ in range(n)], **kw)
    assert got.shape == (2 * n, 16)
    assert torch.equal(got, want) and torch.equal(gl, wl)
    if n > 1 and temperature:   # one generator over all rows: the samples of a prompt differ
        assert not torch.equal(got[0], got[1])


def test_overflow_and_fp8_raise_before_anything_is_written():
    m = _model()
    cache = m.new_shared_cache(2, 3, 8, 2)
    assert (cache.prefix.batch, cache.suffix.batch, cache.batch) == (2, 6, 6)
    assert cache.nbytes() == cache.prefix.nbytes() + cache.suffix.nbytes()
    tokens = torch.zeros(6, dtype=torch.int64)
    m.prefill(torch.zeros(2, 8, dtype=torch.int64), cache.prefix)
    for _ in range(2):
        m.decode_step(tokens, cache)
    before = [t.clone() for t in cache.suffix.k + cache.suffix.v]
    with pytest.raises(ValueError, match="overflow"):
        m.decode_step(tokens, cache)
    assert cache.suffix.host_lengths == [2] * 6 == cache.suffix.lengths.tolist()
    assert all(torch.equal(a, b) for a, b in zip(before, cache.suffix.k + cache.suffix.v))
    with pytest.raises(ValueError, match="extend"):
        m.extend(tokens[:, None], cache)
    with pytest.raises(ValueError, match="fp8"):
        dec.SharedKVCache(1, 1, 2, 1, 8, 8, 64, "cpu", dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="bf16"):
        generate(m, torch.zeros(1, 4, dtype=torch.int64), 2, samples=2, kv="fp8")
    with pytest.raises(ValueError, match="samples"):
        generate(m, torch.zeros(1, 4, dtype=torch.int64), 2, samples=0)
