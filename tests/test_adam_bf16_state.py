"""AdamW moments in bf16 with stochastic rounding (FlatAdamW state_dtype=bf16,
TOA_ADAM_STATE=bf16), the CPU tier: the rounding and its hash against their
definitions, unbiasedness where round-to-nearest stalls, checkpoints in both
moment formats and across them, and the sharded update against the
replicated one (CPU / gloo: both run the Python form of the algorithm the
kernels in csrc/hip/optim.hip implement)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tf_operator_amd.ops.optim import (FlatAdamW, adamw_reference, moment_to_bf16, sr_bf16_reference,
                                       sr_hash_reference)
from tf_operator_amd.parallel import zero
from tf_operator_amd.parallel.flat import FlatParams
from tf_operator_amd.train import sharded_ckpt
from tf_operator_amd.train.llm import LlamaTrainer, load_trainer_state, trainer_state

KEYS = ("master", "exp_avg", "exp_avg_sq")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32) if not isinstance(
        bits, int) else _f32([bits])


def _bits(bf):
    return (bf.view(torch.int16).to(torch.int64) & 0xFFFF).tolist()


def _sr(bits, r):
    b = torch.tensor([x - (1 << 32) if x >= 1 << 31 else x for x in bits], dtype=torch.int64).to(torch.int32)
    return _bits(sr_bf16_reference(b.view(torch.float32), torch.tensor(r, dtype=torch.int64)))


# ------------------------------------------------------------------ 1. the rounding and the hash
def test_sr_bf16_reference_matches_its_definition():
    rs = [0, 1, 0x7FFF, 0x8000, 0xFFFF]
    # exactly representable (low 16 bits zero): unchanged for every r -- 1.0, -2.5, +0, -0, the largest bf16
    for u in (0x3F800000, 0xC0200000, 0x00000000, 0x80000000, 0x7F7F0000):
        assert _sr([u] * len(rs), rs) == [u >> 16] * len(rs), hex(u)
    # exactly halfway between 1.0 and the next bf16: up for r >= 0x8000, down otherwise
    assert _sr([0x3F808000] * 4, [0, 0x7FFF, 0x8000, 0xFFFF]) == [0x3F80, 0x3F80, 0x3F81, 0x3F81]
    # a negative halfway value rounds away from zero on the same r (sign-magnitude bits)
    assert _sr([0xBF808000] * 4, [0, 0x7FFF, 0x8000, 0xFFFF]) == [0xBF80, 0xBF80, 0xBF81, 0xBF81]
    # a fraction f / 65536 above a bf16 goes up exactly when r >= 65536 - f
    assert _sr([0x40490FDB] * 3, [0, 0xF024, 0xF025]) == [0x4049, 0x4049, 0x404A]   # pi: f = 0x0FDB
    # a carry out of the mantissa lands on the next power of two
    assert _sr([0x3FFFFFFF], [1]) == [0x4000]
    # inf and NaN: never touched by r; a NaN whose payload sits in the dropped half stays a NaN
    assert _sr([0x7F800000, 0xFF800000] * 2, [0, 0, 0xFFFF, 0xFFFF]) == [0x7F80, 0xFF80] * 2
    for u in (0x7FC00000, 0x7F800001, 0xFF80FFFF):
        out = sr_bf16_reference(_f32([u - (1 << 32) if u >= 1 << 31 else u] * 2), torch.tensor([0, 0xFFFF]))
        assert bool(out.float().isnan().all()), hex(u)
    # the value the bits stand for
    assert float(sr_bf16_reference(torch.tensor([1.0 + 2.0 ** -8]), torch.tensor([0x8000]))) == 1.0 + 2.0 ** -7


def test_sr_hash_literals():
    """Three (seed, step, i) -> draw triples worked out with plain Python
    integers from the definition in docs/kernels.md: the Python and the C++
    copy of the hash cannot drift apart without one of them failing here
    (the GPU tests compare the kernels with the Python form)."""
    cases = [((0, 1, 0), 0xAA3E5B61), ((12345, 7, 1000003), 0x5AA43B06),
             ((0xDEADBEEF, 200, (1 << 32) + 5), 0xCD780DBB), ((1, 3, (5 << 32) | 0xFFFFFFF8), 0x1E7363E6)]
    for (seed, step, i), want in cases:
        assert int(sr_hash_reference(seed, step, torch.tensor([i], dtype=torch.int64))[0]) == want, (seed, step, i)
    idx = torch.tensor([c[0][2] for c in cases[:1]] * 2, dtype=torch.int64)
    assert sr_hash_reference(0, 1, idx).tolist() == [0xAA3E5B61] * 2   # a pure function of its inputs


# ------------------------------------------------------------------ 2. unbiased where round-to-nearest stalls
def test_bf16_v_is_unbiased_where_round_to_nearest_is_not():
    """2^20 elements, beta2 = 0.999, a constant gradient, 200 steps from zero,
    no clipping: the mean of the bf16 v is within 1e-3 (relative) of the
    fp32-state v = g^2 (1 - beta2^200).  Per element the accumulated rounding
    noise is about 2^-8 (1 - beta2^2)^-1/2 = 0.09 relative; over 2^20
    elements 1e-4, so 1e-3 is some ten standard deviations (the Python
    reference alone gives 1e-5 at this seed).

    The same update with torch's round-to-nearest ends more than 10 % low.
    How far off round-to-nearest ends depends on where v sits in its binade
    (-17 % .. +16 % over one octave of g^2); g = 1.26 puts the last ~80
    steps' increments at 1.3 bf16 steps, which round to 1."""
    n, b2, g, steps = 1 << 20, 0.999, 1.26, 200
    grad = torch.full((n,), g)
    master = torch.zeros(n)
    m = torch.zeros(n, dtype=torch.bfloat16)
    v = torch.zeros(n, dtype=torch.bfloat16)
    gs = torch.full((1,), g)      # round to nearest is the same for every element: one is enough
    vr = torch.zeros(1, dtype=torch.bfloat16)
    for s in range(1, steps + 1):
        adamw_reference(master, grad, m, v, lr=1e-3, beta1=0.9, beta2=b2, eps=1e-8, weight_decay=0.0, step=s,
                        base=0, seed=3)
        vr = vr.float().mul_(b2).addcmul_(gs, gs, value=1 - b2).to(torch.bfloat16)
    want = g * g * (1 - b2 ** steps)
    rel = float(v.double().mean()) / want - 1
    rel_rn = float(vr.double()) / want - 1
    print(f"stochastic {rel:+.2e}  round-to-nearest {rel_rn:+.2e}")
    assert abs(rel) < 1e-3
    assert rel_rn < -0.10
    assert len(torch.unique(v)) > 2    # the elements really draw different bits


# ------------------------------------------------------------------ FlatAdamW on CPU
def _flat(seed=0, n=(300, 77, 1000)):
    g = torch.Generator().manual_seed(seed)
    return FlatParams([torch.nn.Parameter(torch.randn(k, generator=g)) for k in n])


def test_state_dtype_argument():
    f = _flat()
    opt = FlatAdamW(f, state_dtype=torch.bfloat16, seed=5)
    assert f.exp_avg.dtype == f.exp_avg_sq.dtype == torch.bfloat16 and f.master.dtype == torch.float32
    assert f.exp_avg.numel() == f.state_numel and f.moment_dtype == torch.bfloat16
    assert opt.state_dict()["seed"] == 5 and opt.state_dict()["state_dtype"] == "bfloat16"
    assert FlatAdamW(_flat()).flat.exp_avg.dtype == torch.float32          # the default stays fp32
    assert FlatAdamW(_flat()).state_dict()["state_dtype"] == "float32"
    for bad in (torch.float16, "bf16", None):
        with pytest.raises(ValueError):
            FlatAdamW(_flat(), state_dtype=bad)


def test_existing_moments_are_converted_once():
    g = torch.Generator().manual_seed(1)
    f = _flat()
    f.exp_avg = torch.randn(f.numel, generator=g)
    f.exp_avg_sq = torch.rand(f.numel, generator=g)
    m32, v32 = f.exp_avg.clone(), f.exp_avg_sq.clone()
    f.shard_state([(64, 320), (448, f.numel)])     # compact storage: the hash still sees flat indices
    FlatAdamW(f, state_dtype=torch.bfloat16, seed=9, owned=[(64, 320), (448, f.numel)])
    for lo, hi in f.state_ranges:
        idx = torch.arange(lo, hi)
        h = sr_hash_reference(9, 0, idx)
        assert torch.equal(f.state_view(f.exp_avg, lo, hi), sr_bf16_reference(m32[lo:hi], h & 0xFFFF))
        assert torch.equal(f.state_view(f.exp_avg_sq, lo, hi), sr_bf16_reference(v32[lo:hi], h >> 16))
    mb = f.exp_avg.clone()
    FlatAdamW(f, state_dtype=torch.float32, owned=f.state_ranges)            # and back: exact
    assert f.exp_avg.dtype == torch.float32 and torch.equal(f.exp_avg, mb.float())


def test_cpu_step_does_not_depend_on_the_cut():
    """Whole-buffer update == the same update cut into owned ranges."""
    res = []
    for owned in (None, [(0, 128), (128, 512), (512, 1472)]):
        f = _flat()
        assert f.numel == 1472
        opt = FlatAdamW(f, lr=1e-2, state_dtype=torch.bfloat16, seed=11, owned=owned, max_grad_norm=0.0)
        g = torch.Generator().manual_seed(4)
        for _ in range(3):
            f.grad.copy_(torch.randn(f.numel, generator=g))
            opt.step()
        res.append([getattr(f, k).clone() for k in KEYS])
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. checkpoints under TOA_ADAM_STATE=bf16
def _full_state(tr, world):
    if world > 1:
        return zero.gather_full_state(tr.flat, world)
    return {k: getattr(tr.flat, k) for k in KEYS}


def _ckpt_worker(rank, world, port, root, phase, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      TOA_ADAM_STATE="bf16")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, lr=1e-3, seed=rank,
                          bucket_mb=0.01, shard_optimizer=world > 1)
        assert tr.adam_state == "bf16" and tr.flat.exp_avg.dtype == torch.bfloat16
        g = torch.Generator().manual_seed(7)
        batches = [(torch.randint(0, tr.cfg.vocab_size, (2, 33), generator=g)) for _ in range(2 * 6)]
        batches = [(b[:, :-1].contiguous(), b[:, 1:].contiguous()) for b in batches]
        mine = batches[rank::2]    # the world-2 split (a world-1 load does not train on)
        ck = sharded_ckpt.Checkpointer(root, rank, world)
        res = {}
        if phase == "save":
            for i in range(3):
                tr.step([mine[i]])
            ck.save(tr.step_idx, trainer_state(tr))
            at_save = {k: v.clone() for k, v in _full_state(tr, world).items()}
            res["cont"] = [float(tr.step([mine[3 + i]])) for i in range(2)]   # the uninterrupted run
            ck.wait()
            res["at_save"] = at_save
        else:
            load_trainer_state(tr, sharded_ckpt.load_latest(root))
            assert tr.step_idx == 3 and tr.flat.exp_avg.dtype == torch.bfloat16
            if world == 2:
                res["cont"] = [float(tr.step([mine[3 + i]])) for i in range(2)]
        res["state"] = {k: v.clone() for k, v in _full_state(tr, world).items()}
        res["param"] = tr.flat.param.float().clone()
        if rank == 0:
            torch.save(res, out)
    finally:
        dist.destroy_process_group()


def test_bf16_checkpoint_resume_and_reshard(tmp_path):
    """World 2, ZeRO-1, bf16 moments: 3 steps, an asynchronous save, 2 more
    steps.  A fresh world-2 job resumes and reproduces the 2 steps bit for
    bit (losses, master, m, v); the moment files are .bf16 and half the
    master's size; a world-1 job restores the identical state."""
    root = str(tmp_path / "ck")
    a, b, c = (str(tmp_path / f"{x}.pt") for x in "abc")
    mp.spawn(_ckpt_worker, args=(2, _free_port(), root, "save", a), nprocs=2, join=True)
    saved = torch.load(a, weights_only=True)
    d = sharded_ckpt.latest_dir(root)
    assert sorted(os.listdir(d)) == ["manifest.json"] + sorted(
        f"rank{r:05d}.{x}" for r in range(2) for x in ("exp_avg.bf16", "exp_avg_sq.bf16", "json", "master.f32"))
    for r in range(2):
        size = {k: os.path.getsize(os.path.join(d, f"rank{r:05d}.{k}")) for k in
                ("master.f32", "exp_avg.bf16", "exp_avg_sq.bf16")}
        assert size["master.f32"] > 0 and size["exp_avg.bf16"] * 2 == size["exp_avg_sq.bf16"] * 2 == size["master.f32"]
    shares = sharded_ckpt.load_latest(root)
    assert all(s["flat"]["exp_avg"].dtype == torch.bfloat16 and s["opt"]["state_dtype"] == "bfloat16" for s in shares)

    mp.spawn(_ckpt_worker, args=(2, _free_port(), root, "load", b), nprocs=2, join=True)
    resumed = torch.load(b, weights_only=True)
    assert resumed["cont"] == saved["cont"]
    for k in KEYS:
        assert resumed["state"][k].dtype == saved["state"][k].dtype
        assert torch.equal(resumed["state"][k], saved["state"][k]), k
    assert torch.equal(resumed["param"], saved["param"])
    assert float(saved["state"]["exp_avg_sq"].float().abs().max()) > 0

    mp.spawn(_ckpt_worker, args=(1, _free_port(), root, "load", c), nprocs=1, join=True)
    one = torch.load(c, weights_only=True)
    for k in KEYS:
        assert torch.equal(one["state"][k], saved["at_save"][k]), k
    assert torch.equal(one["param"], saved["at_save"]["master"].to(torch.bfloat16).float())


def _trained(adam_state, steps=2):
    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, lr=1e-3, seed=0,
                      adam_state=adam_state)
    for i in range(steps):
        tr.step([tr.synthetic_batch(seed=50 + i)])
    return tr


def test_checkpoints_cross_the_moment_dtype(tmp_path):
    """An fp32 checkpoint loads into a bf16 run (downcast = sr_bf16 of step 0
    at the flat index, whatever ranges the loader cuts) and a bf16 one into
    an fp32 run (exact upcast); master and step are untouched either way."""
    src = {}
    for st in ("fp32", "bf16"):
        tr = _trained(st)
        root = str(tmp_path / st)
        sharded_ckpt.Checkpointer(root).save(tr.step_idx, trainer_state(tr), block=True)
        src[st] = ({k: getattr(tr.flat, k).clone() for k in KEYS}, root)
    n = src["fp32"][0]["master"].numel()
    idx = torch.arange(n)

    ref, root = src["fp32"]
    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, seed=1, adam_state="bf16")
    load_trainer_state(tr, sharded_ckpt.load_latest(root))
    h = sr_hash_reference(0, 0, idx)
    assert tr.flat.exp_avg.dtype == torch.bfloat16 and tr.step_idx == 2
    assert torch.equal(tr.flat.master, ref["master"])
    assert torch.equal(tr.flat.exp_avg, sr_bf16_reference(ref["exp_avg"], h & 0xFFFF))
    assert torch.equal(tr.flat.exp_avg_sq, sr_bf16_reference(ref["exp_avg_sq"], h >> 16))
    assert torch.equal(tr.flat.exp_avg, moment_to_bf16(ref["exp_avg"], "exp_avg", 0, 0))
    # sharded restore of the same checkpoint: the same bits in every range
    cut = n // 2 // 64 * 64
    for rg in ([(0, cut)], [(64, 128), (cut, n)]):
        h2 = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, seed=2,
                          adam_state="bf16").flat
        h2.shard_state(rg)
        h2.load_state_shards([s["flat"] for s in sharded_ckpt.load_latest(root)], set_params="held")
        for lo, hi in rg:
            assert torch.equal(h2.state_view(h2.exp_avg, lo, hi), tr.flat.exp_avg[lo:hi]), (lo, hi)
            assert torch.equal(h2.state_view(h2.exp_avg_sq, lo, hi), tr.flat.exp_avg_sq[lo:hi]), (lo, hi)
    tr.step([tr.synthetic_batch(seed=60)])           # and it trains on

    ref, root = src["bf16"]
    tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, seed=1, adam_state="fp32")
    load_trainer_state(tr, sharded_ckpt.load_latest(root))
    assert tr.flat.exp_avg.dtype == torch.float32 and tr.step_idx == 2
    assert torch.equal(tr.flat.master, ref["master"])
    assert torch.equal(tr.flat.exp_avg, ref["exp_avg"].float())
    assert torch.equal(tr.flat.exp_avg_sq, ref["exp_avg_sq"].float())
    tr.step([tr.synthetic_batch(seed=60)])


def test_adam_state_argument_and_environment(monkeypatch):
    with pytest.raises(ValueError):
        LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=16, adam_state="fp16")
    monkeypatch.setenv("TOA_ADAM_STATE", "half")
    with pytest.raises(ValueError):
        LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=16)
    monkeypatch.setenv("TOA_ADAM_STATE", "bf16")
    assert LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=16).flat.exp_avg.dtype == torch.bfloat16
    monkeypatch.delenv("TOA_ADAM_STATE")
    assert LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=1, seq_len=16).flat.exp_avg.dtype == torch.float32


# ------------------------------------------------------------------ 4. sharded equals replicated
def _zero_worker(rank, world, port, bucket_mb, steps, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        for shard in (False, True):
            tr = LlamaTrainer("llama-tiny", torch.device("cpu"), micro_batch=2, seq_len=32, lr=1e-3, seed=rank,
                              bucket_mb=bucket_mb, shard_optimizer=shard, transposed_weights=shard,
                              adam_state="bf16")
            assert tr.bucketer.shard == shard and tr.flat.exp_avg.dtype == torch.bfloat16
            # clipping off in both arms: the sharded norm is a sum of per-shard sums, the replicated
            # one a single sum over the buffer -- they differ in the last fp32 bit whatever the
            # moments' format (why tests/test_parallel.py compares these two with a tolerance)
            tr.opt.max_grad_norm = 0.0
            batches = [tr.synthetic_batch(seed=100 + i) for i in range(world)]
            losses = [float(tr.step([batches[rank]])) for _ in range(steps)]
            if shard:
                assert tr.flat.exp_avg.numel() * world == tr.flat.numel
            full = _full_state(tr, world if shard else 1)
            res[shard] = (losses, tr.flat.param.detach().float().clone(), {k: full[k].clone() for k in KEYS})
        if rank == 0:
            torch.save(res, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,bucket_mb", [(2, 0.01), (4, 512)])
def test_sharded_bf16_update_matches_replicated(tmp_path, world, bucket_mb):
    """ZeRO-1 with bf16 moments against the replicated update, 3 steps:
    master, m and v bit-identical (both run the Python form; the rounding
    bits are keyed by the flat index, not by the position in a shard)."""
    out = str(tmp_path / "zero.pt")
    mp.spawn(_zero_worker, args=(world, _free_port(), bucket_mb, 3, out), nprocs=world, join=True)
    r = torch.load(out, weights_only=True)
    (l0, p0, s0), (l1, p1, s1) = r[False], r[True]
    for k in KEYS:
        assert s0[k].dtype == s1[k].dtype and torch.equal(s0[k], s1[k]), k
    assert torch.equal(p0, p1) and l0 == l1
