"""Llama-family DP training payload (BASELINE configs #3 / #4 / #5):
TFJob/PyTorchJob Worker=N, one GPU per worker, RCCL over xGMI, fused HIP
kernels, AdamW -- the same step as bench.py (ZeRO-1 sharded optimizer for
N > 1 unless ``--zero 0``).  Every rank checkpoints its own optimizer shard
(train/sharded_ckpt.py, asynchronous) every `--checkpoint-every` steps and
on SIGTERM (preemption; the ranks agree on the stop step first) to
TOA_CHECKPOINT_DIR, and resumes from it on restart -- with ANY world size,
which is what the elastic policy relies on."""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from tf_operator_amd.examples.common import pick_device
from tf_operator_amd.train import dist as tdist
from tf_operator_amd.train import sharded_ckpt
from tf_operator_amd.train.data import SyntheticTokens
from tf_operator_amd.train.llm import LlamaTrainer, load_trainer_state, trainer_state
from tf_operator_amd.train.runtime import Runtime


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama-tiny")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--seq-len", type=int, default=128)
    p.add_argument("--micro-batch", type=int, default=2)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--checkpoint-every", type=int, default=0)
    p.add_argument("--step-sleep", type=float, default=0.0, help="testing: slow steps down")
    p.add_argument("--report-every", type=int, default=0, help="report samples/sec to the operator every N steps")
    p.add_argument("--fixed-batch", action="store_true", help="reuse one resident batch (benchmarking)")
    p.add_argument("--zero", choices=("auto", "0", "1"), default="auto",
                   help="ZeRO-1 sharded optimizer; auto = on for world > 1 (bench.py's default)")
    p.add_argument("--adam-state", choices=("fp32", "bf16"), default=None,
                   help="AdamW moment storage; bf16 = stochastically rounded, 4 B/parameter less state "
                        "(default: TOA_ADAM_STATE, else fp32)")
    p.add_argument("--zero-check", action="store_true", default=None,
                   help="raise on a weight read whose ZeRO-1 all-gather was not waited for (default: TOA_ZERO_CHECK)")
    p.add_argument("--skip-nonfinite", action="store_true", default=None,
                   help="skip the update of a step whose gradient norm is Inf or NaN, on the device; the log "
                        "line counts the skips (default: TOA_SKIP_NONFINITE)")
    p.add_argument("--skip-grad-norm", type=float, default=None, metavar="X",
                   help="with --skip-nonfinite: also skip a step whose gradient norm is above X "
                        "(default: TOA_SKIP_GRAD_NORM, else no limit)")
    p.add_argument("--doc-mask", action="store_true",
                   help="pack rows from documents ending with --eos-id and keep attention inside each document")
    p.add_argument("--eos-id", type=int, default=0, help="the end-of-document token id of --doc-mask")
    p.add_argument("--doc-len", dest="doc_len_arg", default="16:128", metavar="LO:HI",
                   help="document lengths of the synthetic stream under --doc-mask")
    p.add_argument("--sample-every", type=int, default=0, metavar="N",
                   help="every N steps rank 0 samples greedily from the start of its current batch (KV-cache "
                        "decoding) and prints one JSON line {\"sample\": {\"step\", \"tokens\"}}; 0 = never")
    p.add_argument("--sample-tokens", type=int, default=16, metavar="M", help="new tokens per sample")
    p.add_argument("--sample-prompt-len", type=int, default=8, metavar="P", help="prompt tokens per sample")
    p.add_argument("--sample-gemm", choices=["tile", "skinny"], default=None,
                   help="what runs the projections of a sample's decode steps: the training GEMMs (tile) or the "
                        "weight-streaming GEMM for 1 to 16 rows (skinny); default: TOA_DECODE_GEMM, else tile")
    p.add_argument("--sample-prefill-chunk", type=int, default=None, metavar="N",
                   help="prefill a sample's prompt N tokens at a time through the cache-extend kernels instead of all "
                        "at once through the training ops; default: all at once")
    p.add_argument("--sample-temperature", type=float, default=0.0, metavar="T",
                   help="temperature of a sample; 0 = greedy (the default)")
    p.add_argument("--sample-top-k", type=int, default=0, metavar="K", help="keep a sample's K likeliest tokens; 0 = all")
    p.add_argument("--sample-top-p", type=float, default=1.0, metavar="P",
                   help="nucleus filter of a sample, in (0, 1]; below 1 it needs --sample-sampler device")
    p.add_argument("--sample-min-p", type=float, default=0.0, metavar="P",
                   help="drop a sample's tokens below P times the mode's probability, in [0, 1); above 0 it needs "
                        "--sample-sampler device")
    p.add_argument("--sample-seed", type=int, default=0, metavar="S", help="seed of a sample's draws, 0 .. 2^32 - 1")
    p.add_argument("--sample-sampler", choices=["torch", "device"], default=None,
                   help="what picks a sample's tokens: library calls on one generator (torch) or the sampling kernel "
                        "(device); default: TOA_SAMPLER, else torch")
    a = p.parse_args(argv)
    if a.sample_every < 0 or a.sample_tokens < 1 or a.sample_prompt_len < 1:
        p.error("--sample-every needs N >= 0, --sample-tokens and --sample-prompt-len at least 1")
    if not (0.0 <= a.sample_temperature < float("inf")) or a.sample_top_k < 0:
        p.error("--sample-temperature needs a finite T >= 0, --sample-top-k needs K >= 0")
    if not 0.0 < a.sample_top_p <= 1.0 or not 0.0 <= a.sample_min_p < 1.0:
        p.error("--sample-top-p needs 0 < P <= 1, --sample-min-p needs 0 <= P < 1")
    if not 0 <= a.sample_seed < 1 << 32:
        p.error("--sample-seed needs 0 <= S < 2^32")
    if (a.sample_top_p < 1.0 or a.sample_min_p > 0.0) and a.sample_sampler == "torch":
        p.error("--sample-top-p and --sample-min-p need --sample-sampler device")
    if a.sample_prefill_chunk is not None and a.sample_prefill_chunk < 1:
        p.error("--sample-prefill-chunk needs N >= 1")
    if a.sample_every and a.sample_prompt_len > a.seq_len:
        p.error("--sample-prompt-len is longer than --seq-len")
    a.doc_len = None
    if a.doc_mask:
        try:
            lo, hi = (int(x) for x in a.doc_len_arg.split(":"))
        except ValueError:
            p.error("--doc-len takes LO:HI")
        if not 1 <= lo <= hi:
            p.error("--doc-len needs 1 <= LO <= HI")
        a.doc_len = (lo, hi)
    from tf_operator_amd.ops import gemm

    gemm.prewarm_early()  # GEMM plans resolve while the process group and the model come up
    rt = Runtime()
    rt.install_preemption_handler()
    info = rt.init_dist()
    rt.mark("dist_init")
    with rt.guard():
        _train(a, rt, info)


def _stop_agreed(rt, dev) -> bool:
    """True on every rank once ANY rank got SIGTERM (a MAX all-reduce of the
    flag), so all ranks stop -- and save -- after the same step."""
    flag = rt.preempted.is_set()
    if rt.world == 1 or not torch.distributed.is_initialized():
        return flag
    t = torch.tensor([1.0 if flag else 0.0], device=dev)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    return bool(t.item() > 0)


def _sample(a, tr, tokens):
    """One sample (greedy unless --sample-temperature is set) from the first
    --sample-prompt-len tokens of the batch's first row, as one JSON line on
    stdout.  It leaves the run as it was (LlamaTrainer.generate); the token
    list's copy to the host is the only synchronisation."""
    P = a.sample_prompt_len
    out, _ = tr.generate(tokens[:1, :P], a.sample_tokens, gemm=a.sample_gemm, prefill_chunk=a.sample_prefill_chunk,
                         temperature=a.sample_temperature, top_k=a.sample_top_k, top_p=a.sample_top_p,
                         min_p=a.sample_min_p, seed=a.sample_seed, sampler=a.sample_sampler)
    print(json.dumps({"sample": {"step": tr.step_idx, "tokens": out[0, P:].tolist()}}), flush=True)


def _train(a, rt, info):
    # gloo is the CPU plumbing backend, unless asked for explicitly
    # (TOA_DIST_BACKEND=gloo: replicas sharing one GPU, device tensors over gloo)
    dev = pick_device() if info.backend != "gloo" or os.environ.get("TOA_DIST_BACKEND") else torch.device("cpu")
    zero = rt.world > 1 if a.zero == "auto" else a.zero == "1"
    tr = LlamaTrainer(a.model, dev, micro_batch=a.micro_batch, seq_len=a.seq_len, lr=a.lr, shard_optimizer=zero,
                      adam_state=a.adam_state, zero_check=a.zero_check, doc_eos=a.eos_id if a.doc_mask else None,
                      skip_nonfinite=a.skip_nonfinite, skip_grad_norm=a.skip_grad_norm)
    rt.mark("model_init")
    tr.on_phase = rt.mark  # the first step's host-side issue points, in the start-up phases
    ck = sharded_ckpt.Checkpointer(rt.ckpt_dir, rt.rank, rt.world) if rt.ckpt_dir else None
    if ck is not None:
        ck.sync_attempt()  # markers of a crashed earlier attempt never commit this run's saves
    # a resumable stream: batch i of rank r is a function of (seed, r, i), so
    # the checkpointed cursor continues the uninterrupted run's data exactly
    data = SyntheticTokens(a.micro_batch, a.seq_len, tr.cfg.vocab_size, rank=rt.rank, device=dev,
                           fixed=a.fixed_batch, doc_len=a.doc_len, eos_id=a.eos_id if a.doc_mask else None)
    shares = sharded_ckpt.load_latest(rt.ckpt_dir)
    if shares is not None:
        load_trainer_state(tr, shares, data=data)  # re-shards a checkpoint of any world size
        rt.log(f"resumed at step {tr.step_idx} (world {rt.world}) from a world-{shares[0]['world']} checkpoint"
               f" at data cursor {data.cursor}")
        rt.mark("checkpoint_load")
    t0, n0 = time.perf_counter(), tr.step_idx
    while tr.step_idx < a.steps:
        batch = data.next()
        loss = tr.step([batch])
        if a.sample_every and tr.step_idx % a.sample_every == 0 and rt.rank == 0:
            _sample(a, tr, batch[0])
        if tr.step_idx == n0 + 1:
            if dev.type == "cuda":
                torch.cuda.synchronize()
            rt.first_step_done()
            t1 = time.perf_counter()
        if tr.step_idx % 5 == 0 or tr.step_idx == a.steps:
            # float(loss) synchronises already, so the skip count costs no further wait
            skipped = f" skipped {tr.skipped_steps()}" if tr.skip_nonfinite else ""
            rt.log(f"step {tr.step_idx} loss {float(loss):.4f}{skipped}")
        if a.report_every and (tr.step_idx - n0) % a.report_every == 0 and tr.step_idx > n0 + 1:
            # throughput since the first step of this generation (excludes start-up)
            if dev.type == "cuda":
                torch.cuda.synchronize()
            el = time.perf_counter() - t1
            rt.report(samples_per_sec=a.micro_batch * rt.world * (tr.step_idx - n0 - 1) / max(el, 1e-9),
                      step=tr.step_idx, world=rt.world)
        if ck and a.checkpoint_every and tr.step_idx % a.checkpoint_every == 0:
            ck.save(tr.step_idx, trainer_state(tr, data))  # every rank, its own shard; asynchronous
        if _stop_agreed(rt, dev):
            if ck:
                t_s = time.time()
                ck.save(tr.step_idx, trainer_state(tr, data), block=True)
                rt.log(f"preemption checkpoint at step {tr.step_idx} in {time.time() - t_s:.2f}s "
                       f"{ck.last_timing}")
            rt.log(f"preempted at step {tr.step_idx}")
            tdist.shutdown()
            raise SystemExit(143)
        if a.step_sleep:
            time.sleep(a.step_sleep)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    done = tr.step_idx - n0
    if done:
        rt.report(samples_per_sec=a.micro_batch * rt.world * done / dt)
    if ck:
        ck.save(tr.step_idx, trainer_state(tr, data), block=True)
    rt.log(f"done: {tr.step_idx} steps")


if __name__ == "__main__":
    main()
