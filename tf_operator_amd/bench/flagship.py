"""The headline benchmark: "samples/sec (N-worker TFJob) + p50 submit->first-step
latency at 1/2/4/8 GPUs" (BASELINE.json) on config #3, TFJob Worker=N
all-reduce Llama-3-8B bf16 over RCCL/xGMI, one GPU per worker.

Three ways in, one measurement:

* **launcher** (``python bench.py --gpus N``, no ``WORLD_SIZE`` in the env):
  the whole operator stack runs in this process -- fake API server, the
  operator (C++ reconcile core), local kubelet with node-visible devices --
  and the benchmark is SUBMITTED as a ``TFJob`` with ``Worker=N`` whose
  replicas run :func:`run_replica`.  Before it, under ``--full``, ``--latency-probes`` TFJobs
  running the user-facing ``examples/llama_train`` payload for one step are
  submitted and timed from ``create()`` to rank 0's first completed
  optimizer step (reported back to the operator).  This process never
  touches the GPU.
* **torchrun** (the driver's N > 1 launch: ``WORLD_SIZE`` set by the
  elastic agent): every rank runs :func:`run_replica` directly.  Under ``--full``, before any
  rank touches a GPU, rank 0 runs the same latency probes (TFJob Worker=N
  through a local operator stack) while the other ranks wait on the agent's
  store.
* **replica** (an operator-launched worker, or ``--direct``): just the
  timed steps.

The replica: W untimed warm-up steps, then exactly K steps bracketed by a
barrier + ``torch.cuda.synchronize()`` on both sides, MAX over ranks; full
forward + backward + gradient reduce-scatter/all-reduce + AdamW.  Rank 0
builds the one JSON line; ``n_gpus`` is the size of the initialised RCCL
process group, and the run fails when it differs from ``--gpus``.

A plain run does only that: set up, warm up, time the K steps, write the
last step's outputs when ``--dump-outputs DIR`` is given, print the line.
Everything else the benchmark measures -- the latency probes (warm and
cold), the box-speed calibration GEMMs and clock sampling, RCCL's transport
record and the collectives A/B -- runs under ``--full`` only.

Reference: the metric's 8-worker job is
``examples/v1/distribution_strategy/keras-API/multi_worker_strategy-with-keras.py:76-77``
(MultiWorkerMirroredStrategy, NCCL all-reduce), submitted as the TFJob of
``multi_worker_tfjob.yaml``.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import statistics
import sys
import tempfile
import time

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BENCH_PY = os.path.join(REPO_ROOT, "bench.py")
METRIC = "samples/sec ({n}-worker TFJob)"


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--micro-batch", type=int, default=6)  # 243 GiB peak of 288 GB at N=1
    ap.add_argument("--grad-accum", type=int, default=1)
    ap.add_argument("--bucket-mb", type=float, default=None)
    ap.add_argument("--zero", choices=("auto", "0", "1"), default="auto",
                    help="sharded optimizer (reduce-scatter / owned-shard AdamW / all-gather); auto = on for N > 1")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the submit -> first-step latency "
                         "probes, the box-speed calibration, RCCL's transport record and the collectives A/B "
                         "(each with its own option below; without --full they are all off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps rank 0 writes what the last timed step computed as DIR/<name>.npy "
                         "(float32): the loss, and a fixed seeded sample of the updated parameters and of the "
                         "gradients")
    ap.add_argument("--latency-probes", type=int, default=None,
                    help="TFJobs submitted (and timed submit -> first step) before the throughput run; 0 = skip "
                         "(--full: default 3)")
    ap.add_argument("--cold-probes", type=int, default=None,
                    help="extra probe TFJobs whose replicas start as cold processes (a real kubelet's start), "
                         "reported as submit_to_first_step_cold_p50_s; 0 = skip (--full: default 2)")
    ap.add_argument("--probe-timeout", type=float, default=180.0, help="per probe job (s)")
    ap.add_argument("--warm-start", choices=("0", "1"), default="1",
                    help="replicas start as forks of the local kubelet's warm interpreter (torch pre-imported, "
                         "no GPU touched); 0 = a cold python process per replica")
    ap.add_argument("--direct", action="store_true",
                    help="run the replica in this process (no operator; for profilers)")
    ap.add_argument("--result-file", default=None, help=argparse.SUPPRESS)  # replica -> launcher
    ap.add_argument("--rccl-log", choices=("auto", "0", "1"), default=None,
                    help="capture RCCL's transport selection (NCCL_DEBUG=INFO to a file) into the JSON line "
                         "(--full: default auto)")
    ap.add_argument("--calibrate", choices=("0", "1"), default=None,
                    help="box-speed record: fixed-shape GEMM rates around the timed region, clock during it "
                         "(--full: default 1)")
    ap.add_argument("--collectives-ab", choices=("auto", "0", "1"), default=None,
                    help="after the timed region, time the ZeRO-1 collectives on RCCL and on the copy engines "
                         "(copy-engine pulls) in alternating windows of the same process group; auto = on for "
                         "a sharded one-node GPU job with N > 1 (--full: default auto)")
    ap.add_argument("--ab-steps", type=int, default=3, help="timed steps per collectives A/B window")
    return ap


# what only a --full run does: option -> (its default under --full, its "off" value)
FULL_ONLY = {"latency_probes": (3, 0), "cold_probes": (2, 0), "rccl_log": ("auto", "0"), "calibrate": ("1", "0"),
             "collectives_ab": ("auto", "0")}


def resolve_full(args, ap: argparse.ArgumentParser | None = None):
    """A plain run measures the headline figure and nothing else: every
    FULL_ONLY option is off, and asking for one without --full is an error
    (not a silently smaller run).  Under --full each takes its default."""
    for name, (dflt, off) in FULL_ONLY.items():
        v = getattr(args, name)
        if args.full:
            setattr(args, name, dflt if v is None else v)
        elif v is not None and v != off:
            msg = f"--{name.replace('_', '-')} {v} needs --full"
            if ap is None:
                raise ValueError(msg)
            ap.error(msg)
        else:
            setattr(args, name, off)
    return args


def mode() -> str:
    if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return "torchrun" if os.environ.get("TORCHELASTIC_RUN_ID") else "replica"
    return "launcher"


def main(argv=None, t_proc_start=None) -> int:
    ap = parser()
    args = resolve_full(ap.parse_args(argv), ap)
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    t_proc_start = t_proc_start or time.time()
    m = "replica" if args.direct else mode()
    if m == "launcher":
        return run_launcher(args)
    probe, t_probes_done = None, None
    if m == "torchrun" and args.latency_probes > 0:
        probe = _torchrun_probe_phase(args)
        t_probes_done = time.time()
    return run_replica(args, t_proc_start, probe=probe, launched_by=m, t_probes_done=t_probes_done)


# =============================================================================
# submit -> first-step latency probes (through the operator)
# =============================================================================
def _payload(args) -> list[str]:
    return [sys.executable, "-m", "tf_operator_amd.examples.llama_train", "--model", args.model, "--steps", "1",
            "--seq-len", str(args.seq_len), "--micro-batch", str(args.micro_batch)]


def _tfjob(name: str, n: int, command: list[str], env: dict | None = None, cold: bool = False) -> dict:
    from ..sdk import container, pod_template

    tpl = pod_template(container(image="toa/trainer:latest", command=command, gpus=1,
                                 env={"OMP_NUM_THREADS": "8", **(env or {})}))
    if cold:  # local kubelet: start this pod's replicas as fresh processes, not warm forks
        tpl.setdefault("metadata", {}).setdefault("annotations", {})["training.amd.com/start"] = "cold"
    # node-local xGMI layout (csrc/core/nodelocal.cc): the ranks share one
    # node, see each other's GPUs and get LOCAL_RANK / LOCAL_WORLD_SIZE of it
    return {"apiVersion": "kubeflow.org/v1", "kind": "TFJob",
            "metadata": {"name": name, "namespace": "default",
                         "annotations": {"amd.com/node-local": "privileged"}},
            "spec": {"runPolicy": {"cleanPodPolicy": "All"},
                     "tfReplicaSpecs": {"Worker": {"replicas": n, "restartPolicy": "Never", "template": tpl}}}}


def _pod_log_tail(c, name: str, n: int = 40) -> str:
    out = []
    for p in sorted(glob.glob(os.path.join(c.workdir, "pods", "default", name + "-*", "*.log"))):
        try:
            with open(p, errors="replace") as f:
                lines = f.read().splitlines()[-n:]
        except OSError:
            continue
        out.append(f"---- {os.path.relpath(p, c.workdir)}\n" + "\n".join(lines))
    return "\n".join(out)


def _own_vram_counters() -> list[str]:
    """sysfs VRAM counters of the GPUs this process can open: sysfs lists
    every card of the host (other tenants' too), /dev/dri only ours."""
    from ..utils.gpu_metrics import accessible_devices

    own = accessible_devices()
    return [p for p in sorted(glob.glob("/sys/class/drm/card*/device/mem_info_vram_used"))
            if os.path.realpath(os.path.dirname(p)) in own]


def vram_used_bytes() -> int | None:
    """HBM in use on the node's GPUs that this process can access, from the
    amdgpu driver's sysfs counters (no HIP call: the launcher never
    initialises a GPU)."""
    tot, seen = 0, False
    for p in _own_vram_counters():
        try:
            with open(p) as f:
                tot += int(f.read())
            seen = True
        except (OSError, ValueError):
            pass
    return tot if seen else None


def wait_vram_drained(baseline: int | None, timeout: float = 60.0, slack: int = 4 << 30) -> float:
    """After a job's processes exit the driver still scrubs their HBM (about
    33 GB/s on MI355X: ~7 s for a 243 GB Llama-3-8B replica), and a job
    started meanwhile waits for that memory.  Each latency probe starts on a
    drained node; the drain time is reported (``node_drain_s``)."""
    if baseline is None:
        return 0.0
    t0 = time.monotonic()
    while time.monotonic() - t0 < timeout:
        u = vram_used_bytes()
        if u is None or u <= baseline + slack:
            break
        time.sleep(0.05)
    return round(time.monotonic() - t0, 3)


def wait_vram_settled(timeout: float = 120.0, window: float = 2.0, tol: int = 1 << 30) -> float:
    """Block until the node's VRAM counter has stopped falling (moved less
    than `tol` over the last `window` seconds) and return the seconds waited.
    A node can still be scrubbing the HBM of a job that ended just before
    (the previous benchmark run, or whatever used the GPU before this one):
    a drain baseline taken then would be too high, and every later drain
    wait would end early."""
    t0 = time.monotonic()
    hist = []
    while time.monotonic() - t0 < timeout:
        u = vram_used_bytes()
        if u is None:
            return 0.0
        now = time.monotonic()
        hist = [(t, v) for t, v in hist if now - t <= window] + [(now, u)]
        if now - t0 >= window and max(v for _, v in hist) - min(v for _, v in hist) < tol:
            break
        time.sleep(0.05)
    return round(time.monotonic() - t0, 3)


def _run_job(c, name: str, n: int, command: list[str], timeout: float, env=None,
             vram_baseline: int | None = None, cold: bool = False) -> dict:
    """Submit one TFJob Worker=n, wait for it to succeed; return the client
    clock from create() to rank 0's first step plus the breakdown."""
    key = ("default", name)
    t0 = time.time()
    c.client.create(_tfjob(name, n, command, env, cold=cold))
    t_pods = c.wait(lambda: len(c.pods(labels={"job-name": name})) >= n and time.time(), timeout, 0.005,
                    f"{name}: pods created")

    def spawned():
        ts = [v[0] for k, v in c.kubelet.start_times.items() if k[1].startswith(name + "-")]
        return max(ts) if len(ts) >= n else None

    t_spawn = c.wait(spawned, timeout, 0.005, f"{name}: processes spawned")
    deadline = time.monotonic() + timeout
    rep = None
    while time.monotonic() < deadline:
        rep = c.controller.reports.get(key) or {}
        if rep.get("first_step_time"):
            break
        job = c.client.get(name)
        conds = {x["type"] for x in (job.get("status") or {}).get("conditions") or [] if x.get("status") == "True"}
        if "Failed" in conds:
            raise RuntimeError(f"{name} failed before its first step\n{_pod_log_tail(c, name)}")
        time.sleep(0.01)
    else:
        raise TimeoutError(f"{name}: no first step within {timeout:.0f}s\n{_pod_log_tail(c, name)}")
    job = c.client.wait_for_job(name, polling_interval=0.2, timeout_seconds=timeout)
    conds = {x["type"] for x in (job.get("status") or {}).get("conditions") or [] if x.get("status") == "True"}
    if "Succeeded" not in conds:
        raise RuntimeError(f"{name} did not succeed: {sorted(conds)}\n{_pod_log_tail(c, name)}")
    logs = _pod_log_tail(c, name, 400)
    c.client.delete(name)
    # every replica process has exited (and released its HBM) before the next job
    c.wait(lambda: not c.pods(labels={"job-name": name}) and not any(
        k[1].startswith(name + "-") for k in c.kubelet.running), 120, 0.05, f"{name}: cleanup")
    drain_s = wait_vram_drained(vram_baseline)
    t_first = float(rep["first_step_time"])
    return {"submit_to_first_step_s": round(t_first - t0, 4), "node_drain_s": drain_s,
            "submit_to_pods_created_s": round(t_pods - t0, 4),
            "submit_to_processes_spawned_s": round(t_spawn - t0, 4),
            "spawn_to_first_step_s": round(t_first - t_spawn, 4),
            "replica_phases_s": rep.get("phases") or {}, "_logs": logs}


def _cleanup_after_failure(c, name: str, vram_baseline: int | None):
    """A failed probe job: delete it and wait until its processes are gone and
    the node's HBM is scrubbed, so the next job (the benchmark itself) does
    not start on a node still draining (profiles/r4_fresh2: 5.6 s of
    dist_init -> model_init behind a failed probe)."""
    try:
        c.client.delete(name)
        c.wait(lambda: not c.pods(labels={"job-name": name}) and not any(
            k[1].startswith(name + "-") for k in c.kubelet.running), 120, 0.05, f"{name}: cleanup")
        wait_vram_drained(vram_baseline)
    except Exception as e:  # noqa: BLE001
        print(f"[bench] cleanup after {name}: {type(e).__name__}: {e}", file=sys.stderr, flush=True)


def _summary(samples: list[dict]) -> dict:
    if not samples:
        return {}
    tot = [s["submit_to_first_step_s"] for s in samples]

    def med(k):
        return round(statistics.median(s[k] for s in samples), 4)

    phases = {}
    for k in samples[0]["replica_phases_s"]:
        if all(k in s["replica_phases_s"] for s in samples):
            phases[k] = round(statistics.median(s["replica_phases_s"][k] for s in samples), 4)
    return {"p50_s": round(statistics.median(tot), 4), "samples_s": tot, "min_s": min(tot), "max_s": max(tot),
            "breakdown_p50_s": {"submit_to_pods_created": med("submit_to_pods_created_s"),
                                "submit_to_processes_spawned": med("submit_to_processes_spawned_s"),
                                "spawn_to_first_step": med("spawn_to_first_step_s"),
                                "node_drain_after_job": med("node_drain_s"),
                                "replica_phases": phases}}


def _cluster(n: int, warm: bool = False):
    """Started local cluster; with warm start, returned once the kubelet's fork
    server has imported torch (a job submitted earlier would start cold)."""
    from ..testing.cluster import LocalCluster

    c = LocalCluster(gpus=n, grace_seconds=10.0, threadiness=2, warm_python=warm).start()
    if warm:
        try:
            c.wait(c.kubelet.warm_ready, 120, 0.05, "kubelet fork server ready")
        except TimeoutError:  # the kubelet starts replicas cold instead
            print("[bench] kubelet fork server not ready: replicas start cold", file=sys.stderr, flush=True)
    return c


def _start_mode(c) -> str:
    return "warm fork (torch pre-imported)" if c.kubelet.warm_ready() else "cold process"


def probe_latency(args, n: int, c=None) -> dict:
    """`args.latency_probes` TFJob Worker=n submissions of the llama_train
    payload (one optimizer step each), sequentially."""
    own = c is None
    if own:
        c = _cluster(n, args.warm_start == "1")
    samples, cold, err = [], [], None
    # the node's trainer image is "pulled" (page cache warm, the local
    # kubelet's pagecache.py) before jobs are timed, as on a real node
    t_w = time.monotonic()
    try:
        c.wait(c.kubelet.node_warm, 180, 0.05, "node page cache warm")
    except TimeoutError:
        print("[bench] page-cache warmer still running: probes start anyway", file=sys.stderr, flush=True)
    warm_s = round(time.monotonic() - t_w, 3)
    settle_s = wait_vram_settled()  # a clean drain baseline
    base = vram_used_bytes()
    start_mode = _start_mode(c)
    plan = [(f"probe-{i}", False, samples) for i in range(args.latency_probes)]
    plan += [(f"probe-cold-{i}", True, cold) for i in range(getattr(args, "cold_probes", 0))]
    try:
        for name, is_cold, into in plan:
            try:
                s = _run_job(c, name, n, _payload(args), args.probe_timeout, vram_baseline=base, cold=is_cold)
            except Exception as e:  # keep the throughput run alive; report why latency is missing
                err = f"{type(e).__name__}: {str(e)[:2000]}"
                _cleanup_after_failure(c, name, base)
                break
            s.pop("_logs", None)
            s["replica_start"] = "cold process" if is_cold else start_mode
            into.append(s)
            print(f"[bench] {name}: submit->first-step {s['submit_to_first_step_s']:.3f}s", file=sys.stderr,
                  flush=True)
    finally:
        if own:
            c.stop()
    out = _summary(samples)
    out["_raw"] = samples
    out["_cold"] = cold
    out["replica_start"] = start_mode
    out["node_settle_before_probes_s"] = settle_s
    out["node_warm_wait_s"] = warm_s
    if err:
        out["error"] = err
    return out


def _probe_record(s: dict) -> dict:
    """One probe's breakdown for the JSON line (the clock and every phase)."""
    keep = ("submit_to_first_step_s", "submit_to_pods_created_s", "submit_to_processes_spawned_s",
            "spawn_to_first_step_s", "node_drain_s", "replica_phases_s", "replica_start")
    return {k: s[k] for k in keep if k in s}


def _torchrun_probe_phase(args) -> dict | None:
    """Rank 0 runs the probes while the other ranks wait on the elastic
    agent's store -- before any rank has initialised a GPU."""
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    key = f"toa_bench/{os.environ.get('TORCHELASTIC_RUN_ID', 'x')}/{os.environ.get('TORCHELASTIC_RESTART_COUNT', '0')}"
    budget = args.latency_probes * args.probe_timeout + 120
    try:
        store = dist.TCPStore(os.environ.get("MASTER_ADDR", "127.0.0.1"), int(os.environ["MASTER_PORT"]),
                              world_size=None, is_master=False, timeout=__import__("datetime").timedelta(
                                  seconds=budget), wait_for_workers=False)
    except Exception as e:  # no agent store to sync on: skip rather than race the GPUs
        if rank == 0:
            print(f"[bench] latency probes skipped: {e}", file=sys.stderr)
        return {"error": f"no agent store: {e}"}
    if rank == 0:
        try:
            res = probe_latency(args, world)
        finally:
            store.set(key, "done")
        return res
    store.wait([key])
    return None


# =============================================================================
# replica: the timed training steps
# =============================================================================
def _rccl_log_setup(args, launched_by: str):
    """RCCL writes its transport choice per channel at INFO level; send it to
    a per-process file (never to stdout, which carries the JSON line)."""
    want = args.rccl_log == "1" or (args.rccl_log == "auto" and int(os.environ.get("WORLD_SIZE", "1")) > 1)
    if not want or os.environ.get("NCCL_DEBUG"):
        return None
    d = os.environ.get("TOA_BENCH_RCCL_DIR") or os.path.join(tempfile.gettempdir(), "toa_rccl_logs")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"rccl.{os.getpid()}.log")
    os.environ["NCCL_DEBUG"] = "INFO"
    os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,P2P"
    os.environ["NCCL_DEBUG_FILE"] = path
    return path


def summarize_rccl_log(path: str | None) -> dict | None:
    """Count channel connections per transport (P2P/IPC, SHM, NET...) from an
    RCCL INFO log."""
    if not path or not os.path.exists(path):
        return None
    import re

    trans, ver, nch = {}, None, None
    with open(path, errors="replace") as f:
        for line in f:
            m = re.search(r"via (\S+)", line)
            if m and "Channel" in line:
                t = m.group(1)
                trans[t] = trans.get(t, 0) + 1
            m = re.search(r"(?:RCCL|NCCL) version (\S+)", line)
            if m:
                ver = m.group(1)
            m = re.search(r"(\d+) coll channels", line)
            if m:
                nch = int(m.group(1))
    return {"version": ver, "channel_connections_by_transport": trans, "coll_channels": nch, "log": path}


def transport_ok(summary: dict | None, n_ranks: int):
    """True when every RCCL channel connection of this one-node job is P2P
    (P2P/IPC, P2P/direct pointer, ...), False when any went SHM / NET, None
    when unknown (no log, a single rank, or no channels parsed)."""
    if not summary or n_ranks <= 1:
        return None
    trans = summary.get("channel_connections_by_transport") or {}
    if not trans:
        return None
    return all(t.upper().startswith("P2P") for t in trans)


def collectives_ab(tr, batches, args, info, rccl_ok) -> dict:
    """Time the two ZeRO-1 collective transports in the same process group,
    after the headline measurement (which stays on the configured default):
    windows in ABBA order -- the default, the other, the other, the default
    -- each one untimed step after the switch and ``--ab-steps`` timed steps
    bracketed by a barrier + synchronize, MAX over ranks.  The switch
    (``LlamaTrainer.set_collective_transport``) drains and barriers, so no
    pull crosses a window.  Returns {rccl_ms, sdma_ms, windows, ...} or
    {skipped: reason} / {error: ...}; never raises."""
    import torch

    from ..train import dist as tdist

    world = info.world
    want = args.collectives_ab == "1" or (args.collectives_ab == "auto" and world > 1)
    if not want:
        return {"skipped": "off (--collectives-ab 0, or N = 1)"}
    if tr.gather is None:
        return {"skipped": "ZeRO-1 off: no sharded collectives"}
    if info.device.type != "cuda":
        return {"skipped": "copy-engine pulls need GPUs (this run has none)"}
    if int(os.environ.get("LOCAL_WORLD_SIZE", "0")) != world:
        return {"skipped": "ranks span nodes (LOCAL_WORLD_SIZE != world): no IPC pulls"}
    if rccl_ok is False:
        return {"skipped": "RCCL channels are not all P2P: the ranks cannot reach each other's GPUs"}
    default = tr.collective_transport()
    other = "sdma" if default == "rccl" else "rccl"
    k = max(1, args.ab_steps)
    times = {"rccl": [], "sdma": []}
    windows = []
    # TOA_AB_INJECT_SIGNAL=<rank>:<signal number>:<window>: that rank sends
    # itself the signal as that window starts (rehearses the last-line path)
    inj = [int(x) for x in os.environ.get("TOA_AB_INJECT_SIGNAL", "-1:0:0").split(":")]
    try:
        for w, arm in enumerate((default, other, other, default)):
            if inj[0] == info.rank and inj[2] == w:
                sys.stdout.flush()
                os.kill(os.getpid(), inj[1])
            tr.set_collective_transport(arm)
            tr.step(batches)                      # the first step after a switch is not timed
            tdist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                tr.step(batches)
            torch.cuda.synchronize()
            tdist.barrier()
            torch.cuda.synchronize()
            dt = tdist.all_max(time.perf_counter() - t0, info.device)
            times[arm].append(dt / k * 1e3)
            windows.append({"transport": arm, "ms_per_step": round(dt / k * 1e3, 2)})
        tr.set_collective_transport(default)
        if tr.gather is not None:
            tr.gather.wait_all()
        for x in tr._pull_transports():
            x.check()                             # a timed-out peer wait would have poisoned the sdma windows
    except Exception as e:  # noqa: BLE001 - the headline measurement stands; the A/B reports its failure
        return {"error": f"{type(e).__name__}: {str(e)[:500]}", "windows": windows}
    out = {"default": default, "steps_per_window": k, "windows": windows,
           "rccl_ms": round(statistics.median(times["rccl"]), 2), "sdma_ms": round(statistics.median(times["sdma"]), 2)}
    out["faster"] = "sdma" if out["sdma_ms"] < out["rccl_ms"] else "rccl"
    return out


DUMP_SAMPLE = 8 << 20   # parameters sampled by --dump-outputs: 32 MiB of float32


def dump_outputs(path: str, tr, loss) -> dict:
    """What the last timed step handed its caller, as float32 ``.npy`` files
    under `path`: ``loss`` (the step's return value) and ``params`` (the flat
    parameter buffer after the update; above DUMP_SAMPLE elements a fixed,
    seeded sample of its positions, in ascending order).  Returns
    {name: shape}."""
    import numpy as np
    import torch

    os.makedirs(path, exist_ok=True)
    p = tr.flat.param.detach()
    if p.numel() > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(20240229).integers(0, p.numel(), DUMP_SAMPLE, dtype=np.int64))
        p = p.index_select(0, torch.from_numpy(idx).to(p.device))
    arrays = {"loss": np.asarray([float(loss)], dtype=np.float32),
              "params": p.float().cpu().numpy()}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def _ab_watchdog(budget_s: float, emit, code: int = 0):
    """A hung A/B window (a stalled copy-engine pull, a collective that never
    completes) or teardown must not cost the headline line: after `budget_s`
    rank 0 emits what it has (once) and every rank leaves with `code`."""
    import threading

    def fire():
        try:
            emit()
        finally:
            sys.stdout.flush()
            os._exit(code)

    t = threading.Timer(budget_s, fire)
    t.daemon = True
    t.start()
    return t



def run_replica(args, t_proc_start: float, probe: dict | None = None, launched_by: str = "replica",
                t_probes_done: float | None = None) -> int:
    """t_probes_done: under torchrun rank 0 ran the latency probes before
    this replica started its own work; that phase is reported on its own
    (``startup_phases_s["process_start->probes_done"]``) and the replica's
    first_step_s is counted from its end."""
    phases = {"process_start": t_proc_start}
    if t_probes_done is not None:
        phases["probes_done"] = t_probes_done
    rccl_log = _rccl_log_setup(args, launched_by)
    # the RCCL defaults the operator injects into every trainer pod
    # (csrc/core/envgen.cc kRcclDefaults), also under torchrun: collective
    # streams at high priority so the bucketed reduce-scatter / all-gather are
    # not queued behind the GEMMs they overlap
    for k, v in (("TORCH_NCCL_HIGH_PRIORITY", "1"), ("TORCH_NCCL_AVOID_RECORD_STREAMS", "1")):
        os.environ.setdefault(k, v)
    import torch

    from ..train import dist as tdist
    from ..train.llm import LlamaTrainer
    from ..train.runtime import Runtime
    from .calibrate import Calibration

    phases["imports"] = time.time()
    from ..ops import gemm as _gemm

    _gemm.prewarm_early()  # GEMM plans resolve while the process group and the model come up
    rt = Runtime()
    info = tdist.init()
    rt.info = info
    rt.mark("dist_init")
    phases["dist_init"] = time.time()
    import torch.distributed as dist

    rccl_world = dist.get_world_size() if dist.is_initialized() else 1
    backend = dist.get_backend() if dist.is_initialized() else None
    n_gpus = info.world
    dev = info.device
    if n_gpus != args.gpus or rccl_world != args.gpus:
        if info.rank == 0:
            print(f"[bench] FATAL: --gpus {args.gpus} but the process group has {rccl_world} ranks "
                  f"(WORLD_SIZE={n_gpus})", file=sys.stderr, flush=True)
        tdist.shutdown()
        return 3
    torch.manual_seed(0)
    zero = n_gpus > 1 if args.zero == "auto" else args.zero == "1"
    tr = LlamaTrainer(args.model, dev, micro_batch=args.micro_batch, seq_len=args.seq_len,
                      grad_accum=args.grad_accum, bucket_mb=args.bucket_mb, shard_optimizer=zero)
    batches = [tr.synthetic_batch(seed=1000 + info.rank * 97 + i) for i in range(args.grad_accum)]
    if dev.type == "cuda":
        torch.cuda.synchronize()
    rt.mark("model_init")
    phases["model_init"] = time.time()

    loss = tr.step(batches)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    phases["first_step"] = time.time()
    rt.first_step_done()  # -> operator (TFJob launches): the submit->first-step clock of this job
    for _ in range(max(args.warmup - 1, 0)):
        loss = tr.step(batches)
    # box-speed evidence (bench/calibrate.py): fixed-shape GEMM rates just
    # before and just after the timed region, clock sampled during it
    cal = Calibration(dev, enabled=args.calibrate == "1")
    cal.before()
    tdist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    cal.start()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.step(batches)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    tdist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cal.stop()
    cal.after()
    dt = tdist.all_max(dt, dev)
    loss_v = float(loss)
    # data parallelism keeps every replica's weights identical: check it
    # (one fp64 reduction over the flat bf16 buffer, outside the timed region)
    if tr.gather is not None:
        tr.gather.wait_all()
    dumped = dump_outputs(args.dump_outputs, tr, loss) if args.dump_outputs and info.rank == 0 else None
    csum = float(tr.flat.param.sum(dtype=torch.float64))  # no fp32 copy of 16 GB of weights
    in_sync = tdist.all_max(csum, dev) == -tdist.all_max(-csum, dev)
    loss_max = tdist.all_max(loss_v, dev)
    peak_mem = torch.cuda.max_memory_allocated(dev) / 2**30 if dev.type == "cuda" else 0.0
    peak_mem = tdist.all_max(peak_mem, dev)
    steps = max(args.steps, 1)
    ms = dt / steps * 1e3
    global_batch = args.micro_batch * args.grad_accum * n_gpus
    samples_s = global_batch * args.steps / dt if dt > 0 else 0.0
    tokens_s = samples_s * args.seq_len
    flops = tr.cfg.flops_per_token(args.seq_len) * tokens_s
    order = ["process_start"] + (["probes_done"] if "probes_done" in phases else []) + [
        "imports", "dist_init", "model_init", "first_step"]
    startup = {f"{a}->{b}": round(phases[b] - phases[a], 3) for a, b in zip(order, order[1:])}
    on_gpu = dev.type == "cuda"
    rc = 0
    rl = summarize_rccl_log(rccl_log)
    ok = transport_ok(rl, n_gpus)
    any_bad = tdist.all_max(1.0 if ok is False else 0.0, dev) > 0   # any rank's channels off P2P
    out = None
    if info.rank == 0:
        out = {
            "metric": METRIC.format(n=n_gpus),
            "value": round(samples_s, 4),
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "bf16-cpu-reference",
            "data": "synthetic",
            "config": {
                "model": "Llama-3-8B" if args.model == "llama3-8b" else args.model,
                "global_batch": global_batch,
                "seq_len": args.seq_len,
                "parallelism": f"dp{n_gpus}",
                "micro_batch_per_gpu": args.micro_batch,
                "grad_accum": args.grad_accum,
                "optimizer": ("AdamW (fused HIP, fp32 master, clip 1.0)" if on_gpu
                              else "AdamW (PyTorch CPU reference, fp32 master, clip 1.0)")
                             + (", ZeRO-1 sharded" if tr.bucketer.shard else ""),
                "tfjob": f"Worker={n_gpus}",
                "launched_by": {"launcher": "operator", "replica": "operator" if os.environ.get("TOA_JOB_NAME")
                                else "direct", "torchrun": "torchrun"}.get(launched_by, launched_by),
                "weights": "random-init",
                "gemm_policy": getattr(tr, "gemm_mode", "torch"),
            },
            "rccl_world": rccl_world,
            "backend": backend,
            "tokens_per_sec": round(tokens_s, 1),
            "model_tflops_per_gpu": round(flops / n_gpus / 1e12, 1),
            "first_step_s": round(phases["first_step"] - phases.get("probes_done", t_proc_start), 2),
            "startup_phases_s": startup,
            "loss": round(loss_v, 4),
            "loss_max_over_ranks": round(loss_max, 4),
            "replicas_identical": bool(in_sync),
            "peak_mem_gib": round(peak_mem, 1),
            # GEMMs that left the hand-written kernels for the library (ops/gemm.py): 0 at the bench shape
            "gemm_fallbacks": {"calls": sum(_gemm.fallbacks().values()), "by_shape": _gemm.fallbacks()},
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        cr = cal.record()
        if cr is not None:
            out["calibration"] = cr
        if rl:
            out["rccl"] = rl
        if ok is not None:
            # one node: every channel must ride P2P (xGMI); SHM / NET means the
            # ranks could not see each other's GPUs and this run measured the
            # degraded path -- flagged in the record, not hidden
            out["rccl_transport_ok"] = ok
            if not ok:
                print(f"[bench] WARNING: RCCL channels not all P2P on one node: "
                      f"{rl['channel_connections_by_transport']}", file=sys.stderr, flush=True)
        if probe is not None:
            _attach_probe(out, probe)

    from ..utils import lastline

    emitted = []

    def render(ab) -> str:
        return json.dumps(dict(out, collectives_ab=dict(
            ab, rccl_transport_ok=None if ok is None else bool(ok and not any_bad))))

    def emit(ab):
        if out is None or emitted:
            return
        emitted.append(1)
        if args.result_file:
            tmp = args.result_file + ".tmp"
            with open(tmp, "w") as f:
                f.write(render(ab))
            os.replace(tmp, args.result_file)
        else:
            print(render(ab), flush=True)

    # the two ZeRO-1 collective transports, timed after the headline (which
    # stays on the configured default).  The headline line survives the A/B:
    # a hung window -> the watchdog emits it; a fatal signal (a GPU fault in a
    # copy-engine pull, SIGTERM from the elastic agent when a peer dies) -> the
    # native handler writes the pre-rendered line (utils/lastline.py).  Either
    # way the A/B field says what ended it and the process leaves with rc.
    budget = 120.0 + 3.0 * 4 * (max(1, args.ab_steps) + 1) * max(ms, 1.0) / 1e3

    def on_timeout():
        lastline.arm("", rc)
        emit({"error": f"A/B did not finish within {budget:.0f} s"})

    wd = _ab_watchdog(budget, on_timeout, rc)
    armed = False
    runs_ab = args.collectives_ab == "1" or (args.collectives_ab == "auto" and n_gpus > 1)
    if on_gpu and runs_ab and not args.result_file:
        err = {"error": f"signal {lastline.SIGNO} ended the process during the A/B"}
        armed = lastline.arm(render(err) + "\n" if out is not None else "", rc)
    ab = collectives_ab(tr, batches, args, info, False if any_bad else ok)
    emit(ab)
    if armed:
        lastline.arm("", rc)   # the line is out; a fatal signal in the teardown only ends the process
    if "error" not in ab:
        try:
            tr.close()         # copy-engine transports: drain, barrier, then unmap (no-op without them)
        except Exception as e:  # noqa: BLE001 - the line is out; report, then the bounded teardown
            print(f"[bench] closing the copy-engine transports failed: {type(e).__name__}: {e}", file=sys.stderr,
                  flush=True)
    finished = tdist.teardown(failed="error" in ab)
    wd.cancel()
    if armed:
        lastline.disarm()
    if not finished:
        print("[bench] process group teardown did not finish; leaving", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(rc)
    return rc


def _attach_probe(out: dict, probe: dict):
    if probe.get("p50_s") is not None:
        out["submit_to_first_step_p50_s"] = probe["p50_s"]
    out["submit_to_first_step"] = {k: v for k, v in probe.items() if k not in ("p50_s", "_raw", "_cold")}
    if probe.get("replica_start"):
        out["submit_to_first_step"]["replica_start"] = probe["replica_start"]
    # every probe's own breakdown (no logs): an outlier is explained in the record itself
    out["submit_to_first_step"]["probes"] = [_probe_record(s) for s in probe.get("_raw", [])]
    cold = probe.get("_cold") or []
    if cold:
        cs = _summary(cold)
        out["submit_to_first_step_cold_p50_s"] = cs["p50_s"]
        out["submit_to_first_step_cold"] = {"samples_s": cs["samples_s"], "breakdown_p50_s": cs["breakdown_p50_s"],
                                            "replica_start": "cold process",
                                            "probes": [_probe_record(s) for s in cold]}


# =============================================================================
# launcher: the benchmark itself is a TFJob
# =============================================================================
def run_launcher(args) -> int:
    n = args.gpus
    if n < 1:
        print("[bench] --gpus must be >= 1", file=sys.stderr)
        return 2
    c = _cluster(n, args.warm_start == "1")
    try:
        probe = probe_latency(args, n, c) if args.latency_probes > 0 else {}
        res_dir = tempfile.mkdtemp(prefix="toa-bench-")
        res_file = os.path.join(res_dir, "result.json")
        cmd = [sys.executable, BENCH_PY, "--gpus", str(n), "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--model", args.model, "--seq-len", str(args.seq_len), "--micro-batch",
               str(args.micro_batch), "--grad-accum", str(args.grad_accum), "--zero", args.zero,
               "--warm-start", args.warm_start,
               "--rccl-log", args.rccl_log, "--latency-probes", "0", "--result-file", res_file,
               "--calibrate", args.calibrate, "--collectives-ab", args.collectives_ab, "--ab-steps", str(args.ab_steps)]
        if args.bucket_mb is not None:
            cmd += ["--bucket-mb", str(args.bucket_mb)]
        if args.full:
            cmd += ["--full"]
        if args.dump_outputs:
            cmd += ["--dump-outputs", args.dump_outputs]
        timeout = args.probe_timeout + 60 + 30 * (args.steps + args.warmup)
        try:
            job = _run_job(c, "bench", n, cmd, timeout, env={"TOA_BENCH_RCCL_DIR": res_dir, "PYTHONUNBUFFERED": "1"})
        except Exception as e:
            print(f"[bench] benchmark TFJob failed: {e}", file=sys.stderr, flush=True)
            return 1
        if not os.path.exists(res_file):
            print("[bench] benchmark TFJob succeeded but wrote no result\n" + job["_logs"], file=sys.stderr)
            return 1
        with open(res_file) as f:
            out = json.load(f)
        start_mode = _start_mode(c)
    finally:
        c.stop()
    job.pop("_logs", None)
    # the benchmark job is one more submission of the same TFJob shape: part of the p50
    p = _summary(list(probe.get("_raw", [])) + [job])
    if probe.get("error"):
        p["error"] = probe["error"]
    p["bench_job_submit_to_first_step_s"] = job["submit_to_first_step_s"]
    job["replica_start"] = start_mode
    p["_raw"] = list(probe.get("_raw", [])) + [job]
    p["_cold"] = probe.get("_cold", [])
    p["replica_start"] = start_mode
    if "node_settle_before_probes_s" in probe:
        p["node_settle_before_probes_s"] = probe["node_settle_before_probes_s"]
    if "node_warm_wait_s" in probe:
        p["node_warm_wait_s"] = probe["node_warm_wait_s"]
    _attach_probe(out, p)
    print(json.dumps(out), flush=True)
    return 0
