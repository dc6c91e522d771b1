"""bench.py contract on CPU/gloo (the driver's launches, scaled down):
* ``python bench.py --gpus 2`` really runs 2 ranks -- as a TFJob Worker=2
  through the local operator stack -- and reports n_gpus 2, the process
  group size, identical replicas, and the p50 submit->first-step latency;
* the torchrun launch (WORLD_SIZE set by the elastic agent) runs the latency
  probes on rank 0 before any rank starts, then the same measurement;
* a --gpus / world-size mismatch fails instead of mislabelling the run."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --full: the latency probes and the collectives A/B record are not part of a plain run
TINY = ["--model", "llama-tiny", "--seq-len", "64", "--micro-batch", "2", "--steps", "3", "--warmup", "1", "--full"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env():
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
           and not k.startswith("TORCHELASTIC_")}
    env["OMP_NUM_THREADS"] = "2"
    return env


def _json_line(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


def _check(r, n):
    assert r["n_gpus"] == n and r["rccl_world"] == n and r["config"]["tfjob"] == f"Worker={n}"
    assert r["metric"] == f"samples/sec ({n}-worker TFJob)"
    assert r["config"]["parallelism"] == f"dp{n}" and r["config"]["global_batch"] == 2 * n
    assert r["replicas_identical"] is True
    assert r["value"] > 0 and r["steps"] == 3 and r["warmup"] == 1
    phases = {"process_start->imports", "imports->dist_init", "dist_init->model_init", "model_init->first_step"}
    if r["config"]["launched_by"] == "torchrun":  # rank 0's probe phase is its own field, not part of start-up
        phases = (phases - {"process_start->imports"}) | {"process_start->probes_done", "probes_done->imports"}
    assert set(r["startup_phases_s"]) == phases
    lat = r["submit_to_first_step"]
    assert "error" not in lat and r.get("submit_to_first_step_p50_s", 0) > 0, lat
    assert lat["breakdown_p50_s"]["submit_to_pods_created"] < r["submit_to_first_step_p50_s"]
    _check_schema(r, n)


def _check_schema(r, n):
    """Fields the driver's runs are read by (pinned): the GEMM fallback count
    and the ZeRO-1 collectives A/B record.  On a GPU node at N > 1 the A/B
    carries rccl_ms / sdma_ms / windows; here (gloo, no GPU) it says why it
    was skipped."""
    fb = r["gemm_fallbacks"]
    assert set(fb) == {"calls", "by_shape"} and fb["calls"] == sum(fb["by_shape"].values())
    ab = r["collectives_ab"]
    assert "rccl_transport_ok" in ab
    if "rccl_ms" in ab:
        assert ab["sdma_ms"] > 0 and ab["rccl_ms"] > 0 and len(ab["windows"]) == 4
        assert {w["transport"] for w in ab["windows"]} == {"rccl", "sdma"}
    else:
        assert set(ab) & {"skipped", "error"}, ab
        if n > 1:
            assert "GPU" in ab.get("skipped", ""), ab


@pytest.mark.timeout(600)
def test_bench_launcher_two_workers_through_operator():
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *TINY, "--latency-probes", "1", "--cold-probes",
                        "1"], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=580)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    _check(r, 2)
    assert r["config"]["launched_by"] == "operator"
    lat = r["submit_to_first_step"]
    assert len(lat["samples_s"]) == 2  # 1 probe + the benchmark job itself
    assert lat["replica_start"].startswith("warm")  # the default
    # every probe's own breakdown is in the record, and a cold-process probe set beside the warm one
    assert [pr["submit_to_first_step_s"] for pr in lat["probes"]] == lat["samples_s"]
    assert all("replica_phases_s" in pr and "spawn_to_first_step_s" in pr for pr in lat["probes"])
    assert r["submit_to_first_step_cold_p50_s"] > 0
    cold = r["submit_to_first_step_cold"]
    assert cold["replica_start"] == "cold process" and len(cold["probes"]) == 1
    assert cold["probes"][0]["replica_phases_s"]["process_start->runtime"] > 0.2  # paid its own imports
    assert "ZeRO-1" in r["config"]["optimizer"]


@pytest.mark.timeout(600)
def test_bench_launcher_cold_start():
    """--warm-start 0: every replica is a fresh python process (its import
    phase is paid inside submit -> first step); the default forks the
    kubelet's warm interpreter, whose import phase is near zero."""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *TINY, "--latency-probes", "1", "--warm-start", "0",
                        "--cold-probes", "0"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=580)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    _check(r, 2)
    assert r["submit_to_first_step"]["replica_start"] == "cold process"
    assert r["startup_phases_s"]["process_start->imports"] > 0.2, r["startup_phases_s"]


@pytest.mark.timeout(600)
def test_bench_under_torchrun_probes_first():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", *TINY, "--latency-probes", "1",
           "--cold-probes", "0"]
    p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=580)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    _check(r, 2)
    assert r["config"]["launched_by"] == "torchrun"
    assert len(r["submit_to_first_step"]["samples_s"]) == 1


@pytest.mark.timeout(300)
def test_bench_world_mismatch_fails():
    env = _env()
    env.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()))
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *TINY], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=280)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "FATAL" in p.stderr


@pytest.mark.timeout(900)
def test_bench_under_torchrun_four_ranks():
    """A larger world rehearsed on gloo (the driver's N = 4 / 8 launches run
    the same code over RCCL): four ranks under torchrun, ZeRO-1 over four
    shards, latency probes as a TFJob Worker=4 in the node-local layout."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "4", *TINY, "--latency-probes", "1",
           "--cold-probes", "0"]
    env = _env()
    env["OMP_NUM_THREADS"] = "1"
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=880)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    assert r["n_gpus"] == 4 and r["rccl_world"] == 4 and r["config"]["global_batch"] == 8
    assert r["replicas_identical"] is True and "ZeRO-1" in r["config"]["optimizer"]
    assert r["config"]["gemm_policy"] in ("asm", "nosk")  # asm when libtoa_hip carries the kernels
    assert r["submit_to_first_step_p50_s"] > 0


@pytest.mark.timeout(1200)
def test_bench_under_torchrun_eight_ranks():
    """The driver's N = 8 command shape, rehearsed on gloo: torchrun with 8
    ranks, ZeRO-1 over 8 shards, latency probes as a TFJob Worker=8 in the
    node-local layout (verdict r5: the headline job at its real world size)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "8", *TINY, "--zero", "1",
           "--latency-probes", "1", "--cold-probes", "0"]
    env = _env()
    env["OMP_NUM_THREADS"] = "1"
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1180)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    _check(r, 8)
    assert r["config"]["launched_by"] == "torchrun" and "ZeRO-1" in r["config"]["optimizer"]
    assert r["gemm_fallbacks"]["calls"] == 0


@pytest.mark.timeout(1200)
def test_bench_launcher_eight_workers():
    """`python bench.py --gpus 8`: the benchmark submitted as a TFJob Worker=8
    through the local operator stack (the launcher form of the driver's N = 8
    run), eight gloo ranks on the CPU."""
    env = _env()
    env["OMP_NUM_THREADS"] = "1"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "8", *TINY, "--latency-probes", "0", "--cold-probes",
                        "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1180)
    assert p.returncode == 0, p.stderr[-4000:]
    r = _json_line(p.stdout)
    _check(r, 8)
    assert r["config"]["launched_by"] == "operator"
    assert len(r["submit_to_first_step"]["samples_s"]) == 1   # the benchmark job itself


def test_full_only_options_need_full():
    """A plain run is the timed steps alone: every extra is off, asking for one
    without --full is an error, and --full restores each default."""
    from tf_operator_amd.bench import flagship

    ap = flagship.parser()
    plain = flagship.resolve_full(ap.parse_args(["--latency-probes", "0"]))
    assert (plain.latency_probes, plain.cold_probes, plain.calibrate, plain.collectives_ab, plain.rccl_log) == (
        0, 0, "0", "0", "0")
    full = flagship.resolve_full(ap.parse_args(["--full", "--cold-probes", "1"]))
    assert (full.latency_probes, full.cold_probes, full.calibrate, full.collectives_ab, full.rccl_log) == (
        3, 1, "1", "auto", "auto")
    for extra in (["--latency-probes", "1"], ["--cold-probes", "1"], ["--calibrate", "1"], ["--collectives-ab", "auto"],
                  ["--rccl-log", "1"]):
        with pytest.raises(ValueError, match="needs --full"):
            flagship.resolve_full(ap.parse_args(extra))


@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run carries no probe / calibration records, --steps sets the
    timed steps, and --dump-outputs writes the last step's loss and parameters
    as float32 .npy files that a second run with the same arguments repeats
    bit for bit."""
    import numpy as np

    got = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, "bench.py", "--direct", "--gpus", "1", "--model", "llama-tiny", "--seq-len",
                            "64", "--micro-batch", "2", "--steps", "2", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / d)], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=280)
        assert p.returncode == 0, p.stderr[-4000:]
        r = _json_line(p.stdout)
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0
        assert abs(r["value"] - 2 / (r["ms_per_step"] / 1000)) / r["value"] < 0.01
        assert "calibration" not in r and "rccl" not in r and "submit_to_first_step" not in r
        assert sorted(os.listdir(tmp_path / d)) == ["loss.npy", "params.npy"]
        arrs = {n: np.load(tmp_path / d / f"{n}.npy") for n in ("loss", "params")}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert r["dumped_outputs"]["arrays"] == {n: list(a.shape) for n, a in arrs.items()}
        assert arrs["loss"].shape == (1,) and abs(float(arrs["loss"][0]) - r["loss"]) < 1e-3
        assert arrs["params"].size > 1000 and np.isfinite(arrs["params"]).all()
        got.append(arrs)
    assert all(np.array_equal(got[0][n], got[1][n]) for n in got[0])
