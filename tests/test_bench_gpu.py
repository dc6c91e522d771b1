"""bench.py's N > 1 tail on the GPU, rehearsed with four ranks on the one
GPU of the box (gloo carries the process group: RCCL refuses two ranks on
one device; the copy-engine pulls are the real IPC / SDMA path):

* the collectives A/B runs both ZeRO-1 transports after the headline and the
  one JSON line carries it (``collectives_ab``);
* a fatal signal in the middle of the A/B still leaves the headline line
  (written by the native last-line handler, csrc/hip/lastline.hip) with the
  signal in its A/B field, and the job exits 0; a peer dying there makes
  rank 0 report the A/B as failed, not lose the line.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--model", "llama-tiny", "--seq-len", "128", "--micro-batch", "2", "--steps", "3", "--warmup", "1",
        "--latency-probes", "0", "--cold-probes", "0", "--calibrate", "0", "--zero", "1", "--collectives-ab", "1",
        "--ab-steps", "2", "--full"]   # the A/B is not part of a plain run


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(n, extra_env=None, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
           and not k.startswith("TORCHELASTIC_")}
    env.update(TOA_DIST_BACKEND="gloo", TOA_PULL_TIMEOUT_MS="5000", OMP_NUM_THREADS="2",
               TOA_LOCAL_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", str(n), *TINY]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, lines


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [4, 8])
def test_bench_collectives_ab_ranks_on_one_gpu(n):
    """n = 8: the driver's N = 8 command shape (torchrun, 8 ranks, ZeRO-1
    over 8 shards, the A/B's copy-engine pulls at world 8)."""
    p, lines = _run(n)
    assert p.returncode == 0, p.stderr[-4000:]
    assert len(lines) == 1, p.stdout[-3000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == n and r["value"] > 0 and r["replicas_identical"] is True
    ab = r["collectives_ab"]
    print(json.dumps(ab))
    assert "rccl_transport_ok" in ab
    assert "rccl_ms" in ab or "error" in ab, ab
    if "rccl_ms" in ab:     # gloo stands in for RCCL here: only the record's shape is checked
        assert ab["sdma_ms"] > 0 and len(ab["windows"]) == 4


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_signal_during_ab_keeps_the_line():
    p, lines = _run(4, {"TOA_AB_INJECT_SIGNAL": "0:11:1"})
    assert p.returncode == 0, p.stderr[-4000:]
    assert len(lines) == 1, p.stdout[-3000:]
    r = json.loads(lines[0])
    assert r["value"] > 0 and r["n_gpus"] == 4
    assert r["collectives_ab"]["error"] == "signal 11 ended the process during the A/B", r["collectives_ab"]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_peer_dies_during_ab_keeps_the_line():
    p, lines = _run(4, {"TOA_AB_INJECT_SIGNAL": "2:6:2"})
    assert len(lines) == 1, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    r = json.loads(lines[0])
    assert r["value"] > 0 and "error" in r["collectives_ab"], r["collectives_ab"]
    assert p.returncode == 0, p.stderr[-4000:]
