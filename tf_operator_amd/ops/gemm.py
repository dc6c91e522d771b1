"""Row-major bf16 GEMM entry points of the training step.

    linear_fwd(x, w)           y  = x w^T            [M,K] x [N,K] -> [M,N]
    linear_dgrad(dy, w)        dx = dy w             [M,N] x [N,K] -> [M,K]
    wgrad_acc_(g, dy, x)       g += dy^T x           (beta = 1, in place)

The forward / data-gradient forms run on the hand-written assembly kernel
(the default, ``TOA_GEMM=asm``) or on the hipBLASLt layer (csrc/hip/gemm.hip,
one column-major call per form, see there for the transposition algebra;
``TOA_GEMM=nosk``); the weight gradient on the assembly NT kernel
(csrc/asm/wgrad_gen.py), with the HIP NT kernel (csrc/hip/wgrad.hip) as its
fallback.
The per-form solution tables measured by ``scripts/tune_gemm.py`` on an
MI355X are stored next to this file, keyed by the hipBLASLt build.

Modes (``TOA_GEMM``):

* ``asm``: the hand-written gfx950 assembly GEMM (csrc/asm/gemm_gen.py,
  launched from csrc/hip/gemm_asm.hip) for every forward / data-gradient
  GEMM whose shape it takes (M, N multiples of 256, K a multiple of 64 and
  >= 128 -- all Llama forms), with the Llama MLP's SwiGLU fused into the
  gate|up projection's epilogue and its backward into the down projection's
  data gradient (``ops.llm.swiglu_mlp``); anything else as ``nosk``.  No
  hipBLASLt table to load, so nothing to prewarm for these forms.
  ``hip`` is an alias (it named the round-3 HIP TN kernel this replaced).
* ``torch``: torch.matmul, i.e. hipBLASLt's own heuristic.  Per-form
  winners picked in isolation were 2-22 % faster alone, yet the full
  Llama-3-8B step was ~1.3 % SLOWER with them (profiles/r1_gemm_*).
* ``tuned``: the measured per-form table (``gemm_tuning_gfx950.json``).
* ``nosk``: the fastest solution per form among those that are NOT
  stream-K (``gemm_tuning_gfx950_nosk.json``, ``scripts/tune_gemm.py
  --exclude-streamk``).  Stream-K kernels hold one workgroup per CU for the
  whole GEMM, so a collective on another stream gets no CU until it ends
  (profiles/r2_sk_contention; +6.7 % vs +3.4 % under emulated world-8
  ZeRO-1 traffic, profiles/r3_overlap).
* ``auto`` (the default): resolved by :func:`resolve_auto` when the trainer
  starts, to ``asm``.
"""
from __future__ import annotations

import atexit
import ctypes
import json
import os
import threading
import weakref

import torch

from . import _lib
from ..parallel.zero_check import reading

_HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(_HERE, "gemm_tuning_gfx950.json")
TABLE_NOSK = os.path.join(_HERE, "gemm_tuning_gfx950_nosk.json")
_MODE = os.environ.get("TOA_GEMM", "auto")
if _MODE == "hip":
    _MODE = "asm"
_installed = False


def mode() -> str:
    return _MODE


def set_mode(m: str):
    """Select the GEMM policy for this process (before the first GEMM)."""
    global _MODE, _installed
    if m not in ("auto", "torch", "tuned", "nosk", "hip", "asm"):
        raise ValueError(f"unknown GEMM mode {m!r}")
    _MODE = "asm" if m == "hip" else m
    _installed = False


def resolve_auto(world: int = 1) -> str:
    """``auto`` -> ``asm`` (an explicit TOA_GEMM is kept).  Returns the mode
    in force.  The assembly kernel with the library-form slot map, the
    per-shape tile order and the fused SwiGLU epilogues wins in-model: the
    Llama-3-8B step is 5.5 +- 1.6 ms faster than on ``nosk`` (12 ABBA rounds
    in one process, profiles/r5_asm_gemm/inmodel_abba12.log; 9.4 ms less kernel time
    under rocprofv3, profiles/r5_prof1).  Like ``nosk`` it never holds the
    whole chip (one workgroup per tile, no stream-K), so the data-parallel
    collectives overlap it.  Round 4 measured the other way (946.3 vs 930.1
    ms, profiles/r4_wgrad/inmodel_ab.log), before those changes."""
    del world
    if _MODE == "auto":
        set_mode("asm")
    return _MODE


def hipblaslt_build() -> str:
    """Identity of the hipBLASLt library solution indices belong to."""
    for d in ("/opt/rocm/lib", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")):
        p = os.path.join(d, "libhipblaslt.so")
        if os.path.exists(p):
            return os.path.basename(os.path.realpath(p))
    return "unknown"


def _install():
    global _installed
    if _installed:
        return
    _installed = True
    if _lib.has("toa_gemm_set_no_streamk"):
        _lib.call("toa_gemm_set_no_streamk", int(_MODE in ("nosk", "asm")))
    table = TABLE_NOSK if _MODE in ("nosk", "asm") else TABLE
    if not os.path.exists(table):
        return
    with open(table) as f:
        tab = json.load(f)
    if tab.get("hipblaslt") != hipblaslt_build():
        return
    for e in tab.get("entries", []):
        if e.get("index", -1) >= 0:
            _lib.call("toa_gemm_set_algo", e["ta"], e["tb"], e["m"], e["n"], e["k"], e["lda"], e["ldb"], e["ldc"],
                      e["beta_nz"], e.get("out_f32", 0), e["index"])


_prewarm_thread = None
_prewarm_dev = None


def prewarm(device=None, background: bool = True):
    """Resolve the installed table's plans (hipBLASLt handle, solution
    lookup, support checks: ~0.47 s of host work, mostly code-object loading,
    at the first GEMM -- profiles/r3_first) ahead of the first step.  With
    `background` it runs on a helper thread -- ctypes drops the GIL, so the
    caller initialises the process group and the model meanwhile -- and the
    thread is returned (the GEMM layer's lock orders the first real GEMM
    after it).  Idempotent; None when the policy uses no table."""
    global _prewarm_thread, _prewarm_dev
    if _MODE not in ("tuned", "nosk") or not _lib.has("toa_gemm_prewarm"):
        return None
    dev = None if device is None else torch.device(device).index
    dev = torch.cuda.current_device() if dev is None else dev
    if _prewarm_thread is not None:
        if _prewarm_dev != dev:
            # started for another device (a caller guessed LOCAL_RANK): the
            # handle it built is not this replica's -- fail loudly
            raise RuntimeError(f"GEMM prewarm ran on cuda:{_prewarm_dev}, trainer binds cuda:{dev}")
        return _prewarm_thread
    _install()
    _prewarm_dev = dev

    def work():
        torch.cuda.set_device(dev)
        _lib.call_ret("toa_gemm_prewarm")

    if not background:
        work()
        return None
    _prewarm_thread = threading.Thread(target=work, name="toa-gemm-prewarm", daemon=True)
    _prewarm_thread.start()
    # the first step no longer waits for it (first_step), so a one-step job
    # can reach interpreter exit while it is inside the HIP / hipBLASLt
    # loaders; a daemon thread killed there takes the process down with a
    # non-zero exit (profiles/r4_fresh2: a one-step probe job Failed after
    # "done: 1 steps").  Join it at exit instead.
    atexit.register(_join_prewarm)
    return _prewarm_thread


def _join_prewarm(timeout: float = 120.0):
    t = _prewarm_thread
    if t is not None and t.is_alive():
        t.join(timeout)


def prewarm_early():
    """Start :func:`prewarm` at process start, on this replica's GPU (the
    device train/dist.py binds: TOA_LOCAL_DEVICE, the pod-resources
    allocation, else LOCAL_RANK), before the process group and the model
    exist.  No-op off the GPU, for the ``torch`` policy, or without the HIP
    library."""
    if not torch.cuda.is_available():
        return None
    resolve_auto()
    from ..train import dist as tdist

    try:
        local = tdist.local_device_index()
    except Exception:  # noqa: BLE001 - e.g. grpc.RpcError (kubelet socket down), ImportError (no grpcio)
        return None  # the trainer's own init (train/dist.py) hits the same lookup and reports it
    if local >= torch.cuda.device_count():
        return None
    return prewarm(torch.device("cuda", local))


def _ok(*ts):
    if _MODE not in ("tuned", "nosk", "asm") or not _lib.has("toa_gemm"):
        return False
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1):
            return False
    return _lib.use_hip(ts[0])


def _gemm(ta, tb, m, n, k, a, lda, b, ldb, c, ldc, beta):
    _install()
    _lib.call("toa_gemm", ta, tb, m, n, k, _lib.ptr(a), lda, _lib.ptr(b), ldb, _lib.ptr(c), ldc, float(beta),
              int(c.dtype == torch.float32), _lib.stream(c))


_asm_first = False

# GEMMs of a GPU training step that left the hand-written kernels for the
# library (hipBLASLt / torch.matmul) under the ``asm`` policy, per (op, shape):
# a user's TFJob at, say, seq 4000 would otherwise run the library for every
# GEMM without a trace.  Warned once per shape on stderr; the bench record
# carries the counts (``gemm_fallbacks``).
_FALLBACKS: dict = {}
_fallback_lock = threading.Lock()


def _fallback(op: str, shape, target: str, why: str):
    key = f"{op} {'x'.join(str(int(d)) for d in shape)} -> {target}"
    with _fallback_lock:
        n = _FALLBACKS.get(key, 0)
        _FALLBACKS[key] = n + 1
    if n == 0:
        import sys

        print(f"[toa.gemm] WARNING: {key} ({why}); later calls of this shape are counted, not logged",
              file=sys.stderr, flush=True)


def fallbacks() -> dict:
    """{"op MxNxK -> target": calls} since the process started (or reset)."""
    with _fallback_lock:
        return dict(_FALLBACKS)


def reset_fallbacks():
    with _fallback_lock:
        _FALLBACKS.clear()


def _refused(reason: int, M, N, K) -> str:
    """The fallback warning's reason: the launcher's own words for the first
    condition that failed (toa_gemm_shape_why), with the shape."""
    return f"{_lib.shape_why(reason)}: M={M} N={N} K={K}"


class first_step:
    """Context of a trainer's FIRST step under the hipBLASLt policies: every
    forward / data-gradient GEMM the assembly kernel takes runs on it, so the
    step does not wait for the hipBLASLt plans that :func:`prewarm` is still
    loading on its helper thread (profiles/r4_fresh: model_init ->
    first forward issued 0.48-0.63 s without it).  Deterministic: the first
    step always takes this path, whatever the helper thread's progress, and
    later steps never do.  The MLP stays unfused (ops.llm.swiglu_mlp keys on
    the policy)."""

    def __init__(self, on: bool = True):
        # TOA_GEMM_TN_FIRST=0: the first step stays on the steady-state policy
        self.on = (bool(on) and _MODE in ("nosk", "tuned") and _lib.has("toa_gemm_asm")
                   and os.environ.get("TOA_GEMM_TN_FIRST", "1") != "0")

    def __enter__(self):
        global _asm_first
        self.prev, _asm_first = _asm_first, self.on or _asm_first
        return self

    def __exit__(self, *exc):
        global _asm_first
        _asm_first = self.prev
        return False


def _kind_why(*ts) -> str:
    """What the launchers' checks cannot see -- bf16 GPU matrices with unit
    column stride: the first tensor property that is not so, "" if all are."""
    for t in ts:
        if not (t.is_cuda and t.dim() == 2):
            return f"a {t.dim()}-D {t.device.type} tensor, not a GPU matrix"
        if t.dtype != torch.bfloat16:
            return f"dtype {t.dtype}, not bf16"
        if t.stride(1) != 1:
            return f"column stride {t.stride(1)}, not 1"
    return ""


def _gate_why(a: torch.Tensor, w: torch.Tensor, wk: int, kernel: str) -> str:
    """Why (a [M, K], w with K along dim wk) are no operands of `kernel`
    before any shape is asked about, "" if they are."""
    if not _lib.has(kernel):
        return f"library built without {kernel}"
    kind = _kind_why(a, w)
    if not kind and w.shape[wk] != a.shape[1]:
        kind = f"K={a.shape[1]} columns against {w.shape[wk]} in the weight"
    return kind


def _asm_gate(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """The policy runs the TN assembly GEMMs and (x2 [M, K], w [N, K]) are operands of one."""
    return (_MODE == "asm" or _asm_first) and not _gate_why(x2, w, 1, "toa_gemm_asm") and _lib.use_hip(x2)


def _tn_reason(x2: torch.Tensor, w: torch.Tensor) -> int:
    """toa_gemm_shape_check for y [M, N] = x2 w^T, y contiguous.  The form is
    the policy's choice: any row count under ``asm``, whole tiles only under
    first_step (a hipBLASLt policy's start-up), as before."""
    form = "tn_rows" if _MODE == "asm" and _lib.has("toa_gemm_asm_rows") else "tn"
    N = w.shape[0]
    return _lib.shape_check(form, (x2, w), (x2.stride(0), w.stride(0), N), x2.shape[0], N, x2.shape[1])


def asm_takes(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """Operands the assembly GEMM takes for x2 [M, K] w [N, K]^T: bf16 GPU
    rows with unit column stride under a policy that runs it, and a shape its
    launcher takes (csrc/hip/gemm_asm_shapes.h; the table in docs/kernels.md).
    The fused epilogues' predicates (ops/llm.py) ask about their own forms."""
    return _asm_gate(x2, w) and _tn_reason(x2, w) == 0


def linear_fwd(x2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    reading(w, "linear_fwd")
    if asm_takes(x2, w):
        M, N = x2.shape[0], w.shape[0]
        y = torch.empty(M, N, device=x2.device, dtype=x2.dtype)
        # (toa_gemm_asm itself refuses a partial last tile row; same kernel)
        _lib.call("toa_gemm_asm_rows" if M % 256 else "toa_gemm_asm", _lib.ptr(x2), x2.stride(0), _lib.ptr(w),
                  w.stride(0), _lib.ptr(y), N, M, N, x2.shape[1], _lib.stream(x2))
        return y
    lib_ok = _ok(x2, w)
    if _MODE == "asm" and x2.is_cuda and x2.dim() == 2 and w.dim() == 2:
        M, N, K = x2.shape[0], w.shape[0], x2.shape[1]
        _fallback("fwd", (M, N, K), "hipBLASLt" if lib_ok else "torch.matmul",
                  _gate_why(x2, w, 1, "toa_gemm_asm") or _refused(_tn_reason(x2, w), M, N, K))
    if not lib_ok:
        return torch.matmul(x2, w.t())
    M, K = x2.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x2.device, dtype=x2.dtype)
    _gemm(1, 0, N, M, K, w, w.stride(0), x2, x2.stride(0), y, N, 0.0)
    return y


def linear_resadd(x2: torch.Tensor, w: torch.Tensor, r2: torch.Tensor) -> torch.Tensor:
    """y = x2 w^T + r2, the add in the assembly GEMM's epilogue
    (toa_gemm_asm_resadd: the fp32 sum rounded to bf16 once); r2 [M, N] bf16,
    contiguous.  For operands ops.llm's ``*_resadd_ok`` predicates passed:
    anything the launcher refuses raises."""
    reading(w, "linear_resadd")
    y = torch.empty_like(r2)
    _lib.call("toa_gemm_asm_resadd", _lib.ptr(x2), x2.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(y), y.stride(0),
              _lib.ptr(r2), x2.shape[0], w.shape[0], x2.shape[1], _lib.stream(x2))
    return y


# Data gradient dX = dY W of a weight without a transposed copy: "wt" (default)
# leaves it to the library, as before; "nn" runs the NN-form assembly kernel on
# W as stored (csrc/asm/gemm_gen.py kernel_nn), so no copy is needed at all --
# ops.wt.enabled_default then builds none.  An explicit ``_toa_wt`` always wins.
_DGRAD_FORM = None


def dgrad_form() -> str:
    """``wt`` (default) or ``nn``; ``TOA_DGRAD`` sets it without a code change."""
    global _DGRAD_FORM
    if _DGRAD_FORM is None:
        forced = os.environ.get("TOA_DGRAD", "")
        if forced not in ("", "wt", "nn"):
            raise ValueError(f"TOA_DGRAD={forced!r}: expected wt or nn")
        _DGRAD_FORM = forced or "wt"
    return _DGRAD_FORM


def set_dgrad_form(name: str):
    global _DGRAD_FORM
    if name not in ("wt", "nn"):
        raise ValueError(f"unknown data-gradient form {name!r}")
    _DGRAD_FORM = name


def _nn_gate(dy2: torch.Tensor, w: torch.Tensor) -> bool:
    """The policy runs the NN assembly GEMMs and (dy2 [M, K], w [K, N] as stored) are operands of one."""
    return _MODE == "asm" and not _gate_why(dy2, w, 0, "toa_gemm_nn_asm") and _lib.use_hip(dy2)


def _nn_reason(dy2: torch.Tensor, w: torch.Tensor) -> int:
    N = w.shape[1]
    return _lib.shape_check("nn", (dy2, w), (dy2.stride(0), w.stride(0), N), dy2.shape[0], N, dy2.shape[1])


def nn_takes(dy2: torch.Tensor, w: torch.Tensor) -> bool:
    """Operands the NN-form assembly GEMM takes for dX = dy2 [M, K] w [K, N]
    (w as stored) under the ``asm`` policy: see asm_takes."""
    return _nn_gate(dy2, w) and _nn_reason(dy2, w) == 0


def linear_dgrad(dy2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    reading(w, "linear_dgrad")   # the W^T copy is refreshed by the gather's wait: a read of it is a read of w
    wt = getattr(w, "_toa_wt", None)
    if wt is not None:  # W^T kept by ops.wt.TransposedWeights: dx = dy (W^T)^T, the forward's form
        return linear_fwd(dy2, wt)
    why = "no transposed weight copy (ops/wt.py) for this weight"
    if _MODE == "asm" and dgrad_form() == "nn":
        if nn_takes(dy2, w):
            M, N = dy2.shape[0], w.shape[1]
            dx = torch.empty(M, N, device=dy2.device, dtype=dy2.dtype)
            _lib.call("toa_gemm_nn_asm", _lib.ptr(dy2), dy2.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(dx), N,
                      M, N, dy2.shape[1], _lib.stream(dy2))
            return dx
        why = "NN form refused: " + (_gate_why(dy2, w, 0, "toa_gemm_nn_asm")
                                     or _refused(_nn_reason(dy2, w), dy2.shape[0], w.shape[1], dy2.shape[1]))
    lib_ok = _ok(dy2, w)
    if _MODE == "asm" and dy2.is_cuda and dy2.dim() == 2 and w.dim() == 2:
        _fallback("dgrad", (dy2.shape[0], w.shape[1], dy2.shape[1]), "hipBLASLt" if lib_ok else "torch.matmul", why)
    if not lib_ok:
        return torch.matmul(dy2, w)
    M, N = dy2.shape
    K = w.shape[1]
    dx = torch.empty(M, K, device=dy2.device, dtype=dy2.dtype)
    _gemm(0, 0, K, M, N, w, w.stride(0), dy2, dy2.stride(0), dx, K, 0.0)
    return dx


def swiglu_gate_up(x2: torch.Tensor, wgu: torch.Tensor):
    """(gu, s) = (x Wgu^T, silu(gate) * up) from ONE assembly GEMM with the
    SwiGLU in its epilogue; None when the kernel cannot take the shapes."""
    reading(wgu, "swiglu_gate_up")
    M, F, K = x2.shape[0], wgu.shape[0] // 2, x2.shape[1]
    if not (_asm_gate(x2, wgu) and wgu.shape[0] == 2 * F and _lib.shape_check(
            "tn_swiglu_fwd", (x2, wgu), (x2.stride(0), wgu.stride(0), 2 * F, F), M, F, K) == 0):
        return None
    gu = torch.empty(M, 2 * F, device=x2.device, dtype=x2.dtype)
    s = torch.empty(M, F, device=x2.device, dtype=x2.dtype)
    _lib.call("toa_gemm_asm_swiglu", _lib.ptr(x2), x2.stride(0), _lib.ptr(wgu), wgu.stride(0), _lib.ptr(gu), 2 * F,
              _lib.ptr(s), F, M, F, x2.shape[1], _lib.stream(x2))
    return gu, s


def swiglu_down_dgrad(d2: torch.Tensor, wd: torch.Tensor, gu: torch.Tensor):
    """dgu = SwiGLU-backward(gu, ds = d2 Wd) from ONE assembly GEMM on the
    transposed weight copy (ops/wt.py) -- or, without one under
    ``dgrad_form() == "nn"``, on Wd as stored -- with the SwiGLU backward in
    its epilogue (ds is never stored); None when the kernel cannot take it."""
    reading(wd, "swiglu_down_dgrad")
    wdt = getattr(wd, "_toa_wt", None)
    if wdt is None and dgrad_form() == "nn":     # on Wd [D, F] as stored (the NN form)
        M, F = d2.shape[0], wd.shape[1]
        if not (_nn_gate(d2, wd) and _lib.has("toa_gemm_nn_asm_swiglu_bwd") and gu.is_contiguous()
                and gu.shape[1] == 2 * F and _lib.shape_check(
                    "nn_swiglu_bwd", (d2, wd, None, gu), (d2.stride(0), wd.stride(0), 2 * F, 2 * F), M, F,
                    d2.shape[1]) == 0):
            return None
        dgu = torch.empty_like(gu)
        _lib.call("toa_gemm_nn_asm_swiglu_bwd", _lib.ptr(d2), d2.stride(0), _lib.ptr(wd), wd.stride(0), _lib.ptr(gu),
                  2 * F, _lib.ptr(dgu), 2 * F, M, F, d2.shape[1], _lib.stream(d2))
        return dgu
    if wdt is None:
        return None
    M, F = d2.shape[0], wdt.shape[0]
    if not (_asm_gate(d2, wdt) and gu.is_contiguous() and gu.shape[1] == 2 * F and _lib.shape_check(
            "tn_swiglu_bwd", (d2, wdt, None, gu), (d2.stride(0), wdt.stride(0), 2 * F, 2 * F), M, F,
            d2.shape[1]) == 0):
        return None
    dgu = torch.empty_like(gu)
    _lib.call("toa_gemm_asm_swiglu_bwd", _lib.ptr(d2), d2.stride(0), _lib.ptr(wdt), wdt.stride(0), _lib.ptr(gu),
              2 * F, _lib.ptr(dgu), 2 * F, M, F, d2.shape[1], _lib.stream(d2))
    return dgu


_ws = {}
HIP_ERROR_INVALID_VALUE = 1
# weight-gradient kernel: the assembly NT kernel (csrc/asm/wgrad_gen.py;
# 1.30-1.50 PF/s at the Llama forms, 1-12 % faster than the HIP kernel and
# bit-identical to it, profiles/r4_wgrad/) where the library carries it, else
# the HIP kernel (csrc/hip/wgrad.hip).  set_wgrad_kernel switches it for
# in-process A/B runs (scripts/wgrad_inmodel_ab.py).
_WGRAD_KERNEL = None


def wgrad_kernel() -> str:
    """``asm`` (default where the library carries it) or ``hip``;
    ``TOA_WGRAD=hip`` forces the HIP kernel without a code change."""
    global _WGRAD_KERNEL
    if _WGRAD_KERNEL is None:
        forced = os.environ.get("TOA_WGRAD", "")
        if forced not in ("", "asm", "hip"):
            raise ValueError(f"TOA_WGRAD={forced!r}: expected asm or hip")
        _WGRAD_KERNEL = forced or ("asm" if _lib.has("toa_wgrad_asm") else "hip")
    return _WGRAD_KERNEL


def set_wgrad_kernel(name: str):
    """asm | hip (the in-process A/B of scripts/wgrad_inmodel_ab.py)."""
    global _WGRAD_KERNEL
    if name not in ("asm", "hip"):
        raise ValueError(f"unknown weight-gradient kernel {name!r}")
    _WGRAD_KERNEL = name


def _workspace(dev, nbytes):
    """Split-K partials scratch, one per (device, stream): a weight gradient
    on a side stream (ops.llm set_mlp_overlap) must not share it with one on
    the main stream."""
    key = (dev, torch.cuda.current_stream(dev).stream_id if torch.device(dev).type == "cuda" else 0)
    t = _ws.get(key)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
        _ws[key] = t
    return t


# ---- 1 to 16 rows: the weight-streaming GEMM of the decode step (csrc/hip/gemm_skinny.hip).  What it takes is
# csrc/hip/gemm_skinny_shapes.h's to say (toa_gemm_skinny_check); this module adds only what a launcher cannot see:
# the tensors' kind.
def skinny_reason(x2, w, swiglu: bool = False, y=None, ws=None) -> int:
    """toa_gemm_skinny_check for y [M, N] = x2 [M, K] w [N, K]^T (swiglu: w =
    gate | up [2F, K], y = s [M, F]): 0 = taken, else the reason
    :func:`skinny_why` names.  y and ws default to what the launch wrappers
    allocate themselves (contiguous, aligned): x2 stands in for them."""
    M, K = x2.shape
    N = w.shape[0] // 2 if swiglu else w.shape[0]
    y_ptr, ldy = (x2.data_ptr(), N) if y is None else (y.data_ptr(), y.stride(0))
    ws_ptr = x2.data_ptr() if ws is None else ws.data_ptr()
    return _lib.call_ret("toa_gemm_skinny_check", int(swiglu), x2.data_ptr(), w.data_ptr(), y_ptr, ws_ptr,
                         x2.stride(0), w.stride(0), ldy, w.shape[0], M, N, K)


def skinny_why(reason: int) -> str:
    return _lib._fn("toa_gemm_skinny_why")(reason).decode()


def skinny_refusal(x2, w, swiglu: bool = False) -> str:
    """Why (x2 [M, K], w [N, K]) are no operands of the 1-to-16-row GEMM, ""
    if they are: matrices with unit column stride and a common K, bf16 on the
    GPU (CPU tensors of any float dtype take the fp32 reference), and a shape
    the launcher's check takes, in its own words."""
    if not _lib.has("toa_gemm_skinny_check"):
        return "library built without toa_gemm_skinny"
    for t in (x2, w):
        if t.dim() != 2:
            return f"a {t.dim()}-D tensor, not a matrix"
        if t.stride(1) != 1:
            return f"column stride {t.stride(1)}, not 1"
        if t.is_cuda and t.dtype != torch.bfloat16:
            return f"dtype {t.dtype}, not bf16"
    if x2.device != w.device or x2.dtype != w.dtype:
        return f"x ({x2.dtype}, {x2.device}) and w ({w.dtype}, {w.device}) differ"
    if w.shape[1] != x2.shape[1]:
        return f"K={x2.shape[1]} columns against {w.shape[1]} in the weight"
    r = skinny_reason(x2, w, swiglu)
    if r:
        return f"{skinny_why(r)}: M={x2.shape[0]} N={w.shape[0] // 2 if swiglu else w.shape[0]} K={x2.shape[1]}"
    return ""


def skinny_takes(x2, w, swiglu: bool = False) -> bool:
    """bf16 GPU matrices with unit column stride whose shape toa_gemm_skinny_check accepts."""
    return x2.is_cuda and w.is_cuda and not skinny_refusal(x2, w, swiglu)


def _skinny_call(name, ws_name, x2, w, N, swiglu):
    r = skinny_refusal(x2, w, swiglu)
    if r:
        raise ValueError(f"{name}: {r}")
    M, K = x2.shape
    if not _lib.use_hip(x2):
        return None
    y = torch.empty(M, N, device=x2.device, dtype=x2.dtype)
    nbytes = int(_lib.call_ret(ws_name, N, K))
    ws = _workspace(x2.device, nbytes) if nbytes > 0 else None
    _lib.call(name, _lib.ptr(x2), x2.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(y), N, M, N, K, _lib.ptr(ws),
              _lib.stream(x2))
    return y


def linear_skinny(x2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """y [M, N] = x2 [M, K] w [N, K]^T for M <= 16 on toa_gemm_skinny: fp32
    accumulation, one rounding.  Operands skinny_refusal names raise
    ValueError before a launch; CPU tensors take the fp32 reference."""
    reading(w, "linear_skinny")
    y = _skinny_call("toa_gemm_skinny", "toa_gemm_skinny_ws_bytes", x2, w, w.shape[0], False)
    return (x2.float() @ w.float().t()).to(x2.dtype) if y is None else y


def swiglu_skinny(x2: torch.Tensor, wgu: torch.Tensor) -> torch.Tensor:
    """s [M, F] = silu(x2 Wg^T) * (x2 Wu^T), wgu = gate | up [2F, K], for
    M <= 16 on toa_gemm_skinny_swiglu: the product is taken from the fp32
    accumulators and rounded once; gu is never stored."""
    reading(wgu, "swiglu_skinny")
    F_ = wgu.shape[0] // 2
    s = _skinny_call("toa_gemm_skinny_swiglu", "toa_gemm_skinny_swiglu_ws_bytes", x2, wgu, F_, True)
    if s is None:
        gu = x2.float() @ wgu.float().t()
        s = (torch.nn.functional.silu(gu[:, :F_]) * gu[:, F_:]).to(x2.dtype)
    return s


def _wgrad_reason(form: str, g, dy2, x2, split: int = 0) -> int:
    """toa_gemm_shape_check for g [N, K] (+)= dy2 [T, N]^T x2 [T, K] on the
    assembly ("wgrad_asm") or the HIP ("wgrad_hip") kernel.  g stands in for
    the split-K workspace, which is allocated per call (_workspace), aligned."""
    T, N = dy2.shape
    K = x2.shape[1]
    return _lib.shape_check(form, (dy2, x2, g, g), (dy2.stride(0), x2.stride(0), K), N, K, T, split=split)


def _wgrad_asm_selected() -> bool:
    return wgrad_kernel() == "asm" and _lib.has("toa_wgrad_asm_workspace")


def _wgrad_gate_why(g, dy2, x2) -> str:
    """Why (g, dy2 [T, N], x2 [T, K]) are no operands of the hand-written
    weight-gradient kernels before any shape is asked about, "" if they are."""
    if not _lib.has("toa_wgrad"):
        return "library built without toa_wgrad"
    kind = _kind_why(dy2, x2)
    if kind:
        return kind
    if g.dtype != torch.bfloat16:
        return f"gradient dtype {g.dtype}, not bf16"
    if x2.shape[0] != dy2.shape[0]:
        return f"T={dy2.shape[0]} rows of dy against {x2.shape[0]} of x"
    if not g.is_contiguous() or tuple(g.shape) != (dy2.shape[1], x2.shape[1]):
        return f"gradient {tuple(g.shape)} with strides {g.stride()}, not a contiguous [N, K]"
    return ""


def wgrad_hip_ok(g, dy2, x2) -> bool:
    """Shapes/layouts the hand-written weight-gradient kernels take: bf16
    rows with unit column stride, a contiguous g [N, K], and a shape the
    assembly kernel (when selected) or csrc/hip/wgrad.hip takes
    (csrc/hip/gemm_asm_shapes.h)."""
    return not _wgrad_gate_why(g, dy2, x2) and (
        (_wgrad_asm_selected() and _wgrad_reason("wgrad_asm", g, dy2, x2) == 0)
        or _wgrad_reason("wgrad_hip", g, dy2, x2) == 0)


class SumsqSession:
    """The clipping norm from partials the weight-gradient kernels write as
    they produce the gradients (no separate pass over the 16 GB of bf16
    gradients at Llama-3-8B): every 2-D weight in `params` whose gradient
    the assembly kernel produces gets a fixed region of `buf`, 256 floats per
    256 x 256 output tile (wgrad_gen.py KARG "sq"; the split-K tail tiles via
    the reduce kernel).  norm_sq() sums the whole buffer in one fixed-order
    pass when every region was written this step and adds the squares of the
    flat ranges outside the regions (embeddings, norm weights); otherwise it
    falls back to the full pass over the gradient.  Only for an unsharded,
    unreduced world-1 update: the partials are of this rank's gradient.
    Differs from the full pass only in summation order and in squaring the
    fp32 tile values before their bf16 rounding."""

    def __init__(self, flat, params):
        self.flat = flat
        want = {id(p) for p in params}
        self.regions = {}      # grad view data_ptr -> (offset in buf, floats, [N, K])
        off = 0
        covered = []
        for sgm in flat.segments:
            p = sgm.param
            if id(p) not in want or p.dim() != 2 or p.shape[0] % 256 or p.shape[1] % 256:
                continue
            n = (p.shape[0] // 256) * (p.shape[1] // 256) * 256
            self.regions[p.main_grad.data_ptr()] = (off, n, tuple(p.shape))
            covered.append((sgm.offset, sgm.offset + sgm.numel))
            off += n
        self.buf = torch.zeros(max(off, 4), device=flat.device, dtype=torch.float32)
        # the flat ranges no region covers, as contiguous runs
        covered.sort()
        self.rest, pos = [], 0
        for a, b in covered:
            if a > pos:
                self.rest.append((pos, a))
            pos = max(pos, b)
        if pos < flat.numel:
            self.rest.append((pos, flat.numel))
        # the small rest ranges (norm weights) in one launch: offsets / lengths on the device
        small = [(a, b - a) for a, b in self.rest if b - a < (1 << 20)]
        self.rest = [(a, b) for a, b in self.rest if b - a >= (1 << 20)]
        self.small = None
        if small and flat.grad.dtype == torch.bfloat16 and len(small) <= 32768:
            t = torch.tensor(small, dtype=torch.int64).t().contiguous().to(flat.device)
            self.small = (t[0], t[1], len(small))
        elif small:
            self.rest = sorted(self.rest + [(a, a + n) for a, n in small])
        self.written = set()
        self.hits = 0           # steps served from the partials (tests, diagnostics)

    def owns(self, g) -> bool:
        return g.data_ptr() in self.regions

    def arm(self, g) -> bool:
        """Point the next weight-gradient launch at g's region."""
        off, n, shape = self.regions[g.data_ptr()]
        if tuple(g.shape) != shape:
            return False
        _lib.call("toa_wgrad_asm_set_sumsq", self.buf.data_ptr() + 4 * off)
        return True

    def norm_sq(self, out, ws):
        """out[0] = the squared gradient norm; the written set is cleared."""
        f = self.flat
        s = _lib.stream(f.grad)
        full = len(self.written) == len(self.regions)
        self.written = set()
        if not full:
            _lib.call("toa_sumsq", _lib.ptr(f.grad), f.grad.numel(), int(f.grad.dtype == torch.bfloat16),
                      _lib.ptr(ws), _lib.ptr(out), 0, s)
            return out
        self.hits += 1
        _lib.call("toa_sum_f32", _lib.ptr(self.buf), self.buf.numel(), _lib.ptr(ws), _lib.ptr(out), 0, s)
        esz = f.grad.element_size()
        for a, b in self.rest:
            _lib.call("toa_sumsq", f.grad.data_ptr() + esz * a, b - a, int(f.grad.dtype == torch.bfloat16),
                      _lib.ptr(ws), _lib.ptr(out), 1, s)
        if self.small is not None:
            offs, lens, n = self.small
            _lib.call("toa_sumsq_ranges", _lib.ptr(f.grad), _lib.ptr(offs), _lib.ptr(lens), n, _lib.ptr(ws),
                      _lib.ptr(out), 1, s)
        return out


_SESSIONS = weakref.WeakSet()   # live SumsqSession objects (each held by its trainer's optimizer)


def _session_for(g):
    for sess in _SESSIONS:
        if sess.owns(g):
            return sess
    return None


def wgrad_hip_(g, dy2, x2, beta=1.0, split=None):
    """g[N,K] (+)= dy2[T,N]^T x2[T,K] on the hand-written MFMA kernel.
    split=None: the kernel's auto plan (whole-K waves, only the tail tiles
    cut into K-pieces); an int: every tile cut into `split` pieces."""
    _lib.use_hip(dy2)
    T, N = dy2.shape
    K = x2.shape[1]
    split = 0 if split is None else int(split)
    # operands only the assembly kernel takes (a token count or a forced
    # split that csrc/hip/wgrad.hip refuses): its own plan (the split divides
    # the ceil(T / 64) k-tiles), and never the HIP kernel below
    hip_takes = _wgrad_reason("wgrad_hip", g, dy2, x2, split) == 0
    nbytes = int(_lib.call_ret("toa_wgrad_workspace" if hip_takes else "toa_wgrad_asm_workspace", N, K, T, split))
    ws = _workspace(dy2.device, nbytes) if nbytes > 0 else None
    args = (_lib.ptr(dy2), dy2.stride(0), _lib.ptr(x2), x2.stride(0), _lib.ptr(g), K, _lib.ptr(ws),
            N, K, T, int(split), int(beta != 0.0), _lib.stream(dy2))
    kern = wgrad_kernel()
    if kern == "asm":
        # the gradient-norm partials stay on the token counts they were
        # measured at (both kernels' common ones); elsewhere the optimizer's
        # full pass over the gradient gives the clipping norm
        sess = _session_for(g) if _SESSIONS and hip_takes else None
        armed = sess is not None and sess.arm(g)
        try:
            rc = _lib.call_ret("toa_wgrad_asm", *args)
        finally:
            if armed:
                _lib.call("toa_wgrad_asm_set_sumsq", None)   # one-shot: never left for another launch
        if rc == 0:
            if armed:
                sess.written.add(g.data_ptr())
            return g
        if rc != HIP_ERROR_INVALID_VALUE:
            raise RuntimeError(f"toa_wgrad_asm failed: hipError {rc}")
        # a shape / layout the assembly kernel's launcher refuses (it checks
        # before launching): the HIP kernel shares its split plan and reduce
    if not hip_takes:
        raise RuntimeError(f"weight gradient {N}x{K}x{T}: csrc/hip/wgrad.hip does not take it ("
                           + _lib.shape_why(_wgrad_reason("wgrad_hip", g, dy2, x2, split)) + ") and the assembly kernel "
                           + ("refused the operands" if kern == "asm" else f"is not selected ({kern})"))
    _lib.call("toa_wgrad", *args)
    return g


def wgrad_acc_(g: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor, beta: float = 1.0):
    """g[N,K] = beta*g + dy2[M,N]^T @ x2[M,K]  (in place; g bf16 or fp32)."""
    if beta in (0.0, 1.0) and wgrad_hip_ok(g, dy2, x2):
        return wgrad_hip_(g, dy2, x2, beta)
    if dy2.is_cuda and g.dtype == torch.bfloat16 and dy2.dim() == 2 and x2.dim() == 2:
        T, N = dy2.shape
        why = f"beta={beta}, not 0 or 1" if beta not in (0.0, 1.0) else _wgrad_gate_why(g, dy2, x2)
        if not why:
            form = "wgrad_asm" if _wgrad_asm_selected() else "wgrad_hip"
            why = form + ": " + _refused(_wgrad_reason(form, g, dy2, x2), N, x2.shape[1], T)
        _fallback("wgrad", (N, x2.shape[1], T), "hipBLASLt" if _ok(dy2, x2) else "torch.mm", why)
    if (g.dtype == torch.float32 and dy2.dtype == x2.dtype == torch.bfloat16 and g.is_cuda and g.is_contiguous()
            and dy2.stride(1) == 1 and x2.stride(1) == 1 and _lib.has("toa_gemm")):
        # fp32 master-gradient accumulation (small payloads): one hipBLASLt call
        # with bf16 inputs, fp32 C/D and beta = 1 -- no bf16 temporary, cast or add
        M, N = dy2.shape
        K = x2.shape[1]
        _gemm(0, 1, K, N, M, x2, x2.stride(0), dy2, dy2.stride(0), g, K, beta)
        return g
    if not (_ok(dy2, x2) and g.is_contiguous() and g.dtype in (torch.bfloat16, torch.float32)):
        if beta == 0.0:
            g.copy_(torch.mm(dy2.t(), x2))
        elif g.dtype == dy2.dtype:
            g.addmm_(dy2.t(), x2)
        else:
            g.add_(torch.mm(dy2.t(), x2).to(g.dtype))
        return g
    M, N = dy2.shape
    K = x2.shape[1]
    _gemm(0, 1, K, N, M, x2, x2.stride(0), dy2, dy2.stride(0), g, K, beta)
    return g


def form_keys(T: int, shapes: dict) -> list:
    """The (ta, tb, m, n, k, lda, ldb, ldc, beta_nz) forms of linear layers
    `shapes` = {name: (K, N)} at T tokens (forward, dgrad, wgrad)."""
    out = []
    for name, (K, N) in shapes.items():
        out.append((name, "fwd", (1, 0, N, T, K, K, K, N, 0)))
        out.append((name, "dgrad", (0, 0, K, T, N, K, N, K, 0)))
        # dgrad on the transposed weight copy (ops/wt.py, the default): the forward's form
        out.append((name, "dgrad_wt", (1, 0, K, T, N, N, N, K, 0)))
        out.append((name, "wgrad", (0, 1, K, N, T, K, N, K, 1)))
    return out


def kernel_name(key) -> str:
    """hipBLASLt kernel a form currently runs through this layer ("" if none)."""
    if not _lib.has("toa_gemm_kernel_name"):
        return ""
    buf = ctypes.create_string_buffer(512)
    _lib.call_ret("toa_gemm_kernel_name", *key, 0, buf, 512)
    return buf.value.decode(errors="replace")


def current_algo(key) -> int:
    return _lib.call_ret("toa_gemm_current_algo", *key, 0) if _lib.has("toa_gemm_current_algo") else -1


def tune_form(key, device="cuda", exclude_streamk=False):
    """Time all hipBLASLt solutions for one form on scratch buffers
    (optionally only the non-stream-K ones)."""
    ta, tb, m, n, k, lda, ldb, ldc, beta_nz = key
    a_rows, a_cols = (m, k) if not ta else (k, m)   # column-major op(A) source dims
    b_rows, b_cols = (k, n) if not tb else (n, k)
    # column-major X (rows x cols, ld) == row-major tensor [cols, ld]
    A = torch.randn(a_cols, lda, device=device, dtype=torch.bfloat16)
    B = torch.randn(b_cols, ldb, device=device, dtype=torch.bfloat16)
    C = torch.zeros(n, ldc, device=device, dtype=torch.bfloat16)
    del a_rows, b_rows
    bi, bms, dms, nt = ctypes.c_int(-1), ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int(0)
    rc = _lib.call_ret("toa_gemm_tune", ta, tb, m, n, k, _lib.ptr(A), lda, _lib.ptr(B), ldb, _lib.ptr(C), ldc,
                       float(beta_nz), 0, _lib.stream(C), ctypes.byref(bi), ctypes.byref(bms), ctypes.byref(dms),
                       ctypes.byref(nt), int(bool(exclude_streamk)))
    if rc != 0:
        raise RuntimeError(f"toa_gemm_tune failed ({rc}) for {key}")
    return bi.value, bms.value, dms.value, nt.value


def save_table(entries: list, path: str = TABLE):
    with open(path, "w") as f:
        json.dump({"hipblaslt": hipblaslt_build(), "arch": "gfx950", "entries": entries}, f, indent=1)
