"""csrc/hip/gemm_asm_shapes.h, the one statement of what each assembly GEMM
form takes: its boundary table (csrc/hip/tests/gemm_shapes_selftest.cc, built
alone under ASan + UBSan and run as its own process) and the form names
ops/_lib.py passes to toa_gemm_shape_check."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "csrc", "hip")


def test_boundary_table_asan_ubsan(tmp_path):
    exe = str(tmp_path / "gemm_shapes_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(HIP, "tests", "gemm_shapes_selftest.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "gemm shapes selftest OK" in r.stdout


def test_python_form_names_follow_the_header():
    from tf_operator_amd.ops import _lib

    with open(os.path.join(HIP, "gemm_asm_shapes.h")) as f:
        body = re.search(r"enum Form \{(.*?)\};", f.read(), re.S).group(1)
    names = re.findall(r"^\s*F_(\w+)", body, re.M)
    assert names[-1] == "COUNT"
    assert tuple(n.lower() for n in names[:-1]) == _lib.SHAPE_FORMS
    assert len(_lib._SIGS["toa_gemm_shape_check"]) == 18


def test_every_ctypes_signature_names_an_export():
    """Every launcher ops/_lib.py declares argument types for is exported by
    libtoa_hip.so: _load skips a missing one silently, so a row left behind
    when an entry point is deleted would otherwise go unnoticed."""
    from tf_operator_amd.ops import _lib

    assert _lib.available(), _lib.load_error()
    missing = sorted(n for n in list(_lib._SIGS) + sorted(_lib._TYPED_ELSEWHERE) if not hasattr(_lib.lib(), n))
    assert not missing, missing
