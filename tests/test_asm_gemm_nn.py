"""CPU tests of the NN-form assembly GEMMs (csrc/asm/gemm_gen.py kernel_nn:
C = X W with W [K, N] as stored -- the data gradient without a transposed
weight copy) in the functional emulator (csrc/asm/emu.py) against float64.

Tolerances are those of tests/test_asm_gemm.py and test_asm_gemm_tails.py:
``close`` at 8e-3 of the reference's largest magnitude, and more than 99.9 %
of the outputs within 2^-7 relative of the bf16-rounded reference."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "csrc", "asm"))

import emu  # noqa: E402
import gemm_gen  # noqa: E402
import host_args  # noqa: E402
import wgrad_gen  # noqa: E402

from test_asm_gemm import TEXT, bf16, close, tof  # noqa: E402  (the TN tests' helpers and tolerance)
from test_asm_gemm_tails import GUARD, SENTINEL, guarded  # noqa: E402


def run_all(kernel, karg, nwg, mem, **kw):
    e = emu.Emu(TEXT, kernel, **kw)
    for wg in range(nwg):
        e.run(karg, wg, mem)
    return e


def padded(a, extra):
    """`a` as the leading columns of a buffer with `extra` more (NaN) columns
    per row: (the buffer, the row stride in bytes)."""
    buf = np.full((a.shape[0], a.shape[1] + extra), 0x7FC0, np.uint16)
    buf[:, :a.shape[1]] = a
    return buf, 2 * buf.shape[1]


def plain(X, W, M=None, ldw_extra=0, c_rows=None, **kw):
    """C = X W on toa_gemm_nn_asm_plain; X [rows, K], W [K, N]."""
    rows, K = X.shape
    N = W.shape[1]
    tm = -(-rows // 256)
    Wb, ldw = padded(W, ldw_extra)
    mem = emu.Memory()
    ax, aw = mem.add(X), mem.add(Wb)
    Cb = np.zeros((rows, N), np.uint16) if c_rows is None else c_rows
    ac = mem.add(Cb)
    karg = host_args.pack_nn(ax, aw, ac, 0, 2 * K, ldw, 2 * N, 0, K, tm, N // 256, M=M)
    e = run_all("toa_gemm_nn_asm_plain", karg, tm * (N // 256), mem, **kw)
    return mem.bufs[2][1].view(np.uint16).reshape(Cb.shape), e


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (256, 256, 192), (512, 512, 320)])
def test_nn_plain_whole_tiles_emulated(M, N, K):
    """0, 1 and 3 main-loop iterations, strict bounds: W with a padded row
    stride and a per-row ramp (a wrong k row or column shows), X asymmetric."""
    rng = np.random.default_rng(M + N + K)
    X = bf16(rng.standard_normal((M, K)) * (1 + np.arange(K) / K) + 0.25)
    W = bf16(rng.standard_normal((K, N)) + np.arange(K)[:, None] / K)
    C, _ = plain(X, W, ldw_extra=24)
    ref = tof(X) @ tof(W)
    close(tof(C), ref)
    assert np.mean(np.abs(tof(C) - tof(bf16(ref))) <= np.abs(ref) * 2 ** -7) > 0.999


def test_nn_k_pairing_exact():
    """X[m][k] = (k == m % K): C's row m is W's row m % K bit for bit, so the
    k indices of a lane's X fragment are those of its W fragment."""
    M, N, K = 256, 256, 128
    rng = np.random.default_rng(7)
    W = bf16(rng.standard_normal((K, N)))
    X = np.zeros((M, K), np.uint16)
    X[np.arange(M), np.arange(M) % K] = 0x3F80          # bf16 1.0
    C, _ = plain(X, W, ldw_extra=8)
    assert np.array_equal(C, W[np.arange(M) % K])


@pytest.mark.parametrize("M", [300, 1])
def test_nn_plain_m_tail_emulated(M):
    """X has exactly M rows; the rows of the last tile row past M load 0 and
    their stores are dropped (N / 8 sixteen-byte stores per dead row): C's
    sentinel rows after row M come back bit-identical."""
    N, K = 256, 128
    rng = np.random.default_rng(M + N + K)
    X = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((K, N)))
    Cb, e = plain(X, W, M=M, c_rows=guarded(M, N), hw_bounds=True)
    ref = tof(X) @ tof(W)
    close(tof(Cb[:M]), ref)
    assert np.mean(np.abs(tof(Cb[:M]) - tof(bf16(ref))) <= np.abs(ref) * 2 ** -7) > 0.999
    assert (Cb[M:] == SENTINEL).all()
    dead = 256 * -(-M // 256) - M
    assert e.oob_loads > 0 and e.oob_stores == dead * N // 8


def test_nn_w_window_stays_in_range():
    """Strict bounds, M a multiple of 256, W of exactly K rows with nothing
    behind it: no W access leaves its K rows (an access past the resource or
    outside every buffer raises)."""
    M, N, K = 256, 512, 192
    rng = np.random.default_rng(11)
    X, W = bf16(rng.standard_normal((M, K))), bf16(rng.standard_normal((K, N)))
    C, e = plain(X, W)
    close(tof(C), tof(X) @ tof(W))
    assert e.oob_loads == 0 and e.oob_stores == 0


def test_nn_swiglu_bwd_m_tail_emulated():
    """The down projection's data gradient on Wd [D, F] as stored, M = 300
    (the float64 formulas of test_tn_swiglu_bwd_m_tail_emulated)."""
    rng = np.random.default_rng(43)
    M, F, K = 300, 256, 128
    D = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((K, F)) * 0.1)
    GU = bf16(rng.standard_normal((M, 2 * F)))     # exactly M rows: the dead rows' gate / up read 0
    mem = emu.Memory()
    ad, aw, adg, agu = mem.add(D), mem.add(W), mem.add(guarded(M, 2 * F)), mem.add(GU)
    karg = host_args.pack_nn(ad, aw, adg, agu, 2 * K, 2 * F, 4 * F, 4 * F, K, 2, F // 256, fc_b=2 * F, M=M)
    run_all("toa_gemm_nn_asm_swiglu_bwd", karg, 2 * (F // 256), mem, hw_bounds=True)
    raw = mem.bufs[2][1].view(np.uint16).reshape(M + GUARD, 2 * F)
    dgu = tof(raw[:M])
    ds = tof(bf16(tof(D) @ tof(W)))
    g, u = tof(GU[:, :F]), tof(GU[:, F:])
    sg = 1 / (1 + np.exp(-g))
    close(dgu[:, :F], ds * u * sg * (1 + g * (1 - sg)))
    close(dgu[:, F:], ds * g * sg)
    assert (raw[M:] == SENTINEL).all()


@pytest.mark.parametrize("B,S,H", [(2, 256, 4), (1, 512, 2)])
def test_nn_delta_epilogue_emulated(B, S, H):
    """The output projection's data gradient on Wo as stored with the attention
    delta fused: C as the plain NN kernel writes it (bit for bit), ndelta[b, h,
    s] = -sum_d bf16(C)[t][128 h + d] O[t][128 h + d] (the TN delta test)."""
    rng = np.random.default_rng(B * S + H)
    K = 128
    M, N = B * S, H * 128
    X = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((K, N)) * 0.3)
    O = bf16(rng.standard_normal((M, N)))
    outs = []
    for name in ("toa_gemm_nn_asm_plain", "toa_gemm_nn_asm_delta"):
        mem = emu.Memory()
        ax, aw, ac = mem.add(X), mem.add(W), mem.add(np.zeros((M, N), np.uint16))
        ao = mem.add(O)
        ad = mem.add(np.full(B * H * S, np.nan, np.float32))
        delta = name.endswith("delta")
        karg = bytearray(host_args.pack_nn(ax, aw, ac, ao, 2 * K, 2 * N, 2 * N, 0, K, M // 256, N // 256,
                                           fw_b=S if delta else 0, fc_b=H if delta else 0))
        if delta:
            karg[88:96] = int(ad).to_bytes(8, "little")
        run_all(name, bytes(karg), (M // 256) * (N // 256), mem)
        outs.append((mem.bufs[2][1].copy(), mem.bufs[4][1].view(np.float32).copy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    C = tof(outs[1][0].view(np.uint16).reshape(M, N))
    close(C, tof(X) @ tof(W))
    ref = -(C * tof(O)).reshape(B, S, H, 128).sum(-1).transpose(0, 2, 1).reshape(-1)
    got = outs[1][1].astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-6, np.abs(got - ref).max()


def nn_read_addrs():
    """Per transposed W read the NN loop issues: ((hi, odd fragment, immediate,
    wave column half), the 64 lanes' LDS byte addresses inside the W image),
    from the kernel's own prologue run in the emulator and the base registers
    and immediates of its read instructions."""
    e = emu.Emu(TEXT, "toa_gemm_nn_asm_plain")
    reads = {}
    for op, args, mods in e.prog:
        if op == "ds_read_b64_tr_b16":
            off = next(int(m.split(":")[1]) for m in mods if m.startswith("offset:"))
            reads.setdefault((args[1], off), None)
    kind = {f"v{gemm_gen.V_RW}": (False, False), f"v{gemm_gen.V_RWH}": (True, False),
            f"v{gemm_gen.V_RWO}": (False, True), f"v{gemm_gen.V_RWHO}": (True, True)}
    assert {reg for reg, _ in reads} == set(kind)
    M, N, K = 256, 256, 128
    mem = emu.Memory()
    ax, aw, ac = (mem.add(np.zeros((M, K), np.uint16)), mem.add(np.zeros((K, N), np.uint16)),
                  mem.add(np.zeros((M, N), np.uint16)))
    karg = host_args.pack_nn(ax, aw, ac, 0, 2 * K, 2 * N, 2 * N, 0, K, 1, 1)
    e.mem, e.kernarg, e.lds = mem, karg, np.zeros(160 * 1024, np.uint8)
    out = []
    for wid in range(4):
        w = emu.Wave(wid)
        w.s[2] = 0
        w.v[0] = np.arange(64, dtype=np.uint32) + 64 * wid
        while e.step(w) != "barrier":       # the prologue, up to the first barrier: the read bases are set
            pass
        for (reg, off) in reads:
            base = w.v[int(reg[1:])].astype(np.int64)
            out.append((kind[reg] + (off, wid >> 1), base + off - gemm_gen.HALF))
    return out


def test_nn_w_reads_hit_the_image_and_are_conflict_free():
    """Every transposed read of the NN loop lands on wgrad_gen.pos of the row
    and columns its accumulator layout needs -- lane (g, q, p) of fragment i:
    row 8 g + q (+4, +32), chunk 4 (i >> 1) + p of the wave's 16, its half
    (i & 1) ^ par(p) with par(p) = (p & 1) ^ (p >> 1) -- as base + immediate,
    and is conflict-free by the argument of tests/test_asm_wgrad.py: within
    each 32-lane group of a ds_read_b64_tr_b16 no two lanes' dwords share one
    of the 64 banks."""
    seen = set()
    for (hi, odd, off, wn), addrs in nn_read_addrs():
        sub, rest = divmod(off, wgrad_gen.SUB1)
        assert rest % 128 == 0 and rest // 128 < 4 and sub in (0, 1)
        i = 2 * (rest // 128) + odd
        assert off == gemm_gen.nn_frag_offset(i, sub)
        seen.add((i, sub, hi, wn))
        for lane in range(64):
            g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
            row = 32 * sub + 8 * g + q + (4 if hi else 0)
            half = (i & 1) ^ (p & 1) ^ (p >> 1)
            col = 128 * wn + 32 * (i >> 1) + 8 * p + 4 * half
            assert addrs[lane] == wgrad_gen.pos(row, col >> 3) + 2 * (col & 7), (i, sub, hi, wn, lane)
        for grp in (range(0, 32), range(32, 64)):
            banks = {}
            for lane in grp:
                for d in range(2):
                    banks.setdefault((addrs[lane] // 4 + d) % 64, set()).add(addrs[lane] // 4 + d)
            assert len(banks) == 64 and max(len(v) for v in banks.values()) == 1, (i, sub, hi, wn)
    assert len(seen) == 8 * 2 * 2 * 2


def test_nn_fragment_pairs_come_out_in_column_order():
    """Lane groups 1 and 2 hold fragments 2p, 2p + 1 the other way round; the
    epilogue's two EXEC-masked passes order them: with X = the shifted
    identity every stored 16-byte group is W's, column for column (checked bit
    for bit by test_nn_k_pairing_exact); here, that EXEC is all ones again
    wherever the kernel issues anything but an accumulator read."""
    e = emu.Emu(TEXT, "toa_gemm_nn_asm_delta")
    masked = False
    for op, args, mods in e.prog:
        if op == "s_mov_b64" and args[0] == "exec":
            masked = args[1] != "-1"
        else:
            assert not masked or op == "v_accvgpr_read_b32", op


def test_nn_argument_guard():
    """An m that does not fit tiles_m ends the workgroup before any access."""
    mem = emu.Memory()
    ac = mem.add(guarded(256, 256))
    for M in (513, 256):                            # tiles_m = 2 needs 256 < m <= 512
        karg = bytearray(host_args.pack_nn(0, 0, ac, 0, 256, 512, 512, 0, 128, 2, 1))
        karg[92:96] = M.to_bytes(4, "little")
        for name in ("toa_gemm_nn_asm_plain", "toa_gemm_nn_asm_swiglu_bwd"):
            emu.Emu(TEXT, name, hw_bounds=True).run(bytes(karg), 0, mem)
    # one k-tile (K = 64): below the pipeline's two stages
    karg = host_args.pack_nn(0, 0, ac, 0, 128, 512, 512, 0, 64, 1, 1)
    emu.Emu(TEXT, "toa_gemm_nn_asm_plain", hw_bounds=True).run(karg, 0, mem)
    assert (mem.bufs[0][1].view(np.uint16) == SENTINEL).all()


def test_tn_and_wgrad_text_unchanged():
    """The TN kernels' and the weight-gradient kernel's generated bodies are
    those of before the NN form (sha256 per kernel, recorded from that
    generator)."""
    golden = json.load(open(os.path.join(HERE, "golden", "asm_text_sha256.json")))
    lines = TEXT.split("\n")
    names = [ln[:-1] for ln in lines if re.match(r"^(toa_gemm_tn_asm_\w+|toa_wgrad_nt_asm):$", ln)]
    assert names == [g["name"] for g in golden]
    for g in golden:
        s = lines.index(g["name"] + ":")
        e = next(i for i in range(s, len(lines)) if lines[i].startswith(f".size {g['name']},"))
        body = "\n".join(lines[s:e + 1])
        assert hashlib.sha256(body.encode()).hexdigest() == g["sha256"], g["name"]
    assert {"toa_gemm_nn_asm_plain", "toa_gemm_nn_asm_swiglu_bwd", "toa_gemm_nn_asm_delta"} == \
        set(re.findall(r"^(toa_gemm_nn_asm_\w+):", TEXT, re.M))


def test_nn_lds_budget_and_descriptor():
    stage, lds = gemm_gen.nn_layout()
    assert (stage, lds) == (gemm_gen.HALF + wgrad_gen.OPER, 145280) and lds + 1024 <= 160 * 1024
    sizes = dict(re.findall(r"\.amdhsa_kernel (toa_gemm_nn_asm_\w+)\n\s+\.amdhsa_group_segment_fixed_size (\d+)", TEXT))
    assert sizes == {"toa_gemm_nn_asm_plain": "145280", "toa_gemm_nn_asm_swiglu_bwd": "145280",
                     "toa_gemm_nn_asm_delta": "146304"}


def test_pack_nn_bytes():
    """pack_nn follows KARG (ldw = W's row stride, ktiles = K / 64, tiles_n =
    N / 256); pack / pack_nt give the blocks recorded in
    test_kernarg_bytes_of_whole_tile_shapes_unchanged."""
    import struct

    K_ = gemm_gen.KARG
    b = host_args.pack_nn(1 << 32, 2 << 32, 3 << 32, 4 << 32, 384, 1040, 1024, 2048, 192, 2, 2, fc_b=512, M=300)
    assert len(b) == gemm_gen.KARG_BYTES
    assert struct.unpack_from("<QQQQ", b, K_["X"]) == (1 << 32, 2 << 32, 3 << 32, 4 << 32)
    assert struct.unpack_from("<IIII", b, K_["ldx"]) == (384, 1040, 1024, 2048)
    assert struct.unpack_from("<III", b, K_["ktiles"]) == (3, 2, 2)
    assert struct.unpack_from("<II", b, K_["xq"]) == (0, 4)
    assert struct.unpack_from("<II", b, K_["fw"]) == (0, 512)
    assert struct.unpack_from("<I", b, K_["map"]) == (gemm_gen.MAP_DEFAULT,)
    assert struct.unpack_from("<II", b, K_["phase"]) == (0, 300)
    a = host_args.pack(1 << 32, 2 << 32, 3 << 32, 4 << 32, 256, 256, 512, 0, 128, 2, 1)
    assert a.hex() == (
        "0000000001000000" "0000000002000000" "0000000003000000" "0000000004000000"
        "00010000" "00010000" "00020000" "00000000"
        "02000000" "02000000" "01000000" "00000000" "02000000" "08000000"
        "00000000" "00000000" "02000000" "00000000" "00000000" "00000000")
    t = host_args.pack_nt(1 << 32, 2 << 32, 3 << 32, 0, 512, 512, 512, 0, 256, 1, 1, 1, 1)
    assert t.hex() == (
        "0000000001000000" "0000000002000000" "0000000003000000" "0000000000000000"
        "00020000" "00020000" "00020000" "00000000"
        "04000000" "01000000" "01000000" "01000000" "00000000" "01000000"
        "00000000" "00000000" "03000000" "00000000" "0000000000000000")
