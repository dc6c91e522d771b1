"""CPU tests of the assembly GEMMs' token tails (csrc/asm/gemm_gen.py kernarg
"m", csrc/asm/wgrad_gen.py kernarg "t") in the functional emulator's
hardware range-check mode (csrc/asm/emu.py ``hw_bounds``): per lane, a load
past num_records reads 0 and a store past it is dropped.

TN kernels (forward / data gradient): M is the row count of X and C, the last
tile row's resources end at row M.  X has exactly M rows here, so a window
that reaches past them fails with "outside every buffer"; C carries sentinel
rows after row M that must come back bit-identical.

NT kernel (weight gradient): T is the reduction length, the rows of the last
64-row tile past T must add exactly 0 -- also when NaNs lie behind the
operands in memory.

Tolerance: tests/test_asm_gemm.py's ``close`` (8e-3 of the reference's
largest magnitude, against float64)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "csrc", "asm"))

import emu  # noqa: E402
import gemm_gen  # noqa: E402
import host_args  # noqa: E402
import wgrad_gen  # noqa: E402

TEXT = gemm_gen.generate()
WTEXT = wgrad_gen.generate()
GUARD = 8                      # sentinel rows after row M
SENTINEL = 0x5A5A
NAN = 0x7FC0                   # bf16 quiet NaN


def bf16(x):
    return emu.bf16_rne(np.asarray(x, np.float32)).astype(np.uint16)


def tof(b):
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def close(got, ref, tol=8e-3):
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err < tol, err


def guarded(M, cols):
    return np.full((M + GUARD, cols), SENTINEL, np.uint16)


def run_tn(kernel, karg, nwg, mem, **kw):
    e = emu.Emu(TEXT, kernel, hw_bounds=True, **kw)
    for wg in range(nwg):
        e.run(karg, wg, mem)
    return e


def out_rows(mem, idx, M, cols):
    """(the M live rows as float64, the sentinel rows' bits) of buffer idx."""
    raw = mem.bufs[idx][1].view(np.uint16).reshape(M + GUARD, cols)
    return tof(raw[:M]), raw[M:]


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1, 256, 128), (520, 512, 192)])
def test_tn_plain_m_tail_emulated(M, N, K):
    rng = np.random.default_rng(M + N + K)
    X = bf16(rng.standard_normal((M, K)))          # exactly M rows
    W = bf16(rng.standard_normal((N, K)))
    tm = -(-M // 256)
    mem = emu.Memory()
    ax, aw, ac = mem.add(X), mem.add(W), mem.add(guarded(M, N))
    karg = host_args.pack(ax, aw, ac, 0, 2 * K, 2 * K, 2 * N, 0, K, tm, N // 256, M=M)
    e = run_tn("toa_gemm_tn_asm_plain", karg, tm * (N // 256), mem)
    C, guard = out_rows(mem, 2, M, N)
    ref = tof(X) @ tof(W).T
    close(C, ref)
    assert np.mean(np.abs(C - tof(bf16(ref))) <= np.abs(ref) * 2 ** -7) > 0.999
    assert (guard == SENTINEL).all()
    dead = 256 * tm - M
    assert (e.oob_loads > 0) == (dead > 0) and (e.oob_stores > 0) == (dead > 0)
    # every dead row's 16-byte stores were dropped, nothing else: N / 8 per row
    assert e.oob_stores == dead * N // 8


def test_tn_resadd_m_tail_emulated():
    rng = np.random.default_rng(41)
    M, N, K = 300, 256, 128
    X = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((N, K)) * 0.2)
    R = bf16(rng.standard_normal((M, N)))          # exactly M rows: the dead rows' loads read 0
    mem = emu.Memory()
    ax, aw, ac, ar_ = mem.add(X), mem.add(W), mem.add(guarded(M, N)), mem.add(R)
    karg = host_args.pack(ax, aw, ac, ar_, 2 * K, 2 * K, 2 * N, 0, K, 2, N // 256, M=M)
    run_tn("toa_gemm_tn_asm_resadd", karg, 2 * (N // 256), mem)
    C, guard = out_rows(mem, 2, M, N)
    close(C, tof(X) @ tof(W).T + tof(R))
    assert (guard == SENTINEL).all()


def test_tn_swiglu_fwd_m_tail_emulated():
    rng = np.random.default_rng(42)
    M, F, K = 300, 256, 128
    X = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((2 * F, K)) * 0.1)
    mem = emu.Memory()
    ax, aw = mem.add(X), mem.add(W)
    ag, as_ = mem.add(guarded(M, 2 * F)), mem.add(guarded(M, F))
    karg = host_args.pack(ax, aw, ag, as_, 2 * K, 2 * K, 4 * F, 2 * F, K, 2, F // 128, fw_b=F * 2 * K, fc_b=2 * F,
                          M=M)
    run_tn("toa_gemm_tn_asm_swiglu_fwd", karg, 2 * (F // 128), mem)
    gu, guard_gu = out_rows(mem, 2, M, 2 * F)
    s, guard_s = out_rows(mem, 3, M, F)
    ref = tof(X) @ tof(W).T
    close(gu, ref)
    g, u = tof(bf16(ref[:, :F])), tof(bf16(ref[:, F:]))
    close(s, g / (1 + np.exp(-g)) * u)
    assert (guard_gu == SENTINEL).all() and (guard_s == SENTINEL).all()


def test_tn_swiglu_bwd_m_tail_emulated():
    rng = np.random.default_rng(43)
    M, F, K = 300, 256, 128
    D = bf16(rng.standard_normal((M, K)))
    W = bf16(rng.standard_normal((F, K)) * 0.1)
    GU = bf16(rng.standard_normal((M, 2 * F)))     # exactly M rows: the dead rows' gate / up read 0
    mem = emu.Memory()
    ad, aw, adg, agu = mem.add(D), mem.add(W), mem.add(guarded(M, 2 * F)), mem.add(GU)
    karg = host_args.pack(ad, aw, adg, agu, 2 * K, 2 * K, 4 * F, 4 * F, K, 2, F // 256, fc_b=2 * F, M=M)
    run_tn("toa_gemm_tn_asm_swiglu_bwd", karg, 2 * (F // 256), mem)
    dgu, guard = out_rows(mem, 2, M, 2 * F)
    ds = tof(bf16(tof(D) @ tof(W).T))
    g, u = tof(GU[:, :F]), tof(GU[:, F:])
    sg = 1 / (1 + np.exp(-g))
    close(dgu[:, :F], ds * u * sg * (1 + g * (1 - sg)))
    close(dgu[:, F:], ds * g * sg)
    assert (guard == SENTINEL).all()


def run_wgrad(T, split, padded):
    """dW [256, 256] = A[:T]^T B[:T].  padded: the operands are the first T
    rows of buffers whose later rows are bf16 NaN; else exactly T rows."""
    M = N = 256
    rng = np.random.default_rng(T)
    A = bf16(rng.standard_normal((T, M)))
    B = bf16(rng.standard_normal((T, N)))
    pad = 70 if padded else 0                      # past the end of the last 64-row tile
    Ab, Bb = (np.concatenate([x, np.full((pad, x.shape[1]), NAN, np.uint16)]) for x in (A, B))
    full, sp = host_args.wgrad_plan(M, N, T) if split is None else (0, split)
    rem = 1 - full
    mem = emu.Memory()
    aa, ab, ac = mem.add(Ab), mem.add(Bb), mem.add(np.zeros((M, N), np.uint16))
    aw = mem.add(np.zeros(max(1, sp * rem) * 65536, np.float32))
    karg = host_args.pack_nt(aa, ab, ac, aw, 2 * M, 2 * N, 2 * N, 0, 0, 1, 1, full, sp, T=T)
    e = emu.Emu(WTEXT, "toa_wgrad_nt_asm", hw_bounds=True)
    for wg in range(full + rem * sp):
        e.run(karg, wg, mem)
    assert e.oob_loads > 0 and e.oob_stores == 0
    if sp > 1:
        got = mem.bufs[3][1].view(np.float32).reshape(sp, M, N).astype(np.float64).sum(0)
    else:
        got = tof(mem.bufs[2][1].view(np.uint16).reshape(M, N))
    return got, tof(A).T @ tof(B)


@pytest.mark.parametrize("padded", [False, True], ids=["exact", "nan_padded"])
@pytest.mark.parametrize("T,split", [(200, None), (129, None), (200, 2)])
def test_wgrad_t_tail_emulated(T, split, padded):
    got, ref = run_wgrad(T, split, padded)
    assert np.isfinite(got).all()
    close(got, ref)


def test_wgrad_plan_tail_splits_divide_the_k_tiles():
    # shapes accepted before: the plan of csrc/hip/wgrad.hip's wg_plan, unchanged
    assert host_args.wgrad_plan(4096, 4096, 8192) == (256, 1)
    assert host_args.wgrad_plan(4096, 1024, 8192) == (0, 4)
    assert host_args.wgrad_plan(4096, 1024, 8192 - 128) == (0, 3)
    assert host_args.wgrad_plan(4096, 1024, 8192 - 64) == (64, 1)     # 127 k-tiles, K % 128 != 0: no split
    # tails: the largest split in 2..4 that divides ceil(T / 64) and leaves >= 512 rows a piece
    assert host_args.wgrad_plan(4096, 1024, 24000) == (64, 1)         # 375 whole k-tiles: the old rule
    assert host_args.wgrad_plan(4096, 1024, 24008) == (0, 4)          # 376 k-tiles
    assert host_args.wgrad_plan(4096, 1024, 23990) == (0, 3)          # 375 k-tiles
    assert host_args.wgrad_plan(4096, 1024, 8100) == (64, 1)          # 127 k-tiles: prime
    assert host_args.wgrad_plan(4096, 1024, 1000) == (64, 1)          # 16 k-tiles, but 1000 / 2 < 512
    for T in (24008, 23990, 8100, 4001, 1537):
        full, sp = host_args.wgrad_plan(4096, 1024, T)
        assert -(-T // 64) % sp == 0 and -(-T // 64) // sp >= 2


def test_kernarg_bytes_of_whole_tile_shapes_unchanged():
    """pack / pack_nt without M / T: byte for byte the blocks of before the
    tails (recorded from that generator's host_args)."""
    a = host_args.pack(1 << 32, 2 << 32, 3 << 32, 4 << 32, 256, 256, 512, 0, 128, 2, 1)
    assert a.hex() == (
        "0000000001000000" "0000000002000000" "0000000003000000" "0000000004000000"
        "00010000" "00010000" "00020000" "00000000"
        "02000000" "02000000" "01000000" "00000000" "02000000" "08000000"
        "00000000" "00000000" "02000000" "00000000" "00000000" "00000000")
    b = host_args.pack_nt(1 << 32, 2 << 32, 3 << 32, 0, 512, 512, 512, 0, 256, 1, 1, 1, 1)
    assert b.hex() == (
        "0000000001000000" "0000000002000000" "0000000003000000" "0000000000000000"
        "00020000" "00020000" "00020000" "00000000"
        "04000000" "01000000" "01000000" "01000000" "00000000" "01000000"
        "00000000" "00000000" "03000000" "00000000" "0000000000000000")
    # and the new words sit where the old blocks had zeros
    assert host_args.pack(0, 0, 0, 0, 256, 256, 512, 0, 128, 2, 1, M=300)[92:96] == (300).to_bytes(4, "little")
    t = host_args.pack_nt(0, 0, 0, 0, 512, 512, 512, 0, 0, 1, 1, 1, 1, T=200)
    assert t[48:52] == (4).to_bytes(4, "little") and t[72:76] == (200).to_bytes(4, "little")


def test_strict_mode_still_raises_on_an_out_of_range_access():
    """The emulator's default: any access past num_records is an error, so
    every other test keeps its bounds check."""
    rng = np.random.default_rng(5)
    M, N, K = 300, 256, 128
    X, W = bf16(rng.standard_normal((M, K))), bf16(rng.standard_normal((N, K)))
    mem = emu.Memory()
    ax, aw, ac = mem.add(X), mem.add(W), mem.add(guarded(M, N))
    karg = host_args.pack(ax, aw, ac, 0, 2 * K, 2 * K, 2 * N, 0, K, 2, 1, M=M)
    with pytest.raises(IndexError, match="past num_records"):
        emu.Emu(TEXT, "toa_gemm_tn_asm_plain").run(karg, 1, mem)
    assert (mem.bufs[2][1].view(np.uint16).reshape(M + GUARD, N)[M:] == SENTINEL).all()


def test_kernels_end_before_any_access_on_a_row_count_outside_their_tiles():
    """m / t that do not fit tiles_m / the k-tiles (a block the host never
    packs) end the workgroup in the argument guard."""
    mem = emu.Memory()
    ac = mem.add(guarded(256, 256))
    for M in (513, 256):                            # tiles_m = 2 needs 256 < m <= 512
        karg = bytearray(host_args.pack(0, 0, ac, 0, 256, 256, 512, 0, 128, 2, 1))
        karg[92:96] = M.to_bytes(4, "little")
        emu.Emu(TEXT, "toa_gemm_tn_asm_plain", hw_bounds=True).run(bytes(karg), 0, mem)
    for T in (257, 192):                            # 4 k-tiles need 192 < t <= 256
        karg = bytearray(host_args.pack_nt(0, 0, ac, 0, 512, 512, 512, 0, 256, 1, 1, 1, 1))
        karg[72:76] = T.to_bytes(4, "little")
        emu.Emu(WTEXT, "toa_wgrad_nt_asm", hw_bounds=True).run(bytes(karg), 0, mem)
    assert (mem.bufs[0][1].view(np.uint16) == SENTINEL).all()
