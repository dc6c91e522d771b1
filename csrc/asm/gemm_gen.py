#!/usr/bin/env python3
"""Generator of the hand-written gfx950 (CDNA4) assembly GEMM kernels.

    python csrc/asm/gemm_gen.py OUT.s

Emits one code object source with the forward / data-gradient GEMM of the
training step in the "TN" form (both operands contiguous along the
reduction), written instruction by instruction rather than through hipcc:

    C[m][n] = sum_k X[m][k] * W[n][k]      bf16 in, fp32 accumulate

Why assembly: the one-wave-per-SIMD schedule that gives the lowest energy
per MFMA (128 x 128 of C per wave, a third fewer LDS bytes per MFMA than
128 x 64) needs its latency hidden by software pipelining -- fragment reads
for the next k-step issued between the current k-step's MFMAs, the global
prefetch two tiles ahead, accumulators that never leave the AGPRs.  hipcc
did not hold that schedule (round 3: `gemm_tn4w_kernel` shuttled
accumulators and waited `vmcnt(0)`, 0.96-1.02 PF/s; docs/kernels.md).

Structure (every number below is what the generator emits):

  workgroup   256 threads = 4 waves (one per SIMD), tile 256 x 256, BK = 64
  wave        (wm, wn) = (wave & 1, wave >> 1): 128 rows of X x 128 rows of W
              = 8 x 8 tiles of v_mfma_f32_16x16x32_bf16, 256 AGPR accumulators
  LDS         two stages of 66 KiB (X half, W half).  A half is 32 "lines" of
              1056 B (1024 B of data + 32 B pad): line i of the wave-row block
              holds tile rows i, i+16, ..., i+112 (128 B = 64 k each).  A
              fragment read (ds_read_b128: lane l reads line l & 15, 16-B
              chunk l >> 4) is serviced in 4 lane groups of 16; with lines 264
              dwords = 8 banks apart every group covers the 64 banks once, 4
              LDS cycles per read (a 16-B pad, 4 banks apart, collides chunk 1
              of line i with chunk 0 of line i + 1 inside a group: 8 cycles)
  staging     LDS-DMA (`buffer_load_dwordx4 ... lds`): one instruction per
              wave fills one line = 8 rows x 128 B (8 whole cache lines), the
              swizzle-free image needs no source permutation.  16 DMA
              instructions per wave per 64-k tile, bounded by the buffer
              resource (num_records): an address past the tensor reads 0
  pipeline    tile t+2 is staged into the stage tile t just vacated (two
              stages, prefetch distance two), k-step halves of 32:
                phase 1: 64 MFMAs on sub-step 0 fragments; between them the
                         sub-step 1 fragment reads of the same stage, then a
                         barrier per operand half after which that half's
                         DMA for tile t+2 starts
                phase 2: 64 MFMAs on sub-step 1; the rest of the DMA, one
                         counted vmcnt (tile t+1 landed) + barrier, then the
                         next tile's sub-step 0 fragment reads
              three barriers per 64-k tile, vmcnt never 0 inside the loop
  epilogue    accumulators -> bf16 (v_cvt_pk_bf16_f32) -> buffer stores, each
              lane 4 consecutive columns of one row (the W fragment is the
              MFMA's A operand); fused variants:
                plain        C
                swiglu_fwd   gate|up projection: the workgroup's 256 W rows are
                             128 gate rows and the SAME 128 up rows (W keeps
                             its [gate; up] layout); writes gu and
                             s = silu(gate) * up
                swiglu_bwd   down-projection data gradient: ds is never stored;
                             reads gu, writes dgu = [ds*up*silu'(g) | ds*silu(g)]
  grid        one workgroup per tile, XCD-aware: the 8 XCDs get contiguous
              ranges of the tile order, which walks groups of 8 row tiles
              across the column tiles (a group's X strips + the current W
              strip stay in the XCD's L2)

Reference anchor: SURVEY.md K1/K2/K19 and section 7.1 item 5 (MFMA tiles with
fused epilogues); the reference itself has no kernels
(/root/reference/examples/v1/dist-mnist/dist_mnist.py:188-189 is the GEMM +
bias + activation these generalise).  This file is not derived from any
library source: the schedule class (4 waves x 128 x 128, prefetch distance
two) is the one docs/kernels.md and profiles/r3_tn_pmc measured as the
energy-efficient form on MI355X.
"""
from __future__ import annotations

import sys

LINE = 1056              # one LDS line: 8 tile rows x 128 B + 32 B pad
HALF = 32 * LINE         # 256 rows of one operand = 33792 B
STAGE = 2 * HALF         # X half + W half = 67584 B
LDS_BYTES = 2 * STAGE    # 135168 B
KARG_BYTES = 96

# kernarg layout (byte offsets; mirrored by csrc/hip/gemm_asm.hip).  `map`:
# the tile order, bits [3:0] log2 of the group size, bit 4 set = groups of
# COLUMN tiles walk the row tiles (clear: groups of row tiles walk the
# column tiles); `grid`: a persistent kernel's workgroup count.
KARG = {
    "X": 0, "W": 8, "C": 16, "S": 24,
    "ldx": 32, "ldw": 36, "ldc": 40, "lds": 44,
    "ktiles": 48, "tiles_m": 52, "tiles_n": 56, "xq": 60, "xr": 64,
    "per_group": 68, "fw": 72, "fc": 76, "map": 80, "grid": 84, "phase": 88, "m": 92,
}
# `m`: the rows of X / C (0 = tiles_m whole tiles).  tiles_m = ceil(m / 256);
# the last tile row's X / C / S resources end at row m, so the hardware's
# range check zero-fills the loads and drops the stores of the rows past it
# (the delta kernel's bytes 88..95 are a pointer: whole tiles only).
MAP_WALK_COLS = 16
MAP_DEFAULT = 2          # groups of 4 row tiles walk the column tiles

EPIS = ("plain", "swiglu_fwd", "swiglu_bwd", "rope", "delta", "resadd")

# ---------------------------------------------------------------- registers
# SGPRs: s[0:1] kernarg pointer, s2 workgroup id (the descriptor's order)
S_ARGS = 4          # s[4:23]: the 80 B of kernarg
S_X, S_W, S_C, S_S = 4, 6, 8, 10
S_LDX, S_LDW, S_LDC, S_LDS = 12, 13, 14, 15
S_KT, S_TM_N, S_TN_N, S_XQ = 16, 17, 18, 19
S_XR, S_M, S_FW, S_FC = 20, 21, 22, 23   # S_M: rows of X / C (kernarg `m`; the per_group word is not used)
S_TILE, S_TM, S_TN = 24, 25, 26
S_T0, S_T1, S_T2, S_T3 = 27, 28, 29, 30
S_PHASE = 31        # kernarg `phase` word (start offsets of the first wave, phase_delay)
SRD_X, SRD_W, SRD_C, SRD_S = 32, 36, 40, 44
S_M0X, S_M0XT, S_M0W, S_M0WT = 48, 49, 50, 51
S_LOOP = 52
S_SOX = 53          # s53..s59: X DMA row offsets, instructions 1..7
S_SOW = 60          # s60..s66: W DMA row offsets
S_E0, S_E1 = 67, 68  # epilogue scratch
S_Q, S_R = 69, 70   # division results
# timing kernel: s72..s83 six
# s_memtime stamps (aligned pairs), s84..s86 accumulated waits (vm, X-free
# barrier, W-free barrier), s88..s89 the kernel's start stamp
S_TMT, S_ACC, S_T_START = 72, 84, 88
S_ITER, S_GRID = 90, 91   # persistent arms: this workgroup's tile-order index, the grid size
S_MAP, S_KGRID = 92, 93   # kernarg map / grid words (s94, s95: the map's decoded log2 group, walk flag)
S_LG, S_WALK = 94, 95
S_ADVW = 78         # NN kernels: 64 rows of W in bytes (the window's step per k-tile)
N_SGPR = 96

# VGPRs
V_TID = 132
V_DX, V_DW = 1, 133        # DMA lane offsets (bytes)
V_RX, V_RW = 2, 3          # LDS fragment-read bases
V_RXT, V_RWT = 134, 135    # stage toggles (xor masks)
V_FX0, V_FX1 = 4, 36       # X fragments, sub-steps 0 / 1 (8 x 4 VGPRs each)
V_FW0, V_FW1 = 68, 100     # W fragments
V_T = 136                  # 136..139 scratch
V_E = 140                  # 140..255 epilogue scratch

UNIT_GATE_ROWS = 64        # swiglu_fwd: W rows per wave column per half


class Asm:
    def __init__(self, prefix: str = ""):
        self.out: list[str] = []
        self.nlab = 0
        self.prefix = prefix
        self.abort = f"L_{prefix}abort"
        self.stage_exit = f"L_{prefix}stage_exit"

    def __call__(self, s: str):
        self.out.append("  " + s)

    def label(self, name: str):
        self.out.append(name + ":")

    def fresh(self, stem: str) -> str:
        self.nlab += 1
        return f"L_{self.prefix}{stem}_{self.nlab}"

    def raw(self, s: str):
        self.out.append(s)


def vr(base: int, n: int = 1) -> str:
    return f"v{base}" if n == 1 else f"v[{base}:{base + n - 1}]"


def sr(base: int, n: int = 1) -> str:
    return f"s{base}" if n == 1 else f"s[{base}:{base + n - 1}]"


def ar(base: int, n: int = 1) -> str:
    return f"a{base}" if n == 1 else f"a[{base}:{base + n - 1}]"


# ---------------------------------------------------------------- helpers
def udiv(a: Asm, q: int, r: int, num: int, den: int):
    """s_q = s_num / s_den, s_r = s_num % s_den (unsigned, both < 2^24):
    float reciprocal estimate on the VALU, then one exact correction step
    each way on the SALU."""
    # Explicit wait states (hipcc inserts these; hand-written code must):
    # a transcendental's result forwarded to the next VALU, and a VALU
    # result read by v_readfirstlane, both need padding on gfx950 -- without
    # the second, v_readfirstlane returned the PRE-conversion float bits
    # (measured: tile coordinate 0x3fc00000 = 1.5 for 3 / 2; the probe kernel).
    a(f"v_cvt_f32_u32 {vr(V_T)}, {sr(den)}")
    a(f"v_cvt_f32_u32 {vr(V_T + 1)}, {sr(num)}")
    a("s_nop 4")
    a(f"v_rcp_iflag_f32 {vr(V_T)}, {vr(V_T)}")
    a("s_nop 4")
    a(f"v_mul_f32 {vr(V_T)}, {vr(V_T)}, {vr(V_T + 1)}")
    a("s_nop 4")
    a(f"v_cvt_u32_f32 {vr(V_T)}, {vr(V_T)}")
    a("s_nop 4")
    a(f"v_readfirstlane_b32 {sr(q)}, {vr(V_T)}")
    a("s_nop 4")
    a(f"s_mul_i32 {sr(r)}, {sr(q)}, {sr(den)}")
    a(f"s_sub_i32 {sr(r)}, {sr(num)}, {sr(r)}")
    l1, l2 = a.fresh("div"), a.fresh("div")
    a(f"s_cmp_lt_i32 {sr(r)}, 0")
    a(f"s_cbranch_scc0 {l1}")
    a(f"s_sub_u32 {sr(q)}, {sr(q)}, 1")
    a(f"s_add_u32 {sr(r)}, {sr(r)}, {sr(den)}")
    a.label(l1)
    a(f"s_cmp_ge_u32 {sr(r)}, {sr(den)}")
    a(f"s_cbranch_scc0 {l2}")
    a(f"s_add_u32 {sr(q)}, {sr(q)}, 1")
    a(f"s_sub_u32 {sr(r)}, {sr(r)}, {sr(den)}")
    a.label(l2)


def srd(a: Asm, dst: int, base_lo: int, off_lo: int, off_hi: int, nrec: int):
    """dst[0:3] = buffer resource at 64-bit s[base] + (off_hi:off_lo),
    num_records s[nrec] bytes, raw (stride 0), 32-bit dword data format."""
    a(f"s_add_u32 {sr(dst)}, {sr(base_lo)}, {sr(off_lo)}")
    a(f"s_addc_u32 {sr(dst + 1)}, {sr(base_lo + 1)}, {sr(off_hi)}")
    a(f"s_mov_b32 {sr(dst + 2)}, {sr(nrec)}")
    a(f"s_mov_b32 {sr(dst + 3)}, 0x20000")


def mul64(a: Asm, lo: int, hi: int, x: int, y: int):
    """(s_hi:s_lo) = s_x * s_y (unsigned 32 x 32 -> 64)."""
    a(f"s_mul_hi_u32 {sr(hi)}, {sr(x)}, {sr(y)}")
    a(f"s_mul_i32 {sr(lo)}, {sr(x)}, {sr(y)}")


# ---------------------------------------------------------------- prologue
def prologue_args(a: Asm, epi: str = "plain"):
    a(f"s_load_dwordx16 {sr(S_ARGS, 16)}, s[0:1], 0x0")
    a(f"s_load_dwordx4 {sr(S_ARGS + 16, 4)}, s[0:1], 0x40")
    a(f"s_load_dwordx2 {sr(S_MAP, 2)}, s[0:1], 0x50")
    a(f"s_load_dword {sr(S_PHASE)}, s[0:1], {KARG['phase']:#x}")
    if epi != "delta":
        a(f"s_load_dword {sr(S_E0)}, s[0:1], {KARG['m']:#x}")
    a("s_mov_b32 m0, 0")
    a(f"v_mov_b32 {vr(V_TID)}, v0")
    a("s_waitcnt lgkmcnt(0)")
    # defensive: an argument block the host launcher never packs ends the
    # workgroup before any memory access (2 <= ktiles <= 65536, s2 < nwg)
    a(f"s_cmp_lt_u32 {sr(S_KT)}, 2")
    a(f"s_cbranch_scc1 {a.abort}")
    a(f"s_cmp_gt_u32 {sr(S_KT)}, 65536")
    a(f"s_cbranch_scc1 {a.abort}")
    a(f"s_mul_i32 {sr(S_T0)}, {sr(S_TM_N)}, {sr(S_TN_N)}")
    a(f"s_cmp_ge_u32 s2, {sr(S_T0)}")
    a(f"s_cbranch_scc1 {a.abort}")
    a(f"s_lshl_b32 {sr(S_T1)}, {sr(S_XQ)}, 3")
    a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, {sr(S_XR)}")
    a(f"s_cmp_lg_u32 {sr(S_T1)}, {sr(S_T0)}")
    a(f"s_cbranch_scc1 {a.abort}")
    # rows: m = 0 means whole tiles; else (tiles_m - 1) 256 < m <= tiles_m 256
    a(f"s_lshl_b32 {sr(S_M)}, {sr(S_TM_N)}, 8")
    if epi != "delta":
        a(f"s_cmp_eq_u32 {sr(S_E0)}, 0")
        a(f"s_cselect_b32 {sr(S_E0)}, {sr(S_M)}, {sr(S_E0)}")
        a(f"s_sub_u32 {sr(S_T1)}, {sr(S_M)}, {sr(S_E0)}")
        a(f"s_cmp_ge_u32 {sr(S_T1)}, 256")      # (m > tiles_m 256 wraps to a huge value)
        a(f"s_cbranch_scc1 {a.abort}")
        a(f"s_mov_b32 {sr(S_M)}, {sr(S_E0)}")
    # tile order: log2 group <= 6, nothing above the walk bit
    a(f"s_and_b32 {sr(S_LG)}, {sr(S_MAP)}, 15")
    a(f"s_cmp_gt_u32 {sr(S_LG)}, 6")
    a(f"s_cbranch_scc1 {a.abort}")
    a(f"s_cmp_ge_u32 {sr(S_MAP)}, {2 * MAP_WALK_COLS}")
    a(f"s_cbranch_scc1 {a.abort}")
    a(f"s_lshr_b32 {sr(S_WALK)}, {sr(S_MAP)}, 4")
    if epi != "delta":      # (its kernarg bytes 88..95 are the delta pointer, not a phase word)
        phase_delay(a)
    if SCHED["persist"]:
        # persistent: the grid size; 0 would walk one tile forever
        a(f"s_cmp_eq_u32 {sr(S_KGRID)}, 0")
        a(f"s_cbranch_scc1 {a.abort}")
        a(f"s_mov_b32 {sr(S_GRID)}, {sr(S_KGRID)}")
        a(f"s_mov_b32 {sr(S_ITER)}, s2")


PHASE_FIRST_WAVE = 256   # workgroups 0..255: the first one on each of the 256 CUs


def phase_delay(a: Asm):
    """Start offsets for the first wave of workgroups (kernarg `phase`:
    bits [15:0] n, bits [19:16] log2 g; 0 = off).  Every tile of these
    kernels takes the same time, so the 256 workgroups that start together
    keep finishing together, and their epilogues -- a burst of HBM traffic
    with the MFMA pipe idle (the SwiGLU backward loads 256 KiB of gate / up
    and stores 256 KiB per tile) -- all hit memory at once.  Workgroup b of
    the first wave sleeps ((b >> 3) mod g) * n * 512 cycles before its
    prologue: its CU then runs g phase groups apart for the rest of the
    kernel (the next workgroups are dispatched to whichever CU frees first),
    so each epilogue burst meets 1/g of the chip's traffic.  (b >> 3: the
    dispatcher deals workgroups round-robin over the 8 XCDs, so every XCD
    gets every phase.)"""
    l_done, l_sleep = a.fresh("phase_done"), a.fresh("phase_sleep")
    a(f"s_cmp_ge_u32 s2, {PHASE_FIRST_WAVE}")
    a(f"s_cbranch_scc1 {l_done}")
    a(f"s_and_b32 {sr(S_T0)}, {sr(S_PHASE)}, 0xffff")            # n
    a(f"s_lshr_b32 {sr(S_T1)}, {sr(S_PHASE)}, 16")
    a(f"s_and_b32 {sr(S_T1)}, {sr(S_T1)}, 15")                   # log2 g
    a(f"s_lshl_b32 {sr(S_T2)}, 1, {sr(S_T1)}")
    a(f"s_sub_u32 {sr(S_T2)}, {sr(S_T2)}, 1")
    a(f"s_lshr_b32 {sr(S_T3)}, s2, 3")
    a(f"s_and_b32 {sr(S_T3)}, {sr(S_T3)}, {sr(S_T2)}")           # phase group
    a(f"s_mul_i32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_T3)}")           # sleeps of 512 cycles
    a.label(l_sleep)
    a(f"s_cmp_eq_u32 {sr(S_T0)}, 0")
    a(f"s_cbranch_scc1 {l_done}")
    a("s_sleep 8")
    a(f"s_sub_u32 {sr(S_T0)}, {sr(S_T0)}, 1")
    a(f"s_branch {l_sleep}")
    a.label(l_done)


def tile_setup(a: Asm, epi: str, bid: str = "s2", form: str = "tn"):
    """Tile of block `bid` -> S_TILE, (S_TM, S_TN), SRD_X / SRD_W.  form "nn":
    W is [K, N] as stored, its resource the 64-row window of k-tile 0 at
    column 256 tn (the NN kernels below)."""
    # --- XCD remap: blocks b, b+8, ... share an XCD; give each XCD a
    # contiguous range of the tile order (bijective for any nwg)
    a(f"s_and_b32 {sr(S_T0)}, {bid}, 7")              # xcd
    a(f"s_lshr_b32 {sr(S_T1)}, {bid}, 3")             # b / 8
    a(f"s_add_u32 {sr(S_T2)}, {sr(S_XQ)}, 1")         # q + 1
    a(f"s_mul_i32 {sr(S_T3)}, {sr(S_T0)}, {sr(S_T2)}")  # xcd * (q+1)
    a(f"s_mul_i32 {sr(S_TILE)}, {sr(S_XR)}, {sr(S_T2)}")  # r * (q+1)
    a(f"s_sub_u32 {sr(S_T2)}, {sr(S_T0)}, {sr(S_XR)}")  # xcd - r
    a(f"s_mul_i32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_XQ)}")  # (xcd - r) * q
    a(f"s_add_u32 {sr(S_TILE)}, {sr(S_TILE)}, {sr(S_T2)}")
    a(f"s_cmp_lt_u32 {sr(S_T0)}, {sr(S_XR)}")
    a(f"s_cselect_b32 {sr(S_TILE)}, {sr(S_T3)}, {sr(S_TILE)}")
    a(f"s_add_u32 {sr(S_TILE)}, {sr(S_TILE)}, {sr(S_T1)}")
    # --- tile -> (tm, tn) by the kernarg map: groups of 2^lg tiles of the
    # grouped dimension (rows; columns when the walk bit is set) walk the
    # other dimension's tiles.  A = grouped tile count (S_E0), B = walked (S_E1)
    a(f"s_cmp_eq_u32 {sr(S_WALK)}, 0")
    a(f"s_cselect_b32 {sr(S_E0)}, {sr(S_TM_N)}, {sr(S_TN_N)}")
    a(f"s_cselect_b32 {sr(S_E1)}, {sr(S_TN_N)}, {sr(S_TM_N)}")
    a(f"s_lshl_b32 {sr(S_T3)}, {sr(S_E1)}, {sr(S_LG)}")   # tiles per group
    udiv(a, S_Q, S_R, S_TILE, S_T3)                     # group, within
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_Q)}, {sr(S_LG)}")  # first tile of the group
    a(f"s_sub_u32 {sr(S_T1)}, {sr(S_E0)}, {sr(S_T0)}")
    a(f"s_lshl_b32 {sr(S_T2)}, 1, {sr(S_LG)}")
    a(f"s_min_u32 {sr(S_T1)}, {sr(S_T1)}, {sr(S_T2)}")  # gsz
    a(f"s_mov_b32 {sr(S_T2)}, {sr(S_R)}")
    udiv(a, S_Q, S_R, S_T2, S_T1)                       # within / gsz, within % gsz
    a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_R)}")   # grouped-dimension tile
    a(f"s_cmp_eq_u32 {sr(S_WALK)}, 0")
    a(f"s_cselect_b32 {sr(S_TM)}, {sr(S_T0)}, {sr(S_Q)}")
    a(f"s_cselect_b32 {sr(S_TN)}, {sr(S_Q)}, {sr(S_T0)}")

    # --- buffer resources at the tile's first row / column
    # X: rows tm*256 .. +255 (the last tile row: up to row m), every k
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TM)}, 8")
    mul64(a, S_T2, S_T3, S_T0, S_LDX)
    tile_rows_bytes(a, S_T1, S_LDX)
    srd(a, SRD_X, S_X, S_T2, S_T3, S_T1)
    if form == "nn":
        # W: rows 0..63, columns tn*256 .. +255: 63 row strides + 512 B, so the
        # last window ends with W's row K - 1 (it advances 64 rows per k-tile)
        a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TN)}, 9")
        a(f"s_mul_i32 {sr(S_T1)}, {sr(S_LDW)}, 63")
        a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, 512")
        a(f"s_mov_b32 {sr(S_T3)}, 0")
        srd(a, SRD_W, S_W, S_T0, S_T3, S_T1)
        a(f"s_lshl_b32 {sr(S_ADVW)}, {sr(S_LDW)}, 6")
        return
    # W: rows tn*256 (tn*128 for the gate|up projection)
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TN)}, {7 if epi == 'swiglu_fwd' else 8}")
    mul64(a, S_T2, S_T3, S_T0, S_LDW)
    a(f"s_lshl_b32 {sr(S_T1)}, {sr(S_LDW)}, 8")
    if epi == "swiglu_fwd":
        a(f"s_lshr_b32 {sr(S_T1)}, {sr(S_T1)}, 1")    # 128 rows of each half
        a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, {sr(S_FW)}")  # + the up half's offset
    srd(a, SRD_W, S_W, S_T2, S_T3, S_T1)


def tile_rows_bytes(a: Asm, dst: int, ld: int):
    """s[dst] = min(256, m - 256 tm) * s[ld]: num_records of a window over the
    tile row's live rows.  Row strides are multiples of 16 B, so no 16-B
    access straddles the bound."""
    a(f"s_lshl_b32 {sr(dst)}, {sr(S_TM)}, 8")
    a(f"s_sub_u32 {sr(dst)}, {sr(S_M)}, {sr(dst)}")
    a(f"s_min_u32 {sr(dst)}, {sr(dst)}, 256")
    a(f"s_mul_i32 {sr(dst)}, {sr(dst)}, {sr(ld)}")


def tile_c(a: Asm, epi: str):
    """SRD_C (and SRD_S) of the tile at (S_TM, S_TN)."""
    # C (and S): rows tm*256, columns tn*256 (tn*128 for the gate|up epilogue)
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TM)}, 8")
    mul64(a, S_T2, S_T3, S_T0, S_LDC)
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TN)}, {8 if epi == 'swiglu_fwd' else 9}")  # column bytes
    a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_T0)}")
    a(f"s_addc_u32 {sr(S_T3)}, {sr(S_T3)}, 0")
    tile_rows_bytes(a, S_T1, S_LDC)
    srd(a, SRD_C, S_C, S_T2, S_T3, S_T1)
    if epi in ("delta", "resadd"):   # O / the residual: the same tile of a tensor laid out like C
        a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TM)}, 8")
        mul64(a, S_T2, S_T3, S_T0, S_LDC)
        a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TN)}, 9")
        a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_T0)}")
        a(f"s_addc_u32 {sr(S_T3)}, {sr(S_T3)}, 0")
        tile_rows_bytes(a, S_T1, S_LDC)
        srd(a, SRD_S, S_S, S_T2, S_T3, S_T1)
    if epi in ("swiglu_fwd", "swiglu_bwd"):
        a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TM)}, 8")
        mul64(a, S_T2, S_T3, S_T0, S_LDS)
        a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_TN)}, {8 if epi == 'swiglu_fwd' else 9}")
        a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_T0)}")
        a(f"s_addc_u32 {sr(S_T3)}, {sr(S_T3)}, 0")
        tile_rows_bytes(a, S_T1, S_LDS)
        srd(a, SRD_S, S_S, S_T2, S_T3, S_T1)



def prologue(a: Asm, epi: str, form: str = "tn"):
    prologue_args(a, epi)
    tile_setup(a, epi, sr(S_ITER) if SCHED["persist"] else "s2", form)
    tile_c(a, epi)
    prologue_lanes(a, epi)
    if form == "nn":
        nn_lanes(a)


def prologue_lanes(a: Asm, epi: str):
    # --- DMA lane offsets.  Wave w's instruction j fills LDS line w + 4j of
    # the half: rows (w + 4(j%4)) + 16*(lane>>3) [+ 128 for j >= 4], k chunk
    # lane & 7.  Per-lane part -> V_DX / V_DW, per-instruction part -> s[SO*].
    v = V_T
    a(f"v_lshrrev_b32 {vr(v)}, 6, {vr(V_TID)}")            # w
    a(f"v_and_b32 {vr(v + 1)}, 63, {vr(V_TID)}")           # lane
    a(f"v_lshrrev_b32 {vr(v + 2)}, 3, {vr(v + 1)}")        # lane >> 3
    a(f"v_and_b32 {vr(v + 3)}, 7, {vr(v + 1)}")            # lane & 7
    a(f"v_lshlrev_b32 {vr(v + 3)}, 4, {vr(v + 3)}")        # chunk bytes
    # X: row = w + 16 (lane >> 3)
    a(f"v_lshl_add_u32 {vr(V_DX)}, {vr(v + 2)}, 4, {vr(v)}")
    a(f"v_mul_lo_u32 {vr(V_DX)}, {vr(V_DX)}, {sr(S_LDX)}")
    a(f"v_add_u32 {vr(V_DX)}, {vr(V_DX)}, {vr(v + 3)}")
    # W: LDS row t = w + 4 jj + 16 q (q = lane >> 3) holds W row n(t) with
    # n = 32 (q >> 1) + 8 jj + 4 (q & 1) + w, so MFMA fragments 2p and 2p+1
    # give each lane 8 CONSECUTIVE output columns (16-byte epilogue stores).
    # SwiGLU: the same within each 64-row half, q & 3 in place of q, the up
    # half (q >> 2) F rows further.
    qq = v + 2
    a(f"v_and_b32 {vr(V_DW)}, {3 if epi == 'swiglu_fwd' else 7}, {vr(qq)}")
    a(f"v_lshrrev_b32 {vr(V_DW)}, 1, {vr(V_DW)}")                 # (q[&3]) >> 1
    a(f"v_lshlrev_b32 {vr(V_DW)}, 5, {vr(V_DW)}")                 # 32 (q >> 1)
    a(f"v_add_u32 {vr(V_DW)}, {vr(V_DW)}, {vr(v)}")               # + w
    a(f"v_and_b32 {vr(V_E)}, 1, {vr(qq)}")                        # q & 1
    a(f"v_lshl_add_u32 {vr(V_DW)}, {vr(V_E)}, 2, {vr(V_DW)}")     # + 4 (q & 1)
    a(f"v_mul_lo_u32 {vr(V_DW)}, {vr(V_DW)}, {sr(S_LDW)}")
    a(f"v_add_u32 {vr(V_DW)}, {vr(V_DW)}, {vr(v + 3)}")           # + chunk bytes
    if epi == "swiglu_fwd":
        a(f"v_lshrrev_b32 {vr(V_E)}, 2, {vr(qq)}")                # 0 / 1: gate / up
        a(f"v_mul_lo_u32 {vr(V_E)}, {vr(V_E)}, {sr(S_FW)}")
        a(f"v_add_u32 {vr(V_DW)}, {vr(V_DW)}, {vr(V_E)}")
    for j in range(1, 8):
        rows_x = 4 * (j % 4) + 128 * (j // 4)
        rows_w = 8 * (j % 4) + (UNIT_GATE_ROWS if epi == "swiglu_fwd" else 128) * (j // 4)
        a(f"s_mul_i32 {sr(S_SOX + j - 1)}, {sr(S_LDX)}, {rows_x}")
        a(f"s_mul_i32 {sr(S_SOW + j - 1)}, {sr(S_LDW)}, {rows_w}")
    # --- LDS-DMA bases (M0): wave w at line w of the stage's half
    a("s_nop 4")
    a(f"v_readfirstlane_b32 {sr(S_T0)}, {vr(v)}")          # w
    a("s_nop 4")
    a(f"s_mul_i32 {sr(S_M0X)}, {sr(S_T0)}, {LINE}")
    a(f"s_add_u32 {sr(S_M0XT)}, {sr(S_M0X)}, {STAGE}")
    a(f"s_xor_b32 {sr(S_M0XT)}, {sr(S_M0XT)}, {sr(S_M0X)}")
    a(f"s_add_u32 {sr(S_M0W)}, {sr(S_M0X)}, {HALF}")
    a(f"s_add_u32 {sr(S_M0WT)}, {sr(S_M0W)}, {STAGE}")
    a(f"s_xor_b32 {sr(S_M0WT)}, {sr(S_M0WT)}, {sr(S_M0W)}")
    # --- fragment read bases: line (lane & 15), chunk (lane >> 4), wave half
    a(f"v_and_b32 {vr(v + 2)}, 15, {vr(v + 1)}")
    a(f"v_mul_u32_u24 {vr(v + 2)}, {LINE}, {vr(v + 2)}")
    a(f"v_lshrrev_b32 {vr(v + 3)}, 4, {vr(v + 1)}")
    a(f"v_lshl_add_u32 {vr(v + 2)}, {vr(v + 3)}, 4, {vr(v + 2)}")
    a(f"v_and_b32 {vr(v + 3)}, 1, {vr(v)}")                # wm
    a(f"v_mul_u32_u24 {vr(v + 3)}, {16 * LINE}, {vr(v + 3)}")
    a(f"v_add_u32 {vr(V_RX)}, {vr(v + 2)}, {vr(v + 3)}")
    a(f"v_lshrrev_b32 {vr(v + 3)}, 1, {vr(v)}")            # wn
    a(f"v_mul_u32_u24 {vr(v + 3)}, {16 * LINE}, {vr(v + 3)}")
    a(f"v_add_u32 {vr(V_RW)}, {vr(v + 2)}, {vr(v + 3)}")
    a(f"v_add_u32 {vr(V_RW)}, {HALF}, {vr(V_RW)}")
    a(f"v_add_u32 {vr(V_RXT)}, {STAGE}, {vr(V_RX)}")
    a(f"v_xor_b32 {vr(V_RXT)}, {vr(V_RXT)}, {vr(V_RX)}")
    a(f"v_add_u32 {vr(V_RWT)}, {STAGE}, {vr(V_RW)}")
    a(f"v_xor_b32 {vr(V_RWT)}, {vr(V_RWT)}, {vr(V_RW)}")


def zero_acc(a: Asm):
    for i in range(256):
        a(f"v_accvgpr_write_b32 {ar(i)}, 0")


# ---------------------------------------------------------------- main loop
def dma(a: Asm, half: str, j: int) -> list[str]:
    """Instructions for DMA piece j (0..7) of the X or W half: set M0 to the
    line, one buffer_load_dwordx4 ... lds."""
    srd_, vo, so, m0 = (SRD_X, V_DX, S_SOX, S_M0X) if half == "x" else (SRD_W, V_DW, S_SOW, S_M0W)
    out = []
    if j == 0:
        out.append(f"s_mov_b32 m0, {sr(m0)}")
    else:
        out.append(f"s_add_u32 m0, m0, {4 * LINE}")
    # gfx9 hazard: an LDS-DMA reads M0 one wait state after the SALU write
    # (LLVM's checkReadM0Hazards; hipcc always separates the two)
    out.append("s_nop 0")
    soff = "0" if j == 0 else sr(so + j - 1)
    out.append(f"buffer_load_dwordx4 {vr(vo)}, {sr(srd_, 4)}, {soff} offen lds")
    return out


def advance(half: str) -> list[str]:
    s = SRD_X if half == "x" else SRD_W
    return [f"s_add_u32 {sr(s)}, {sr(s)}, 128", f"s_addc_u32 {sr(s + 1)}, {sr(s + 1)}, 0"]


def frag_read(kind: str, f: int, sub: int) -> str:
    base = V_RX if kind == "x" else V_RW
    dst = (V_FX0 if sub == 0 else V_FX1) if kind == "x" else (V_FW0 if sub == 0 else V_FW1)
    off = 128 * f + 64 * sub
    return f"ds_read_b128 {vr(dst + 4 * f, 4)}, {vr(base)} offset:{off}"


def mfma(i: int, j: int, sub: int) -> str:
    fw = (V_FW0 if sub == 0 else V_FW1) + 4 * i
    fx = (V_FX0 if sub == 0 else V_FX1) + 4 * j
    acc = 4 * (8 * i + j)
    return f"v_mfma_f32_16x16x32_bf16 {ar(acc, 4)}, {vr(fw, 4)}, {vr(fx, 4)}, {ar(acc, 4)}"


# What a kernel variant changes in the code below (_with_knobs): `persist`, a
# workgroup per CU walks its tiles (PLAIN_VARIANTS, SWIGLU_PERSIST_VARIANTS);
# `timing`, the diagnostic s_memtime stamps (1: waits, 2: stretches).
SCHED = {"persist": False, "timing": 0}


def _stamp(k: int) -> str:
    return f"s_memtime {sr(S_TMT + 2 * k, 2)}"


def _accum(acc: int, k_end: int, k_begin: int) -> list[str]:
    """acc += low dword of stamp k_end - stamp k_begin (timing kernel; the
    stamps have returned: called after an lgkmcnt(0))."""
    return [f"s_sub_u32 {sr(S_E0)}, {sr(S_TMT + 2 * k_end)}, {sr(S_TMT + 2 * k_begin)}",
            f"s_add_u32 {sr(S_ACC + acc)}, {sr(S_ACC + acc)}, {sr(S_E0)}"]


# The main loop's slot map: every fragment read, barrier, DMA piece and the
# next-tile wait placed after a given MFMA (0..127), the placement a
# well-tuned 4-wave, 256 x 256 x 64 library kernel uses on gfx950 (observed
# from its instruction stream: pieces spread over the whole iteration, three
# of the W pieces after the next-tile wait).  `split`: every barrier that
# many MFMAs after its wait (the MFMA issued in between runs while the wave
# waits at the barrier); `m0_lag`: M0, set once before the first piece of
# each half, advances that many MFMAs after each piece, so the next piece (at
# least one MFMA later) needs no s_nop; `adv`: the slots of the X / W resource
# advances, a few MFMAs after the half's last piece.  The next-tile wait
# counts the pieces issued before it in this iteration; pieces after it (for
# tile t + 2) land by the NEXT iteration's wait.  Shared with the
# weight-gradient kernel (wgrad_gen.iteration) and the NN kernels
# (iteration_nn).
SLOT_MAP = {"x1": [0, 2, 4, 6, 8, 10, 12, 14], "xbar": 20, "w1": [24, 27, 30, 33, 36, 38, 40, 42], "wbar": 50,
            "xdma": [22, 25, 28, 31, 34, 52, 55, 58], "wdma": [61, 64, 85, 87, 89, 96, 100, 124], "wait": 91,
            "x0": [93, 94, 95, 97, 98, 102, 103, 104], "w0": [105, 106, 109, 112, 114, 117, 120, 123],
            "split": 1, "m0_lag": 1, "adv": {"x": 65, "w": 125}}


def span_slots(m: dict):
    """Stamp slots of the timing kernel's three stretches (after MFMA lo ..
    after MFMA hi): X pieces, W pieces before the next-tile wait, W pieces
    after it."""
    pre = [n for n in m["wdma"] if n < m["wait"]]
    post = [n for n in m["wdma"] if n > m["wait"]]
    return ((m["xdma"][0] - 1, m["xdma"][-1]), (pre[0] - 1, pre[-1]),
            ((post[0] - 1, post[-1]) if post else (m["wait"] + 1, m["wait"] + 2)))


def span_mfmas(m: dict) -> list[int]:
    return [hi - lo for lo, hi in span_slots(m)]


def iteration_map(a: Asm, with_dma: bool, next_reads: bool):
    """One 64-k tile placed by SLOT_MAP: 128 MFMAs (0..63 sub-step 0, 64..127
    sub-step 1) with the reads / DMA / waits in the gaps after them."""
    m = SLOT_MAP
    split, lag = m["split"], m["m0_lag"]
    slots: dict[int, list[str]] = {n: [] for n in range(128)}
    for j, n in enumerate(m["x1"]):
        slots[n].append(frag_read("x", j, 1))
    for i, n in enumerate(m["w1"]):
        slots[n].append(frag_read("w", i, 1))
    assert max(m["x1"]) < m["xbar"] and max(m["w1"]) < m["wbar"] and max(m["x1"] + m["w1"]) < 63
    tm, sp = SCHED["timing"] == 1, SCHED["timing"] == 2
    vm = 0
    if with_dma:
        for bar in (m["xbar"], m["wbar"]):
            slots[bar].append("s_waitcnt lgkmcnt(0)")
            slots[bar + split].append("s_barrier")
        for half, key, bar in (("x", "xdma", m["xbar"]), ("w", "wdma", m["wbar"])):
            srd_, vo, so, m0 = (SRD_X, V_DX, S_SOX, S_M0X) if half == "x" else (SRD_W, V_DW, S_SOW, S_M0W)
            pos = m[key]
            assert sorted(pos) == pos and pos[0] > bar + split and len(set(pos)) == 8
            slots[pos[0] - 1].append(f"s_mov_b32 m0, {sr(m0)}")
            for j, n in enumerate(pos):
                soff = "0" if j == 0 else sr(so + j - 1)
                slots[n].append(f"buffer_load_dwordx4 {vr(vo)}, {sr(srd_, 4)}, {soff} offen lds")
                if j < 7:
                    # an MFMA between every M0 write and the next piece (the
                    # M0 -> LDS-DMA hazard wants one wait state)
                    assert pos[j + 1] > n + lag
                    slots[n + lag].append(f"s_add_u32 m0, m0, {4 * LINE}")
            adv = m["adv"][half]
            assert pos[-1] <= adv < 128
            slots[adv] += advance(half) + [f"s_xor_b32 {sr(m0)}, {sr(m0)}, {sr(m0 + 1)}"]
        # the two halves' pieces must not interleave (one running M0)
        assert max(m["xdma"]) + lag < min(m["wdma"]) - 1
        vm = sum(1 for n in m["xdma"] + m["wdma"] if n < m["wait"])

    def stamp_around(k, n):
        """stamp k before the wait in slot n, stamp k+1 right after its
        barrier (slot n + split; with a split the MFMA between them counts)"""
        slots[n].insert(slots[n].index(next(x for x in slots[n] if x.startswith("s_waitcnt"))), _stamp(k))
        b = slots[n + split]
        b.insert(b.index("s_barrier") + 1, _stamp(k + 1))

    if with_dma and tm:  # waits: X-free and W-free barriers (the vm wait below)
        for k, bar in ((2, m["xbar"]), (4, m["wbar"])):
            stamp_around(k, bar)
    if with_dma and sp:  # stretches: X pieces, W pieces before the wait, W pieces after it
        for k, (lo, hi) in enumerate(span_slots(m)):
            slots[lo].append(_stamp(2 * k))
            slots[hi].append(_stamp(2 * k + 1))
    if next_reads:
        # the next tile (staged one iteration ago) has landed: own DMA by the
        # counted wait, everyone's by the barrier
        w = m["wait"]
        slots[w].append(f"s_waitcnt vmcnt({vm})")
        slots[w + split] += ["s_barrier", f"v_xor_b32 {vr(V_RX)}, {vr(V_RX)}, {vr(V_RXT)}",
                             f"v_xor_b32 {vr(V_RW)}, {vr(V_RW)}, {vr(V_RWT)}"]
        if tm and with_dma:
            stamp_around(0, w)
        assert min(m["x0"] + m["w0"]) > w + split and max(m["x0"] + m["w0"]) < 126
        for j, n in enumerate(m["x0"]):
            slots[n].append(frag_read("x", j, 0))
        for i, n in enumerate(m["w0"]):
            slots[n].append(frag_read("w", i, 0))
        slots[126].append("s_waitcnt lgkmcnt(0)")
        if with_dma and (tm or sp):
            slots[126] += _accum(0, 1, 0) + _accum(1, 3, 2) + _accum(2, 5, 4)
    for n in range(128):
        sub, mm = divmod(n, 64)
        i, j = divmod(mm, 8)
        if n == 64:
            # phase 2 consumes the sub-step 1 fragments read in phase 1
            a("s_waitcnt lgkmcnt(0)")
        # every MFMA (8 B) on an 8-byte boundary: a hand-written stream
        # shifted by 4 mod 8 bytes runs ~13 % slower on gfx950
        # (MI355X_MICROARCH.md, code-placement sensitivity); the
        # assembler pads with a 4-byte s_nop 0 only where needed
        a(".p2alignl 3, 0xbf800000")
        a(mfma(i, j, sub))
        for ins in slots[n]:
            a(ins)



# ---------------------------------------------------------------- epilogues
def acc_index(i: int, j: int) -> int:
    return 4 * (8 * i + j)


ROPE_DEPTH = 2   # cos / sin row blocks loaded this many blocks ahead (staging in the fragment VGPRs)


def epilogue_rope(a: Asm):
    """The fused-QKV projection's epilogue with RoPE and the head-major
    relayout (replaces toa_rope_fwd): C is never written as [T, (Hq + 2 Hkv)
    128]; wave (wm, wn) owns head h = 2 tn + wn for 128 tokens and stores
    them rotated (q, k heads; rotate-half pairs (d, d + 64), both in the
    lane: fragment pairs p and p + 2) or as they are (v heads) into out =
    [q: B Hq S 128 | k: B Hkv S 128 | v: B Hkv S 128] bf16 (kernarg C).
    Rotation on the fp32 accumulators (the unfused path rotated the bf16-
    rounded GEMM output).  Kernarg S: cos | sin [2][S][64] fp32; fw = S (a
    multiple of 256, so a tile's 256 tokens are one sequence's), fc = Hq |
    Hkv << 16.  cos / sin rows for row block j + ROPE_DEPTH load while j is
    rotated (counted vmcnt, as epilogue_swiglu_bwd)."""
    v = V_T
    # ---- wave-uniform: w, wm, wn, head, batch, s0 (SGPRs S_E0.. / S_T*)
    a(f"v_lshrrev_b32 {vr(v)}, 6, {vr(V_TID)}")
    a("s_nop 4")
    a(f"v_readfirstlane_b32 {sr(S_Q)}, {vr(v)}")              # w
    a(f"s_and_b32 {sr(S_R)}, {sr(S_Q)}, 1")                   # wm
    a(f"s_lshr_b32 {sr(S_Q)}, {sr(S_Q)}, 1")                  # wn
    a(f"s_lshl_b32 {sr(S_E0)}, {sr(S_TN)}, 1")
    a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_Q)}")         # head h
    a(f"s_lshl_b32 {sr(S_T3)}, {sr(S_TM)}, 8")                # first token of the tile
    udiv(a, S_T0, S_T1, S_T3, S_FW)                           # b = t0 / S, s_tile = t0 % S
    a(f"s_lshl_b32 {sr(S_R)}, {sr(S_R)}, 7")
    a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, {sr(S_R)}")         # s0 = s_tile + 128 wm
    a(f"s_and_b32 {sr(S_T2)}, {sr(S_FC)}, 0xffff")            # Hq
    a(f"s_lshr_b32 {sr(S_T3)}, {sr(S_FC)}, 16")               # Hkv
    # Btot = tiles_m 256 / S (whole sequences): S_E1
    a(f"s_lshl_b32 {sr(S_Q)}, {sr(S_TM_N)}, 8")
    udiv(a, S_E1, S_R, S_Q, S_FW)
    # head row index (in units of S rows of 128 elements) into out, by section:
    #   q: (b Hq + h) ; k: Btot Hq + b Hkv + (h - Hq) ; v: Btot (Hq + Hkv) + b Hkv + (h - Hq - Hkv)
    l_k, l_v, l_base = a.fresh("rope_k"), a.fresh("rope_v"), a.fresh("rope_base")
    a(f"s_mov_b32 {sr(S_LOOP)}, 1")                           # rotate flag (q and k heads)
    a(f"s_cmp_ge_u32 {sr(S_E0)}, {sr(S_T2)}")
    a(f"s_cbranch_scc1 {l_k}")
    a(f"s_mul_i32 {sr(S_Q)}, {sr(S_T0)}, {sr(S_T2)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_E0)}")
    a(f"s_branch {l_base}")
    a.label(l_k)
    a(f"s_sub_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_T2)}")        # h - Hq
    a(f"s_mul_i32 {sr(S_Q)}, {sr(S_E1)}, {sr(S_T2)}")         # Btot Hq
    a(f"s_cmp_ge_u32 {sr(S_E0)}, {sr(S_T3)}")
    a(f"s_cbranch_scc1 {l_v}")
    a(f"s_mul_i32 {sr(S_R)}, {sr(S_T0)}, {sr(S_T3)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_R)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_E0)}")
    a(f"s_branch {l_base}")
    a.label(l_v)
    a(f"s_mov_b32 {sr(S_LOOP)}, 0")
    a(f"s_sub_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_T3)}")        # h - Hq - Hkv
    a(f"s_mul_i32 {sr(S_R)}, {sr(S_E1)}, {sr(S_T3)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_R)}")           # Btot (Hq + Hkv)
    a(f"s_mul_i32 {sr(S_R)}, {sr(S_T0)}, {sr(S_T3)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_R)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_E0)}")
    a.label(l_base)
    # byte offset of (head row, s0): (S_Q S + s0) 256 -> SRD_C over this wave's 128 rows
    a(f"s_mul_i32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_FW)}")
    a(f"s_add_u32 {sr(S_Q)}, {sr(S_Q)}, {sr(S_T1)}")
    a(f"s_mov_b32 {sr(S_R)}, 256")
    mul64(a, S_T2, S_T3, S_Q, S_R)
    a(f"s_mov_b32 {sr(S_R)}, {128 * 256}")
    srd(a, SRD_C, S_C, S_T2, S_T3, S_R)
    # cos / sin rows s0 .. s0 + 127: SRD_S at cos + s0 256, sin + S 256 (soffset S_E1 = S 256)
    a(f"s_mov_b32 {sr(S_R)}, 256")
    mul64(a, S_T2, S_T3, S_T1, S_R)
    a(f"s_mul_i32 {sr(S_E1)}, {sr(S_FW)}, 256")
    a(f"s_add_u32 {sr(S_R)}, {sr(S_E1)}, {128 * 256}")
    srd(a, SRD_S, S_S, S_T2, S_T3, S_R)
    # ---- per lane: C offset (row l & 15, group g = l >> 4: 16 g bytes), cos offset 32 g bytes
    a(f"v_and_b32 {vr(v + 1)}, 63, {vr(V_TID)}")
    a(f"v_and_b32 {vr(v + 2)}, 15, {vr(v + 1)}")
    a(f"v_lshlrev_b32 {vr(v + 2)}, 8, {vr(v + 2)}")           # row * 256
    a(f"v_lshrrev_b32 {vr(v + 3)}, 4, {vr(v + 1)}")           # g
    a(f"v_lshl_add_u32 {vr(V_E)}, {vr(v + 3)}, 4, {vr(v + 2)}")      # out: 16 g
    a(f"v_lshl_add_u32 {vr(V_E + 1)}, {vr(v + 3)}, 5, {vr(v + 2)}")  # cos: 32 g
    a(f"s_mov_b32 {sr(S_T0)}, 0")                             # row block soffset (out and cos: 16 rows x 256 B)
    a(f"s_mov_b32 {sr(S_T1)}, 0")                             # cos prefetch soffset
    a(f"s_add_u32 {sr(S_T2)}, {sr(S_E1)}, 0")                 # sin prefetch soffset (S 256 + row block)
    l_plain, l_end = a.fresh("rope_plain"), a.fresh("rope_end")
    a(f"s_cmp_eq_u32 {sr(S_LOOP)}, 0")
    a(f"s_cbranch_scc1 {l_plain}")
    D = ROPE_DEPTH
    seq: list = []

    def slot(j):
        return V_FX0 + 32 * (j % D)             # cos 16 regs, sin 16 regs

    def issue(j):
        st = slot(j)
        for p in range(2):
            for h in range(2):
                a(f"buffer_load_dwordx4 {vr(st + 8 * p + 4 * h, 4)}, {vr(V_E + 1)}, {sr(SRD_S, 4)}, {sr(S_T1)} offen offset:{128 * p + 16 * h}")
                a(f"buffer_load_dwordx4 {vr(st + 16 + 8 * p + 4 * h, 4)}, {vr(V_E + 1)}, {sr(SRD_S, 4)}, {sr(S_T2)} offen offset:{128 * p + 16 * h}")
                seq.extend([("L", j), ("L", j)])
        a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, 4096")
        a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, 4096")

    for j in range(min(D, 8)):
        issue(j)
    f, pk, t = V_E + 8, V_E + 40, V_E + 56
    for j in range(8):
        for p in range(4):
            read_pair(a, f + 8 * p, p, j)
        last = max(i for i, x in enumerate(seq) if x == ("L", j))
        a(f"s_waitcnt vmcnt({min(63, len(seq) - last - 1)})")
        cs, sn = slot(j), slot(j) + 16
        for p in range(2):
            for e in range(8):
                x1, x2 = f + 8 * p + e, f + 8 * (p + 2) + e
                c_, s_ = cs + 8 * p + e, sn + 8 * p + e
                a(f"v_mul_f32 {vr(t)}, {vr(x2)}, {vr(s_)}")
                a(f"v_mul_f32 {vr(t + 1)}, {vr(x1)}, {vr(s_)}")
                a(f"v_mul_f32 {vr(t + 2)}, {vr(x1)}, {vr(c_)}")
                a(f"v_fma_f32 {vr(x2)}, {vr(x2)}, {vr(c_)}, {vr(t + 1)}")   # x2 c + x1 s
                a(f"v_sub_f32 {vr(x1)}, {vr(t + 2)}, {vr(t)}")              # x1 c - x2 s
        if j + D < 8:
            issue(j + D)                          # into the slot just consumed
        for p in range(4):
            cvt_pack8(a, pk + 4 * p, f + 8 * p)
        for p in range(4):
            store16(a, pk + 4 * p, V_E, SRD_C, S_T0, p)
        seq.extend([("S", j)] * 4)
        a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, 4096")
        a("s_nop 1")
    a(f"s_branch {l_end}")
    # ---- v heads: the relayout alone
    a.label(l_plain)
    for j in range(8):
        for p in range(4):
            read_pair(a, f + 8 * p, p, j)
        for p in range(4):
            cvt_pack8(a, pk + 4 * p, f + 8 * p)
        for p in range(4):
            store16(a, pk + 4 * p, V_E, SRD_C, S_T0, p)
        a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, 4096")
        a("s_nop 1")
    a.label(l_end)


DELTA_DEPTH = 2      # O row blocks loaded this many blocks ahead
SRD_DL = 72          # s72..s75: the delta rows of this wave (kernarg bytes 88..95)


def epilogue_delta(a: Asm):
    """The attention output projection's data gradient dO = dY Wo (plain C
    stores) with the attention backward's delta fused in: ndelta[(b H + h) S
    + s] = -sum_d dO[t][128 h + d] O[t][128 h + d] over the wave's head h =
    2 tn + wn (kernarg S = O, laid out like C; fw = S, fc = H; bytes 88..95
    = ndelta fp32 [B, H, S]).  dO enters as the bf16 values stored (what the
    attention backward's dP reads).  A row's 128 columns sit in 4 lanes
    (l & 15 fixed); their partial sums meet in 1 KiB of LDS past the
    pipeline's stages; O row blocks load DELTA_DEPTH blocks ahead.  Replaces
    attn_delta_kernel's pass over dO and O (csrc/hip/attention.hip)."""
    v = V_T
    a(f"s_load_dwordx2 {sr(SRD_DL, 2)}, s[0:1], 0x58")
    a(f"v_lshrrev_b32 {vr(v)}, 6, {vr(V_TID)}")
    a("s_nop 4")
    a(f"v_readfirstlane_b32 {sr(S_Q)}, {vr(v)}")              # w
    a(f"s_and_b32 {sr(S_R)}, {sr(S_Q)}, 1")                   # wm
    a(f"s_lshr_b32 {sr(S_T2)}, {sr(S_Q)}, 1")                 # wn
    a(f"s_lshl_b32 {sr(S_T3)}, {sr(S_TN)}, 1")
    a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_T3)}")        # head h
    a(f"s_lshl_b32 {sr(S_T3)}, {sr(S_TM)}, 8")
    udiv(a, S_T0, S_T1, S_T3, S_FW)                           # b, s_tile
    a(f"s_lshl_b32 {sr(S_R)}, {sr(S_R)}, 7")
    a(f"s_add_u32 {sr(S_T1)}, {sr(S_T1)}, {sr(S_R)}")         # s0
    a(f"s_mul_i32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_FC)}")
    a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_T2)}")        # b H + h
    a(f"s_mul_i32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_FW)}")
    a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_T1)}")        # row of s0
    a(f"s_lshl_b32 {sr(S_T0)}, {sr(S_T0)}, 2")
    a("s_waitcnt lgkmcnt(0)")
    a(f"s_add_u32 {sr(SRD_DL)}, {sr(SRD_DL)}, {sr(S_T0)}")
    a(f"s_addc_u32 {sr(SRD_DL + 1)}, {sr(SRD_DL + 1)}, 0")
    a(f"s_mov_b32 {sr(SRD_DL + 2)}, {128 * 4}")
    a(f"s_mov_b32 {sr(SRD_DL + 3)}, 0x20000")
    # lanes: LDS scratch (wave w: 256 B at LDS_BYTES + 256 w), the delta row (l & 15)
    a(f"v_and_b32 {vr(v + 1)}, 63, {vr(V_TID)}")
    a(f"v_lshlrev_b32 {vr(v + 2)}, 2, {vr(V_TID)}")            # 4 (64 w + l)
    a(f"v_add_u32 {vr(v + 2)}, {LDS_BYTES}, {vr(v + 2)}")       # write address
    a(f"v_and_b32 {vr(v + 3)}, 15, {vr(v + 1)}")
    a(f"v_lshlrev_b32 {vr(v + 3)}, 2, {vr(v + 3)}")             # 4 (l & 15): delta offset
    a(f"v_sub_u32 {vr(V_E + 2)}, {vr(v + 2)}, {vr(v + 1)}")    # ... 4 l ...
    a(f"v_sub_u32 {vr(V_E + 2)}, {vr(V_E + 2)}, {vr(v + 1)}")
    a(f"v_sub_u32 {vr(V_E + 2)}, {vr(V_E + 2)}, {vr(v + 1)}")
    a(f"v_sub_u32 {vr(V_E + 2)}, {vr(V_E + 2)}, {vr(v + 1)}")  # wave base: LDS_BYTES + 256 w
    a(f"v_add_u32 {vr(V_E + 2)}, {vr(V_E + 2)}, {vr(v + 3)}")  # + 4 (l & 15): the row's 4 partials at +0/64/128/192
    a(f"s_mov_b32 {sr(S_E0)}, 0")                             # row block offset (C and O)
    a(f"s_lshl_b32 {sr(S_E1)}, {sr(S_LDC)}, 4")
    a(f"s_mov_b32 {sr(S_T2)}, 0")                             # O prefetch row block offset
    D = DELTA_DEPTH
    seq: list = []

    def slot(j):
        return V_FX0 + 16 * (j % D)

    def issue(j):
        for p in range(4):
            a(f"buffer_load_dwordx4 {vr(slot(j) + 4 * p, 4)}, {vr(V_E)}, {sr(SRD_S, 4)}, {sr(S_T2)} offen offset:{64 * p}")
            seq.append(("L", j))
        a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_E1)}")

    for j in range(min(D, 8)):
        issue(j)
    f, pk, ob, acc = V_E + 8, V_E + 40, V_E + 56, V_E + 72
    for j in range(8):
        for p in range(4):
            read_pair(a, f + 8 * p, p, j)
        for p in range(4):
            cvt_pack8(a, pk + 4 * p, f + 8 * p)
        for p in range(4):
            store16(a, pk + 4 * p, V_E, SRD_C, S_E0, p)
        seq.extend([("S", j)] * 4)
        for p in range(4):
            unpack8(a, f + 8 * p, pk + 4 * p)                  # dO as stored (bf16)
        last = max(i for i, x in enumerate(seq) if x == ("L", j))
        a(f"s_waitcnt vmcnt({min(63, len(seq) - last - 1)})")
        for p in range(4):
            unpack8(a, ob + 8 * (p % 2), slot(j) + 4 * p)
            for e in range(8):
                if p == 0 and e == 0:
                    a(f"v_mul_f32 {vr(acc)}, {vr(f)}, {vr(ob)}")
                else:
                    a(f"v_fma_f32 {vr(acc)}, {vr(f + 8 * p + e)}, {vr(ob + 8 * (p % 2) + e)}, {vr(acc)}")
        if j + D < 8:
            issue(j + D)
        a(f"ds_write_b32 {vr(v + 2)}, {vr(acc)}")
        a("s_waitcnt lgkmcnt(0)")
        for q in range(4):
            a(f"ds_read_b32 {vr(acc + 1 + q)}, {vr(V_E + 2)} offset:{64 * q}")
        a("s_waitcnt lgkmcnt(0)")
        a(f"v_add_f32 {vr(acc + 1)}, {vr(acc + 1)}, {vr(acc + 2)}")
        a(f"v_add_f32 {vr(acc + 3)}, {vr(acc + 3)}, {vr(acc + 4)}")
        a(f"v_add_f32 {vr(acc + 1)}, {vr(acc + 1)}, {vr(acc + 3)}")
        a(f"v_sub_f32 {vr(acc + 1)}, 0, {vr(acc + 1)}")        # -delta
        a(f"s_mov_b32 {sr(S_T3)}, {64 * j}")
        a(f"buffer_store_dword {vr(acc + 1)}, {vr(v + 3)}, {sr(SRD_DL, 4)}, {sr(S_T3)} offen")
        seq.append(("S", j))
        a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_E1)}")
        a("s_nop 1")


def epilogue_resadd(a: Asm):
    """C = X W^T + R (bf16 R laid out like C, kernarg S): the residual add of
    the attention output and MLP down projections in their epilogue, so the
    RMSNorm after it reads one tensor and writes one (ops/gemm.linear_resadd,
    called by ops/llm.attention_block and swiglu_mlp).  R row blocks
    load DELTA_DEPTH blocks ahead (counted vmcnt); the sum is rounded to bf16
    once, as the unfused add of the bf16 GEMM output and R is not (the fused
    path adds in fp32 before the one rounding)."""
    a(f"s_mov_b32 {sr(S_E0)}, 0")
    a(f"s_lshl_b32 {sr(S_E1)}, {sr(S_LDC)}, 4")
    a(f"s_mov_b32 {sr(S_T2)}, 0")
    D = DELTA_DEPTH
    seq: list = []

    def slot(j):
        return V_FX0 + 16 * (j % D)

    def issue(j):
        for p in range(4):
            a(f"buffer_load_dwordx4 {vr(slot(j) + 4 * p, 4)}, {vr(V_E)}, {sr(SRD_S, 4)}, {sr(S_T2)} offen offset:{64 * p}")
            seq.append(("L", j))
        a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_E1)}")

    for j in range(min(D, 8)):
        issue(j)
    f, pk, rb = V_E + 8, V_E + 40, V_E + 56
    for j in range(8):
        for p in range(4):
            read_pair(a, f + 8 * p, p, j)
        last = max(i for i, x in enumerate(seq) if x == ("L", j))
        a(f"s_waitcnt vmcnt({min(63, len(seq) - last - 1)})")
        for p in range(4):
            unpack8(a, rb, slot(j) + 4 * p)
            for e in range(8):
                a(f"v_add_f32 {vr(f + 8 * p + e)}, {vr(f + 8 * p + e)}, {vr(rb + e)}")
        if j + D < 8:
            issue(j + D)
        for p in range(4):
            cvt_pack8(a, pk + 4 * p, f + 8 * p)
        for p in range(4):
            store16(a, pk + 4 * p, V_E, SRD_C, S_E0, p)
        seq.extend([("S", j)] * 4)
        a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_E1)}")
        a("s_nop 1")


def epi_offsets(a: Asm, epi: str):
    """Per-lane output byte offsets.  Lane l of wave (wm, wn) holds, for
    fragments (2p, j) and (2p+1, j): row m = wm*128 + 16 j + (l & 15) and the
    8 columns n = 32 p + 8 (l >> 4) .. +7 of the wave's W rows (the W-row
    permutation of the DMA): one 16-byte store per pair p."""
    v = V_T
    a(f"v_lshrrev_b32 {vr(v)}, 6, {vr(V_TID)}")            # w
    a(f"v_and_b32 {vr(v + 1)}, 63, {vr(V_TID)}")           # lane
    a(f"v_and_b32 {vr(v + 2)}, 15, {vr(v + 1)}")
    a(f"v_and_b32 {vr(v + 3)}, 1, {vr(v)}")
    a(f"v_lshl_add_u32 {vr(v + 2)}, {vr(v + 3)}, 7, {vr(v + 2)}")  # row in tile
    a(f"v_lshrrev_b32 {vr(v + 1)}, 4, {vr(v + 1)}")        # lane >> 4
    a(f"v_lshlrev_b32 {vr(v + 1)}, 4, {vr(v + 1)}")        # 16 B per lane group
    a(f"v_lshrrev_b32 {vr(v)}, 1, {vr(v)}")                # wn
    # column bytes of the wave: plain / bwd 128 cols per wave, fwd 64 units
    a(f"v_lshlrev_b32 {vr(v)}, {8 if epi != 'swiglu_fwd' else 7}, {vr(v)}")
    a(f"v_add_u32 {vr(v + 1)}, {vr(v + 1)}, {vr(v)}")      # col bytes
    # V_E+0: C offset, V_E+1: S offset (fwd: s; bwd: gu)
    a(f"v_mul_lo_u32 {vr(V_E)}, {vr(v + 2)}, {sr(S_LDC)}")
    a(f"v_add_u32 {vr(V_E)}, {vr(V_E)}, {vr(v + 1)}")
    if epi != "plain":
        a(f"v_mul_lo_u32 {vr(V_E + 1)}, {vr(v + 2)}, {sr(S_LDS)}")
        a(f"v_add_u32 {vr(V_E + 1)}, {vr(V_E + 1)}, {vr(v + 1)}")
    if epi == "swiglu_fwd":
        a(f"v_add_u32 {vr(V_E + 2)}, {sr(S_FC)}, {vr(V_E)}")  # up half of gu
    if epi == "swiglu_bwd":
        a(f"v_add_u32 {vr(V_E + 2)}, {sr(S_FC)}, {vr(V_E)}")      # up half of dgu
        a(f"v_add_u32 {vr(V_E + 3)}, {sr(S_FC)}, {vr(V_E + 1)}")  # up half of gu


def read_acc4(a: Asm, dst: int, acc: int):
    for r in range(4):
        a(f"v_accvgpr_read_b32 {vr(dst + r)}, {ar(acc + r)}")


def cvt_pack(a: Asm, dst: int, src: int):
    a(f"v_cvt_pk_bf16_f32 {vr(dst)}, {vr(src)}, {vr(src + 1)}")
    a(f"v_cvt_pk_bf16_f32 {vr(dst + 1)}, {vr(src + 2)}, {vr(src + 3)}")


def unpack_bf16(a: Asm, dst: int, src: int):
    """dst[0..3] = f32 of the 4 bf16 in src[0..1] (element order kept)."""
    a(f"v_lshlrev_b32 {vr(dst)}, 16, {vr(src)}")
    a(f"v_and_b32 {vr(dst + 1)}, 0xffff0000, {vr(src)}")
    a(f"v_lshlrev_b32 {vr(dst + 2)}, 16, {vr(src + 1)}")
    a(f"v_and_b32 {vr(dst + 3)}, 0xffff0000, {vr(src + 1)}")


LOG2E = 1.4426950408889634
NN_SWAP = False                 # set while an NN kernel is generated (kernel_nn)
S_EX_SAME, S_EX_SWAP = 84, 86   # NN epilogues: EXEC masks of the lanes whose fragment pairs are in / out of column order


def read_pair(a: Asm, dst: int, p: int, j: int, ioff: int = 0):
    """dst[0..7] = the lane's 8 consecutive columns of fragments (2p, j) and
    (2p+1, j) (ioff: fragment offset, 4 for SwiGLU's up half).  In the NN
    kernels (NN_SWAP) lane groups 1 and 2 hold the pair's two fragments the
    other way round: two EXEC-masked passes put them in column order."""
    if NN_SWAP:
        a(f"s_mov_b64 exec, {sr(S_EX_SAME, 2)}")        # lanes 0..15, 48..63
    read_acc4(a, dst, acc_index(2 * p + ioff, j))
    read_acc4(a, dst + 4, acc_index(2 * p + 1 + ioff, j))
    if NN_SWAP:
        a(f"s_mov_b64 exec, {sr(S_EX_SWAP, 2)}")        # lanes 16..47
        read_acc4(a, dst + 4, acc_index(2 * p + ioff, j))
        read_acc4(a, dst, acc_index(2 * p + 1 + ioff, j))
        a("s_mov_b64 exec, -1")


def cvt_pack8(a: Asm, dst: int, src: int):
    cvt_pack(a, dst, src)
    cvt_pack(a, dst + 2, src + 4)


def unpack8(a: Asm, dst: int, src: int):
    unpack_bf16(a, dst, src)
    unpack_bf16(a, dst + 4, src + 2)


def store16(a: Asm, data: int, voff: int, srd_: int, soff: int, p: int):
    a(f"buffer_store_dwordx4 {vr(data, 4)}, {vr(voff)}, {sr(srd_, 4)}, {sr(soff)} offen offset:{64 * p} nt")


def epilogue_plain(a: Asm):
    a(f"s_mov_b32 {sr(S_E0)}, 0")                             # row block offset
    a(f"s_lshl_b32 {sr(S_E1)}, {sr(S_LDC)}, 4")              # 16 rows
    for j in range(8):
        f, pk = V_E + 8, V_E + 40                             # 32 f32, 16 packed
        for p in range(4):
            read_pair(a, f + 8 * p, p, j)
        for p in range(4):
            cvt_pack8(a, pk + 4 * p, f + 8 * p)
        for p in range(4):
            store16(a, pk + 4 * p, V_E, SRD_C, S_E0, p)
        a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_E1)}")


def silu_times(a: Asm, out: int, g: int, u: int, t: int, n: int):
    """out[e] = silu(g[e]) * u[e] = g / (1 + 2^(-g log2 e)) * u, e < n
    (batched per op: a transcendental's result is consumed n instructions
    later, past the forwarding hazard).  The non-transcendental ops work on
    register pairs (v_pk_*_f32; constants -log2 e and 1.0 as pairs at
    V_E + 4 / V_E + 6)."""
    for e in range(0, n, 2):
        a(f"v_pk_mul_f32 {vr(t + e, 2)}, {vr(V_E + 4, 2)}, {vr(g + e, 2)}")
    for e in range(n):
        a(f"v_exp_f32 {vr(t + e)}, {vr(t + e)}")
    for e in range(0, n, 2):
        a(f"v_pk_add_f32 {vr(t + e, 2)}, {vr(V_E + 6, 2)}, {vr(t + e, 2)}")
    for e in range(n):
        a(f"v_rcp_f32 {vr(t + e)}, {vr(t + e)}")
    for e in range(0, n, 2):
        a(f"v_pk_mul_f32 {vr(t + e, 2)}, {vr(g + e, 2)}, {vr(t + e, 2)}")
    for e in range(0, n, 2):
        a(f"v_pk_mul_f32 {vr(out + e, 2)}, {vr(t + e, 2)}, {vr(u + e, 2)}")


def epilogue_swiglu_fwd(a: Asm):
    """Fragments 0..3 gate, 4..7 the same hidden units' up values: pairs
    p = 0, 1 of each give a lane 8 consecutive units."""
    a(f"s_mov_b32 {sr(S_E0)}, 0")
    a(f"s_lshl_b32 {sr(S_E1)}, {sr(S_LDC)}, 4")
    a(f"s_mov_b32 {sr(S_T0)}, 0")
    a(f"s_lshl_b32 {sr(S_T1)}, {sr(S_LDS)}, 4")
    # (V_E + 3: the scalar form's -log2 e, read by nothing since silu_times
    # works on pairs; the instruction stays, the kernel's bytes are pinned)
    a(f"v_mov_b32 {vr(V_E + 3)}, {-LOG2E!r}")
    for x in (4, 5):
        a(f"v_mov_b32 {vr(V_E + x)}, {-LOG2E!r}")
    for x in (6, 7):
        a(f"v_mov_b32 {vr(V_E + x)}, 1.0")
    for j in range(8):
        g, u = V_E + 8, V_E + 24            # 16 f32 each (2 pairs)
        for p in range(2):
            read_pair(a, g + 8 * p, p, j)
            read_pair(a, u + 8 * p, p, j, ioff=4)
        pg, pu = V_E + 40, V_E + 48         # packed bf16 (8 regs each)
        for p in range(2):
            cvt_pack8(a, pg + 4 * p, g + 8 * p)
            cvt_pack8(a, pu + 4 * p, u + 8 * p)
        for p in range(2):
            store16(a, pg + 4 * p, V_E, SRD_C, S_E0, p)
            store16(a, pu + 4 * p, V_E + 2, SRD_C, S_E0, p)
        sv, ps = V_E + 88, V_E + 104
        # s = silu(g) * u straight from the fp32 accumulators (no bf16 round
        # trip: 32 VALU per row block fewer; the unfused path and round 4
        # used the stored bf16 values, a difference below bf16 rounding)
        for h in range(2):                  # scratch: the free V_E + 56 .. 63
            silu_times(a, sv + 8 * h, g + 8 * h, u + 8 * h, V_E + 56, 8)
        for p in range(2):
            cvt_pack8(a, ps + 4 * p, sv + 8 * p)
        for p in range(2):
            store16(a, ps + 4 * p, V_E + 1, SRD_S, S_T0, p)
        a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_E1)}")
        a(f"s_add_u32 {sr(S_T0)}, {sr(S_T0)}, {sr(S_T1)}")
        # no drain -- a store reads its data registers within two wait states
        # of issue (cdna_hip_programming.md, asm stores), and the next row
        # block rewrites them dozens of instructions later


EPI_DEPTH = 6    # SwiGLU backward: gu row blocks loaded this many rounds ahead (staging in the free fragment VGPRs)



def epilogue_swiglu_bwd(a: Asm):
    """The SwiGLU backward epilogue (acc = ds, never stored; gu rows: gate at
    n, up at F + n) with its gu loads software-pipelined: 16 rounds (8 row
    blocks x 2 column halves), round r's 4 loads issued EPI_DEPTH rounds
    ahead into staging slots in the main loop's fragment VGPRs (free here),
    each round waiting only for its own loads (counted vmcnt: VMEM completes
    in issue order) instead of draining every load and store per round -- the
    round-4 form exposed a full memory latency 32 times per tile (59 % MFMA
    busy in the model, profiles/r5_pmc)."""
    a(f"s_mov_b32 {sr(S_E0)}, 0")                             # dgu row block
    a(f"s_lshl_b32 {sr(S_E1)}, {sr(S_LDC)}, 4")
    a(f"s_mov_b32 {sr(S_T2)}, 0")                             # gu row block of the next prefetch
    a(f"s_lshl_b32 {sr(S_T1)}, {sr(S_LDS)}, 4")
    # pairs (the math runs on v_pk_*_f32): -log2 e (V_E + 4), 1.0 (V_E + 6), -1.0 (V_E + 10)
    for x in (4, 5):
        a(f"v_mov_b32 {vr(V_E + x)}, {-LOG2E!r}")
    for x in (6, 7):
        a(f"v_mov_b32 {vr(V_E + x)}, 1.0")
    for x in (10, 11):
        a(f"v_mov_b32 {vr(V_E + x)}, -1.0")
    rounds = [(j, half) for j in range(8) for half in range(2)]
    D = EPI_DEPTH
    seq: list = []     # VMEM ops in issue order: ("L" | "S", round)

    def slot(r):
        return V_FX0 + 16 * (r % D)                           # lg = slot, lu = slot + 8

    def issue_loads(r):
        j, half = rounds[r]
        lg, lu = slot(r), slot(r) + 8
        for q, p in enumerate((2 * half, 2 * half + 1)):
            a(f"buffer_load_dwordx4 {vr(lg + 4 * q, 4)}, {vr(V_E + 1)}, {sr(SRD_S, 4)}, {sr(S_T2)} offen offset:{64 * p}")
            a(f"buffer_load_dwordx4 {vr(lu + 4 * q, 4)}, {vr(V_E + 3)}, {sr(SRD_S, 4)}, {sr(S_T2)} offen offset:{64 * p}")
            seq.extend([("L", r), ("L", r)])
        if half == 1:
            a(f"s_add_u32 {sr(S_T2)}, {sr(S_T2)}, {sr(S_T1)}")   # the next prefetch reads the next row block

    for r in range(min(D, len(rounds))):
        issue_loads(r)
    for r, (j, half) in enumerate(rounds):
        ps_ = (2 * half, 2 * half + 1)
        d = V_E + 24                        # 16 f32: ds (no memory dependency: first)
        for q, p in enumerate(ps_):
            read_pair(a, d + 8 * q, p, j)
        pd = V_E + 40                       # bf16-rounded ds, then unpacked
        for q in range(2):
            cvt_pack8(a, pd + 4 * q, d + 8 * q)
        for q in range(2):
            unpack8(a, d + 8 * q, pd + 4 * q)
        last = max(i for i, x in enumerate(seq) if x == ("L", r))
        a(f"s_waitcnt vmcnt({min(63, len(seq) - last - 1)})")   # this round's loads only
        lg, lu = slot(r), slot(r) + 8
        gf, uf = V_E + 48, V_E + 64
        for q in range(2):
            unpack8(a, gf + 8 * q, lg + 4 * q)
            unpack8(a, uf + 8 * q, lu + 4 * q)
        if r + D < len(rounds):
            issue_loads(r + D)              # into the slot just unpacked
        sg, tmp, tt = V_E + 80, V_E + 96, V_E + 8
        for e in range(0, 16, 2):           # sg = 1 / (1 + exp(-g))
            a(f"v_pk_mul_f32 {vr(sg + e, 2)}, {vr(V_E + 4, 2)}, {vr(gf + e, 2)}")
        for e in range(16):
            a(f"v_exp_f32 {vr(sg + e)}, {vr(sg + e)}")
        for e in range(0, 16, 2):
            a(f"v_pk_add_f32 {vr(sg + e, 2)}, {vr(V_E + 6, 2)}, {vr(sg + e, 2)}")
        for e in range(16):
            a(f"v_rcp_f32 {vr(sg + e)}, {vr(sg + e)}")
        for e in range(0, 16, 2):           # du = d * g * sg  -> tmp
            a(f"v_pk_mul_f32 {vr(tmp + e, 2)}, {vr(d + e, 2)}, {vr(gf + e, 2)}")
            a(f"v_pk_mul_f32 {vr(tmp + e, 2)}, {vr(tmp + e, 2)}, {vr(sg + e, 2)}")
        for e in range(0, 16, 2):           # dg = d * u * sg * (1 + g (1 - sg)) -> uf
            a(f"v_pk_fma_f32 {vr(tt, 2)}, {vr(sg + e, 2)}, {vr(V_E + 10, 2)}, {vr(V_E + 6, 2)}")
            a(f"v_pk_fma_f32 {vr(tt, 2)}, {vr(gf + e, 2)}, {vr(tt, 2)}, {vr(V_E + 6, 2)}")
            a(f"v_pk_mul_f32 {vr(uf + e, 2)}, {vr(d + e, 2)}, {vr(uf + e, 2)}")
            a(f"v_pk_mul_f32 {vr(uf + e, 2)}, {vr(uf + e, 2)}, {vr(sg + e, 2)}")
            a(f"v_pk_mul_f32 {vr(uf + e, 2)}, {vr(uf + e, 2)}, {vr(tt, 2)}")
        pdg, pdu = V_E + 40, V_E + 112      # 8 + 4 regs: reuse gf for the last du pair
        for q in range(2):
            cvt_pack8(a, pdg + 4 * q, uf + 8 * q)
        cvt_pack8(a, pdu, tmp)
        cvt_pack8(a, gf, tmp + 8)
        for q, p in enumerate(ps_):
            store16(a, pdg + 4 * q, V_E, SRD_C, S_E0, p)
        store16(a, pdu, V_E + 2, SRD_C, S_E0, ps_[0])
        store16(a, gf, V_E + 2, SRD_C, S_E0, ps_[1])
        seq.extend([("S", r)] * 4)
        a("s_nop 1")                        # store data read before the next round rewrites it
        if half == 1:
            a(f"s_add_u32 {sr(S_E0)}, {sr(S_E0)}, {sr(S_E1)}")



# ---------------------------------------------------------------- kernel
def kernel(epi: str, trace: bool = False, variant: str = "") -> tuple[str, str]:
    """trace=True: the diagnostic trace variant of the plain kernel (markers
    into a host-coherent buffer in the S slot; toa_gemm_tn_asm_trace).
    variant: the name suffix of a kernel generated under _with_knobs (the
    persistent arms, the timing kernels)."""
    name = "toa_gemm_tn_asm_trace" if trace else f"toa_gemm_tn_asm_{epi}" + (f"_{variant}" if variant else "")
    if SCHED["timing"]:
        name = "toa_gemm_tn_asm_timing" + ("" if SCHED["timing"] == 1 else str(SCHED["timing"]))
    a = Asm(prefix=("trace_" if trace else epi + "_" + (variant + "_" if variant else "")))
    a.raw(f".globl {name}")
    a.raw(".p2align 8")
    a.raw(f".type {name},@function")
    a.raw(f"{name}:")
    prologue(a, epi)
    timing = SCHED["timing"]
    if timing:
        a(f"s_memtime {sr(S_T_START, 2)}")
        for k in range(3):
            a(f"s_mov_b32 {sr(S_ACC + k)}, 0")
    if trace:
        for ins in trace_setup(a) + trace_mark(1):
            a(ins)
    # --- prologue DMA: tile 0 -> stage 0, tile 1 -> stage 1
    prologue_dma(a)
    # 256 accumulator writes while the first tiles are in flight, not ahead
    # of their DMA (~1k issue cycles per tile off the critical path)
    zero_acc(a)
    # both stages toggled twice: M0 bases are back at stage 0 for tile 2
    a("s_waitcnt vmcnt(16)")                       # own tile-0 pieces
    a("s_barrier")                                 # everyone's
    if trace:
        for ins in trace_mark(2):
            a(ins)
    if epi == "plain" and not trace and not variant:
        stage_exit(a, 1)
    persist = SCHED["persist"]
    assert not persist or (not trace and not SCHED["timing"])
    l_tile = a.fresh("tile")
    if persist:
        a.label(l_tile)
    for j in range(8):
        a(frag_read("x", j, 0))
    for i in range(8):
        a(frag_read("w", i, 0))
    a("s_waitcnt lgkmcnt(0)")
    a(f"s_sub_u32 {sr(S_LOOP)}, {sr(S_KT)}, 2")
    l_loop, l_tail = a.fresh("loop"), a.fresh("tail")
    a(f"s_cmp_eq_u32 {sr(S_LOOP)}, 0")
    a(f"s_cbranch_scc1 {l_tail}")
    a(".p2alignl 6, 0xbf800000")   # loop head on a 64-byte boundary (s_nop padding)
    a.label(l_loop)
    iteration_map(a, with_dma=True, next_reads=True)
    a(f"s_sub_u32 {sr(S_LOOP)}, {sr(S_LOOP)}, 1")
    a(f"s_cmp_eq_u32 {sr(S_LOOP)}, 0")
    a(f"s_cbranch_scc0 {l_loop}")
    a.label(l_tail)
    iteration_map(a, with_dma=False, next_reads=True)
    iteration_map(a, with_dma=False, next_reads=False)
    if epi == "plain" and not trace and not variant:
        stage_exit(a, 2)
    if timing:
        a(_stamp(0))                                # main loop done
    # MFMA results -> VALU reads: let the last MFMAs retire
    a("s_nop 15")
    a("s_nop 15")
    if trace:
        for ins in trace_mark(9000):
            a(ins)
    if persist:
        persistent_next(a, epi, l_tile)
    if epi != "rope":
        epi_offsets(a, epi)
    {"plain": epilogue_plain, "swiglu_fwd": epilogue_swiglu_fwd, "swiglu_bwd": epilogue_swiglu_bwd,
     "rope": epilogue_rope, "delta": epilogue_delta, "resadd": epilogue_resadd}[epi](a)
    if trace or timing:
        a("s_waitcnt vmcnt(0)")
    # else: end with the epilogue's stores still in flight -- the wave's end
    # does not wait for them, so the next workgroup on this CU starts its
    # prologue while they drain (the hardware completes them)
    if timing:
        # record per (workgroup, wave): vm wait, X-free barrier, W-free barrier,
        # start -> loop end, epilogue, k-tiles, workgroup id, 0 (cycles)
        a(_stamp(1))
        a("s_waitcnt lgkmcnt(0)")
        a(f"s_sub_u32 {sr(S_TMT + 4)}, {sr(S_TMT)}, {sr(S_T_START)}")
        a(f"s_sub_u32 {sr(S_TMT + 5)}, {sr(S_TMT + 2)}, {sr(S_TMT)}")
        for ins in trace_setup(a):
            a(ins)
        for k, src in enumerate((sr(S_ACC), sr(S_ACC + 1), sr(S_ACC + 2), sr(S_TMT + 4), sr(S_TMT + 5), sr(S_KT),
                                 "s2", "0")):
            a(f"v_mov_b32 {vr(V_T + 2)}, {src}")
            a(f"buffer_store_dword {vr(V_T + 2)}, {vr(V_T + 3)}, {sr(SRD_S, 4)}, 0 offen offset:{4 * k}")
        a("s_waitcnt vmcnt(0)")
    if trace:
        for ins in trace_setup(a)[-3:] + trace_mark(9999):
            a(ins)
    a.label(a.abort)
    a("s_endpgm")
    if epi == "plain" and not trace and not variant:
        a.label(a.stage_exit)
        a("s_waitcnt vmcnt(0)")
        a("s_endpgm")
    a.raw(f".size {name}, .-{name}")
    body = "\n".join(a.out)
    # the delta epilogue's partial sums: 4 waves x 256 B of LDS past the stages
    desc, meta = _descriptor(name, lds_bytes=LDS_BYTES + 1024 if epi == "delta" else None)
    return body + "\n" + desc, meta


def prologue_dma(a: Asm):
    """k-tiles 0 and 1 of the tile -> stages 0 and 1 (M0 bases end at stage 0)."""
    for _ in range(2):
        for half in ("x", "w"):
            for j in range(8):
                for ins in dma(a, half, j):
                    a(ins)
            for ins in advance(half):
                a(ins)
        a(f"s_xor_b32 {sr(S_M0X)}, {sr(S_M0X)}, {sr(S_M0XT)}")
        a(f"s_xor_b32 {sr(S_M0W)}, {sr(S_M0W)}, {sr(S_M0WT)}")


def persistent_next(a: Asm, epi: str, l_tile: str):
    """Persistent arms: this workgroup's next tile is S_ITER + grid.  If there
    is one, its first two k-tiles are staged (every wave's reads of the
    current tile are done: barrier) BEFORE the current tile's epilogue, so
    their flight hides under the epilogue; then the epilogue, the next tile's
    C resource, zeroed accumulators, and back to the tile loop."""
    l_last, l_even, l_par = a.fresh("last"), a.fresh("even"), a.fresh("par")
    # stage parity back to 0: the M0 bases toggled KT times this tile, the read bases KT - 1
    a(f"s_bitcmp1_b32 {sr(S_KT)}, 0")
    a(f"s_cbranch_scc0 {l_even}")
    a(f"s_xor_b32 {sr(S_M0X)}, {sr(S_M0X)}, {sr(S_M0XT)}")
    a(f"s_xor_b32 {sr(S_M0W)}, {sr(S_M0W)}, {sr(S_M0WT)}")
    a(f"s_branch {l_par}")
    a.label(l_even)
    a(f"v_xor_b32 {vr(V_RX)}, {vr(V_RX)}, {vr(V_RXT)}")
    a(f"v_xor_b32 {vr(V_RW)}, {vr(V_RW)}, {vr(V_RWT)}")
    a.label(l_par)
    a(f"s_add_u32 {sr(S_ITER)}, {sr(S_ITER)}, {sr(S_GRID)}")
    a(f"s_mul_i32 {sr(S_T0)}, {sr(S_TM_N)}, {sr(S_TN_N)}")
    a(f"s_cmp_ge_u32 {sr(S_ITER)}, {sr(S_T0)}")
    a(f"s_cbranch_scc1 {l_last}")
    a("s_barrier")                                 # every wave done reading this tile's LDS
    tile_setup(a, epi, sr(S_ITER))                 # SRD_X / SRD_W / (S_TM, S_TN) of the next tile
    prologue_dma(a)
    epi_offsets(a, epi)
    n0 = len(a.out)
    {"plain": epilogue_plain, "swiglu_fwd": epilogue_swiglu_fwd, "swiglu_bwd": epilogue_swiglu_bwd}[epi](a)
    n_vm = sum(1 for ins in a.out[n0:] if ins.lstrip().startswith(("buffer_load", "buffer_store")))
    tile_c(a, epi)
    zero_acc(a)
    # the next tile's k-tile 0 landed: k-tile 1's 16 pieces and the epilogue's
    # loads / stores are younger (plain: 32 stores -> 48; the SwiGLU epilogues
    # issue more than the counter holds, and their own waits already retired
    # everything up to their last load: 63 is then no wait at all)
    a(f"s_waitcnt vmcnt({min(63, 16 + n_vm)})")
    a("s_barrier")
    a(f"s_branch {l_tile}")
    a.label(l_last)


# ---------------------------------------------------------------- NN form
# C[m][n] = sum_k X[m][k] * W[k][n]: the data gradient dX = dY W read from the
# weight AS STORED ([K = out features, N = in features], row stride ldw), so
# no transposed copy of W is kept.  The TN kernel's X half (lines, LDS-DMA,
# ds_read_b128) plus the weight-gradient kernel's operand image for W
# (wgrad_gen: a 64 (k) x 256 (n) window per k-tile, row pairs as one-DMA
# blocks at blockbase, fragments through ds_read_b64_tr_b16 from two base
# VGPRs, rows +0 and +4).  A lane's W fragment holds k = 32 sub + 8 (l >> 4)
# .. +7 (two transposed reads), the k of its X fragment's ds_read_b128.
#
# The accumulators keep the TN kernels' shape (fragments 2p and 2p + 1 give a
# lane the 8 consecutive columns of one 16-byte chunk), so every epilogue
# applies: source lane (g, q, p) = (l >> 4, (l >> 2) & 3, l & 3) of fragment i
# reads row 8 g + q, chunk 4 (i >> 1) + p of the wave's 16, and of that chunk
# the 8-byte half (i & 1) ^ par(p), par(p) = (p & 1) ^ (p >> 1).  Were the
# half i & 1 in every lane (TN's layout exactly), the 32 lanes of a read would
# reach only every other pair of banks (chunks sit on 16-byte boundaries: the
# LDS-DMA places 16 bytes per lane): 2-way conflicts.  With par the four
# pieces of a row fall at 0, 24, 72, 80 (mod 32: 0, 24, 8, 16) and the eight
# rows of a read group at multiples of 32 mod 256: every bank once, 2 LDS
# cycles per read (tests/test_asm_gemm_nn.py).  The price: in lane groups 1
# and 2 (par = 1) fragment 2p holds the chunk's upper half and 2p + 1 its
# lower; read_pair puts them in order with two EXEC-masked passes of
# v_accvgpr_read (256 more per tile), the only change to the epilogues.  The
# half is part of the read base, so odd fragments have bases of their own.
#
# LDS per stage: X half (HALF) + W image (wgrad_gen.OPER) = 72640 B, two
# stages 145280 B, the delta epilogue's 1 KiB behind them.
NN_EPIS = ("plain", "swiglu_bwd", "delta")
# W read bases and stage toggles beside V_RW / V_RWT (even fragments, rows +0): rows +4, and both for the odd
# fragments (main loop only: epilogue scratch)
V_RWH, V_RWHT, V_RWO, V_RWOT, V_RWHO, V_RWHOT = (V_E + k for k in range(4, 10))
NN_BASES = ((V_RW, V_RWT), (V_RWH, V_RWHT), (V_RWO, V_RWOT), (V_RWHO, V_RWHOT))


def _wgrad():
    import wgrad_gen   # lazy: it imports this module
    return wgrad_gen


def nn_layout() -> tuple[int, int]:
    """(bytes per stage, LDS bytes of the two stages) of the NN kernels."""
    stage = HALF + _wgrad().OPER
    return stage, 2 * stage


def nn_frag_offset(i: int, sub: int) -> int:
    """Immediate of W fragment i, sub-step `sub`, from the lane's read base
    (of its parity: the chunk's half is in the base)."""
    wg = _wgrad()
    return wg.pos(0, 4 * (i >> 1)) + wg.SUB1 * sub


def nn_lanes(a: Asm):
    """The W side's lane state after prologue_lanes (V_T = w, V_T + 1 = lane
    still hold; its TN values of these registers are replaced): V_DW, the
    piece offsets, the M0 bases, the two read bases and their toggles."""
    wg = _wgrad()
    stage, _ = nn_layout()
    v = V_T
    # DMA: wave w's piece j is block 8 w + j of the window (rows 16 w + 2 j + s)
    wg.dma_lane(a, v, V_E)
    a(f"v_mul_lo_u32 {vr(V_DW)}, {vr(v + 2)}, {sr(S_LDW)}")
    a(f"v_add_u32 {vr(V_DW)}, {vr(V_DW)}, {vr(v + 3)}")
    for j in range(1, 8):
        a(f"s_mul_i32 {sr(S_SOW + j - 1)}, {sr(S_LDW)}, {2 * j}")
    a("s_nop 4")
    a(f"v_readfirstlane_b32 {sr(S_T0)}, {vr(v)}")              # w
    a("s_nop 4")
    a(f"s_mul_i32 {sr(S_M0W)}, {sr(S_T0)}, {wg.blockbase(8)}")
    a(f"s_add_u32 {sr(S_M0W)}, {sr(S_M0W)}, {HALF}")
    a(f"s_add_u32 {sr(S_M0WT)}, {sr(S_M0W)}, {stage}")
    a(f"s_xor_b32 {sr(S_M0WT)}, {sr(S_M0WT)}, {sr(S_M0W)}")
    # read bases: pos(8 g + q, p) + the wave's 128 columns, rows +4 two blocks on
    a(f"v_lshrrev_b32 {vr(v + 2)}, 4, {vr(v + 1)}")                 # g
    a(f"v_bfe_u32 {vr(v + 3)}, {vr(v + 1)}, 3, 1")                  # q >> 1
    a(f"v_lshl_add_u32 {vr(v + 2)}, {vr(v + 2)}, 2, {vr(v + 3)}")   # block 4 g + (q >> 1)
    a(f"v_bfe_u32 {vr(v + 3)}, {vr(v + 1)}, 2, 1")                  # q & 1: the block's second row
    a(f"v_lshlrev_b32 {vr(v + 3)}, 5, {vr(v + 3)}")
    a(f"v_bfe_u32 {vr(V_E)}, {vr(v + 1)}, 1, 1")                    # p >> 1: chunk pair
    a(f"v_lshl_add_u32 {vr(v + 3)}, {vr(V_E)}, 6, {vr(v + 3)}")
    a(f"v_and_b32 {vr(V_E)}, 1, {vr(v + 1)}")                       # p & 1: chunk of the pair
    a(f"v_lshl_add_u32 {vr(v + 3)}, {vr(V_E)}, 4, {vr(v + 3)}")
    a(f"v_lshrrev_b32 {vr(V_E)}, 1, {vr(v)}")                       # wn
    a(f"v_lshl_add_u32 {vr(v + 3)}, {vr(V_E)}, 9, {vr(v + 3)}")     # 128 columns = 16 chunks
    a(f"v_add_u32 {vr(v + 3)}, {HALF}, {vr(v + 3)}")
    # the chunk's half: 8 par(p) for even fragments, 8 (1 - par(p)) for odd ones
    a(f"v_bfe_u32 {vr(V_E)}, {vr(v + 1)}, 1, 1")
    a(f"v_and_b32 {vr(V_E + 1)}, 1, {vr(v + 1)}")
    a(f"v_xor_b32 {vr(V_E)}, {vr(V_E)}, {vr(V_E + 1)}")             # par(p)
    a(f"v_lshlrev_b32 {vr(V_E)}, 3, {vr(V_E)}")
    a(f"v_add_u32 {vr(V_E + 10)}, {vr(v + 3)}, {vr(V_E)}")
    a(f"v_sub_u32 {vr(V_E + 11)}, {vr(v + 3)}, {vr(V_E)}")
    a(f"v_add_u32 {vr(V_E + 11)}, 8, {vr(V_E + 11)}")
    for dst, dblock, part in ((V_RW, 0, V_E + 10), (V_RWH, 2, V_E + 10), (V_RWO, 0, V_E + 11),
                              (V_RWHO, 2, V_E + 11)):
        a(f"v_add_u32 {vr(V_E + 1)}, {dblock}, {vr(v + 2)}")
        wg.blockbase_v(a, V_E + 2, V_E + 1, V_E + 3)
        a(f"v_add_u32 {vr(dst)}, {vr(V_E + 2)}, {vr(part)}")
    for base, tg in NN_BASES:
        a(f"v_add_u32 {vr(tg)}, {stage}, {vr(base)}")
        a(f"v_xor_b32 {vr(tg)}, {vr(tg)}, {vr(base)}")


def nn_m0_step(half: str, j: int) -> int:
    """M0 from piece j to piece j + 1."""
    wg = _wgrad()
    return 4 * LINE if half == "x" else wg.blockbase(j + 1) - wg.blockbase(j)


def nn_advance(half: str) -> list[str]:
    if half == "x":
        return advance("x")
    return [f"s_add_u32 {sr(SRD_W)}, {sr(SRD_W)}, {sr(S_ADVW)}", f"s_addc_u32 {sr(SRD_W + 1)}, {sr(SRD_W + 1)}, 0"]


def nn_frag_reads(i: int, sub: int) -> list[str]:
    dst = (V_FW0 if sub == 0 else V_FW1) + 4 * i
    off = nn_frag_offset(i, sub)
    lo, hi = (V_RWO, V_RWHO) if i & 1 else (V_RW, V_RWH)
    return [f"ds_read_b64_tr_b16 {vr(dst, 2)}, {vr(lo)} offset:{off}",
            f"ds_read_b64_tr_b16 {vr(dst + 2, 2)}, {vr(hi)} offset:{off}"]


def nn_prologue_dma(a: Asm):
    """k-tiles 0 and 1 -> stages 0 and 1 (M0 bases end at stage 0)."""
    for _ in range(2):
        for half, srd_, vo, so, m0 in (("x", SRD_X, V_DX, S_SOX, S_M0X), ("w", SRD_W, V_DW, S_SOW, S_M0W)):
            a(f"s_mov_b32 m0, {sr(m0)}")
            for j in range(8):
                a("s_nop 0")                     # M0 -> LDS-DMA hazard (dma())
                soff = "0" if j == 0 else sr(so + j - 1)
                a(f"buffer_load_dwordx4 {vr(vo)}, {sr(srd_, 4)}, {soff} offen lds")
                if j < 7:
                    a(f"s_add_u32 m0, m0, {nn_m0_step(half, j)}")
            for ins in nn_advance(half):
                a(ins)
        a(f"s_xor_b32 {sr(S_M0X)}, {sr(S_M0X)}, {sr(S_M0XT)}")
        a(f"s_xor_b32 {sr(S_M0W)}, {sr(S_M0W)}, {sr(S_M0WT)}")


def iteration_nn(a: Asm, with_dma: bool, next_reads: bool):
    """One 64-k tile of the NN loop on SLOT_MAP: a W slot carries the fragment's two transposed reads, so
    a sub-step issues 8 + 16 reads; the 16 DMA pieces, both barriers and the
    counted next-tile wait sit where the TN loop has them."""
    m = SLOT_MAP
    split, lag = m["split"], m["m0_lag"]
    slots: dict[int, list[str]] = {n: [] for n in range(128)}
    for j, n in enumerate(m["x1"]):
        slots[n].append(frag_read("x", j, 1))
    for i, n in enumerate(m["w1"]):
        slots[n] += nn_frag_reads(i, 1)
    assert max(m["x1"]) < m["xbar"] and max(m["w1"]) < m["wbar"]
    vm = 0
    if with_dma:
        for bar in (m["xbar"], m["wbar"]):
            slots[bar].append("s_waitcnt lgkmcnt(0)")
            slots[bar + split].append("s_barrier")
        for half, key, bar in (("x", "xdma", m["xbar"]), ("w", "wdma", m["wbar"])):
            srd_, vo, so, m0 = (SRD_X, V_DX, S_SOX, S_M0X) if half == "x" else (SRD_W, V_DW, S_SOW, S_M0W)
            pos = m[key]
            assert sorted(pos) == pos and pos[0] > bar + split and len(set(pos)) == 8
            slots[pos[0] - 1].append(f"s_mov_b32 m0, {sr(m0)}")
            for j, n in enumerate(pos):
                soff = "0" if j == 0 else sr(so + j - 1)
                slots[n].append(f"buffer_load_dwordx4 {vr(vo)}, {sr(srd_, 4)}, {soff} offen lds")
                if j < 7:
                    assert lag >= 1 and pos[j + 1] > n + lag      # an MFMA between an M0 write and the next piece
                    slots[n + lag].append(f"s_add_u32 m0, m0, {nn_m0_step(half, j)}")
            adv = m["adv"][half]
            assert pos[-1] <= adv < 128
            slots[adv] += nn_advance(half) + [f"s_xor_b32 {sr(m0)}, {sr(m0)}, {sr(m0 + 1)}"]
        assert max(m["xdma"]) + lag < min(m["wdma"]) - 1          # one running M0
        vm = sum(1 for n in m["xdma"] + m["wdma"] if n < m["wait"])
    if next_reads:
        w = m["wait"]
        slots[w].append(f"s_waitcnt vmcnt({vm})")
        slots[w + split] += ["s_barrier"] + [f"v_xor_b32 {vr(b)}, {vr(b)}, {vr(t)}"
                                             for b, t in ((V_RX, V_RXT),) + NN_BASES]
        assert min(m["x0"] + m["w0"]) > w + split and max(m["x0"] + m["w0"]) < 126
        for j, n in enumerate(m["x0"]):
            slots[n].append(frag_read("x", j, 0))
        for i, n in enumerate(m["w0"]):
            slots[n] += nn_frag_reads(i, 0)
        slots[126].append("s_waitcnt lgkmcnt(0)")
    for n in range(128):
        sub, mm = divmod(n, 64)
        i, j = divmod(mm, 8)
        if n == 64:
            a("s_waitcnt lgkmcnt(0)")
        a(".p2alignl 3, 0xbf800000")
        a(mfma(i, j, sub))
        for ins in slots[n]:
            a(ins)


def kernel_nn(epi: str) -> tuple[str, str]:
    """toa_gemm_nn_asm_<epi>: the kernarg block is KARG with `ldw` the row
    stride of W [K, N] and ktiles = K / 64; tiles, tile order, M tail
    (kernarg `m`) and argument guard are the TN kernels'."""
    assert epi in NN_EPIS
    name = f"toa_gemm_nn_asm_{epi}"
    stage, lds = nn_layout()
    g = globals()
    saved = {k: g[k] for k in ("STAGE", "LDS_BYTES", "NN_SWAP")}
    g["STAGE"], g["LDS_BYTES"] = stage, lds      # the X half's toggles, the delta epilogue's scratch
    g["NN_SWAP"] = True                          # read_pair: lane groups 1, 2 hold their fragment pairs swapped
    try:
        a = Asm(prefix=f"nn_{epi}_")
        a.raw(f".globl {name}")
        a.raw(".p2align 8")
        a.raw(f".type {name},@function")
        a.raw(f"{name}:")
        prologue(a, epi, form="nn")
        nn_prologue_dma(a)
        zero_acc(a)                                    # under the first tiles' flight
        a("s_waitcnt vmcnt(16)")                       # own tile-0 pieces
        a("s_barrier")                                 # everyone's
        for j in range(8):
            a(frag_read("x", j, 0))
        for i in range(8):
            for ins in nn_frag_reads(i, 0):
                a(ins)
        a("s_waitcnt lgkmcnt(0)")
        a(f"s_sub_u32 {sr(S_LOOP)}, {sr(S_KT)}, 2")
        l_loop, l_tail = a.fresh("loop"), a.fresh("tail")
        a(f"s_cmp_eq_u32 {sr(S_LOOP)}, 0")
        a(f"s_cbranch_scc1 {l_tail}")
        a(".p2alignl 6, 0xbf800000")
        a.label(l_loop)
        iteration_nn(a, with_dma=True, next_reads=True)
        a(f"s_sub_u32 {sr(S_LOOP)}, {sr(S_LOOP)}, 1")
        a(f"s_cmp_eq_u32 {sr(S_LOOP)}, 0")
        a(f"s_cbranch_scc0 {l_loop}")
        a.label(l_tail)
        iteration_nn(a, with_dma=False, next_reads=True)
        iteration_nn(a, with_dma=False, next_reads=False)
        a("s_nop 15")                                  # MFMA results -> VALU reads
        a("s_nop 15")
        for r, word in ((S_EX_SAME, 0x0000FFFF), (S_EX_SAME + 1, 0xFFFF0000), (S_EX_SWAP, 0xFFFF0000),
                        (S_EX_SWAP + 1, 0x0000FFFF)):
            a(f"s_mov_b32 {sr(r)}, {word:#x}")
        epi_offsets(a, epi)
        {"plain": epilogue_plain, "swiglu_bwd": epilogue_swiglu_bwd, "delta": epilogue_delta}[epi](a)
        a.label(a.abort)
        a("s_endpgm")
        a.raw(f".size {name}, .-{name}")
        desc, meta = _descriptor(name, lds_bytes=lds + (1024 if epi == "delta" else 0))
        return "\n".join(a.out) + "\n" + desc, meta
    finally:
        g.update(saved)


TRACE_REC = 32   # bytes per (workgroup, wave) trace record


def trace_setup(a: Asm) -> list[str]:
    """Diagnostic trace kernel only: SRD over the host-coherent trace buffer
    (pointer in the S slot), V_T+3 = this wave's record offset."""
    return [f"s_mov_b32 {sr(SRD_S)}, {sr(S_S)}", f"s_mov_b32 {sr(SRD_S + 1)}, {sr(S_S + 1)}",
            f"s_mul_i32 {sr(SRD_S + 2)}, {sr(S_TM_N)}, {sr(S_TN_N)}",
            f"s_mul_i32 {sr(SRD_S + 2)}, {sr(SRD_S + 2)}, {4 * TRACE_REC}",
            f"s_mov_b32 {sr(SRD_S + 3)}, 0x20000", "s_mov_b32 s71, 0",
            f"v_lshrrev_b32 {vr(V_T + 3)}, 6, {vr(V_TID)}",
            f"v_lshl_add_u32 {vr(V_T + 3)}, s2, 2, {vr(V_T + 3)}",
            f"v_mul_u32_u24 {vr(V_T + 3)}, {TRACE_REC}, {vr(V_T + 3)}"]


def trace_mark(code: int) -> list[str]:
    """Record (code, loop counter, M0, SRD_X lo, SRD_W lo, M0 bases, seq) for
    this wave, system-coherent, drained: after a fault the host reads how far
    every wave got (scripts/asm_gemm_bench.py --trace)."""
    out = ["s_add_u32 s71, s71, 1"]
    for k, src in enumerate((str(code), sr(S_LOOP), "m0", sr(SRD_X), sr(SRD_W), sr(S_M0X), sr(S_M0W), "s71")):
        out.append(f"v_mov_b32 {vr(V_T + 2)}, {src}")
        out.append(f"buffer_store_dword {vr(V_T + 2)}, {vr(V_T + 3)}, {sr(SRD_S, 4)}, 0 offen offset:{4 * k} sc0 sc1")
    out.append("s_waitcnt vmcnt(0)")
    return out


def stage_exit(a: Asm, stage: int):
    """Diagnostic (plain kernel only, whose fc argument is otherwise unused):
    fc == stage ends the workgroup here, after draining its DMA -- bisects a
    hardware fault by how far the kernel gets (scripts/asm_gemm_bench.py)."""
    a(f"s_cmp_eq_u32 {sr(S_FC)}, {stage}")
    a(f"s_cbranch_scc1 {a.stage_exit}")


def _descriptor(name: str, lds_bytes: int | None = None, n_sgpr: int | None = None,
                karg_bytes: int | None = None) -> tuple[str, str]:
    LDS_BYTES = globals()["LDS_BYTES"] if lds_bytes is None else lds_bytes  # noqa: N806
    N_SGPR = globals()["N_SGPR"] if n_sgpr is None else n_sgpr  # noqa: N806
    KARG_BYTES = globals()["KARG_BYTES"] if karg_bytes is None else karg_bytes  # noqa: N806
    desc = f"""
.rodata
.p2align 6
.amdhsa_kernel {name}
  .amdhsa_group_segment_fixed_size {LDS_BYTES}
  .amdhsa_private_segment_fixed_size 0
  .amdhsa_kernarg_size {KARG_BYTES}
  .amdhsa_user_sgpr_count 2
  .amdhsa_user_sgpr_kernarg_segment_ptr 1
  .amdhsa_system_sgpr_workgroup_id_x 1
  .amdhsa_system_vgpr_workitem_id 0
  .amdhsa_next_free_vgpr 512
  .amdhsa_next_free_sgpr {N_SGPR}
  .amdhsa_accum_offset 256
  .amdhsa_reserve_vcc 1
  .amdhsa_float_denorm_mode_32 3
  .amdhsa_float_denorm_mode_16_64 3
  .amdhsa_dx10_clamp 1
  .amdhsa_ieee_mode 1
.end_amdhsa_kernel
.text
"""
    meta = f"""  - .args:
      - .offset: 0
        .size: {KARG_BYTES}
        .value_kind: by_value
    .group_segment_fixed_size: {LDS_BYTES}
    .kernarg_segment_align: 8
    .kernarg_segment_size: {KARG_BYTES}
    .max_flat_workgroup_size: 256
    .name: {name}
    .private_segment_fixed_size: 0
    .sgpr_count: {N_SGPR + 6}
    .sgpr_spill_count: 0
    .symbol: {name}.kd
    .vgpr_count: 512
    .agpr_count: 256
    .vgpr_spill_count: 0
    .wavefront_size: 64
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .language: OpenCL C
    .language_version:
      - 2
      - 0
"""
    return desc, meta


PROBE_SGPRS = 72   # s0..s71: what the plain prologue writes (the timing kernel's s72.. are not dumped)
PROBE_MAGIC = (0x626F7270, 0x31657461)   # "prob" "ate1" in the fw / fc argument slots


def probe_kernel() -> tuple[str, str]:
    """Diagnostic kernel: the plain kernel's prologue, then a dump of every
    SGPR s0..s71 and, per thread, the DMA / fragment / epilogue offsets to
    the buffer in the S argument slot -- ONLY when fw / fc hold PROBE_MAGIC
    (a kernarg block that did not arrive intact stores nothing).  Compared
    with the emulator's dump of the same prologue (tests/test_asm_gemm.py,
    scripts/asm_gemm_bench.py --probe)."""
    name = "toa_gemm_tn_asm_probe"
    a = Asm(prefix="probe_")
    a.raw(f".globl {name}")
    a.raw(".p2align 8")
    a.raw(f".type {name},@function")
    a.raw(f"{name}:")
    prologue(a, "plain")
    epi_offsets(a, "plain")
    end = a.fresh("end")
    a(f"s_cmp_eq_u32 {sr(S_FW)}, {PROBE_MAGIC[0]:#x}")
    a(f"s_cbranch_scc0 {end}")
    a(f"s_cmp_eq_u32 {sr(S_FC)}, {PROBE_MAGIC[1]:#x}")
    a(f"s_cbranch_scc0 {end}")
    # workgroup b dumps to S + b * PROBE_WORDS * 4
    a(f"s_mul_i32 {sr(S_E0)}, s2, {PROBE_WORDS * 4}")
    a(f"s_add_u32 {sr(SRD_S)}, {sr(S_S)}, {sr(S_E0)}")
    a(f"s_addc_u32 {sr(SRD_S + 1)}, {sr(S_S + 1)}, 0")
    a(f"s_mov_b32 {sr(SRD_S + 2)}, {PROBE_WORDS * 4}")
    a(f"s_mov_b32 {sr(SRD_S + 3)}, 0x20000")
    a(f"v_mov_b32 {vr(V_T + 1)}, 0")
    for r in range(PROBE_SGPRS):
        if r in (SRD_S, SRD_S + 1, SRD_S + 2, SRD_S + 3, S_E0):
            continue
        a(f"v_mov_b32 {vr(V_T)}, {sr(r)}")
        a(f"buffer_store_dword {vr(V_T)}, {vr(V_T + 1)}, {sr(SRD_S, 4)}, 0 offen offset:{4 * r}")
    a(f"v_mov_b32 {vr(V_T)}, m0")
    a(f"buffer_store_dword {vr(V_T)}, {vr(V_T + 1)}, {sr(SRD_S, 4)}, 0 offen offset:{4 * PROBE_SGPRS}")
    # per thread: 8 words at 4 * (PROBE_VBASE + 8 tid)
    a(f"v_lshlrev_b32 {vr(V_T + 1)}, 5, {vr(V_TID)}")
    for k, reg in enumerate((V_DX, V_DW, V_RX, V_RW, V_RXT, V_RWT, V_E, V_TID)):
        a(f"buffer_store_dword {vr(reg)}, {vr(V_T + 1)}, {sr(SRD_S, 4)}, 0 offen offset:{4 * (PROBE_VBASE + k)}")
    a("s_waitcnt vmcnt(0)")
    a.label(end)
    a.label(a.abort)
    a("s_endpgm")
    a.raw(f".size {name}, .-{name}")
    body = "\n".join(a.out)
    desc, meta = _descriptor(name)
    return body + "\n" + desc, meta


PROBE_VBASE = 128
PROBE_WORDS = PROBE_VBASE + 8 * 256


# The persistent plain kernel (a workgroup per CU walks its tiles, the next
# tile staged under the epilogue), launched by toa_gemm_asm_set_persist /
# TOA_ASM_PERSIST.
PLAIN_VARIANTS = (("v3", {"persist": True}),)
# measured (profiles/r4_asm_gemm/ab1..diag2): MFMAs on 8-byte boundaries, ending
# with the epilogue's stores in flight, two barriers per tile and the wait 16
# MFMAs earlier all within noise (+-1.5 %); LDS lines of 1040 B (same speed
# despite 2-way read conflicts), DMA pieces bunched after each barrier
# (-2..-4 %) and groups of 16 row tiles (-1..-7 %) rejected; groups of 4, the
# next-tile wait at MFMA 95 and the X-free barrier 16 MFMAs after the last X
# read taken into the product kernel (+1..+4 %); an L2 prefetch of the tile two
# beyond the DMA (one 4-B load per line, its own bounded resources) -16..-24 %
# (profiles/r4_asm_gemm/ab3): the extra loads share the counted vmcnt waits.
# Round 5 (profiles/r5_asm_gemm/): the SLOT_MAP placement (barriers one MFMA
# after their waits, M0 / resource advances one MFMA after the pieces) +0.5..2 %
# over the same slots without the lags at every form, taken into the product
# kernel; the library's second loop body for odd SIMDs (with and without MFMA
# alignment) -1..-3 %.  The arms themselves are pruned (docs/kernels.md).


# Persistent fused SwiGLU GEMMs (one workgroup per CU walks its tiles; the
# next tile's first two k-tiles are staged before the current tile's
# epilogue, so its gu loads / dgu stores overlap that DMA instead of a fresh
# workgroup's prologue): A/B arms with correct outputs, launched by
# toa_gemm_asm_set_swiglu_persist.
SWIGLU_PERSIST_VARIANTS = (("swiglu_fwd", "p1", {"persist": True}), ("swiglu_bwd", "p1", {"persist": True}))

# The timing diagnostics of the plain kernel (toa_gemm_asm_timing).
TIMING_VARIANTS = (("timing", {"timing": 1}), ("timing2", {"timing": 2}))


def _with_knobs(knobs: dict, fn):
    """Run fn() with the SCHED entries in `knobs` overridden."""
    saved = dict(SCHED)
    assert set(knobs) <= set(SCHED)
    SCHED.update(knobs)
    try:
        return fn()
    finally:
        SCHED.update(saved)


def generate() -> str:
    import attn_bwd_gen  # the attention forward, the dK / dV backward and the weight-gradient
    import attn_gen      # kernel share this code object (lazy: they import this module)
    import wgrad_gen

    kernels = [kernel(epi) for epi in EPIS]
    kernels += [_with_knobs(knobs, lambda: kernel("plain", variant=vname)) for vname, knobs in PLAIN_VARIANTS]
    kernels += [_with_knobs(knobs, lambda: kernel(epi, variant=vname)) for epi, vname, knobs in SWIGLU_PERSIST_VARIANTS]
    kernels += [wgrad_gen.kernel(), *attn_gen.all_kernels(), probe_kernel(), kernel("plain", trace=True)]
    kernels += [_with_knobs(knobs, lambda: kernel("plain", variant=vname)) for vname, knobs in TIMING_VARIANTS]
    kernels += attn_bwd_gen.all_kernels()
    kernels += [kernel_nn(epi) for epi in NN_EPIS]   # the data gradients on W as stored
    parts = ['.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', ".amdhsa_code_object_version 5", ".text"]
    parts += [body for body, _ in kernels]
    # what hipcc emits after the last kernel: s_nop padding, so the
    # instruction prefetcher never runs off the end of the code object
    parts.append(".text\n.p2alignl 6, 3212836864\n.fill 256, 4, 3212836864")   # s_nop 0
    parts.append(".amdgpu_metadata\n---\namdhsa.version:\n  - 1\n  - 2\namdhsa.target: amdgcn-amd-amdhsa--gfx950\namdhsa.kernels:\n"
                 + "".join(meta for _, meta in kernels) + "...\n.end_amdgpu_metadata")
    return "\n".join(parts) + "\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "gemm_tn_asm.s"
    with open(out, "w") as f:
        f.write(generate())
