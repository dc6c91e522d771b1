// What the weight-streaming GEMM on fp8 weights for 1 to 16 rows and its
// quantiser (gemm_w8.hip) take, and the GEMM's launch plan: the one statement
// of both.  The launchers refuse anything whose check is not R_OK before a
// launch, and Python asks the same function through toa_gemm_skinny_w8_check
// (ops/gemm.py skinny_w8_refusal) instead of restating it.  Plain C++17, no HIP.
//
//   quantiser  w[N][K] bf16 -> q[N][K] e4m3 (OCP "fn": largest finite 448, 0x7f / 0xff NaN), scale[N] fp32 = 2^e
//   plain      y[M][N] = bf16(scale[n] * sum_k x[m][k] q[n][k])
//   SwiGLU     q = gate | up [2F][K], scale[2F];  s[M][F] = silu(scale g) * (scale u);  N = F
//
// x and y are bf16, q is one byte per element, the accumulation is fp32.  The
// check returns the FIRST condition that fails.  ldx and ldy are elements of
// bf16, ldw is BYTES of q (they are its elements).  The kernel forms every
// address as a 64-bit offset from its base; M, N and K are ints.
//
// Why these constants (gfx950, 256 CUs):
//   KSTEP    one 16-byte load of q per lane is 16 values of k, and the MFMA's four lane groups make 64.
//   TILES    a workgroup owns TILES = 2 row tiles sharing every x fragment, so the 32 bytes of x a lane needs per
//            16 bytes of q are loaded once per 32 bytes of q: x traffic from L2 equals the q stream at M = 16
//            instead of twice it.  The SwiGLU form's two tiles are the gate and the up tile of the same columns.
//   UNROLL   TILES * UNROLL = 8 loads of q in flight per lane, the count the bf16 kernel keeps; with the 2 * UNROLL
//            loads of x that is 64 VGPRs of loads, which leaves 8 waves a workgroup without spilling.
//   WAVES    8 waves with disjoint K slices, as in the bf16 kernel: two per SIMD to cover the conversions of one
//            with the loads of the other.
//   MIN_WGS  128: the Llama-3-8B projections (192, 128, 896 and 128 workgroups) stay whole, one launch each.  At 256
//            qkv, attention out and down split in two: down measured 18 to 20 us against 23 to 29 us whole, qkv 11 to
//            14 us against 10 to 12 us, and the decode step, which waits on the host's launches, was slower with the
//            three merge launches per layer than on bf16 (docs/kernels.md "Decoding on fp8 weights").
#pragma once

#include <cstdint>

#include "e4m3_quant.h"

namespace toa_w8 {

// ---- the kernel's constants
constexpr int MAX_M = 16;    // rows of x: the N side of one v_mfma_f32_16x16x32_bf16
constexpr int TILE_N = 16;   // rows of q per MFMA tile
constexpr int TILES = 2;     // row tiles per workgroup (plain: adjacent ones, the last workgroup one if N / 16 is odd)
constexpr int CHUNK = 16;    // columns per lane and k-step: one 16-byte load of q, two of x, two MFMAs
constexpr int KSTEP = 64;    // k per k-step: CHUNK columns in each of the wave's four lane groups
constexpr int WAVES = 8;     // waves per workgroup, each with its own K slice of the workgroup's tiles
constexpr int UNROLL = 4;    // k-steps per pass
constexpr int MIN_WGS = 128; // fewer workgroups than this: K is split across workgroups
constexpr int MAX_SPLIT = 8;
constexpr int MERGE_BLOCK = 256;    // threads of the merge kernel, one per (row, four columns)
constexpr int QUANT_BLOCK = 256;    // threads of the quantiser's workgroup, one row of w each workgroup
constexpr int QUANT_LDS_K = 16384;  // the quantiser keeps a row of up to this many columns (32 KB) in LDS between
                                    // its two passes; a longer one is read again (from L2: 1 MB at most is in between)

enum Form { F_PLAIN = 0, F_SWIGLU, F_COUNT };

struct Operands {
  uintptr_t X, W, Y, WS, SCALE;   // W: q.  WS: the fp32 workspace (toa_gemm_skinny_w8_ws_bytes; unused at 0 bytes)
  int64_t ldx, ldw, ldy;          // ldw in bytes
  int64_t w_rows;                 // rows behind q and entries behind scale (the launchers pass what the form needs)
  int M, N, K;                    // N = F for the SwiGLU form
};

enum Reason {
  R_OK = 0,
  R_M,
  R_N,
  R_K,
  R_LD,
  R_ALIGN,
  R_W_ROWS,
  R_SCALE,
  R_WORKSPACE,
  R_FORM,
  R_COUNT
};

constexpr const char* why(int reason) {
  switch (reason) {
    case R_OK: return "taken";
    case R_M: return "M (rows) outside 1 .. 16";
    case R_N: return "N (F) not a positive multiple of 16";
    case R_K: return "K not a positive multiple of 16";
    case R_LD: return "row stride under the row, or not a multiple of 16 bytes";
    case R_ALIGN: return "base address null or not 16-byte aligned";
    case R_W_ROWS: return "q has fewer than N rows (SwiGLU: not 2F rows)";
    case R_SCALE: return "scale null or not 4-byte aligned";
    case R_WORKSPACE: return "split-K workspace null or not 16-byte aligned";
    case R_FORM: return "unknown form";
    default: return "unknown reason";
  }
}

// ---- the launch plan, a function of the rows of q and K alone (rows = N, SwiGLU: 2F)
constexpr int rows_of(int form, int N) { return form == F_SWIGLU ? 2 * N : N; }
constexpr int ksteps(int K) { return (K + KSTEP - 1) / KSTEP; }
constexpr int workgroups(int rows) { return (rows / TILE_N + TILES - 1) / TILES; }

// K pieces across workgroups: doubled while the grid has under MIN_WGS workgroups and every wave would keep a
// full pass of UNROLL k-steps
constexpr int split(int rows, int K) {
  const int64_t wgs = workgroups(rows);
  int s = 1;
  while (s < MAX_SPLIT && wgs * s < MIN_WGS && ksteps(K) / (2 * s * WAVES) >= UNROLL) s *= 2;
  return s;
}

// k-steps per slice; slice i = piece * WAVES + wave takes steps [i * per, min((i + 1) * per, ksteps))
constexpr int slice_steps(int rows, int K) {
  const int slices = split(rows, K) * WAVES;
  return (ksteps(K) + slices - 1) / slices;
}

// bytes of fp32 workspace: [split][MAX_M][rows] partials; 0 without a split
constexpr int64_t ws_bytes(int form, int N, int K) {
  if (N <= 0 || K <= 0 || N % TILE_N) return 0;
  const int s = split(rows_of(form, N), K);
  return s > 1 ? (int64_t)s * MAX_M * rows_of(form, N) * 4 : 0;
}

constexpr bool ld_ok(int64_t ld, int64_t cols, int64_t unit) { return ld >= cols && ld % unit == 0; }
constexpr bool al16(uintptr_t p) { return p != 0 && (p & 15) == 0; }

constexpr Reason check(int form, const Operands& o) {
  if (form != F_PLAIN && form != F_SWIGLU) return R_FORM;
  if (o.M < 1 || o.M > MAX_M) return R_M;
  if (o.N <= 0 || o.N % TILE_N) return R_N;
  if (o.K <= 0 || o.K % CHUNK) return R_K;
  if (!ld_ok(o.ldx, o.K, 8) || !ld_ok(o.ldw, o.K, 16) || !ld_ok(o.ldy, o.N, 8)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.Y)) return R_ALIGN;
  if (form == F_SWIGLU ? o.w_rows != 2 * (int64_t)o.N : o.w_rows < o.N) return R_W_ROWS;
  if (o.SCALE == 0 || (o.SCALE & 3)) return R_SCALE;
  if (ws_bytes(form, o.N, o.K) > 0 && !al16(o.WS)) return R_WORKSPACE;
  return R_OK;
}

// ---- the quantiser: w [N][K] bf16 with row stride ldw elements, q with row stride ldq bytes
// The exponent e of scale = 2^e of a row: e4m3_quant.h, the rule the fp8 KV cache shares.
using toa_e4m3::E_MAX;
using toa_e4m3::E_MIN;
using toa_e4m3::scale_exponent;

constexpr bool quant_ok(uintptr_t w, uintptr_t q, uintptr_t scale, int64_t ldw, int64_t ldq, int N, int K) {
  return N > 0 && K > 0 && K % CHUNK == 0 && ld_ok(ldw, K, 8) && ld_ok(ldq, K, 16) && al16(w) && al16(q) &&
         scale != 0 && (scale & 3) == 0;
}

}  // namespace toa_w8
