// What the weight-streaming GEMM for 1 to 16 rows (gemm_skinny.hip) takes, and
// its launch plan: the one statement of both.  The launchers refuse anything
// whose check is not R_OK before a launch, and Python asks the same function
// through toa_gemm_skinny_check (ops/gemm.py skinny_takes) instead of restating
// it.  Plain C++17, no HIP: csrc/hip/tests/gemm_skinny_selftest.cc compiles it
// alone.
//
//   plain    y[M][N] = x[M][K] w[N][K]^T
//   SwiGLU   w = gate | up [2F][K];  s[M][F] = silu(x wg^T) * (x wu^T);  N = F
//
// The check returns the FIRST condition that fails.  Sizes are elements of
// bf16 unless a name says bytes.  The kernel forms every address as a 64-bit
// element offset from its base, so no offset has a 2^32 limit; M, N and K are
// ints.
#pragma once

#include <cstdint>

namespace toa_skinny {

// ---- the kernel's constants
constexpr int MAX_M = 16;    // rows of x: the N side of one v_mfma_f32_16x16x32_bf16
constexpr int TILE_N = 16;   // rows of W per MFMA tile; a workgroup owns one tile (SwiGLU: a gate and an up tile)
constexpr int KSTEP = 32;    // k per MFMA: one 16-byte load per lane and tile
constexpr int WAVES = 8;     // waves per workgroup, each with its own K slice of the workgroup's tile
constexpr int UNROLL = 8;    // 16-byte W loads a lane keeps in flight: k-steps per pass (SwiGLU: UNROLL / 2, two tiles)
constexpr int MIN_WGS = 256; // fewer row tiles than this (under WAVES waves per CU of 256): K is split across workgroups
constexpr int MAX_SPLIT = 8;

enum Form { F_PLAIN = 0, F_SWIGLU, F_COUNT };

struct Operands {
  uintptr_t X, W, Y, WS;     // WS: the fp32 workspace (toa_gemm_skinny_ws_bytes; unused at 0 bytes)
  int64_t ldx, ldw, ldy;
  int64_t w_rows;            // rows behind W (the launchers cannot see them and pass what the form needs)
  int M, N, K;               // N = F for the SwiGLU form
};

enum Reason {
  R_OK = 0,
  R_M,
  R_N,
  R_K,
  R_LD,
  R_ALIGN,
  R_W_ROWS,
  R_WORKSPACE,
  R_FORM,
  R_COUNT
};

constexpr const char* why(int reason) {
  switch (reason) {
    case R_OK: return "taken";
    case R_M: return "M (rows) outside 1 .. 16";
    case R_N: return "N (F) not a positive multiple of 16";
    case R_K: return "K not a positive multiple of 8";
    case R_LD: return "row stride under the row or not a multiple of 8";
    case R_ALIGN: return "base address null or not 16-byte aligned";
    case R_W_ROWS: return "W has fewer than N rows (SwiGLU: not 2F rows)";
    case R_WORKSPACE: return "split-K workspace null or not 16-byte aligned";
    case R_FORM: return "unknown form";
    default: return "unknown reason";
  }
}

// ---- the launch plan, a function of (N, K) alone
constexpr int ksteps(int K) { return (K + KSTEP - 1) / KSTEP; }

// K pieces across workgroups: doubled while the grid has under MIN_WGS workgroups and every wave would keep a
// full pass of UNROLL k-steps
constexpr int split(int N, int K) {
  const int64_t tiles = N / TILE_N;
  int s = 1;
  while (s < MAX_SPLIT && tiles * s < MIN_WGS && ksteps(K) / (2 * s * WAVES) >= UNROLL) s *= 2;
  return s;
}

// k-steps per slice; slice i = piece * WAVES + wave takes steps [i * per, min((i + 1) * per, ksteps))
constexpr int slice_steps(int N, int K) {
  const int slices = split(N, K) * WAVES;
  return (ksteps(K) + slices - 1) / slices;
}

// bytes of fp32 workspace: [split][MAX_M][N] partials (SwiGLU: [split][MAX_M][2F]); 0 without a split
constexpr int64_t ws_bytes(int form, int N, int K) {
  if (N <= 0 || K <= 0 || N % TILE_N) return 0;
  const int s = split(N, K);
  return s > 1 ? (int64_t)s * MAX_M * N * 4 * (form == F_SWIGLU ? 2 : 1) : 0;
}

constexpr bool ld_ok(int64_t ld, int64_t cols) { return ld >= cols && ld % 8 == 0; }
constexpr bool al16(uintptr_t p) { return p != 0 && (p & 15) == 0; }

constexpr Reason check(int form, const Operands& o) {
  if (form != F_PLAIN && form != F_SWIGLU) return R_FORM;
  if (o.M < 1 || o.M > MAX_M) return R_M;
  if (o.N <= 0 || o.N % TILE_N) return R_N;
  if (o.K <= 0 || o.K % 8) return R_K;
  if (!ld_ok(o.ldx, o.K) || !ld_ok(o.ldw, o.K) || !ld_ok(o.ldy, o.N)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.Y)) return R_ALIGN;
  if (form == F_SWIGLU ? o.w_rows != 2 * (int64_t)o.N : o.w_rows < o.N) return R_W_ROWS;
  if (ws_bytes(form, o.N, o.K) > 0 && !al16(o.WS)) return R_WORKSPACE;
  return R_OK;
}

}  // namespace toa_skinny
