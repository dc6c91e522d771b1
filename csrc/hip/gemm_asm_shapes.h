// What each assembly GEMM form takes: the one statement of it.  The launchers
// (gemm_asm.hip, wgrad.hip) refuse anything whose check is not R_OK before a
// launch, and Python asks the same functions through toa_gemm_shape_check
// (ops/_lib.py shape_check) instead of restating them.  Plain C++17, no HIP:
// csrc/hip/tests/gemm_shapes_selftest.cc compiles it alone.
//
// Every check returns the FIRST condition that fails.  Sizes are elements of
// bf16 unless a name says bytes; a null output pointer counts as aligned (a
// caller may ask before it allocates).
#pragma once

#include <cstdint>

namespace toa_shapes {

// a row stride: at least the row, whole 16-byte chunks, a 256-row tile under 2^32 bytes
constexpr bool ld_ok(int64_t ld, int64_t min_cols) { return ld >= min_cols && ld % 8 == 0 && ld * 2 * 256 < (1ll << 32); }
constexpr bool al16(uintptr_t p) { return (p & 15) == 0; }
inline bool al16(const void* p) { return al16((uintptr_t)p); }

// Operands of one call, by slot.  Per form:
//   TN*            C[M][N] = X[M][K] W[N][K]^T (+ epilogue), strides ldx, ldw, ldc
//   NN*            C[M][N] = X[M][K] W[K][N]
//   *SWIGLU_FWD    N = F, C = gu [M][2F] (ldc), S = s [M][F] (lds)
//   *SWIGLU_BWD    N = F, C = dgu [M][2F] (ldc), S = gu [M][2F] (lds)
//   TN_ROPE        C = q | k | v, S = the cos | sin table; Sq, Hq, Hkv (N follows from the heads)
//   *DELTA         S = O (laid out like C), D = the fp32 -delta rows; Sq, H
//   TN_RESADD      S = the residual (laid out like C)
//   WGRAD_*        C[M][N] (+)= X[K][M]^T W[K][N] (K the tokens; strides ldx >= M, ldw >= N),
//                  S = the fp32 split-K workspace, split (0 = the auto plan)
struct Operands {
  uintptr_t X, W, C, S, D;
  int64_t ldx, ldw, ldc, lds;
  int M, N, K;
  int Sq, H, Hq, Hkv, split;
};

enum Form {
  F_TN = 0,          // whole 256-row tiles (toa_gemm_asm and the diagnostic entries)
  F_TN_ROWS,         // any row count
  F_TN_SWIGLU_FWD,
  F_TN_SWIGLU_BWD,
  F_TN_ROPE,
  F_TN_DELTA,
  F_TN_RESADD,
  F_NN,
  F_NN_SWIGLU_BWD,
  F_NN_DELTA,
  F_WGRAD_ASM,
  F_WGRAD_HIP,
  F_COUNT
};

enum Reason {
  R_OK = 0,
  R_M_RANGE,
  R_M_TILES,
  R_N,
  R_K,
  R_LD,
  R_ALIGN,
  R_F,
  R_SEQ,
  R_HEADS,
  R_DELTA_PTR,
  R_OUT32,
  R_TABLE32,
  R_W_UP32,
  R_WG_OUT,
  R_WG_TOKENS,
  R_SPLIT,
  R_WG_KTILES,
  R_WORKSPACE,
  R_WG_PIECES,
  R_WG_HIP_SPLIT,
  R_WG_HIP_TOKENS,
  R_FORM,
  R_COUNT
};

constexpr const char* why(int reason) {
  switch (reason) {
    case R_OK: return "taken";
    case R_M_RANGE: return "M (rows) outside 1 .. 2^28 - 1";
    case R_M_TILES: return "M not a multiple of 256 (this form takes whole tiles only)";
    case R_N: return "N not a multiple of 256";
    case R_K: return "K not a multiple of 64 >= 128";
    case R_LD: return "row stride under the row, not a multiple of 8 or 2^23 elements and over";
    case R_ALIGN: return "base address not 16-byte aligned";
    case R_F: return "F not a multiple of 128 (SwiGLU forward) / 256 (backward)";
    case R_SEQ: return "S not a multiple of 256 that divides M";
    case R_HEADS: return "head counts outside 1 .. 4096 or heads x 128 != N";
    case R_DELTA_PTR: return "delta rows null or not 4-byte aligned";
    case R_OUT32: return "q | k | v output of 2^32 bytes or more";
    case R_TABLE32: return "cos | sin table of 2^32 bytes or more";
    case R_W_UP32: return "up half of W 2^32 bytes or more from its base";
    case R_WG_OUT: return "weight gradient dims not multiples of 256";
    case R_WG_TOKENS: return "no tokens";
    case R_SPLIT: return "split outside 0 .. 4";
    case R_WG_KTILES: return "64-token k-tiles not divisible by the split or under 2 a piece (T < 65)";
    case R_WORKSPACE: return "split-K workspace null or not 16-byte aligned";
    case R_WG_PIECES: return "split x tail tiles 2^14 or more";
    case R_WG_HIP_SPLIT: return "tokens not a multiple of 128 x split";
    case R_WG_HIP_TOKENS: return "tokens not a multiple of 128 from 1024";
    case R_FORM: return "unknown form";
    default: return "unknown reason";
  }
}

namespace detail {

// X [M][K] and W [N][K]: what every TN form starts with
constexpr Reason tn_common(const Operands& o, bool rows) {
  if (o.M <= 0) return R_M_RANGE;
  if (!rows && o.M % 256) return R_M_TILES;
  if (o.K < 128 || o.K % 64) return R_K;
  if (!ld_ok(o.ldx, o.K) || !ld_ok(o.ldw, o.K)) return R_LD;
  if (!al16(o.X) || !al16(o.W)) return R_ALIGN;
  if (o.M >= (1 << 28)) return R_M_RANGE;
  return R_OK;
}

// X [M][K] and W [K][N] as stored; n_reason: what a bad N is called (F for the SwiGLU form)
constexpr Reason nn_common(const Operands& o, bool rows, Reason n_reason) {
  if (o.M <= 0) return R_M_RANGE;
  if (!rows && o.M % 256) return R_M_TILES;
  if (o.M >= (1 << 28)) return R_M_RANGE;
  if (o.N <= 0 || o.N % 256) return n_reason;
  if (o.K < 128 || o.K % 64) return R_K;
  if (!ld_ok(o.ldx, o.K) || !ld_ok(o.ldw, o.N)) return R_LD;
  if (!al16(o.X) || !al16(o.W)) return R_ALIGN;
  return R_OK;
}

constexpr Reason n256(const Operands& o) { return o.N <= 0 || o.N % 256 ? R_N : R_OK; }

// C [M][cols] (and S where it is laid out next to it)
constexpr Reason out_ok(const Operands& o, int64_t cols, bool with_s) {
  if (!ld_ok(o.ldc, cols)) return R_LD;
  if (!al16(o.C) || (with_s && !al16(o.S))) return R_ALIGN;
  return R_OK;
}

// the delta epilogue's own: -delta rows, heads of 128 columns, whole sequences of whole tiles
constexpr Reason delta_ok(const Operands& o) {
  if (o.D == 0 || (o.D & 3)) return R_DELTA_PTR;
  if (o.H <= 0 || (int64_t)o.H * 128 != o.N) return R_HEADS;
  if (o.Sq <= 0 || o.Sq % 256 || o.M % o.Sq) return R_SEQ;
  return R_OK;
}

// SwiGLU backward: gu (S, lds) and dgu (C, ldc), both [M][2F]
constexpr Reason swiglu_bwd_io(const Operands& o) {
  if (!ld_ok(o.lds, 2 * (int64_t)o.N) || !ld_ok(o.ldc, 2 * (int64_t)o.N)) return R_LD;
  if (!al16(o.S) || !al16(o.C)) return R_ALIGN;
  return R_OK;
}

}  // namespace detail

#define TOA_SHAPES_TRY(expr) \
  if (const Reason r_ = (expr); r_ != R_OK) return r_

constexpr Reason check_tn(const Operands& o, bool rows) {
  TOA_SHAPES_TRY(detail::tn_common(o, rows));
  TOA_SHAPES_TRY(detail::n256(o));
  return detail::out_ok(o, o.N, false);
}

constexpr Reason check_tn_resadd(const Operands& o) {
  TOA_SHAPES_TRY(detail::tn_common(o, true));
  TOA_SHAPES_TRY(detail::n256(o));
  return detail::out_ok(o, o.N, true);
}

constexpr Reason check_tn_swiglu_fwd(const Operands& o) {
  TOA_SHAPES_TRY(detail::tn_common(o, true));
  if (o.N <= 0 || o.N % 128) return R_F;
  if (!ld_ok(o.ldc, 2 * (int64_t)o.N) || !ld_ok(o.lds, o.N)) return R_LD;
  if (!al16(o.C) || !al16(o.S)) return R_ALIGN;
  // the up half's row offset in W and the last tile's rows behind it, in bytes
  if ((int64_t)o.N * o.ldw * 2 + 128 * o.ldw * 2 >= (1ll << 32)) return R_W_UP32;
  return R_OK;
}

constexpr Reason check_tn_swiglu_bwd(const Operands& o) {
  TOA_SHAPES_TRY(detail::tn_common(o, true));
  if (o.N <= 0 || o.N % 256) return R_F;
  return detail::swiglu_bwd_io(o);
}

// the cos | sin table [2][S][64] fp32 and one tile's rows behind it, in bytes
constexpr bool rope_table_fits(int64_t S) { return S * 512 + 128 * 256 < (1ll << 32); }

constexpr Reason check_tn_rope(const Operands& o) {
  const int64_t N = ((int64_t)o.Hq + 2 * (int64_t)o.Hkv) * 128;
  TOA_SHAPES_TRY(detail::tn_common(o, false));
  if (o.Hq <= 0 || o.Hkv <= 0 || o.Hq > 4096 || o.Hkv > 4096) return R_HEADS;
  if (N % 256) return R_N;
  if (o.Sq <= 0 || o.Sq % 256 || o.M % o.Sq) return R_SEQ;
  if (!al16(o.C) || !al16(o.S)) return R_ALIGN;
  if ((int64_t)o.M * N * 2 >= (1ll << 32)) return R_OUT32;
  if (!rope_table_fits(o.Sq)) return R_TABLE32;   // (S <= M: the limit above is met first)
  return R_OK;
}

constexpr Reason check_tn_delta(const Operands& o) {
  TOA_SHAPES_TRY(detail::tn_common(o, false));
  TOA_SHAPES_TRY(detail::n256(o));
  TOA_SHAPES_TRY(detail::out_ok(o, o.N, true));
  return detail::delta_ok(o);
}

constexpr Reason check_nn(const Operands& o) {
  TOA_SHAPES_TRY(detail::nn_common(o, true, R_N));
  return detail::out_ok(o, o.N, false);
}

constexpr Reason check_nn_swiglu_bwd(const Operands& o) {
  TOA_SHAPES_TRY(detail::nn_common(o, true, R_F));
  return detail::swiglu_bwd_io(o);
}

constexpr Reason check_nn_delta(const Operands& o) {
  TOA_SHAPES_TRY(detail::nn_common(o, false, R_N));
  TOA_SHAPES_TRY(detail::out_ok(o, o.N, true));
  return detail::delta_ok(o);
}

// ---- weight gradients: C[M][N] (+)= X[K][M]^T W[K][N], K the token count.
// The launch plan: `full` whole-K tiles (whole waves of the 256 CUs) and the
// tail tiles cut into `split` k-pieces so the last wave is as full as
// possible.  Auto (split argument 0): the largest split in 2..4 that fits the
// tail into one wave and leaves 512 rows a piece -- pieces of whole 128-row
// steps for the HIP kernel; for the assembly kernel at K % 64 != 0 (its own:
// ceil(K / 64) k-tiles, the last one cut by the operands' buffer resources) a
// split that DIVIDES the k-tiles.  Nothing to split: the tail runs whole.  An
// explicit split cuts every tile (1 = none).  csrc/asm/host_args.py
// wgrad_plan mirrors it for the emulator tests.
struct WgradPlan {
  int split, full;
};

constexpr WgradPlan wgrad_plan(int M, int N, int K, int split, bool asm_kernel) {
  const int tiles = (M / 256) * (N / 256), rem = tiles % 256;
  if (split != 0) return {split, split == 1 ? tiles : 0};
  int best = 1;
  for (int s = 2; rem && s <= 4; ++s) {
    const bool whole = asm_kernel && K % 64 ? ((K + 63) / 64) % s == 0 : K % (128 * s) == 0;
    if (rem * s <= 256 && whole && K / s >= 512) best = s;
  }
  return {best, best > 1 ? tiles - rem : tiles};
}

// bytes of fp32 workspace the plan's k-pieces need
constexpr int64_t wgrad_workspace(int M, int N, int K, int split, bool asm_kernel) {
  const WgradPlan p = wgrad_plan(M, N, K, split, asm_kernel);
  return p.split > 1 ? (int64_t)p.split * ((M / 256) * (N / 256) - p.full) * 256 * 256 * 4 : 0;
}

constexpr Reason wgrad_dims(const Operands& o) {
  if (o.M <= 0 || o.N <= 0) return R_WG_OUT;
  if (o.K <= 0) return R_WG_TOKENS;
  if (o.M % 256 || o.N % 256) return R_WG_OUT;
  return R_OK;
}

constexpr Reason check_wgrad_asm(const Operands& o, WgradPlan* plan = nullptr) {
  TOA_SHAPES_TRY(wgrad_dims(o));
  if (o.split < 0 || o.split > 4) return R_SPLIT;
  if (!ld_ok(o.ldx, o.M) || !ld_ok(o.ldw, o.N) || !ld_ok(o.ldc, o.N)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.C)) return R_ALIGN;
  const WgradPlan p = wgrad_plan(o.M, o.N, o.K, o.split, true);
  const int kt = (o.K + 63) / 64;   // k-tiles; K % 64 rows of the last one are live when K % 64 != 0
  if (kt % p.split || kt / p.split < 2) return R_WG_KTILES;
  if (p.split > 1 && (o.S == 0 || !al16(o.S))) return R_WORKSPACE;
  if ((int64_t)p.split * ((o.M / 256) * (o.N / 256) - p.full) >= (1 << 14)) return R_WG_PIECES;
  if (plan) *plan = p;
  return R_OK;
}

// csrc/hip/wgrad.hip: its k-loop runs 4 stages of 32 rows, it stages both
// operands in 16-byte chunks and stores C in 8-byte ones, and it is used (and
// was measured) from 1024 tokens
constexpr Reason check_wgrad_hip(const Operands& o, WgradPlan* plan = nullptr) {
  TOA_SHAPES_TRY(wgrad_dims(o));
  if (o.split < 0) return R_SPLIT;
  if ((o.ldx | o.ldw | o.ldc) % 8) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.C)) return R_ALIGN;
  const WgradPlan p = wgrad_plan(o.M, o.N, o.K, o.split, false);
  if (o.K % (128 * p.split)) return R_WG_HIP_SPLIT;
  if (p.split > 1 && o.S == 0) return R_WORKSPACE;
  if (o.K % 128 || o.K < 1024) return R_WG_HIP_TOKENS;
  if (plan) *plan = p;
  return R_OK;
}

#undef TOA_SHAPES_TRY

constexpr Reason check(int form, const Operands& o) {
  switch (form) {
    case F_TN: return check_tn(o, false);
    case F_TN_ROWS: return check_tn(o, true);
    case F_TN_SWIGLU_FWD: return check_tn_swiglu_fwd(o);
    case F_TN_SWIGLU_BWD: return check_tn_swiglu_bwd(o);
    case F_TN_ROPE: return check_tn_rope(o);
    case F_TN_DELTA: return check_tn_delta(o);
    case F_TN_RESADD: return check_tn_resadd(o);
    case F_NN: return check_nn(o);
    case F_NN_SWIGLU_BWD: return check_nn_swiglu_bwd(o);
    case F_NN_DELTA: return check_nn_delta(o);
    case F_WGRAD_ASM: return check_wgrad_asm(o);
    case F_WGRAD_HIP: return check_wgrad_hip(o);
    default: return R_FORM;
  }
}

}  // namespace toa_shapes
