// What the weight-streaming GEMM on fp8 weights for 65 to 128 rows
// (gemm_wide_w8.hip) takes, and its launch plan: the one statement of both.
// The launchers refuse anything whose check is not R_OK before a launch, and
// Python asks the same function through toa_gemm_wide_w8_check (ops/gemm.py
// wide_w8_refusal) instead of restating it.  Plain C++17, no HIP.
//
//   plain    y[M][N] = bf16(scale[n] * sum_k x[m][k] q[n][k])
//   SwiGLU   q = gate | up [2F][K], scale[2F];  s[M][F] = silu(scale g) * (scale u);  N = F
//
// x and y are bf16, q is OCP e4m3, one byte per element, with one fp32 scale
// per row (toa_quant_w8's tensors), the accumulation is fp32.  The check
// returns the FIRST condition that fails.  ldx and ldy are elements of bf16,
// ldw is BYTES of q (they are its elements).  The kernel forms every address
// as a 64-bit offset from its base; M, N and K are ints.
//
// Why these constants (gfx950, 256 CUs, 160 KB of LDS a CU):
//   KSTEP    one 16-byte load of q per lane is 16 values of k, and the MFMA's four lane groups make 64: two
//            v_mfma_f32_16x16x32_bf16 per tile of x and row tile of q (gemm_stream_w8.hip's k-step).
//   TILES    a wave owns TILES = 2 row tiles of q that share every B fragment (plain: adjacent tiles; SwiGLU: the
//            gate and the up tile of the same columns): one conversion of a q fragment (8 v_cvt_pk_f32_fp8 and 8
//            v_cvt_pk_bf16_f32 for 16 bytes) feeds 2 MT = 10 .. 16 MFMAs, a quarter to a half of the conversions per
//            MFMA of the 17-to-64-row kernel, and a pair of ds_read_b128 of x feeds four MFMAs.  The accumulators
//            are TILES * MT * 4 = 64 VGPRs at MT = 8.
//   RG, KG, KC   RG = 4 row groups x KG = 2 K groups, gemm_wide.hip's workgroup and so its grid plan: WG_ROWS = 128
//            rows of q a workgroup, KC = KG * SPC * KSTEP = 128 columns a chunk, 16 KB of q against 32 KB of x from
//            L2 per workgroup and chunk at M = 128.  Both x buffers are 2 * 128 rows * 272 B = 69 632 B of static
//            LDS.  That is over the 64 KB the bf16 kernel's header stops at, and under the CU's 160 KB: the kernel's
//            registers leave one workgroup a CU in any case, so nothing else wants the rest.  The K groups' merge of
//            both tiles at once is 64 KB at MT = 8 and fits in the buffers: one write, one barrier, one read, not
//            gemm_wide.hip's tile-at-a-time merge with its second barrier pair.
//            The other geometry, RG = 8, KG = 1, KC = 64, WG_ROWS = 256 in 36 KB (no K-group merge, 16 KB of x per
//            16 KB of q, half the workgroups on the small forms), was not built and not measured.
//   PAD      8 elements, 16 bytes: an LDS row is 272 B = 17 * 16 B and 17 is odd, so the 16 rows that the 16 lanes of
//            one k group read start at 16 different multiples of 16 B modulo 256 B, in either half of the fragment.
//   LOADS    8 16-byte loads of q per lane in flight, the count the other streaming GEMMs keep: DEPTH = LOADS /
//            (TILES * SPC) = 4 chunks ahead in both forms.  The x ring is DEPTH * 4 16-byte registers a thread at
//            MT = 7 and 8 (a chunk of x is 32 KB over 512 threads), 64 VGPRs, beside 32 of q.
//   MIN_WGS, MAX_SPLIT, MIN_CHUNKS   gemm_wide.hip's rule: K is split across workgroups while the grid STAYS AT OR
//            UNDER one workgroup a CU and a piece keeps two trips of the load ring.  A chunk is twice the bf16
//            kernel's columns, so the same MIN_CHUNKS gives half its split: Llama-3-8B qkv 48 workgroups x 4,
//            attention out 32 x 4, gate|up 224 x 1, down 32 x 8.  MIN_CHUNKS = 4 (attention out 32 x 8, pieces of
//            the ring's depth, all prologue) was not measured here; at 17 to 64 rows it lost.
#pragma once

#include <cstdint>

namespace toa_wide_w8 {

// ---- the kernel's constants
constexpr int MIN_M = 65;    // fewer rows are gemm_stream_w8.hip's
constexpr int MAX_M = 128;   // rows of x: eight 16-row tiles on the N side of v_mfma_f32_16x16x32_bf16
constexpr int TILE_N = 16;   // rows of q per MFMA tile
constexpr int TILES = 2;     // row tiles per wave, sharing every B fragment
constexpr int CHUNK = 16;    // columns per lane and k-step: one 16-byte load of q, 32 bytes of x, two MFMAs per tile
constexpr int KSTEP = 64;    // k per k-step: CHUNK columns in each of the wave's four lane groups
constexpr int RG = 4;        // row groups per workgroup
constexpr int KG = 2;        // K groups per row group, merged through LDS in group order
constexpr int WAVES = RG * KG;
constexpr int WG_ROWS = RG * TILES * TILE_N;   // rows of q per workgroup: 128 (SwiGLU: 64 gate rows and their 64 up rows)
constexpr int SPC = 1;       // k-steps per K group and chunk
constexpr int KC = KG * SPC * KSTEP;   // columns of x staged in LDS per chunk: 128
constexpr int PAD = 8;       // elements of padding per LDS row of x
constexpr int LOADS = 8;     // 16-byte q loads per lane issued ahead of the chunk that is computing
constexpr int MIN_WGS = 256; // one workgroup per CU of 256: K is split while the grid stays at or under this
constexpr int MIN_CHUNKS = 8;   // chunks a piece keeps at the least: two trips of the load ring
constexpr int MAX_SPLIT = 8;
constexpr int MERGE_BLOCK = 256;   // threads of the merge kernel, one per (row, four columns)
constexpr int LDS_LIMIT = 160 * 1024;   // bytes of LDS a workgroup may hold on gfx950

enum Form { F_PLAIN = 0, F_SWIGLU, F_COUNT };

struct Operands {
  uintptr_t X, W, Y, WS, SCALE;   // W: q.  WS: the fp32 workspace (toa_gemm_wide_w8_ws_bytes; unused at 0 bytes)
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
    case R_M: return "M (rows) outside 65 .. 128";
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
constexpr int chunks(int K) { return (K + KC - 1) / KC; }
constexpr int workgroups(int rows) { return (rows + WG_ROWS - 1) / WG_ROWS; }

// K pieces across workgroups: doubled while the doubled grid has at most MIN_WGS workgroups and every piece would
// keep MIN_CHUNKS chunks
constexpr int split(int rows, int K) {
  const int64_t wgs = workgroups(rows);
  int s = 1;
  while (s < MAX_SPLIT && wgs * 2 * s <= MIN_WGS && chunks(K) / (2 * s) >= MIN_CHUNKS) s *= 2;
  return s;
}

// chunks per piece; piece p takes chunks [p * per, min((p + 1) * per, chunks))
constexpr int piece_chunks(int rows, int K) {
  const int s = split(rows, K);
  return (chunks(K) + s - 1) / s;
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
  if (o.M < MIN_M || o.M > MAX_M) return R_M;
  if (o.N <= 0 || o.N % TILE_N) return R_N;
  if (o.K <= 0 || o.K % CHUNK) return R_K;
  if (!ld_ok(o.ldx, o.K, 8) || !ld_ok(o.ldw, o.K, 16) || !ld_ok(o.ldy, o.N, 8)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.Y)) return R_ALIGN;
  if (form == F_SWIGLU ? o.w_rows != 2 * (int64_t)o.N : o.w_rows < o.N) return R_W_ROWS;
  if (o.SCALE == 0 || (o.SCALE & 3)) return R_SCALE;
  if (ws_bytes(form, o.N, o.K) > 0 && !al16(o.WS)) return R_WORKSPACE;
  return R_OK;
}

}  // namespace toa_wide_w8
