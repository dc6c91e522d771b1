// What the weight-streaming GEMM for 65 to 128 rows (gemm_wide.hip) takes, and
// its launch plan: the one statement of both.  The launchers refuse anything
// whose check is not R_OK before a launch, and Python asks the same function
// through toa_gemm_wide_check (ops/gemm.py wide_takes) instead of restating
// it.  Plain C++17, no HIP.
//
//   plain    y[M][N] = x[M][K] w[N][K]^T
//   SwiGLU   w = gate | up [2F][K];  s[M][F] = silu(x wg^T) * (x wu^T);  N = F
//
// The check returns the FIRST condition that fails.  Sizes are elements of
// bf16 unless a name says bytes.  The kernel forms every address as a 64-bit
// element offset from its base, so no offset has a 2^32 limit; M, N and K are
// ints.
//
// Why these constants (gfx950, 256 CUs, 64 KB of static LDS):
//   TILES    a wave owns TILES = 2 row tiles of W that share every B fragment (plain: adjacent tiles; SwiGLU: the
//            gate and the up tile of the same columns): one ds_read_b128 of x feeds two MFMAs, so LDS serves 8 KB a
//            wave and chunk for 16 MFMAs at MT = 8, the ratio of gemm_stream.hip's SwiGLU form and half the traffic
//            per MFMA of its plain form.  The accumulators are TILES * MT * 4 = 64 VGPRs at MT = 8.  With RG = 4 row
//            groups a workgroup owns WG_ROWS = 128 rows of W, so L2 serves 16 KB of x per 16 KB of W.
//   SPC, KC  one k-step per K group and chunk: KC = KG * SPC * KSTEP = 64 columns.  An LDS buffer is 128 rows of
//            KC + PAD elements, 18 KB, both 36 KB.  KC = 128 would be 68 KB, over the static limit, and was not built.
//   PAD      8 elements: an LDS row is 144 B = 9 * 16 B and 9 is odd, so the 16 rows that the 16 lanes of one k group
//            read start at 16 different multiples of 16 B modulo 256 B, on 16 disjoint sets of four banks.
//   LOADS    8 16-byte loads of W per lane in flight, the count the other streaming GEMMs keep: DEPTH = LOADS /
//            (TILES * SPC) = 4 chunks ahead in both forms, and DEPTH * 2 16-byte registers of x a thread.
//   MIN_WGS, MAX_SPLIT, MIN_CHUNKS   K is split across workgroups while the grid STAYS AT OR UNDER one workgroup a
//            CU and a piece keeps two trips of the load ring.  gemm_stream.hip doubles once more (until the grid is
//            no longer under MIN_WGS); here the kernel's registers leave one workgroup a CU, so a grid of 1.5 per CU
//            runs in two rounds for the time of the split below it, with twice the workspace: a partial is 512 B a
//            row of x and column tile, [split][128][rows of W] fp32 in all, which at split 8 and M = 128 is half of
//            W's own bytes for a square W.  Llama-3-8B: qkv 48 workgroups x 4, attention out 32 x 8, gate|up 224 x 1,
//            down 32 x 8.  The other rule was not measured.
#pragma once

#include <cstdint>

namespace toa_wide {

// ---- the kernel's constants
constexpr int MIN_M = 65;    // fewer rows are gemm_stream.hip's
constexpr int MAX_M = 128;   // rows of x: eight 16-row tiles on the N side of v_mfma_f32_16x16x32_bf16
constexpr int TILE_N = 16;   // rows of W per MFMA tile
constexpr int TILES = 2;     // row tiles per wave, sharing every B fragment
constexpr int KSTEP = 32;    // k per MFMA: one 16-byte load per lane and tile
constexpr int RG = 4;        // row groups per workgroup
constexpr int KG = 2;        // K groups per row group, merged through LDS in group order
constexpr int WAVES = RG * KG;
constexpr int WG_ROWS = RG * TILES * TILE_N;   // rows of W per workgroup: 128 (SwiGLU: 64 gate rows and their 64 up rows)
constexpr int SPC = 1;       // k-steps per K group and chunk
constexpr int KC = KG * SPC * KSTEP;   // columns of x staged in LDS per chunk: 64
constexpr int PAD = 8;       // elements of padding per LDS row of x
constexpr int LOADS = 8;     // 16-byte W loads per lane issued ahead of the chunk that is computing
constexpr int MIN_WGS = 256; // one workgroup per CU of 256: K is split while the grid stays at or under this
constexpr int MIN_CHUNKS = 8;   // chunks a piece keeps at the least: two trips of the load ring
constexpr int MAX_SPLIT = 8;
constexpr int MERGE_BLOCK = 256;   // threads of the merge kernel, one per (row, four columns)

enum Form { F_PLAIN = 0, F_SWIGLU, F_COUNT };

struct Operands {
  uintptr_t X, W, Y, WS;     // WS: the fp32 workspace (toa_gemm_wide_ws_bytes; unused at 0 bytes)
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
    case R_M: return "M (rows) outside 65 .. 128";
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

// ---- the launch plan, a function of the rows of W and K alone (rows = N, SwiGLU: 2F)
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

constexpr bool ld_ok(int64_t ld, int64_t cols) { return ld >= cols && ld % 8 == 0; }
constexpr bool al16(uintptr_t p) { return p != 0 && (p & 15) == 0; }

constexpr Reason check(int form, const Operands& o) {
  if (form != F_PLAIN && form != F_SWIGLU) return R_FORM;
  if (o.M < MIN_M || o.M > MAX_M) return R_M;
  if (o.N <= 0 || o.N % TILE_N) return R_N;
  if (o.K <= 0 || o.K % 8) return R_K;
  if (!ld_ok(o.ldx, o.K) || !ld_ok(o.ldw, o.K) || !ld_ok(o.ldy, o.N)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.Y)) return R_ALIGN;
  if (form == F_SWIGLU ? o.w_rows != 2 * (int64_t)o.N : o.w_rows < o.N) return R_W_ROWS;
  if (ws_bytes(form, o.N, o.K) > 0 && !al16(o.WS)) return R_WORKSPACE;
  return R_OK;
}

}  // namespace toa_wide
