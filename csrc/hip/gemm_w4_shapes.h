// What the weight-streaming GEMM on MXFP4 weights for 1 to 16 rows and its
// quantiser (gemm_w4.hip) take, and the GEMM's launch plan: the one statement
// of both.  The launchers refuse anything whose check is not R_OK before a
// launch, and Python asks the same function through toa_gemm_skinny_w4_check
// (ops/gemm.py skinny_w4_refusal) instead of restating it.  Plain C++17, no HIP.
//
//   format     w[N][K] bf16 -> q[N][K/2] bytes, element 2i in the low nibble of byte i, 2i+1 in the high one, each
//              e2m1 (sign, 2 exponent bits, 1 mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6); scale[N][K/32] bytes, one
//              e8m0 per block of BLOCK = 32 values of k: byte X stands for 2^(X - 127), 0xff for NaN
//   plain      y[M][N] = bf16(sum_k x[m][k] deq[n][k]),  deq = e2m1 * 2^(X - 127), exactly a bf16 value
//   SwiGLU     q = gate | up [2F][K/2], scale[2F][K/32];  s[M][F] = silu(g) * u;  N = F
//
// x and y are bf16, the accumulation is fp32, nothing is multiplied after the
// sum.  The check returns the FIRST condition that fails.  ldx and ldy are
// elements of bf16, ldw is BYTES of q, lds BYTES of scale.  The kernel forms
// every address as a 64-bit offset from its base; M, N and K are ints.
//
// Why these constants (gfx950, 256 CUs):
//   KSTEP    one 16-byte load of q per lane is one block of 32 values of k, and the MFMA's four lane groups make 128.
//   TILES    a lane needs 64 bytes of x per 16 bytes of q.  A workgroup owns TILES = 4 row tiles sharing every x
//            fragment in registers, so x traffic from L2 equals the q stream at M = 16, as in the fp8 kernel.  The
//            SwiGLU form's four tiles are two gate tiles and the up tiles of the same columns.
//   UNROLL   TILES * UNROLL = 8 loads of q and 4 * UNROLL = 8 of x in flight per lane, the 64 VGPRs of loads of the
//            fp8 kernel.  Within a pass lane group g owns the UNROLL consecutive blocks 4 s + UNROLL g + u, so
//            one 4-byte load of scales per tile serves the pass (SCALE_ALIGN).
//   WAVES    8 waves with disjoint K slices, as in the bf16 and fp8 kernels.
//   MIN_WGS  128.  Four tiles leave qkv, attention out and down of Llama-3-8B with 96, 64 and 64 workgroups, which
//            measured slower than the fp8 kernel on all three (down at one row 31.5 us against 23.4), so where four
//            tiles would leave under MIN_WGS workgroups a workgroup owns TILES_FEW = 2 (192, 128, 128).  K is split
//            only below MIN_WGS workgroups at two tiles: the Llama-3-8B projections stay whole, one launch each.  The
//            fp8 kernel's record (gemm_w8_shapes.h) is that the merge launches of a split cost the decode step,
//            which waits on the host's launches, more than the split saves.
#pragma once

#include <cstdint>

namespace toa_w4 {

// ---- the kernel's constants
constexpr int MAX_M = 16;    // rows of x: the N side of one v_mfma_f32_16x16x32_bf16
constexpr int TILE_N = 16;   // rows of q per MFMA tile
constexpr int TILES = 4;     // row tiles per workgroup (plain: adjacent ones; SwiGLU: two gate tiles and their up tiles)
constexpr int TILES_FEW = 2; // the same where four tiles a workgroup would leave under MIN_WGS workgroups
constexpr int BLOCK = 32;    // values of k per scale byte, and per lane and k-step: one 16-byte load of q, four of x
constexpr int KSTEP = 128;   // k per k-step: one block in each of the wave's four lane groups
constexpr int WAVES = 8;     // waves per workgroup, each with its own K slice of the workgroup's tiles
constexpr int UNROLL = 2;    // k-steps per pass
constexpr int MIN_WGS = 128; // fewer workgroups than this: two tiles a workgroup, then K is split across workgroups
constexpr int MAX_SPLIT = 8;
constexpr int MERGE_BLOCK = 256;   // threads of the merge kernel, one per (row, four columns)
constexpr int QUANT_BLOCK = 256;   // threads of the quantiser's workgroup, one row of w each workgroup, one block each
                                   // thread; it keeps nothing in LDS, so K has no limit of its own
constexpr int SCALE_ALIGN = 4;     // bytes: the kernel reads a row's scales four at a time
constexpr int E_MIN = -100, E_MAX = 100;   // the clamp of a block's exponent e; X = e + 127
constexpr int X_NAN = 0xff;

static_assert(4 % UNROLL == 0, "a lane group's UNROLL blocks of a pass lie in one aligned 4-byte word of scales");

enum Form { F_PLAIN = 0, F_SWIGLU, F_COUNT };

struct Operands {
  uintptr_t X, W, Y, WS, SCALE;   // W: q.  WS: the fp32 workspace (toa_gemm_skinny_w4_ws_bytes; unused at 0 bytes)
  int64_t ldx, ldw, ldy, lds;     // ldw, lds in bytes
  int64_t w_rows;                 // rows behind q and behind scale (the launchers pass what the form needs)
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
    case R_K: return "K not a positive multiple of 32";
    case R_LD: return "row stride under the row, or not a multiple of 16 bytes";
    case R_ALIGN: return "base address null or not 16-byte aligned";
    case R_W_ROWS: return "q has fewer than N rows (SwiGLU: not 2F rows)";
    case R_SCALE: return "scale null, not 4-byte aligned, or its row stride under K / 32 or not a multiple of 4 bytes";
    case R_WORKSPACE: return "split-K workspace null or not 16-byte aligned";
    case R_FORM: return "unknown form";
    default: return "unknown reason";
  }
}

// ---- the launch plan, a function of the rows of q and K alone (rows = N, SwiGLU: 2F)
constexpr int rows_of(int form, int N) { return form == F_SWIGLU ? 2 * N : N; }
constexpr int ksteps(int K) { return (K + KSTEP - 1) / KSTEP; }
constexpr int tiles(int rows) { return (rows / TILE_N + TILES - 1) / TILES >= MIN_WGS ? TILES : TILES_FEW; }
constexpr int workgroups(int rows) { return (rows / TILE_N + tiles(rows) - 1) / tiles(rows); }

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
constexpr bool scale_ok(uintptr_t p, int64_t lds, int K) {
  return p != 0 && p % SCALE_ALIGN == 0 && ld_ok(lds, K / BLOCK, SCALE_ALIGN);
}
// the least row stride of scale the kernel takes, for whoever allocates it
constexpr int64_t scale_ld(int K) { return (K / BLOCK + SCALE_ALIGN - 1) / SCALE_ALIGN * SCALE_ALIGN; }

constexpr Reason check(int form, const Operands& o) {
  if (form != F_PLAIN && form != F_SWIGLU) return R_FORM;
  if (o.M < 1 || o.M > MAX_M) return R_M;
  if (o.N <= 0 || o.N % TILE_N) return R_N;
  if (o.K <= 0 || o.K % BLOCK) return R_K;
  if (!ld_ok(o.ldx, o.K, 8) || !ld_ok(o.ldw, o.K / 2, 16) || !ld_ok(o.ldy, o.N, 8)) return R_LD;
  if (!al16(o.X) || !al16(o.W) || !al16(o.Y)) return R_ALIGN;
  if (form == F_SWIGLU ? o.w_rows != 2 * (int64_t)o.N : o.w_rows < o.N) return R_W_ROWS;
  if (!scale_ok(o.SCALE, o.lds, o.K)) return R_SCALE;
  if (ws_bytes(form, o.N, o.K) > 0 && !al16(o.WS)) return R_WORKSPACE;
  return R_OK;
}

// ---- the quantiser: w [N][K] bf16 with row stride ldw elements, q with row stride ldq bytes, scale with lds bytes
// The exponent e of a block's scale 2^e from the magnitude bits (sign cleared) of its largest |w|, a finite bf16:
// the least e with amax <= 6 * 2^e = 1.5 * 2^(e + 2), clamped to E_MIN .. E_MAX; 0 for a block of zeros.  With
// amax = m * 2^E, 1 <= m < 2: e = E - 2 if m <= 1.5 (mantissa field <= 0x40), else E - 1.  A subnormal amax has
// E = -127 here and meets the clamp either way.
constexpr int scale_exponent(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int e = (int)(amax_bits >> 7) - 127 - 2 + ((amax_bits & 0x7f) > 0x40 ? 1 : 0);
  return e < E_MIN ? E_MIN : e > E_MAX ? E_MAX : e;
}

// The e2m1 code of |v| = |w| * 2^-e, round to nearest, ties to the even code: the count of the thresholds passed,
// where the ties 0.25, 1.25, 2.5 and 5 stay below and 0.75, 1.75 and 3.5 go up.  Above 5 -- beyond 6 only where e met
// its clamp or the block holds an infinity -- the code is 7, the format's largest: saturation, made explicit.  A NaN
// passes no threshold (its block's scale says NaN).
constexpr uint32_t e2m1_code(float a) {
  return (uint32_t)(a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
}

constexpr bool quant_ok(uintptr_t w, uintptr_t q, uintptr_t scale, int64_t ldw, int64_t ldq, int64_t lds, int N,
                        int K) {
  return N > 0 && K > 0 && K % BLOCK == 0 && ld_ok(ldw, K, 8) && ld_ok(ldq, K / 2, 16) && al16(w) && al16(q) &&
         scale != 0 && lds >= K / BLOCK;
}

}  // namespace toa_w4
