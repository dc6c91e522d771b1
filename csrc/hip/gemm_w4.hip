// Decode projections on MXFP4 weights (gfx950): a quantiser and a
// weight-streaming GEMM for 1 to 16 rows that reads four bits per weight and
// one scale byte per 32 weights.
//
//   toa_quant_w4               w[N][K] bf16 -> q[N][K/2] e2m1 pairs, scale[N][K/32] e8m0
//   toa_gemm_skinny_w4         y[M][N] = bf16(sum_k x[m][k] deq[n][k]),  deq = e2m1 * 2^(X - 127)
//   toa_gemm_skinny_w4_swiglu  q = gate | up [2F][K/2];  s[M][F] = silu(g) * u
//
// x and y bf16, fp32 accumulation, one rounding to bf16.  The format, what the
// launchers take and the launch plan: gemm_w4_shapes.h (every name in capitals
// below is a constant there).
//
// The GEMM.  The tokens sit on the MFMA's N side, as in gemm_w8.hip.  A k-step
// is KSTEP = 128 columns, one block of 32 in each of the wave's four lane
// groups: lane (r = l & 15, g = l >> 4) loads the 16 bytes of one block b of
// q[n0 + r] and, if r < M, the same 32 columns of x[r] as four 16-byte loads.
// The block's scale byte X goes into the exponent field of an fp32 (X << 23)
// and sixteen v_cvt_scalef32_pk_bf16_fp4 -- one per byte: the low nibble to the
// low half, the block scale applied inside, 0xff giving NaN -- turn the four
// words into 32 bf16 values, already scaled and exact.  Word i feeds one
// v_mfma_f32_16x16x32_bf16 against the i-th x load.  The MFMA sums over its 32
// (lane group, j) slots whatever k they stand for, and A and B assign them the
// same k, so each MFMA adds 32 of the step's 128 products.
//
// Scales.  A pass is UNROLL k-steps from k-step s on, the 4 UNROLL blocks from
// 4 s on, and lane group g owns the UNROLL consecutive ones 4 s + UNROLL g + u
// (u the k-step within the pass) and not every fourth: they lie in one aligned
// 4-byte word of the row's scales, so one 4-byte load per tile and pass serves
// the UNROLL loads of q, and a byte is selected per k-step.  Hence scale rows
// aligned to SCALE_ALIGN.
//
// A workgroup owns T = TILES = 4 row tiles that share every x fragment in
// registers: four adjacent tiles of the plain form, two gate tiles and their
// two up tiles of the SwiGLU form; a short last workgroup leaves tiles out by a
// predicate that is uniform over the workgroup.  Where four tiles would leave
// under MIN_WGS workgroups it owns T = TILES_FEW = 2 (gemm_w4_shapes.h tiles:
// the measurement behind it is there).  Its WAVES waves take disjoint
// K slices -- slice i = piece * WAVES + wave, slice_steps k-steps each: whole
// passes load without a condition, the slice's last partial pass is predicated
// per block, and a block at or beyond K or the slice's end is zeros (x) and
// not a load.  The waves merge through LDS in wave order.  With split > 1 the
// workgroup writes its fp32 partial to the workspace [split][MAX_M][rows of q]
// and a merge kernel adds the pieces in piece order and holds the SwiGLU.  No
// float atomics, no counters, nothing read that this call did not write.  A
// column of D depends on that column of B alone, so a row's bits depend on that
// row of x, on q, on the scales and on (rows of q, K) only.
//
// The quantiser.  One workgroup per row of w, one thread per block of 32: four
// 16-byte loads, the block's largest magnitude as an integer maximum of the
// bf16 bits (the block lives in one lane, so nothing crosses lanes), the
// exponent rule scale_exponent, the elements as e2m1_code of |w| 2^-e (exact in
// fp32), one 16-byte store of q and one byte of scale.  A block with a
// non-finite element gets X = 0xff.
#include "toa_common.h"

#include "gemm_w4_shapes.h"

using namespace toa_w4;

typedef __attribute__((ext_vector_type(8))) short w4_s16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t w4_u32x2;

namespace {

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// eight e2m1 nibbles (one word) times the block scale -> eight bf16 in the order of k, exact
__device__ __forceinline__ w4_s16x8 cvt8(uint32_t w, float scale) {
  const u32x4 v = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3))};
  return __builtin_bit_cast(w4_s16x8, v);
}

// one block of one tile against the lane's four x fragments of the same 32 columns
__device__ __forceinline__ f32x4 mfma4(u32x4 a, float scale, const u32x4* b, f32x4 acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(a[i], scale), __builtin_bit_cast(w4_s16x8, b[i]), acc, 0, 0, 0);
  return acc;
}

template <bool SWIGLU, int T>
__global__ __launch_bounds__(WAVES * 64) void gemm_w4_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                             const uint8_t* __restrict__ q, int64_t ldw,
                                                             const uint8_t* __restrict__ scale, int64_t lds,
                                                             bf16_t* __restrict__ y, int64_t ldy,
                                                             float* __restrict__ ws, int M, int N, int K, int per,
                                                             int nsplit) {
  __shared__ f32x4 red[WAVES][T][64];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int piece = blockIdx.y;
  // the first row of q of tile t, which is also its first row of scale and its first column of a workspace row;
  // SwiGLU: the first T / 2 tiles are gate tiles, the others the up tiles of the same columns
  constexpr int P = T / 2;
  int base[T];
  bool have[T];   // uniform over the workgroup
#pragma unroll
  for (int t = 0; t < T; ++t) {
    base[t] = SWIGLU ? (t / P) * N + (blockIdx.x * P + t % P) * TILE_N : (blockIdx.x * T + t) * TILE_N;
    have[t] = SWIGLU ? (blockIdx.x * P + t % P) * TILE_N < N : base[t] < N;
  }
  const int nsteps = ksteps(K), nblocks = K / BLOCK;
  const int s0 = min((piece * WAVES + wave) * per, nsteps), s1 = min(s0 + per, nsteps);
  const bool live = r < M;   // this lane's row of x exists

  // this lane's first block of a pass from k-step 0 on, and the byte of the scale word its k-step u selects
  const int b_lane = UNROLL * g, sel0 = b_lane % 4;
  const uint8_t* qp[T];
  const uint8_t* sp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t row = (have[t] ? base[t] : base[0]) + r;
    qp[t] = q + row * ldw + (BLOCK / 2) * b_lane;
    sp[t] = scale + row * lds + (b_lane - sel0);
  }
  const bf16_t* xrow = x + (int64_t)(live ? r : 0) * ldx + BLOCK * b_lane;

  const u32x4 zero = {0u, 0u, 0u, 0u};
  const f32x4 fzero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = fzero;

  // whole passes: every k-step below s1 and every lane's blocks below K
  int s = s0;
  for (; s + UNROLL <= s1 && (int64_t)(s + UNROLL) * KSTEP <= K; s += UNROLL) {
    u32x4 a[T][UNROLL], b[UNROLL][4];
    uint32_t sc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      sc[t] = have[t] ? *(const uint32_t*)(sp[t] + 4 * s) : 0u;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a[t][u] = have[t] ? ld16(qp[t] + (int64_t)(4 * s + u) * (BLOCK / 2)) : zero;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) b[u][i] = live ? ld16(xrow + (int64_t)(4 * s + u) * BLOCK + 8 * i) : zero;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = mfma4(a[t][u], __uint_as_float(((sc[t] >> (8 * (sel0 + u))) & 0xffu) << 23), b[u], acc[t]);
  }
  // the slice's last, partial pass: blocks at or beyond the slice's end or K are zeros, not loads
  if (s < s1) {
    const int end = min(4 * s1, nblocks);
    const bool any = 4 * s + b_lane < end;   // the lane's first block of the pass exists, so its scale word does
    u32x4 a[T][UNROLL], b[UNROLL][4];
    uint32_t sc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      sc[t] = have[t] && any ? *(const uint32_t*)(sp[t] + 4 * s) : 0u;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const bool ok = have[t] && 4 * s + b_lane + u < end;
        a[t][u] = ok ? ld16(qp[t] + (int64_t)(4 * s + u) * (BLOCK / 2)) : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool ok = live && 4 * s + b_lane + u < end;
#pragma unroll
      for (int i = 0; i < 4; ++i) b[u][i] = ok ? ld16(xrow + (int64_t)(4 * s + u) * BLOCK + 8 * i) : zero;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      // a block that is not there takes the scale 2^0, so a byte of the padding (0xff: NaN) never meets its zeros
      const bool ok = 4 * s + b_lane + u < end;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const uint32_t X = ok ? (sc[t] >> (8 * (sel0 + u))) & 0xffu : 127u;
        acc[t] = mfma4(a[t][u], __uint_as_float(X << 23), b[u], acc[t]);
      }
    }
  }

  // the waves' slices, in wave order
#pragma unroll
  for (int t = 0; t < T; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave != 0 || !live) return;
  f32x4 sum[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    sum[t] = red[0][t][lane];
#pragma unroll
    for (int v = 1; v < WAVES; ++v) sum[t] += red[v][t][lane];
  }
  // D: this lane holds row r of x, columns 4 g .. 4 g + 3 of each tile
  if (nsplit > 1) {
    float* p = ws + ((int64_t)piece * MAX_M + r) * (SWIGLU ? 2 * N : N) + 4 * g;
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (have[t]) *(f32x4*)(p + base[t]) = sum[t];
    return;
  }
#pragma unroll
  for (int t = 0; t < (SWIGLU ? P : T); ++t) {
    if (!have[t]) continue;
    f32x4 o = sum[t];
    if (SWIGLU) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = silu_mul(sum[t][j], sum[t + P][j]);
    }
    const w4_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
    *(w4_u32x2*)(y + (int64_t)r * ldy + base[t] + 4 * g) = out;
  }
}

// The pieces of a split launch in piece order, then the SwiGLU: one thread per (row, four columns).
template <bool SWIGLU>
__global__ __launch_bounds__(MERGE_BLOCK) void gemm_w4_merge_kernel(const float* __restrict__ ws,
                                                                    bf16_t* __restrict__ y, int64_t ldy, int M, int N,
                                                                    int nsplit) {
  constexpr int T = SWIGLU ? 2 : 1;
  const int quads = N / 4;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * quads) return;
  const int m = (int)(i / quads), n = (int)(i % quads) * 4;
  const int64_t cols = (int64_t)T * N;
  f32x4 sum[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float* p = ws + (int64_t)m * cols + (int64_t)t * N + n;
    sum[t] = *(const f32x4*)p;
    for (int s = 1; s < nsplit; ++s) sum[t] += *(const f32x4*)(p + (int64_t)s * MAX_M * cols);
  }
  f32x4 o = sum[0];
  if (SWIGLU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = silu_mul(sum[0][j], sum[T - 1][j]);
  }
  const w4_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(w4_u32x2*)(y + (int64_t)m * ldy + n) = out;
}

template <bool SWIGLU>
int launch(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const uint8_t* scale, int64_t lds, bf16_t* y,
           int64_t ldy, int M, int N, int K, float* ws, hipStream_t stream) {
  const int form = SWIGLU ? F_SWIGLU : F_PLAIN;
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)q, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws, o.SCALE = (uintptr_t)scale;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.lds = lds, o.M = M, o.N = N, o.K = K;
  o.w_rows = rows_of(form, N);   // the caller's statement: the launcher cannot see behind the pointers
  if (check(form, o) != R_OK) return (int)hipErrorInvalidValue;
  const int rows = rows_of(form, N);
  const int nsplit = split(rows, K), per = slice_steps(rows, K);
  const dim3 grid(workgroups(rows), nsplit), block(WAVES * 64);
  if (tiles(rows) == TILES)
    hipLaunchKernelGGL((gemm_w4_kernel<SWIGLU, TILES>), grid, block, 0, stream, x, ldx, q, ldw, scale, lds, y, ldy, ws,
                       M, N, K, per, nsplit);
  else
    hipLaunchKernelGGL((gemm_w4_kernel<SWIGLU, TILES_FEW>), grid, block, 0, stream, x, ldx, q, ldw, scale, lds, y, ldy,
                       ws, M, N, K, per, nsplit);
  int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit == 1) return rc;
  const int64_t units = (int64_t)M * (N / 4);
  hipLaunchKernelGGL((gemm_w4_merge_kernel<SWIGLU>), dim3((unsigned)((units + MERGE_BLOCK - 1) / MERGE_BLOCK)),
                     dim3(MERGE_BLOCK), 0, stream, (const float*)ws, y, ldy, M, N, nsplit);
  return (int)hipGetLastError();
}

// ---- the quantiser
__global__ __launch_bounds__(QUANT_BLOCK) void quant_w4_kernel(const bf16_t* __restrict__ w, int64_t ldw,
                                                               uint8_t* __restrict__ q, int64_t ldq,
                                                               uint8_t* __restrict__ scale, int64_t lds, int K) {
  const int n = blockIdx.x;
  const bf16_t* wr = w + (int64_t)n * ldw;
  for (int b = threadIdx.x; b < K / BLOCK; b += QUANT_BLOCK) {
    u32x4 in[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) in[i] = ld16(wr + (int64_t)b * BLOCK + 8 * i);
    // For bf16 bits with the sign cleared, integer order is the order of |w|, and anything from 0x7f80 on is an
    // infinity or a NaN.
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) m = max(m, max(in[i][j] & 0x7fffu, (in[i][j] >> 16) & 0x7fffu));
    const bool finite = m < 0x7f80u;
    const int e = finite ? scale_exponent(m) : 0;
    const float down = __uint_as_float((uint32_t)(127 - e) << 23);   // 2^-e: the product below is exact
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float f[8];
      unpack8(in[i], f);
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = f[j] * down;
        word |= (e2m1_code(fabsf(v)) | ((__float_as_uint(v) >> 28) & 8u)) << (4 * j);
      }
      out[i] = word;
    }
    st16(q + (int64_t)n * ldq + (int64_t)b * (BLOCK / 2), out);
    scale[(int64_t)n * lds + b] = (uint8_t)(finite ? e + 127 : X_NAN);
  }
}

}  // namespace

extern "C" int toa_quant_w4(const bf16_t* w, int64_t ldw, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t lds, int N,
                            int K, hipStream_t stream) {
  if (!quant_ok((uintptr_t)w, (uintptr_t)q, (uintptr_t)scale, ldw, ldq, lds, N, K)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_w4_kernel, dim3(N), dim3(QUANT_BLOCK), 0, stream, w, ldw, q, ldq, scale, lds, K);
  return (int)hipGetLastError();
}

extern "C" int toa_gemm_skinny_w4(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const uint8_t* scale,
                                  int64_t lds, bf16_t* y, int64_t ldy, int M, int N, int K, float* ws,
                                  hipStream_t stream) {
  return launch<false>(x, ldx, q, ldw, scale, lds, y, ldy, M, N, K, ws, stream);
}

extern "C" int toa_gemm_skinny_w4_swiglu(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw,
                                         const uint8_t* scale, int64_t lds, bf16_t* s, int64_t ldy, int M, int F,
                                         int K, float* ws, hipStream_t stream) {
  return launch<true>(x, ldx, q, ldw, scale, lds, s, ldy, M, F, K, ws, stream);
}

// form: 0 plain, 1 SwiGLU (N = F).  0 = taken, else the first condition that fails; toa_gemm_skinny_w4_why names it.
extern "C" int toa_gemm_skinny_w4_check(int form, const void* x, const void* q, const void* y, const void* ws,
                                        const void* scale, int64_t ldx, int64_t ldw, int64_t ldy, int64_t lds,
                                        int64_t w_rows, int M, int N, int K) {
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)q, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws, o.SCALE = (uintptr_t)scale;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.lds = lds, o.w_rows = w_rows, o.M = M, o.N = N, o.K = K;
  return (int)check(form, o);
}
extern "C" const char* toa_gemm_skinny_w4_why(int reason) { return why(reason); }
// bytes of fp32 workspace of the plain form (N, K) / the SwiGLU form (F, K); 0: no split, ws is not read
extern "C" int64_t toa_gemm_skinny_w4_ws_bytes(int N, int K) { return ws_bytes(F_PLAIN, N, K); }
extern "C" int64_t toa_gemm_skinny_w4_swiglu_ws_bytes(int F, int K) { return ws_bytes(F_SWIGLU, F, K); }
// the plan, for tests and the benchmark, by the rows of q (N; SwiGLU: 2F): K pieces across workgroups, k-steps per
// wave slice
extern "C" int toa_gemm_skinny_w4_split(int rows, int K) { return rows > 0 && K > 0 ? split(rows, K) : 0; }
extern "C" int toa_gemm_skinny_w4_slice_steps(int rows, int K) { return rows > 0 && K > 0 ? slice_steps(rows, K) : 0; }
// the header's constants, for the tests' shapes and whoever allocates the scales
extern "C" int toa_gemm_skinny_w4_constant(int which) {
  constexpr int v[] = {KSTEP,  BLOCK,       WAVES,       UNROLL, MAX_SPLIT, TILE_N,
                       TILES,  MERGE_BLOCK, SCALE_ALIGN, MAX_M,  TILES_FEW, MIN_WGS};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : 0;
}
