// Decode projections on fp8 weights (gfx950): a quantiser and a weight-streaming
// GEMM for 1 to 16 rows that reads one byte per weight.
//
//   toa_quant_w8               w[N][K] bf16 -> q[N][K] OCP e4m3, scale[N] fp32 = 2^e
//   toa_gemm_skinny_w8         y[M][N] = bf16(scale[n] * sum_k x[m][k] q[n][k])
//   toa_gemm_skinny_w8_swiglu  q = gate | up [2F][K];  s[M][F] = silu(scale g) * (scale u)
//
// x and y bf16, fp32 accumulation, one fp32 multiply by the scale, one
// rounding to bf16.  What the launchers take and the launch plan:
// gemm_w8_shapes.h (every name in capitals below is a constant there).
//
// The GEMM.  The tokens sit on the MFMA's N side, as in gemm_skinny.hip, but a
// k-step is KSTEP = 64 columns: lane (r = l & 15, g = l >> 4) loads the 16
// bytes q[n0 + r][k0 + 16 g .. + 16) and, if r < M, the same 16 columns of
// x[r] as two 16-byte loads.  Bytes 0 .. 7 become eight bf16 values in
// registers (v_cvt_pk_f32_fp8 on both halves of a word, v_cvt_pk_bf16_f32:
// exact, every e4m3 value is a bf16 value; 16 VALU instructions per load) and
// go through one v_mfma_f32_16x16x32_bf16 against the first x load, bytes
// 8 .. 15 through a second against the second.  The MFMA sums over its 32
// (lane group, j) slots whatever k they stand for, and A and B assign them
// the same k, so each MFMA adds 32 of the step's 64 products.
//
// A workgroup owns TILES = 2 row tiles that share every x fragment: two
// adjacent tiles of the plain form (the last workgroup owns one if N / 16 is
// odd; the predicate is uniform over the workgroup), the gate and the up tile
// of the SwiGLU form.  Its WAVES waves take disjoint K slices -- slice
// i = piece * WAVES + wave, slice_steps k-steps each -- with UNROLL k-steps
// per pass: whole passes load without a condition, the slice's last partial
// pass is predicated per k-step, and a lane's 16-column chunk at or beyond K
// is zeros, not a load.  The waves merge through LDS in wave order.  With
// split > 1 the workgroup writes its fp32 partial to the workspace
// [split][MAX_M][rows of q] and a merge kernel adds the pieces in piece order;
// the scale and the SwiGLU come after the last add.  No float atomics, no
// counters, nothing read that this call did not write.  A column of D depends
// on that column of B alone, so a row's bits depend on that row of x, on q,
// on scale and on (rows of q, K) only.
//
// x is not staged in LDS: the waves of a workgroup split K, so no two of them
// read the same x, and the two tiles of one wave share it in registers
// already.  LDS staging would pay only if the waves split the rows of q
// instead and a workgroup owned 8 or more row tiles; that is gemm_stream.hip's
// design and its fp8 twin is not built here.
//
// The quantiser.  One workgroup per row: 16-byte loads, the largest magnitude
// as an integer maximum of the bf16 bits (wave shuffles, then LDS across the
// waves), the row kept in LDS for the second pass when K <= QUANT_LDS_K and
// read again otherwise, 16-byte stores of q.  q = e4m3(float(w) * 2^-e), round
// to nearest even by v_cvt_pk_fp8_f32; the product is exact and at most 448
// unless e met its clamp, where the overflow is made explicit (below).  A row
// with a non-finite element gets scale = NaN, so its column of y is NaN.
#include "toa_common.h"

#include "gemm_w8_shapes.h"

using namespace toa_w8;

typedef __attribute__((ext_vector_type(8))) short w8_s16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t w8_u32x2;
typedef __attribute__((ext_vector_type(2))) float w8_f32x2;

namespace {

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// eight e4m3 bytes (two words) -> eight bf16, exact
__device__ __forceinline__ w8_s16x8 cvt8(uint32_t w0, uint32_t w1) {
  const w8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const w8_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  const u32x4 v = {pack2(a[0], a[1]), pack2(b[0], b[1]), pack2(c[0], c[1]), pack2(d[0], d[1])};
  return __builtin_bit_cast(w8_s16x8, v);
}

__device__ __forceinline__ f32x4 mfma(w8_s16x8 a, u32x4 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(w8_s16x8, b), acc, 0, 0, 0);
}

template <bool SWIGLU>
__global__ __launch_bounds__(WAVES * 64) void gemm_w8_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                             const uint8_t* __restrict__ q, int64_t ldw,
                                                             const float* __restrict__ scale, bf16_t* __restrict__ y,
                                                             int64_t ldy, float* __restrict__ ws, int M, int N, int K,
                                                             int per, int nsplit) {
  __shared__ f32x4 red[WAVES][TILES][64];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int piece = blockIdx.y;
  // the first row of q of tile t, which is also its first entry of scale and its first column of a workspace row
  const int base0 = SWIGLU ? blockIdx.x * TILE_N : blockIdx.x * TILES * TILE_N;
  const int base1 = SWIGLU ? N + base0 : base0 + TILE_N;
  const bool two = SWIGLU || base1 < N;   // uniform over the workgroup
  const int nsteps = ksteps(K);
  const int s0 = min((piece * WAVES + wave) * per, nsteps), s1 = min(s0 + per, nsteps);
  const bool live = r < M;   // this lane's row of x exists

  const uint8_t* q0 = q + (int64_t)(base0 + r) * ldw + CHUNK * g;
  const uint8_t* q1 = q + (int64_t)((two ? base1 : base0) + r) * ldw + CHUNK * g;
  const bf16_t* xrow = x + (int64_t)(live ? r : 0) * ldx + CHUNK * g;

  const u32x4 zero = {0u, 0u, 0u, 0u};
  const f32x4 fzero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc0 = fzero, acc1 = fzero;

  // whole passes: every k-step below s1 and every lane's 16 columns below K
  int s = s0;
  for (; s + UNROLL <= s1 && (int64_t)(s + UNROLL) * KSTEP <= K; s += UNROLL) {
    const int64_t k0 = (int64_t)s * KSTEP;
    u32x4 a0[UNROLL], a1[UNROLL], b0[UNROLL], b1[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      a0[u] = ld16(q0 + k0 + u * KSTEP);
      a1[u] = two ? ld16(q1 + k0 + u * KSTEP) : zero;
    }
    if (live) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        b0[u] = ld16(xrow + k0 + u * KSTEP);
        b1[u] = ld16(xrow + k0 + u * KSTEP + 8);
      }
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) b0[u] = b1[u] = zero;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      acc0 = mfma(cvt8(a0[u][0], a0[u][1]), b0[u], acc0);
      acc1 = mfma(cvt8(a1[u][0], a1[u][1]), b0[u], acc1);
      acc0 = mfma(cvt8(a0[u][2], a0[u][3]), b1[u], acc0);
      acc1 = mfma(cvt8(a1[u][2], a1[u][3]), b1[u], acc1);
    }
  }
  // the slice's last, partial pass: k-steps at or beyond s1 and 16-column chunks at or beyond K are zeros, not loads
  if (s < s1) {
    u32x4 a0[UNROLL], a1[UNROLL], b0[UNROLL], b1[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k = (int64_t)(s + u) * KSTEP;
      const bool ok = s + u < s1 && k + CHUNK * g < K;
      a0[u] = ok ? ld16(q0 + k) : zero;
      a1[u] = ok && two ? ld16(q1 + k) : zero;
      b0[u] = ok && live ? ld16(xrow + k) : zero;
      b1[u] = ok && live ? ld16(xrow + k + 8) : zero;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      acc0 = mfma(cvt8(a0[u][0], a0[u][1]), b0[u], acc0);
      acc1 = mfma(cvt8(a1[u][0], a1[u][1]), b0[u], acc1);
      acc0 = mfma(cvt8(a0[u][2], a0[u][3]), b1[u], acc0);
      acc1 = mfma(cvt8(a1[u][2], a1[u][3]), b1[u], acc1);
    }
  }

  // the waves' slices, in wave order
  red[wave][0][lane] = acc0;
  red[wave][1][lane] = acc1;
  __syncthreads();
  if (wave != 0 || !live) return;
  f32x4 sum0 = red[0][0][lane], sum1 = red[0][1][lane];
#pragma unroll
  for (int v = 1; v < WAVES; ++v) {
    sum0 += red[v][0][lane];
    sum1 += red[v][1][lane];
  }
  // D: this lane holds row r, columns 4 g .. 4 g + 3 of each tile
  const int c0 = base0 + 4 * g, c1 = base1 + 4 * g;
  if (nsplit > 1) {
    float* p = ws + ((int64_t)piece * MAX_M + r) * (SWIGLU ? 2 * N : N);
    *(f32x4*)(p + c0) = sum0;
    if (two) *(f32x4*)(p + c1) = sum1;
    return;
  }
  f32x4 o0, o1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o0[j] = sum0[j] * scale[c0 + j];
    o1[j] = two ? sum1[j] * scale[c1 + j] : 0.f;
    if (SWIGLU) o0[j] = silu_mul(o0[j], o1[j]);
  }
  const w8_u32x2 out0 = {pack2(o0[0], o0[1]), pack2(o0[2], o0[3])};
  *(w8_u32x2*)(y + (int64_t)r * ldy + c0) = out0;
  if (!SWIGLU && two) {
    const w8_u32x2 out1 = {pack2(o1[0], o1[1]), pack2(o1[2], o1[3])};
    *(w8_u32x2*)(y + (int64_t)r * ldy + c1) = out1;
  }
}

// The pieces of a split launch in piece order, then the scale (and the SwiGLU): one thread per (row, four columns).
template <bool SWIGLU>
__global__ __launch_bounds__(MERGE_BLOCK) void gemm_w8_merge_kernel(const float* __restrict__ ws,
                                                                    const float* __restrict__ scale,
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
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[t][j] *= scale[(int64_t)t * N + n + j];
  }
  f32x4 o = sum[0];
  if (SWIGLU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = silu_mul(sum[0][j], sum[T - 1][j]);
  }
  const w8_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(w8_u32x2*)(y + (int64_t)m * ldy + n) = out;
}

template <bool SWIGLU>
int launch(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const float* scale, bf16_t* y, int64_t ldy,
           int M, int N, int K, float* ws, hipStream_t stream) {
  const int form = SWIGLU ? F_SWIGLU : F_PLAIN;
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)q, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws, o.SCALE = (uintptr_t)scale;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.M = M, o.N = N, o.K = K;
  o.w_rows = rows_of(form, N);   // the caller's statement: the launcher cannot see behind the pointers
  if (check(form, o) != R_OK) return (int)hipErrorInvalidValue;
  const int rows = rows_of(form, N);
  const int nsplit = split(rows, K), per = slice_steps(rows, K);
  const dim3 grid(workgroups(rows), nsplit), block(WAVES * 64);
  hipLaunchKernelGGL((gemm_w8_kernel<SWIGLU>), grid, block, 0, stream, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per,
                     nsplit);
  int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit == 1) return rc;
  const int64_t units = (int64_t)M * (N / 4);
  hipLaunchKernelGGL((gemm_w8_merge_kernel<SWIGLU>), dim3((unsigned)((units + MERGE_BLOCK - 1) / MERGE_BLOCK)),
                     dim3(MERGE_BLOCK), 0, stream, (const float*)ws, scale, y, ldy, M, N, nsplit);
  return (int)hipGetLastError();
}

// ---- the quantiser (the exponent rule, to_e4m3x4 and amax_bits: e4m3_quant.h)
__global__ __launch_bounds__(QUANT_BLOCK) void quant_w8_kernel(const bf16_t* __restrict__ w, int64_t ldw,
                                                               uint8_t* __restrict__ q, int64_t ldq,
                                                               float* __restrict__ scale, int K) {
  __shared__ u32x4 row[QUANT_LDS_K / 8];
  __shared__ uint32_t red[QUANT_BLOCK / 64];
  const int n = blockIdx.x, chunks = K / CHUNK;
  const bf16_t* wr = w + (int64_t)n * ldw;
  const bool keep = K <= QUANT_LDS_K;   // uniform

  // pass 1: the row's largest magnitude.  For bf16 bits with the sign cleared, integer order is the order of |w|,
  // and anything from 0x7f80 on is an infinity or a NaN.
  uint32_t m = 0;
  for (int c = threadIdx.x; c < chunks; c += QUANT_BLOCK) {
    const u32x4 lo = ld16(wr + (int64_t)c * CHUNK), hi = ld16(wr + (int64_t)c * CHUNK + 8);
    if (keep) row[2 * c] = lo, row[2 * c + 1] = hi;   // read back by this thread alone
    m = amax_bits(amax_bits(m, lo), hi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < QUANT_BLOCK / 64; ++v) m = max(m, red[v]);

  const bool finite = m < 0x7f80u;
  const int e = finite ? scale_exponent(m) : 0;
  if (threadIdx.x == 0) scale[n] = finite ? __uint_as_float((uint32_t)(127 + e) << 23) : __uint_as_float(0x7fc00000u);
  const float down = __uint_as_float((uint32_t)(127 - e) << 23);   // 2^-e: the product below is exact

  // pass 2
  for (int c = threadIdx.x; c < chunks; c += QUANT_BLOCK) {
    u32x4 in[2];
    if (keep) {
      in[0] = row[2 * c], in[1] = row[2 * c + 1];
    } else {
      in[0] = ld16(wr + (int64_t)c * CHUNK), in[1] = ld16(wr + (int64_t)c * CHUNK + 8);
    }
    u32x4 out;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[8];
      unpack8(in[h], f);
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] *= down;
      out[2 * h] = to_e4m3x4(f);
      out[2 * h + 1] = to_e4m3x4(f + 4);
    }
    st16(q + (int64_t)n * ldq + (int64_t)c * CHUNK, out);
  }
}

}  // namespace

extern "C" int toa_quant_w8(const bf16_t* w, int64_t ldw, uint8_t* q, int64_t ldq, float* scale, int N, int K,
                            hipStream_t stream) {
  if (!quant_ok((uintptr_t)w, (uintptr_t)q, (uintptr_t)scale, ldw, ldq, N, K)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_w8_kernel, dim3(N), dim3(QUANT_BLOCK), 0, stream, w, ldw, q, ldq, scale, K);
  return (int)hipGetLastError();
}

extern "C" int toa_gemm_skinny_w8(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const float* scale,
                                  bf16_t* y, int64_t ldy, int M, int N, int K, float* ws, hipStream_t stream) {
  return launch<false>(x, ldx, q, ldw, scale, y, ldy, M, N, K, ws, stream);
}

extern "C" int toa_gemm_skinny_w8_swiglu(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw,
                                         const float* scale, bf16_t* s, int64_t lds, int M, int F, int K, float* ws,
                                         hipStream_t stream) {
  return launch<true>(x, ldx, q, ldw, scale, s, lds, M, F, K, ws, stream);
}

// form: 0 plain, 1 SwiGLU (N = F).  0 = taken, else the first condition that fails; toa_gemm_skinny_w8_why names it.
extern "C" int toa_gemm_skinny_w8_check(int form, const void* x, const void* q, const void* y, const void* ws,
                                        const void* scale, int64_t ldx, int64_t ldw, int64_t ldy, int64_t w_rows,
                                        int M, int N, int K) {
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)q, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws, o.SCALE = (uintptr_t)scale;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.w_rows = w_rows, o.M = M, o.N = N, o.K = K;
  return (int)check(form, o);
}
extern "C" const char* toa_gemm_skinny_w8_why(int reason) { return why(reason); }
// bytes of fp32 workspace of the plain form (N, K) / the SwiGLU form (F, K); 0: no split, ws is not read
extern "C" int64_t toa_gemm_skinny_w8_ws_bytes(int N, int K) { return ws_bytes(F_PLAIN, N, K); }
extern "C" int64_t toa_gemm_skinny_w8_swiglu_ws_bytes(int F, int K) { return ws_bytes(F_SWIGLU, F, K); }
// the plan, for tests and the benchmark, by the rows of q (N; SwiGLU: 2F): K pieces across workgroups, k-steps per
// wave slice
extern "C" int toa_gemm_skinny_w8_split(int rows, int K) { return rows > 0 && K > 0 ? split(rows, K) : 0; }
extern "C" int toa_gemm_skinny_w8_slice_steps(int rows, int K) { return rows > 0 && K > 0 ? slice_steps(rows, K) : 0; }
// the header's constants, for the tests' shapes
extern "C" int toa_gemm_skinny_w8_constant(int which) {
  constexpr int v[] = {KSTEP, CHUNK, WAVES, UNROLL, MAX_SPLIT, TILE_N, TILES, MERGE_BLOCK, QUANT_LDS_K, MAX_M};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : 0;
}
