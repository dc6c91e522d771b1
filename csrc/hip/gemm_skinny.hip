// Weight-streaming GEMM for 1 to 16 rows (gfx950): the projections of a
// KV-cache decode step, where every weight byte is read once for a handful of
// token rows and HBM sets the time.
//
//   toa_gemm_skinny         y[M][N] = x[M][K] w[N][K]^T
//   toa_gemm_skinny_swiglu  w = gate | up [2F][K];  s[M][F] = silu(x wg^T) * (x wu^T)
//
// bf16 operands, fp32 accumulation, one rounding to bf16; the SwiGLU product
// is taken from the fp32 accumulators.  What the launchers take and the launch
// plan: gemm_skinny_shapes.h (every name in capitals below is a constant there).
//
// The tokens sit on the MFMA's N side.  One v_mfma_f32_16x16x32_bf16 takes
// A = 16 rows of W and B = x^T: lane l holds A[row l&15][k = 8(l>>4) + j] and
// B[k = 8(l>>4) + j][col l&15], so both fragments are one 16-byte k-contiguous
// global load per lane straight into registers -- no LDS image, no transpose.
// Lanes whose l&15 >= M supply zeros and load nothing.  D comes back as
// y[m = l&15][n0 + 4(l>>4) + r], r = 0..3: one 8-byte store per lane.  A
// column of D depends on that column of B alone, so a row's bits do not depend
// on M or on the other rows.
//
// Grid (N / TILE_N row tiles, split pieces), WAVES waves.  A workgroup owns
// one row tile (SwiGLU: the gate tile and the up tile of the same 16 columns
// of s, sharing the x fragment); its waves take disjoint K slices of it --
// slice i = piece * WAVES + wave, slice_steps(N, K) k-steps each, so the
// slicing is a function of (N, K) alone -- and keep UNROLL 16-byte W loads in
// flight per lane.  A slice's whole passes load without a condition; the one
// partial pass at its end (and the one partial 8-column chunk at the end of K)
// is predicated per k-step.  The waves' accumulators merge through LDS in wave
// order.  With split(N, K) > 1 (few row tiles: under WAVES waves per CU) the
// workgroup writes its fp32 partial to the workspace [split][MAX_M][cols]
// and a second kernel adds the pieces in piece order and finishes; no float
// atomics, no counters, nothing read that this call did not write.
#include "toa_common.h"

#include "gemm_skinny_shapes.h"

using namespace toa_skinny;

typedef __attribute__((ext_vector_type(8))) short sk_s16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t sk_u32x2;

namespace {

// The W stream with the default cache policy (0, the default) or non-temporal (1): toa_gemm_skinny_set_nt, for
// in-process A/B runs.  Measured on an MI355X over rotating copies of W (scripts/decode_step_bench.py, docs/kernels.md
// "Decoding"): non-temporal loads were 0 to 16 % SLOWER at every Llama-3-8B form and row count, so they are not the default.
int g_skinny_nt = 0;

template <bool NT>
__device__ __forceinline__ u32x4 ld_w(const bf16_t* p) {
  return NT ? __builtin_nontemporal_load((const u32x4*)p) : *(const u32x4*)p;
}

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

template <bool SWIGLU, bool NT>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                                 const bf16_t* __restrict__ w, int64_t ldw,
                                                                 bf16_t* __restrict__ y, int64_t ldy,
                                                                 float* __restrict__ ws, int M, int N, int K, int per,
                                                                 int nsplit) {
  constexpr int TILES = SWIGLU ? 2 : 1;
  constexpr int STEPS = UNROLL / TILES;   // k-steps per pass
  __shared__ f32x4 red[WAVES][TILES][64];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * TILE_N, piece = blockIdx.y;
  const int nsteps = ksteps(K);
  const int s0 = min((piece * WAVES + wave) * per, nsteps), s1 = min(s0 + per, nsteps);
  const bool live = r < M;   // this lane's row of x exists

  const bf16_t* wrow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) wrow[t] = w + ((int64_t)t * N + n0 + r) * ldw + 8 * g;
  const bf16_t* xrow = x + (int64_t)(live ? r : 0) * ldx + 8 * g;

  const u32x4 zero = {0u, 0u, 0u, 0u};
  const f32x4 fzero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = fzero;

  // whole passes: every k-step below s1 and every lane's 8 columns below K
  int s = s0;
  for (; s + STEPS <= s1 && (int64_t)(s + STEPS) * KSTEP <= K; s += STEPS) {
    const int64_t k0 = (int64_t)s * KSTEP;
    u32x4 a[TILES][STEPS], b[STEPS];
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) a[t][u] = ld_w<NT>(wrow[t] + k0 + u * KSTEP);
    }
    if (live) {
#pragma unroll
      for (int u = 0; u < STEPS; ++u) b[u] = ld16(xrow + k0 + u * KSTEP);
    } else {
#pragma unroll
      for (int u = 0; u < STEPS; ++u) b[u] = zero;
    }
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
#pragma unroll
      for (int t = 0; t < TILES; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sk_s16x8, a[t][u]),
                                                         __builtin_bit_cast(sk_s16x8, b[u]), acc[t], 0, 0, 0);
    }
  }
  // the slice's last, partial pass: k-steps at or beyond s1 and 8-column chunks at or beyond K are zeros, not loads
  if (s < s1) {
    u32x4 a[TILES][STEPS], b[STEPS];
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
      const int64_t k = (int64_t)(s + u) * KSTEP;
      const bool ok = s + u < s1 && k + 8 * g < K;
#pragma unroll
      for (int t = 0; t < TILES; ++t) a[t][u] = ok ? ld_w<NT>(wrow[t] + k) : zero;
      b[u] = ok && live ? ld16(xrow + k) : zero;
    }
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
#pragma unroll
      for (int t = 0; t < TILES; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sk_s16x8, a[t][u]),
                                                         __builtin_bit_cast(sk_s16x8, b[u]), acc[t], 0, 0, 0);
    }
  }

  // the waves' slices, in wave order
#pragma unroll
  for (int t = 0; t < TILES; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave != 0 || !live) return;
  f32x4 sum[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    sum[t] = red[0][t][lane];
#pragma unroll
    for (int v = 1; v < WAVES; ++v) sum[t] += red[v][t][lane];
  }
  const int n = n0 + 4 * g;   // this lane's four columns of row r
  if (nsplit > 1) {
    const int64_t cols = (int64_t)TILES * N;
    float* p = ws + ((int64_t)piece * MAX_M + r) * cols + n;
#pragma unroll
    for (int t = 0; t < TILES; ++t) *(f32x4*)(p + (int64_t)t * N) = sum[t];
    return;
  }
  f32x4 o = sum[0];
  if (SWIGLU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = silu_mul(sum[0][j], sum[TILES - 1][j]);
  }
  const sk_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(sk_u32x2*)(y + (int64_t)r * ldy + n) = out;
}

// The pieces of a split launch in piece order: one thread per (row, four columns).
template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemm_skinny_merge_kernel(const float* __restrict__ ws, bf16_t* __restrict__ y,
                                                                int64_t ldy, int M, int N, int nsplit) {
  constexpr int TILES = SWIGLU ? 2 : 1;
  const int quads = N / 4;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * quads) return;
  const int m = (int)(i / quads), n = (int)(i % quads) * 4;
  const int64_t cols = (int64_t)TILES * N;
  f32x4 sum[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const float* p = ws + (int64_t)m * cols + (int64_t)t * N + n;
    sum[t] = *(const f32x4*)p;
    for (int s = 1; s < nsplit; ++s) sum[t] += *(const f32x4*)(p + (int64_t)s * MAX_M * cols);
  }
  f32x4 o = sum[0];
  if (SWIGLU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = silu_mul(sum[0][j], sum[TILES - 1][j]);
  }
  const sk_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(sk_u32x2*)(y + (int64_t)m * ldy + n) = out;
}

template <bool SWIGLU>
int launch(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, bf16_t* y, int64_t ldy, int M, int N, int K,
           float* ws, hipStream_t stream) {
  const int form = SWIGLU ? F_SWIGLU : F_PLAIN;
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)w, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.M = M, o.N = N, o.K = K;
  o.w_rows = SWIGLU ? 2 * (int64_t)N : N;   // the caller's statement: the launcher cannot see behind the pointer
  if (check(form, o) != R_OK) return (int)hipErrorInvalidValue;
  const int nsplit = split(N, K), per = slice_steps(N, K);
  const dim3 grid(N / TILE_N, nsplit), block(WAVES * 64);
  if (g_skinny_nt)
    hipLaunchKernelGGL((gemm_skinny_kernel<SWIGLU, true>), grid, block, 0, stream, x, ldx, w, ldw, y, ldy, ws, M, N, K,
                       per, nsplit);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<SWIGLU, false>), grid, block, 0, stream, x, ldx, w, ldw, y, ldy, ws, M, N,
                       K, per, nsplit);
  int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit == 1) return rc;
  const int64_t units = (int64_t)M * (N / 4);
  hipLaunchKernelGGL((gemm_skinny_merge_kernel<SWIGLU>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream,
                     (const float*)ws, y, ldy, M, N, nsplit);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int toa_gemm_skinny(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, bf16_t* y, int64_t ldy,
                               int M, int N, int K, float* ws, hipStream_t stream) {
  return launch<false>(x, ldx, w, ldw, y, ldy, M, N, K, ws, stream);
}

extern "C" int toa_gemm_skinny_swiglu(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, bf16_t* s,
                                      int64_t lds, int M, int F, int K, float* ws, hipStream_t stream) {
  return launch<true>(x, ldx, w, ldw, s, lds, M, F, K, ws, stream);
}

// form: 0 plain, 1 SwiGLU (N = F).  0 = taken, else the first condition that fails; toa_gemm_skinny_why names it.
extern "C" int toa_gemm_skinny_check(int form, const void* x, const void* w, const void* y, const void* ws,
                                     int64_t ldx, int64_t ldw, int64_t ldy, int64_t w_rows, int M, int N, int K) {
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)w, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.w_rows = w_rows, o.M = M, o.N = N, o.K = K;
  return (int)check(form, o);
}
extern "C" const char* toa_gemm_skinny_why(int reason) { return why(reason); }
// bytes of fp32 workspace of the plain form (N, K) / the SwiGLU form (F, K); 0: no split, ws is not read
extern "C" int64_t toa_gemm_skinny_ws_bytes(int N, int K) { return ws_bytes(F_PLAIN, N, K); }
extern "C" int64_t toa_gemm_skinny_swiglu_ws_bytes(int F, int K) { return ws_bytes(F_SWIGLU, F, K); }
// the plan, for tests and the benchmark: K pieces across workgroups, k-steps per wave slice
extern "C" int toa_gemm_skinny_split(int N, int K) { return N > 0 && K > 0 ? split(N, K) : 0; }
extern "C" int toa_gemm_skinny_slice_steps(int N, int K) { return N > 0 && K > 0 ? slice_steps(N, K) : 0; }
extern "C" int toa_gemm_skinny_set_nt(int nt) {
  g_skinny_nt = nt != 0;
  return 0;
}
