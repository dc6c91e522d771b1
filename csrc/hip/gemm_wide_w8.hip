// Weight-streaming GEMM on fp8 weights for 65 to 128 rows (gfx950): the
// projections of a decode step of groups x samples rows on shared prompts, of a
// prefill chunk of up to 128 tokens and of a KV-cache extend of that many rows
// on a weights snapshot, one byte read per weight.
//
//   toa_gemm_wide_w8         y[M][N] = bf16(scale[n] * sum_k x[m][k] q[n][k])
//   toa_gemm_wide_w8_swiglu  q = gate | up [2F][K], scale[2F];  s[M][F] = silu(scale g) * (scale u)
//
// x and y bf16, q OCP e4m3 with one fp32 scale per row (toa_quant_w8's
// tensors), fp32 accumulation, one fp32 multiply by the scale, one rounding to
// bf16; under SwiGLU both accumulators are scaled, then silu(g) * u, rounded
// once: gemm_w8.hip's rules.  What the launchers take and the launch plan:
// gemm_wide_w8_shapes.h (every name in capitals below is a constant there).
//
// Operand sides.  The tokens sit on the MFMA's N side and q on the A side, never
// staged: a k-step is KSTEP = 64 columns, lane (r = l & 15, g = l >> 4) loads
// the 16 bytes q[n0 + r][k0 + 16 g .. + 16) straight into registers and turns
// them into two bf16 A fragments (gemm_stream_w8.hip's cvt8: exact, every e4m3
// value is a bf16 value).  The lane's B operand of a tile of x is the 32
// contiguous bytes x[16 mt + r][k0 + 16 g .. + 16) from LDS, two ds_read_b128:
// bytes 0 .. 7 of q meet the first, bytes 8 .. 15 the second, so A and B give
// each of an MFMA's 32 (lane group, j) slots the same k, and each
// v_mfma_f32_16x16x32_bf16 adds 32 of the step's 64 products.  A wave owns
// TILES = 2 row tiles of q that share every B fragment (plain: tiles n0 and
// n0 + 16, the last wave of a grid one tile if N / 16 is odd; SwiGLU: the gate
// and the up tile of the same 16 columns of s), so one pair of conversions
// feeds 2 MT MFMAs a tile, MT = ceil(M / 16) = 5 .. 8 at compile time: a quarter
// to a half of the conversions per MFMA of the 17-to-64-row kernel.  D comes
// back as y[16 mt + (l & 15)][n0 + 4 (l >> 4) + j], j = 0 .. 3: one 8-byte store
// per lane, tile of x and tile of q.
//
// x goes through LDS.  A workgroup of WAVES waves is RG row groups x KG K
// groups and owns WG_ROWS = 128 rows of q.  It walks its K range in chunks of
// KC = 128 columns; all its threads copy x[16 MT][KC] with 16-byte loads,
// global -> registers -> LDS, two LDS buffers of 128 rows, 69 632 B of static
// LDS (one workgroup a CU of 160 KB), one barrier per chunk (chunk c + 1 is
// written after chunk c's MFMAs into the buffer chunk c - 1 was read from,
// which the barrier ending chunk c - 1 released).  Rows at or beyond M are
// zeroed in both buffers once and never loaded; columns at or beyond K are
// staged as zeros and not loaded.  Inside a chunk K group g takes k-step g.  An
// LDS row is KC + PAD elements, 272 B = 17 x 16 B: the 16 rows that the 16 lanes
// of one k group read start 16 B apart modulo 256 B, on 16 disjoint sets of
// four banks, in either half of the fragment.
//
// Loads run DEPTH = LOADS / (TILES * SPC) = 4 chunks ahead of the MFMAs, q's
// and x's, in register slots named at compile time: slot d of both rings holds
// chunks c0 + d, c0 + d + DEPTH, ...; each has one loader and one reader per
// trip and nothing moves between slots.  Each iteration issues x of chunk
// c + DEPTH, computes chunk c from registers and LDS, issues q of chunk
// c + DEPTH into the slot just read, then writes chunk c + 1 of x to LDS.
// Whole chunks load unconditionally; the chunk holding K's end and the chunks
// past a piece's end are predicated.
//
// The KG K groups of a row group merge through LDS in group order, both of a
// wave's tiles at once: 64 KB at MT = 8, inside the x buffers they reuse.  With
// split(rows of q, K) > 1 the workgroup takes piece blockIdx.y of the chunks
// and writes its fp32 partial to the workspace [split][MAX_M][rows of q]; a
// second kernel adds the pieces in piece order, then scales, then applies
// SwiGLU.  No float atomics, no counters, nothing read that this call did not
// write.  Chunking, the K groups' k-steps, the split and both merge orders are
// functions of (rows of q, K) alone and a column of D depends on that column
// of B alone, so a row's bits depend on that row of x, on q, on scale and on
// (rows of q, K) only: not on M, the row's index or an earlier launch.
//
// Row groups whose first tile is at or beyond the rows of q load and store
// nothing but stage x and keep every barrier.
#include "toa_common.h"

#include <type_traits>

#include "gemm_wide_w8_shapes.h"

using namespace toa_wide_w8;

typedef __attribute__((ext_vector_type(8))) short ww8_s16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t ww8_u32x2;
typedef __attribute__((ext_vector_type(2))) float ww8_f32x2;

namespace {

constexpr int THREADS = WAVES * 64;
constexpr int ROW_BYTES = (KC + PAD) * 2;          // one LDS row of x
constexpr int XBUF_BYTES = MAX_M * ROW_BYTES;      // one LDS buffer: x[128][KC + PAD]
constexpr int PIECES_PER_ROW = KC / 8;             // 16-byte pieces in a row of a chunk
constexpr int DEPTH = LOADS / (TILES * SPC);       // chunks the loads run ahead
static_assert(2 * XBUF_BYTES <= LDS_LIMIT, "static LDS over a gfx950 CU's");
static_assert((KG - 1) * RG * TILES * (MAX_M / 16) * 64 * 16 <= 2 * XBUF_BYTES, "the K groups' merge does not fit in the x buffers");
static_assert(DEPTH >= 2 && DEPTH % 2 == 0 && DEPTH <= MIN_CHUNKS, "the load ring and the two LDS buffers");
static_assert(KSTEP == 4 * CHUNK && CHUNK == 16, "one 16-byte load of q per lane and k-step");
static_assert((ROW_BYTES / 16) % 2 == 1, "LDS rows must start an odd number of 16-byte units apart");

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// eight e4m3 bytes (two words) -> eight bf16, exact
__device__ __forceinline__ ww8_s16x8 cvt8(uint32_t w0, uint32_t w1) {
  const ww8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const ww8_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  const u32x4 v = {pack2(a[0], a[1]), pack2(b[0], b[1]), pack2(c[0], c[1]), pack2(d[0], d[1])};
  return __builtin_bit_cast(ww8_s16x8, v);
}

__device__ __forceinline__ f32x4 mfma(ww8_s16x8 a, u32x4 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(ww8_s16x8, b), acc, 0, 0, 0);
}

// One thread's share of staging a chunk of x: XP 16-byte pieces (row p / 16, columns 8 (p % 16) ..), p = thread +
// THREADS i.  A piece whose row is at or beyond M is not live: its LDS slots are zeroed once, before the first chunk,
// and never written again.  So that a whole chunk's loads stand in straight-line code with no lane asked anything, a
// thread whose piece is not live loads row M - 1's piece instead (a row that is there) and drops it.
template <int XP>
struct XStage {
  const bf16_t* ptr[XP];   // the piece's address in chunk 0 (not live: row M - 1's)
  int col[XP];             // the piece's first column inside the chunk
  int lds[XP];             // its byte offset inside an LDS buffer, -1: not live
};

// chunk c of x into registers.  WHOLE: every column of the chunk is below K
template <int XP, bool WHOLE>
__device__ __forceinline__ void load_x(const XStage<XP>& xs, int c, int K, u32x4 (&v)[XP]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int64_t k = (int64_t)c * KC + xs.col[i];
    v[i] = WHOLE || (xs.lds[i] >= 0 && k < K) ? ld16(xs.ptr[i] + (int64_t)c * KC) : zero;
  }
}

// chunk c of this wave's q fragments into registers: SPC k-steps of each tile, 16 bytes = 16 columns a lane
template <bool WHOLE>
__device__ __forceinline__ void load_q(const uint8_t* const (&qrow)[TILES], int c, int kstep0, int g, int K,
                                       u32x4 (&a)[TILES][SPC]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int u = 0; u < SPC; ++u) {
    const int64_t k = (int64_t)c * KC + (int64_t)(kstep0 + u) * KSTEP;
    const bool ok = WHOLE || k + CHUNK * g < K;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = ok ? ld16(qrow[t] + k) : zero;
  }
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <int N, int I = 0, class F>
__device__ __forceinline__ void step_seq(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    step_seq<N, I + 1>(f);
  }
}

// One wave's work.  ACTIVE: its row group's first tile exists; a wave whose row group is at or beyond the rows of q
// stages x and keeps every barrier, and that is all.
template <bool SWIGLU, int MT, bool ACTIVE>
__device__ __forceinline__ void wide_w8_wave(unsigned char* smem, const bf16_t* __restrict__ x, int64_t ldx,
                                             const uint8_t* __restrict__ q, int64_t ldw,
                                             const float* __restrict__ scale, bf16_t* __restrict__ y, int64_t ldy,
                                             float* __restrict__ ws, int M, int N, int K, int per, int nsplit) {
  constexpr bool active = ACTIVE;
  constexpr int XP = (MT * 16 * PIECES_PER_ROW + THREADS - 1) / THREADS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int rg = wave % RG, kg = wave / RG;
  const int piece = blockIdx.y;
  // the first row of q of tile t, which is also its first entry of scale and its first column of a workspace row;
  // base[0] is the tile's first column of y as well (SwiGLU: of s)
  int base[TILES];
  base[0] = SWIGLU ? blockIdx.x * (RG * TILE_N) + rg * TILE_N : blockIdx.x * WG_ROWS + rg * (TILES * TILE_N);
  base[1] = SWIGLU ? N + base[0] : base[0] + TILE_N;
  const bool two = SWIGLU || base[1] < N;   // uniform over the wave: the plain form's last row group may own one tile
  const int nchunks = chunks(K);
  const int c0 = min(piece * per, nchunks), c1 = min(c0 + per, nchunks);
  const int whole_to = K / KC;                             // chunks below this have every column below K
  const int kstep0 = kg * SPC;

  XStage<XP> xs;
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int p = tid + THREADS * i, row = p / PIECES_PER_ROW, c8 = p % PIECES_PER_ROW;
    const bool live = row < M;
    xs.col[i] = 8 * c8;
    xs.lds[i] = live ? row * ROW_BYTES + 16 * c8 : -1;
    xs.ptr[i] = x + (int64_t)(live ? row : M - 1) * ldx + 8 * c8;
    if (!live && row < 16 * MT) {   // a row of zeros in both buffers, for every chunk
      *(u32x4*)(smem + row * ROW_BYTES + 16 * c8) = u32x4{0u, 0u, 0u, 0u};
      *(u32x4*)(smem + XBUF_BYTES + row * ROW_BYTES + 16 * c8) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  // a tile that is not there reads tile 0's rows (rows that are) and its sums are dropped
  const uint8_t* qrow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
    qrow[t] = q + (int64_t)(active ? base[t == 0 || two ? t : 0] + r : 0) * ldw + CHUNK * g;

  const u32x4 zero = {0u, 0u, 0u, 0u};
  const f32x4 fzero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[TILES][MT];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[t][m] = fzero;
  }

  // Chunk c into registers.  steady: c is below c1 and all its columns are below K, so no load is asked anything;
  // else nothing at or beyond c1 and, in K's last chunk, no column at or beyond K and no row that is not live.
  auto issue_x = [&](auto steady, int c, u32x4(&v)[XP]) {
    if constexpr (decltype(steady)::value) {
      load_x<XP, true>(xs, c, K, v);
    } else if (c < c1) {
      load_x<XP, false>(xs, c, K, v);
    } else {
#pragma unroll
      for (int i = 0; i < XP; ++i) v[i] = zero;
    }
  };
  auto issue_q = [&](auto steady, int c, u32x4(&a)[TILES][SPC]) {
    if constexpr (decltype(steady)::value) {
      load_q<true>(qrow, c, kstep0, g, K, a);
    } else if (c < c1) {
      load_q<false>(qrow, c, kstep0, g, K, a);
    } else {
#pragma unroll
      for (int u = 0; u < SPC; ++u) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) a[t][u] = zero;
      }
    }
  };
  auto stage = [&](const u32x4(&v)[XP], int buf) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      if (xs.lds[i] >= 0) *(u32x4*)(smem + buf * XBUF_BYTES + xs.lds[i]) = v[i];
    }
  };

  // Slot d of both rings holds chunks c0 + d, c0 + d + DEPTH, ...  DEPTH is even: chunk c0 + j is in LDS buffer
  // j & 1 = d & 1.
  const int frag = r * ROW_BYTES + (kstep0 * KSTEP + CHUNK * g) * 2;   // this lane's B fragment of tile 0, k-step 0
  u32x4 xq[DEPTH][XP], aq[DEPTH][TILES][SPC];
  // One chunk: x of chunk c + DEPTH is issued into the slot whose x went to LDS one step ago; the MFMAs of chunk c;
  // q of chunk c + DEPTH into the slot they have just read; x of chunk c + 1 to LDS; the barrier.
  auto step = [&](auto steady, int c, auto slot) {
    constexpr int d = decltype(slot)::value, buf = d & 1;
    issue_x(steady, c + DEPTH, xq[d]);
    if (active) {
#pragma unroll
      for (int u = 0; u < SPC; ++u) {
        ww8_s16x8 lo[TILES], hi[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          lo[t] = cvt8(aq[d][t][u][0], aq[d][t][u][1]);
          hi[t] = cvt8(aq[d][t][u][2], aq[d][t][u][3]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const unsigned char* bp = smem + buf * XBUF_BYTES + frag + m * 16 * ROW_BYTES + u * KSTEP * 2;
          const u32x4 b0 = *(const u32x4*)bp, b1 = *(const u32x4*)(bp + 16);
#pragma unroll
          for (int t = 0; t < TILES; ++t) acc[t][m] = mfma(lo[t], b0, acc[t][m]);
#pragma unroll
          for (int t = 0; t < TILES; ++t) acc[t][m] = mfma(hi[t], b1, acc[t][m]);
        }
      }
      issue_q(steady, c + DEPTH, aq[d]);
    }
    if (decltype(steady)::value || c + 1 < c1) stage(xq[(d + 1) % DEPTH], buf ^ 1);
    __syncthreads();
  };
  // DEPTH steps with the slots as constants
  auto trip = [&](auto steady, int c) {
    step_seq<DEPTH>([&](auto slot) {
      if (decltype(steady)::value || c + decltype(slot)::value < c1) step(steady, c + decltype(slot)::value, slot);
    });
  };

  const int lim = min(c1, whole_to);
  if (c0 + DEPTH <= lim) {
    step_seq<DEPTH>([&](auto slot) {
      constexpr int d = decltype(slot)::value;
      issue_x(std::true_type{}, c0 + d, xq[d]);
      if (active) issue_q(std::true_type{}, c0 + d, aq[d]);
    });
  } else {
    step_seq<DEPTH>([&](auto slot) {
      constexpr int d = decltype(slot)::value;
      issue_x(std::false_type{}, c0 + d, xq[d]);
      if (active) issue_q(std::false_type{}, c0 + d, aq[d]);
    });
  }
  if (c0 < c1) stage(xq[0], 0);
  __syncthreads();

  int c = c0;
  for (; c + 2 * DEPTH <= lim; c += DEPTH) trip(std::true_type{}, c);   // every chunk issued is whole and below c1
  for (; c < c1; c += DEPTH) trip(std::false_type{}, c);

  // The K groups in group order, both tiles at once.  Every read of the x buffers is behind the last barrier, so the
  // merge reuses them: (KG - 1) * RG * TILES * MT blocks of 64 f32x4, 64 KB of the buffers' 68 at MT = 8.
  f32x4* red = (f32x4*)smem;
  if (kg != 0 && active) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m) red[((((kg - 1) * RG + rg) * TILES + t) * MT + m) * 64 + lane] = acc[t][m];
    }
  }
  __syncthreads();
  if (kg != 0 || !active) return;
#pragma unroll
  for (int v = 1; v < KG; ++v) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[t][m] += red[((((v - 1) * RG + rg) * TILES + t) * MT + m) * 64 + lane];
    }
  }
  // D: this lane holds rows 16 m + r, columns 4 g .. 4 g + 3 of each tile
  if (nsplit > 1) {
    const int64_t cols = SWIGLU ? 2 * (int64_t)N : N;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int row = 16 * m + r;
      if (row >= M) continue;
      float* p = ws + ((int64_t)piece * MAX_M + row) * cols + 4 * g;
      *(f32x4*)(p + base[0]) = acc[0][m];
      if (two) *(f32x4*)(p + base[1]) = acc[1][m];
    }
    return;
  }
  float sc[TILES][4];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[t][j] = t == 0 || two ? scale[base[t] + 4 * g + j] : 0.f;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = 16 * m + r;
    if (row >= M) continue;
    f32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = acc[0][m][j] * sc[0][j];
      o1[j] = acc[1][m][j] * sc[1][j];
      if (SWIGLU) o0[j] = silu_mul(o0[j], o1[j]);
    }
    const ww8_u32x2 out0 = {pack2(o0[0], o0[1]), pack2(o0[2], o0[3])};
    *(ww8_u32x2*)(y + (int64_t)row * ldy + base[0] + 4 * g) = out0;
    if (!SWIGLU && two) {
      const ww8_u32x2 out1 = {pack2(o1[0], o1[1]), pack2(o1[2], o1[3])};
      *(ww8_u32x2*)(y + (int64_t)row * ldy + base[1] + 4 * g) = out1;
    }
  }
}

template <bool SWIGLU, int MT>
__global__ __launch_bounds__(THREADS) void gemm_wide_w8_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                               const uint8_t* __restrict__ q, int64_t ldw,
                                                               const float* __restrict__ scale,
                                                               bf16_t* __restrict__ y, int64_t ldy,
                                                               float* __restrict__ ws, int M, int N, int K, int per,
                                                               int nsplit) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XBUF_BYTES];
  // wave-uniform: both sides walk the same chunks and meet at the same number of barriers
  const int rg = (threadIdx.x >> 6) % RG;
  const int first = SWIGLU ? blockIdx.x * (RG * TILE_N) + rg * TILE_N : blockIdx.x * WG_ROWS + rg * (TILES * TILE_N);
  if (first < N)
    wide_w8_wave<SWIGLU, MT, true>(smem, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit);
  else
    wide_w8_wave<SWIGLU, MT, false>(smem, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit);
}

// The pieces of a split launch in piece order, then the scale (and the SwiGLU): one thread per (row, four columns).
template <bool SWIGLU>
__global__ __launch_bounds__(MERGE_BLOCK) void gemm_wide_w8_merge_kernel(const float* __restrict__ ws,
                                                                         const float* __restrict__ scale,
                                                                         bf16_t* __restrict__ y, int64_t ldy, int M,
                                                                         int N, int nsplit) {
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
  const ww8_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(ww8_u32x2*)(y + (int64_t)m * ldy + n) = out;
}

template <bool SWIGLU, int MT>
void launch_mt(dim3 grid, const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const float* scale, bf16_t* y,
               int64_t ldy, float* ws, int M, int N, int K, int per, int nsplit, hipStream_t stream) {
  hipLaunchKernelGGL((gemm_wide_w8_kernel<SWIGLU, MT>), grid, dim3(THREADS), 0, stream, x, ldx, q, ldw, scale, y, ldy,
                     ws, M, N, K, per, nsplit);
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
  const int nsplit = split(rows, K), per = piece_chunks(rows, K);
  const dim3 grid(workgroups(rows), nsplit);
  switch ((M + 15) / 16) {   // the plan above is (rows, K)'s; M chooses only how many tiles of x a q fragment feeds
    case 5: launch_mt<SWIGLU, 5>(grid, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit, stream); break;
    case 6: launch_mt<SWIGLU, 6>(grid, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit, stream); break;
    case 7: launch_mt<SWIGLU, 7>(grid, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit, stream); break;
    default: launch_mt<SWIGLU, 8>(grid, x, ldx, q, ldw, scale, y, ldy, ws, M, N, K, per, nsplit, stream);
  }
  int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit == 1) return rc;
  const int64_t units = (int64_t)M * (N / 4);
  hipLaunchKernelGGL((gemm_wide_w8_merge_kernel<SWIGLU>), dim3((unsigned)((units + MERGE_BLOCK - 1) / MERGE_BLOCK)),
                     dim3(MERGE_BLOCK), 0, stream, (const float*)ws, scale, y, ldy, M, N, nsplit);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int toa_gemm_wide_w8(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const float* scale,
                                bf16_t* y, int64_t ldy, int M, int N, int K, float* ws, hipStream_t stream) {
  return launch<false>(x, ldx, q, ldw, scale, y, ldy, M, N, K, ws, stream);
}

extern "C" int toa_gemm_wide_w8_swiglu(const bf16_t* x, int64_t ldx, const uint8_t* q, int64_t ldw, const float* scale,
                                       bf16_t* s, int64_t lds, int M, int F, int K, float* ws, hipStream_t stream) {
  return launch<true>(x, ldx, q, ldw, scale, s, lds, M, F, K, ws, stream);
}

// form: 0 plain, 1 SwiGLU (N = F).  0 = taken, else the first condition that fails; toa_gemm_wide_w8_why names it.
extern "C" int toa_gemm_wide_w8_check(int form, const void* x, const void* q, const void* y, const void* ws,
                                      const void* scale, int64_t ldx, int64_t ldw, int64_t ldy, int64_t w_rows, int M,
                                      int N, int K) {
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)q, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws, o.SCALE = (uintptr_t)scale;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.w_rows = w_rows, o.M = M, o.N = N, o.K = K;
  return (int)check(form, o);
}
extern "C" const char* toa_gemm_wide_w8_why(int reason) { return why(reason); }
// bytes of fp32 workspace of the plain form (N, K) / the SwiGLU form (F, K); 0: no split, ws is not read
extern "C" int64_t toa_gemm_wide_w8_ws_bytes(int N, int K) { return ws_bytes(F_PLAIN, N, K); }
extern "C" int64_t toa_gemm_wide_w8_swiglu_ws_bytes(int F, int K) { return ws_bytes(F_SWIGLU, F, K); }
// the plan, for tests and the benchmark, by the rows of q (N; SwiGLU: 2F): K pieces across workgroups, chunks of KC
// columns per piece
extern "C" int toa_gemm_wide_w8_split(int rows, int K) { return rows > 0 && K > 0 ? split(rows, K) : 0; }
extern "C" int toa_gemm_wide_w8_piece_chunks(int rows, int K) { return rows > 0 && K > 0 ? piece_chunks(rows, K) : 0; }
// the constants the tests' shapes are named from: 0 KC, 1 KG, 2 SPC, 3 KSTEP, 4 WG_ROWS, 5 MIN_CHUNKS, 6 MAX_M,
// 7 MIN_M, 8 TILE_N, 9 TILES, 10 CHUNK, 11 MERGE_BLOCK
extern "C" int toa_gemm_wide_w8_constant(int which) {
  constexpr int v[] = {KC, KG, SPC, KSTEP, WG_ROWS, MIN_CHUNKS, MAX_M, MIN_M, TILE_N, TILES, CHUNK, MERGE_BLOCK};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : 0;
}
