// Weight-streaming GEMM for 17 to 64 rows (gfx950): the projections of a
// KV-cache extend (drafted tokens to verify, a second turn, a prefill chunk)
// and of decode steps of more than 16 rows, where every weight byte is still
// read once and HBM sets the time.
//
//   toa_gemm_stream         y[M][N] = x[M][K] w[N][K]^T
//   toa_gemm_stream_swiglu  w = gate | up [2F][K];  s[M][F] = silu(x wg^T) * (x wu^T)
//
// bf16 operands, fp32 accumulation, one rounding to bf16; the SwiGLU product
// is taken from the fp32 accumulators.  What the launchers take and the launch
// plan: gemm_stream_shapes.h (every name in capitals below is a constant there).
//
// The tokens sit on the MFMA's N side, as in gemm_skinny.hip: one
// v_mfma_f32_16x16x32_bf16 takes A = 16 rows of W, lane l holding
// A[row l&15][k = 8(l>>4) + j], one 16-byte k-contiguous global load straight
// into registers, and B[k = 8(l>>4) + j][col l&15] = one 16-row tile of x.
// A W fragment feeds MT = ceil(M / 16) MFMAs, one per tile of x (the kernel is
// instantiated for MT = 2, 3, 4); W is never staged and each of its bytes is
// read once per launch.  D comes back as y[16 mt + (l&15)][n0 + 4(l>>4) + r],
// r = 0..3: one 8-byte store per lane and tile.
//
// x goes through LDS.  A workgroup of WAVES waves is RG row groups x KG K
// groups and owns RG * TILE_N = 64 rows of W (SwiGLU: the gate rows and the up
// rows of the same 64 columns of s, sharing the x fragments), so L2 serves x
// once per 64 rows of W and not once per 16.  The workgroup walks its K range
// in chunks of KC columns.  All its threads copy x[16 MT][KC] with 16-byte
// loads: global -> registers -> LDS, two LDS buffers, one barrier per chunk
// (chunk c + 1 is written after chunk c's MFMAs into the buffer that chunk
// c - 1 was read from, which the barrier ending chunk c - 1 released).  Rows
// at or beyond M are zeroed in both buffers once and never loaded; columns at
// or beyond K are staged as zeros and not loaded.  Inside a chunk K group g takes k-steps g SPC .. g SPC + SPC - 1; a
// B fragment is one ds_read_b128 per lane and tile of x.  An LDS row is KC +
// PAD elements, 272 B: the 16 rows that the 16 lanes of one k group read start
// 16 B apart modulo 256 B, on 16 disjoint sets of four banks.
//
// Loads run DEPTH = LOADS / (tiles * SPC) chunks ahead of the MFMAs, both W's
// and x's: returns are counted in issue order, so an x chunk that were loaded
// only one chunk ahead would make its LDS write wait for every W load before
// it.  Each iteration issues chunk c + DEPTH, computes chunk c from registers
// and LDS, then writes chunk c + 1 of x (issued DEPTH - 1 iterations ago) to
// LDS: at that wait DEPTH - 1 chunks of x and DEPTH chunks of W, LOADS 16-byte
// loads per lane, stay in flight.
//
// The KG K groups of a row group merge through LDS in group order.  With
// split(N, K) > 1 (under MIN_WGS workgroups) the workgroup takes piece
// blockIdx.y of the chunks and writes its fp32 partial to the workspace
// [split][MAX_M][cols]; a second kernel adds the pieces in piece order and
// finishes.  No float atomics, no counters, nothing read that this call did
// not write.  Chunking, the K groups' k-steps, the split and both merge orders
// are functions of (N, K) alone and a column of D depends on that column of B
// alone, so a row's bits depend on that row of x, on W and on (N, K) only.
//
// Row groups at or beyond N (N is a multiple of 16, not of 64) load and store
// nothing but stage x and keep every barrier.
#include "toa_common.h"

#include <type_traits>

#include "gemm_stream_shapes.h"

using namespace toa_stream;

typedef __attribute__((ext_vector_type(8))) short st_s16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t st_u32x2;

namespace {

constexpr int THREADS = WAVES * 64;
constexpr int ROW_BYTES = (KC + PAD) * 2;          // one LDS row of x
constexpr int XBUF_BYTES = MAX_M * ROW_BYTES;      // one LDS buffer: x[64][KC + PAD]
constexpr int PIECES_PER_ROW = KC / 8;             // 16-byte pieces in a row of a chunk
static_assert(2 * XBUF_BYTES <= 64 * 1024, "static LDS over 64 KB");
static_assert(RG * 2 * (MAX_M / 16) * 64 * 16 <= 2 * XBUF_BYTES, "the K groups' merge does not fit in the x buffers");

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

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
__device__ __forceinline__ void load_x(const XStage<XP>& xs, int c, int K, u32x4 (&q)[XP]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int64_t k = (int64_t)c * KC + xs.col[i];
    q[i] = WHOLE || (xs.lds[i] >= 0 && k < K) ? ld16(xs.ptr[i] + (int64_t)c * KC) : zero;
  }
}

// chunk c of this wave's W fragments into registers: SPC k-steps of each tile
template <int TILES, bool WHOLE>
__device__ __forceinline__ void load_w(const bf16_t* const (&wrow)[TILES], int c, int kstep0, int g, int K,
                                       u32x4 (&a)[TILES][SPC]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int u = 0; u < SPC; ++u) {
    const int64_t k = (int64_t)c * KC + (int64_t)(kstep0 + u) * KSTEP;
    const bool ok = WHOLE || k + 8 * g < K;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = ok ? ld16(wrow[t] + k) : zero;
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

// One wave's work.  ACTIVE: its row group's 16 rows of W exist (n0 < N); a wave whose row group is at or beyond N
// stages x and keeps every barrier, and that is all.
template <bool SWIGLU, int MT, bool ACTIVE>
__device__ __forceinline__ void stream_wave(unsigned char* smem, const bf16_t* __restrict__ x, int64_t ldx,
                                            const bf16_t* __restrict__ w, int64_t ldw, bf16_t* __restrict__ y,
                                            int64_t ldy, float* __restrict__ ws, int M, int N, int K, int per,
                                            int nsplit) {
  constexpr bool active = ACTIVE;
  constexpr int TILES = SWIGLU ? 2 : 1;
  constexpr int DEPTH = LOADS / (TILES * SPC);            // chunks the loads run ahead
  constexpr int XP = (MT * 16 * PIECES_PER_ROW + THREADS - 1) / THREADS;
  static_assert(DEPTH >= 2 && DEPTH % 2 == 0 && DEPTH <= MIN_CHUNKS, "the load ring and the two LDS buffers");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int rg = wave % RG, kg = wave / RG;
  const int n0 = blockIdx.x * WG_N + rg * TILE_N, piece = blockIdx.y;
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
  const bf16_t* wrow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) wrow[t] = w + ((int64_t)t * N + (active ? n0 + r : 0)) * ldw + 8 * g;

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
  auto issue_x = [&](auto steady, int c, u32x4(&q)[XP]) {
    if constexpr (decltype(steady)::value) {
      load_x<XP, true>(xs, c, K, q);
    } else if (c < c1) {
      load_x<XP, false>(xs, c, K, q);
    } else {
#pragma unroll
      for (int i = 0; i < XP; ++i) q[i] = zero;
    }
  };
  auto issue_w = [&](auto steady, int c, u32x4(&a)[TILES][SPC]) {
    if constexpr (decltype(steady)::value) {
      load_w<TILES, true>(wrow, c, kstep0, g, K, a);
    } else if (c < c1) {
      load_w<TILES, false>(wrow, c, kstep0, g, K, a);
    } else {
#pragma unroll
      for (int u = 0; u < SPC; ++u) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) a[t][u] = zero;
      }
    }
  };
  auto stage = [&](const u32x4(&q)[XP], int buf) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      if (xs.lds[i] >= 0) *(u32x4*)(smem + buf * XBUF_BYTES + xs.lds[i]) = q[i];
    }
  };

  // Slot d of both rings holds chunks c0 + d, c0 + d + DEPTH, ...: every register has one loader and one reader per
  // trip and nothing is moved between slots, so no move waits on a load in flight.  DEPTH is even: chunk c0 + j is
  // in LDS buffer j & 1 = d & 1.
  const int frag = r * ROW_BYTES + (kstep0 * KSTEP + 8 * g) * 2;   // this lane's B fragment of tile 0, k-step 0
  u32x4 xq[DEPTH][XP], aq[DEPTH][TILES][SPC];
  // One chunk: x of chunk c + DEPTH is issued into the slot whose x went to LDS one step ago; the MFMAs of chunk c;
  // W of chunk c + DEPTH into the slot they have just read; x of chunk c + 1 to LDS; the barrier.
  auto step = [&](auto steady, int c, auto slot) {
    constexpr int d = decltype(slot)::value, buf = d & 1;
    issue_x(steady, c + DEPTH, xq[d]);
    if (active) {
#pragma unroll
      for (int u = 0; u < SPC; ++u) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const u32x4 b = *(const u32x4*)(smem + buf * XBUF_BYTES + frag + m * 16 * ROW_BYTES + u * KSTEP * 2);
#pragma unroll
          for (int t = 0; t < TILES; ++t)
            acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(st_s16x8, aq[d][t][u]),
                                                                __builtin_bit_cast(st_s16x8, b), acc[t][m], 0, 0, 0);
        }
      }
      issue_w(steady, c + DEPTH, aq[d]);
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
      if (active) issue_w(std::true_type{}, c0 + d, aq[d]);
    });
  } else {
    step_seq<DEPTH>([&](auto slot) {
      constexpr int d = decltype(slot)::value;
      issue_x(std::false_type{}, c0 + d, xq[d]);
      if (active) issue_w(std::false_type{}, c0 + d, aq[d]);
    });
  }
  if (c0 < c1) stage(xq[0], 0);
  __syncthreads();

  int c = c0;
  for (; c + 2 * DEPTH <= lim; c += DEPTH) trip(std::true_type{}, c);   // every chunk issued is whole and below c1
  for (; c < c1; c += DEPTH) trip(std::false_type{}, c);

  // the K groups in group order; every read of the x buffers is behind the last barrier, so the merge reuses them
  f32x4* red = (f32x4*)smem;
  if (kg != 0 && active) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m) red[(((kg - 1) * RG + rg) * TILES + t) * MT * 64 + m * 64 + lane] = acc[t][m];
    }
  }
  __syncthreads();
  if (kg != 0 || !active) return;
#pragma unroll
  for (int v = 1; v < KG; ++v) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[t][m] += red[(((v - 1) * RG + rg) * TILES + t) * MT * 64 + m * 64 + lane];
    }
  }
  const int n = n0 + 4 * g;   // this lane's four columns of rows 16 m + r
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = 16 * m + r;
    if (row >= M) continue;
    if (nsplit > 1) {
      const int64_t cols = (int64_t)TILES * N;
      float* p = ws + ((int64_t)piece * MAX_M + row) * cols + n;
#pragma unroll
      for (int t = 0; t < TILES; ++t) *(f32x4*)(p + (int64_t)t * N) = acc[t][m];
      continue;
    }
    f32x4 o = acc[0][m];
    if (SWIGLU) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = silu_mul(acc[0][m][j], acc[TILES - 1][m][j]);
    }
    const st_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
    *(st_u32x2*)(y + (int64_t)row * ldy + n) = out;
  }
}

template <bool SWIGLU, int MT>
__global__ __launch_bounds__(THREADS) void gemm_stream_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                              const bf16_t* __restrict__ w, int64_t ldw,
                                                              bf16_t* __restrict__ y, int64_t ldy,
                                                              float* __restrict__ ws, int M, int N, int K, int per,
                                                              int nsplit) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XBUF_BYTES];
  // wave-uniform: both sides walk the same chunks and meet at the same number of barriers
  if ((int)(blockIdx.x * WG_N + (threadIdx.x >> 6) % RG * TILE_N) < N)
    stream_wave<SWIGLU, MT, true>(smem, x, ldx, w, ldw, y, ldy, ws, M, N, K, per, nsplit);
  else
    stream_wave<SWIGLU, MT, false>(smem, x, ldx, w, ldw, y, ldy, ws, M, N, K, per, nsplit);
}

// The pieces of a split launch in piece order: one thread per (row, four columns).
template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemm_stream_merge_kernel(const float* __restrict__ ws, bf16_t* __restrict__ y,
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
  const st_u32x2 out = {pack2(o[0], o[1]), pack2(o[2], o[3])};
  *(st_u32x2*)(y + (int64_t)m * ldy + n) = out;
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
  const int nsplit = split(N, K), per = piece_chunks(N, K);
  const dim3 grid(workgroups(N), nsplit), block(THREADS);
  switch ((M + 15) / 16) {   // the plan above is (N, K)'s; M chooses only how many tiles of x a W fragment feeds
    case 2:
      hipLaunchKernelGGL((gemm_stream_kernel<SWIGLU, 2>), grid, block, 0, stream, x, ldx, w, ldw, y, ldy, ws, M, N, K,
                         per, nsplit);
      break;
    case 3:
      hipLaunchKernelGGL((gemm_stream_kernel<SWIGLU, 3>), grid, block, 0, stream, x, ldx, w, ldw, y, ldy, ws, M, N, K,
                         per, nsplit);
      break;
    default:
      hipLaunchKernelGGL((gemm_stream_kernel<SWIGLU, 4>), grid, block, 0, stream, x, ldx, w, ldw, y, ldy, ws, M, N, K,
                         per, nsplit);
  }
  int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit == 1) return rc;
  const int64_t units = (int64_t)M * (N / 4);
  hipLaunchKernelGGL((gemm_stream_merge_kernel<SWIGLU>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream,
                     (const float*)ws, y, ldy, M, N, nsplit);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int toa_gemm_stream(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, bf16_t* y, int64_t ldy,
                               int M, int N, int K, float* ws, hipStream_t stream) {
  return launch<false>(x, ldx, w, ldw, y, ldy, M, N, K, ws, stream);
}

extern "C" int toa_gemm_stream_swiglu(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, bf16_t* s,
                                      int64_t lds, int M, int F, int K, float* ws, hipStream_t stream) {
  return launch<true>(x, ldx, w, ldw, s, lds, M, F, K, ws, stream);
}

// form: 0 plain, 1 SwiGLU (N = F).  0 = taken, else the first condition that fails; toa_gemm_stream_why names it.
extern "C" int toa_gemm_stream_check(int form, const void* x, const void* w, const void* y, const void* ws,
                                     int64_t ldx, int64_t ldw, int64_t ldy, int64_t w_rows, int M, int N, int K) {
  Operands o = {};
  o.X = (uintptr_t)x, o.W = (uintptr_t)w, o.Y = (uintptr_t)y, o.WS = (uintptr_t)ws;
  o.ldx = ldx, o.ldw = ldw, o.ldy = ldy, o.w_rows = w_rows, o.M = M, o.N = N, o.K = K;
  return (int)check(form, o);
}
extern "C" const char* toa_gemm_stream_why(int reason) { return why(reason); }
// bytes of fp32 workspace of the plain form (N, K) / the SwiGLU form (F, K); 0: no split, ws is not read
extern "C" int64_t toa_gemm_stream_ws_bytes(int N, int K) { return ws_bytes(F_PLAIN, N, K); }
extern "C" int64_t toa_gemm_stream_swiglu_ws_bytes(int F, int K) { return ws_bytes(F_SWIGLU, F, K); }
// the plan, for tests and the benchmark: K pieces across workgroups, chunks of KC columns per piece
extern "C" int toa_gemm_stream_split(int N, int K) { return N > 0 && K > 0 ? split(N, K) : 0; }
extern "C" int toa_gemm_stream_piece_chunks(int N, int K) { return N > 0 && K > 0 ? piece_chunks(N, K) : 0; }
// the constants the tests' shapes are named from: 0 KC, 1 KG, 2 SPC, 3 KSTEP, 4 WG_N, 5 MIN_CHUNKS, 6 MAX_M
extern "C" int toa_gemm_stream_constant(int which) {
  constexpr int v[] = {KC, KG, SPC, KSTEP, WG_N, MIN_CHUNKS, MAX_M};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : 0;
}
