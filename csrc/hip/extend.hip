// KV-cache extend for the Llama stack (gfx950): T new tokens per batch row, at
// per-row start positions, against the cached keys plus the chunk's own.
// T = 1 from a filled cache is a decode step, T = P from an empty cache a
// prefill; everything in between is chunked prefill and continuation.
//
// Cache layout (kv_cache.h): K and V [B, Hkv, C, D] bf16, K stored rotated.
//
//   toa_extend_rope_append  qkv rows of the T tokens -> rotated q [B, T, Hq, D],
//                           rotated k and v into slots start[b] + t, t < count[b]
//                           (kv_rope_append_kernel, kv_cache.hip)
//   toa_attn_extend         query (b, t, h) against keys 0 .. start[b] + t of its
//                           KV head (the append ran first: its own key is there),
//                           split over keys: fp32 partials (max, normaliser,
//                           unnormalised O) per (row, split) into a workspace,
//                           then the merge kernel (kv_split_merge_kernel,
//                           kv_cache.hip) writes bf16 [B, T, Hq, D].
//
// With T tokens a KV head has T G query rows (G = Hq / Hkv), so both products
// run on the MFMA (v_mfma_f32_16x16x32_bf16), fp32 scores, softmax and
// accumulators.  The orientation is the training forward's (attention.hip):
//   S^T[key][row] = K . Q^T    A = K fragment, B = Q fragment: a lane owns one
//                              query row (column lane & 15) and 4 keys of every
//                              16; row max and sum are lane-local plus two
//                              shuffles, the rescale factor is per lane
//   O^T[d][row]  += V^T . P^T  the S^T accumulators, rounded to bf16, are the B
//                              operand as they stand; V^T comes out of the
//                              key-major LDS image by ds_read_b64_tr_b16
// (docs/kernels.md, "Extending the cache").
//
// No float atomics, and every sum runs in a fixed order: at a fixed split_keys
// the bits of one query token's output depend on its q row, keys and values
// 0 .. pos of its cache row, pos and split_keys only -- not on T, the token's
// index in the call, count, max_len or the batch.  Three things carry that:
// key blocks aligned to absolute key indices, fully masked blocks that are
// exact no-ops, and a merge over the splits at or below pos, in order.
#include "kv_cache.h"

typedef __attribute__((ext_vector_type(8))) short ext_s16x8;
typedef __attribute__((ext_vector_type(4))) short ext_s16x4;

#define EXT_KB 64  // keys per block: 4 S^T tiles of 16 keys, 2 k-steps of P V
#define EXT_QB 64  // query rows per workgroup: one 16-row MFMA tile per wave

// The largest limit among the query rows r0 .. r1 of a KV head (row r is token
// r / G): the tokens of a row are there up to the first that is not.
__device__ __forceinline__ int ext_span_limit(int st, int cnt, int r0, int r1, int G, int C, int max_len) {
  if (kv_token_last_key(st, cnt, r0 / G, C, max_len) < 0) return -1;
  return kv_token_last_key(st, cnt, min(min(r1 / G, cnt - 1), C - 1 - st), C, max_len);
}

extern "C" int toa_extend_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* start,
                                      const int* count, bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int T, int Hq,
                                      int Hkv, int D, int C, int tab_rows, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || B <= 0 || T < 1 || C <= 0 || tab_rows <= 0)
    return (int)hipErrorInvalidValue;
  return kv_launch_rope_append(qkv, cosv, sinv, start, count, q, kc, vc, B, T, Hq, Hkv, D, C, tab_rows, stream);
}

// ---------------------------------------------------------------------------
// Extend attention, split over keys.
//
// Grid (key split, KV head x query chunk, batch row), 256 threads = 4 waves.
// The query rows of one KV head are r = t G + g; a workgroup takes EXT_QB = 64
// of them, one 16-row MFMA tile per wave, so a tile may straddle tokens and
// every lane carries its own row's causal limit.  Key blocks of EXT_KB = 64
// keys start at multiples of 64 of the absolute key index; the workgroup
// stages one block of K and of V into LDS (global -> registers while the
// previous block is computed -> LDS), once for all its rows, and walks the
// blocks of its split up to the largest limit among its rows.  Rows of K / V at
// or beyond start + count -- slots that may hold anything -- are staged as
// zeros: a masked score never reaches a result through the select below, and a
// weight of exactly 0 times a zero (or a later token's finite) value adds an
// exact 0.
//
// LDS images: [64 keys][D bf16 + 16 B], rows of RS = 2 D + 16 bytes.  K is read
// row-wise (16 B per lane: key lane & 15, columns 32 s + 8 (lane >> 4) ...),
// V by ds_read_b64_tr_b16: the 16-lane group h reads the 4 keys 4 h .. 4 h + 3
// (of a 16-key tile) x 16 columns and leaves lane i with column i of those 4
// keys -- the k order in which the S^T accumulators hold P.
//
// Per (row, split) the partial goes to the workspace (kv_cache.h).
// A row writes its partial of a split only if the split starts at or below the
// row's limit; the merge kernel reads exactly those.
// ---------------------------------------------------------------------------
__device__ __forceinline__ ext_s16x4 ext_tr_read(const char* p) {
  typedef __attribute__((address_space(3))) ext_s16x4 lds_s16x4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}

template <int D>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, const int* __restrict__ start,
                                                          const int* __restrict__ count, float* __restrict__ ws_o,
                                                          float* __restrict__ ws_ml, int T, int Hq, int Hkv, int C,
                                                          int max_len, int split, int nsplit, int nchunk,
                                                          float scale_log2) {
  constexpr int RS = 2 * D + 16;          // bytes per LDS row
  constexpr int NCH = D / 8;              // 16-B chunks per key row
  constexpr int NL = EXT_KB * NCH / 256;  // chunks of K (and of V) per thread per block
  constexpr int NS = D / 32;              // k-steps of Q K^T
  constexpr int ND = D / 16;              // 16-row d tiles of O^T
  __shared__ __attribute__((aligned(16))) char ks[EXT_KB * RS];
  __shared__ __attribute__((aligned(16))) char vs[EXT_KB * RS];

  const int sp = blockIdx.x, b = blockIdx.z;
  const int kvh = blockIdx.y / nchunk, chunk = blockIdx.y % nchunk;
  const int G = Hq / Hkv, rows = T * G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, hg = lane >> 4;
  const int st = start[b], cnt = min(count[b], T);
  const int k0 = sp * split;

  // the workgroup's, the wave's and the lane's last key (-1: none)
  const int wg_r0 = chunk * EXT_QB, wv_r0 = wg_r0 + wave * 16;
  const int wg_lim = ext_span_limit(st, cnt, wg_r0, wg_r0 + EXT_QB - 1, G, C, max_len);
  if (wg_lim < k0) return;  // the whole workgroup: nothing to add, nothing written
  const int wv_lim = __builtin_amdgcn_readfirstlane(ext_span_limit(st, cnt, wv_r0, wv_r0 + 15, G, C, max_len));
  const int myr = wv_r0 + col;
  const int myt = myr / G, myg = myr % G;
  const int lim = myr < rows ? kv_token_last_key(st, cnt, myt, C, max_len) : -1;
  const int64_t qrow = ((int64_t)b * T + min(myt, T - 1)) * Hq + kvh * G + myg;

  // Q fragments (the B operand): Q[row][32 s + 8 hg .. + 7]
  ext_s16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    qf[s] = __builtin_bit_cast(ext_s16x8, lim >= 0 ? ld16(q + qrow * D + 32 * s + 8 * hg) : z);
  }

  f32x4 acc[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // rows of K / V that hold this row's keys: below start + count, the cache and max_len
  const int kvalid = min(min(st + cnt, C), max_len);
  const int kend = min(min(k0 + split, wg_lim + 1), kvalid);
  const bf16_t* kb = kc + ((int64_t)b * Hkv + kvh) * C * D;
  const bf16_t* vb = vc + ((int64_t)b * Hkv + kvh) * C * D;

  u32x4 stk[NL], stv[NL];
  auto gload = [&](int base) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = tid + 256 * i;
      const int key = base + e / NCH, c = e % NCH;
      const int64_t off = (int64_t)min(key, kvalid - 1) * D + c * 8;  // clamped: always inside the row's keys
      stk[i] = ld16(kb + off);
      stv[i] = ld16(vb + off);
    }
  };
  auto swrite = [&](int base) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = tid + 256 * i;
      const int kr = e / NCH, c = e % NCH;
      const bool in = base + kr < kvalid;
      const u32x4 z = {0u, 0u, 0u, 0u};
      *(u32x4*)(ks + kr * RS + c * 16) = in ? stk[i] : z;
      *(u32x4*)(vs + kr * RS + c * 16) = in ? stv[i] : z;
    }
  };

  // lane-constant LDS offsets
  const int kro = col * RS + hg * 16;                                             // + 16 kt RS + 64 s
  const int vro = (4 * hg + (col >> 2)) * RS + (col & 3) * 8;                     // + (32 ks2 [+ 16]) RS + 32 dt

  gload(k0);
  for (int base = k0; base < kend; base += EXT_KB) {
    __syncthreads();  // the previous block's reads are done
    swrite(base);
    __syncthreads();
    if (base + EXT_KB < kend) gload(base + EXT_KB);
    if (base > wv_lim) continue;  // wave-uniform: no row of this wave sees the block

    // ---- S^T = K Q^T: 4 tiles of 16 keys; sc[kt][j] is key base + 16 kt + 4 hg + j of row col
    f32x4 sc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const ext_s16x8 kf = __builtin_bit_cast(ext_s16x8, *(const u32x4*)(ks + kro + kt * 16 * RS + s * 64));
        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc[kt], 0, 0, 0);
      }
    }
    // ---- online softmax of the lane's row over the block: a masked score is -inf, its weight an explicit 0
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = base + 16 * kt + 4 * hg + j <= lim;
        sc[kt][j] = ok ? sc[kt][j] * scale_log2 : -INFINITY;
        mx = fmaxf(mx, sc[kt][j]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float mr = mn == -INFINITY ? 0.f : mn;
    const float alpha = mn == m ? 1.f : exp2_fast(m - mr);  // an unchanged maximum rescales by exactly 1
    uint32_t pk[4][2];
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const float p0 = sc[kt][j] == -INFINITY ? 0.f : exp2_fast(sc[kt][j] - mr);
        const float p1 = sc[kt][j + 1] == -INFINITY ? 0.f : exp2_fast(sc[kt][j + 1] - mr);
        const uint32_t w = pack2(p0, p1);  // P is bf16 only as the MFMA operand; the normaliser sums what V sees
        pk[kt][j >> 1] = w;
        ps += __uint_as_float(w << 16);
        ps += __uint_as_float(w & 0xffff0000u);
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int i = 0; i < ND; ++i) acc[i] *= alpha;
    // ---- O^T += V^T P^T: 2 k-steps of 32 keys; element j of the fragments is key 32 k2 + 16 (j >> 2) + 4 hg + (j & 3)
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      typedef __attribute__((ext_vector_type(4))) uint32_t u4;
      const u4 pw = {pk[2 * k2][0], pk[2 * k2][1], pk[2 * k2 + 1][0], pk[2 * k2 + 1][1]};
      const ext_s16x8 pf = __builtin_bit_cast(ext_s16x8, pw);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const ext_s16x4 lo = ext_tr_read(vs + vro + (32 * k2) * RS + 32 * dt);
        const ext_s16x4 hi = ext_tr_read(vs + vro + (32 * k2 + 16) * RS + 32 * dt);
        const ext_s16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[dt], 0, 0, 0);
      }
    }
  }

  // acc[dt][j] is O[row col][16 dt + 4 hg + j]
  if (lim >= k0) {
    const int64_t slot = (((int64_t)b * T + myt) * Hq + kvh * G + myg) * nsplit + sp;
    float* po = ws_o + slot * D + 4 * hg;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) *(f32x4*)(po + 16 * dt) = acc[dt];
    if (hg == 0) {
      ws_ml[slot * 2] = m;
      ws_ml[slot * 2 + 1] = l;
    }
  }
}

// q, o [B, T, Hq, D], kc / vc [B, Hkv, C, D] bf16; start, count [B] int32
// (device); ws: fp32, B T Hq nsplit (D + 2) floats with nsplit =
// ceil(max_len / split_keys), or 1 for split_keys 0 (one split over all keys).
// max_len: a host-side bound of start + count (1 .. C) that sizes the grid;
// keys at or beyond it are not attended.  split_keys: 0 or a power of two >= 64.
extern "C" int toa_attn_extend(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int* start,
                               const int* count, float* ws, bf16_t* o, int B, int T, int Hq, int Hkv, int C, int D,
                               int max_len, int split_keys, float scale, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return (int)hipErrorInvalidValue;
  if (split_keys != 0 && (split_keys < 64 || (split_keys & (split_keys - 1)) != 0)) return (int)hipErrorInvalidValue;
  if (B <= 0 || B > 65535 || T < 1 || C <= 0 || max_len < 1 || max_len > C) return (int)hipErrorInvalidValue;
  const int G = Hq / Hkv;
  const int64_t nchunk = ((int64_t)T * G + EXT_QB - 1) / EXT_QB;
  const int64_t gy = (int64_t)Hkv * nchunk;
  const int64_t mrows = (int64_t)B * T * Hq;
  if (gy > 65535 || mrows > 0x7fffffff) return (int)hipErrorInvalidValue;
  // split_keys 0: one split that no key index reaches the end of
  const int split = split_keys ? split_keys : 0x40000000;
  const int nsplit = split_keys ? (max_len + split_keys - 1) / split_keys : 1;
  if (nsplit > 65535) return (int)hipErrorInvalidValue;
  float* ws_o = ws;
  float* ws_ml = ws + mrows * nsplit * D;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid(nsplit, (unsigned)gy, B);
  if (D == 128)
    hipLaunchKernelGGL((attn_extend_kernel<128>), grid, dim3(256), 0, stream, q, kc, vc, start, count, ws_o, ws_ml, T,
                       Hq, Hkv, C, max_len, split, nsplit, (int)nchunk, scale_log2);
  else
    hipLaunchKernelGGL((attn_extend_kernel<64>), grid, dim3(256), 0, stream, q, kc, vc, start, count, ws_o, ws_ml, T,
                       Hq, Hkv, C, max_len, split, nsplit, (int)nchunk, scale_log2);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  return kv_launch_split_merge(ws_o, ws_ml, start, count, o, B, T, Hq, D, C, max_len, split, nsplit, stream);
}
