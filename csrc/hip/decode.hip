// KV-cache decoding for the Llama stack (gfx950): one new token per batch row
// against a cache of past keys.
//
// Cache layout (kv_cache.h): K and V are [B, Hkv, C, D] bf16 per layer, the
// keys of one KV head contiguous -- what a decode step streams.
//
//   toa_decode_rope_append  qkv row of the new token -> rotated q [B, Hq, D],
//                           rotated k and v into slot pos[b] of the caches
//                           (kv_rope_append_kernel, kv_cache.hip)
//   toa_attn_decode         q against keys 0 .. len[b]-1, split over keys:
//                           fp32 partials (max, normaliser, unnormalised O)
//                           per split into a workspace, then the merge kernel
//                           (kv_split_merge_kernel, kv_cache.hip) writes bf16
//                           [B, Hq, D].  No float atomics; every sum runs in a
//                           fixed order, so a row's bits depend on that row's
//                           q, cache, len and split_keys only.
//
// The dot products run on the VALU: a decode step reads each K/V byte once for
// at most 8 query rows (the heads of one GQA group), 1 FMA per byte and head,
// far below what the vector units issue while HBM delivers the bytes; an MFMA
// tile would be 8 rows of 16 or 32, idle for the rest, and wants K/V images in
// LDS that this kernel never needs (docs/kernels.md, "Decoding").
#include "kv_cache.h"

#include <algorithm>

// One token per row at position pos[b]: the shared kernel with T = 1 and no
// count.  A position outside the cache or the table writes nothing to the
// caches and a zero q row (KVCache never produces one).
extern "C" int toa_decode_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* pos,
                                      bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int Hq, int Hkv, int D, int C,
                                      int tab_rows, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || B <= 0 || C <= 0 || tab_rows <= 0)
    return (int)hipErrorInvalidValue;
  return kv_launch_rope_append(qkv, cosv, sinv, pos, nullptr, q, kc, vc, B, 1, Hq, Hkv, D, C, tab_rows, stream);
}

// ---------------------------------------------------------------------------
// Decode attention, split over keys.
//
// Grid (key split, KV head x head chunk, batch row), 256 threads.  A key row
// is D bf16 = LPK = D/8 lanes of 16 B; the NG = 256 / LPK lane groups of a
// workgroup each own every NG-th key of the split and run their own online
// softmax over them, for all GT query heads of the chunk at once (GT = the
// whole GQA group up to 8 heads: each K/V byte is loaded once for the group).
// A lane keeps its 8 columns of q (pre-scaled, fp32) and of the unnormalised
// output per head; the score's sum over the LPK lanes of a group is four (three)
// DPP adds, after which every lane of the group holds the same bits.
// Per iteration a lane has KU K loads and KU V loads of 16 B in flight.
// At the end the groups' (m, l, acc) merge in a fixed order -- across the
// groups of a wave by shuffles, across the four waves through LDS -- and the
// split's partial goes to the workspace (kv_cache.h; a row is (b, h)).
// A split that starts at or beyond len[b] writes nothing; the merge kernel
// reads the splits below len[b] only.  Keys at or beyond len[b] are never
// loaded.  A maximum of -inf (no key seen yet) is replaced by 0 before it is
// subtracted, as in lse_merge and the cross-entropy forward.
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
  return v + __int_as_float(o);
}

// Sum over the LPK (8 or 16) adjacent lanes of a key group, left in every one of them.
template <int LPK>
__device__ __forceinline__ float group_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the 8
  if (LPK == 16) v = dpp_add<0x140>(v);  // row_mirror: the other half of the 16
  return v;
}

// (m, l, acc) <- (m, l, acc) (+) (m2, l2, acc2), the -inf maximum guarded
__device__ __forceinline__ void part_merge(float& m, float& l, float* acc, float m2, float l2, const float* acc2) {
  const float mn = fmaxf(m, m2);
  const float mr = mn == -INFINITY ? 0.f : mn;
  const float a1 = exp2_fast(m - mr), a2 = exp2_fast(m2 - mr);
  l = l * a1 + l2 * a2;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = acc[j] * a1 + acc2[j] * a2;
  m = mn;
}

#define TOA_DECODE_KU 4

template <int D, int GT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, const int* __restrict__ lens,
                                                          float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq,
                                                          int Hkv, int C, int split, int nsplit, float scale_log2) {
  constexpr int LPK = D / 8;     // lanes per key row
  constexpr int NG = 256 / LPK;  // key groups per workgroup
  constexpr int KU = TOA_DECODE_KU;
  __shared__ float red_o[4][GT][D];
  __shared__ float red_ml[4][GT][2];

  const int sp = blockIdx.x, b = blockIdx.z;
  const int G = Hq / Hkv, chunks = G / GT;
  const int kvh = blockIdx.y / chunks, h0 = kvh * G + (blockIdx.y % chunks) * GT;
  const int len = min(max(lens[b], 0), C);
  const int k0 = sp * split;
  if (k0 >= len) return;  // the whole workgroup: nothing to add, nothing written
  const int k1 = min(k0 + split, len);
  const int tid = threadIdx.x, c = tid % LPK, grp = tid / LPK;

  float qf[GT][8], acc[GT][8], m[GT], l[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    unpack8(ld16(q + ((int64_t)b * Hq + h0 + g) * D + c * 8), qf[g]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qf[g][j] *= scale_log2;
      acc[g][j] = 0.f;
    }
    m[g] = -INFINITY;
    l[g] = 0.f;
  }
  const bf16_t* kb = kc + ((int64_t)b * Hkv + kvh) * C * D + c * 8;
  const bf16_t* vb = vc + ((int64_t)b * Hkv + kvh) * C * D + c * 8;

  for (int base = k0; base < k1; base += NG * KU) {
    u32x4 kr[KU], vr[KU];
    bool ok[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int key = base + u * NG + grp;
      ok[u] = key < k1;
      const u32x4 z = {0u, 0u, 0u, 0u};
      kr[u] = ok[u] ? ld16(kb + (int64_t)key * D) : z;
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int key = base + u * NG + grp;
      const u32x4 z = {0u, 0u, 0u, 0u};
      vr[u] = ok[u] ? ld16(vb + (int64_t)key * D) : z;
    }
    float s[GT][KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += qf[g][j] * kf[j];
        d = group_sum<LPK>(d);
        s[g][u] = ok[u] ? d : -INFINITY;
      }
    }
    float p[GT][KU];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < KU; ++u) mn = fmaxf(mn, s[g][u]);
      const float mr = mn == -INFINITY ? 0.f : mn;
      const float alpha = exp2_fast(m[g] - mr);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        p[g][u] = ok[u] ? exp2_fast(s[g][u] - mr) : 0.f;
        ps += p[g][u];
      }
      l[g] = l[g] * alpha + ps;
      m[g] = mn;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      float vf[8];
      unpack8(vr[u], vf);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] += p[g][u] * vf[j];
      }
    }
  }

  // the groups of a wave, lanes LPK, 2 LPK, ... apart: a binary tree whose root is group 0 (only the lower
  // partner of each pair is read again, so every merge that counts is (lower, upper))
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
      float a2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a2[j] = __shfl_xor(acc[g][j], off, 64);
      part_merge(m[g], l[g], acc[g], m2, l2, a2);
    }
  }
  const int lane = tid & 63, wid = tid >> 6;
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red_o[wid][g][lane * 8 + j] = acc[g][j];
      if (lane == 0) {
        red_ml[wid][g][0] = m[g];
        red_ml[wid][g][1] = l[g];
      }
    }
  }
  __syncthreads();
  if (tid < GT * LPK) {
    const int g = tid / LPK, cc = tid % LPK;
    float M = red_ml[0][g][0], L = red_ml[0][g][1], a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = red_o[0][g][cc * 8 + j];
    for (int w = 1; w < 4; ++w) part_merge(M, L, a, red_ml[w][g][0], red_ml[w][g][1], &red_o[w][g][cc * 8]);
    const int64_t slot = ((int64_t)b * Hq + h0 + g) * nsplit + sp;
    float* po = ws_o + slot * D + cc * 8;
    const f32x4 lo = {a[0], a[1], a[2], a[3]}, hi = {a[4], a[5], a[6], a[7]};
    *(f32x4*)po = lo;
    *(f32x4*)(po + 4) = hi;
    if (cc == 0) {
      ws_ml[slot * 2] = M;
      ws_ml[slot * 2 + 1] = L;
    }
  }
}

template <int D>
static void launch_decode(int GT, dim3 grid, hipStream_t stream, const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                          const int* lens, float* ws_o, float* ws_ml, int Hq, int Hkv, int C, int split, int nsplit,
                          float scale_log2) {
#define TOA_DECODE_LAUNCH(G_)                                                                                       \
  hipLaunchKernelGGL((attn_decode_kernel<D, G_>), grid, dim3(256), 0, stream, q, kc, vc, lens, ws_o, ws_ml, Hq, Hkv, \
                     C, split, nsplit, scale_log2)
  if (GT == 8)
    TOA_DECODE_LAUNCH(8);
  else if (GT == 4)
    TOA_DECODE_LAUNCH(4);
  else if (GT == 2)
    TOA_DECODE_LAUNCH(2);
  else
    TOA_DECODE_LAUNCH(1);
#undef TOA_DECODE_LAUNCH
}

// q [B, Hq, D], kc / vc [B, Hkv, C, D] bf16; lens [B] int32 (device); ws: fp32,
// B Hq nsplit (D + 2) floats with nsplit = ceil(max_len / split_keys); o [B, Hq, D] bf16.
// max_len: a host-side bound of len[b] (1 .. C) that sizes the grid; keys at or
// beyond it are not attended.  split_keys: a power of two >= 64.
extern "C" int toa_attn_decode(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int* lens, float* ws,
                               bf16_t* o, int B, int Hq, int Hkv, int C, int D, int max_len, int split_keys,
                               float scale, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return (int)hipErrorInvalidValue;
  if (split_keys < 64 || (split_keys & (split_keys - 1)) != 0) return (int)hipErrorInvalidValue;
  if (B <= 0 || B > 65535 || C <= 0 || max_len < 1 || max_len > C) return (int)hipErrorInvalidValue;
  const int G = Hq / Hkv;
  int GT = 8;
  while (G % GT) GT >>= 1;  // the largest power of two <= 8 that divides the group
  const int64_t gy = (int64_t)Hkv * (G / GT);
  if (gy > 65535) return (int)hipErrorInvalidValue;
  const int nsplit = (max_len + split_keys - 1) / split_keys;
  float* ws_o = ws;
  float* ws_ml = ws + (int64_t)B * Hq * nsplit * D;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid(nsplit, (unsigned)gy, B);
  if (D == 128)
    launch_decode<128>(GT, grid, stream, q, kc, vc, lens, ws_o, ws_ml, Hq, Hkv, C, split_keys, nsplit, scale_log2);
  else
    launch_decode<64>(GT, grid, stream, q, kc, vc, lens, ws_o, ws_ml, Hq, Hkv, C, split_keys, nsplit, scale_log2);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  return kv_launch_split_merge(ws_o, ws_ml, lens, nullptr, o, B, 1, Hq, D, C, max_len, split_keys, nsplit, stream);
}
