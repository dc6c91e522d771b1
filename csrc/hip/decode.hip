// KV-cache decoding for the Llama stack (gfx950): one new token per batch row
// against a cache of past keys.
//
// Cache layout: K and V are [B, Hkv, C, D] bf16 per layer (C = capacity), K
// stored already rotated, so the keys of one KV head are contiguous -- what a
// decode step streams.
//
//   toa_decode_rope_append  qkv row of the new token -> rotated q [B, Hq, D],
//                           rotated k and v into slot pos[b] of the caches
//   toa_attn_decode         q against keys 0 .. len[b]-1, split over keys:
//                           fp32 partials (max, normaliser, unnormalised O)
//                           per split into a workspace, then a merge kernel
//                           writes bf16 [B, Hq, D].  No float atomics; every
//                           sum runs in a fixed order, so a row's bits depend
//                           on that row's q, cache, len and split_keys only.
//
// The dot products run on the VALU: a decode step reads each K/V byte once for
// at most 8 query rows (the heads of one GQA group), 1 FMA per byte and head,
// far below what the vector units issue while HBM delivers the bytes; an MFMA
// tile would be 8 rows of 16 or 32, idle for the rest, and wants K/V images in
// LDS that this kernel never needs (docs/kernels.md, "Decoding").
#include "toa_common.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// RoPE at a per-row position + append.  qkv: [B, (Hq + 2 Hkv) D], cos/sin:
// [tab_rows, D/2] fp32 (ops.llm.rope_tables), pos: [B] int32.  The rotation is
// rope_fwd_kernel's (llm.hip), expression for expression: the same input row
// at the same position gives the same q and k bits as the training path.
// Work unit = one (row, qkv-head, 8-wide pair chunk).  A row whose position is
// outside the cache or the table writes nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_rope_append_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ cosv, const float* __restrict__ sinv,
    const int* __restrict__ pos, bf16_t* __restrict__ q, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int B,
    int Hq, int Hkv, int D, int C, int tab_rows) {
  const int half = D / 2, cpd = half / 8;
  const int H3 = Hq + 2 * Hkv;
  const int64_t units = (int64_t)B * H3 * cpd;
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int c = u % cpd;
  const int64_t r = u / cpd;
  const int h = r % H3;
  const int b = r / H3;
  const int s = pos[b];
  if (s < 0 || s >= C || s >= tab_rows) return;
  const bf16_t* src = qkv + b * (int64_t)(H3 * D) + h * D + c * 8;
  u32x4 x1v = ld16(src), x2v = ld16(src + half);
  if (h >= Hq + Hkv) {  // V: as it is
    const int g = h - Hq - Hkv;
    bf16_t* dst = vc + (((int64_t)b * Hkv + g) * C + s) * D + c * 8;
    st16(dst, x1v);
    st16(dst + half, x2v);
    return;
  }
  float x1[8], x2[8], y1[8], y2[8];
  unpack8(x1v, x1);
  unpack8(x2v, x2);
  const float* cp = cosv + (int64_t)s * half + c * 8;
  const float* sp = sinv + (int64_t)s * half + c * 8;
  f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4);
  f32x4 s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
  float cs[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
  float sn[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    y1[j] = x1[j] * cs[j] - x2[j] * sn[j];
    y2[j] = x2[j] * cs[j] + x1[j] * sn[j];
  }
  u32x4 o1 = pack8(y1), o2 = pack8(y2);
  bf16_t* dst = h < Hq ? q + ((int64_t)b * Hq + h) * D + c * 8
                       : kc + (((int64_t)b * Hkv + (h - Hq)) * C + s) * D + c * 8;
  st16(dst, o1);
  st16(dst + half, o2);
}

extern "C" int toa_decode_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* pos,
                                      bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int Hq, int Hkv, int D, int C,
                                      int tab_rows, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || B <= 0 || C <= 0 || tab_rows <= 0)
    return (int)hipErrorInvalidValue;
  const int64_t units = (int64_t)B * (Hq + 2 * Hkv) * (D / 16);
  hipLaunchKernelGGL(decode_rope_append_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, qkv,
                     cosv, sinv, pos, q, kc, vc, B, Hq, Hkv, D, C, tab_rows);
  return (int)hipGetLastError();
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
// split's partial goes to the workspace:
//   ws_o  [B, Hq, nsplit, D] fp32 unnormalised output
//   ws_ml [B, Hq, nsplit, 2] fp32 running max (log2 domain), normaliser
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

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

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

// One workgroup per (query head, batch row), one thread per column: the
// row's non-empty splits in order.  len[b] == 0 gives a row of zeros.
__global__ void attn_decode_merge_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                         const int* __restrict__ lens, bf16_t* __restrict__ o, int Hq, int D, int C,
                                         int split, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int len = min(max(lens[b], 0), C);
  const int ns = min((len + split - 1) / split, nsplit);
  const int64_t slot0 = ((int64_t)b * Hq + h) * nsplit;
  float M = -INFINITY;
  for (int i = 0; i < ns; ++i) M = fmaxf(M, ws_ml[(slot0 + i) * 2]);
  const float mr = M == -INFINITY ? 0.f : M;
  float L = 0.f, a = 0.f;
  for (int i = 0; i < ns; ++i) {
    const float w = exp2_fast(ws_ml[(slot0 + i) * 2] - mr);
    L += ws_ml[(slot0 + i) * 2 + 1] * w;
    a += ws_o[(slot0 + i) * D + d] * w;
  }
  o[((int64_t)b * Hq + h) * D + d] = f2bf(L > 0.f ? a / L : 0.f);
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
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(Hq, B), dim3(D), 0, stream, (const float*)ws_o,
                     (const float*)ws_ml, lens, o, Hq, D, C, split_keys, nsplit);
  return (int)hipGetLastError();
}
