// The fp8 KV cache (gfx950): e4m3 keys and values with one power-of-two scale
// per (token, KV head), half the bytes a decode step streams and half the
// footprint.  Format, operands and constants: kv_cache_q8_shapes.h; the
// quantiser rule: e4m3_quant.h (the fp8 weights' rule on one D-wide row).
//
//   toa_decode_rope_append_q8  one token per row: rotated q, slot pos[b] of the cache
//   toa_extend_rope_append_q8  T tokens per row: slots start[b] + t, t < count[b]
//   toa_kv_quant_rows          rotated k and v [B, Hkv, P, D] bf16 -> slots 0 .. P - 1
//   toa_attn_decode_q8         q against keys 0 .. len[b] - 1 of the fp8 cache
//   (toa_attn_extend_q8: extend.hip's kernel with the e4m3 staging)
//
// K is quantised after the rotation and after its rounding to bf16, so a slot
// holds quantize(the bf16 row the bf16 cache would hold), byte * scale is that
// row's bf16 value wherever e4m3 holds it, and quantising a dequantised row
// again changes nothing.
//
// The decode kernel keeps toa_attn_decode's split over keys, workspace, merge
// kernel (kv_cache.hip) and fixed merge order; its data path is its own.  A
// lane loads 8 BYTES of a key row -- 8 columns, so a row is still D / 8 lanes
// and group_sum's DPP tree, the 8 q + 8 acc columns per head and the whole GQA
// group per byte carry over -- with KU = 8 rows of K and of V in flight, the
// bytes in flight of the bf16 kernel.  v_cvt_pk_f32_fp8 takes the bytes
// straight to fp32.  No element is scaled: k_scale[key] multiplies the score
// once per (key, head) after the group sum, v_scale[key] multiplies the weight
// p once per (key, head) before the accumulation; both are exact multiplies by
// powers of two, so every sum sees the bits it would see on dequantised
// values.  The normaliser sums the unscaled p.  A scale is one 4-byte load per
// key at the same address in the lanes of a group.  The softmax runs on KS = 4
// keys at a time, so the scores cost the registers they cost in the bf16
// kernel.  Keys at or beyond len[b] load neither bytes nor scales; a NaN scale
// at a valid key gives NaN, as a NaN bf16 key does.
#include "kv_cache.h"

#include "e4m3_quant.h"
#include "kv_cache_q8_shapes.h"

using namespace toa_kvq8;

typedef __attribute__((ext_vector_type(2))) uint32_t q8_u32x2;
typedef __attribute__((ext_vector_type(2))) float q8_f32x2;

namespace {

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t v) {
  return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true));
}

// The maximum over the 4, 8 or 16 adjacent lanes of a row, left in every one of them (group_sum's tree).
__device__ __forceinline__ uint32_t group_max(uint32_t v, int lanes) {
  v = dpp_max<0xB1>(v);                    // quad_perm [1, 0, 3, 2]
  v = dpp_max<0x4E>(v);                    // quad_perm [2, 3, 0, 1]
  if (lanes >= 8) v = dpp_max<0x141>(v);   // row_half_mirror
  if (lanes >= 16) v = dpp_max<0x140>(v);  // row_mirror
  return v;
}

__device__ __forceinline__ void st8(void* p, const uint32_t* w) {
  const q8_u32x2 v = {w[0], w[1]};
  *reinterpret_cast<q8_u32x2*>(p) = v;
}

// eight e4m3 bytes -> eight floats, exact
__device__ __forceinline__ void cvt8(const q8_u32x2 w, float* f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const q8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const q8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0], f[4 * i + 1] = lo[1], f[4 * i + 2] = hi[0], f[4 * i + 3] = hi[1];
  }
}

// ---------------------------------------------------------------------------
// RoPE at position start[b] + t, quantise, append: kv_rope_append_kernel
// (kv_cache.hip) with its work unit, its predicate and its rotation,
// expression for expression, so q has the bf16 path's bits and K the bits the
// bf16 cache would hold before they are quantised.  The D / 16 lanes of a head
// row are adjacent (4 or 8, aligned, all in the same branch): the largest
// magnitude of the row's bf16 bits is a DPP maximum over them, every lane
// derives the same exponent, stores its two 8-byte pieces, and lane 0 stores
// the scale.  A token that is not there writes a zero q row and nothing else.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void kv_rope_append_q8_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ cosv, const float* __restrict__ sinv,
    const int* __restrict__ start, const int* __restrict__ count, bf16_t* __restrict__ q, uint8_t* __restrict__ k8,
    uint8_t* __restrict__ v8, float* __restrict__ kscale, float* __restrict__ vscale, int B, int T, int Hq, int Hkv,
    int D, int C, int tab_rows) {
  const int half = D / 2, cpd = half / 8;
  const int H3 = Hq + 2 * Hkv;
  const int64_t units = (int64_t)B * T * H3 * cpd;
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int c = u % cpd;
  int64_t r = u / cpd;
  const int h = r % H3;
  r /= H3;  // b T + t
  const int t = r % T;
  const int b = r / T;
  const int st = start[b];
  const bool there =
      st >= 0 && (!count || t < count[b]) && st < C && t < C - st && st < tab_rows && t < tab_rows - st;
  if (!there) {
    if (h < Hq) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      bf16_t* dst = q + (r * Hq + h) * D + c * 8;
      st16(dst, z);
      st16(dst + half, z);
    }
    return;
  }
  const int s = st + t;
  const bf16_t* src = qkv + r * (int64_t)(H3 * D) + h * D + c * 8;
  u32x4 x1v = ld16(src), x2v = ld16(src + half);
  const bool isv = h >= Hq + Hkv;  // uniform over the row's lanes
  u32x4 o1 = x1v, o2 = x2v;        // V: as it is
  if (!isv) {
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
    o1 = pack8(y1), o2 = pack8(y2);
    if (h < Hq) {
      bf16_t* dst = q + (r * Hq + h) * D + c * 8;
      st16(dst, o1);
      st16(dst + half, o2);
      return;
    }
  }
  const int g = isv ? h - Hq - Hkv : h - Hq;
  const int64_t slot = ((int64_t)b * Hkv + g) * C + s;
  const e4m3_row_scale rs = e4m3_scale_of(group_max(amax_bits(amax_bits(0u, o1), o2), cpd));
  uint32_t w1[2], w2[2];
  e4m3_quant8(o1, rs.down, w1);
  e4m3_quant8(o2, rs.down, w2);
  uint8_t* dst = (isv ? v8 : k8) + slot * D + c * 8;
  st8(dst, w1);
  st8(dst + half, w2);
  if (c == 0) (isv ? vscale : kscale)[slot] = rs.scale;
}

// ---------------------------------------------------------------------------
// Whole-prompt prefill: rows of k and v [B Hkv, P, D] bf16 into slots
// 0 .. P - 1 of a cache whose rows of one (b, KV head) are C slots apart.
// Grid (row blocks, K | V): a row is D / 8 adjacent lanes of one 16-byte load
// and one 8-byte store each, 256 / (D / 8) = 16 or 32 rows per workgroup.
// Slots at or beyond P are not touched.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void kv_quant_rows_kernel(const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, uint8_t* __restrict__ k8,
                                                              uint8_t* __restrict__ v8, float* __restrict__ kscale,
                                                              float* __restrict__ vscale, int64_t rows, int P, int D,
                                                              int C) {
  const int lpr = D / COLS;
  const int64_t u = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
  const int64_t row = u / lpr;  // (b Hkv + g) P + p
  if (row >= rows) return;      // whole rows: BLOCK is a multiple of lpr
  const int c = (int)(u % lpr);
  const bool isv = blockIdx.y != 0;
  const u32x4 x = ld16((isv ? v : k) + row * D + c * COLS);
  const e4m3_row_scale rs = e4m3_scale_of(group_max(amax_bits(0u, x), lpr));
  uint32_t w[2];
  e4m3_quant8(x, rs.down, w);
  const int64_t slot = (row / P) * C + row % P;
  st8((isv ? v8 : k8) + slot * D + c * COLS, w);
  if (c == 0) (isv ? vscale : kscale)[slot] = rs.scale;
}

// ---------------------------------------------------------------------------
// Decode attention on the fp8 cache, split over keys.  Grid (key split, KV head
// x head chunk, batch row), 256 threads, as attn_decode_kernel (decode.hip):
// the NG = 256 / LPK lane groups each own every NG-th key of the split.  Per
// iteration a lane has KU = 8 loads of 8 bytes of K, as many of V and the 2 KU
// scales in flight, then runs the online softmax over them KS = 4 keys at a
// time.
// ---------------------------------------------------------------------------
template <int D, int GT>
__global__ __launch_bounds__(BLOCK) void attn_decode_q8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ k8, const uint8_t* __restrict__ v8,
    const float* __restrict__ kscale, const float* __restrict__ vscale, const int* __restrict__ lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq, int Hkv, int C, int split, int nsplit,
    float scale_log2) {
  constexpr int LPK = D / COLS;    // lanes per key row
  constexpr int NG = BLOCK / LPK;  // key groups per workgroup
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
  const int64_t head = ((int64_t)b * Hkv + kvh) * C;
  const uint8_t* kb = k8 + head * D + c * COLS;
  const uint8_t* vb = v8 + head * D + c * COLS;
  const float* ksb = kscale + head;
  const float* vsb = vscale + head;

  for (int base = k0; base < k1; base += NG * KU) {
    q8_u32x2 kr[KU], vr[KU];
    float ksc[KU], vsc[KU];
    bool ok[KU];
    const q8_u32x2 z = {0u, 0u};
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int key = base + u * NG + grp;
      ok[u] = key < k1;
      kr[u] = ok[u] ? *(const q8_u32x2*)(kb + (int64_t)key * D) : z;
      ksc[u] = ok[u] ? ksb[key] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int key = base + u * NG + grp;
      vr[u] = ok[u] ? *(const q8_u32x2*)(vb + (int64_t)key * D) : z;
      vsc[u] = ok[u] ? vsb[key] : 0.f;
    }
#pragma unroll
    for (int u0 = 0; u0 < KU; u0 += KS) {
      float s[GT][KS];
#pragma unroll
      for (int u = 0; u < KS; ++u) {
        float kf[8];
        cvt8(kr[u0 + u], kf);
#pragma unroll
        for (int g = 0; g < GT; ++g) {
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) d += qf[g][j] * kf[j];
          d = group_sum<LPK>(d) * ksc[u0 + u];
          s[g][u] = ok[u0 + u] ? d : -INFINITY;
        }
      }
      float p[GT][KS];
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        float mn = m[g];
#pragma unroll
        for (int u = 0; u < KS; ++u) mn = fmaxf(mn, s[g][u]);
        const float mr = mn == -INFINITY ? 0.f : mn;
        const float alpha = exp2_fast(m[g] - mr);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < KS; ++u) {
          p[g][u] = ok[u0 + u] ? exp2_fast(s[g][u] - mr) : 0.f;
          ps += p[g][u];
        }
        l[g] = l[g] * alpha + ps;
        m[g] = mn;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < KS; ++u) {
        float vf[8];
        cvt8(vr[u0 + u], vf);
#pragma unroll
        for (int g = 0; g < GT; ++g) {
          const float pv = p[g][u] * vsc[u0 + u];  // exact: a power of two
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[g][j] += pv * vf[j];
        }
      }
    }
  }

  // the groups of a wave, then the four waves through LDS: attn_decode_kernel's tree and order
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

template <int D, int GT>
void launch_decode_q8(dim3 grid, hipStream_t stream, const bf16_t* q, const uint8_t* k8, const uint8_t* v8,
                      const float* kscale, const float* vscale, const int* lens, float* ws_o, float* ws_ml, int Hq,
                      int Hkv, int C, int split, int nsplit, float scale_log2) {
  hipLaunchKernelGGL((attn_decode_q8_kernel<D, GT>), grid, dim3(BLOCK), 0, stream, q, k8, v8, kscale, vscale, lens,
                     ws_o, ws_ml, Hq, Hkv, C, split, nsplit, scale_log2);
}

Operands operands(const void* k8, const void* v8, const void* kscale, const void* vscale, int B, int T, int Hq,
                  int Hkv, int D, int C, int limit, int split_keys) {
  Operands o = {};
  o.K8 = (uintptr_t)k8, o.V8 = (uintptr_t)v8, o.KSCALE = (uintptr_t)kscale, o.VSCALE = (uintptr_t)vscale;
  o.B = B, o.T = T, o.Hq = Hq, o.Hkv = Hkv, o.D = D, o.C = C, o.limit = limit, o.split_keys = split_keys;
  return o;
}

int launch_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* start, const int* count,
                  bf16_t* q, uint8_t* k8, uint8_t* v8, float* kscale, float* vscale, int B, int T, int Hq, int Hkv,
                  int D, int C, int tab_rows, hipStream_t stream) {
  if (check(OP_APPEND, operands(k8, v8, kscale, vscale, B, T, Hq, Hkv, D, C, tab_rows, 0)) != R_OK)
    return (int)hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)B * T * (Hq + 2 * Hkv) * (D / 16) + BLOCK - 1) / BLOCK;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_rope_append_q8_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, qkv, cosv, sinv, start,
                     count, q, k8, v8, kscale, vscale, B, T, Hq, Hkv, D, C, tab_rows);
  return (int)hipGetLastError();
}

}  // namespace

// toa_decode_rope_append's arguments with the fp8 cache's four tensors in the two caches' place
extern "C" int toa_decode_rope_append_q8(const bf16_t* qkv, const float* cosv, const float* sinv, const int* pos,
                                         bf16_t* q, uint8_t* k8, uint8_t* v8, float* kscale, float* vscale, int B,
                                         int Hq, int Hkv, int D, int C, int tab_rows, hipStream_t stream) {
  return launch_append(qkv, cosv, sinv, pos, nullptr, q, k8, v8, kscale, vscale, B, 1, Hq, Hkv, D, C, tab_rows,
                       stream);
}

extern "C" int toa_extend_rope_append_q8(const bf16_t* qkv, const float* cosv, const float* sinv, const int* start,
                                         const int* count, bf16_t* q, uint8_t* k8, uint8_t* v8, float* kscale,
                                         float* vscale, int B, int T, int Hq, int Hkv, int D, int C, int tab_rows,
                                         hipStream_t stream) {
  if (!count) return (int)hipErrorInvalidValue;
  return launch_append(qkv, cosv, sinv, start, count, q, k8, v8, kscale, vscale, B, T, Hq, Hkv, D, C, tab_rows,
                       stream);
}

// k, v [B, Hkv, P, D] bf16, contiguous and 16-byte aligned -> slots 0 .. P - 1 of the cache [B, Hkv, C, D]
extern "C" int toa_kv_quant_rows(const bf16_t* k, const bf16_t* v, uint8_t* k8, uint8_t* v8, float* kscale,
                                 float* vscale, int B, int Hkv, int P, int D, int C, hipStream_t stream) {
  if (check(OP_FILL, operands(k8, v8, kscale, vscale, B, P, 0, Hkv, D, C, 0, 0)) != R_OK)
    return (int)hipErrorInvalidValue;
  if (!k || !v || (((uintptr_t)k | (uintptr_t)v) & 15)) return (int)hipErrorInvalidValue;
  const int64_t rows = (int64_t)B * Hkv * P;
  const int64_t blocks = (rows * (D / COLS) + BLOCK - 1) / BLOCK;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_quant_rows_kernel, dim3((unsigned)blocks, 2), dim3(BLOCK), 0, stream, k, v, k8, v8, kscale,
                     vscale, rows, P, D, C);
  return (int)hipGetLastError();
}

// toa_attn_decode's arguments (its workspace, max_len and split_keys too) on the fp8 cache
extern "C" int toa_attn_decode_q8(const bf16_t* q, const uint8_t* k8, const uint8_t* v8, const float* kscale,
                                  const float* vscale, const int* lens, float* ws, bf16_t* o, int B, int Hq, int Hkv,
                                  int C, int D, int max_len, int split_keys, float scale, hipStream_t stream) {
  if (check(OP_DECODE, operands(k8, v8, kscale, vscale, B, 1, Hq, Hkv, D, C, max_len, split_keys)) != R_OK)
    return (int)hipErrorInvalidValue;
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
#define TOA_Q8_LAUNCH(D_, G_)                                                                                      \
  launch_decode_q8<D_, G_>(grid, stream, q, k8, v8, kscale, vscale, lens, ws_o, ws_ml, Hq, Hkv, C, split_keys, nsplit, \
                           scale_log2)
#define TOA_Q8_LAUNCH_D(D_)                                                                  \
  (GT == 8 ? TOA_Q8_LAUNCH(D_, 8) : GT == 4 ? TOA_Q8_LAUNCH(D_, 4) : GT == 2 ? TOA_Q8_LAUNCH(D_, 2) \
                                                                             : TOA_Q8_LAUNCH(D_, 1))
  if (D == 128)
    TOA_Q8_LAUNCH_D(128);
  else
    TOA_Q8_LAUNCH_D(64);
#undef TOA_Q8_LAUNCH_D
#undef TOA_Q8_LAUNCH
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  return kv_launch_split_merge(ws_o, ws_ml, lens, nullptr, o, B, 1, Hq, D, C, max_len, split_keys, nsplit, stream);
}

// op: kv_cache_q8_shapes.h's Op (0 append, 1 fill, 2 decode, 3 extend).  0 = taken, else the first condition that
// fails; toa_kv_q8_why names it.
extern "C" int toa_kv_q8_check(int op, const void* k8, const void* v8, const void* kscale, const void* vscale, int B,
                               int T, int Hq, int Hkv, int D, int C, int limit, int split_keys) {
  return (int)check(op, operands(k8, v8, kscale, vscale, B, T, Hq, Hkv, D, C, limit, split_keys));
}
extern "C" const char* toa_kv_q8_why(int reason) { return why(reason); }
