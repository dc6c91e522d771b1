// The two kernels that KV-cache decoding and extending share (gfx950): RoPE +
// append of new tokens, and the merge of a split attention's partials.  The
// entry points are toa_decode_* (decode.hip) and toa_extend_* (extend.hip);
// cache and workspace layouts are in kv_cache.h.
#include "kv_cache.h"

// ---------------------------------------------------------------------------
// RoPE at position start[b] + t, and append.  qkv: [B, T, (Hq + 2 Hkv) D],
// cos/sin: [tab_rows, D/2] fp32 (ops.llm.rope_tables), start / count: [B]
// int32, count == nullptr: every token is there (toa_decode_rope_append: T = 1,
// start is pos).  The rotation is rope_fwd_kernel's (llm.hip), expression for
// expression: the same input row at the same position gives the same q and k
// bits as the training path.  Work unit = one (row, token, qkv-head, 8-wide
// pair chunk).  A token with t >= count[b], or whose position is outside the
// cache or the table, writes nothing to the caches and a zero q row -- also
// when decoding, where KVCache never produces such a position.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_rope_append_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ cosv, const float* __restrict__ sinv,
    const int* __restrict__ start, const int* __restrict__ count, bf16_t* __restrict__ q, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, int B, int T, int Hq, int Hkv, int D, int C, int tab_rows) {
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
  bf16_t* dst = h < Hq ? q + (r * Hq + h) * D + c * 8 : kc + (((int64_t)b * Hkv + (h - Hq)) * C + s) * D + c * 8;
  st16(dst, o1);
  st16(dst + half, o2);
}

int kv_launch_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* start, const int* count,
                          bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int T, int Hq, int Hkv, int D, int C,
                          int tab_rows, hipStream_t stream) {
  const int64_t blocks = ((int64_t)B * T * (Hq + 2 * Hkv) * (D / 16) + 255) / 256;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_rope_append_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qkv, cosv, sinv, start,
                     count, q, kc, vc, B, T, Hq, Hkv, D, C, tab_rows);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Grid (token x query head, batch row), one thread per column: the row's
// splits that start at or below its last key -- the partials the main kernel
// wrote -- in index order.  A row without keys (a length of 0, a token that is
// not there) gets zeros.  A maximum of -inf is replaced by 0 before it is
// subtracted, as in part_merge.
// ---------------------------------------------------------------------------
__global__ void kv_split_merge_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                      const int* __restrict__ start, const int* __restrict__ count,
                                      bf16_t* __restrict__ o, int T, int Hq, int D, int C, int max_len, int split,
                                      int nsplit) {
  const int b = blockIdx.y, t = blockIdx.x / Hq, d = threadIdx.x;
  const int64_t row = (int64_t)b * gridDim.x + blockIdx.x;  // (b T + t) Hq + h
  const int lim = count ? kv_token_last_key(start[b], min(count[b], T), t, C, max_len)
                        : kv_last_key(start[b], C, max_len);
  const int ns = lim < 0 ? 0 : min(lim / split + 1, nsplit);
  const int64_t slot0 = row * nsplit;
  float M = -INFINITY;
  for (int i = 0; i < ns; ++i) M = fmaxf(M, ws_ml[(slot0 + i) * 2]);
  const float mr = M == -INFINITY ? 0.f : M;
  float L = 0.f, a = 0.f;
  for (int i = 0; i < ns; ++i) {
    const float w = exp2_fast(ws_ml[(slot0 + i) * 2] - mr);
    L += ws_ml[(slot0 + i) * 2 + 1] * w;
    a += ws_o[(slot0 + i) * D + d] * w;
  }
  o[row * D + d] = f2bf(L > 0.f ? a / L : 0.f);
}

int kv_launch_split_merge(const float* ws_o, const float* ws_ml, const int* start, const int* count, bf16_t* o, int B,
                          int T, int Hq, int D, int C, int max_len, int split, int nsplit, hipStream_t stream) {
  hipLaunchKernelGGL(kv_split_merge_kernel, dim3((unsigned)(T * Hq), B), dim3(D), 0, stream, ws_o, ws_ml, start,
                     count, o, T, Hq, D, C, max_len, split, nsplit);
  return (int)hipGetLastError();
}
