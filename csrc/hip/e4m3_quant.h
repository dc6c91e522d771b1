// The power-of-two e4m3 quantiser rule that the fp8 weights (gemm_w8.hip) and
// the fp8 KV cache (kv_cache_q8.hip) share: one scale = 2^e per row, the row's
// elements as OCP e4m3 "fn" bytes (largest finite 448, 0x7f / 0xff NaN) of
// w * 2^-e.  The exponent rule is plain C++17 (the shape headers and Python's
// reference restate nothing else); the packing is device code.
#pragma once

#include <cstdint>

namespace toa_e4m3 {

// The exponent e of scale = 2^e from the magnitude bits (sign cleared) of a row's largest |w|, a finite bf16: the
// least e with amax <= 448 * 2^e = 1.75 * 2^(e + 8), clamped to -100 .. 100; 0 for a row of zeros.  With amax =
// m * 2^E, 1 <= m < 2: e = E - 8 if m <= 1.75 (mantissa field <= 0x60), else E - 7.  A subnormal amax has E = -127
// here and meets the clamp either way.
constexpr int E_MIN = -100, E_MAX = 100;
constexpr int scale_exponent(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int e = (int)(amax_bits >> 7) - 127 - 8 + ((amax_bits & 0x7f) > 0x60 ? 1 : 0);
  return e < E_MIN ? E_MIN : e > E_MAX ? E_MAX : e;
}

}  // namespace toa_e4m3

#if defined(__HIPCC__)
#include "toa_common.h"

// four floats -> four e4m3 bytes, round to nearest even.  Beyond the format (|f| > 448: only where the exponent met
// its clamp, or in a row with a non-finite element) the bytes are set here and not left to the conversion's mode:
// up to the tie at 464 the largest finite code 0x7e, past it and for NaN the NaN code 0x7f, the sign kept.
__device__ __forceinline__ uint32_t to_e4m3x4(const float* f) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
  uint32_t out = (uint32_t)w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!(fabsf(f[i]) <= 448.f)) {
      const uint32_t code = (fabsf(f[i]) <= 464.f ? 0x7eu : 0x7fu) | ((__float_as_uint(f[i]) >> 24) & 0x80u);
      out = (out & ~(0xffu << (8 * i))) | (code << (8 * i));
    }
  }
  return out;
}

// The largest magnitude of eight bf16 as an integer maximum of their bits: with the sign cleared, integer order is
// the order of |w|, and anything from 0x7f80 on is an infinity or a NaN.
__device__ __forceinline__ uint32_t amax_bits(uint32_t m, const u32x4 v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) m = max(m, max(v[i] & 0x7fffu, (v[i] >> 16) & 0x7fffu));
  return m;
}

// What a row's amax bits decide: the scale to store (NaN for a row with a non-finite element) and the factor
// 2^-e that makes the row's products exact.
struct e4m3_row_scale {
  float scale, down;
};
__device__ __forceinline__ e4m3_row_scale e4m3_scale_of(uint32_t amax) {
  const bool finite = amax < 0x7f80u;
  const int e = finite ? toa_e4m3::scale_exponent(amax) : 0;
  return {finite ? __uint_as_float((uint32_t)(127 + e) << 23) : __uint_as_float(0x7fc00000u),
          __uint_as_float((uint32_t)(127 - e) << 23)};
}

// eight bf16 (one 16-byte vector) times down -> eight e4m3 bytes (two words)
__device__ __forceinline__ void e4m3_quant8(const u32x4 v, float down, uint32_t* out) {
  float f[8];
  unpack8(v, f);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] *= down;
  out[0] = to_e4m3x4(f);
  out[1] = to_e4m3x4(f + 4);
}
#endif
