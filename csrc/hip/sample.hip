// Token sampling on the device (gfx950): temperature, top-k, top-p and min-p
// in one kernel, one workgroup per row of logits [B, V].
//
// The result is defined by integer arithmetic (tf_operator_amd/ops/sample.py is
// the normative reference, docs/kernels.md "Sampling" the prose):
//
//   x        a logit; NaN counts as -inf, -0 as +0.  key(x) is its order-
//            preserving 32-bit image, m the row maximum.
//   q(x)     2^32 where x == m (decided first), 0 where x == -inf, else
//            min(rint(2^32 * exp2((x - m) * (log2e / T))), 2^32 - 1) in fp32.
//            Every mass is a uint64 sum of q: exact, so no summation order
//            can change it (V <= 2^20).
//   order    key descending, index ascending among equal keys.  top-k and
//            top-p are prefixes of it, found by a radix select over the key
//            (8 bits per pass: 2 passes for bf16, 4 for fp32) with histograms
//            of counts and of mass; equal keys have equal q, so the ties at a
//            threshold are counted, then admitted in index order.
//   kept     the shorter prefix, less the tokens with q < ceil(min_p * 2^32).
//   draw     r = umul64hi(h64, Z_kept), h64 two mix32 chains over (seed,
//            stream id, position); the token is the first index whose
//            cumulative kept mass in index order exceeds r.
//
// A row's token is a pure function of (its logits, its parameters, seed, its
// stream id, its position).  No float atomics, no scratch, nothing read back;
// every loop runs a trip count fixed by V and the row's parameters.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int SAMPLE_THREADS = 1024;            // one workgroup per row
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr uint32_t KEY_NEG_INF = 0x007FFFFFu;   // key(-inf), the lowest key there is
constexpr uint32_t NO_INDEX = 0xFFFFFFFFu;
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t mix32(uint32_t h) {  // murmur3 finaliser, as in optim.hip
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// One 32-bit draw of (seed, stream id, position); c tells the two draws apart.
__device__ __forceinline__ uint32_t draw32(uint32_t seed, int64_t sid, uint32_t pos, uint32_t c) {
  const uint32_t a = mix32(seed + c);
  const uint32_t b = mix32((uint32_t)((uint64_t)sid >> 32) + a);
  return mix32(pos ^ mix32((uint32_t)sid ^ b));
}

// The logit's fp32 bits, canonical: NaN -> -inf, -0 -> +0.
template <int DT>
__device__ __forceinline__ uint32_t load_bits(const void* row, int i) {
  uint32_t u = DT == 0 ? (uint32_t)((const uint16_t*)row)[i] << 16 : ((const uint32_t*)row)[i];
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0xFF800000u;
  if (u == 0x80000000u) u = 0u;
  return u;
}

__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// q of a token below the maximum, saturated to 32 bits.
__device__ __forceinline__ uint32_t weight(uint32_t u, float m, float c) {
  if (u == 0xFF800000u) return 0u;
  const float w = __builtin_amdgcn_exp2f((__uint_as_float(u) - m) * c) * 4294967296.0f;
  return w < 4294967296.0f ? (uint32_t)rintf(w) : 0xFFFFFFFFu;
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += shfl_xor64(v, d);
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = shfl_xor64(v, d);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_scan(u64 v, int lane) {  // inclusive, lane 0 first
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = shfl_up64(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// Wave 0, after a histogram pass: the highest digit d with
// sum(val[d' > d]) < rem <= sum(val[d' >= d]), val the counts or the masses.
// sel = {d, sum of val above d, sum of mass above d}.  Lane l owns digits
// 255 - 4l .. 252 - 4l, so ascending lanes walk the digits downwards.
__device__ __forceinline__ void select_digit(const uint32_t* h_cnt, const u64* h_mass, bool by_mass, u64 rem, u64* sel,
                                             int lane) {
  u64 v[4], ms[4], sv = 0, sm = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = 255 - 4 * lane - j;
    ms[j] = h_mass[d];
    v[j] = by_mass ? ms[j] : (u64)h_cnt[d];
    sv += v[j];
    sm += ms[j];
  }
  u64 ev = wave_scan(sv, lane) - sv, em = wave_scan(sm, lane) - sm;
  if (ev < rem && rem <= ev + sv) {
    bool done = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!done && rem <= ev + v[j]) {
        sel[0] = (u64)(255 - 4 * lane - j);
        sel[1] = ev;
        sel[2] = em;
        done = true;
      }
      ev += v[j];
      em += ms[j];
    }
  }
}

template <int DT>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_kernel(
    const void* __restrict__ logits, int64_t ld, int V, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p, const float* __restrict__ min_p,
    const int64_t* __restrict__ stream_id, const int* __restrict__ position, uint32_t seed,
    int64_t* __restrict__ tokens, uint32_t* __restrict__ weights) {
  __shared__ uint32_t h_cnt[256];
  __shared__ u64 h_mass[256];
  __shared__ u64 w_max[SAMPLE_WAVES], w_tot[SAMPLE_WAVES], w_tie[SAMPLE_WAVES], w_kept[SAMPLE_WAVES];
  __shared__ uint32_t w_fin[SAMPLE_WAVES];
  __shared__ u64 sel[3];
  __shared__ uint32_t s_tie_idx, s_token;

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const void* x = (const char*)logits + (int64_t)row * ld * (DT == 0 ? 2 : 4);
  // wave wv owns the contiguous indices lo .. hi-1, walked 64 at a time
  const int seg = (V + SAMPLE_WAVES - 1) / SAMPLE_WAVES;
  const int lo = min(wv * seg, V), hi = min(lo + seg, V);
  const int steps = (seg + 63) / 64;
  constexpr int NPASS = DT == 0 ? 2 : 4;

  if (tid == 0) {
    sel[0] = sel[1] = sel[2] = 0;
    s_tie_idx = NO_INDEX;
  }

  // ---- the maximum, its lowest index, and whether any logit is finite
  u64 best = 0;
  uint32_t fin = 0;
  for (int s = 0; s < steps; ++s) {
    const int i = lo + s * 64 + lane;
    if (i < hi) {
      const uint32_t u = load_bits<DT>(x, i);
      const u64 pk = ((u64)key_of(u) << 32) | (uint32_t)~(uint32_t)i;
      best = pk > best ? pk : best;
      fin |= (u & 0x7F800000u) != 0x7F800000u;
    }
  }
  best = wave_max(best);
  fin = __any(fin) ? 1u : 0u;
  if (lane == 0) {
    w_max[wv] = best;
    w_fin[wv] = fin;
  }
  __syncthreads();
  best = 0;
  fin = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    best = w_max[w] > best ? w_max[w] : best;
    fin |= w_fin[w];
  }
  const uint32_t kmax = (uint32_t)(best >> 32), amax = ~(uint32_t)best;
  const float m = __uint_as_float(bits_of(kmax));
  const float T = temperature[row];
  const float c = 1.44269504f / T;
  if (tid == 0) s_token = amax;

  auto q_sat = [&](uint32_t u) -> uint32_t { return key_of(u) == kmax ? 0xFFFFFFFFu : weight(u, m, c); };
  auto q_of = [&](uint32_t u) -> u64 { return key_of(u) == kmax ? (1ull << 32) : (u64)weight(u, m, c); };

  if (weights != nullptr) {
    uint32_t* wrow = weights + (int64_t)row * V;
    for (int s = 0; s < steps; ++s) {
      const int i = lo + s * 64 + lane;
      if (i < hi) wrow[i] = q_sat(load_bits<DT>(x, i));
    }
  }
  if (!fin || !(T > 0.0f)) {  // no finite logit: token 0; temperature 0: the argmax
    if (tid == 0) tokens[row] = fin ? (int64_t)amax : 0;
    return;
  }

  // One histogram pass of the radix select: counts and mass per digit of the
  // keys that agree with `pref` above the digit.
  auto hist_pass = [&](uint32_t pref, int p, bool with_cnt) {
    const int shift = 24 - 8 * p;
    const uint32_t himask = p == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    if (tid < 256) {
      h_cnt[tid] = 0;
      h_mass[tid] = 0;
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      const int i = lo + s * 64 + lane;
      if (i < hi) {
        const uint32_t u = load_bits<DT>(x, i), key = key_of(u);
        if (((key ^ pref) & himask) == 0) {
          const int d = (key >> shift) & 255;
          if (with_cnt) atomicAdd(&h_cnt[d], 1u);
          const u64 q = q_of(u);
          if (q) atomicAdd(&h_mass[d], q);
        }
      }
    }
    __syncthreads();
  };
  // bf16: the 16 bits the passes did not visit follow from the sign
  auto whole_key = [&](uint32_t pref) -> uint32_t {
    return DT == 0 ? (pref | ((pref & 0x80000000u) ? 0u : 0xFFFFu)) : pref;
  };

  bool all = true;          // the kept prefix is the whole row
  uint32_t kst = 0;         // else: keys above kst, and the first ntie tokens of key kst
  u64 ntie = 0, zk = 0;
  const int k = top_k[row];
  const float p_top = top_p[row];
  const bool k_on = k > 0 && k < V, p_on = p_top < 1.0f;

  if (k_on) {
    uint32_t pref = 0;
    u64 rem = (u64)k, mass_gt = 0;
    for (int p = 0; p < NPASS; ++p) {
      hist_pass(pref, p, true);
      if (wv == 0) select_digit(h_cnt, h_mass, false, rem, sel, lane);
      __syncthreads();
      pref |= (uint32_t)sel[0] << (24 - 8 * p);
      rem -= sel[1];
      mass_gt += sel[2];
    }
    kst = whole_key(pref);
    ntie = rem;
    all = false;
    zk = mass_gt + rem * q_of(bits_of(kst));
  } else if (p_on) {  // the mass of the whole row
    u64 z = 0;
    for (int s = 0; s < steps; ++s) {
      const int i = lo + s * 64 + lane;
      if (i < hi) z += q_of(load_bits<DT>(x, i));
    }
    z = wave_sum(z);
    if (lane == 0) w_tot[wv] = z;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) zk += w_tot[w];
  }

  if (p_on) {
    // t = max(1, ceil(P * zk / 2^32)), P = floor(p * 2^32)
    const u64 P = (u64)floorf(fmaxf(p_top, 0.0f) * 4294967296.0f);
    const u64 plo = P * zk, phi = __umul64hi(P, zk);
    const u64 slo = plo + 0xFFFFFFFFull;
    const u64 shi = phi + (slo < plo ? 1ull : 0ull);
    u64 rem = (shi << 32) | (slo >> 32);
    rem = rem < 1 ? 1 : rem;
    uint32_t pref = 0;
    for (int p = 0; p < NPASS; ++p) {
      hist_pass(pref, p, false);
      if (wv == 0) select_digit(h_cnt, h_mass, true, rem, sel, lane);
      __syncthreads();
      pref |= (uint32_t)sel[0] << (24 - 8 * p);
      rem -= sel[1];
    }
    kst = whole_key(pref);
    u64 qk = q_of(bits_of(kst));
    qk = qk < 1 ? 1 : qk;
    ntie = (rem + qk - 1) / qk;
    all = false;
  }

  // ---- the index of the ntie-th token of key kst: ties enter in index order
  uint32_t tie_idx = NO_INDEX;
  if (!all) {
    uint32_t cnt = 0;
    for (int s = 0; s < steps; ++s) {
      const int i = lo + s * 64 + lane;
      const bool f = i < hi && key_of(load_bits<DT>(x, i)) == kst;
      cnt += __popcll(__ballot(f));
    }
    if (lane == 0) w_tie[wv] = cnt;
    __syncthreads();
    u64 carry = 0;
    for (int w = 0; w < SAMPLE_WAVES; ++w) carry += w < wv ? w_tie[w] : 0;
    if (carry < ntie && ntie <= carry + cnt) {  // this wave holds it
      for (int s = 0; s < steps; ++s) {
        const int i = lo + s * 64 + lane;
        const bool f = i < hi && key_of(load_bits<DT>(x, i)) == kst;
        const u64 mask = __ballot(f);
        const u64 upto = carry + __popcll(mask & (~0ull >> (63 - lane)));
        if (f && upto == ntie) s_tie_idx = (uint32_t)i;
        carry += __popcll(mask);
      }
    }
    __syncthreads();
    tie_idx = s_tie_idx;
  }

  // ---- the kept mass per wave, the draw, and the scan in index order
  const float mp = min_p[row];
  uint32_t minq = 0;
  if (mp > 0.0f) minq = mp < 1.0f ? (uint32_t)ceilf(mp * 4294967296.0f) : 0xFFFFFFFFu;
  auto kept_q = [&](int i) -> u64 {
    if (i >= hi) return 0;
    const uint32_t u = load_bits<DT>(x, i), key = key_of(u);
    const bool in = all || key > kst || (key == kst && (uint32_t)i <= tie_idx);
    return in && q_sat(u) >= minq ? q_of(u) : 0;
  };
  u64 mine = 0;
  for (int s = 0; s < steps; ++s) mine += kept_q(lo + s * 64 + lane);
  mine = wave_sum(mine);
  if (lane == 0) w_kept[wv] = mine;
  __syncthreads();
  u64 z = 0, carry = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    carry += w < wv ? w_kept[w] : 0;
    z += w_kept[w];
  }
  const int64_t sid = stream_id[row];
  const uint32_t pos = (uint32_t)position[row];
  const u64 h64 = ((u64)draw32(seed, sid, pos, 0x9E3779B9u) << 32) | draw32(seed, sid, pos, 0x7F4A7C15u);
  const u64 r = __umul64hi(h64, z);
  if (carry <= r && r < carry + mine) {  // this wave holds the token
    for (int s = 0; s < steps; ++s) {
      const int i = lo + s * 64 + lane;
      const u64 v = kept_q(i);
      const u64 inc = carry + wave_scan(v, lane);
      if (v && inc - v <= r && r < inc) s_token = (uint32_t)i;
      carry = shfl64(inc, 63);
    }
  }
  __syncthreads();
  if (tid == 0) tokens[row] = (int64_t)s_token;
}

}  // namespace

// logits [B, V] bf16 (dtype 0) or fp32 (1), ld elements between rows;
// temperature / top_p / min_p fp32 [B], top_k int32 [B], stream_id int64 [B],
// position int32 [B]; tokens int64 [B]; weights uint32 [B, V] or null (each
// token's q, saturated at 2^32 - 1: the tests' view of the float stage).
extern "C" int toa_sample_tokens(int dtype, const void* logits, int64_t ld, int B, int V, const float* temperature,
                                 const int* top_k, const float* top_p, const float* min_p, const int64_t* stream_id,
                                 const int* position, uint32_t seed, int64_t* tokens, uint32_t* weights,
                                 hipStream_t stream) {
  if (B < 1 || V < 1 || V > (1 << 20) || ld < V || (dtype != 0 && dtype != 1)) return (int)hipErrorInvalidValue;
  if (!logits || !temperature || !top_k || !top_p || !min_p || !stream_id || !position || !tokens)
    return (int)hipErrorInvalidValue;
  if (dtype == 0)
    hipLaunchKernelGGL(sample_tokens_kernel<0>, dim3(B), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, temperature,
                       top_k, top_p, min_p, stream_id, position, seed, tokens, weights);
  else
    hipLaunchKernelGGL(sample_tokens_kernel<1>, dim3(B), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, temperature,
                       top_k, top_p, min_p, stream_id, position, seed, tokens, weights);
  return (int)hipGetLastError();
}
