// Shared-prompt decoding for the Llama stack (gfx950): n samples per prompt on
// one copy of the prompt's keys and values.
//
// Caches (decode_shared_shapes.h): the prefix K, V [groups, Hkv, Cp, D] bf16,
// one row per prompt, written by the prefill and read-only afterwards; the
// suffix K, V [B, Hkv, Cs, D], B = groups x samples, row g samples + j holding
// what sample j of prompt g generated.  K is stored rotated, as in kv_cache.h.
//
//   toa_shared_rope_append   qkv row of the new token -> q and k rotated at the
//                            absolute position base[b / samples] + pos[b], k and
//                            v into slot pos[b] of the suffix cache
//   toa_attn_decode_shared   row b against prefix keys 0 .. plen[b / samples] - 1
//                            and suffix keys 0 .. slen[b] - 1, three launches:
//     prefix  attn_shared_prefix_kernel, below: the samples x G query rows of a
//             (prompt, KV head) against the prompt's keys on the MFMA, split
//             over keys, each K / V byte read once per prompt
//     suffix  attn_decode_kernel (decode.hip) on the suffix cache, its partials
//             left unmerged: keys differ per row, at most G rows share them
//     merge   shared_merge_kernel: a row's prefix partials, then its suffix
//             partials, in index order -> bf16 [B, Hq, D]
//
// No float atomics and every sum in a fixed order: a row's bits depend on its
// q, its prefix, its suffix, the two lengths and split_keys only -- not on
// samples, the row's place in its group, other groups or the grids' bounds.
// Keys at or beyond a length are never loaded into a result; a masked score is
// -inf and its weight an explicit 0; a maximum that can still be -inf is
// replaced by 0 before it is subtracted (docs/kernels.md, "Shared prompts").
#include "kv_cache.h"

#include "decode_shared_shapes.h"

using namespace toa_dshared;

typedef __attribute__((ext_vector_type(8))) short shr_s16x8;
typedef __attribute__((ext_vector_type(4))) short shr_s16x4;

// ---------------------------------------------------------------------------
// RoPE at base[b / samples] + pos[b], append at pos[b].  kv_rope_append_kernel
// (kv_cache.hip) with T = 1 and two numbers where it has one: the expressions
// are its own, so the same row at the same absolute position gives the q and k
// bits of toa_decode_rope_append.  A slot outside the suffix cache or a
// position outside the table writes no cache slot and a zero q row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shared_rope_append_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ cosv, const float* __restrict__ sinv,
    const int* __restrict__ base, const int* __restrict__ pos, bf16_t* __restrict__ q, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, int B, int samples, int Hq, int Hkv, int D, int C, int tab_rows) {
  const int half = D / 2, cpd = half / 8;
  const int H3 = Hq + 2 * Hkv;
  const int64_t units = (int64_t)B * H3 * cpd;
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int c = u % cpd;
  const int64_t r = u / cpd / H3;  // b
  const int h = (u / cpd) % H3;
  const int b = (int)r;
  const int slot = pos[b], bs = base[b / samples];
  const bool there = slot >= 0 && slot < C && bs >= 0 && bs < tab_rows && slot < tab_rows - bs;
  if (!there) {
    if (h < Hq) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      bf16_t* dst = q + (r * Hq + h) * D + c * 8;
      st16(dst, z);
      st16(dst + half, z);
    }
    return;
  }
  const int s = bs + slot;
  const bf16_t* src = qkv + r * (int64_t)(H3 * D) + h * D + c * 8;
  u32x4 x1v = ld16(src), x2v = ld16(src + half);
  if (h >= Hq + Hkv) {  // V: as it is
    const int g = h - Hq - Hkv;
    bf16_t* dst = vc + (((int64_t)b * Hkv + g) * C + slot) * D + c * 8;
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
  bf16_t* dst = h < Hq ? q + (r * Hq + h) * D + c * 8 : kc + (((int64_t)b * Hkv + (h - Hq)) * C + slot) * D + c * 8;
  st16(dst, o1);
  st16(dst + half, o2);
}

// qkv [B, (Hq + 2 Hkv) D], base [B / samples], pos [B] int32 (device); q [B, Hq, D]; kc / vc [B, Hkv, C, D]
extern "C" int toa_shared_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* base,
                                      const int* pos, bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int samples, int Hq,
                                      int Hkv, int D, int C, int tab_rows, hipStream_t stream) {
  Operands o = {};
  o.B = B, o.samples = samples, o.groups = samples >= 1 ? B / samples : 0, o.Hq = Hq, o.Hkv = Hkv, o.D = D;
  o.Cp = 1, o.Cs = C, o.split_keys = 64;
  if (check(o) != R_OK || tab_rows <= 0) return (int)hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)B * (Hq + 2 * Hkv) * (D / 16) + 255) / 256;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(shared_rope_append_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qkv, cosv, sinv, base,
                     pos, q, kc, vc, B, samples, Hq, Hkv, D, C, tab_rows);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// The prefix part, split over keys.
//
// Grid (key split, KV head x query chunk, prompt), 256 threads = 4 waves.  The
// query rows of one (prompt, KV head) are r = j G + g, sample j and head g of
// the group; a workgroup takes a chunk of 16 NT of them (NT <= 4 tiles) and
// EVERY wave holds the Q fragments and the fp32 accumulators of all NT tiles.
// The waves divide the keys instead: steps of KEYS = 32 keys, wave w taking the
// steps w, w + 4, ... of the split, so a K or V byte is read by exactly one
// wave of one workgroup per query chunk, and the main loop has no workgroup
// barrier.
//
// Orientation as in extend.hip: S^T[key][row] = K . Q^T, so a lane owns one
// query row (lane & 15) and 4 keys of every 16 (lane >> 4): row maximum and sum
// are lane-local plus two shuffles, and the S^T accumulators, rounded to bf16,
// are the B operand of O^T[d][row] += V^T . P^T as they stand.
//   K   global -> registers -> the A operand: lane (c, h) loads K[key 16 kt + c][32 s + 8 h ..], 16 B.
//       No LDS: nobody else wants these bytes.
//   V   global -> registers -> a wave-private LDS image [32 keys][D bf16 + 16 B] ->
//       ds_read_b64_tr_b16, which leaves lane i of a 16-lane group with column i
//       of the group's 4 keys: the k order in which the accumulators hold P.
//       One fragment serves all NT tiles.
// The next step's K and V are fetched into registers while this one computes.
// Loads are clamped to key plen - 1, always inside the prompt; V rows at or
// beyond plen are staged as zeros and their scores masked.
//
// At the end the waves' partials of each tile merge through LDS (the V images'
// space, after a barrier) in wave order, and wave 0 writes the split's partial
// (kv_cache.h's workspace layout; a row is (b, h), b = prompt x samples + j).
// A wave without keys holds (-inf, 0, 0), which the merge passes over exactly.
// A split that starts at or beyond plen writes nothing.
//
// Resources (D = 128, NT = 4, the largest): decode_shared_shapes.h and
// docs/kernels.md "Shared prompts"; no scratch.
// ---------------------------------------------------------------------------
__device__ __forceinline__ shr_s16x4 shr_tr_read(const char* p) {
  typedef __attribute__((address_space(3))) shr_s16x4 lds_s16x4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}

template <int D, int NT>
__global__ __launch_bounds__(BLOCK) void attn_shared_prefix_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kp, const bf16_t* __restrict__ vp,
    const int* __restrict__ plens, float* __restrict__ ws_o, float* __restrict__ ws_ml, int samples, int Hq, int Hkv,
    int Cp, int max_plen, int split, int nsplit, int nchunk, float scale_log2) {
  constexpr int RS = 2 * D + 16;       // bytes per row of the V image
  constexpr int NCH = D / 8;           // 16-B chunks per key row
  constexpr int NS = D / 32;           // k-steps of K Q^T
  constexpr int ND = D / 16;           // 16-row d tiles of O^T
  constexpr int NV = KEYS * NCH / 64;  // chunks of V per lane and step
  constexpr int IMG = KEYS * RS;       // bytes of a wave's V image = of a wave's partial of one tile
  constexpr int PW = 4 * ND + 2;       // fp32 words of a lane's partial of one tile
  static_assert(64 * PW * 4 == IMG, "a wave's partial of one tile fits its V image");
  __shared__ __attribute__((aligned(16))) char lds[WAVES * IMG];

  const int sp = blockIdx.x, grp = blockIdx.z;
  const int kvh = blockIdx.y / nchunk, chunk = blockIdx.y % nchunk;
  const int G = Hq / Hkv, R = samples * G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, hg = lane >> 4;
  const int plen = kv_last_key(plens[grp], Cp, max_plen) + 1;
  const int k0 = sp * split;
  if (k0 >= plen) return;  // the whole workgroup: nothing to add, nothing written
  const int kend = min(k0 + split, plen);

  // Q fragments (the B operand) of every tile: Q[row][32 s + 8 hg .. + 7]; rows beyond R are zeros
  shr_s16x8 qf[NT][NS];
  int64_t orow[NT];  // (b Hq + h) of the lane's row in tile t, -1 beyond R
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int r = (chunk * NT + t) * TILE + col;
    orow[t] = r < R ? ((int64_t)grp * samples + r / G) * Hq + kvh * G + r % G : -1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      qf[t][s] = __builtin_bit_cast(shr_s16x8, r < R ? ld16(q + orow[t] * D + 32 * s + 8 * hg) : z);
    }
  }
  f32x4 acc[NT][ND];
  float m[NT], l[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int i = 0; i < ND; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[t] = -INFINITY;
    l[t] = 0.f;
  }

  const int64_t head = ((int64_t)grp * Hkv + kvh) * Cp;
  const bf16_t* kb = kp + head * D + 8 * hg;
  const bf16_t* vb = vp + head * D;
  char* img = lds + wave * IMG;
  const int vro = (4 * hg + (col >> 2)) * RS + (col & 3) * 8;  // + 16 RS for the second 16 keys, + 32 dt

  u32x4 kr[2][NS], vr[NV];
  auto gload = [&](int key0) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int key = min(key0 + 16 * kt + col, plen - 1);  // clamped: always inside the prompt's keys
#pragma unroll
      for (int s = 0; s < NS; ++s) kr[kt][s] = ld16(kb + (int64_t)key * D + 32 * s);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = lane + 64 * i;
      const int key = min(key0 + e / NCH, plen - 1);
      vr[i] = ld16(vb + (int64_t)key * D + (e % NCH) * 8);
    }
  };

  int key0 = k0 + KEYS * wave;
  if (key0 < kend) gload(key0);
  for (; key0 < kend; key0 += WAVES * KEYS) {
    __builtin_amdgcn_wave_barrier();  // the previous step's reads of the image come first
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = lane + 64 * i;
      const u32x4 z = {0u, 0u, 0u, 0u};
      *(u32x4*)(img + (e / NCH) * RS + (e % NCH) * 16) = key0 + e / NCH < plen ? vr[i] : z;
    }
    shr_s16x8 kf[2][NS];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < NS; ++s) kf[kt][s] = __builtin_bit_cast(shr_s16x8, kr[kt][s]);
    if (key0 + WAVES * KEYS < kend) gload(key0 + WAVES * KEYS);
    __builtin_amdgcn_wave_barrier();

    // ---- per tile: S^T = K Q^T (sc[kt][j] is key key0 + 16 kt + 4 hg + j of row col), the online softmax of the
    // lane's row, P rounded to bf16 as the MFMA operand; the normaliser sums what V sees
    shr_s16x8 pf[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 sc[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][s], qf[t][s], sc[kt], 0, 0, 0);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = key0 + 16 * kt + 4 * hg + j < plen;
          sc[kt][j] = ok ? sc[kt][j] * scale_log2 : -INFINITY;
          mx = fmaxf(mx, sc[kt][j]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[t], mx);
      const float mr = mn == -INFINITY ? 0.f : mn;
      const float alpha = mn == m[t] ? 1.f : exp2_fast(m[t] - mr);  // an unchanged maximum rescales by exactly 1
      uint32_t pk[4];
      float ps = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
          const float p0 = sc[kt][j] == -INFINITY ? 0.f : exp2_fast(sc[kt][j] - mr);
          const float p1 = sc[kt][j + 1] == -INFINITY ? 0.f : exp2_fast(sc[kt][j + 1] - mr);
          const uint32_t w = pack2(p0, p1);
          pk[2 * kt + (j >> 1)] = w;
          ps += __uint_as_float(w << 16);
          ps += __uint_as_float(w & 0xffff0000u);
        }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[t] = l[t] * alpha + ps;
      m[t] = mn;
#pragma unroll
      for (int i = 0; i < ND; ++i) acc[t][i] *= alpha;
      const u32x4 pw = {pk[0], pk[1], pk[2], pk[3]};
      pf[t] = __builtin_bit_cast(shr_s16x8, pw);
    }
    // ---- O^T += V^T P^T: element j of the fragments is key key0 + 16 (j >> 2) + 4 hg + (j & 3)
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const shr_s16x4 lo = shr_tr_read(img + vro + 32 * dt);
      const shr_s16x4 hi = shr_tr_read(img + vro + 16 * RS + 32 * dt);
      const shr_s16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[t], acc[t][dt], 0, 0, 0);
    }
  }

  // ---- the waves' partials, tile by tile, in wave order; acc[t][dt][j] is O[row col][16 dt + 4 hg + j]
  __syncthreads();  // every wave is done with its V image
  float* red = (float*)lds;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (wave > 0) {
      float* p = red + (wave - 1) * PW * 64 + lane;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) p[(4 * dt + j) * 64] = acc[t][dt][j];
      p[4 * ND * 64] = m[t];
      p[(4 * ND + 1) * 64] = l[t];
    }
    __syncthreads();
    if (wave == 0) {
      float M = m[t], L = l[t];
      for (int w = 0; w < WAVES - 1; ++w) {
        const float* p = red + w * PW * 64 + lane;
        const float m2 = p[4 * ND * 64], l2 = p[(4 * ND + 1) * 64];
        const float mn = fmaxf(M, m2);
        const float mr = mn == -INFINITY ? 0.f : mn;
        const float a1 = exp2_fast(M - mr), a2 = exp2_fast(m2 - mr);
        L = L * a1 + l2 * a2;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[t][dt][j] = acc[t][dt][j] * a1 + p[(4 * dt + j) * 64] * a2;
        M = mn;
      }
      if (orow[t] >= 0) {
        const int64_t slot = orow[t] * nsplit + sp;
        float* po = ws_o + slot * D + 4 * hg;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) *(f32x4*)(po + 16 * dt) = acc[t][dt];
        if (hg == 0) {
          ws_ml[slot * 2] = M;
          ws_ml[slot * 2 + 1] = L;
        }
      }
    }
    if (t + 1 < NT) __syncthreads();  // the merge's reads come before the next tile's writes
  }
}

// ---------------------------------------------------------------------------
// Grid (query head, row), one thread per column: the row's prefix partials that
// the prefix kernel wrote (splits starting below plen), then its suffix
// partials (splits starting below slen), each in index order.  A row without
// keys gets zeros.  kv_split_merge_kernel's sums over two lists.
// ---------------------------------------------------------------------------
__global__ void shared_merge_kernel(const float* __restrict__ po, const float* __restrict__ pml,
                                    const float* __restrict__ so, const float* __restrict__ sml,
                                    const int* __restrict__ plens, const int* __restrict__ slens,
                                    bf16_t* __restrict__ o, int samples, int D, int Cp, int Cs, int max_plen,
                                    int max_slen, int split, int np, int ns) {
  const int b = blockIdx.y, d = threadIdx.x;
  const int64_t row = (int64_t)b * gridDim.x + blockIdx.x;  // b Hq + h
  const int plast = kv_last_key(plens[b / samples], Cp, max_plen), slast = kv_last_key(slens[b], Cs, max_slen);
  const int n1 = plast < 0 ? 0 : min(plast / split + 1, np);
  const int n2 = slast < 0 ? 0 : min(slast / split + 1, ns);
  const int64_t p0 = row * np, s0 = row * ns;
  float M = -INFINITY;
  for (int i = 0; i < n1; ++i) M = fmaxf(M, pml[(p0 + i) * 2]);
  for (int i = 0; i < n2; ++i) M = fmaxf(M, sml[(s0 + i) * 2]);
  const float mr = M == -INFINITY ? 0.f : M;
  float L = 0.f, a = 0.f;
  for (int i = 0; i < n1; ++i) {
    const float w = exp2_fast(pml[(p0 + i) * 2] - mr);
    L += pml[(p0 + i) * 2 + 1] * w;
    a += po[(p0 + i) * D + d] * w;
  }
  for (int i = 0; i < n2; ++i) {
    const float w = exp2_fast(sml[(s0 + i) * 2] - mr);
    L += sml[(s0 + i) * 2 + 1] * w;
    a += so[(s0 + i) * D + d] * w;
  }
  o[row * D + d] = f2bf(L > 0.f ? a / L : 0.f);
}

template <int D>
static void launch_prefix(int NT, dim3 grid, hipStream_t stream, const bf16_t* q, const bf16_t* kp, const bf16_t* vp,
                          const int* plens, float* ws_o, float* ws_ml, int samples, int Hq, int Hkv, int Cp,
                          int max_plen, int split, int nsplit, int nchunk, float scale_log2) {
#define TOA_SHARED_LAUNCH(N_)                                                                                        \
  hipLaunchKernelGGL((attn_shared_prefix_kernel<D, N_>), grid, dim3(BLOCK), 0, stream, q, kp, vp, plens, ws_o, ws_ml, \
                     samples, Hq, Hkv, Cp, max_plen, split, nsplit, nchunk, scale_log2)
  if (NT == 4)
    TOA_SHARED_LAUNCH(4);
  else if (NT == 3)
    TOA_SHARED_LAUNCH(3);
  else if (NT == 2)
    TOA_SHARED_LAUNCH(2);
  else
    TOA_SHARED_LAUNCH(1);
#undef TOA_SHARED_LAUNCH
}

// q, o [B, Hq, D]; kp / vp [groups, Hkv, Cp, D], plens [groups]; ks / vs [B, Hkv, Cs, D], slens [B]; int32 lengths
// on the device.  ws: fp32, B Hq (np + ns) (D + 2) words (decode_shared_shapes.h ws_floats): the prefix's ws_o, the
// suffix's ws_o, the prefix's ws_ml, the suffix's (the outputs first, so both stay 16-byte aligned).  max_plen, max_slen:
// host-side bounds of the lengths that size the grids (0: that part is not launched); keys at or beyond them are not
// attended.  split_keys: a power of two >= 64, of both parts.
extern "C" int toa_attn_decode_shared(const bf16_t* q, const bf16_t* kp, const bf16_t* vp, const int* plens,
                                      const bf16_t* ks, const bf16_t* vs, const int* slens, float* ws, bf16_t* o,
                                      int B, int groups, int samples, int Hq, int Hkv, int Cp, int Cs, int D,
                                      int max_plen, int max_slen, int split_keys, float scale, hipStream_t stream) {
  Operands c = {};
  c.B = B, c.groups = groups, c.samples = samples, c.Hq = Hq, c.Hkv = Hkv, c.D = D, c.Cp = Cp, c.Cs = Cs;
  c.max_plen = max_plen, c.max_slen = max_slen, c.split_keys = split_keys;
  if (check(c) != R_OK) return (int)hipErrorInvalidValue;
  const int G = Hq / Hkv, R = samples * G;
  const int np = (max_plen + split_keys - 1) / split_keys, ns = (max_slen + split_keys - 1) / split_keys;
  const int64_t rows = (int64_t)B * Hq;
  float* po = ws;
  float* so = po + rows * np * D;
  float* pml = so + rows * ns * D;
  float* sml = pml + rows * np * 2;
  int rc = 0;
  if (np > 0) {
    const int NT = tiles(R), nchunk = chunks(R);
    const dim3 grid(np, (unsigned)(Hkv * nchunk), groups);
    const float scale_log2 = scale * 1.4426950408889634f;
    if (D == 128)
      launch_prefix<128>(NT, grid, stream, q, kp, vp, plens, po, pml, samples, Hq, Hkv, Cp, max_plen, split_keys, np,
                         nchunk, scale_log2);
    else
      launch_prefix<64>(NT, grid, stream, q, kp, vp, plens, po, pml, samples, Hq, Hkv, Cp, max_plen, split_keys, np,
                        nchunk, scale_log2);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  if (ns > 0) {
    rc = kv_launch_decode_partials(q, ks, vs, slens, so, sml, B, Hq, Hkv, Cs, D, split_keys, ns, scale, stream);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(shared_merge_kernel, dim3(Hq, B), dim3(D), 0, stream, po, pml, so, sml, plens, slens, o, samples,
                     D, Cp, Cs, max_plen, max_slen, split_keys, np, ns);
  return (int)hipGetLastError();
}

// The check and its words for Python's error messages; the workspace's size.
extern "C" int toa_decode_shared_check(int B, int groups, int samples, int Hq, int Hkv, int D, int Cp, int Cs,
                                       int max_plen, int max_slen, int split_keys) {
  Operands c = {B, groups, samples, Hq, Hkv, D, Cp, Cs, max_plen, max_slen, split_keys};
  return (int)check(c);
}

extern "C" const char* toa_decode_shared_why(int reason) { return why(reason); }
