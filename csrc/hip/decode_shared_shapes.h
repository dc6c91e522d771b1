// What shared-prompt decoding (decode_shared.hip) takes, and the constants of
// its prefix kernel: the one statement of both.  The launchers refuse anything
// whose check is not R_OK before a launch; Python asks the same function
// through toa_decode_shared_check only to name the reason.  Plain C++17, no HIP.
//
//   prefix  K, V [groups][Hkv][Cp][D] bf16, plen[groups]: one row per prompt, read-only while decoding
//   suffix  K, V [B][Hkv][Cs][D] bf16, slen[B], B = groups x samples: row g samples + j is sample j of prompt g
//   q, o    [B][Hq][D] bf16
//
// Why these constants (gfx950):
//   TILE      the 16 query rows of one v_mfma_f32_16x16x32_bf16; the rows of a (prompt, KV head) are
//             r = j G + g, samples x G of them (G = Hq / Hkv).
//   MAX_TILES a wave keeps the Q fragments and the fp32 accumulators of up to 4 tiles (64 rows) in registers:
//             at D = 128 that is 64 + 128 VGPRs of the 512 a wave has at one wave per SIMD.  More rows take
//             further query chunks on the grid.
//   KEYS      keys per wave and step: two S^T tiles of 16 keys, one k-step of 32 keys of P V.  The four waves of
//             a workgroup take the steps w, w + 4, ... of their split, so each K / V byte is read by one wave.
#pragma once

namespace toa_dshared {

constexpr int TILE = 16;
constexpr int MAX_TILES = 4;
constexpr int KEYS = 32;
constexpr int WAVES = 4;
constexpr int BLOCK = 64 * WAVES;

// row tiles per wave, and query chunks on the grid, for `rows` = samples x G query rows of a (prompt, KV head)
constexpr int tiles(int rows) { return rows >= TILE * MAX_TILES ? MAX_TILES : (rows + TILE - 1) / TILE; }
constexpr int chunks(int rows) { return (rows + TILE * tiles(rows) - 1) / (TILE * tiles(rows)); }

struct Operands {
  int B, groups, samples, Hq, Hkv, D;
  int Cp, Cs;              // capacities of the prefix and the suffix cache
  int max_plen, max_slen;  // host-side bounds of plen and slen that size the grids: 0 .. Cp, 0 .. Cs
  int split_keys;          // a power of two >= 64
};

enum Reason { R_OK = 0, R_HEAD_DIM, R_HEADS, R_SAMPLES, R_ROWS, R_SIZES, R_LIMIT, R_SPLIT, R_COUNT };

constexpr const char* why(int reason) {
  switch (reason) {
    case R_OK: return "taken";
    case R_HEAD_DIM: return "head dim not 64 or 128";
    case R_HEADS: return "query heads not a positive multiple of the kv heads";
    case R_SAMPLES: return "samples under 1";
    case R_ROWS: return "rows of q not groups x samples";
    case R_SIZES: return "groups or a capacity not positive, or a grid dimension above 65535";
    case R_LIMIT: return "max_plen outside 0 .. prefix capacity, or max_slen outside 0 .. capacity";
    case R_SPLIT: return "split_keys not a power of two >= 64";
    default: return "unknown reason";
  }
}

// attention: every field; the RoPE-append passes Cp = 1, the limits 0 and split_keys 64
constexpr Reason check(const Operands& o) {
  if (o.D != 64 && o.D != 128) return R_HEAD_DIM;
  if (o.Hq <= 0 || o.Hkv <= 0 || o.Hq % o.Hkv != 0) return R_HEADS;
  if (o.samples < 1) return R_SAMPLES;
  if (o.groups <= 0 || o.B <= 0 || (long long)o.groups * o.samples != o.B) return o.groups <= 0 ? R_SIZES : R_ROWS;
  if (o.Cp <= 0 || o.Cs <= 0 || o.B > 65535) return R_SIZES;
  const int G = o.Hq / o.Hkv;
  if ((long long)o.samples * G > 0x7fffffff / 2) return R_SIZES;
  if ((long long)o.Hkv * chunks(o.samples * G) > 65535 || o.Hq > 65535) return R_SIZES;
  if (o.max_plen < 0 || o.max_plen > o.Cp || o.max_slen < 0 || o.max_slen > o.Cs) return R_LIMIT;
  if (o.split_keys < 64 || (o.split_keys & (o.split_keys - 1)) != 0) return R_SPLIT;
  return R_OK;
}

// fp32 words of the attention's workspace: per (row, head, split of the prefix or of the suffix) D of
// unnormalised output, the running maximum and the normaliser
constexpr long long ws_floats(const Operands& o) {
  const long long np = (o.max_plen + o.split_keys - 1) / o.split_keys, ns = (o.max_slen + o.split_keys - 1) / o.split_keys;
  return (long long)o.B * o.Hq * (np + ns) * (o.D + 2);
}

}  // namespace toa_dshared
