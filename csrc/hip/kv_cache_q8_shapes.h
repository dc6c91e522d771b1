// What the fp8 KV cache's kernels (kv_cache_q8.hip, and extend.hip's e4m3
// instantiation) take: the one statement of it.  The launchers refuse anything
// whose check is not R_OK before a launch, and Python asks the same function
// through toa_kv_q8_check (ops/decode.py _q8_refusal) instead of restating it.
// Plain C++17, no HIP.
//
//   cache   K8, V8 [B][Hkv][C][D] e4m3 bytes (OCP "fn"), k_scale, v_scale [B][Hkv][C] fp32 = 2^e (e4m3_quant.h's
//           rule on one D-wide row; NaN for a row with a non-finite element).  A slot holds quantize(the bf16 row
//           the bf16 cache would hold); scale * byte is a bf16 value.
//   append  qkv [B][T][(Hq + 2 Hkv) D] bf16 -> rotated q [B][T][Hq][D] bf16, slots start[b] + t of the cache
//   fill    k, v [B][Hkv][P][D] bf16 -> slots 0 .. P - 1 of the cache
//   decode  q [B][Hq][D] bf16 against keys 0 .. len[b] - 1 -> o [B][Hq][D] bf16
//   extend  q [B][T][Hq][D] bf16, token t against keys 0 .. start[b] + t
//
// Why these constants (gfx950):
//   COLS    a lane owns 8 columns of a key row: 8 bytes of the cache (one 8-byte load or store), 16 of a bf16 row.
//           A row is D / 8 lanes, as in the bf16 decode kernel, so its DPP sum and its 8 q + 8 acc columns per head
//           carry over, the whole GQA group up to 8 heads per byte, without scratch.
//   KU      8 key rows of K and of V in flight per lane: 8 x 8 B, the bytes the bf16 kernel keeps (4 x 16 B).
//   KS      the online softmax runs on KS = 4 keys at a time, the bf16 kernel's count: the scores of 8 heads x 8
//           keys at once would cost 32 VGPRs more than the loads gained.
#pragma once

#include <cstdint>

namespace toa_kvq8 {

constexpr int COLS = 8;     // columns (bytes of the cache) per lane
constexpr int KU = 8;       // key rows of K and of V in flight per lane of the decode kernel
constexpr int KS = 4;       // key rows per softmax update
constexpr int BLOCK = 256;  // threads of every kernel here

enum Op { OP_APPEND = 0, OP_FILL, OP_DECODE, OP_EXTEND, OP_COUNT };

struct Operands {
  uintptr_t K8, V8, KSCALE, VSCALE;  // the cache
  int B, T, Hq, Hkv, D, C;           // T: tokens per row (append, extend; 1 when decoding), P for fill
  int limit;                         // append: rows of the RoPE table; decode, extend: max_len; fill: unused
  int split_keys;                    // decode: a power of two >= 64; extend: that or 0
};

enum Reason { R_OK = 0, R_OP, R_HEAD_DIM, R_HEADS, R_SIZES, R_TOKENS, R_LIMIT, R_SPLIT, R_CACHE, R_SCALE, R_COUNT };

constexpr const char* why(int reason) {
  switch (reason) {
    case R_OK: return "taken";
    case R_OP: return "unknown operation";
    case R_HEAD_DIM: return "head dim not 64 or 128";
    case R_HEADS: return "query heads not a positive multiple of the kv heads";
    case R_SIZES: return "batch or capacity not positive, or a batch above 65535";
    case R_TOKENS: return "tokens per row under 1, or above the capacity";
    case R_LIMIT: return "max_len outside 1 .. capacity, or an empty RoPE table";
    case R_SPLIT: return "split_keys not a power of two >= 64 (extend: or 0)";
    case R_CACHE: return "cache bytes null or not 16-byte aligned";
    case R_SCALE: return "k_scale / v_scale null or not 4-byte aligned";
    default: return "unknown reason";
  }
}

constexpr Reason check(int op, const Operands& o) {
  if (op < 0 || op >= OP_COUNT) return R_OP;
  if (o.D != 64 && o.D != 128) return R_HEAD_DIM;
  if (o.Hkv <= 0 || (op != OP_FILL && (o.Hq <= 0 || o.Hq % o.Hkv != 0))) return R_HEADS;
  if (o.B <= 0 || o.C <= 0 || (op != OP_APPEND && op != OP_FILL && o.B > 65535)) return R_SIZES;
  if (o.T < 1 || (op == OP_FILL && o.T > o.C)) return R_TOKENS;
  if (op == OP_APPEND ? o.limit <= 0 : op != OP_FILL && (o.limit < 1 || o.limit > o.C)) return R_LIMIT;
  if (op == OP_DECODE || op == OP_EXTEND) {
    const int s = o.split_keys;
    if (!(op == OP_EXTEND && s == 0) && (s < 64 || (s & (s - 1)) != 0)) return R_SPLIT;
  }
  if (o.K8 == 0 || o.V8 == 0 || ((o.K8 | o.V8) & 15)) return R_CACHE;
  if (o.KSCALE == 0 || o.VSCALE == 0 || ((o.KSCALE | o.VSCALE) & 3)) return R_SCALE;
  return R_OK;
}

}  // namespace toa_kvq8
