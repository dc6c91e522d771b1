// What KV-cache decoding (decode.hip) and extending (extend.hip) share; the
// kernels declared here are compiled once, in kv_cache.hip.
//
// Cache layout: K and V are [B, Hkv, C, D] bf16 per layer (C = capacity), K
// stored already rotated, so the keys of one KV head are contiguous.
//
// Workspace of a split attention: fp32, rows x nsplit x (D + 2) words, where a
// row is one query (b, t, h) -- (b T + t) Hq + h, T = 1 when decoding -- and
// nsplit = ceil(max_len / split_keys):
//   ws_o  [rows, nsplit, D] unnormalised output
//   ws_ml [rows, nsplit, 2] running max (log2 domain), normaliser
// The main kernels write the partial of (row, split) only if the split starts
// at or below the row's last key; kv_split_merge_kernel reads exactly those.
#pragma once
#include "toa_common.h"

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// The last of a row's n keys 0 .. n - 1, or -1 for none (n <= 0).  n is cut to
// the cache, and to max_len, which bounds the keys as it bounds the grid.
__device__ __forceinline__ int kv_last_key(int n, int C, int max_len) {
  return max(min(min(n, C), max_len), 0) - 1;
}

// The last key that token t of an extended row attends -- its own, at position
// st + t -- or -1 for a token that is not there (t >= cnt, or a position
// outside the cache).
__device__ __forceinline__ int kv_token_last_key(int st, int cnt, int t, int C, int max_len) {
  if (st < 0 || st >= C || t >= cnt || t >= C - st) return -1;
  return kv_last_key(st + t + 1, C, max_len);
}

// RoPE at position start[b] + t of the T tokens of row b, t < count[b], and
// append to the caches.  count == nullptr: every token is there (decoding:
// T = 1, start is pos).  Arguments are the entry points' to check.
int kv_launch_rope_append(const bf16_t* qkv, const float* cosv, const float* sinv, const int* start, const int* count,
                          bf16_t* q, bf16_t* kc, bf16_t* vc, int B, int T, int Hq, int Hkv, int D, int C,
                          int tab_rows, hipStream_t stream);

// The splits of every query row -> o [B, T, Hq, D] bf16.  count != nullptr:
// the row's last key is kv_token_last_key(start[b], count[b], t); nullptr
// (decoding, T = 1): start holds the rows' lengths, kv_last_key(start[b]).
int kv_launch_split_merge(const float* ws_o, const float* ws_ml, const int* start, const int* count, bf16_t* o, int B,
                          int T, int Hq, int D, int C, int max_len, int split, int nsplit, hipStream_t stream);
