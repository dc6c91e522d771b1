// Boundary table of gemm_asm_shapes.h: per form, operands at the edges of
// every condition and the reason the check must return.  The expected reasons
// were read off the launchers' condition chains as they stood before the
// header existed (gemm_asm.hip common_ok / nn_ok / wgrad_asm_launch, wgrad.hip
// toa_wgrad), not off the header.
//
// `py`, written per row from the Python of that time: what its predicate
// answered for the same operands (YES / NO), or NA where it had none -- an
// operand it never saw (the output it allocates itself, a forced split, the
// workspace) or a form it tried by launching (the delta epilogues).  The
// predicates: ops/gemm.py asm_takes under the policy that picks the form (tn:
// first_step, whole tiles; tn_rows, nn: ``asm``), nn_takes, swiglu_gate_up /
// swiglu_down_dgrad, wgrad_hip_ok with the token rule of the row's kernel;
// ops/llm.py _resadd_ok and qkv_rope_attention_ok.  main() holds the header's
// answer against py as well: they agree on every row but the ones kDiffer
// names, where the old pair itself disagreed or Python keeps a rule of its
// own.  Builds alone: g++ -std=c++17 -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../gemm_asm_shapes.h"

using namespace toa_shapes;

namespace {

constexpr uintptr_t A = 0x10000;   // an aligned base
constexpr int64_t LD_MAX = (1ll << 23) - 8;

struct Row {
  std::string what;
  int form;
  Operands o;
  Reason want;
  int py;   // the old Python predicate's answer
};
enum { NA = -1, NO = 0, YES = 1 };

// Rows where the header's answer and the old Python predicate's differ, each for a stated cause.
const std::set<std::string> kDiffer = {
    // Python required a contiguous residual (still does: a tensor-kind gate); the launcher takes a padded one
    "tn_resadd ldc=cols+8", "tn_resadd ldc=8388600",
    // Python did not know the launcher's 32-bit limit on the up half's offset: taken, then refused mid-step
    "tn_swiglu_fwd up half over 2^32",
    // Python asks for grouped query heads, Hq % Hkv == 0 (still does: the attention's rule, not the GEMM's)
    "tn_rope Hkv > Hq",
    // wgrad_hip_ok checked strides % 8 only, not that a stride covers its row; no columns passed its N % 256
    "wgrad_asm dY stride M-8", "wgrad_asm N=0",
};
std::vector<Row> rows;

using Edit = std::function<void(Operands&)>;

void add(const std::string& what, int form, Operands o, const Edit& edit, Reason want, int py) {
  edit(o);
  rows.push_back({what, form, o, want, py});
}

// C [M][N] = X [M][K] W [N][K]^T, everything contiguous
Operands tn(int M = 256, int N = 256, int K = 128) {
  Operands o = {};
  o.X = o.W = o.C = o.S = o.D = A;
  o.ldx = o.ldw = K, o.ldc = o.lds = N;
  o.M = M, o.N = N, o.K = K;
  return o;
}
Operands nn(int M = 256, int N = 256, int K = 128) {
  Operands o = tn(M, N, K);
  o.ldw = N;
  return o;
}
Operands swiglu_fwd(int F) {   // gu [M][2F] in C, s [M][F] in S
  Operands o = tn(256, F, 128);
  o.ldc = 2 * F, o.lds = F;
  return o;
}
Operands swiglu_bwd(int F, bool nn_form) {   // dgu in C, gu in S, both [M][2F]
  Operands o = nn_form ? nn(256, F, 128) : tn(256, F, 128);
  o.ldc = o.lds = 2 * F;
  return o;
}
Operands rope(int M = 256, int S = 256, int Hq = 2, int Hkv = 1) {
  Operands o = tn(M, 0, 128);
  o.ldc = o.lds = 0, o.Sq = S, o.Hq = Hq, o.Hkv = Hkv;
  return o;
}
Operands delta(bool nn_form, int M = 256, int S = 256, int H = 2) {
  Operands o = nn_form ? nn(M) : tn(M);
  o.Sq = S, o.H = H;
  return o;
}
Operands wgrad(int T, int split = 0, int M = 256, int N = 256) {   // dW [M][N] (+)= dY [T][M]^T X [T][N]
  Operands o = {};
  o.X = o.W = o.C = o.S = A;
  o.ldx = M, o.ldw = o.ldc = N;
  o.M = M, o.N = N, o.K = T, o.split = split;
  return o;
}

const Edit none = [](Operands&) {};

// what all forms with X [M][K], a 256-multiple N and C [M][N] share
// py_tail: asm_takes on a partial tile row under the policy that picks this form (``asm``: yes; first_step: no).
// resadd: C is laid out like the residual, which Python wanted contiguous; elsewhere Python allocates C itself.
void plain_edges(const char* name, int form, const Operands& base, bool rows_free, bool is_nn, int py_tail,
                 bool resadd) {
  const std::string n = name;
  const Reason tail = rows_free ? R_OK : R_M_TILES;
  const struct { int M; Reason want; int py; } ms[] = {{0, R_M_RANGE, NO}, {1, tail, py_tail}, {255, tail, py_tail},
                                                       {256, R_OK, YES}, {257, tail, py_tail},
                                                       {(1 << 28) - 1, tail, py_tail}, {1 << 28, R_M_RANGE, NO}};
  for (auto& m : ms) add(n + " M=" + std::to_string(m.M), form, base, [&](Operands& o) { o.M = m.M; }, m.want, m.py);
  const struct { int N; Reason want; int py; } ns[] = {{0, R_N, NO}, {128, R_N, NO}, {256, R_OK, YES}, {384, R_N, NO}};
  for (auto& v : ns)
    add(n + " N=" + std::to_string(v.N), form, base, [&](Operands& o) {
      o.N = v.N, o.ldc = v.N;
      if (is_nn) o.ldw = v.N;
    }, v.want, v.py);
  const struct { int K; Reason want; int py; } ks[] = {{64, R_K, NO}, {128, R_OK, YES}, {160, R_K, NO}, {192, R_OK, YES}};
  for (auto& v : ks)
    add(n + " K=" + std::to_string(v.K), form, base, [&](Operands& o) {
      o.K = v.K, o.ldx = v.K;
      if (!is_nn) o.ldw = v.K;
    }, v.want, v.py);
  // row strides: X and (TN) W against K, (NN) W and C against N.  py_in: Python on an input's stride; py_c: on C's
  const struct { int64_t d; bool abs; Reason want; int py_in, py_c; } lds[] = {
      {-8, false, R_LD, NO, resadd ? NO : NA},    {0, false, R_OK, YES, resadd ? YES : NA},
      {4, false, R_LD, NO, resadd ? NO : NA},     {8, false, R_OK, YES, resadd ? NO : NA},
      {LD_MAX, true, R_OK, YES, resadd ? NO : NA}, {LD_MAX + 8, true, R_LD, NO, resadd ? NO : NA}};
  for (auto& v : lds) {
    const std::string s = v.abs ? "=" + std::to_string(v.d) : "=cols" + (v.d < 0 ? std::to_string(v.d) : "+" + std::to_string(v.d));
    add(n + " ldx" + s, form, base, [&](Operands& o) { o.ldx = v.abs ? v.d : o.K + v.d; }, v.want, v.py_in);
    add(n + " ldw" + s, form, base, [&](Operands& o) { o.ldw = v.abs ? v.d : (is_nn ? o.N : o.K) + v.d; }, v.want, v.py_in);
    add(n + " ldc" + s, form, base, [&](Operands& o) { o.ldc = v.abs ? v.d : o.N + v.d; }, v.want, v.py_c);
  }
  add(n + " X % 16 == 8", form, base, [](Operands& o) { o.X += 8; }, R_ALIGN, NO);
  add(n + " W % 16 == 8", form, base, [](Operands& o) { o.W += 8; }, R_ALIGN, NO);
  add(n + " C % 16 == 8", form, base, [](Operands& o) { o.C += 8; }, R_ALIGN, NA);
  add(n + " C not allocated yet", form, base, [](Operands& o) { o.C = 0; }, R_OK, YES);
}

void build_table() {
  plain_edges("tn", F_TN, tn(), false, false, NO, false);
  plain_edges("tn_rows", F_TN_ROWS, tn(), true, false, YES, false);
  plain_edges("tn_resadd", F_TN_RESADD, tn(), true, false, YES, true);
  plain_edges("nn", F_NN, nn(), true, true, YES, false);
  add("tn_resadd R % 16 == 8", F_TN_RESADD, tn(), [](Operands& o) { o.S += 8; }, R_ALIGN, NO);
  // the first failure wins, in the launchers' order
  add("tn M, K and X all bad: M first", F_TN, tn(0, 384, 160), [](Operands& o) { o.X += 8; }, R_M_RANGE, NO);
  add("tn K before the strides", F_TN, tn(256, 256, 160), [](Operands& o) { o.ldx = 4; }, R_K, NO);
  add("tn X, W strides before N", F_TN, tn(256, 384, 128), [](Operands& o) { o.ldw = 132; }, R_LD, NO);
  add("tn 2^28 after the alignment", F_TN, tn(1 << 28), [](Operands& o) { o.W += 8; }, R_ALIGN, NO);
  add("nn 2^28 before N", F_NN, nn(1 << 28, 384), none, R_M_RANGE, NO);
  add("nn N before K", F_NN, nn(256, 384, 160), none, R_N, NO);

  // SwiGLU: F in N; the forward takes 128-multiples, the backward 256-multiples
  for (int F : {128, 256, 384}) {
    const std::string f = " F=" + std::to_string(F);
    add("tn_swiglu_fwd" + f, F_TN_SWIGLU_FWD, swiglu_fwd(F), none, R_OK, YES);                                    // F % 128
    add("tn_swiglu_bwd" + f, F_TN_SWIGLU_BWD, swiglu_bwd(F, false), none, F % 256 ? R_F : R_OK, F == 256 ? YES : NO);   // asm_takes: N % 256
    add("nn_swiglu_bwd" + f, F_NN_SWIGLU_BWD, swiglu_bwd(F, true), none, F % 256 ? R_F : R_OK, F == 256 ? YES : NO);    // nn_takes: N % 256
  }
  add("tn_swiglu_fwd F=64", F_TN_SWIGLU_FWD, swiglu_fwd(64), none, R_F, NO);
  add("tn_swiglu_fwd F=0", F_TN_SWIGLU_FWD, swiglu_fwd(0), none, R_F, NO);
  add("tn_swiglu_fwd M=257", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.M = 257; }, R_OK, YES);
  add("tn_swiglu_bwd M=257", F_TN_SWIGLU_BWD, swiglu_bwd(256, false), [](Operands& o) { o.M = 257; }, R_OK, YES);
  add("nn_swiglu_bwd M=257", F_NN_SWIGLU_BWD, swiglu_bwd(256, true), [](Operands& o) { o.M = 257; }, R_OK, YES);
  add("tn_swiglu_fwd K=64", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.K = o.ldx = o.ldw = 64; }, R_K, NO);
  add("tn_swiglu_fwd gu stride 2F-8", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.ldc -= 8; }, R_LD, NA);
  add("tn_swiglu_fwd s stride F+4", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.lds += 4; }, R_LD, NA);
  add("tn_swiglu_fwd s % 16 == 8", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.S += 8; }, R_ALIGN, NA);
  add("tn_swiglu_fwd up half just under 2^32", F_TN_SWIGLU_FWD, swiglu_fwd(128), [](Operands& o) { o.ldw = LD_MAX; }, R_OK, YES);
  add("tn_swiglu_fwd up half over 2^32", F_TN_SWIGLU_FWD, swiglu_fwd(256), [](Operands& o) { o.ldw = LD_MAX; }, R_W_UP32, YES);
  for (int nf = 0; nf < 2; ++nf) {
    const int form = nf ? F_NN_SWIGLU_BWD : F_TN_SWIGLU_BWD;
    const std::string n = nf ? "nn_swiglu_bwd" : "tn_swiglu_bwd";
    add(n + " gu stride 2F-8", form, swiglu_bwd(256, nf), [](Operands& o) { o.lds -= 8; }, R_LD, NO);
    add(n + " dgu stride 2F+8", form, swiglu_bwd(256, nf), [](Operands& o) { o.ldc += 8; }, R_OK, NA);
    add(n + " gu % 16 == 8", form, swiglu_bwd(256, nf), [](Operands& o) { o.S += 8; }, R_ALIGN, NO);
    add(n + " K=160", form, swiglu_bwd(256, nf), [](Operands& o) { o.K = o.ldx = 160; }, R_K, NO);
  }

  // RoPE: Hq = 2, Hkv = 1 is N = 512
  add("tn_rope smallest", F_TN_ROPE, rope(), none, R_OK, YES);
  add("tn_rope M=257", F_TN_ROPE, rope(257), none, R_M_TILES, NO);
  add("tn_rope S=0", F_TN_ROPE, rope(256, 0), none, R_SEQ, NO);
  add("tn_rope S=128", F_TN_ROPE, rope(256, 128), none, R_SEQ, NO);
  add("tn_rope M=768 S=512", F_TN_ROPE, rope(768, 512), none, R_SEQ, NO);
  add("tn_rope M=768 S=256", F_TN_ROPE, rope(768, 256), none, R_OK, YES);
  add("tn_rope Hq=0", F_TN_ROPE, rope(256, 256, 0, 1), none, R_HEADS, NO);
  add("tn_rope Hq=4097", F_TN_ROPE, rope(256, 256, 4097, 1), none, R_HEADS, NO);
  add("tn_rope Hkv=0", F_TN_ROPE, rope(256, 256, 2, 0), none, R_HEADS, NO);
  add("tn_rope Hkv=4097", F_TN_ROPE, rope(256, 256, 2, 4097), none, R_HEADS, NO);
  add("tn_rope Hq=4096 Hkv=4096", F_TN_ROPE, rope(256, 256, 4096, 4096), none, R_OK, YES);
  add("tn_rope Hkv > Hq", F_TN_ROPE, rope(256, 256, 2, 4), none, R_OK, NO);
  add("tn_rope (Hq + 2 Hkv) 128 = 384", F_TN_ROPE, rope(256, 256, 1, 1), none, R_N, NO);
  add("tn_rope table % 16 == 8", F_TN_ROPE, rope(), [](Operands& o) { o.S += 8; }, R_ALIGN, NA);
  add("tn_rope M N 2 = 2^32 - 2^18", F_TN_ROPE, rope((1 << 22) - 256), none, R_OK, YES);
  add("tn_rope M N 2 = 2^32", F_TN_ROPE, rope(1 << 22), none, R_OUT32, NO);
  add("tn_rope M N 2 = 2^32 (16 + 2 x 8 heads)", F_TN_ROPE, rope(524288, 256, 16, 8), none, R_OUT32, NO);
  add("tn_rope one tile row under it", F_TN_ROPE, rope(524288 - 256, 256, 16, 8), none, R_OK, YES);
  // (the table limit S 512 + 2^15 < 2^32 needs S >= 2^23 - 64 <= M, where M N 2 is over 2^32
  // already: the launcher's order reports the output; the limit itself is checked in main)
  add("tn_rope S = M = 2^23 - 256", F_TN_ROPE, rope((1 << 23) - 256, (1 << 23) - 256), none, R_OUT32, NO);

  // delta: heads of 128 columns, H 128 == N
  for (int nf = 0; nf < 2; ++nf) {
    const int form = nf ? F_NN_DELTA : F_TN_DELTA;
    const std::string n = nf ? "nn_delta" : "tn_delta";
    add(n + " smallest", form, delta(nf), none, R_OK, NA);
    add(n + " M=257", form, delta(nf, 257), none, R_M_TILES, NA);
    add(n + " S=0", form, delta(nf, 256, 0), none, R_SEQ, NA);
    add(n + " S=128", form, delta(nf, 256, 128), none, R_SEQ, NA);
    add(n + " M=768 S=512", form, delta(nf, 768, 512), none, R_SEQ, NA);
    add(n + " H=0", form, delta(nf, 256, 256, 0), none, R_HEADS, NA);
    add(n + " H 128 != N", form, delta(nf, 256, 256, 3), none, R_HEADS, NA);
    add(n + " N=384", form, delta(nf, 256, 256, 3), [&](Operands& o) { o.N = o.ldc = 384; if (nf) o.ldw = 384; }, R_N, NA);
    add(n + " K=160", form, delta(nf), [&](Operands& o) { o.K = o.ldx = 160; if (!nf) o.ldw = 160; }, R_K, NA);
    add(n + " O % 16 == 8", form, delta(nf), [](Operands& o) { o.S += 8; }, R_ALIGN, NA);
    add(n + " no delta rows", form, delta(nf), [](Operands& o) { o.D = 0; }, R_DELTA_PTR, NA);
    add(n + " delta rows % 4 == 2", form, delta(nf), [](Operands& o) { o.D += 2; }, R_DELTA_PTR, NA);
    add(n + " delta rows % 16 == 4", form, delta(nf), [](Operands& o) { o.D += 4; }, R_OK, NA);
    add(n + " delta rows before the heads", form, delta(nf, 256, 128, 3), [](Operands& o) { o.D = 0; }, R_DELTA_PTR, NA);
  }

  // the assembly weight gradient: ceil(T / 64) k-tiles, at least 2 a piece
  // py: _asm_wgrad_takes_tokens, T >= 65
  const struct { int T; Reason want; int py; } ts[] = {{64, R_WG_KTILES, NO}, {65, R_OK, YES}, {127, R_OK, YES},
                                                       {128, R_OK, YES}, {1000, R_OK, YES}, {1024, R_OK, YES},
                                                       {0, R_WG_TOKENS, NO}, {1, R_WG_KTILES, NO}};
  for (auto& t : ts) add("wgrad_asm T=" + std::to_string(t.T), F_WGRAD_ASM, wgrad(t.T), none, t.want, t.py);
  // (wgrad_hip_ok never saw a forced split)
  const struct { int T, split; Reason want; } ss[] = {{1024, 1, R_OK}, {1024, 4, R_OK}, {1024, 5, R_SPLIT},
                                                      {1024, -1, R_SPLIT}, {200, 2, R_OK}, {200, 3, R_WG_KTILES},
                                                      {129, 2, R_WG_KTILES}, {200, 4, R_WG_KTILES}, {3072, 3, R_OK}};
  for (auto& s : ss)
    add("wgrad_asm T=" + std::to_string(s.T) + " split=" + std::to_string(s.split), F_WGRAD_ASM, wgrad(s.T, s.split),
        none, s.want, NA);
  add("wgrad_asm M=128", F_WGRAD_ASM, wgrad(1024, 0, 128), none, R_WG_OUT, NO);
  add("wgrad_asm N=0", F_WGRAD_ASM, wgrad(1024, 0, 256, 0), none, R_WG_OUT, YES);
  add("wgrad_asm N=384", F_WGRAD_ASM, wgrad(1024, 0, 256, 384), none, R_WG_OUT, NO);
  add("wgrad_asm dY stride M-8", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.ldx -= 8; }, R_LD, YES);
  add("wgrad_asm X stride N+4", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.ldw += 4; }, R_LD, NO);
  add("wgrad_asm dY stride M+256 (a column view)", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.ldx += 256; }, R_OK, YES);
  add("wgrad_asm dW stride 2^23", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.ldc = LD_MAX + 8; }, R_LD, NO);
  add("wgrad_asm X % 16 == 8", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.W += 8; }, R_ALIGN, NO);
  add("wgrad_asm auto split 2, no workspace", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.S = 0; }, R_WORKSPACE, NA);
  add("wgrad_asm auto split 2, workspace % 16 == 8", F_WGRAD_ASM, wgrad(1024), [](Operands& o) { o.S += 8; }, R_WORKSPACE, NA);
  add("wgrad_asm split 1 needs no workspace", F_WGRAD_ASM, wgrad(1024, 1), [](Operands& o) { o.S = 0; }, R_OK, NA);
  add("wgrad_asm T=1000 runs whole: no workspace", F_WGRAD_ASM, wgrad(1000), [](Operands& o) { o.S = 0; }, R_OK, NA);
  add("wgrad_asm 4 x 4032 pieces", F_WGRAD_ASM, wgrad(1024, 4, 16384, 16128), none, R_OK, NA);
  add("wgrad_asm 4 x 4096 pieces", F_WGRAD_ASM, wgrad(1024, 4, 16384, 16384), none, R_WG_PIECES, NA);

  // the HIP weight gradient: 128-row steps per piece, from 1024 tokens.  (T = 896 is the one row where
  // the old pair disagreed -- toa_wgrad launched it, ops/gemm.py never sent it; the form is Python's answer.)
  // py: _hip_wgrad_takes_tokens, T % 128 == 0 and T >= 1024
  const struct { int T; Reason want; int py; } hs[] = {{896, R_WG_HIP_TOKENS, NO}, {1024, R_OK, YES},
                                                       {1088, R_WG_HIP_SPLIT, NO}, {1152, R_OK, YES}, {0, R_WG_TOKENS, NO}};
  for (auto& t : hs) add("wgrad_hip T=" + std::to_string(t.T), F_WGRAD_HIP, wgrad(t.T), none, t.want, t.py);
  // wgrad_hip_ok wanted 16-byte aligned bases for either kernel; toa_wgrad itself did not look
  add("wgrad_hip dY % 16 == 8", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.X += 8; }, R_ALIGN, NO);
  add("wgrad_hip X % 16 == 8", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.W += 8; }, R_ALIGN, NO);
  add("wgrad_hip dW % 16 == 8", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.C += 8; }, R_ALIGN, NO);
  add("wgrad_hip dY stride M+256 (a column view)", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.ldx += 256; }, R_OK, YES);
  add("wgrad_hip T=3072 split=3", F_WGRAD_HIP, wgrad(3072, 3), none, R_OK, NA);
  add("wgrad_hip T=1024 split=3", F_WGRAD_HIP, wgrad(1024, 3), none, R_WG_HIP_SPLIT, NA);
  add("wgrad_hip split=-1", F_WGRAD_HIP, wgrad(1024, -1), none, R_SPLIT, NA);
  add("wgrad_hip M=128", F_WGRAD_HIP, wgrad(1024, 0, 128), none, R_WG_OUT, NO);
  add("wgrad_hip dY stride M+4", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.ldx += 4; }, R_LD, NO);
  add("wgrad_hip auto split 2, no workspace", F_WGRAD_HIP, wgrad(1024), [](Operands& o) { o.S = 0; }, R_WORKSPACE, NA);
  add("wgrad_hip split 1 needs no workspace", F_WGRAD_HIP, wgrad(1024, 1), [](Operands& o) { o.S = 0; }, R_OK, NA);

  add("no such form", F_COUNT, tn(), none, R_FORM, NA);
  add("no such form (-1)", -1, tn(), none, R_FORM, NA);
}

// the plans tests/test_ops_gpu.py pins on the device (toa_wgrad_split), and the tails' own
static_assert(wgrad_plan(4352, 4096, 4096, 0, false).split == 4 && wgrad_plan(4352, 4096, 4096, 0, false).full == 256, "");
static_assert(wgrad_plan(5376, 4096, 3072, 0, false).split == 3, "");
static_assert(wgrad_plan(1024, 1024, 2048, 0, false).split == 4 && wgrad_plan(1024, 1024, 2048, 0, false).full == 0, "");
static_assert(wgrad_plan(4096, 4096, 2048, 0, false).split == 1 && wgrad_plan(4096, 4096, 2048, 0, false).full == 256, "");
static_assert(wgrad_plan(256, 256, 1024, 0, true).split == 2 && wgrad_plan(256, 256, 1000, 0, true).split == 1, "");
static_assert(wgrad_plan(256, 256, 1100, 0, true).split == 2, "18 k-tiles, 550 rows a piece");
static_assert(wgrad_plan(256, 256, 1100, 0, false).split == 1, "no whole 128-row steps");
static_assert(wgrad_plan(512, 768, 2048, 2, true).full == 0 && wgrad_plan(512, 768, 2048, 1, true).full == 6, "");
static_assert(wgrad_workspace(4352, 4096, 4096, 0, false) == 4ll * 16 * 256 * 256 * 4, "16 tail tiles in 4 pieces");
static_assert(wgrad_workspace(512, 768, 2048, 2, true) == 2ll * 6 * 256 * 256 * 4, "");
static_assert(wgrad_workspace(4096, 4096, 2048, 0, true) == 0, "");
// the RoPE table's 32-bit limit, just under and at its bound
static_assert(rope_table_fits((1 << 23) - 65) && !rope_table_fits((1 << 23) - 64), "");
static_assert(ld_ok(LD_MAX, 128) && !ld_ok(LD_MAX + 8, 128) && !ld_ok(120, 128) && !ld_ok(132, 128), "");
static_assert(check_tn(Operands{A, A, A, 0, 0, 128, 128, 256, 0, 256, 256, 128, 0, 0, 0, 0, 0}, false) == R_OK, "constexpr");

}  // namespace

int main() {
  build_table();
  int bad = 0, taken = 0;
  for (const Row& r : rows) {
    const Reason got = check(r.form, r.o);
    taken += got == R_OK;
    const bool differs = r.py != NA && (got == R_OK) != (r.py == YES);
    if (differs != (kDiffer.count(r.what) == 1)) {
      ++bad;
      std::printf("FAIL %-45s the old Python predicate said %d, the check %d (%s)%s\n", r.what.c_str(), r.py, (int)got,
                  why(got), differs ? "" : ": listed in kDiffer, but they agree");
    }
    if (got != r.want) {
      ++bad;
      std::printf("FAIL %-45s want %d (%s)\n     %-45s got  %d (%s)\n", r.what.c_str(), (int)r.want, why(r.want), "",
                  (int)got, why(got));
    }
  }
  for (const std::string& name : kDiffer) {
    bool found = false;
    for (const Row& r : rows) found |= r.what == name;
    if (!found) {
      ++bad;
      std::printf("FAIL kDiffer names no row: %s\n", name.c_str());
    }
  }
  // every reason has its own words, and the table reaches all of them but the shadowed table limit
  std::set<std::string> words;
  std::set<int> seen;
  for (int r = 0; r < R_COUNT; ++r) words.insert(why(r));
  for (const Row& r : rows) seen.insert(r.want);
  if ((int)words.size() != R_COUNT || std::strcmp(why(R_COUNT), "unknown reason") != 0) {
    ++bad;
    std::printf("FAIL reason texts are not distinct\n");
  }
  for (int r = 0; r < R_COUNT; ++r)
    if (!seen.count(r) && r != R_TABLE32) {
      ++bad;
      std::printf("FAIL no row reaches reason %d (%s)\n", r, why(r));
    }
  if (bad) return 1;
  std::printf("gemm shapes selftest OK: %zu rows, %d taken\n", rows.size(), taken);
  return 0;
}
