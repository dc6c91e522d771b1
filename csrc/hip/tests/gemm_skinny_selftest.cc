// Boundary table of gemm_skinny_shapes.h: every reason once, with the value on
// each side of its boundary, and the launch plan at the shapes the tests and
// the Llama-3-8B decode step use.  The expected answers are written from the
// statement of what the kernel takes (docs/kernels.md "Decoding"), not read
// off the header.  Builds alone: g++ -std=c++17 -fsanitize=address,undefined.
#include <cstdio>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../gemm_skinny_shapes.h"

using namespace toa_skinny;

namespace {

constexpr uintptr_t A = 0x10000;   // an aligned base

struct Row {
  std::string what;
  int form;
  Operands o;
  Reason want;
};
std::vector<Row> rows;

using Edit = std::function<void(Operands&)>;

// y [M][N] = x [M][K] w [N][K]^T, everything contiguous; N = 16 and K = 4096 - 24 split K in two, so a workspace counts
Operands plain(int M = 8, int N = 48, int K = 520) {
  Operands o = {};
  o.X = o.W = o.Y = o.WS = A;
  o.ldx = o.ldw = K, o.ldy = N, o.w_rows = N;
  o.M = M, o.N = N, o.K = K;
  return o;
}
Operands swiglu(int M = 8, int F = 48, int K = 520) {
  Operands o = plain(M, F, K);
  o.w_rows = 2 * F;
  return o;
}

void add(const std::string& what, int form, Operands o, const Edit& edit, Reason want) {
  edit(o);
  rows.push_back({what, form, o, want});
}

void table() {
  const Edit none = [](Operands&) {};
  for (int form : {F_PLAIN, F_SWIGLU}) {
    const std::string f = form == F_PLAIN ? "plain " : "swiglu ";
    const auto base = [&](int M = 8, int N = 48, int K = 520) { return form == F_PLAIN ? plain(M, N, K) : swiglu(M, N, K); };
    add(f + "as it is", form, base(), none, R_OK);
    // M in 1 .. 16
    add(f + "M=0", form, base(0), none, R_M);
    add(f + "M=1", form, base(1), none, R_OK);
    add(f + "M=16", form, base(16), none, R_OK);
    add(f + "M=17", form, base(17), none, R_M);
    add(f + "M=-1", form, base(-1), none, R_M);
    // N a positive multiple of 16
    add(f + "N=0", form, base(8, 0), none, R_N);
    add(f + "N=8", form, base(8, 8), none, R_N);
    add(f + "N=16", form, base(8, 16), none, R_OK);
    add(f + "N=24", form, base(8, 24), none, R_N);
    add(f + "N=32", form, base(8, 32), none, R_OK);
    // K a positive multiple of 8
    add(f + "K=0", form, base(8, 48, 0), none, R_K);
    add(f + "K=8", form, base(8, 48, 8), none, R_OK);
    add(f + "K=12", form, base(8, 48, 12), [](Operands& o) { o.ldx = o.ldw = 16; }, R_K);
    add(f + "K=16", form, base(8, 48, 16), none, R_OK);
    // strides: at least the row, multiples of 8
    add(f + "ldx=K-8", form, base(), [](Operands& o) { o.ldx = o.K - 8; }, R_LD);
    add(f + "ldx=K+8", form, base(), [](Operands& o) { o.ldx = o.K + 8; }, R_OK);
    add(f + "ldx=K+4", form, base(), [](Operands& o) { o.ldx = o.K + 4; }, R_LD);
    add(f + "ldw=K-8", form, base(), [](Operands& o) { o.ldw = o.K - 8; }, R_LD);
    add(f + "ldw=K+8", form, base(), [](Operands& o) { o.ldw = o.K + 8; }, R_OK);
    add(f + "ldw=K+4", form, base(), [](Operands& o) { o.ldw = o.K + 4; }, R_LD);
    add(f + "ldy=N-8", form, base(), [](Operands& o) { o.ldy = o.N - 8; }, R_LD);
    add(f + "ldy=N+8", form, base(), [](Operands& o) { o.ldy = o.N + 8; }, R_OK);
    add(f + "ldy=N+4", form, base(), [](Operands& o) { o.ldy = o.N + 4; }, R_LD);
    add(f + "strides of 2^40", form, base(), [](Operands& o) { o.ldx = o.ldw = o.ldy = 1ll << 40; }, R_OK);
    // bases: 16-byte aligned, not null
    add(f + "x + 2 bytes", form, base(), [](Operands& o) { o.X += 2; }, R_ALIGN);
    add(f + "x + 16 bytes", form, base(), [](Operands& o) { o.X += 16; }, R_OK);
    add(f + "w + 8 bytes", form, base(), [](Operands& o) { o.W += 8; }, R_ALIGN);
    add(f + "w + 16 bytes", form, base(), [](Operands& o) { o.W += 16; }, R_OK);
    add(f + "y + 2 bytes", form, base(), [](Operands& o) { o.Y += 2; }, R_ALIGN);
    add(f + "y + 16 bytes", form, base(), [](Operands& o) { o.Y += 16; }, R_OK);
    add(f + "x null", form, base(), [](Operands& o) { o.X = 0; }, R_ALIGN);
    add(f + "w null", form, base(), [](Operands& o) { o.W = 0; }, R_ALIGN);
    add(f + "y null", form, base(), [](Operands& o) { o.Y = 0; }, R_ALIGN);
    // the workspace: needed where K is split across workgroups (16 rows of W, 128 k-steps: two pieces), only there
    add(f + "no split, null workspace", form, base(), [](Operands& o) { o.WS = 0; }, R_OK);
    add(f + "no split, K one step short", form, base(8, 16, 4072 - 32), [](Operands& o) { o.WS = 0; }, R_OK);
    add(f + "split, workspace", form, base(8, 16, 4072), none, R_OK);
    add(f + "split, null workspace", form, base(8, 16, 4072), [](Operands& o) { o.WS = 0; }, R_WORKSPACE);
    add(f + "split, workspace + 4 bytes", form, base(8, 16, 4072), [](Operands& o) { o.WS += 4; }, R_WORKSPACE);
    add(f + "split, workspace + 16 bytes", form, base(8, 16, 4072), [](Operands& o) { o.WS += 16; }, R_OK);
    // the first failing condition, in the header's order
    add(f + "M=0 and N=8", form, base(0, 8), none, R_M);
    add(f + "N=8 and K=12", form, base(8, 8, 12), none, R_N);
    add(f + "K=12 and short strides", form, base(8, 48, 12), [](Operands& o) { o.ldx = 8; }, R_K);
    add(f + "short stride and x + 2", form, base(), [](Operands& o) { o.ldw = 8, o.X += 2; }, R_LD);
  }
  // the rows behind W
  add("plain w_rows=N-1", F_PLAIN, plain(), [](Operands& o) { o.w_rows = o.N - 1; }, R_W_ROWS);
  add("plain w_rows=N+1", F_PLAIN, plain(), [](Operands& o) { o.w_rows = o.N + 1; }, R_OK);
  add("swiglu w_rows=2F-1", F_SWIGLU, swiglu(), [](Operands& o) { o.w_rows = 2 * o.N - 1; }, R_W_ROWS);
  add("swiglu w_rows=2F+1", F_SWIGLU, swiglu(), [](Operands& o) { o.w_rows = 2 * o.N + 1; }, R_W_ROWS);
  add("swiglu w_rows=F", F_SWIGLU, swiglu(), [](Operands& o) { o.w_rows = o.N; }, R_W_ROWS);
  add("x + 2 and w_rows short", F_PLAIN, plain(), [](Operands& o) { o.X += 2, o.w_rows = 0; }, R_ALIGN);
  add("w_rows short and null workspace", F_PLAIN, plain(8, 16, 4072), [](Operands& o) { o.w_rows = 0, o.WS = 0; },
      R_W_ROWS);
  // forms
  add("form -1", -1, plain(), [](Operands&) {}, R_FORM);
  add("form 2", F_COUNT, plain(), [](Operands&) {}, R_FORM);
  add("form 2, M=0", F_COUNT, plain(0), [](Operands&) {}, R_FORM);
}

int fails = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::printf("FAIL %s\n", what.c_str());
    ++fails;
  }
}

// (N, K) -> pieces across workgroups, k-steps per wave slice, workspace bytes of the plain form
void plan(int N, int K, int want_split, int want_per, int64_t want_ws) {
  const std::string what = "plan N=" + std::to_string(N) + " K=" + std::to_string(K);
  expect(split(N, K) == want_split, what + " split " + std::to_string(split(N, K)));
  expect(slice_steps(N, K) == want_per, what + " steps per slice " + std::to_string(slice_steps(N, K)));
  expect(ws_bytes(F_PLAIN, N, K) == want_ws, what + " workspace");
  expect(ws_bytes(F_SWIGLU, N, K) == 2 * want_ws, what + " SwiGLU workspace");
  // the slices cover every k-step
  expect((int64_t)slice_steps(N, K) * split(N, K) * WAVES >= ksteps(K), what + " coverage");
}

}  // namespace

int main() {
  static_assert(check(F_PLAIN, Operands{A, A, A, 0, 8, 8, 16, 16, 1, 16, 8}) == R_OK, "constexpr");
  table();
  std::set<int> seen;
  for (const Row& r : rows) {
    const Reason got = check(r.form, r.o);
    seen.insert(r.want);
    expect(got == r.want, r.what + ": got '" + why(got) + "', want '" + why(r.want) + "'");
  }
  for (int r = 0; r < R_COUNT; ++r) {
    expect(seen.count(r) == 1, std::string("no row for reason '") + why(r) + "'");
    expect(std::string(why(r)) != "unknown reason", "reason " + std::to_string(r) + " has no text");
  }
  expect(std::string(why(R_COUNT)) == "unknown reason", "why(R_COUNT)");
  // the Llama-3-8B decode step: no form splits across workgroups (256 row tiles and more)
  plan(6144, 4096, 1, 16, 0);
  plan(4096, 4096, 1, 16, 0);
  plan(14336, 4096, 1, 16, 0);
  plan(4096, 14336, 1, 56, 0);
  plan(128256, 4096, 1, 16, 0);
  // few row tiles: pieces while every wave keeps UNROLL k-steps
  plan(16, 8, 1, 1, 0);
  plan(16, 40, 1, 1, 0);
  plan(48, 520, 1, 3, 0);
  plan(16, 2280, 1, 9, 0);             // 72 k-steps, the last one of 8 columns: a whole pass and a partial one a wave
  plan(16, 4072 - 32, 1, 16, 0);
  plan(16, 4072, 2, 8, 2 * 16 * 16 * 4);
  plan(2048, 2048, 1, 8, 0);           // 128 tiles, 64 k-steps: a split would leave 4 steps a wave
  plan(2048, 8192, 2, 16, 2ll * 16 * 2048 * 4);
  plan(16, 1 << 20, 8, 512, 8 * 16 * 16 * 4);
  plan(4080, 8192, 2, 16, 2ll * 16 * 4080 * 4);   // 255 tiles
  expect(ws_bytes(F_PLAIN, 8, 4096) == 0 && ws_bytes(F_PLAIN, 0, 4096) == 0 && ws_bytes(F_PLAIN, 16, 0) == 0,
         "workspace of a refused shape");
  if (fails) {
    std::printf("gemm skinny selftest: %d FAILED of %zu rows\n", fails, rows.size());
    return 1;
  }
  std::printf("gemm skinny selftest OK (%zu rows)\n", rows.size());
  return 0;
}
