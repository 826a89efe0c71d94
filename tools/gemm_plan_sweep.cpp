// Walks the GEMM planner (get_amd/csrc/gemm_plan.h: Batch's tile choice, the fast-path rule, the two split-K plans with their
// workspace layout, the kernel configuration and the grid) over shape classes on the CPU, checks the invariants the kernels rely
// on, and asserts the plans the project already relies on exactly.  Exits non-zero on any violation.
// Plain host C++:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_sweep.cpp -o gemm_plan_sweep
#include "../get_amd/csrc/gemm_plan.h"
#include <stdio.h>
#include <vector>

using namespace gh;

static long long g_bad = 0;
#define CHECK(cond, ...)                                                             \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (g_bad++ < 20) { printf("VIOLATION %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                                                \
  } while (0)

// operands are never read: aligned addresses of no object
static float* const PTR = reinterpret_cast<float*>(0x10000);
constexpr int NARROW_MASK = 14;      // gemm_batch.h NARROW_DEFAULT
// the split-K part of a registered workspace (gemm_ops.hip make_workspace: the last 1/16 serves the column sums; below 1 MiB: none)
static size_t ws_split_bytes(size_t bytes) {
  if (bytes < (1u << 20)) return 0;
  const size_t tail = (bytes / 16) & ~(size_t)15;
  return (bytes - tail) & ~(size_t)15;
}
static const size_t WS_BYTES[3] = {0, ws_split_bytes((size_t)1 << 20), ws_split_bytes((size_t)256 << 20)};

// ---- what Batch::add does to the launch descriptor (column blocks, row tiles, the longest contraction), without the pointers
struct Built { Launch L; int k_total; bool tn_pp; };
static void start(Built& b) {
  memset(&b.L, 0, sizeof(b.L));
  b.L.ksplit = 1;
  b.k_total = 0;
  b.tn_pp = false;
}
static void push(Built& b, const Problem& q, bool tn, int bm) {
  b.L.p[b.L.nprob++] = q;
  const int bm_eff = row_tile(tn, b.tn_pp, q.elt, bm);
  const int mt = (q.M + bm_eff - 1) / bm_eff;
  if (mt > b.L.m_tiles) b.L.m_tiles = mt;
  if (b.tn_pp && (q.N + 255) / 256 > b.L.n_tiles) b.L.n_tiles = (q.N + 255) / 256;
  if (q.seg[0].K > b.k_total) b.k_total = q.seg[0].K;
}
static Problem nt_problem(int M, int N, int K, int K2, int elt) {
  Problem p = make_problem(M, N, EPI_STORE, PTR, N);
  p.elt = elt;
  p.seg[0] = make_seg_nt(PTR, K, PTR, K + K2, K, nullptr, elt);
  if (K2 > 0) p.seg[p.nseg++] = make_seg_nt(PTR, K2, PTR, K + K2, K2, nullptr, elt);
  return p;
}
static Problem tn_prob(int I, int J, int K, int elt) {      // gemm_batch.h tn_problem
  Problem p = make_problem(I, J, EPI_ATOMIC, PTR, J);
  p.seg[0] = make_seg_tn(PTR, I, I, PTR, J, J, K);
  p.elt = elt;
  if (elt) { p.seg[0].vecA = I % 8 == 0; p.seg[0].vecB = J % 8 == 0; }
  return p;
}
// the launches of ONE product whose output is N columns wide (gh_linear_fwd / gh_linear_bwd: a Batch of its own per product)
static std::vector<Built> linear_launches(bool tn, int M, int N, int K, int bm, int bn) {
  std::vector<Built> out;
  Built b;
  start(b);
  for (int n0 = 0; n0 < N; n0 += bn) {
    const int w = N - n0 < bn ? N - n0 : bn;
    Problem q = tn ? tn_prob(M, N, K, 0) : nt_problem(M, N, K, 0, 0);
    q.N = w;
    if (tn) q.seg[0].vecB = vec_ok(PTR + n0, q.seg[0].ldb, q.N);      // PTR + n0 is a float address: four columns = 16 bytes
    if (b.L.nprob == GH_MAX_PROBLEMS) { out.push_back(b); start(b); }
    push(b, q, tn, bm);
  }
  out.push_back(b);
  return out;
}

// ---- per-configuration statistics
struct Stat { long long plans; int ks_min, ks_max; long long grid_min, grid_max; };
static Stat g_stat[CFG_NCONFIGS];
static const char* const CFG_NAME[CFG_NCONFIGS] = {"32x320", "64x320", "64x160", "128x256 bf16", "256x256 bf16", "TN ping-pong"};
static void book(GemmConfig c, int ks, long long grid) {
  Stat& s = g_stat[c];
  if (s.plans++ == 0) { s.ks_min = s.ks_max = ks; s.grid_min = s.grid_max = grid; }
  if (ks < s.ks_min) s.ks_min = ks;
  if (ks > s.ks_max) s.ks_max = ks;
  if (grid < s.grid_min) s.grid_min = grid;
  if (grid > s.grid_max) s.grid_max = grid;
}
// the configurations launch_cfg (gemm_ops.hip) has a kernel for, for a launch that passed the fast rule
static bool has_kernel(GemmConfig c, bool tn, bool elt) {
  if (c == CFG_TN_PP) return tn && elt;
  if (elt) return c == CFG_64x320 || (!tn && (c == CFG_128x256 || c == CFG_256x256));
  return c == CFG_32x320 || c == CFG_64x320 || c == CFG_64x160;
}
// grid in 64 bits, as the planner's int arithmetic must come out
static long long grid64(const Launch& L, bool tn, bool fast) {
  const long long n_outer = tn ? L.ksplit : L.m_tiles;
  const long long n_inner = tn ? (long long)L.m_tiles * L.nprob : (long long)L.nprob * L.ksplit;
  return nt_few(L, tn, fast) ? n_outer * n_inner : 8 * ((n_outer + 7) / 8) * n_inner;
}
static void check_grid(const Launch& L, bool tn, bool fast, GemmConfig c, const char* what) {
  const long long g = c == CFG_TN_PP ? 8LL * L.per : grid64(L, tn, fast);
  CHECK(g > 0 && g <= 2147483647LL, "%s grid %lld (nprob %d m_tiles %d ksplit %d)", what, g, L.nprob, L.m_tiles, L.ksplit);
  if (c != CFG_TN_PP && g <= 2147483647LL) CHECK(gemm_grid(L, tn, fast) == g, "%s gemm_grid %d != %lld", what, gemm_grid(L, tn, fast), g);
  book(c, L.ksplit, g);
}

static long long g_tn_not8 = 0, g_tn_ge12 = 0, g_cs_counted_unused = 0, g_elt_few_rows = 0;

// ---- (a) the sweep: weight gradients
static void sweep_tn() {
  const int rows[] = {1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 960, 1023, 1024, 1025, 2500, 4095, 4096, 4097,
                      8191, 8192, 8193, 14208, 16383, 16384, 16385, 24575, 24576, 24577, 32767, 32768, 32769, 96000, 1 << 20, (1 << 21) - 1, 1 << 21};
  const int wI[] = {4, 8, 12, 20, 64, 68, 300, 768, 1024, 3844};      // rows of the output (the weight's)
  const int wJ[] = {4, 8, 12, 36, 160, 256, 300, 320, 768};            // columns of a problem (a column block, or a whole output for ping-pong)
  for (int elt = 0; elt < 2; ++elt)
    for (int I : wI)
      for (int J : wJ) {
        if (elt && (I % 8 || J % 8)) continue;      // gh_linear_wgrad_bf16 / the cell require it of bf16 operands
        for (int K : rows)
          for (int nprob = 1; nprob <= GH_MAX_PROBLEMS; ++nprob)
            for (int w = 0; w < 3; ++w) {
              const bool have_ws = WS_BYTES[w] > 0;
              Built b;
              start(b);
              const Problem p = tn_prob(I, J, K, elt);
              b.tn_pp = tn_pp_ok(p, true, have_ws);
              if (!b.tn_pp && J > 320) continue;      // Batch::add cuts such a problem into column blocks
              for (int i = 0; i < nprob; ++i) push(b, p, true, 64);
              const bool fast = fast_ok(b.L, true);
              for (int cs = 0; cs < 2; ++cs)
                for (int mode = 0; mode < 4; ++mode) {
                  if (elt && mode) continue;      // the bf16 storage pipeline runs in mode 0
                  bool has_cs[GH_MAX_PROBLEMS];
                  for (int i = 0; i < nprob; ++i) has_cs[i] = cs != 0;
                  const TnPlan P = tn_split_plan(b.L, b.tn_pp, b.k_total, has_cs, have_ws, WS_BYTES[w], mode);
                  const int ktile = b.tn_pp ? 64 : elt ? 32 : 16;
                  CHECK(P.kchunk > 0 && P.kchunk % ktile == 0, "TN kchunk %d (K tile %d) I %d J %d K %d nprob %d", P.kchunk, ktile, I, J, K, nprob);
                  CHECK((long long)(P.ksplit - 1) * P.kchunk < K && K <= (long long)P.ksplit * P.kchunk,
                        "TN cover ksplit %d kchunk %d K %d I %d J %d nprob %d elt %d pp %d", P.ksplit, P.kchunk, K, I, J, nprob, elt, (int)b.tn_pp);
                  if (b.tn_pp)
                    CHECK(8LL * P.per >= (long long)nprob * b.L.m_tiles * b.L.n_tiles * P.ksplit, "ping-pong per %d I %d J %d K %d nprob %d", P.per, I, J, K, nprob);
                  if (!elt && !b.tn_pp && P.ksplit >= 12) { ++g_tn_ge12; if (P.ksplit % 8) ++g_tn_not8; }
                  if (P.use_ws) {
                    size_t at = 0;      // regions: the tiles problem by problem, then the column-sum partials: consecutive from 0
                    for (int i = 0; i < nprob; ++i) {
                      CHECK(P.tile_off[i] == at && at % 4 == 0, "workspace tiles of problem %d at %zu, expected %zu", i, P.tile_off[i], at);
                      at += (size_t)P.ksplit * I * J;
                    }
                    for (int i = 0; i < nprob && P.cs_in_launch; ++i) {
                      CHECK(P.cs_off[i] == at && at % 4 == 0, "workspace column sums of problem %d at %zu, expected %zu (I %d ksplit %d)", i, P.cs_off[i], at, I, P.ksplit);
                      at += (size_t)P.ksplit * I;
                    }
                    CHECK(P.used == at && P.need <= WS_BYTES[w], "workspace used %zu floats, regions end at %zu, need %zu of %zu B", P.used, at, P.need, WS_BYTES[w]);
                    if (!P.want_cs || P.cs_in_launch) CHECK(P.used * sizeof(float) == P.need, "workspace used %zu floats != need %zu B", P.used, P.need);
                    else { CHECK(P.used * sizeof(float) < P.need, "need %zu", P.need); ++g_cs_counted_unused; }
                    CHECK(P.reduce_elems > 0, "reduce grid of %d elements", P.reduce_elems);
                  } else {
                    CHECK(!P.cs_in_launch, "column sums in the launch without the workspace");
                  }
                  if (cs == 0 && mode == 0) {
                    Launch L = b.L;
                    L.ksplit = P.ksplit; L.kchunk = P.kchunk; L.per = P.per;
                    const ConfigPlan c = gemm_config(L, true, b.tn_pp, true, false, false, false, mode);
                    if (b.tn_pp && !P.use_ws) continue;      // Batch::flush refuses it: no launch
                    if (fast) CHECK(has_kernel(c.cfg, true, elt != 0), "TN configuration %d elt %d", (int)c.cfg, elt);
                    L.m_tiles = c.m_tiles;
                    check_grid(L, true, fast, c.cfg, "TN");
                  }
                }
            }
      }
}

// ---- (a) the sweep: NT launches
static void sweep_nt() {
  const int rows[] = {1, 3, 7, 31, 32, 33, 64, 95 * 32, 96 * 32, 97 * 32, 95 * 64, 96 * 64, 8191, 8192, 8193, 14208, 16383, 16384, 16385, 24575, 24576,
                      24577, 32767, 32768, 32769, 96000, 1 << 20, (1 << 21) - 1, 1 << 21};
  const int Ks[] = {1, 3, 4, 16, 17, 20, 32, 33, 64, 65, 68, 300, 768, 3556, 6272, 8192};
  const int Ns[] = {4, 12, 36, 160, 256, 300, 320};
  for (int M : rows)
    for (int wide_bf16 = 0; wide_bf16 < 2; ++wide_bf16)
      for (int elt = 0; elt < 2; ++elt) {
        if (wide_bf16 && !elt) continue;      // Batch's promise: wide_bf16 => every problem holds bf16
        for (int site = 0; site <= 7; site += (site == 1 ? 2 : 1) * (site == 3 ? 4 : 1))      // 0, 1, 3, 7: never, unset bit, set bit, unset bit
          for (int mode = 0; mode < 4; ++mode) {
            if (elt && mode) continue;
            for (int N : Ns) {
              if (wide_bf16 && N % 256) continue;
              if (elt && N % 8) continue;
              const TilePlan t = tile_plan(false, M, wide_bf16 != 0, site, N, mode, NARROW_MASK);
              CHECK(t.bm > 0 && t.bn > 0 && (!t.narrow || !t.wide) && (!t.wide256 || t.wide), "tile bm %d bn %d", t.bm, t.bn);
              if (N > t.bn) continue;      // (a column block)
              for (int K : Ks) {
                if (elt && K % 8) continue;
                for (int K2 = 0; K2 <= K; K2 += K) {
                  for (int nprob = 1; nprob <= GH_MAX_PROBLEMS; ++nprob) {
                    Built b;
                    start(b);
                    const Problem p = nt_problem(M, N, K, K2, elt);
                    for (int i = 0; i < nprob; ++i) push(b, p, false, t.bm);
                    const bool fast = fast_ok(b.L, false);
                    for (int w = 0; w < 3; ++w) {
                      Launch L = b.L;
                      const NtSplitPlan S = nt_split_plan(L, WS_BYTES[w] > 0, WS_BYTES[w]);
                      if (S.ok) {
                        CHECK(S.ks >= 2 && (long long)(S.ks - 1) * S.ct < S.tmax && S.tmax <= (long long)S.ks * S.ct, "NT split ks %d ct %d tmax %d", S.ks, S.ct, S.tmax);
                        CHECK(S.need <= WS_BYTES[w] && S.finish_grid > 0, "NT split need %zu of %zu, finish grid %d", S.need, WS_BYTES[w], S.finish_grid);
                        size_t at = 0;
                        for (int i = 0; i < nprob; ++i) { CHECK(S.off[i] == at && at % 4 == 0, "NT split tiles of problem %d at %zu", i, S.off[i]); at += (size_t)S.ks * M * N; }
                        CHECK(at * sizeof(float) == S.need, "NT split regions end at %zu floats, need %zu B", at, S.need);
                        L.ksplit = S.ks; L.kchunk = 16 * S.ct;
                      }
                      const ConfigPlan c = gemm_config(L, false, false, t.big, t.narrow, t.wide, t.wide256, mode);
                      CHECK(c.m_tiles > 0, "m_tiles %d", c.m_tiles);
                      if (fast) {
                        if (elt && !t.big) ++g_elt_few_rows;      // (no Batch in the layers does this: bf16 problems come with activation-sized row hints)
                        else CHECK(has_kernel(c.cfg, false, elt != 0), "NT configuration %s elt %d rows %d", CFG_NAME[c.cfg], elt, M);
                      }
                      L.m_tiles = c.m_tiles;
                      check_grid(L, false, fast, c.cfg, "NT");
                    }
                  }
                }
              }
            }
          }
      }
}

// ---- (b) the plans the project relies on, exactly
static int g_named = 0;
#define EXPECT(what, got, want)                                                                              \
  do {                                                                                                       \
    ++g_named;                                                                                               \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                           \
    if (g_ != w_) { ++g_bad; printf("NAMED PLAN %s: %s = %lld, expected %lld\n", what, #got, g_, w_); }     \
  } while (0)

static const size_t WS_DEFAULT = WS_BYTES[2];      // get_amd/_lib.py ensure_workspace: 256 MiB

// one NT product of gh_linear_fwd (M, N, K) = (m, n, k) or of gh_linear_bwd's dX (m, k, n): Batch(false, m, s)
struct NtWant { int m, n, k; int launches, nprob0, cfg, m_tiles, ks, finish_split; };      // ks = 1: unsplit (finish_split unused)
static void named_nt(const char* what, const NtWant& w, size_t ws_bytes = WS_DEFAULT) {
  const TilePlan t = tile_plan(false, w.m, false, 0, 0, 0, NARROW_MASK);
  std::vector<Built> ls = linear_launches(false, w.m, w.n, w.k, t.bm, t.bn);
  EXPECT(what, ls.size(), w.launches);
  Launch L = ls[0].L;
  EXPECT(what, L.nprob, w.nprob0);
  const NtSplitPlan S = nt_split_plan(L, ws_bytes > 0, ws_bytes);
  EXPECT(what, S.ok ? S.ks : 1, w.ks);
  if (S.ok) { EXPECT(what, S.finish_split, w.finish_split); L.ksplit = S.ks; L.kchunk = 16 * S.ct; }
  const ConfigPlan c = gemm_config(L, false, false, t.big, t.narrow, t.wide, t.wide256, 0);
  EXPECT(what, c.cfg, w.cfg);
  EXPECT(what, c.m_tiles, w.m_tiles);
}
// the dW product of gh_linear_bwd for y[m][n] = x[m][k] w[n][k]^T: output [n][k], contracted over m; Batch(true, m, s)
struct TnWant { int m, k, n; int launches, nprob0, m_tiles, ksplit, kchunk, use_ws; };
static void named_tn(const char* what, const TnWant& w, size_t ws_bytes = WS_DEFAULT) {
  const TilePlan t = tile_plan(true, w.m, false, 0, 0, 0, NARROW_MASK);
  std::vector<Built> ls = linear_launches(true, w.n, w.k, w.m, t.bm, t.bn);
  EXPECT(what, ls.size(), w.launches);
  const Launch& L = ls[0].L;
  EXPECT(what, L.nprob, w.nprob0);
  EXPECT(what, L.m_tiles, w.m_tiles);
  bool has_cs[GH_MAX_PROBLEMS] = {};
  const TnPlan P = tn_split_plan(L, false, ls[0].k_total, has_cs, ws_bytes > 0, ws_bytes, 0);
  EXPECT(what, P.ksplit, w.ksplit);
  EXPECT(what, P.kchunk, w.kchunk);
  EXPECT(what, P.use_ws, w.use_ws);
}

static void named_plans() {
  const int C32 = CFG_32x320, C64 = CFG_64x320;
  // tests/test_gpu_gemm_paths.py FWD_FAST: (m, k, n) there is {m, n, k} here
  named_nt("fwd (7, 20, 12)", {7, 12, 20, 1, 1, C32, 1, 1, 0});
  named_nt("fwd (64, 4, 12)", {64, 12, 4, 1, 1, C32, 2, 1, 0});
  named_nt("fwd (33, 128, 16)", {33, 16, 128, 1, 1, C32, 2, 2, 0});
  named_nt("fwd (960, 300, 300)", {960, 300, 300, 1, 1, C32, 30, 4, 0});
  named_nt("fwd (3, 960, 300)", {3, 300, 960, 1, 1, C32, 1, 15, 0});
  named_nt("fwd (3, 1024, 300)", {3, 300, 1024, 1, 1, C32, 1, 16, 1});
  named_nt("fwd (4, 2048, 772)", {4, 772, 2048, 1, 3, C32, 1, 32, 1});
  named_nt("fwd (32, 3556, 300)", {32, 300, 3556, 1, 1, C32, 1, 45, 1});
  named_nt("fwd (32, 4096, 768)", {32, 768, 4096, 1, 3, C32, 1, 64, 1});
  named_nt("fwd (257, 68, 324)", {257, 324, 68, 1, 2, C32, 9, 1, 0});
  named_nt("fwd (5, 8, 3844)", {5, 3844, 8, 2, 12, C32, 1, 1, 0});
  named_nt("fwd (8200, 20, 16)", {8200, 16, 20, 1, 1, C32, 257, 1, 0});      // the occupancy rule: 129 tiles of 64 rows -> 257 of 32
  named_nt("fwd (8200, 20, 960)", {8200, 960, 20, 1, 3, C64, 129, 1, 0});
  named_nt("fwd (2500, 32, 24)", {2500, 24, 32, 1, 1, C32, 79, 1, 0});
  named_nt("fwd (260, 4, 1024)", {260, 1024, 4, 1, 4, C32, 9, 1, 0});
  // ... test_fwd_split_plan_refused_for_lack_of_workspace: none, or 1 MiB
  named_nt("fwd (32, 3556, 300) no workspace", {32, 300, 3556, 1, 1, C32, 1, 1, 0}, 0);
  named_nt("fwd (32, 3556, 300) 1 MiB", {32, 300, 3556, 1, 1, C32, 1, 1, 0}, WS_BYTES[1]);
  named_nt("fwd (960, 300, 300) 1 MiB", {960, 300, 300, 1, 1, C32, 30, 1, 0}, WS_BYTES[1]);
  // BWD_OF_FWD / BWD_TN, dX: (M, N, K) = (m, k, n)
  named_nt("dx (960, 300, 300)", {960, 300, 300, 1, 1, C32, 30, 4, 0});
  named_nt("dx (3, 960, 300)", {3, 960, 300, 1, 3, C32, 1, 4, 0});
  named_nt("dx (3, 1024, 300)", {3, 1024, 300, 1, 4, C32, 1, 4, 0});
  named_nt("dx (4, 2048, 772)", {4, 2048, 772, 1, 7, C32, 1, 10, 0});
  named_nt("dx (32, 3556, 300)", {32, 3556, 300, 1, 12, C32, 1, 4, 0});
  named_nt("dx (32, 4096, 768)", {32, 4096, 768, 2, 12, C32, 1, 12, 0});
  named_nt("dx (257, 68, 324)", {257, 68, 324, 1, 1, C32, 9, 5, 0});
  named_nt("dx (5, 8, 3844)", {5, 8, 3844, 1, 1, C32, 1, 49, 1});
  named_nt("dx (8200, 20, 16)", {8200, 20, 16, 1, 1, C32, 257, 1, 0});
  named_nt("dx (260, 4, 1024)", {260, 4, 1024, 1, 1, C32, 9, 16, 1});
  // dW: {m, k, n, launches, problems of the first, row tiles, chunks, rows per chunk, partial tiles in the workspace}
  named_tn("dw (960, 300, 300)", {960, 300, 300, 1, 1, 5, 3, 320, 1});
  named_tn("dw (4, 2048, 772)", {4, 2048, 772, 1, 7, 13, 1, 16, 0});
  named_tn("dw (32, 3556, 300)", {32, 3556, 300, 1, 12, 5, 1, 32, 0});
  named_tn("dw (32, 4096, 768)", {32, 4096, 768, 2, 12, 12, 1, 32, 0});
  named_tn("dw (5, 8, 3844)", {5, 8, 3844, 1, 1, 61, 1, 16, 0});
  named_tn("dw (8200, 20, 16)", {8200, 20, 16, 1, 1, 1, 24, 352, 1});
  named_tn("dw (8200, 20, 960)", {8200, 20, 960, 1, 1, 15, 24, 352, 1});
  named_tn("dw (8200, 6, 962)", {8200, 6, 962, 1, 1, 16, 24, 352, 0});      // generic kernel: n % 4 -> atomics whatever the workspace
  named_tn("dw (2500, 32, 24)", {2500, 32, 24, 1, 1, 1, 9, 288, 1});
  named_tn("dw (4000, 16, 12)", {4000, 16, 12, 1, 1, 1, 16, 256, 1});
  named_tn("dw (8448, 12, 20)", {8448, 12, 20, 1, 1, 1, 32, 272, 1});
  named_tn("dw (5, 3844, 12)", {5, 3844, 12, 2, 12, 1, 1, 16, 0});
  named_tn("dw (2500, 30, 22)", {2500, 30, 22, 1, 1, 1, 9, 288, 0});
  named_tn("dw (260, 4, 1024)", {260, 4, 1024, 1, 1, 16, 1, 272, 0});

  // the bench step: 96 000 activation rows x 300 take the narrow tile at the call sites 2 - 4 of NARROW_DEFAULT alone ...
  for (int site = 0; site <= 7; ++site) {
    const TilePlan t = tile_plan(false, 96000, false, site, 300, 0, NARROW_MASK);
    EXPECT("96000 rows x 300", t.narrow, site >= 2 && site <= 4);
    EXPECT("96000 rows x 300", t.bn, site >= 2 && site <= 4 ? 160 : 320);
    EXPECT("96000 rows x 300", t.bm, 64);
    // ... realistic evidence counts (14 208 rows: thin) at every call site, and never in another GEMM mode
    EXPECT("14208 rows x 300", tile_plan(false, 14208, false, site, 300, 0, NARROW_MASK).narrow, site > 0);
    EXPECT("14208 rows x 300, mode 1", tile_plan(false, 14208, false, site, 300, 1, NARROW_MASK).narrow, 0);
    // h = 768 in fp32: 160-column blocks cover 768 columns with less padding (800 against 960)
    EXPECT("96000 rows x 768", tile_plan(false, 96000, false, site, 768, 0, NARROW_MASK).narrow, site > 0);
  }
  // ... bf16 storage, h = 768: the 256 x 256 tile from 32 768 rows, the 128 x 256 tile below
  EXPECT("bf16 96000 rows", tile_plan(false, 96000, true, 1, 768, 0, NARROW_MASK).bm, 256);
  EXPECT("bf16 14208 rows", tile_plan(false, 14208, true, 1, 768, 0, NARROW_MASK).bm, 128);
  // ... and a cell's seven 768 x 768 weight gradients over 96 000 rows: 63 ping-pong tiles x 4 chunks = 252 of 256 workgroups
  {
    Built b;
    start(b);
    const Problem p = tn_prob(768, 768, 96000, 1);
    b.tn_pp = tn_pp_ok(p, true, true);
    EXPECT("h = 768 dW", b.tn_pp, 1);
    for (int i = 0; i < 7; ++i) push(b, p, true, 64);
    bool has_cs[GH_MAX_PROBLEMS] = {};
    const TnPlan P = tn_split_plan(b.L, b.tn_pp, b.k_total, has_cs, true, WS_DEFAULT, 0);
    EXPECT("h = 768 dW", b.L.m_tiles * b.L.n_tiles * b.L.nprob, 63);
    EXPECT("h = 768 dW", P.ksplit, 4);
    EXPECT("h = 768 dW", P.kchunk, 24000);
    EXPECT("h = 768 dW", P.per, 32);
    EXPECT("h = 768 dW", P.use_ws, 1);
  }
}

int main() {
  sweep_tn();
  sweep_nt();
  named_plans();
  for (int c = 0; c < CFG_NCONFIGS; ++c) {
    const Stat& s = g_stat[c];
    if (s.plans) printf("%-14s %9lld plans  ksplit %d .. %d  grid %lld .. %lld\n", CFG_NAME[c], s.plans, s.ks_min, s.ks_max, s.grid_min, s.grid_max);
    else printf("%-14s         0 plans\n", CFG_NAME[c]);
  }
  printf("fp32 TN plans with ksplit >= 12: %lld, of them not a multiple of 8: %lld (information)\n", g_tn_ge12, g_tn_not8);
  printf("TN plans whose workspace need counts column-sum partials the launch does not carry: %lld (information)\n", g_cs_counted_unused);
  printf("bf16 problems on a few-row Batch (no kernel on the 32 x 320 tile; no layer builds one): %lld (information)\n", g_elt_few_rows);
  printf("named plans: %d values asserted\n", g_named);
  printf("%s\n", g_bad ? "VIOLATIONS" : "no violation");
  return g_bad ? 1 : 0;
}
