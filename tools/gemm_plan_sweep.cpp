// Walks the GEMM planner (get_amd/csrc/gemm_plan.h: Batch's tile choice, the fast-path rule, the two split-K plans with their
// workspace layout, the kernel configuration and the grid) over shape classes on the CPU, checks the invariants the kernels rely
// on, and asserts the plans the project already relies on exactly, among them every launch of the GGNN cell entries
// for the cases of tests/test_gpu_cell_paths.py.  Exits non-zero on any violation.  With an argument it also prints
// the cell cases' launches.
// Plain host C++:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_sweep.cpp -o gemm_plan_sweep
#include "../get_amd/csrc/gemm_plan.h"
#include <stdio.h>
#include <string>
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

// ---- (c) the launches of the GGNN cell entries (cell_ops.hip cell_fwd_impl / cell_bwd_impl as the public entries call them: one
// stream, no fused next cell, no second row buffer), for every case of tests/test_gpu_cell_paths.py.  A launch is written as
//   NT:  <tile> [xK(T)F] fast|generic pN tM      K chunks of T K tiles and nt_finish_kernel's shape F (1 = a workgroup per row)
//   TN:  TN kK*R ws|atomic cs+|cs-|-- fast|generic pN      K chunks of R rows; partial tiles in the workspace or atomics; column
//        sums fused into the launch (cs+), wanted but left to launch_colsum3 (cs-), not wanted (--)
// and a call as its launches in order.  NULL_ / MIS: an aligned address and one a float past a 16-byte boundary.
static float* const MIS = PTR + 1;
struct CellCase {
  int M, seg0, din, h;          // rows of the launches; seg0 > 0: node-compact with padding rows (Problem::seg0_rows)
  int ids, drop, score, sdrop;  // forward: gathered rows, input dropout, fused scorer projection (and its dropout)
  int mode;                     // GEMM mode
  size_t ws;                    // split-K bytes of the workspace (0: none)
  int mis;                      // forward: 0 none, 1 w_z0, 2 b_r0, 3 xp, 4 out; backward: 1 = x / the table
  int elt;                      // bf16 storage entries
};
static void add_blocks(Built& b, const Problem& p, bool tn, int bm, int bn) {
  for (int n0 = 0; n0 < p.N; n0 += bn) {      // Batch::add: a block's pointers move by multiples of 4 floats, its alignment stays
    Problem q = p;
    q.N = p.N - n0 < bn ? p.N - n0 : bn;
    if (tn) q.seg[0].vecB = q.elt ? (al16(q.seg[0].B) && q.seg[0].ldb % 8 == 0 && q.N % 8 == 0) : vec_ok(q.seg[0].B, q.seg[0].ldb, q.N);
    push(b, q, tn, bm);
  }
}
static std::string nt_line(Built& b, const TilePlan& t, bool narrow, int mode, size_t ws) {
  Launch L = b.L;
  const NtSplitPlan S = nt_split_plan(L, ws > 0, ws);
  if (S.ok) { L.ksplit = S.ks; L.kchunk = 16 * S.ct; }
  const ConfigPlan c = gemm_config(L, false, false, t.big, narrow, t.wide, t.wide256, mode);
  char buf[128];
  int n = snprintf(buf, sizeof(buf), "%s", CFG_NAME[c.cfg]);
  if (S.ok) n += snprintf(buf + n, sizeof(buf) - n, " x%d(%d)%d", S.ks, S.ct, S.finish_split);
  snprintf(buf + n, sizeof(buf) - n, " %s p%d t%d", fast_ok(b.L, false) ? "fast" : "generic", L.nprob, c.m_tiles);
  return buf;
}
static std::string tn_line(Built& b, const bool* has_cs, int mode, size_t ws) {
  const TnPlan P = tn_split_plan(b.L, b.tn_pp, b.k_total, has_cs, ws > 0, ws, mode);
  char buf[128];
  snprintf(buf, sizeof(buf), "TN%s k%d*%d %s %s %s p%d", b.tn_pp ? " ping-pong" : "", P.ksplit, P.kchunk,
           (b.tn_pp && !P.use_ws) ? "refused" : P.use_ws ? "ws" : "atomic", P.want_cs ? (P.cs_in_launch ? "cs+" : "cs-") : "--", fast_ok(b.L, true) ? "fast" : "generic", b.L.nprob);
  return buf;
}
static Problem cell_nt(const CellCase& c, int N, int epi, float* C, const float* A, int lda, const float* B, int K, const int32_t* gather = nullptr) {
  Problem p = make_problem(c.M, N, epi, C, N);
  p.elt = c.elt;
  p.seg[0] = make_seg_nt(A, lda, B, K, K, gather, c.elt);
  return p;
}
static std::string cell_fwd_lines(const CellCase& c) {
  const int h = c.h, din = c.din;
  float* xp = c.mis == 3 ? MIS : PTR;
  static const int32_t* const IDS = reinterpret_cast<const int32_t*>(0x20000);
  const bool wide = c.elt && h % 256 == 0;
  std::string out;
  {  // xp = dropout(x) Wp^T
    const TilePlan t = tile_plan(false, c.M, wide, 7, h, c.mode, NARROW_MASK);
    Built b; start(b);
    Problem p = cell_nt(c, h, EPI_STORE, xp, PTR, din, PTR, din, c.ids ? IDS : nullptr);
    if (c.drop) p.drop_mode = 1;
    add_blocks(b, p, false, t.bm, t.bn);
    out += nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  {  // z, r
    const TilePlan t = tile_plan(false, c.M, wide, 1, h, c.mode, NARROW_MASK);
    Built b; start(b);
    Problem pz = cell_nt(c, h, EPI_SIGMOID_Z, PTR, PTR, h, c.mis == 1 ? MIS : PTR, h);
    pz.seg[pz.nseg++] = make_seg_nt(xp, h, PTR, h, h, nullptr, c.elt);
    pz.bias = PTR; pz.bias2 = PTR;
    Problem pr = cell_nt(c, h, EPI_SIGMOID_R, PTR, PTR, h, PTR, h);
    pr.seg[pr.nseg++] = make_seg_nt(xp, h, PTR, h, h, nullptr, c.elt);
    pr.bias = c.mis == 2 ? MIS : PTR; pr.bias2 = PTR; pr.out1 = PTR; pr.in0 = xp;
    pz.seg0_rows = pr.seg0_rows = c.seg0;
    add_blocks(b, pz, false, t.bm, t.bn);
    add_blocks(b, pr, false, t.bm, t.bn);
    out += " | " + nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  {  // h gate, the convex update and the scorer projection
    TilePlan t = tile_plan(false, c.M, wide && !c.score, 2, h, c.mode, NARROW_MASK);
    if (c.score && t.narrow && h > 2 * t.bn) { t.narrow = false; t.bn = 320; }
    Built b; start(b);
    Problem ph = cell_nt(c, h, EPI_TANH_H, PTR, PTR, h, PTR, h);
    ph.seg[ph.nseg++] = make_seg_nt(PTR, h, PTR, h, h, nullptr, c.elt);
    ph.bias = PTR; ph.bias2 = PTR; ph.out1 = c.mis == 4 ? MIS : PTR; ph.in0 = PTR; ph.in1 = xp;
    ph.seg0_rows = c.seg0;
    if (c.score) { ph.w2 = PTR; ph.e = PTR; if (c.sdrop) ph.drop_mode = 2; }
    if (c.score && h > t.bn && !(t.narrow && h <= 2 * t.bn)) return out + " | refused";      // Batch::add: whole rows only
    add_blocks(b, ph, false, t.bm, t.bn);
    out += " | " + nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  return out;
}
// dx: the caller wants the input gradient; else (with ids) the re-associated path when cell_bwd_impl's conditions hold
static std::string cell_bwd_lines(const CellCase& c, bool dx) {
  const int h = c.h, din = c.din, M = c.M;
  const bool wide = c.elt && h % 256 == 0;
  static const int32_t* const IDS = reinterpret_cast<const int32_t*>(0x20000);
  const float* x = c.mis == 1 ? MIS : PTR;
  const size_t ts_bytes = 20 * (size_t)h * din;
  // (the workspace as registered: ws is its split-K part, 15/16 of it)
  const bool nodx = !dx && !c.elt && din <= h && din % 4 == 0 && h % 4 == 0 && c.ws > 0 && c.ws / 2 >= ts_bytes;
  std::string out;
  auto tn = [&](int I, int J, const float* B, const int32_t* gatherB) {
    Problem p = make_problem(I, J, EPI_ATOMIC, PTR, J);
    p.seg[0] = make_seg_tn(PTR, I, I, B, J, J, M, nullptr, gatherB);
    p.elt = c.elt;
    if (c.elt) { p.seg[0].vecA = I % 8 == 0; p.seg[0].vecB = al16(B) && J % 8 == 0; }
    return p;
  };
  if (nodx) {
    const size_t ws_left = c.ws - ts_bytes;
    {
      const TilePlan t = tile_plan(false, M, false, 3, h, c.mode, NARROW_MASK);
      Built b; start(b);
      Problem p1 = cell_nt(c, h, EPI_BWD_DRX, PTR, PTR, h, PTR, h);
      p1.out1 = PTR; p1.in0 = PTR; p1.in1 = PTR;
      add_blocks(b, p1, false, t.bm, t.bn);
      out += nt_line(b, t, t.narrow, c.mode, c.ws);
    }
    const float* X = (c.ids || c.drop) ? PTR : x;
    {
      Built b; start(b);
      bool has_cs[GH_MAX_PROBLEMS] = {};
      const Problem ps[4] = {tn(h, din, X, nullptr), tn(h, din, X, nullptr), tn(h, h, PTR, nullptr), tn(h, din, X, nullptr)};
      for (int i = 0; i < 4; ++i) { add_blocks(b, ps[i], true, 64, 320); if (i < 3) has_cs[b.L.nprob - 1] = true; }
      out += " | " + tn_line(b, has_cs, c.mode, ws_left);
    }
    {
      Built b; start(b);
      bool has_cs[GH_MAX_PROBLEMS] = {};
      for (int i = 0; i < 3; ++i) add_blocks(b, tn(h, din, PTR, nullptr), true, 64, 320);
      out += " | " + tn_line(b, has_cs, c.mode, ws_left);
    }
    return out;
  }
  {  // da = dhp Wh0 ; d(r xp) = dhp Wh1
    const TilePlan t = tile_plan(false, M, wide, 3, h, c.mode, NARROW_MASK);
    Built b; start(b);
    Problem p0 = cell_nt(c, h, EPI_STORE, PTR, PTR, h, PTR, h);
    Problem p1 = cell_nt(c, h, EPI_BWD_DRX, PTR, PTR, h, PTR, h);
    p1.out1 = PTR; p1.in0 = PTR; p1.in1 = PTR;
    add_blocks(b, p0, false, t.bm, t.bn);
    add_blocks(b, p1, false, t.bm, t.bn);
    out += nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  {  // da += dzp Wz0 + drp Wr0 ; dxp += dzp Wz1 + drp Wr1
    const TilePlan t = tile_plan(false, M, wide, 4, h, c.mode, NARROW_MASK);
    Built b; start(b);
    for (int i = 0; i < 2; ++i) {
      Problem p = cell_nt(c, h, EPI_STORE, PTR, PTR, h, PTR, h);
      p.seg[p.nseg++] = make_seg_nt(PTR, h, PTR, h, h, nullptr, c.elt);
      p.accumulate = 1;
      add_blocks(b, p, false, t.bm, t.bn);
    }
    out += " | " + nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  if (dx) {
    const TilePlan t = tile_plan(false, M, wide && din % 256 == 0, 5, din, c.mode, NARROW_MASK);
    Built b; start(b);
    Problem p = cell_nt(c, din, EPI_STORE, PTR, PTR, h, PTR, h);
    p.io = 0;
    if (c.drop) p.drop_mode = 3;
    add_blocks(b, p, false, t.bm, t.bn);
    out += " | " + nt_line(b, t, t.narrow, c.mode, c.ws);
  }
  {  // the seven weight gradients in one Batch
    std::string lines;
    Built b; start(b);
    bool has_cs[GH_MAX_PROBLEMS] = {};
    const bool cs = c.elt ? true : h % 4 == 0;
    auto flush = [&]() { lines += " | " + tn_line(b, has_cs, c.mode, c.ws); start(b); for (bool& v : has_cs) v = false; };
    auto add = [&](const Problem& p, bool want) {
      const bool pp = tn_pp_ok(p, true, c.ws > 0);
      if (b.L.nprob > 0 && pp != b.tn_pp) flush();      // (a launch is one kernel)
      for (int n0 = 0; n0 < p.N; n0 += pp ? (1 << 30) : 320) {
        if (b.L.nprob == GH_MAX_PROBLEMS) flush();
        Problem q = p;
        q.N = pp ? p.N : (p.N - n0 < 320 ? p.N - n0 : 320);
        if (!c.elt) q.seg[0].vecB = vec_ok(q.seg[0].B, q.seg[0].ldb, q.N);
        b.tn_pp = pp;
        push(b, q, true, 64);
      }
      if (want) has_cs[b.L.nprob - 1] = true;
    };
    for (int i = 0; i < 6; ++i) add(tn(h, h, PTR, nullptr), cs && i % 2 == 0);
    const bool gathered = (c.ids || c.drop || c.elt) && din <= h;      // operand rows materialised by gather_rows into `da`
    add(tn(h, din, gathered ? PTR : x, (!gathered && c.ids) ? IDS : nullptr), false);
    flush();
    out += lines;
  }
  return out;
}
struct CellWant { const char* name; CellCase c; int bwd; const char* want; };      // bwd: 0 forward, 1 backward with dx, 2 without
static void named_cell_plans(bool print) {
  const size_t W = WS_DEFAULT, W1 = WS_BYTES[1];
  static const CellWant wants[] = {
    {"fwd (3,20,8,8) x", {60,0,8,8,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,8,8) ids drop", {60,0,8,8,1,1,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,12,20) x", {60,0,12,20,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,12,20) ids drop", {60,0,12,20,1,1,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,12,20) x fp32x3p", {60,0,12,20,0,0,0,0,3,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"fwd (2,100,64,64) split", {200,0,64,64,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 x2(4)0 fast p1 t7"},
    {"fwd (2,100,64,64) split fp32x3p", {200,0,64,64,0,0,0,0,3,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 x2(4)0 fast p1 t7"},
    {"fwd (2,100,300,300) split", {200,0,300,300,0,0,0,0,0,W,0,0}, 0,
     "32x320 x4(5)0 fast p1 t7 | 32x320 x8(5)0 fast p2 t7 | 32x320 x8(5)0 fast p1 t7"},
    {"fwd (3,20,64,512) split", {60,0,64,512,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p2 t2 | 32x320 x16(4)1 fast p4 t2 | 32x320 x16(4)1 fast p2 t2"},
    {"fwd (2,100,64,64) compact", {200,133,64,64,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 fast p2 t7 | 32x320 fast p1 t7"},
    {"fwd (2,100,64,64) score", {200,0,64,64,0,0,1,1,0,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 fast p1 t7"},
    {"fwd (2,100,64,64) drop", {200,0,64,64,0,1,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 x2(4)0 fast p1 t7"},
    {"fwd (2,100,300,300) drop", {200,0,300,300,0,1,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t7 | 32x320 x8(5)0 fast p2 t7 | 32x320 x8(5)0 fast p1 t7"},
    {"fwd (3,20,300,1) generic", {60,0,300,1,0,0,0,0,0,W,0,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,6,6) generic", {60,0,6,6,0,0,0,0,0,W,0,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,12,30) generic", {60,0,12,30,0,0,0,0,0,W,0,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,12,30) generic compact", {60,27,12,30,0,0,0,0,0,W,0,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,8,8) w misaligned", {60,0,8,8,0,0,0,0,0,W,1,0}, 0,
     "32x320 fast p1 t2 | 32x320 generic p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,8,8) bias misaligned", {60,0,8,8,0,0,0,0,0,W,2,0}, 0,
     "32x320 fast p1 t2 | 32x320 generic p2 t2 | 32x320 fast p1 t2"},
    {"fwd (3,20,8,8) xp misaligned", {60,0,8,8,0,0,0,0,0,W,3,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,8,8) out misaligned", {60,0,8,8,0,0,0,0,0,W,4,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,6,6) score", {60,0,6,6,0,0,1,0,0,W,0,0}, 0,
     "32x320 generic p1 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2"},
    {"fwd (3,20,8,480) score", {60,0,8,480,0,0,1,0,0,W,0,0}, 0,
     "32x320 fast p2 t2 | 32x320 x15(4)0 fast p4 t2 | refused"},
    {"fwd (82,100,48,160)", {8200,0,48,160,0,0,0,0,0,W,0,0}, 0,
     "64x160 fast p1 t129 | 64x160 fast p2 t129 | 64x160 fast p1 t129"},
    {"fwd (82,100,300,300)", {8200,0,300,300,0,0,0,0,0,W,0,0}, 0,
     "64x160 fast p2 t129 | 64x160 fast p4 t129 | 64x160 fast p2 t129"},
    {"fwd (82,100,300,300) fp32x3p", {8200,0,300,300,0,0,0,0,3,W,0,0}, 0,
     "32x320 fast p1 t257 | 32x320 fast p2 t257 | 32x320 fast p1 t257"},
    {"fwd (120,100,48,160) fp32x3p", {12000,0,48,160,0,0,0,0,3,W,0,0}, 0,
     "32x320 fast p1 t375 | 64x320 fast p2 t188 | 32x320 fast p1 t375"},
    {"fwd (82,100,300,300) score", {8200,0,300,300,0,0,1,1,0,W,0,0}, 0,
     "64x160 fast p2 t129 | 64x160 fast p4 t129 | 64x160 fast p2 t129"},
    {"fwd (82,100,300,300) score compact 8192", {8192,7868,300,300,0,0,1,1,0,W,0,0}, 0,
     "64x160 fast p2 t128 | 64x160 fast p4 t128 | 64x160 fast p2 t128"},
    {"fwd (82,100,300,300) score compact 8198", {8198,7868,300,300,0,0,1,1,0,W,0,0}, 0,
     "64x160 fast p2 t129 | 64x160 fast p4 t129 | 64x160 fast p2 t129"},
    {"fwd (82,100,48,160) compact 8192", {8192,7868,48,160,0,0,0,0,0,W,0,0}, 0,
     "64x160 fast p1 t128 | 64x160 fast p2 t128 | 64x160 fast p1 t128"},
    {"fwd (250,100,300,300)", {25000,0,300,300,0,0,0,0,0,W,0,0}, 0,
     "64x320 fast p1 t391 | 64x320 fast p2 t391 | 64x160 fast p2 t391"},
    {"fwd (251,100,300,300)", {25100,0,300,300,0,0,0,0,0,W,0,0}, 0,
     "64x320 fast p1 t393 | 32x320 fast p2 t785 | 64x160 fast p2 t393"},
    {"fwd (82,100,300,300) compact 3718", {3718,0,300,300,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t117 | 32x320 fast p2 t117 | 32x320 fast p1 t117"},
    {"fwd (82,100,300,300) compact 8200 of 3718", {8200,3718,300,300,0,0,0,0,0,W,0,0}, 0,
     "64x160 fast p2 t129 | 64x160 fast p4 t129 | 64x160 fast p2 t129"},
    {"fwd (3,20,12,20) compact 27", {27,0,12,20,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t1 | 32x320 fast p2 t1 | 32x320 fast p1 t1"},
    {"fwd (3,20,12,20) compact 60 of 27", {60,27,12,20,0,0,0,0,0,W,0,0}, 0,
     "32x320 fast p1 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2"},
    {"bwd dx (3,20,12,20)", {60,0,12,20,0,0,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (3,20,12,20) fp32x3p", {60,0,12,20,0,0,0,0,3,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (2,100,64,64)", {200,0,64,64,0,0,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 fast p1 t7 | TN k1*208 atomic cs- fast p7"},
    {"bwd dx (2,100,64,64) fp32x3p", {200,0,64,64,0,0,0,0,3,W,0,0}, 1,
     "32x320 fast p2 t7 | 32x320 x2(4)0 fast p2 t7 | 32x320 fast p1 t7 | TN k1*208 atomic cs- fast p7"},
    {"bwd dx (3,20,16,128)", {60,0,16,128,0,0,0,0,0,W,0,0}, 1,
     "32x320 x2(4)0 fast p2 t2 | 32x320 x4(4)0 fast p2 t2 | 32x320 x2(4)0 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (82,100,300,300)", {8200,0,300,300,0,0,0,0,0,W,0,0}, 1,
     "64x160 fast p4 t129 | 64x160 fast p4 t129 | 64x160 fast p2 t129 | TN k24*352 ws cs+ fast p7"},
    {"bwd dx (3,20,12,20) drop", {60,0,12,20,0,1,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (3,20,12,20) ids", {60,0,12,20,1,0,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (3,20,12,20) ids drop table misaligned", {60,0,12,20,1,1,0,0,0,W,1,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (3,20,6,6)", {60,0,6,6,0,0,0,0,0,W,0,0}, 1,
     "32x320 generic p2 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2 | TN k1*64 atomic -- generic p7"},
    {"bwd dx (3,7,6,6) ids", {21,0,6,6,1,0,0,0,0,W,0,0}, 1,
     "32x320 generic p2 t1 | 32x320 generic p2 t1 | 32x320 generic p1 t1 | TN k1*32 atomic -- generic p7"},
    {"bwd dx (3,20,12,30)", {60,0,12,30,0,0,0,0,0,W,0,0}, 1,
     "32x320 generic p2 t2 | 32x320 generic p2 t2 | 32x320 generic p1 t2 | TN k1*64 atomic -- generic p7"},
    {"bwd dx (3,20,20,12) x", {60,0,20,12,0,0,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd dx (3,20,20,12) ids", {60,0,20,12,1,0,0,0,0,W,0,0}, 1,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | 32x320 fast p1 t2 | TN k1*64 atomic cs- generic p7"},
    {"bwd nodx (3,20,12,20)", {60,0,12,20,1,0,0,0,0,W,0,0}, 2,
     "32x320 fast p1 t2 | TN k1*64 atomic cs- fast p4 | TN k1*64 atomic -- fast p3"},
    {"bwd nodx (82,100,300,300)", {8200,0,300,300,1,1,0,0,0,W,0,0}, 2,
     "64x160 fast p2 t129 | TN k24*352 ws cs+ fast p4 | TN k24*352 ws -- fast p3"},
    {"bwd nodx (82,100,48,160)", {8200,0,48,160,1,0,0,0,0,W,0,0}, 2,
     "64x160 fast p1 t129 | TN k24*352 ws cs+ fast p4 | TN k24*352 ws -- fast p3"},
    {"bwd nodx (3,20,20,12) din > h", {60,0,20,12,1,0,0,0,0,W,0,0}, 2,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | TN k1*64 atomic cs- generic p7"},
    {"bwd nodx (3,20,6,8) din % 4", {60,0,6,8,1,0,0,0,0,W,0,0}, 2,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | TN k1*64 atomic cs- generic p7"},
    {"bwd nodx (3,20,12,30) h % 4", {60,0,12,30,1,0,0,0,0,W,0,0}, 2,
     "32x320 generic p2 t2 | 32x320 generic p2 t2 | TN k1*64 atomic -- generic p7"},
    {"bwd nodx (3,20,12,20) no workspace", {60,0,12,20,1,0,0,0,0,0,0,0}, 2,
     "32x320 fast p2 t2 | 32x320 fast p2 t2 | TN k1*64 atomic cs- fast p7"},
    {"bwd nodx (3,20,300,300) 1 MiB", {60,0,300,300,1,0,0,0,0,W1,0,0}, 2,
     "32x320 x4(5)0 fast p2 t2 | 32x320 fast p2 t2 | TN k1*64 atomic cs- fast p7"},
    {"bf16 fwd (82,100,48,160)", {8200,0,48,160,0,0,0,0,0,W,0,1}, 0,
     "64x320 fast p1 t129 | 64x320 fast p2 t129 | 64x320 fast p1 t129"},
    {"bf16 fwd (82,100,256,256)", {8200,0,256,256,0,0,0,0,0,W,0,1}, 0,
     "128x256 bf16 fast p1 t65 | 128x256 bf16 fast p2 t65 | 128x256 bf16 fast p1 t65"},
    {"bf16 fwd (328,100,256,256)", {32800,0,256,256,0,0,0,0,0,W,0,1}, 0,
     "256x256 bf16 fast p1 t129 | 256x256 bf16 fast p2 t129 | 256x256 bf16 fast p1 t129"},
    {"bf16 fwd (328,100,256,256) drop", {32800,0,256,256,0,1,0,0,0,W,0,1}, 0,
     "128x256 bf16 fast p1 t257 | 256x256 bf16 fast p2 t129 | 256x256 bf16 fast p1 t129"},
    {"bf16 fwd (82,100,64,192)", {8200,0,64,192,0,0,0,0,0,W,0,1}, 0,
     "64x320 fast p2 t129 | 64x320 fast p4 t129 | 64x320 fast p2 t129"},
    {"bf16 fwd (90,100,48,160) compact 9000", {9000,8668,48,160,1,0,0,0,0,W,0,1}, 0,
     "64x320 fast p1 t141 | 64x320 fast p2 t141 | 64x320 fast p1 t141"},
    {"bf16 bwd (82,100,48,160)", {8200,0,48,160,0,0,0,0,0,W,0,1}, 1,
     "64x320 fast p2 t129 | 64x320 fast p2 t129 | 64x320 fast p1 t129 | TN k2*4128 ws cs+ fast p7"},
    {"bf16 bwd (82,100,256,256)", {8200,0,256,256,0,0,0,0,0,W,0,1}, 1,
     "128x256 bf16 fast p2 t65 | 128x256 bf16 fast p2 t65 | 128x256 bf16 fast p1 t65 | TN k2*4128 ws cs+ fast p7"},
    {"bf16 bwd (328,100,256,256)", {32800,0,256,256,0,0,0,0,0,W,0,1}, 1,
     "256x256 bf16 fast p2 t129 | 256x256 bf16 fast p2 t129 | 256x256 bf16 fast p1 t129 | TN ping-pong k31*1088 ws cs+ fast p7"},
    {"bf16 bwd (82,100,64,192) ids drop", {8200,0,64,192,1,1,0,0,0,W,0,1}, 1,
     "64x320 fast p4 t129 | 64x320 fast p4 t129 | 64x320 fast p1 t129 | TN k2*4128 ws cs+ fast p7"},
    {"bf16 bwd (90,100,48,160) compact", {8668,0,48,160,1,0,0,0,0,W,0,1}, 1,
     "64x320 fast p2 t136 | 64x320 fast p2 t136 | 64x320 fast p1 t136 | TN k2*4352 ws cs+ fast p7"},
  };
  for (const CellWant& w : wants) {
    const std::string got = w.bwd ? cell_bwd_lines(w.c, w.bwd == 1) : cell_fwd_lines(w.c);
    if (print) printf("CELL %-44s %s\n", w.name, got.c_str());
    ++g_named;
    if (got != w.want) { ++g_bad; printf("NAMED CELL PLAN %s:\n   got      %s\n   expected %s\n", w.name, got.c_str(), w.want); }
  }
}

int main(int argc, char** argv) {
  sweep_tn();
  sweep_nt();
  named_plans();
  named_cell_plans(argc > 1);
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
