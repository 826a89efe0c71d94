// What the GEMM engine offers the layers built on it (cell_ops.hip, dense_ops.hip): a layer fills in Problems, hands them to a
// Batch and reads the Batch's outcome.  The only GEMM header a layer file includes, and it brings in no kernel: Batch's methods
// live in gemm_batch.hip (host code: the plans of gemm_plan.h), the three launchers below in gemm_ops.hip next to their kernels.
// workspace_for() and gemm_mode() are in common.h.
#pragma once
#include "common.h"
#include "gemm_types.h"    // Problem, Launch, EPI_*, make_problem / make_seg_*

namespace gh {

// Call sites of the activation-sized NT launches, passed as Batch's `site`.  The values are bit positions (site - 1) of
// NARROW_DEFAULT, which is measured: they do not change.
enum BatchSite : int {
  SITE_NONE = 0,            // never narrow (e.g. the attention's t product with its head scores: keeps the 64 x 320 tile)
  SITE_CELL_ZR = 1,         // cell forward: z / r gate pair
  SITE_CELL_H = 2,          // cell forward: h gate
  SITE_CELL_BWD_H = 3,      // cell backward: da / d(r xp) pair
  SITE_CELL_BWD_ZR = 4,     // cell backward: da / dxp accumulation pair
  SITE_CELL_BWD_DX = 5,     // cell backward: dx (single problem, K = 300)
  SITE_ATT_BWD_DRIGHT = 6,  // attention backward: dright into the producing cell's gate head (single problem, K = 300)
  SITE_CELL_PROJ = 7,       // cell forward: the projection xp (single problem, K = 300)
};
constexpr int NARROW_DEFAULT = 14;     // call-site mask of the 64 x 160 tile (see Batch::narrow): cell forward h gate (2), cell backward da / d(r xp) pair (3) and da / dxp accumulation pair (4).  A/B on the bench step: 153.3 K -> 155.2 K pairs/s; the single-problem K = 300 sites (5, 6, 7) and the z / r pair (1) measured -0.1 .. +0.1 %

// launches that took the generic kernel since the last reset (gh_gemm_path_counters' second counter): a layer that prepared its
// operands for the fast kernels only compares the count before and after its launches
long long generic_launches();

// Collects problems that share their row space, splits wide outputs into column blocks the tile
// can hold, and launches them GH_MAX_PROBLEMS at a time.
struct Batch {
  // wide_bf16: every problem of this batch is a bf16-storage NT problem whose widths are multiples of 256 (h = 768)
  // site: SITE_NONE = never narrow; else narrow when the site's bit is set in NARROW_DEFAULT
  // n_hint: output width of the site's problems -- widths that 160-column blocks cover with less padding than 320-column
  // blocks (h = 768: 800 against 960 computed columns) take the narrow tile at every site (configs[4] in fp32: 26.1 -> 28.4 K pairs/s)
  Batch(bool tn, int rows_hint, hipStream_t s, bool wide_bf16 = false, int site = SITE_NONE, int n_hint = 0);
  void add(const Problem& p);
  void flush();
  // TN: bias gradients fused into the weight-gradient launch (Problem::colsum): for the problem added last, up to two outputs that
  // receive (+=) the column sums of the A operand.  colsum_fused tells the caller whether that happened.
  void want_colsum(float* o, float* o2) { if (L.nprob > 0) { cs_out[L.nprob - 1] = o; cs_out2[L.nprob - 1] = o2; } }

  int bm, bn;                   // rows / columns of the tile the constructor chose (bn: the column block wide outputs are split into)
  hipError_t err = hipSuccess;
  bool colsum_fused = false;
  bool colsum_missed = false;   // a requested column sum could be produced neither by the launch nor by the fallback kernel (bf16 operands without workspace)
  bool split_done = false;      // the last flush took the few-row split-K plan (its finish kernel applied the problems' row epilogues)
  float* g_ws = nullptr;        // the stream's split-K scratch (workspace_for), NULL = none registered
  size_t g_ws_bytes = 0;
  // 64 x 160 fp32 tile (CFG_64x160): half the accumulators -> <= 128 VGPRs -> FOUR workgroups per CU instead of three,
  // two column blocks per 300-wide problem.  More resident workgroups run more of the neighbours' epilogue streams underneath
  // the K loops: launches with stream-heavy epilogues gain, plain-store launches lose (prototype, tools/glds_proto.hip NHALF:
  // h-gate-like epilogue K = 300: 62.6 -> 68.2 TF, K = 600: 87.7 -> 90.5; plain store: 92.4 -> 88.7).  Chosen per call site.
  bool narrow = false;
  // EPI_ATT on rows wider than one column block (h = 768): every block applies tanh(. + u) to its columns and reduces ITS share
  // of the head scores W2 . t into a partial buffer of its own, e + block * e_block_stride (plain stores: the consumer,
  // att_softmax_fwd, adds the partials in block order -- deterministic).  0 = whole rows only.
  long long e_block_stride = 0;

 private:      // the engine's own state (gemm_batch.hip; the plans themselves: gemm_plan.h)
  Launch L;
  bool tn, big;
  hipStream_t s;
  int k_total = 0;
  float* cs_out[GH_MAX_PROBLEMS] = {nullptr};
  float* cs_out2[GH_MAX_PROBLEMS] = {nullptr};
  bool wide = false;      // 128 x 256 bf16 tile (CFG_128x256)
  bool wide256 = false;   // 256 x 256 x 64 bf16 tile, 8 waves, ping-pong K loop (CFG_256x256)
  // weight gradients of the bf16 storage pipeline on the 256 x 256 x 64 ping-pong tile (gemm_tn_pp.hip.h): the batch's problems stay
  // WHOLE outputs (no 320-column blocks), the kernel walks their 256 x 256 tiles.  Decided by the first problem of a launch.
  bool tn_pp = false;
  void reset();
  hipError_t launch_any();
  bool nt_split();
};

// EPI_ATT as a pass of its own over a stored product t [M][ha] (in place): t = tanh(t + u[urow ? urow[m] : m / l]), e = W2 t.
// The wide-hidden fallback of the concat attention; one wave per row (nt_finish_kernel).
int launch_att_finish(float* t, const float* u, const float* w2, float* e, const int32_t* urow, int M, int ha, int l, int heads, hipStream_t s);
// out [I][J] += the sum of n_parts partials [I][J] stored I * J floats apart (J % 4 == 0): few outputs, many partials -- one wave
// per float4 (reduce_partials_wave_kernel)
int launch_reduce_wave(const float* parts, int n_parts, float* out, int I, int J, hipStream_t s);
// Weight-sized NN products, all row-major: C [I][J] += sum over the item's terms of A_t [I][K_t] . B_t [K_t][J].  The cell
// backward's fix-up of its re-associated weight gradients (cell_ops.hip): ten 300^3 products in one launch, every output tile
// owned by one workgroup that adds its K chunks in a fixed order -- no atomics (nn_accumulate_kernel).
constexpr int NN_MAX_TERMS = 5, NN_MAX_ITEMS = 6;
struct NnTerm { const float* A; const float* B; int lda, ldb, K, vec; };      // vec: filled in by the launcher (16-byte loads of A)
struct NnItem { float* C; int I, J, ldc, nterm, tile0; NnTerm t[NN_MAX_TERMS]; };      // tile0: filled in by the launcher
struct NnArgs { NnItem it[NN_MAX_ITEMS]; int n; };
inline void nn_add_term(NnItem& it, const float* A, int lda, const float* B, int ldb, int K) {
  it.t[it.nterm++] = NnTerm{A, B, lda, ldb, K, 0};
}
int launch_nn_accumulate(NnArgs& R, hipStream_t s);      // (items with the most terms first: their tiles run longest)

inline Problem gemm_problem(int M, int N, int epi, float* C, int ldc, const float* A, int lda, const float* B, int ldb,
                            int K, const int32_t* gatherA = nullptr, int elt = 0) {
  Problem p = make_problem(M, N, epi, C, ldc);
  p.elt = elt;
  p.seg[0] = make_seg_nt(A, lda, B, ldb, K, gatherA, elt);
  return p;
}
inline void add_seg(Problem& p, const float* A, int lda, const float* B, int ldb, int K) {
  p.seg[p.nseg++] = make_seg_nt(A, lda, B, ldb, K, nullptr, p.elt);
}
inline void set_dropout(Problem& p, int mode, int ld, float drop_p, unsigned seed) {
  if (drop_p <= 0.f) return;
  p.drop_mode = mode; p.drop_ld = ld; p.drop_col0 = 0; p.drop_seed = seed;
  const double t = (double)drop_p * 4294967296.0;
  p.drop_thresh = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
  p.drop_scale = 1.0f / (1.0f - drop_p);
}
inline Problem tn_problem(int I, int J, float* C, int ldc, const float* A, int lda, const float* B, int ldb, int K,
                          const int32_t* gatherB = nullptr, int elt = 0) {
  Problem p = make_problem(I, J, EPI_ATOMIC, C, ldc);
  p.seg[0] = make_seg_tn(A, lda, I, B, ldb, J, K, nullptr, gatherB);
  p.elt = elt;
  if (elt) {
    p.seg[0].vecA = ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && lda % 8 == 0 && I % 8 == 0;
    p.seg[0].vecB = ((reinterpret_cast<uintptr_t>(B) & 15) == 0) && ldb % 8 == 0 && J % 8 == 0;
  }
  return p;
}

}  // namespace gh
