// The launch descriptors of the GEMM engine and their inline host builders: what a layer fills in (gemm_batch.h), what the planner
// reads (gemm_plan.h) and what the kernels receive by value (gemm.hip.h).  Plain C++ with nothing from HIP, so that the planner and
// its sweep (tools/gemm_plan_sweep.cpp) compile without the kernels.
#pragma once
#include <stdint.h>
#include <string.h>

namespace gh {

enum EpiKind : int {
  EPI_STORE = 0,   // C = v (+bias[col]) (+C when accumulate)
  EPI_SIGMOID_Z,   // z = sigmoid(v+bias) -> C
  EPI_SIGMOID_R,   // r = sigmoid(v+bias) -> C ; out1 = r * in0            (in0 = xp)
  EPI_TANH_H,      // h = tanh(v+bias) -> C ; out1 = h*z + xp*(1-z)        (in0 = z, in1 = xp)
  EPI_ATT,         // t = tanh(v + u[rowg ? rowg[row] : row/R][col]) -> C ; e[row][c] = sum_col t*w2[c][col]
  EPI_BWD_DRX,     // v = d(r*xp): C(drp) = v*xp*r*(1-r) ; out1(dxp) += v*r  (in0 = xp, in1 = r)
  EPI_ATOMIC,      // atomicAdd(C, v)   (TN split-K)
  EPI_GATE_PRE,    // g = v (+ gin): the GGNN cell backward's elementwise head fused into the GEMM that PRODUCES g (fast NT
                   // kernel only): C(dhp) = g z (1-h^2) ; out1(dzp) = g (h-xp) z (1-z) ; out2(dxp) = g (1-z)
                   // (in0 = z, in1 = hh, in2 = xp of the cell that consumes g; g itself is never stored)
};

struct Seg {
  const float* A; const int32_t* gatherA; int lda; int vecA;
  const float* B; const int32_t* gatherB; int ldb; int vecB;
  int K;
};

struct Problem {
  Seg seg[2];
  int nseg;
  int M, N;
  int epi;
  int accumulate;
  float* C; int ldc;
  const float* bias;
  const float* bias2;       // optional second bias added to `bias` (b?0 + b?1 of a gate; NT fast kernel and the generic kernel)
  float* out1;
  const float* in0; const float* in1;   // same leading dimension as C
  const float* u; const float* w2; float* e; int ldu; int R; int heads;
  int seg0_rows;            // > 0: segment 0's A operand is all zero for rows >= seg0_rows (fast kernel skips it per tile)
  const int32_t* rowg;      // EPI_ATT: u row of output row m is rowg[m] when non-null (node-compact layout), else m / R
  long long split_stride;   // TN: element offset of K-chunk `ks`'s partial tile (0 = all chunks hit C, atomically)
  // TN: when non-null, the column sums of the A operand over this workgroup's K chunk (= the bias gradient that
  // belongs to this weight gradient) are written to colsum[ks * colsum_stride + column]; fast kernel only
  float* colsum; long long colsum_stride;
  // stateless input dropout (wrapper.py:189-190): element (row, col) of the dropped matrix [rows][drop_ld] is kept
  // iff hash(seed, row*drop_ld + col) >= drop_thresh and then scaled by drop_scale = 1/(1-p).
  // drop_mode: 0 off, 1 = A of segment 0 (NT), 3 = C in the EPI_STORE epilogue (gradient w.r.t. the dropped
  //            input).  Fast kernel only.  (The weight-gradient GEMM gets its masked operand from gather_rows:
  //            hashing in the TN loader pushed that kernel over 168 VGPRs, i.e. from 3 to 2 waves per SIMD.)
  int drop_mode; int drop_ld; int drop_col0; unsigned drop_seed; unsigned drop_thresh; float drop_scale;
  // bf16 storage pipeline (gemm_nt.hip.h MODE 2 / gemm_tn.hip.h bf16): elt = 1 -> A and B hold bf16 (lda/ldb/K in
  // elements); io bits say which epilogue streams are bf16: 1 = C, 2 = out1, 4 = in0, 8 = in1, 16 = in2, 32 = out2 (the last
  // two: EPI_GATE_PRE); c32 (EPI_TANH_H): also
  // write the fp32 value of out1 there (the cell output the fp32 consumers read)
  int elt; int io; float* c32;
  // EPI_TANH_H with the fused scorer projection on a COLUMN BLOCK of the row (narrow tile): this block's partial dot product is
  // ADDED to e[row] (zeroed by the caller; two blocks -> two addends -> the sum does not depend on their order)
  int e_atomic;
  // EPI_GATE_PRE: optional addend of g (same shape as C), third input stream, third output stream
  const float* gin; const float* in2; float* out2;
};

#define GH_MAX_PROBLEMS 12     // (sizeof(Launch) = 12 x 336 + 32 = 4064 of the 4096 kernarg bytes: the head's 3556-wide products are 12 column blocks)
struct Launch {
  Problem p[GH_MAX_PROBLEMS];
  int nprob;
  int m_tiles;   // max over problems of ceil(M / BM)
  int ksplit;    // TN: number of K chunks (1 otherwise)
  int kchunk;    // TN: rows per chunk, multiple of 16
  int dbg;       // measurement only (tool build, GH_DBG; 0 in the product): DBG_* bits below
  int n_tiles;   // gemm_tn_pp_kernel: max over problems of ceil(N / 256) (its problems are whole outputs, not column blocks)
  int per;       // gemm_tn_pp_kernel: work items per XCD (XCD x runs items [x per, (x + 1) per) of the chunk-major list)
};
static_assert(sizeof(Launch) <= 4096, "Launch travels by value in the kernarg segment (4 KB)");
// Launch::dbg bits: timing instruments of the tool build (common.h GH_DBG_BITS).  They skip or time parts of the same kernels.
constexpr int DBG_NO_EPILOGUE = 1;      // K loop only
constexpr int DBG_NO_KLOOP = 2;         // epilogue only (one K tile)
constexpr int DBG_EPI_TICKS = 1024;     // 256-tile epilogue: per-kind tick sums into g_nt_phase (gh_debug_nt_phases)

// The kernel configurations a launch can run on: what the planner chooses (gemm_plan.h gemm_config) and the engine's launch_gemm
// turns into launch_cfg<WM, WN, NI, MI> (workgroup = WM x WN waves, wave tile = 16 MI x 16 NI) or launch_tn_pp.
enum GemmConfig : int {
  CFG_32x320,      // <1, 4, 5>: few-row launches, and the occupancy rule's 32-row tiles
  CFG_64x320,      // <2, 2, 10>: activation-sized launches; every weight gradient but the ping-pong ones; bf16 storage too
  CFG_64x160,      // <2, 2, 5>: the narrow tile (Batch::narrow), fp32 NT only
  CFG_128x256,     // <2, 2, 8, 4>: bf16 storage, NT only
  CFG_256x256,     // <2, 4, 4, 8>: bf16 storage, NT only, 8 waves, ping-pong K loop
  CFG_TN_PP,       // gemm_tn_pp_kernel: bf16 weight gradients on the 256 x 256 x 64 ping-pong tile
  CFG_NCONFIGS
};

// ---------------------------------------------------------------------------------- host side
inline int vec_ok(const void* p, int ld, int inner) {
  return ((reinterpret_cast<uintptr_t>(p) & 15) == 0) && (ld % 4 == 0) && (inner % 4 == 0);
}

inline Seg make_seg(const float* A, int lda, const float* B, int ldb, int K, int n_inner,
                    const int32_t* gatherA = nullptr, const int32_t* gatherB = nullptr) {
  Seg s;
  s.A = A; s.lda = lda; s.gatherA = gatherA; s.vecA = vec_ok(A, lda, K);
  s.B = B; s.ldb = ldb; s.gatherB = gatherB; s.vecB = vec_ok(B, ldb, n_inner);
  s.K = K;
  return s;
}
// NT: A [M][lda] (rows optionally gathered), B [N][ldb]; both rows hold the K contraction values contiguously
inline Seg make_seg_nt(const float* A, int lda, const float* B, int ldb, int K, const int32_t* gatherA = nullptr, int elt = 0) {
  Seg s;
  const int q = elt ? 8 : 4;          // elements per 16 bytes
  s.A = A; s.lda = lda; s.gatherA = gatherA; s.vecA = ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && lda % q == 0 && K % q == 0;
  s.B = B; s.ldb = ldb; s.gatherB = nullptr; s.vecB = ((reinterpret_cast<uintptr_t>(B) & 15) == 0) && ldb % q == 0 && K % q == 0;
  s.K = K;
  return s;
}
inline Seg make_seg_tn(const float* A, int lda, int I, const float* B, int ldb, int J, int K,
                       const int32_t* gatherA = nullptr, const int32_t* gatherB = nullptr) {
  Seg s;
  s.A = A; s.lda = lda; s.gatherA = gatherA; s.vecA = vec_ok(A, lda, I);
  s.B = B; s.ldb = ldb; s.gatherB = gatherB; s.vecB = vec_ok(B, ldb, J);
  s.K = K;
  return s;
}

inline Problem make_problem(int M, int N, int epi, float* C, int ldc) {
  Problem p;
  memset(&p, 0, sizeof(p));
  p.M = M; p.N = N; p.epi = epi; p.C = C; p.ldc = ldc; p.nseg = 1;
  return p;
}

}  // namespace gh
