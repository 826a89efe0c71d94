// The arithmetic of the GEMM engine without its launches: which tile a Batch takes, whether a launch may run on the fast kernels,
// how a weight gradient (TN) or a few-row product (NT) is split over K, where its partial tiles lie in the workspace, which kernel
// configuration a launch runs on and with what grid.  Plain host C++ with no HIP call, no HIP include and no global state; it reads
// sizes, flags and the alignment of pointer values, never what a pointer points to.  The GEMM mode (gh_set_gemm_mode), the workspace
// size and the hints come in as arguments.  gemm_batch.hip is its only user in the library -- an edit here does not rebuild the kernels
// -- and tools/gemm_plan_sweep.cpp walks it on the CPU.  Every tuning constant sits here next to the measurement that justifies it.
#pragma once
#include "gemm_types.h"
#include <stddef.h>

namespace gh {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the tile of a Batch (its constructor) ---------------------------------------------------------------------------------
struct TilePlan {
  bool big;         // 64x320 tile (2x2 waves) for the activation-sized GEMMs, 32x320 (1x4) for few-row ones
  bool wide;        // 128 x 256 bf16 tile
  bool wide256;     // 256 x 256 x 64 bf16 tile, 8 waves, ping-pong K loop
  bool narrow;      // 64 x 160 fp32 tile
  int bm, bn;
};
// narrow_mask: the call sites (bit site - 1) that take the narrow tile by measurement (gemm_batch.h NARROW_DEFAULT)
inline TilePlan tile_plan(bool tn_, int rows_hint, bool wide_bf16, int site, int n_hint, int mode, int narrow_mask) {
  TilePlan t = {};
  t.big = tn_ || rows_hint >= 8192;      // 64x320 tile (2x2 waves) for the activation-sized GEMMs, 32x320 (1x4) for few-row ones
  t.bm = t.big ? 64 : 32;
  t.bn = 320;
  if (wide_bf16 && t.big && !tn_) { t.wide = true; t.bm = 128; t.bn = 256; }
  // 256 x 256 x 64 / 8 waves, one workgroup per CU, ping-pong K loop + software-pipelined epilogue (gemm_nt_pp.hip.h, round 6):
  // the default for activation-sized launches of the bf16 storage pipeline -- configs[4], B = 32: gemm_big 4.25 -> 3.09 ms per
  // step, 128.1 -> 148.6 K pairs/s.  (Round 3's 256 x 256 tile -- the 128 x 256 tile's K loop on 8 waves, 32-deep stages --
  // measured 0.200 against 0.207: not the tile size but the loop structure is the lever.)  Launches below 32 768 rows (fewer
  // than 1.5 workgroups per CU) keep the 128 x 256 tile.
  constexpr int tile256_rows = 32768;
  if (t.wide && rows_hint >= tile256_rows) { t.wide256 = true; t.bm = 256; }
  const bool less_pad = n_hint > 0 && (n_hint + 159) / 160 * 160 < (n_hint + 319) / 320 * 320;
  // launches whose 64 x 320 grid would not fill one round of 768 workgroup slots (realistic evidence counts: 14 208 rows = 222
  // row tiles) get twice the workgroups on 1024 slots: 99.0 -> 102.0 K pairs/s on the Snopes-histogram step at B = 32
  const bool thin = rows_hint <= 24576;
  if (site > 0 && t.big && !tn_ && !t.wide && mode == 0 && (((narrow_mask >> (site - 1)) & 1) || less_pad || thin)) { t.narrow = true; t.bn = 160; }
  // (launches without a call-site id, e.g. the attention's t product with its head scores, keep the 64 x 320 tile)
  return t;
}

// ---- fast-path preconditions -----------------------------------------------------------------------------------------------
// of gemm_nt.hip.h (NT: both operands contraction-contiguous) and gemm_tn.hip.h (TN); both LDS-DMA
// rule 0: the launch may run on the fast kernels; else the rule that sends it to the generic kernel, the problem it failed on and,
// seg >= 0, the segment (gemm_batch.hip's tool build prints them)
struct FastRule { int rule, prob, seg; };
inline bool s_lds_bad(const Problem& p) { return p.seg[0].lda % 8 || p.seg[0].ldb % 8; }
inline FastRule fast_rule(const Launch& L, bool tn) {
  for (int i = 0; i < L.nprob; ++i) {
    const Problem& p = L.p[i];
    const int ns = tn ? 1 : p.nseg;
    for (int j = 0; j < ns; ++j) {
      const Seg& s = p.seg[j];
      if (!s.vecA || !s.vecB || s.gatherB || s.K < 4) return {1, i, -1};
      if (tn && s.gatherA) return {2, i, -1};
    }
    if (p.elt && tn && (p.M % 8 || p.N % 8 || s_lds_bad(p))) return {3, i, -1};
    if (!tn) {  // operands are addressed through buffer descriptors: 31-bit byte offsets
      for (int j = 0; j < p.nseg; ++j) {
        if (4.0 * (double)p.seg[j].ldb * (double)p.N >= 2147483648.0) return {4, i, -1};
        if (!p.seg[j].gatherA && 4.0 * (double)p.seg[j].lda * (double)p.M >= 2147483648.0) return {5, i, j};   // (gathered tables: < 2 GB by contract)
      }
    }
    if (tn) {
      const Seg& s = p.seg[0];
      if (4.0 * (double)s.lda * (double)s.K >= 2147483648.0 || 4.0 * (double)s.ldb * (double)s.K >= 2147483648.0) return {6, i, -1};
    }
    if (p.N % 4 || p.N < 4 || p.ldc % 4 || !al16(p.C)) return {7, i, -1};
    if (tn && (p.M % 4 || p.M < 4)) return {8, i, -1};
    if ((p.bias && !al16(p.bias)) || (p.bias2 && !al16(p.bias2)) || (p.out1 && !al16(p.out1)) || (p.in0 && !al16(p.in0)) || (p.in1 && !al16(p.in1)))
      return {9, i, -1};
    if (p.epi == EPI_ATT && (!al16(p.u) || p.ldu % 4 || !al16(p.w2))) return {10, i, -1};
    if (p.epi == EPI_TANH_H && p.w2 && !al16(p.w2)) return {11, i, -1};
    if (p.epi == EPI_GATE_PRE && (tn || !p.in0 || !p.in1 || !p.in2 || !p.out1 || !p.out2 || !al16(p.in2) || !al16(p.out2) ||
                                  (p.gin && !al16(p.gin)))) return {12, i, -1};
  }
  return {0, -1, -1};
}
inline bool fast_ok(const Launch& L, bool tn) { return fast_rule(L, tn).rule == 0; }

// bf16 weight-gradient GEMM on the 256 x 256 x 64 ping-pong tile (gemm_tn_pp.hip.h): K-chunk rows from which a batch of whole-output
// problems takes it (below: the 128 x 320 tile, gemm_tn_bf16_kernel<2, 2, 10, 4>)
constexpr int TN_PP_ROWS = 16384;
inline bool tn_pp_ok(const Problem& p, bool tn, bool have_ws) {
  if (!tn || !p.elt || p.nseg != 1 || !have_ws || p.epi != EPI_ATOMIC) return false;
  const Seg& sg = p.seg[0];
  if (sg.gatherA || sg.gatherB || !sg.vecA || !sg.vecB || sg.K < TN_PP_ROWS) return false;
  if (p.M % 256 || p.N % 256 || p.ldc % 4 || (reinterpret_cast<uintptr_t>(p.C) & 15)) return false;
  return (size_t)sg.K * (size_t)sg.lda * 2 < ((size_t)1 << 31) && (size_t)sg.K * (size_t)sg.ldb * 2 < ((size_t)1 << 31);
}
// rows of the tile that Batch::add counts a problem's row tiles in (Launch::m_tiles)
inline int row_tile(bool tn, bool tn_pp, int elt, int bm) {
  return tn_pp ? 256 : (tn && elt) ? 128 : bm;      // (bf16 TN: the 128 x 320 tile; all problems of a TN launch share the storage mode)
}

// ---- weight gradients (TN): the split over K and the workspace -------------------------------------------------------------
struct TnPlan {
  int ksplit, kchunk, per;      // Launch::ksplit / kchunk / per
  bool want_cs;                 // some problem asked for its column sums (Batch::want_colsum)
  bool cs_in_launch;            // ... and the launch carries them: partials behind the tiles in the workspace
  bool use_ws;                  // partial tiles go to the workspace (else: atomics into C)
  size_t need;                  // bytes the plan asked of the workspace (column-sum partials counted whether carried or not)
  size_t tile_off[GH_MAX_PROBLEMS];      // use_ws: where problem i's ksplit partial tiles [M][N] start, in floats
  size_t cs_off[GH_MAX_PROBLEMS];        // cs_in_launch and has_cs[i]: where its ksplit column-sum partials [M] start
  size_t used;                  // floats of the workspace the regions take: they are consecutive from 0
  int reduce_elems;             // float4 elements of the largest reduce item (reduce_partials_kernel's grid)
};
// L: the launch as Batch::add left it (problems, m_tiles, n_tiles); k_total: the longest contraction; has_cs[i]: problem i wants
// its column sums; ws_bytes: the split-K part of the stream's workspace (have_ws = 0: none registered)
inline TnPlan tn_split_plan(const Launch& L, bool tn_pp, int k_total, const bool* has_cs, bool have_ws, size_t ws_bytes, int mode) {
  TnPlan P = {};
  const int n_inner = L.m_tiles * L.nprob;
  constexpr int target = 2304;
  int ks = (target + n_inner - 1) / n_inner;   // three resident rounds of 256 CUs x 3 workgroups (measured on the bench step: 1152 -> 2.06 ms,
                                               // 1536 -> 1.95, 2304 -> 1.86, 3072 -> 1.84 but more partials to reduce; one round 20 % slower)
  // shortest K chunk: 256 rows (fp32).  bf16 storage, wide outputs (h = 768: 64 x 320 partial tiles of 80 KB each): a single
  // 768 x 768 product split into 64 chunks writes and re-reads more partial-tile bytes than it streams operands
  constexpr int min_rows16 = 4096;      // (A/B on configs[4]: 256 / 1024 / 2048 / 4096 rows = 106.76 / 106.72 / 106.81 / 107.17 K pairs/s)
  const int min_rows = L.p[0].elt ? min_rows16 : 256;
  const int ks_max = (k_total / min_rows > 1) ? k_total / min_rows : 1;
  if (ks > ks_max) ks = ks_max;
  if (ks < 1) ks = 1;
  // The K chunks are dealt round-robin to the 8 XCDs (chunk c runs on XCD c % 8, gemm_tn.hip.h): a chunk count that is
  // not a multiple of 8 leaves some XCDs one chunk (1 / 8 of their work at 65 chunks) more than the others.  Measured on
  // the bench step (A/B, one box): 65 chunks 158.6 K pairs/s, 72 chunks 159.9 K, 85 chunks 156.4 K.
  const int align = tn_pp ? 64 : L.p[0].elt ? 32 : 16;      // K tile of the kernel (bf16 storage: 32 rows, ping-pong tile: 64)
  if (tn_pp) {
    // one workgroup per CU: as many K chunks as fill ONE round of 256 workgroups when that occupies >= 85 % of them (h = 768: a
    // cell's 7 outputs = 63 tiles x 4 chunks = 252), else two rounds; chunks of at least 1024 rows.  The XCD rule does not apply:
    // the kernel deals its items to the XCDs in runs.
    const int tiles = L.nprob * L.m_tiles * L.n_tiles;
    const int ks1 = 256 / tiles > 0 ? 256 / tiles : 1, ks2 = 512 / tiles > 0 ? 512 / tiles : 1;
    const double e1 = tiles * ks1 / 256.0, e2 = tiles * ks2 / 512.0;
    ks = (e1 >= 0.85 || e1 >= e2) ? ks1 : ks2;
    const int kmax = k_total / 1024 > 1 ? k_total / 1024 : 1;
    if (ks > kmax) ks = kmax;
    // (the partial tiles must fit the workspace: fewer chunks otherwise)
    size_t out_bytes = 0;
    for (int i = 0; i < L.nprob; ++i) out_bytes += ((size_t)L.p[i].M * L.p[i].N + (has_cs[i] ? (size_t)L.p[i].M : 0)) * sizeof(float);
    while (ks > 1 && (size_t)ks * out_bytes > ws_bytes) --ks;
  } else
  if (ks >= 12) ks = ((ks + 4) / 8) * 8;
  int chunk = (k_total + ks - 1) / ks;
  chunk = ((chunk + align - 1) / align) * align;
  P.kchunk = chunk;
  P.ksplit = (k_total + chunk - 1) / chunk;
  if (tn_pp) P.per = (L.nprob * L.m_tiles * L.n_tiles * P.ksplit + 7) / 8;
  if (!tn_pp && P.ksplit >= 12 && P.ksplit % 8 != 0) {      // rounding the chunk up dropped a chunk or two: stretch the chunks to the multiple of 8 below
    const int k8 = (P.ksplit / 8) * 8;
    chunk = (((k_total + k8 - 1) / k8 + align - 1) / align) * align;
    if ((k_total + chunk - 1) / chunk % 8 == 0) { P.kchunk = chunk; P.ksplit = (k_total + chunk - 1) / chunk; }
  }
  // partial tiles -> workspace when it is big enough and every output is float4-shaped
  size_t need = 0;
  bool want_cs0 = false;
  for (int i = 0; i < L.nprob; ++i) want_cs0 = want_cs0 || has_cs[i];
  // (a single chunk also goes through the workspace when the ping-pong kernel runs it -- it only writes partial tiles -- or when
  //  bf16 operands want their bias gradient: that rides in the fused kernels' workspace path only)
  bool ws_ok = have_ws && (P.ksplit > 1 || tn_pp || (want_cs0 && L.p[0].elt));
  bool any_cs = false;
  for (int i = 0; i < L.nprob && ws_ok; ++i) {
    if (L.p[i].N % 4) ws_ok = false;
    need += (size_t)P.ksplit * L.p[i].M * L.p[i].N * sizeof(float);
    if (has_cs[i]) { need += (size_t)P.ksplit * L.p[i].M * sizeof(float); any_cs = true; }
  }
  if (any_cs && !(ws_ok && need <= ws_bytes && fast_ok(L, true) && (mode != 1 || L.p[0].elt))) any_cs = false;
  P.want_cs = want_cs0;
  P.cs_in_launch = any_cs;
  P.need = need;
  P.use_ws = ws_ok && need <= ws_bytes;
  if (!P.use_ws) return P;
  size_t w = 0;
  int max_elems = 0;
  for (int i = 0; i < L.nprob; ++i) {
    const Problem& q = L.p[i];
    P.tile_off[i] = w;
    w += (size_t)P.ksplit * q.M * q.N;
    if (q.M * (q.N / 4) > max_elems) max_elems = q.M * (q.N / 4);
  }
  int max_cs = 0;          // bias-gradient partials [ksplit][M] behind the tiles
  for (int i = 0; i < L.nprob && any_cs; ++i) {
    const Problem& q = L.p[i];
    if (!has_cs[i]) continue;
    P.cs_off[i] = w;
    w += (size_t)P.ksplit * q.M;
    if (q.M / 4 > max_cs) max_cs = q.M / 4;
  }
  if (max_cs > max_elems) max_elems = max_cs;
  P.used = w;
  P.reduce_elems = max_elems;
  return P;
}

// ---- few-row NT products: the split over K ---------------------------------------------------------------------------------
// (evidence level, head): too few row tiles to fill 256 CUs, so split K across workgroups, keep the partial tiles in the workspace
// and finish with nt_finish_kernel
struct NtSplitPlan {
  bool ok;                 // false: the launch runs unsplit
  int ks, ct;              // chunks (Launch::ksplit) and K tiles of 16 per chunk (Launch::kchunk = 16 ct)
  int tmax;                // K tiles of 16 over a problem's concatenated segments
  size_t need;             // bytes of workspace
  size_t off[GH_MAX_PROBLEMS];      // where problem i's ks partial tiles [M][N] start, in floats
  int finish_split;        // nt_finish_kernel: 1 = a workgroup per row, 0 = a wave per row
  int finish_grid;         // ... and its grid's x (y = the problems)
};
inline NtSplitPlan nt_split_plan(const Launch& L, bool have_ws, size_t ws_bytes) {
  NtSplitPlan P = {};
  const int blocks = L.m_tiles * L.nprob;
  constexpr int max_blocks = 96;
  if (!have_ws || blocks >= max_blocks || !fast_ok(L, false)) return P;
  int tmax = 0;          // K tiles over the concatenated segments (every problem of a launch is split alike)
  for (int i = 0; i < L.nprob; ++i) {
    const Problem& q = L.p[i];
    if (q.epi == EPI_ATOMIC || q.epi == EPI_GATE_PRE || q.drop_mode != 0 || (q.epi == EPI_TANH_H && q.w2) || q.seg0_rows > 0 || q.elt) return P;   // (fp32 problems only)
    int t = 0;
    for (int j = 0; j < q.nseg; ++j) t += (q.seg[j].K + 15) / 16;
    if (i > 0 && t != tmax) return P;
    tmax = t;
  }
  int ks = tmax / 4;
  // workgroups wanted: one per CU -- two for long contractions (>= 128 K tiles, e.g. the evidence-level attention at h = 768:
  // K = 6272), where a split-K workgroup is MFMA-bound rather than latency-bound (A/B configs[4] bf16: 256 / 512 / 768 =
  // 107.7 / 108.7 / 108.1 K pairs/s; headline and Snopes-count steps unchanged at any of them)
  const int tgt = tmax >= 128 ? 512 : 256;
  const int want = (tgt + blocks - 1) / blocks;
  if (ks > want) ks = want;
  if (ks < 2) return P;
  const int ct = (tmax + ks - 1) / ks;     // tiles per chunk
  ks = (tmax + ct - 1) / ct;
  if (ks < 2) return P;
  size_t need = 0;
  for (int i = 0; i < L.nprob; ++i) need += (size_t)ks * L.p[i].M * L.p[i].N * sizeof(float);
  if (need > ws_bytes) return P;
  size_t w = 0;
  int max_m = 0;
  for (int i = 0; i < L.nprob; ++i) {
    P.off[i] = w;
    w += (size_t)ks * L.p[i].M * L.p[i].N;
    if (L.p[i].M > max_m) max_m = L.p[i].M;
  }
  P.ok = true; P.ks = ks; P.ct = ct; P.tmax = tmax; P.need = need;
  // many partials over few rows: a workgroup per row (the four waves share the partials); otherwise a wave per row
  P.finish_split = (ks >= 16 && max_m <= 8192) ? 1 : 0;      // (ks = 9, M = 960 -- the claim cell, the evidence-level attention -- measured equal or slower split)
  P.finish_grid = P.finish_split ? max_m : (max_m + 3) / 4;
  return P;
}

// ---- the kernel configuration of a launch (Batch::launch_any) and its grid -------------------------------------------------
struct ConfigPlan { GemmConfig cfg; int m_tiles; };      // m_tiles: Launch::m_tiles, recounted where the rule changes the row tile
inline int recount_m_tiles(const Launch& L, int rows) {
  int mt = 0;
  for (int i = 0; i < L.nprob; ++i) { const int t = (L.p[i].M + rows - 1) / rows; if (t > mt) mt = t; }
  return mt;
}
// big / narrow / wide / wide256: the Batch's tile (tile_plan; a layer may have set `narrow` itself)
inline ConfigPlan gemm_config(const Launch& L, bool tn, bool tn_pp, bool big, bool narrow, bool wide, bool wide256, int mode) {
  if (tn && tn_pp) return {CFG_TN_PP, L.m_tiles};
  if (narrow && !tn && L.ksplit == 1 && !L.p[0].elt) return {CFG_64x160, L.m_tiles};
  if (big && !tn && L.ksplit == 1 && !L.p[0].elt) {
    // Occupancy-aware tile choice.  The chip holds 768 workgroups of either configuration (3 per CU); a grid of 64-row
    // tiles that ends in a thinly filled last round (e.g. 976 workgroups = 1.27 rounds, the node-compact single-problem
    // launches) runs faster on 32-row tiles (1937 workgroups = 2.52 rounds): measured 83 vs 78 TF at K = 300.
    const double r = (double)L.m_tiles * L.nprob / 768.0;
    const double frac = r - (double)(long long)r;
    if (mode != 1 && r < 3.0 && frac > 0.02 && frac < 0.45) return {CFG_32x320, recount_m_tiles(L, 32)};
  }
  if (wide256) {
    // the ping-pong loop's preconditions (gemm_nt_pp.hip.h): whole 64-deep K tiles, no K split, no dropout inside the K loop
    bool ok = L.ksplit == 1;
    for (int i = 0; i < L.nprob; ++i) {
      if (L.p[i].drop_mode == 1) ok = false;
      for (int j = 0; j < L.p[i].nseg; ++j) if (L.p[i].seg[j].K % 64) ok = false;
    }
    if (ok) return {CFG_256x256, L.m_tiles};
    return {CFG_128x256, recount_m_tiles(L, 128)};
  }
  if (wide) return {CFG_128x256, L.m_tiles};
  return {big ? CFG_64x320 : CFG_32x320, L.m_tiles};
}

// workgroups of a launch_cfg launch (every configuration but CFG_TN_PP, whose grid is 8 * Launch::per)
inline bool nt_few(const Launch& L, bool tn, bool fast) {
  return !tn && L.m_tiles < 8 && fast;      // gemm_nt.hip.h: linear work decode for launches of fewer than 8 row tiles
}
inline int gemm_grid(const Launch& L, bool tn, bool fast) {
  const int n_outer = tn ? L.ksplit : L.m_tiles;
  const int n_inner = tn ? L.m_tiles * L.nprob : L.nprob * L.ksplit;
  return nt_few(L, tn, fast) ? n_outer * n_inner : 8 * ((n_outer + 7) / 8) * n_inner;
}

}  // namespace gh
