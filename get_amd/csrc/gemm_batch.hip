// Batch's methods (declared in gemm_batch.h, with the comments on its knobs): column blocks, and the plans of gemm_plan.h turned
// into launches of the engine (gemm_engine.h).  Host code only -- no kernel, no kernel launch, none of the kernel headers -- so
// an edit of a tile rule or a split-K plan compiles in seconds.
#include "gemm_batch.h"
#include "gemm_engine.h"
#include "gemm_plan.h"

namespace gh {

// tool build: GH_FASTOK_DEBUG=1 names the rule that sent a launch to the generic kernel (seg >= 0: and that segment's sizes)
static bool fast_checked(const Launch& L, bool tn) {
  const FastRule r = fast_rule(L, tn);
  static const bool dbg = measure_env("GH_FASTOK_DEBUG", 0) != 0;
  if (dbg && r.rule) {
    fprintf(stderr, "gemm: generic kernel (fast_ok rule %d, problem %d)\n", r.rule, r.prob);
    const Problem& p = L.p[r.prob];
    if (r.seg >= 0) fprintf(stderr, "   seg %d lda %d M %d N %d K %d\n", r.seg, p.seg[r.seg].lda, p.M, p.N, p.seg[r.seg].K);
  }
  return r.rule == 0;
}

Batch::Batch(bool tn_, int rows_hint, hipStream_t s_, bool wide_bf16, int site, int n_hint) : tn(tn_), s(s_) {
  const Workspace w = workspace_for(s_);
  g_ws = w.p; g_ws_bytes = w.bytes;
  const TilePlan t = tile_plan(tn_, rows_hint, wide_bf16, site, n_hint, gemm_mode(), NARROW_DEFAULT);
  big = t.big; bm = t.bm; bn = t.bn; wide = t.wide; wide256 = t.wide256; narrow = t.narrow;
  reset();
}
void Batch::reset() {
  L.nprob = 0; L.m_tiles = 0; L.ksplit = 1; L.kchunk = 0; k_total = 0; L.n_tiles = 0; L.per = 0;
  static const int dbg = measure_env("GH_DBG", 0);      // (tool build: DBG_* bits, gemm_types.h)
  L.dbg = dbg;
  for (int i = 0; i < GH_MAX_PROBLEMS; ++i) cs_out[i] = cs_out2[i] = nullptr;
}

void Batch::add(const Problem& p) {
  // row reductions need whole rows -- except the scorer's single dot product, which two column blocks may add up (e_atomic)
  const bool scorer_blocks = p.epi == EPI_TANH_H && p.w2 && p.N > bn && narrow && p.N <= 2 * bn;
  const bool att_blocks = p.epi == EPI_ATT && p.N > bn && e_block_stride > 0;
  // ... or, with a partial buffer per block (e_block_stride), any number of them: the scorer kernel adds the partials in block order
  const bool scorer_parts = p.epi == EPI_TANH_H && p.w2 && p.N > bn && !scorer_blocks && e_block_stride > 0;
  if ((p.epi == EPI_ATT || (p.epi == EPI_TANH_H && p.w2)) && p.N > bn && !scorer_blocks && !att_blocks && !scorer_parts) { err = hipErrorInvalidValue; return; }
  if (tn) {
    const bool want = tn_pp_ok(p, tn, g_ws != nullptr);
    if (L.nprob > 0 && want != tn_pp) flush();      // (a launch is one kernel: problems of the other kind start the next one)
    if (L.nprob == 0) tn_pp = want;
  }
  const int bn = tn_pp ? (1 << 30) : this->bn;
  for (int n0 = 0; n0 < p.N; n0 += bn) {
    Problem q = p;
    q.N = (p.N - n0 < bn) ? p.N - n0 : bn;
    auto adv = [](const float* ptr, size_t elems, bool bf) { return (const float*)((const char*)ptr + elems * (bf ? 2 : 4)); };
    for (int i = 0; i < q.nseg; ++i) {
      if (tn) {
        q.seg[i].B = adv(q.seg[i].B, (size_t)n0, q.elt);
        q.seg[i].vecB = q.elt ? (((reinterpret_cast<uintptr_t>(q.seg[i].B) & 15) == 0) && q.seg[i].ldb % 8 == 0 && q.N % 8 == 0)
                              : vec_ok(q.seg[i].B, q.seg[i].ldb, q.N);
      } else {
        q.seg[i].B = adv(q.seg[i].B, (size_t)n0 * q.seg[i].ldb, q.elt);       // B is [N][ldb]: a column block of C is a row block of B
      }
    }
    q.C = (float*)adv(q.C, (size_t)n0, q.io & 1);
    q.drop_col0 = p.drop_col0 + n0;
    if (q.bias) q.bias += n0;
    if (q.bias2) q.bias2 += n0;
    if (q.out1) q.out1 = (float*)adv(q.out1, (size_t)n0, q.io & 2);
    if (q.in0) q.in0 = adv(q.in0, (size_t)n0, q.io & 4);
    if (q.in1) q.in1 = adv(q.in1, (size_t)n0, q.io & 8);
    if (q.c32) q.c32 += n0;
    if (q.gin) q.gin += n0;
    if (q.in2) q.in2 = adv(q.in2, (size_t)n0, q.io & 16);
    if (q.out2) q.out2 = (float*)adv(q.out2, (size_t)n0, q.io & 32);
    if (scorer_blocks) { q.w2 += n0; q.e_atomic = 1; }
    if (scorer_parts) { q.w2 += n0; q.e = p.e + (size_t)(n0 / bn) * (size_t)e_block_stride; q.e_atomic = 2; }
    if (att_blocks) { q.w2 += n0; q.u += n0; q.e = p.e + (size_t)(n0 / bn) * (size_t)e_block_stride; q.e_atomic = 2; }      // (2: own partial buffer, plain stores)
    if (L.nprob == GH_MAX_PROBLEMS) flush();
    L.p[L.nprob++] = q;
    const int bm_eff = row_tile(tn, tn_pp, q.elt, bm);
    const int mt = (q.M + bm_eff - 1) / bm_eff;
    if (mt > L.m_tiles) L.m_tiles = mt;
    if (tn_pp && (q.N + 255) / 256 > L.n_tiles) L.n_tiles = (q.N + 255) / 256;
    if (q.seg[0].K > k_total) k_total = q.seg[0].K;
  }
}

void Batch::flush() {
  if (L.nprob == 0 || err != hipSuccess) { reset(); return; }
  if (tn) {
    bool has_cs[GH_MAX_PROBLEMS];
    for (int i = 0; i < L.nprob; ++i) has_cs[i] = cs_out[i] != nullptr;
    const TnPlan P = tn_split_plan(L, tn_pp, k_total, has_cs, g_ws != nullptr, g_ws_bytes, gemm_mode());
    L.kchunk = P.kchunk; L.ksplit = P.ksplit; L.per = P.per;
    if (P.want_cs && !P.cs_in_launch) {
      // this launch cannot carry its column sums (no workspace, generic kernel): fp32 operands get them from the streaming
      // kernel right here, so that a Batch whose problems span several launches (h = 768: 21 column-block problems) never ends
      // up with some bias gradients fused and others missing; bf16 operands have no such kernel -- the caller is told
      for (int i = 0; i < L.nprob; ++i) {
        if (!cs_out[i]) continue;
        const Seg& sg = L.p[i].seg[0];
        if (L.p[i].elt || sg.lda != L.p[i].M) { colsum_missed = true; continue; }
        if (launch_colsum3(sg.A, nullptr, nullptr, cs_out[i], nullptr, nullptr, sg.K, L.p[i].M, s, cs_out2[i], nullptr, nullptr)) colsum_missed = true;
        else colsum_fused = true;
      }
    }
    if (P.use_ws) {
      ReduceArgs R;
      R.n = L.nprob;
      for (int i = 0; i < L.nprob; ++i) {
        Problem& q = L.p[i];
        float* w = g_ws + P.tile_off[i];
        R.it[i] = ReduceItem{w, q.C, q.M, q.N, q.ldc, L.ksplit, (long long)q.M * q.N};
        q.C = w; q.ldc = q.N; q.epi = EPI_STORE; q.accumulate = 0; q.split_stride = (long long)q.M * q.N;
      }
      const int n_tiles = R.n;      // bias-gradient partials [ksplit][M] behind the tiles, summed into one or two outputs
      for (int i = 0; i < L.nprob && P.cs_in_launch; ++i) {
        Problem& q = L.p[i];
        if (!cs_out[i]) continue;
        float* w = g_ws + P.cs_off[i];
        q.colsum = w; q.colsum_stride = q.M;
        R.it[R.n++] = ReduceItem{w, cs_out[i], 1, q.M, q.M, L.ksplit, (long long)q.M};
        if (cs_out2[i] && R.n - n_tiles < GH_MAX_PROBLEMS) R.it[R.n++] = ReduceItem{w, cs_out2[i], 1, q.M, q.M, L.ksplit, (long long)q.M};
      }
      hipError_t e = launch_any();
      if (e != hipSuccess) err = e;
      // one reduce launch: the bias-gradient partials ride behind the tiles (their workgroups beyond the first exit at once)
      e = launch_reduce_partials(R, P.reduce_elems, s);
      if (R.n > n_tiles) colsum_fused = true;
      if (e != hipSuccess) err = e;
      reset();
      return;
    }
  }
  if (tn && tn_pp) { err = hipErrorInvalidValue; reset(); return; }      // (the ping-pong kernel writes partial tiles only: no workspace, no launch)
  if (!tn && nt_split()) return;
  hipError_t e = launch_any();
  if (e != hipSuccess) err = e;
  reset();
}

hipError_t Batch::launch_any() {
  const ConfigPlan c = gemm_config(L, tn, tn_pp, big, narrow, wide, wide256, gemm_mode());
  if (c.cfg == CFG_TN_PP) return launch_tn_pp(L, s);
  L.m_tiles = c.m_tiles;
  const bool fast = fast_checked(L, tn);
  return launch_gemm(c.cfg, L, tn, fast, gemm_grid(L, tn, fast), s);
}

// the few-row split-K plan (gemm_plan.h nt_split_plan), when it applies: the launch into the workspace and its finish kernel
bool Batch::nt_split() {
  const NtSplitPlan P = nt_split_plan(L, g_ws != nullptr, g_ws_bytes);
  if (!P.ok) return false;
  FinishArgs F;
  F.n = L.nprob;
  F.split = P.finish_split;
  for (int i = 0; i < L.nprob; ++i) {
    Problem& q = L.p[i];
    float* w = g_ws + P.off[i];
    F.it[i] = FinishItem{w, (long long)q.M * q.N, P.ks, q.M, q.N, q.epi, q.accumulate, q.ldc,
                         q.C, q.bias, q.bias2, q.out1, q.in0, q.in1, q.u, q.w2, q.e, q.ldu, q.R, q.heads, q.rowg};
    q.C = w; q.ldc = q.N; q.epi = EPI_STORE; q.accumulate = 0; q.bias = nullptr; q.bias2 = nullptr;
    q.split_stride = (long long)q.M * q.N;
  }
  L.ksplit = P.ks;
  L.kchunk = P.ct * 16;
  hipError_t e = launch_any();
  if (e != hipSuccess) err = e;
  e = launch_nt_finish(F, P.finish_grid, s);
  split_done = true;
  if (e != hipSuccess) err = e;
  reset();
  return true;
}

}  // namespace gh
