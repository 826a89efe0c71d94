// The GGNN cell, forward and backward, on the GEMM engine (gemm_batch.h) and the streaming launchers of common.h: host code
// only, no kernel.  See include/get_hip.h for the contract of the four entry points.
#include "../../include/get_hip.h"
#include "gemm_batch.h"
#include "common.h"

using namespace gh;

// bf: bf16 storage pipeline -- x (or the table behind ids), the weights and xp/a/z/rr/rx/hh/out hold bf16 (pointers typed
// float* all the same); out32 then receives the fp32 copy of the cell output.  Biases, score_w and score_x stay fp32.
int gh::cell_fwd_impl(int bf, float* out32, const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                const int32_t* goff, int m_real, int m_rows,
                                const float* x, const int32_t* ids, int n, int r, int din, int h,
                                const float* w_p, const float* w_z0, const float* w_z1, const float* w_r0,
                                const float* w_r1, const float* w_h0, const float* w_h1,
                                const float* b_z0, const float* b_z1, const float* b_r0, const float* b_r1,
                                const float* b_h0, const float* b_h1,
                                float* xp, float* a, float* z, float* rr, float* rx, float* hh, float* out,
                                float drop_p, uint32_t drop_seed,
                                const float* score_w, float* score_x, float score_drop_p, uint32_t score_drop_seed,
                                gh_stream_t stream, int pad_out_dead, int* score_parts, float* xdrop) {
  hipStream_t s = (hipStream_t)stream;
  if (score_parts) *score_parts = 1;
  GH_REQUIRE(n > 0 && r > 0 && din > 0 && h > 0, "ggnn_cell_fwd: bad sizes n=%d r=%d din=%d h=%d", n, r, din, h);
  // (out32 may be NULL when no consumer reads the cell output as fp32: composite forward -- the first cell's scorer projection is fused,
  //  the second cell's word attention reads the bf16 rows)
  GH_REQUIRE(!bf || (din % 8 == 0 && h % 8 == 0), "ggnn_cell_fwd_bf16: needs din %% 8 == 0, h %% 8 == 0 (din=%d h=%d)", din, h);
  if (!goff) { m_real = n * r; m_rows = n * r; }
  GH_REQUIRE(m_real >= 0 && m_real <= m_rows && m_rows <= n * r, "ggnn_cell_fwd: node-compact rows %d/%d do not fit n*r=%d", m_real, m_rows, n * r);
  const int M = m_rows;
  if (M == 0) return 0;
  GH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "ggnn_cell_fwd: dropout p=%f not in [0,1)", drop_p);
  // the stateless dropout mask hashes a 32-BIT element index row * width + column (device_utils.h drop_hash): beyond 2^32 elements
  // two rows would share their mask
  GH_REQUIRE((drop_p <= 0.f && score_drop_p <= 0.f) || (long long)M * (long long)(din > h ? din : h) < (1LL << 32),
             "ggnn_cell_fwd: %d rows x %d columns exceed the dropout mask's 32-bit element index", M, din > h ? din : h);
  GH_REQUIRE((score_w == nullptr) == (score_x == nullptr), "ggnn_cell_fwd: score_w and score_x come together");
  GH_REQUIRE(score_drop_p >= 0.f && score_drop_p < 1.f, "ggnn_cell_fwd: scorer dropout p=%f not in [0,1)", score_drop_p);
  const bool wide = bf && h % 256 == 0;      // 128 x 256 bf16 tiles cover the width exactly (h = 768)
  // bf16 storage with dropout: masking the A fragments costs ~100 VALU instructions per 16-row tile and K tile (eight hashes on
  // packed bf16 pairs) against 8 MFMAs -- the projection ran at half the rate of the same product without a mask (configs[4]:
  // 376 us against ~190).  With a scratch row buffer from the caller (xdrop [m_rows][din] bf16) the masked operand -- gathered
  // embedding rows included -- is materialised once by the streaming kernel the backward used anyway (launch_gather_rows), the
  // projection reads it as a plain operand, and the backward's dW_proj re-uses it instead of gathering again.
  const bool pre_drop = bf && xdrop && drop_p > 0.f && din <= h;
  if (pre_drop) {
    if (int e = launch_gather_rows(x, ids, xdrop, M, din, s, drop_p, drop_seed, 1)) return e;
  }
  {  // xp = dropout(x) Wp^T   (wrapper.py:189-191); embedding rows gathered by the loader, the dropout mask applied to the fragments
    Batch b(false, M, s, wide, SITE_CELL_PROJ, h);
    Problem p = pre_drop ? gemm_problem(M, h, EPI_STORE, xp, h, xdrop, din, w_p, din, din, nullptr, bf)
                         : gemm_problem(M, h, EPI_STORE, xp, h, x, din, w_p, din, din, ids, bf);
    p.io = bf ? 1 : 0;
    if (!pre_drop) set_dropout(p, 1, din, drop_p, drop_seed);
    b.add(p);
    b.flush();
    GH_REQUIRE(b.err != hipErrorInvalidValue || drop_p == 0.f, "ggnn_cell_fwd: fused dropout needs float4-shaped rows (din=%d, h=%d)", din, h);
    GH_CHECK_HIP(b.err);
  }
  bool partial_zero = false;
  // zero fills of this cell -- the padding rows of `a` that a row tile can touch (below) and the scorer's partial dot products
  // (two column blocks add into score_x) -- ride on the aggregation launch when its kernel variant takes them: two memset
  // dispatches less per step
  ZeroFill zf = {nullptr, 0, nullptr, 0};
  bool zf_done = false, score_zero = false;
  if (score_w) {
    Batch bh(false, M, s, false, SITE_CELL_H, h);
    score_zero = bh.narrow && h <= 2 * bh.bn && h > bh.bn;
  }
  if (m_rows > m_real) {
    // padding rows of the node-compact layout have no neighbours.  The fast gate GEMMs skip the aggregation segment for
    // every row tile at or beyond seg0_rows (= m_real), so only the tile that straddles m_real ever reads such rows: zero
    // the rows up to the next 128-row boundary (the largest row tile) plus one tile instead of all (m_rows - m_real) of
    // them (40 MB at the bench shape).  Only when the operands are shaped for the fast kernel -- the generic kernel
    // reads every row; the launches below are checked to have taken the fast path.
    const uintptr_t al = (uintptr_t)a | (uintptr_t)xp | (uintptr_t)z | (uintptr_t)rr | (uintptr_t)rx | (uintptr_t)hh | (uintptr_t)out |
                         (uintptr_t)w_z0 | (uintptr_t)w_z1 | (uintptr_t)w_r0 | (uintptr_t)w_r1 | (uintptr_t)w_h0 | (uintptr_t)w_h1 |
                         (uintptr_t)b_z0 | (uintptr_t)b_z1 | (uintptr_t)b_r0 | (uintptr_t)b_r1 | (uintptr_t)b_h0 | (uintptr_t)b_h1;
    // (and only while the activations stay below the 2 GB a buffer descriptor addresses: beyond that the gate GEMMs take the
    //  generic kernel -- fast_ok -- which reads every row)
    partial_zero = ((al & 15) == 0) && (h % (bf ? 8 : 4) == 0) && h >= 4 && 4.0 * (double)h * (double)M < 2147483648.0;
    const int zfull = ((m_real + 127) / 128 + 1) * 128;
    const int zend = (partial_zero && zfull < m_rows) ? zfull : m_rows;
    if (!bf) { zf.p0 = a + (size_t)m_real * h; zf.n0 = (long long)(zend - m_real) * h; }
    if (!bf && score_zero && M % 4 == 0) { zf.p1 = score_x; zf.n1 = M; }
    if (int e = launch_spmm(bits, dinv, vals, keep, goff, m_real, xp, a, n, r, h, 0, 0, s, bf, bf ? nullptr : &zf, &zf_done)) return e;   // a = A_hat xp (:192)
    if (!zf_done)
      GH_CHECK_HIP(hipMemsetAsync((char*)a + (size_t)m_real * h * (bf ? 2 : 4), 0, (size_t)(bf ? 2 : 4) * (size_t)(zend - m_real) * h, s));
  } else {
    if (int e = launch_spmm(bits, dinv, vals, keep, goff, m_real, xp, a, n, r, h, 0, 0, s, bf)) return e;   // a = A_hat xp (:192)
  }
  const long long generic_before = generic_launches();
  {  // z, r gates (:194-200): [a | xp] . [W?0 | W?1]^T as two K segments
    Batch b(false, M, s, wide, SITE_CELL_ZR, h);
    Problem pz = gemm_problem(M, h, EPI_SIGMOID_Z, z, h, a, h, w_z0, h, h, nullptr, bf);
    pz.io = bf ? 1 : 0;
    add_seg(pz, xp, h, w_z1, h, h);
    pz.bias = b_z0; pz.bias2 = b_z1;
    Problem pr = gemm_problem(M, h, EPI_SIGMOID_R, rr, h, a, h, w_r0, h, h, nullptr, bf);
    pr.io = bf ? 7 : 0;
    add_seg(pr, xp, h, w_r1, h, h);
    pr.bias = b_r0; pr.bias2 = b_r1; pr.out1 = rx; pr.in0 = xp;
    if (m_rows > m_real) pz.seg0_rows = pr.seg0_rows = (m_real > 0 ? m_real : 1);
    b.add(pz); b.add(pr);
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  {  // h gate and the convex update (:202-206); optionally the GSL word scorer's projection of the result (:167)
    // score_parts (caller provides score_x for ceil(h / column block) x M floats): rows wider than two column blocks keep their
    // tile and every block writes its share of the projection to a partial of its own ([block][M]; gh_scorer_gsl score_parts)
    const bool parts_ok = score_w && score_parts != nullptr;
    Batch b(false, M, s, wide && (!score_w || parts_ok), SITE_CELL_H, h);
    if (parts_ok && h > b.bn && !(b.narrow && h <= 2 * b.bn)) {
      b.e_block_stride = M;
      *score_parts = (h + b.bn - 1) / b.bn;
    } else if (score_w && b.narrow) {
      if (h > 2 * b.bn) { b.narrow = false; b.bn = 320; }      // more than two column blocks: whole rows on the 320-wide tile
      else if (h > b.bn && !(zf_done && zf.p1 == score_x)) GH_CHECK_HIP(hipMemsetAsync(score_x, 0, sizeof(float) * (size_t)M, s));   // two blocks add their partial dot products
    }
    Problem ph = gemm_problem(M, h, EPI_TANH_H, hh, h, a, h, w_h0, h, h, nullptr, bf);
    ph.io = bf ? 15 : 0; ph.c32 = bf ? out32 : nullptr;
    add_seg(ph, rx, h, w_h1, h, h);
    ph.bias = b_h0; ph.bias2 = b_h1; ph.out1 = out; ph.in0 = z; ph.in1 = xp;
    if (m_rows > m_real) ph.seg0_rows = (m_real > 0 ? m_real : 1);
    if (score_w) {
      ph.w2 = score_w; ph.e = score_x;
      if (pad_out_dead && m_rows > m_real) ph.ldu = 1;
      set_dropout(ph, 2, h, score_drop_p, score_drop_seed);
    }
    b.add(ph);
    b.flush();
    GH_REQUIRE(b.err != hipErrorInvalidValue || !score_w, "ggnn_cell_fwd: the fused scorer projection needs h %% 4 == 0 and h <= 320 (h=%d)", h);
    GH_CHECK_HIP(b.err);
  }
  GH_REQUIRE(!partial_zero || generic_launches() == generic_before,
             "ggnn_cell_fwd: internal -- a gate GEMM took the generic kernel although the padding rows of `a` were only zeroed for the fast one");
  return 0;
}

extern "C" int gh_ggnn_cell_fwd(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                const int32_t* goff, int m_real, int m_rows,
                                const float* x, const int32_t* ids, int n, int r, int din, int h,
                                const float* w_p, const float* w_z0, const float* w_z1, const float* w_r0,
                                const float* w_r1, const float* w_h0, const float* w_h1,
                                const float* b_z0, const float* b_z1, const float* b_r0, const float* b_r1,
                                const float* b_h0, const float* b_h1,
                                float* xp, float* a, float* z, float* rr, float* rx, float* hh, float* out,
                                float drop_p, uint32_t drop_seed,
                                const float* score_w, float* score_x, float score_drop_p, uint32_t score_drop_seed,
                                gh_stream_t stream) {
  return cell_fwd_impl(0, nullptr, bits, dinv, vals, keep, goff, m_real, m_rows, x, ids, n, r, din, h, w_p, w_z0, w_z1, w_r0, w_r1,
                       w_h0, w_h1, b_z0, b_z1, b_r0, b_r1, b_h0, b_h1, xp, a, z, rr, rx, hh, out, drop_p, drop_seed, score_w,
                       score_x, score_drop_p, score_drop_seed, stream, 0, nullptr, nullptr);
}

extern "C" int gh_ggnn_cell_fwd_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                     const int32_t* goff, int m_real, int m_rows,
                                     const void* x, const int32_t* ids, int n, int r, int din, int h,
                                     const void* w_p, const void* w_z0, const void* w_z1, const void* w_r0,
                                     const void* w_r1, const void* w_h0, const void* w_h1,
                                     const float* b_z0, const float* b_z1, const float* b_r0, const float* b_r1,
                                     const float* b_h0, const float* b_h1,
                                     void* xp, void* a, void* z, void* rr, void* rx, void* hh, void* out, float* out32,
                                     float drop_p, uint32_t drop_seed,
                                     const float* score_w, float* score_x, float score_drop_p, uint32_t score_drop_seed,
                                     gh_stream_t stream) {
  typedef const float* cf;
  typedef float* mf;
  return cell_fwd_impl(1, out32, bits, dinv, vals, keep, goff, m_real, m_rows, (cf)x, ids, n, r, din, h, (cf)w_p, (cf)w_z0, (cf)w_z1,
                       (cf)w_r0, (cf)w_r1, (cf)w_h0, (cf)w_h1, b_z0, b_z1, b_r0, b_r1, b_h0, b_h1, (mf)xp, (mf)a, (mf)z, (mf)rr,
                       (mf)rx, (mf)hh, (mf)out, drop_p, drop_seed, score_w, score_x, score_drop_p, score_drop_seed, stream, 0, nullptr, nullptr);
}

// bf: bf16 storage pipeline -- x / table, wt_*, the saved xp..hh and the scratch dhp..da hold bf16; g, dx and every weight /
// bias gradient stay fp32.
int gh::cell_bwd_impl(int bf, const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                const int32_t* goff, int m_real,
                                const float* x, const int32_t* ids, int n, int r, int din, int h,
                                const float* wt_p, const float* wt_z0, const float* wt_z1, const float* wt_r0,
                                const float* wt_r1, const float* wt_h0, const float* wt_h1,
                                const float* xp, const float* a, const float* z, const float* rr, const float* rx,
                                const float* hh, const float* g,
                                float* dhp, float* dzp, float* drp, float* dxp, float* da,
                                float* dx, float* dw_p, float* dw_z0, float* dw_z1, float* dw_r0, float* dw_r1,
                                float* dw_h0, float* dw_h1, float* db_z, float* db_r, float* db_h,
                                float* db_z1, float* db_r1, float* db_h1, float drop_p, uint32_t drop_seed,
                                gh_stream_t stream, gh_stream_t wstream, hipEvent_t ev_l1, hipEvent_t ev_agg,
                                int pre_done, const GateFuse* next, const float* xdrop, float* ybuf, int nodx_ok) {
  hipStream_t s = (hipStream_t)stream;
  // Weight-gradient stream (composite backward, model_ops.hip): the split-K weight-gradient GEMMs only need dzp / drp / dhp
  // (final after the first dX launch) and, for dW_proj, dxp (final after the aggregation).  On their own stream they run
  // underneath the rest of the chain -- the streaming kernels of one stream (gate_bwd_pre, aggregation, gather, partial
  // reduces) hide under the other stream's MFMA-bound launches, which two launches on ONE stream never do.
  hipStream_t sw = wstream ? (hipStream_t)wstream : s;
  const bool two = sw != s;
  GH_REQUIRE(!two || (ev_l1 && ev_agg), "ggnn_cell_bwd: a separate weight-gradient stream needs its two events");
  GH_REQUIRE(n > 0 && r > 0 && din > 0 && h > 0, "ggnn_cell_bwd: bad sizes");
  GH_REQUIRE(!bf || (din % 8 == 0 && h % 8 == 0 && din <= h), "ggnn_cell_bwd_bf16: needs din %% 8 == 0, h %% 8 == 0, din <= h (din=%d h=%d)", din, h);
  if (!goff) m_real = n * r;
  GH_REQUIRE(m_real >= 0 && m_real <= n * r, "ggnn_cell_bwd: node-compact rows %d do not fit n*r=%d", m_real, n * r);
  GH_REQUIRE(drop_p <= 0.f || (long long)n * r * (long long)din < (1LL << 32),
             "ggnn_cell_bwd: %d rows x %d columns exceed the dropout mask's 32-bit element index", n * r, din);
  const int M = m_real;      // padding rows receive no gradient and contribute none
  if (M == 0) return 0;
  // out = h z + xp (1-z):  dhp = g z (1-h^2), dzp = g (h-xp) z (1-z), dxp = g (1-z)
  // (pre_done: the GEMM that produced g already wrote the three straight from its epilogue, EPI_GATE_PRE -- g itself was
  //  never stored and gate_bwd_pre's 4 reads + 3 writes shrink to the 3 + 3 the producing epilogue added)
  if (!pre_done)
    if (int e = launch_gate_bwd_pre(g, z, hh, xp, dhp, dzp, dxp, (size_t)M * h, s, bf)) return e;
  const bool wide = bf && h % 256 == 0;
  // No input gradient leaves this cell (frozen embeddings behind ids, or an input that needs none): da and the full dxp would
  // only feed dW_p.  With X the masked, gathered input rows, Y = A_hat X (so a = Y Wp^T, xp = X Wp^T) and E = dxp after the
  // d(r xp) product, the weight gradients re-associate:
  //     T_g = G_g^T Y (g = z, r, h), S_g = G_g^T X (g = z, r)            five h x din outputs over the M rows
  //     dW_g0 = T_g Wp^T,  dW_g1 = S_g Wp^T,  dW_p = E^T X + Wz1^T S_z + Wr1^T S_r + sum_g W_g0^T T_g
  // Four of the five activation-sized NT products (da from three gates, dxp from two) are gone, the aggregation moves from da
  // to X, and ten weight-sized products (launch_nn_accumulate) finish the job.  T / S live in the tail of the stream's split-K
  // workspace, which the weight-gradient launches are told not to use.
  const size_t ts_floats = 5 * (size_t)h * (size_t)din;
  const Workspace wsp = workspace_for(s);
  const bool nodx = nodx_ok && !dx && !next && !bf && !two && din <= h && din % 4 == 0 && h % 4 == 0 && wsp.p != nullptr &&
                    (reinterpret_cast<uintptr_t>(wsp.p) & 15) == 0 && wsp.bytes / 2 >= ts_floats * sizeof(float);
  if (nodx) {
    const size_t hd = (size_t)h * (size_t)din;
    float* ts = wsp.p + wsp.bytes / sizeof(float) - ts_floats;      // (wsp.bytes and 20 h din are multiples of 16)
    float *t_z = ts, *t_r = ts + hd, *t_h = ts + 2 * hd, *s_z = ts + 3 * hd, *s_r = ts + 4 * hd;
    const size_t ws_left = wsp.bytes - ts_floats * sizeof(float);
    {  // d(r xp) = dhp Wh1 -> drp, dxp += .   (no da)
      Batch b(false, M, s, false, SITE_CELL_BWD_H, h);
      Problem p1 = gemm_problem(M, h, EPI_BWD_DRX, drp, h, dhp, h, wt_h1, h, h);
      p1.out1 = dxp; p1.in0 = xp; p1.in1 = rr;
      b.add(p1);
      b.flush();
      GH_CHECK_HIP(b.err);
    }
    const float* X = x;
    if (ids || drop_p > 0.f) {      // embedding gather and / or the forward's dropout mask, once, into the free `da` scratch
      if (int e = launch_gather_rows(x, ids, da, M, din, s, drop_p, drop_seed, 0)) return e;
      X = da;
    }
    bool cs_ok = false;
    auto add_s = [&](Batch& b) {      // the problems that read X and E
      b.add(tn_problem(h, din, s_z, din, dzp, h, X, din, M));  if (!ybuf) b.want_colsum(db_z, db_z1);
      b.add(tn_problem(h, din, s_r, din, drp, h, X, din, M));  if (!ybuf) b.want_colsum(db_r, db_r1);
      b.add(tn_problem(h, h, dw_h1, h, dhp, h, rx, h, M));     if (!ybuf) b.want_colsum(db_h, db_h1);
      b.add(tn_problem(h, din, dw_p, din, dxp, h, X, din, M));
    };
    if (ybuf) {  // one weight-gradient launch; the zero fill of T / S rides on the aggregation
      ZeroFill zf = {ts, (long long)ts_floats, nullptr, 0};
      bool zf_done = false;
      if (int e = launch_spmm(bits, dinv, vals, keep, goff, m_real, X, ybuf, n, r, din, 0, 0, s, 0, &zf, &zf_done)) return e;   // Y = A_hat X
      if (!zf_done) GH_CHECK_HIP(hipMemsetAsync(ts, 0, ts_floats * sizeof(float), s));
      Batch b(true, M, s);
      b.g_ws_bytes = ws_left;
      b.add(tn_problem(h, din, t_z, din, dzp, h, ybuf, din, M));  b.want_colsum(db_z, db_z1);
      b.add(tn_problem(h, din, t_r, din, drp, h, ybuf, din, M));  b.want_colsum(db_r, db_r1);
      b.add(tn_problem(h, din, t_h, din, dhp, h, ybuf, din, M));  b.want_colsum(db_h, db_h1);
      add_s(b);
      b.flush();
      GH_CHECK_HIP(b.err);
      cs_ok = b.colsum_fused && !b.colsum_missed;
    } else {     // no second row buffer: X and E first, then Y takes the place of dxp
      GH_CHECK_HIP(hipMemsetAsync(ts, 0, ts_floats * sizeof(float), s));
      Batch b(true, M, s);
      b.g_ws_bytes = ws_left;
      add_s(b);
      b.flush();
      GH_CHECK_HIP(b.err);
      cs_ok = b.colsum_fused && !b.colsum_missed;
      if (int e = launch_spmm(bits, dinv, vals, keep, goff, m_real, X, dxp, n, r, din, 0, 0, s, 0)) return e;   // Y = A_hat X
      Batch b2(true, M, s);
      b2.g_ws_bytes = ws_left;
      b2.add(tn_problem(h, din, t_z, din, dzp, h, dxp, din, M));
      b2.add(tn_problem(h, din, t_r, din, drp, h, dxp, din, M));
      b2.add(tn_problem(h, din, t_h, din, dhp, h, dxp, din, M));
      b2.flush();
      GH_CHECK_HIP(b2.err);
    }
    NnArgs R;
    memset(&R, 0, sizeof(R));
    R.n = 6;
    NnItem& ip = R.it[0];      // dW_p first: five terms, its tiles run longest
    ip.C = dw_p; ip.I = h; ip.J = din; ip.ldc = din;
    nn_add_term(ip, wt_z0, h, t_z, din, h);
    nn_add_term(ip, wt_r0, h, t_r, din, h);
    nn_add_term(ip, wt_h0, h, t_h, din, h);
    nn_add_term(ip, wt_z1, h, s_z, din, h);
    nn_add_term(ip, wt_r1, h, s_r, din, h);
    float* const dwg[5] = {dw_z0, dw_r0, dw_h0, dw_z1, dw_r1};
    for (int i = 0; i < 5; ++i) {      // dW_g0 = T_g Wp^T, dW_g1 = S_g Wp^T (wt_p = Wp^T as stored, [din][h])
      NnItem& it = R.it[1 + i];
      it.C = dwg[i]; it.I = h; it.J = h; it.ldc = h;
      nn_add_term(it, ts + i * hd, din, wt_p, h, din);
    }
    if (int e = launch_nn_accumulate(R, s)) return e;
    if (cs_ok) return 0;
    return launch_colsum3(dzp, drp, dhp, db_z, db_r, db_h, M, h, s, db_z1, db_r1, db_h1);
  }
  {  // hp = a Wh0^T + (r xp) Wh1^T:  da = dhp Wh0 ; d(r xp) = dhp Wh1 -> drp, dxp += .
    Batch b(false, M, s, wide, SITE_CELL_BWD_H, h);
    Problem p0 = gemm_problem(M, h, EPI_STORE, da, h, dhp, h, wt_h0, h, h, nullptr, bf);
    Problem p1 = gemm_problem(M, h, EPI_BWD_DRX, drp, h, dhp, h, wt_h1, h, h, nullptr, bf);
    p1.out1 = dxp; p1.in0 = xp; p1.in1 = rr;
    p0.io = bf ? 1 : 0; p1.io = bf ? 15 : 0;
    b.add(p0); b.add(p1);
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  const bool cs = bf ? true : (h % 4 == 0);      // (any float4-shaped width since round 5: Batch::flush satisfies every request itself)
  // the six gate weight gradients with their bias gradients: on the weight-gradient stream right after the first dX launch when
  // there is one (two), else with dW_proj at the end
  auto add_gate_wgrads = [&](Batch& b) {
    b.add(tn_problem(h, h, dw_z0, h, dzp, h, a, h, M, nullptr, bf));  if (cs) b.want_colsum(db_z, db_z1);
    b.add(tn_problem(h, h, dw_z1, h, dzp, h, xp, h, M, nullptr, bf));
    b.add(tn_problem(h, h, dw_r0, h, drp, h, a, h, M, nullptr, bf));  if (cs) b.want_colsum(db_r, db_r1);
    b.add(tn_problem(h, h, dw_r1, h, drp, h, xp, h, M, nullptr, bf));
    b.add(tn_problem(h, h, dw_h0, h, dhp, h, a, h, M, nullptr, bf));  if (cs) b.want_colsum(db_h, db_h1);
    b.add(tn_problem(h, h, dw_h1, h, dhp, h, rx, h, M, nullptr, bf));
  };
  bool colsum_done = false;
  if (two) {  // six of the seven weight gradients start here, on the weight-gradient stream
    GH_CHECK_HIP(hipEventRecord(ev_l1, s));
    GH_CHECK_HIP(hipStreamWaitEvent(sw, ev_l1, 0));
    Batch b(true, M, sw);
    add_gate_wgrads(b);
    b.flush();
    GH_CHECK_HIP(b.err);
    colsum_done = b.colsum_fused && !b.colsum_missed;
    if (!colsum_done) {
      GH_REQUIRE(!bf, "ggnn_cell_bwd_bf16: the bias gradients need the split-K workspace (gh_set_workspace)");
      if (int e = launch_colsum3(dzp, drp, dhp, db_z, db_r, db_h, M, h, sw, db_z1, db_r1, db_h1)) return e;
    }
  }
  {  // da += dzp Wz0 + drp Wr0 ; dxp += dzp Wz1 + drp Wr1
    Batch b(false, M, s, wide, SITE_CELL_BWD_ZR, h);
    Problem p0 = gemm_problem(M, h, EPI_STORE, da, h, dzp, h, wt_z0, h, h, nullptr, bf);
    add_seg(p0, drp, h, wt_r0, h, h);
    p0.accumulate = 1;
    Problem p1 = gemm_problem(M, h, EPI_STORE, dxp, h, dzp, h, wt_z1, h, h, nullptr, bf);
    add_seg(p1, drp, h, wt_r1, h, h);
    p1.accumulate = 1;
    p0.io = p1.io = bf ? 1 : 0;
    b.add(p0); b.add(p1);
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  if (int e = launch_spmm(bits, dinv, vals, keep, goff, m_real, da, dxp, n, r, h, 1, 1, s, bf)) return e;   // dxp += A_hat^T da
  if (two) {
    GH_CHECK_HIP(hipEventRecord(ev_agg, s));
    GH_CHECK_HIP(hipStreamWaitEvent(sw, ev_agg, 0));
  }
  if (dx || next) {  // dx = (dxp Wp) . mask/(1-p)
    GH_REQUIRE(!next || (din % 4 == 0 && (next->bf16 != 0) == (bf != 0)), "ggnn_cell_bwd: the fused gate head needs float4-shaped rows and both cells in the same storage mode");
    Batch b(false, M, s, wide && din % 256 == 0, SITE_CELL_BWD_DX, din);
    Problem p = gemm_problem(M, din, next ? EPI_GATE_PRE : EPI_STORE, next ? next->dhp : dx, din, dxp, h, wt_p, h, h, nullptr, bf);      // dx itself is fp32
    if (next) {      // dx IS the gradient w.r.t. the previous cell's output: write that cell's dhp / dzp / dxp instead of dx
      p.in0 = next->z; p.in1 = next->hh; p.in2 = next->xp; p.out1 = next->dzp; p.out2 = next->dxp;
      p.io = next->bf16 ? (1 | 2 | 4 | 8 | 16 | 32) : 0;
    }
    set_dropout(p, 3, din, drop_p, drop_seed);
    b.add(p);
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  {  // weight gradients: G^T X over the M rows, split-K partial tiles + reduce.  The bias gradients are the column
     // sums of dzp / drp / dhp: they ride along with the first GEMM that streams each of them (no separate
     // column-sum pass over 3 x M x h values) whenever the launch takes the workspace path.
    Batch b(true, M, sw);
    if (!two) add_gate_wgrads(b);
    if (bf && xdrop && drop_p > 0.f && din <= h) {
      // the forward left the masked (and gathered) operand rows in xdrop (cell_fwd_impl pre_drop): no second gather pass
      b.add(tn_problem(h, din, dw_p, din, dxp, h, xdrop, din, M, nullptr, bf));
    } else if ((ids || drop_p > 0.f || bf) && din <= h) {
      // operand rows materialised once into the (now free) `da` scratch -- embedding gather and/or the forward's
      // dropout mask applied in that one streaming pass -- so the split-K GEMM loader stays a plain copy
      if (int e = launch_gather_rows(x, ids, da, M, din, sw, drop_p, drop_seed, bf)) return e;
      b.add(tn_problem(h, din, dw_p, din, dxp, h, da, din, M, nullptr, bf));
    } else {
      GH_REQUIRE(drop_p == 0.f, "ggnn_cell_bwd: fused dropout needs din (%d) <= h (%d)", din, h);
      b.add(tn_problem(h, din, dw_p, din, dxp, h, x, din, M, ids));
    }
    b.flush();
    GH_CHECK_HIP(b.err);
    if (two || (b.colsum_fused && !b.colsum_missed)) return 0;
  }
  GH_REQUIRE(!bf, "ggnn_cell_bwd_bf16: the bias gradients need the split-K workspace (gh_set_workspace)");
  return launch_colsum3(dzp, drp, dhp, db_z, db_r, db_h, M, h, s, db_z1, db_r1, db_h1);
}

extern "C" int gh_ggnn_cell_bwd(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                const int32_t* goff, int m_real,
                                const float* x, const int32_t* ids, int n, int r, int din, int h,
                                const float* wt_p, const float* wt_z0, const float* wt_z1, const float* wt_r0,
                                const float* wt_r1, const float* wt_h0, const float* wt_h1,
                                const float* xp, const float* a, const float* z, const float* rr, const float* rx,
                                const float* hh, const float* g,
                                float* dhp, float* dzp, float* drp, float* dxp, float* da,
                                float* dx, float* dw_p, float* dw_z0, float* dw_z1, float* dw_r0, float* dw_r1,
                                float* dw_h0, float* dw_h1, float* db_z, float* db_r, float* db_h,
                                float* db_z1, float* db_r1, float* db_h1, float drop_p, uint32_t drop_seed,
                                gh_stream_t stream) {
  return cell_bwd_impl(0, bits, dinv, vals, keep, goff, m_real, x, ids, n, r, din, h, wt_p, wt_z0, wt_z1, wt_r0, wt_r1, wt_h0, wt_h1,
                       xp, a, z, rr, rx, hh, g, dhp, dzp, drp, dxp, da, dx, dw_p, dw_z0, dw_z1, dw_r0, dw_r1, dw_h0, dw_h1,
                       db_z, db_r, db_h, db_z1, db_r1, db_h1, drop_p, drop_seed, stream, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1);
}

extern "C" int gh_ggnn_cell_bwd_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                                     const int32_t* goff, int m_real,
                                     const void* x, const int32_t* ids, int n, int r, int din, int h,
                                     const void* wt_p, const void* wt_z0, const void* wt_z1, const void* wt_r0,
                                     const void* wt_r1, const void* wt_h0, const void* wt_h1,
                                     const void* xp, const void* a, const void* z, const void* rr, const void* rx,
                                     const void* hh, const float* g,
                                     void* dhp, void* dzp, void* drp, void* dxp, void* da,
                                     float* dx, float* dw_p, float* dw_z0, float* dw_z1, float* dw_r0, float* dw_r1,
                                     float* dw_h0, float* dw_h1, float* db_z, float* db_r, float* db_h,
                                     float* db_z1, float* db_r1, float* db_h1, float drop_p, uint32_t drop_seed,
                                     gh_stream_t stream) {
  typedef const float* cf;
  typedef float* mf;
  return cell_bwd_impl(1, bits, dinv, vals, keep, goff, m_real, (cf)x, ids, n, r, din, h, (cf)wt_p, (cf)wt_z0, (cf)wt_z1, (cf)wt_r0,
                       (cf)wt_r1, (cf)wt_h0, (cf)wt_h1, (cf)xp, (cf)a, (cf)z, (cf)rr, (cf)rx, (cf)hh, g, (mf)dhp, (mf)dzp, (mf)drp,
                       (mf)dxp, (mf)da, dx, dw_p, dw_z0, dw_z1, dw_r0, dw_r1, dw_h0, dw_h1, db_z, db_r, db_h, db_z1, db_r1,
                       db_h1, drop_p, drop_seed, stream, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1);
}
