// The concat attention and the linear layers on the GEMM engine (gemm_batch.h) and the streaming launchers of common.h: host code
// only, no kernel.  See include/get_hip.h for the contract of the entry points.
#include "../../include/get_hip.h"
#include "gemm_batch.h"
#include "common.h"
#include "device_utils.h"

using namespace gh;

// Concat attention, generalised for the composite model entry points (model_ops.hip):
//   nl / rowu: `left` has nl rows and output row m takes the left projection u[rowu[m]] (the word level's left input is the
//              CLAIM vector: one u row per claim instead of one per pair; rowu = NULL keeps nl == b and the per-pair map);
//   att_out / att_ld: where `attended` goes (row pitch att_ld >= dr * heads: straight into a wider concatenation buffer).
int gh::att_fwd_impl(const float* left, int nl, const int32_t* rowu, const float* right, const float* mask, const int32_t* goff,
                 const int32_t* rowg, int m_real, int b, int l, int xl, int dr, int ha, int heads, const float* w1, const float* w2,
                 float* u, float* t, float* e, float* weights, float* attended, hipStream_t s, int u_mode,
                 const void* right16, const void* w1_16) {
  GH_REQUIRE(heads >= 1 && heads <= 8, "concat_att: heads=%d not in [1,8]", heads);
  GH_REQUIRE(b > 0 && l > 0 && dr > 0 && ha > 0, "concat_att_fwd: bad sizes");
  GH_REQUIRE(u_mode >= 0 && u_mode <= 2, "concat_att_fwd: u_mode %d not in {0,1,2}", u_mode);
  GH_REQUIRE((goff == nullptr) == (rowg == nullptr), "concat_att_fwd: goff and rowg come together");
  if (!goff) m_real = b * l;
  GH_REQUIRE(m_real >= 0 && m_real <= b * l, "concat_att_fwd: node-compact rows %d do not fit b*l=%d", m_real, b * l);
  if (!rowu && u_mode != 1) nl = b;      // (the u-only call names its row count itself)
  const int M = m_real;
  const bool one_block = ha <= Batch(false, M, s).bn;      // column block of the tile configuration this launch will use
  GH_REQUIRE(one_block || (ha % 4 == 0 && aligned16(t) && aligned16(u) && aligned16(w2)),
             "concat_att_fwd: attention hidden %d wider than one column block needs float4-shaped rows", ha);
  const int xl_in = (left && xl > 0) ? xl : 0;      // column offset of the right branch inside linear1.weight
  if (u_mode != 2) {
    if (left && xl > 0) {  // u = W1[:, :xl] . left -- once per pair / claim, not per token (two_branches_attention.py:137-140)
      Batch bt(false, nl, s);
      bt.add(gemm_problem(nl, ha, EPI_STORE, u, ha, left, xl, w1, xl + dr, xl));
      bt.flush();
      GH_CHECK_HIP(bt.err);
    } else {
      GH_CHECK_HIP(hipMemsetAsync(u, 0, sizeof(float) * (size_t)nl * ha, s));
    }
  }
  if (u_mode == 1) return 0;
  if (!(left && xl > 0)) xl = 0;
  const int32_t* urow = rowu ? rowu : rowg;
  const float* e_parts = nullptr;
  int n_parts = 0;
  bool right_is16 = false;
  if (M > 0) {  // t = tanh(W1[:, xl:] . right_t + u) ; e = W2 t  (:140-141)
    // bf16 storage mode with the twins at hand (right16 = the producing cell's bf16 output, w1_16 = bf16(linear1.weight)): the
    // product runs on the bf16-storage kernel (v_mfma_f32_16x16x32_bf16 from bf16 LDS images, half the operand bytes) instead of
    // rounding fp32 fragments in registers (MODE 1) -- the same bf16 operand values, fp32 accumulation and fp32 t either way
    const bool use16 = right16 && w1_16 && gemm_mode() == 1 && M >= 8192 && dr % 8 == 0 && (xl_in + dr) % 8 == 0 && xl_in % 8 == 0 && ha % 8 == 0;
    GH_REQUIRE(use16 || right, "concat_att_fwd: no fp32 right operand and the bf16 twins do not apply");
    right_is16 = use16;
    Batch bt(false, M, s, use16 && ha % 256 == 0);
    Problem p = use16 ? gemm_problem(M, ha, EPI_ATT, t, ha, (const float*)right16, dr,
                                     (const float*)((const unsigned short*)w1_16 + xl_in), xl_in + dr, dr, nullptr, 1)
                      : gemm_problem(M, ha, EPI_ATT, t, ha, right, dr, w1 + xl_in, xl_in + dr, dr);
    p.u = u; p.ldu = ha; p.R = l; p.w2 = w2; p.heads = heads; p.e = e; p.rowg = urow;
    // wide hidden layer (h = 768): a row spans several column blocks.  Activation-sized launches let every block reduce its share
    // of the head scores into a partial buffer of its own (stream workspace; att_softmax_fwd sums the partials in block order);
    // without the workspace (or for few-row launches, whose split-K plan finishes whole rows anyway) the product is stored and the
    // tanh + W2 reduction runs as a row-per-wave pass over it.
    bool blocks = false;
    if (!one_block) {
      const int nb = (ha + bt.bn - 1) / bt.bn;
      const Workspace wsp = workspace_for(s);
      const size_t need = (size_t)nb * (size_t)M * heads * sizeof(float);
      if (M >= 8192 && wsp.p && need <= wsp.bytes && ha % 4 == 0) {
        blocks = true;
        bt.e_block_stride = (long long)M * heads;
        p.e = wsp.p;
        e_parts = wsp.p; n_parts = nb;
      } else {
        p.epi = EPI_STORE;
      }
    }
    bt.add(p);
    bt.flush();
    GH_CHECK_HIP(bt.err);
    if (!one_block && !blocks)
      if (int err = launch_att_finish(t, u, w2, e, urow, M, ha, l, heads, s)) return err;
  }
  // (bf16 storage mode: the weighted sum reads the bf16 rows the product above read -- the caller need not keep an fp32 copy)
  return launch_att_softmax_fwd(e, mask, right, goff, m_real, b, l, dr, heads, weights, attended, s, e_parts, n_parts,
                                (long long)M * heads, right_is16 ? right16 : nullptr);   // (:142-147)
}

extern "C" int gh_concat_att_fwd(const float* left, const float* right, const float* mask, const int32_t* goff,
                                 const int32_t* rowg, int m_real, int b, int l, int xl,
                                 int dr, int ha, int heads, const float* w1, const float* w2,
                                 float* u, float* t, float* e, float* weights, float* attended,
                                 gh_stream_t stream) {
  return att_fwd_impl(left, b, nullptr, right, mask, goff, rowg, m_real, b, l, xl, dr, ha, heads, w1, w2, u, t, e, weights, attended,
                      (hipStream_t)stream);
}

// Backward.  claim_offsets / nl / du_c (all or none): the left input has nl rows, one per CLAIM, and pair p belongs to the
// claim c with claim_offsets[c] <= p < claim_offsets[c+1]: the per-pair du is summed per claim into du_c [nl][ha] first and
// dleft / the left part of dw1 are computed from (du_c, left) over nl rows.  dleft_accumulate: dleft += .
int gh::att_bwd_impl(const float* left, const float* right, const int32_t* goff, int m_real, int b, int l,
                 int xl, int dr, int ha, int heads, const float* w1t, const float* w2, const float* t, const float* weights,
                 const float* g_att, const float* g_w, float* de, float* dpre, float* du,
                 float* dleft, float* dright, float* dw1, float* dw2,
                 const int32_t* claim_offsets, int nl, float* du_c, int dleft_accumulate, hipStream_t s,
                 const int32_t* rowg, float* dw_tmp, const GateFuse* next, int dleft_late, float* dw2_buf,
                 const void* right16, const void* w1t_16) {
  GH_REQUIRE(heads >= 1 && heads <= 8, "concat_att: heads=%d not in [1,8]", heads);
  if (!goff) m_real = b * l;
  GH_REQUIRE(m_real >= 0 && m_real <= b * l, "concat_att_bwd: node-compact rows %d do not fit b*l=%d", m_real, b * l);
  GH_REQUIRE((claim_offsets == nullptr) == (du_c == nullptr), "concat_att_bwd: claim_offsets and du_c come together");
  const int M = m_real;
  if (!left) xl = 0;
  if (!claim_offsets) nl = b;
  const float* dul = claim_offsets ? du_c : du;      // the left branch's pre-activation gradient, one row per left row
  const int ldw = xl + dr;
  // Two-phase use (the caller may put the weight gradient of linear1 on another stream): dw1 == NULL skips its two
  // launches; dright == NULL is the complementary "dw1 only" call on buffers (dpre, du) a first call has filled.
  const bool weights_only = (dright == nullptr);
  GH_REQUIRE(!weights_only || dw1, "concat_att_bwd: dright == NULL asks for the dw1-only phase, which needs dw1");
  // bf16 storage mode with the twins at hand: dpre is produced as bf16 (the products below round it to bf16 anyway) and the
  // dright / dW1 products run on the bf16-storage kernels -- same operand values as the in-register rounding of MODE 1
  const bool use16 = right16 && w1t_16 && gemm_mode() == 1 && m_real >= 8192 && dr % 8 == 0 && ha % 8 == 0 && xl % 8 == 0;
  void* const dpre16 = use16 ? (void*)dpre : nullptr;
  float* dw2_part = nullptr;
  if (!weights_only) {
  int dw_written = 0;
  if (int e = launch_att_softmax_bwd(right, weights, g_att, g_w, goff, m_real, b, l, dr, heads, de, dright, s, rowg, dw_tmp, &dw_written,
                                     use16 ? right16 : nullptr)) return e;
  // dW2 = de^T t rides along with the dpre pass (per-pair partials in the workspace, one reduce)
  const size_t dw2_bytes = (size_t)b * heads * ha * sizeof(float);
  const Workspace wsp = workspace_for(s);
  const bool late = dleft_late && dw2_buf && ha % 4 == 0;      // partials in the caller's buffer, reduced by the second call
  dw2_part = late ? dw2_buf : ((wsp.p && dw2_bytes <= wsp.bytes && ha % 4 == 0) ? wsp.p : nullptr);
  if (int e = launch_att_dpre(de, w2, t, goff, m_real, b, l, ha, heads, dpre, du, dw2_part, s, dw_written ? dw_tmp : nullptr,
                              dw_written ? weights : nullptr, dw_written ? de : nullptr, dpre16,
                              (long long)m_real * heads, dw_written > 1 ? dw_written : 1)) return e;
  if (dw2_part && !late)
    if (int e = launch_reduce_wave(dw2_part, b, dw2, heads, ha, s)) return e;
  if (claim_offsets && xl > 0 && !dleft_late)
    if (int e = gh_seg_sum(du, claim_offsets, du_c, nl, ha, (gh_stream_t)s)) return e;
  const float* w1t_r16 = use16 ? (const float*)((const unsigned short*)w1t_16 + (size_t)xl * ha) : nullptr;
  GH_REQUIRE(!next || !next->bf16 || use16, "concat_att_bwd: a bf16 gate head needs the bf16 twins of right and w1t");
  if (M > 0 && next) {  // dright (= the gradient of the cell that produced `right`) is consumed by that cell's gate head only:
    Batch bt(false, M, s, use16 && dr % 256 == 0, SITE_ATT_BWD_DRIGHT, dr);      // g = softmax part (in dright) + dpre W1[:, xl:] goes straight into dhp / dzp / dxp
    Problem p = use16 ? gemm_problem(M, dr, EPI_GATE_PRE, next->dhp, dr, (const float*)dpre16, ha, w1t_r16, ha, ha, nullptr, 1)
                      : gemm_problem(M, dr, EPI_GATE_PRE, next->dhp, dr, dpre, ha, w1t + (size_t)xl * ha, ha, ha);
    p.gin = dright; p.in0 = next->z; p.in1 = next->hh; p.in2 = next->xp; p.out1 = next->dzp; p.out2 = next->dxp;
    p.io = next->bf16 ? (1 | 2 | 4 | 8 | 16 | 32) : 0;
    bt.add(p);
    bt.flush();
    GH_CHECK_HIP(bt.err);
  } else if (M > 0) {  // dright += dpre W1[:, xl:]
    Batch bt(false, M, s, use16 && dr % 256 == 0);
    Problem p = use16 ? gemm_problem(M, dr, EPI_STORE, dright, dr, (const float*)dpre16, ha, w1t_r16, ha, ha, nullptr, 1)
                      : gemm_problem(M, dr, EPI_STORE, dright, dr, dpre, ha, w1t + (size_t)xl * ha, ha, ha);
    p.accumulate = 1;
    bt.add(p);
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  if (xl > 0 && dleft && !dleft_late) {  // dleft = du W1[:, :xl]
    Batch bt(false, nl, s);
    Problem p = gemm_problem(nl, xl, EPI_STORE, dleft, xl, dul, ha, w1t, ha, ha);
    p.accumulate = dleft_accumulate ? 1 : 0;
    bt.add(p);
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  if (!dw2_part && M > 0) {  // no workspace: `heads` rows are not float4-shaped, so this one takes the generic kernel
    Batch bt(true, M, s);
    bt.add(tn_problem(heads, ha, dw2, ha, de, heads, t, ha, M));
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  }
  if (weights_only && dleft_late) {
    if (dw2_buf && ha % 4 == 0)      // the first call left the per-pair dW2 partials in dw2_buf
      if (int e = launch_reduce_wave(dw2_buf, b, dw2, heads, ha, s)) return e;
    if (claim_offsets && xl > 0)
      if (int e = gh_seg_sum(du, claim_offsets, du_c, nl, ha, (gh_stream_t)s)) return e;
  }
  if (weights_only && dleft_late && xl > 0 && dleft) {  // the left gradient, deferred to this (weight-gradient stream) call
    Batch bt(false, nl, s);
    Problem p = gemm_problem(nl, xl, EPI_STORE, dleft, xl, dul, ha, w1t, ha, ha);
    p.accumulate = dleft_accumulate ? 1 : 0;
    bt.add(p);
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  if (!dw1) return 0;
  if (M > 0) {
    Batch bt(true, M, s);
    if (use16) bt.add(tn_problem(ha, dr, dw1 + xl, ldw, (const float*)dpre16, ha, (const float*)right16, dr, M, nullptr, 1));
    else bt.add(tn_problem(ha, dr, dw1 + xl, ldw, dpre, ha, right, dr, M));
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  if (xl > 0) {
    Batch bt(true, nl, s);
    bt.add(tn_problem(ha, xl, dw1, ldw, dul, ha, left, xl, nl));
    bt.flush();
    GH_CHECK_HIP(bt.err);
  }
  return 0;
}

extern "C" int gh_concat_att_bwd(const float* left, const float* right, const int32_t* goff, int m_real, int b, int l,
                                 int xl, int dr, int ha, int heads, const float* w1t, const float* w2, const float* t, const float* weights,
                                 const float* g_att, const float* g_w, float* de, float* dpre, float* du,
                                 float* dleft, float* dright, float* dw1, float* dw2, gh_stream_t stream) {
  return att_bwd_impl(left, right, goff, m_real, b, l, xl, dr, ha, heads, w1t, w2, t, weights, g_att, g_w, de, dpre, du, dleft, dright,
                      dw1, dw2, nullptr, b, nullptr, 0, (hipStream_t)stream, nullptr, nullptr, nullptr);
}

// y[m][n] = [x0 | x1] . W^T + bias with W [n][k0 + k1] as stored: the head's first layer on the concatenation
// [claim vector | attended evidences] (graph_based_semantic_structure.py:251-267) without materialising the concatenation.
// w_out / b_out / y_out / n_out (optional): a second linear layer of n_out <= 8 columns on top (the head's out[1], 300 -> 2 classes):
// y_out = y . w_out^T + b_out rides in the split-K finish kernel when the product takes that plan, else one extra launch.
int gh::linear2_fwd(const float* x0, int k0, const float* x1, int k1, const float* w, const float* bias, float* y, int m, int n, hipStream_t s,
                    const float* w_out, const float* b_out, float* y_out, int n_out) {
  Batch b(false, m, s);
  Problem p = gemm_problem(m, n, EPI_STORE, y, n, x0, k0, w, k0 + k1, k0);
  if (k1 > 0) add_seg(p, x1, k1, w + k0, k0 + k1, k1);
  p.bias = bias;
  const bool two = w_out && y_out && n_out >= 1;
  const bool fuse = two && n_out <= 8 && n % 4 == 0 && n <= b.bn && aligned16(w_out);
  if (fuse) { p.w2 = w_out; p.e = y_out; p.heads = n_out; p.in0 = b_out; }
  b.add(p);
  b.flush();
  GH_CHECK_HIP(b.err);
  if (two && !(fuse && b.split_done)) return launch_tiny_linear_fwd(y, w_out, b_out, y_out, m, n, n_out, s);
  return 0;
}
// dx0 [m][k0] (+)= g Wt[:k0] ; dx1 [m][k1] = g Wt[k0:] (wt = W^T [k0+k1][n]) ; dw [n][k0+k1] += g^T [x0 | x1] ; db += colsum(g).
// dx_only / dw_only split the call in two phases (weight gradients on another stream).
int gh::linear2_bwd(const float* x0, int k0, const float* x1, int k1, const float* wt, const float* g, int m, int n,
                float* dx0, int dx0_accumulate, float* dx1, float* dw, float* db, hipStream_t s) {
  if (dx0 || dx1) {
    Batch b(false, m, s);
    if (dx0) { Problem p = gemm_problem(m, k0, EPI_STORE, dx0, k0, g, n, wt, n, n); p.accumulate = dx0_accumulate ? 1 : 0; b.add(p); }
    if (dx1 && k1 > 0) b.add(gemm_problem(m, k1, EPI_STORE, dx1, k1, g, n, wt + (size_t)k0 * n, n, n));
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  if (dw) {
    Batch b(true, m, s);
    b.add(tn_problem(n, k0, dw, k0 + k1, g, n, x0, k0, m));
    if (k1 > 0) b.add(tn_problem(n, k1, dw + k0, k0 + k1, g, n, x1, k1, m));
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  if (db) return launch_colsum(g, db, m, n, s);
  return 0;
}

extern "C" int gh_linear_fwd(const float* x, const float* w, const float* bias, float* y, int m, int k, int n,
                             gh_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  GH_REQUIRE(m > 0 && k > 0 && n > 0, "linear_fwd: bad sizes");
  if (n <= 8) return launch_tiny_linear_fwd(x, w, bias, y, m, k, n, s);      // the 2-class head: one wave per row
  Batch b(false, m, s);
  Problem p = gemm_problem(m, n, EPI_STORE, y, n, x, k, w, k, k);
  p.bias = bias;
  b.add(p);
  b.flush();
  GH_CHECK_HIP(b.err);
  return 0;
}

extern "C" int gh_linear_wgrad_bf16(const void* g16, int ldg, const void* x16, int ldx, int m, int n, int k,
                                    float* dw, int lddw, float* db, gh_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  GH_REQUIRE(m > 0 && k > 0 && n > 0 && g16 && x16 && dw, "linear_wgrad_bf16: bad arguments");
  GH_REQUIRE(n % 8 == 0 && k % 8 == 0 && ldg % 8 == 0 && ldx % 8 == 0 && ldg >= n && ldx >= k && lddw >= k && lddw % 4 == 0,
             "linear_wgrad_bf16: widths and leading dimensions must be multiples of 8 (lddw: of 4)");
  GH_REQUIRE(((reinterpret_cast<uintptr_t>(g16) | reinterpret_cast<uintptr_t>(x16) | reinterpret_cast<uintptr_t>(dw)) & 15) == 0,
             "linear_wgrad_bf16: operands must be 16-byte aligned");
  Batch b(true, m, s);
  GH_REQUIRE(b.g_ws != nullptr, "linear_wgrad_bf16: needs the split-K workspace (gh_set_workspace)");
  b.add(tn_problem(n, k, dw, lddw, (const float*)g16, ldg, (const float*)x16, ldx, m, nullptr, 1));
  if (db) b.want_colsum(db, nullptr);
  b.flush();
  GH_CHECK_HIP(b.err);
  GH_REQUIRE(!db || (b.colsum_fused && !b.colsum_missed), "linear_wgrad_bf16: the bias gradient did not fit the split-K workspace");
  return 0;
}

extern "C" int gh_linear_bwd(const float* x, const float* wt, const float* w, const float* g, int m, int k, int n, float* dx,
                             float* dw, float* db, gh_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  GH_REQUIRE(m > 0 && k > 0 && n > 0, "linear_bwd: bad sizes");
  if (n <= 8 && w) return launch_tiny_linear_bwd(x, w, g, dx, dw, db, m, k, n, s);
  if (dx) {
    Batch b(false, m, s);
    b.add(gemm_problem(m, k, EPI_STORE, dx, k, g, n, wt, n, n));
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  if (dw) {
    Batch b(true, m, s);
    b.add(tn_problem(n, k, dw, k, g, n, x, k, m));
    b.flush();
    GH_CHECK_HIP(b.err);
  }
  if (db) return launch_colsum(g, db, m, n, s);
  return 0;
}
