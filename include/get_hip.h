/*
 * get_hip.h -- C-ABI of libget_hip.so, the MI355X (gfx950) implementation of the
 * CRIPAC-DIG/GET hot path: sliding-window word-graph build, gated graph cells with
 * graph-structure-learning (GSL) top-k refinement, and the word-/evidence-level
 * multi-head "concat" attention.
 *
 * The reference has no FFI boundary of its own (it is pure Python on ATen); its
 * boundary is the nn.Module API listed in SURVEY.md section 8(b).  Every entry
 * point below names the reference function whose device work it replaces
 * (paths relative to the upstream tree).  get_amd/ mirrors the reference's
 * module classes on top of these.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; all float data is
 *     fp32, dense, row-major; ids are int32; adjacency bit rows are uint64 words
 *   - nothing allocates: outputs and scratch are caller-provided
 *   - stream-ordered; `stream` is a hipStream_t passed as void*.  Calls carry all their state in their arguments
 *     except three pieces of process configuration: the split-K scratch (registered per stream with
 *     gh_set_stream_workspace, or one default buffer with gh_set_workspace -- concurrent streams that both run
 *     backward passes need one buffer each), the GEMM arithmetic mode (gh_set_gemm_mode, set before launching work)
 *     and the measurement hook (gh_profile_*, single stream by design)
 *   - returns 0 on success, non-zero on error (message via gh_last_error());
 *     never aborts the process
 *
 * Packed adjacency of one graph with R (padded) nodes, W = ceil(R/64):
 *   bits[R][W]  uint64  bit j of row i set  <=>  A[i][j] != 0
 *   dinv[R]     float   deg(i)^-1/2 of the binary graph (0 for padding rows);
 *                       edge weight = dinv[i]*dinv[j]       ("normalised" mode)
 *   vals[R][R]  float   optional dense edge weights; when non-NULL they are used
 *                       instead of dinv ("weighted" mode: any dense adjacency
 *                       the reference API hands over)
 *   keep[W]     uint64  optional GSL keep-set; refined edge (i,j) exists iff
 *                       bit(i,j) && (keep(i) || keep(j))    (wrapper.py:221-225)
 *
 * Node-compact row layout (optional; `goff` != NULL selects it, NULL keeps the reference's padded layout).
 * The reference pads every evidence graph to R nodes and runs all of them through the GGNN cells
 * (graph_based_semantic_structure.py:99-107); a padding node has no edges and is masked out of the attention
 * (:180), so it never influences a real node's output or any gradient -- its only observable effect is that its
 * score competes in GSL's top-k (wrapper.py:216-219).  In the compact layout the n graphs' REAL nodes are stored
 * back to back and all padding nodes after them:
 *   goff[n+1]   int32   goff[g] = first feature row of graph g's real nodes; m_real = goff[n]
 *   node j <  n_g of graph g  ->  feature row goff[g] + j
 *   node j >= n_g of graph g  ->  feature row m_real + (g*R - goff[g]) + (j - n_g)         (m_tot = n*R rows in all)
 * Kernels that only matter for real nodes (second cell, attention, every backward) then run on the first m_real
 * rows; the first cell's forward and the scorer still see all m_tot rows.  bits/dinv/vals/keep, scores and ids keep
 * their padded [g][R] indexing.  `m_real` is passed by value, so the host must know it (sum of the node counts).
 */
#ifndef GET_HIP_H
#define GET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gh_stream_t;

#define GH_ABI_VERSION 10

int gh_abi_version(void);
/* Thread-local message of the last failing call on this thread (never NULL). */
const char* gh_last_error(void);

/* ---- a1  graph build: interactions.py:334-351 convert_text + :11-18 _laplacian_normalize ----
 * tokens[n_texts][fixed_length] raw token sequence (post-padded), lengths[n_texts].
 * Out: node_ids[n_texts][fixed_length] de-duplicated ids in first-occurrence order (0 padded),
 *      n_nodes[n_texts], bits[n_texts][R][W], dinv[n_texts][R]   (R = fixed_length). */
int gh_graph_build(const int32_t* tokens, const int32_t* lengths, int n_texts, int fixed_length, int window,
                   int32_t* node_ids, int32_t* n_nodes, uint64_t* bits, float* dinv, gh_stream_t stream);

/* Dense adjacency handed over by the reference API ((N,R,R) float64 from handlers/mz_sampler.py:146,
 * cast by `.float()` at graph_based_semantic_structure.py:99,149) -> packed bits + fp32 values.  The bit pattern is the
 * union of A's and A^T's non-zero patterns (entries present on one side only carry the value 0), so that the
 * transposed aggregation of the backward pass sees every entry of an adjacency whose pattern is not symmetric. */
int gh_adj_pack_f64(const double* adj, int n, int r, uint64_t* bits, float* vals, gh_stream_t stream);
int gh_adj_pack_f32(const float* adj, int n, int r, uint64_t* bits, float* vals, gh_stream_t stream);

/* De-padding of what the reference fitter holds before its per-claim loop
 * (Fitting/FittingFC/char_man_fitter_query_repr1.py:196-250: `evd_doc_contents` (b, n_max, r) ids and `evd_docs_adj`
 * (b, n_max, r, r) float64, `[:evd_count]` sliced claim by claim with two host syncs each) in one launch:
 * pair p = sum(counts[:c]) + j for every slot j < counts[c] (counts clamped to [0, n_max]) gets its ids narrowed to int32
 * (d_ids [b*n_max][r], rows [0, pairs) written), its adjacency packed as gh_adj_pack_f64 does (bits [b*n_max][r][W],
 * vals [b*n_max][r][r] -- see below) and its number of real nodes (id >= 1) in n_nodes [b*n_max].
 * The adjacency convert_text produces (interactions.py:11-18: D^-1/2 A D^-1/2 of a binary graph) is RECOGNISED: for such a
 * pair only bits and dinv [b*n_max][r] (= 1 / sqrt(row degree), exactly as gh_graph_build writes it) are written -- the
 * kernels' "normalised" mode -- and vals stays untouched, unless force_vals != 0.
 * stats[5] (device, int64): {pairs, real nodes over all pairs, pairs whose ids are not prefix-shaped or whose padding
 * nodes carry edges -- must be 0 for the node-compact layout (gh_ragged_plan) to apply --, pairs whose values are NOT the
 * normalised graph (0: hand bits + dinv to the kernels; > 0: the batch needs the weighted mode -- call again with
 * force_vals = 1 so that vals is complete), reserved}. */
int gh_ref_depad(const int64_t* counts, int b, int n_max, int r, const void* ids, int ids_i64, const double* adj,
                 int32_t* d_ids, uint64_t* bits, float* vals, float* dinv, int32_t* n_nodes, int64_t* stats, int force_vals,
                 gh_stream_t stream);

/* Node-compact layout plan from the node counts of gh_graph_build (device arrays):
 *   goff[n+1] (see above); rowg[n*r] graph of every compact row; src[n*r] padded row index g*r+j of every compact
 *   row (scatter/gather between the two layouts); cids[n*r] = node_ids[src[.]] and maskf[n*r] = (cids >= 1) as float,
 *   the word attention's mask (both NULL ok: not written). */
int gh_ragged_plan(const int32_t* n_nodes, const int32_t* node_ids, int n, int r, int32_t* goff, int32_t* rowg,
                   int32_t* src, int32_t* cids, float* maskf, gh_stream_t stream);

/* ---- aggregation  a = A_hat x : Models/BiDAF/wrapper.py:192 `adj.matmul(x)` ----
 * x,y [n][r][h] (goff == NULL) or node-compact [m_real][h].  transpose: use A^T (backward of the weighted mode);
 * accumulate: y += . */
int gh_spmm(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
            const int32_t* goff, int m_real, const float* x, float* y, int n, int r, int h, int transpose,
            int accumulate, gh_stream_t stream);

/* The same aggregation on the bf16 storage pipeline's activations (what gh_ggnn_cell_fwd_bf16 / _bwd_bf16 run internally, exposed for
 * the parity test and the micro-benchmark): x16, y16 hold bf16, 16-byte aligned rows, h % 8 == 0.  Graphs of r <= 128 nodes run as a
 * dense product per graph on the matrix pipe (the fp32 edge weights split three ways into bf16: products exact to fp32 precision,
 * fp32 accumulation), larger ones on the edge-list kernel (fp32 sums in the fp32 kernel's order); either way ONE rounding to bf16
 * at the store (accumulate: y16 is read, added in fp32, rounded once). */
int gh_spmm_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                 const int32_t* goff, int m_real, const void* x16, void* y16, int n, int r, int h, int transpose,
                 int accumulate, gh_stream_t stream);

/* ---- weight packing: W[n_out][n_in] -> Wt[n_in][n_out] ----
 * The MFMA GEMMs take both operands contraction-contiguous: forward products x.W^T use the weight exactly as
 * PyTorch stores it, the backward's dX = g.W needs the transposed copy made here (refreshed once per optimiser step). */
int gh_transpose(const float* w, float* wt, int rows, int cols, gh_stream_t stream);
/* All weights of a model in one launch: n matrices, HOST arrays of device pointers and sizes. */
int gh_transpose_batch(int n, const void* const* src_host, void* const* dst_host, const int* rows_host,
                       const int* cols_host, gh_stream_t stream);

/* ---- a2  GGNN cell: Models/BiDAF/wrapper.py:188-208 GGNN.forward ----
 * Input rows are x[m][din] (m = n*r), or emb[ids[m]][din] when ids != NULL (fused
 * embedding gather, graph_based_semantic_structure.py:100,150).
 * w_*: the reference's linear.weight tensors as stored: w_p[h][din]; w_z0,w_z1,w_r0,w_r1,w_h0,w_h1 [h][h].
 * b_?0, b_?1: the two biases of every gate (each [h]); the epilogues add both.
 * Saved for backward (all [m][h]): xp, a, z, r, rx, hh.  out [m][h].
 * drop_p > 0: the cell's input dropout (wrapper.py:185-190) is applied inside the first GEMM's loader with a
 * stateless mask -- element (m,k) kept iff hash(drop_seed, m*din+k) >= drop_p*2^32, scaled by 1/(1-drop_p);
 * pass the same (drop_p, drop_seed) to the backward.  Needs din % 4 == 0 and h % 4 == 0.
 * goff != NULL: node-compact layout; the cell runs on the first m_rows rows (m_real <= m_rows <= n*r; rows beyond
 * m_real are padding nodes: no neighbours).  goff == NULL: m_real/m_rows are ignored, m = n*r.
 * NOTE (node-compact, m_rows > m_real): rows >= m_real of the SAVED tensors r (`rr`) and h~ (`hh`) are UNDEFINED on return --
 * they are backward-only state and the backward never touches a padding row, so the fast epilogues do not store them
 * (xp, a, z, rx and out ARE written for every row < m_rows).  Do not dump or reuse those rows.
 * score_w/score_x (both or neither; needs h % 4 == 0 and h <= 320): the GSL word scorer that consumes this cell's
 * output (wrapper.py:167, GGNN(h->1)) starts with proj(dropout(out)), a [m][h] x [h] product; with score_w[h] =
 * that proj weight the last GEMM's epilogue writes score_x[m] = dropout(out)[m] . score_w while `out` is still in
 * registers (mask = the scorer's own: hash(score_drop_seed, m*h+k) >= score_drop_p*2^32), and gh_scorer_gsl then
 * takes score_x instead of re-reading `out`. */
int gh_ggnn_cell_fwd(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                     const int32_t* goff, int m_real, int m_rows,
                     const float* x, const int32_t* ids, int n, int r, int din, int h,
                     const float* w_p, const float* w_z0, const float* w_z1, const float* w_r0,
                     const float* w_r1, const float* w_h0, const float* w_h1,
                     const float* b_z0, const float* b_z1, const float* b_r0, const float* b_r1,
                     const float* b_h0, const float* b_h1,
                     float* xp, float* a, float* z, float* rr, float* rx, float* hh, float* out,
                     float drop_p, uint32_t drop_seed,
                     const float* score_w, float* score_x, float score_drop_p, uint32_t score_drop_seed,
                     gh_stream_t stream);

/* Backward of the cell.  wt_*: TRANSPOSED weights (gh_transpose of linear.weight): wt_p[din][h], the others [h][h].
 * g [m][h] = dL/dout.  Scratch (all [m][h]): dhp, dzp, drp, dxp, da.
 * Outputs: dx [m][din] (may be NULL: frozen embedding), and ACCUMULATED (+=) into
 * dw_p[h][din], dw_z0..dw_h1 [h][h], db_z[h], db_r[h], db_h[h]  (caller zeroes them, or hands the
 * parameters' own .grad buffers).  b?0 and b?1 share one gradient: db_z1/db_r1/db_h1 (NULL ok) receive
 * the same column sums, so both biases' .grad can be fed without a copy.
 * goff != NULL: node-compact layout, the backward runs on the m_real real-node rows only (padding rows get and give
 * no gradient; dx rows beyond m_real are not written).
 * Alignment (both fp32 entries): every tensor needs its element's alignment only (4 bytes).  16-byte aligned tensors whose
 * rows are a multiple of 4 floats take the vector kernels; anything else -- a width that is no multiple of 4, or a base
 * address off a 16-byte boundary, x / the table behind ids included -- takes kernels that touch single floats only (the
 * generic GEMM, gate_bwd_pre's scalar kernel, gather_rows' single-float loop), with the same results.  The bf16 entries
 * require 16-byte aligned tensors. */
int gh_ggnn_cell_bwd(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                     const int32_t* goff, int m_real,
                     const float* x, const int32_t* ids, int n, int r, int din, int h,
                     const float* wt_p, const float* wt_z0, const float* wt_z1, const float* wt_r0,
                     const float* wt_r1, const float* wt_h0, const float* wt_h1,
                     const float* xp, const float* a, const float* z, const float* rr, const float* rx,
                     const float* hh, const float* g,
                     float* dhp, float* dzp, float* drp, float* dxp, float* da,
                     float* dx, float* dw_p, float* dw_z0, float* dw_z1, float* dw_r0, float* dw_r1,
                     float* dw_h0, float* dw_h1, float* db_z, float* db_r, float* db_h,
                     float* db_z1, float* db_r1, float* db_h1, float drop_p, uint32_t drop_seed, gh_stream_t stream);

/* ---- bf16 STORAGE variant of the cell (BASELINE configs[4]: "h=768 bf16 ... MFMA projections") ----
 * Same computation and argument order as gh_ggnn_cell_fwd / _bwd with these tensors holding bf16 instead of fp32:
 *   forward : x (rows, or the embedding table behind ids), the seven weights, xp a z rr rx hh, out;
 *             out32 [m][h] fp32 additionally receives the cell output for the fp32 consumers (attention, scorer stays fused)
 *   backward: x / table, the seven TRANSPOSED weights, the saved xp..hh, the scratch dhp dzp drp dxp da
 * Biases, g, dx, score_w/score_x and every weight/bias gradient stay fp32; all arithmetic accumulates in fp32
 * (v_mfma_f32_16x16x32_bf16; gate math in fp32 registers).  Needs din % 8 == 0, h % 8 == 0, din <= h, at least 8192 rows
 * and the split-K workspace.  Results follow the fp32 path to bf16 accuracy (tests/test_gpu_model.py states the tolerances). */
int gh_ggnn_cell_fwd_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                          const int32_t* goff, int m_real, int m_rows,
                          const void* x, const int32_t* ids, int n, int r, int din, int h,
                          const void* w_p, const void* w_z0, const void* w_z1, const void* w_r0,
                          const void* w_r1, const void* w_h0, const void* w_h1,
                          const float* b_z0, const float* b_z1, const float* b_r0, const float* b_r1,
                          const float* b_h0, const float* b_h1,
                          void* xp, void* a, void* z, void* rr, void* rx, void* hh, void* out, float* out32,
                          float drop_p, uint32_t drop_seed,
                          const float* score_w, float* score_x, float score_drop_p, uint32_t score_drop_seed,
                          gh_stream_t stream);
int gh_ggnn_cell_bwd_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                          const int32_t* goff, int m_real,
                          const void* x, const int32_t* ids, int n, int r, int din, int h,
                          const void* wt_p, const void* wt_z0, const void* wt_z1, const void* wt_r0,
                          const void* wt_r1, const void* wt_h0, const void* wt_h1,
                          const void* xp, const void* a, const void* z, const void* rr, const void* rx,
                          const void* hh, const float* g,
                          void* dhp, void* dzp, void* drp, void* dxp, void* da,
                          float* dx, float* dw_p, float* dw_z0, float* dw_z1, float* dw_r0, float* dw_r1,
                          float* dw_h0, float* dw_h1, float* db_z, float* db_r, float* db_h,
                          float* db_z1, float* db_r1, float* db_h1, float drop_p, uint32_t drop_seed, gh_stream_t stream);

/* ---- a2(300->1) + a3  word scorer + GSL top-k: wrapper.py:167-168, GSL.forward :215-227 ----
 * feat [n][r][h]; w_p[h] = scorer proj.linear.weight; gate[12] = {wz0,bz0,wz1,bz1,wr0,br0,wr1,br1,
 * wh0,bh0,wh1,bh1} (the six 1x1 linears).  k = int(rate * r) computed by the caller.
 * Out: score[n][r], keep[n][W] (bit i set <=> node i among the k best; ties -> lower index).
 * drop_p/drop_seed: the scorer cell's own input dropout in training mode (same stateless mask as above).
 * goff != NULL: feat is node-compact [n*r][h] INCLUDING the padding rows (they compete in the top-k).
 * pads_collapsed (with goff, drop_p == 0 only): without dropout all padding rows of a batch are identical, so feat
 * holds just ONE of them, at row goff[n] (feat is [goff[n] + 1][h]); every padding node scores with that row.
 * Exactly one of feat / score_x is non-NULL: score_x[rows] = the projections proj(dropout(feat)) already produced by
 * gh_ggnn_cell_fwd's epilogue (same row indexing as feat; w_p, h and the dropout arguments are then unused). */
int gh_scorer_gsl(const uint64_t* bits, const float* dinv, const float* vals, const int32_t* goff, int pads_collapsed,
                  const float* feat, const float* score_x, const float* w_p, const float* gate, int n, int r, int h, int k,
                  float* score, uint64_t* keep, float drop_p, uint32_t drop_seed, gh_stream_t stream);
/* GSL alone on given scores (GSL.forward on arbitrary score input). */
int gh_gsl_topk(const float* score, int n, int r, int k, uint64_t* keep, gh_stream_t stream);
/* Dense view of a (refined) packed adjacency, for callers that want GSL.forward's dense result. */
int gh_adj_unpack(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                  int n, int r, float* adj, gh_stream_t stream);

/* ---- a5/a6  concat attention: thirdparty/two_branches_attention.py:121-148 (left != NULL) and
 *      thirdparty/self_attention.py:75-100 (left == NULL) ----
 * left [b][xl] (or NULL, xl = 0), right [b][l][dr], mask [b][l] float (0 = padded).
 * w1 = linear1.weight [ha][xl+dr] as stored; w2 = linear2.weight [heads][ha] (heads <= 8).
 * Saved: u [b][ha] (left branch, hoisted out of the per-token product), t [b*l][ha] (tanh), e [b*l][heads].
 * Out: weights [b][l][heads], attended [b][dr][heads].
 * goff/rowg != NULL (both): right, mask, t, e, weights are node-compact with m_real rows, pair g owning rows
 * [goff[g], goff[g+1]) (at most l of them) and rowg[row] = g; softmax runs over the pair's real rows only. */
int gh_concat_att_fwd(const float* left, const float* right, const float* mask, const int32_t* goff,
                      const int32_t* rowg, int m_real, int b, int l, int xl, int dr,
                      int ha, int heads, const float* w1, const float* w2,
                      float* u, float* t, float* e, float* weights, float* attended, gh_stream_t stream);
/* Backward.  w1t = transpose of linear1.weight: [xl+dr][ha].  g_att [b][dr][heads], g_w [b][l][heads] or NULL.
 * Scratch: de [b*l][heads], dpre [b*l][ha], du [b][ha].
 * Out: dleft [b][xl] (NULL ok), dright [b][l][dr]; ACCUMULATED: dw1 [ha][xl+dr], dw2 [heads][ha].
 * Two-phase use (e.g. the weight gradient of linear1 on another stream): dw1 == NULL leaves its launches out;
 * dright == NULL is the complementary call that computes ONLY dw1 from the dpre / du a first call has filled.
 * ha must be a multiple of 4 and at most 1024 (the pass through the tanh layer walks float4 columns, at most 256 per row): the
 * forward also accepts ha % 4 != 0 up to 320 and wider multiples of 4, the backward refuses both ("att_dpre: attention hidden ..."). */
int gh_concat_att_bwd(const float* left, const float* right, const int32_t* goff, int m_real, int b, int l, int xl,
                      int dr, int ha, int heads,
                      const float* w1t, const float* w2, const float* t, const float* weights,
                      const float* g_att, const float* g_w,
                      float* de, float* dpre, float* du,
                      float* dleft, float* dright, float* dw1, float* dw2, gh_stream_t stream);

/* ---- GEMM arithmetic mode (process-wide, default 0) ----
 * 0: exact fp32 MFMA everywhere -- the mode every parity claim and the headline benchmark are made in.
 * 1: (the host layer additionally routes the evidence cells through gh_ggnn_cell_*_bf16 in this mode) the big-tile GEMMs (cell gates, dX, attention projections with >= 8192 rows, and the split-K weight gradients)
 *    round their operands to bf16 while staging them in LDS and use v_mfma_f32_16x16x16_bf16 with fp32 accumulation;
 *    storage, epilogues, bias gradients and all small GEMMs stay fp32.  For BASELINE configs[4] ("h=768 bf16"); results then
 *    match the fp32 oracle to bf16 accuracy only (~1e-2 relative on logits). */
int gh_set_gemm_mode(int mode);
/* 2 ("fp32x3", opt-in): fp32 storage and results; every product of the activation-sized NT launches is formed on the bf16 MFMA
 *    from 3-way bf16 splits of both operands (six of the nine cross terms; error below one fp32 rounding of the product).
 * 3 ("fp32x3 with pre-split weights", opt-in): as 2, with the weight operand's pieces read from an image the library keeps
 *    per weight view (made on first use).  The caller tells the library when weights were rewritten: gh_weights_changed()
 *    marks every image stale (a stale image is re-made by the launch that meets it), gh_fp32x3_refresh(stream) re-makes all
 *    of them in one launch (call it after the optimiser step), gh_fp32x3_clear() frees them (before weights are freed). */
int gh_weights_changed(void);
int gh_fp32x3_refresh(gh_stream_t stream);
int gh_fp32x3_clear(void);

/* ---- split-K scratch for the weight-gradient GEMMs ----
 * Caller-owned device buffer (stays registered until replaced; NULL unregisters).  With it the
 * K-chunk partial tiles are written with plain stores and reduced by a second kernel; without it
 * (or when it is too small) the chunks add into the output with fp32 atomics.  All work that uses
 * it is ordered on the stream of the call, so one buffer serves one stream at a time. */
int gh_set_workspace(void* ptr, int64_t bytes);
/* The same, for work launched on `stream` of the CURRENT device only (takes precedence over the default buffer; NULL ptr
 * unregisters).  The registry is keyed by (hipGetDevice(), stream): the default stream has handle 0 on every device. */
int gh_set_stream_workspace(gh_stream_t stream, void* ptr, int64_t bytes);

/* ---- plain linear y = x W^T + b (model head, graph_based_semantic_structure.py:69-72) ---- */
int gh_linear_fwd(const float* x, const float* w, const float* bias, float* y, int m, int k, int n,
                  gh_stream_t stream);
/* dx = g W (NULL ok; wt = W^T [k][n]); dw += g^T x; db += colsum(g) (NULL ok).  w = W as stored (NULL ok): layers with
 * n <= 8 outputs (the 2-class head) then run as one row-per-wave kernel instead of three MFMA launches. */
int gh_linear_bwd(const float* x, const float* wt, const float* w, const float* g, int m, int k, int n,
                  float* dx, float* dw, float* db, gh_stream_t stream);

/* Weight gradient of a linear layer of the bf16 storage pipeline (gh_ggnn_cell_bwd_bf16's building block, exposed for callers'
 * own layers and for the exact parity test of the kernel): g16 [m][ldg] and x16 [m][ldx] hold bf16 (n resp. k columns used),
 *     dw[n][k] (fp32, leading dimension lddw) += g^T x,      db[n] (fp32, NULL ok) += colsum(g),
 * products exact, fp32 accumulation, a fixed summation order.  Needs the split-K workspace (gh_set_workspace), 16-byte aligned
 * operands with ldg % 8 == ldx % 8 == 0 and n % 8 == k % 8 == 0.  Outputs whose widths are multiples of 256 over >= 16 384 rows run
 * on the 256 x 256 x 64 ping-pong tile (gemm_tn_pp.hip.h), the rest on the 128 x 320 tile (gemm_tn.hip.h). */
int gh_linear_wgrad_bf16(const void* g16, int ldg, const void* x16, int ldx, int m, int n, int k,
                         float* dw, int lddw, float* db, gh_stream_t stream);

/* ---- graph encoders: Models/BiDAF/wrapper.py:7-67 GraphAttentionLayer, :70-112 GAT, :115-151 GCN ----
 * Padded layout only (no node-compact plan), r <= 256 nodes per graph, fp32.
 *
 * One GAT layer, all `heads` heads at once (wrapper.py:27-53 per head; :99-108 the stack):
 *   h   [n*r][heads*f]  = x [n*r][din] W_cat, one GEMM; W_cat = [W_0 | W_1 | ...] (each head's W is [din][f]), handed over
 *                         TRANSPOSED as w_lin [heads*f][din] (the nn.Linear layout gh_linear_fwd takes)
 *   a   [heads][2f]      each head's attention vector (the reference's a[2f][1])
 *   e_ij = LeakyReLU_alpha(h_i . a[:f] + h_j . a[f:]) on the edges, softmax over j; an edge is a refined bit (keep-set as
 *   in gh_spmm) whose value is > 0 when vals != NULL (the reference masks with adj > 0); a row without an edge is uniform,
 *   1/r over all r nodes (the reference's -9e15 fill).  drop_p > 0: dropout of the attention entries with the stateless
 *   mask of the cells, entry (head hd, graph g, i, j) kept iff hash(drop_seed, (((layer*heads + hd)*n + g)*r + i)*r + j)
 *   >= drop_p*2^32, scaled by 1/(1-drop_p).  hp [n*r][heads*f] = P h per head (saved).  mode 1 (hidden layer, concat=True):
 *   out [n*r][heads*f] = elu(hp); mode 2 (a lone concat=False layer): out = hp; mode 0 (the GAT's output layer,
 *   wrapper.py:108-110): out [n*r][f] = relu(sum_hd hp_hd / r).
 *   Saved for the backward: s [n*r][heads][2] the score halves, stats [n*r][heads][2] = (row max, 1 / row sum).
 *   Needs heads <= 8, f <= 1024. */
int gh_gat_layer_fwd(const uint64_t* bits, const float* vals, const uint64_t* keep, const float* x, const float* w_lin,
                     const float* a, int n, int r, int din, int heads, int f, float alpha, int mode, int layer,
                     float drop_p, uint32_t drop_seed, float* h, float* s, float* stats, float* hp, float* out,
                     gh_stream_t stream);
/* Backward of the layer: same arguments as the forward, its saved tensors, and g = dL/dout ([n*r][heads*f] or [n*r][f]).
 * w_cat [din][heads*f] (the W's side by side, as stored).  Scratch: dh [n*r][heads*f], da_part [n][heads][2f].
 * Outputs: dx [n*r][din] (NULL ok), and ACCUMULATED (+=) into dw_cat [din][heads*f] and da [heads][2f].
 * No global atomics: column sums of the edge softmax are reduced in LDS, da over the graphs in a fixed order. */
int gh_gat_layer_bwd(const uint64_t* bits, const float* vals, const uint64_t* keep, const float* x, const float* w_cat,
                     const float* a, int n, int r, int din, int heads, int f, float alpha, int mode, int layer,
                     float drop_p, uint32_t drop_seed, const float* h, const float* s, const float* stats,
                     const float* hp, const float* out, const float* g, float* dh, float* da_part, float* dx,
                     float* dw_cat, float* da, gh_stream_t stream);
/* GCN normalisation (wrapper.py:125-135): D^-1/2 A D^-1/2 with D the row sums of the adjacency VALUES over the refined
 * pattern, pow(-0.5) with inf -> 0, written as a per-row scale [n][r]:
 *   vals == NULL (normalised graph, value dinv_i dinv_j): scale_i = dinv_i (dinv_i sum_{j in N(i)} dinv_j)^-1/2, and
 *                 A_hat is again a normalised graph: gh_spmm with dinv = scale;
 *   vals != NULL: scale_i = (sum_j vals_ij)^-1/2 and A_hat x = scale . (gh_spmm on vals)(scale . x)  (gh_scale_rows). */
int gh_gcn_norm(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep, int n, int r,
                float* scale, gh_stream_t stream);
/* Feature dropout of the encoders (wrapper.py:101,105,141): y = x * mask / (1 - p), the cells' stateless mask over the
 * element index row*cols + col (in-place ok; the backward is the same call on the gradient). */
int gh_feat_dropout(const float* x, float* y, int rows, int cols, float p, uint32_t seed, gh_stream_t stream);
/* y[i][c] = x[i][c] * scale[i] (scale NULL: 1), zeroed where mask[i][c] <= 0 (mask NULL: none; mask == x is relu(x)). */
int gh_scale_rows(const float* x, const float* scale, const float* mask, float* y, int rows, int cols, gh_stream_t stream);

/* ---- single-query attention ablations: thirdparty/two_branches_attention.py Dot :9-38, BiLinear :41-70, BiLinearTanh
 *      :151-191; thirdparty/self_attention.py SelfAttentionICLR2017 :13-48, MultiHeadSelfAttentionICLR17OnWord :103-153 ----
 * Padded layout only, fp32, mask [b][l] float (0 = padded), one workgroup per sequence, no floating-point atomics (two
 * runs are bit-identical).  A sequence whose mask is all zero yields NaN weights and a NaN output row, as the reference's
 * softmax of all -inf does; other sequences are unaffected.  Widths that are multiples of 4 on 16-byte aligned operands
 * move 16 bytes per lane, every other shape takes a scalar path.
 *
 * Attention scored by a query vector (two_branches_attention.py:29-37 Dot; :62-69 BiLinear with q = W(left)):
 *   s_l = right[b][l] . q[b];  weights[b] = softmax over the unmasked l (running maximum subtracted), exactly 0 where
 *   masked;  avg[b] = sum_l weights[b][l] right[b][l].   Needs l <= 4096 and d <= 2048. */
int gh_query_att_fwd(const float* q, const float* right, const float* mask, int b, int l, int d,
                     float* weights /*[b][l]*/, float* avg /*[b][d]*/, gh_stream_t stream);
/* Backward of the above from g_avg [b][d] and g_w [b][l] (NULL ok): with dw_l = g_w_l + g_avg . right_l and
 * ds_l = w_l (dw_l - sum_j w_j dw_j):  dright_l = w_l g_avg + ds_l q,  dq = sum_l ds_l right_l.  Every row of dright is
 * written (exact zeros where the weight is 0); nothing is accumulated. */
int gh_query_att_bwd(const float* q, const float* right, const float* weights,
                     const float* g_avg, const float* g_w /*NULL ok*/, int b, int l, int d,
                     float* dq /*[b][d]*/, float* dright /*[b][l][d]*/, gh_stream_t stream);
/* Additive (tanh) attention over a separate value tensor (two_branches_attention.py:183-190 BiLinearTanh with
 * pre = left_linear(left_tsr), u = right_linear(right_tsr), w2 = combine.weight, values = left_tsr;
 * self_attention.py:143-150 MultiHeadSelfAttentionICLR17OnWord and :39-47 SelfAttentionICLR2017 with pre = linear1(tsr),
 * u = NULL, w2 = linear2.weight, values = original resp. tsr):
 *   t = tanh(pre[b][l] + u[b]) (saved; rows of padded positions are not written),  e[b][l][c] = w2[c] . t,
 *   weights = masked softmax over l per head,  attended[b][c] = sum_l weights[b][l][c] values[b][l].
 * Needs heads <= 8 and l * heads <= 8192 (l <= 1024 at eight heads); longer sequences are rejected. */
int gh_tanh_att_fwd(const float* pre /*[b][l][ha]*/, const float* u /*[b][ha] or NULL*/, const float* w2 /*[heads][ha]*/,
                    const float* mask, const float* values /*[b][l][dv]*/, int b, int l, int ha, int heads, int dv,
                    float* t /*saved tanh [b][l][ha]*/, float* weights /*[b][l][heads]*/, float* attended /*[b][heads][dv]*/,
                    gh_stream_t stream);
/* Backward from g_att [b][heads][dv] and g_w [b][l][heads] (NULL ok).  Out: dpre [b][l][ha] and dvalues [b][l][dv] (every
 * row written, exact zeros at padded positions), du [b][ha] = sum_l dpre (NULL when the forward had no u); dw2 [heads][ha]
 * is ACCUMULATED (+=) from per-sequence partials ([b][heads][ha] floats on the stream workspace, which must be registered:
 * gh_set_stream_workspace / gh_set_workspace) summed over the sequences in a fixed order. */
int gh_tanh_att_bwd(const float* t, const float* w2, const float* weights, const float* values,
                    const float* g_att, const float* g_w /*NULL ok*/, int b, int l, int ha, int heads, int dv,
                    float* dpre, float* du /*NULL when the forward had no u*/, float* dw2 /*ACCUMULATED*/, float* dvalues,
                    gh_stream_t stream);

/* ---- multi-head query/key/value attention: thirdparty/two_branches_attention.py ScaledDotProductAttention :391-422 as
 *      MultiHeadAttentionOriginal :271-347 calls it, and the residual LayerNorm of :345 ----
 * fp32, no floating-point atomics (two runs are bit-identical), nothing is allocated.
 *
 * Masked multi-head dot-product attention (:414-421; the reference divides by no temperature: softmax(q k^T)), replacing
 * the per-operand permute(2, 0, 1, 3).contiguous() copies of :334-336, the two bmm, the softmax and both masked_fill of
 * :414-421 and the permute copy of :340-341:
 *   q [b][lq][heads * dk], k [b][lk][heads * dk], v [b][lk][heads * dv], row r of batch i at (i * l + r) * ld, each with its
 *   own leading dimension (ld >= heads * width): head h is the column slice [h * width, (h + 1) * width), read in place
 *   from the projection GEMM's output.  mask [b][lq][lk] uint8, nonzero = masked, shared by all heads.
 *   weights [heads * b][lq][lk] (index h * b + i, the reference's order) is always written: softmax over the unmasked
 *   keys with the running maximum subtracted, exactly 0.0 at masked positions; a query row with every key masked has
 *   all-zero weights and an all-zero output row (never NaN).  out [b][lq][heads * dv] (leading dimension ldo) = weights v_h.
 * Limits: 1 <= heads <= 16, lq <= 1024, lk <= 1024, dk <= 512, dv <= 512, b * ceil(max(lq, lk) / 16) < 2^31; anything
 * beyond them is rejected with an error and nothing is written.  Rows that are 16-byte aligned (ld % 4 == 0, width % 4 ==
 * 0, aligned base) move 16 bytes per lane, every other shape takes single-float accesses. */
int gh_mha_sdpa_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv,
                    const uint8_t* mask, int b, int heads, int lq, int lk, int dk, int dv,
                    float* weights, float* out, int ldo, gh_stream_t stream);
/* Backward of the above (autograd of :414-421 and of the permutes around it) from g_out [b][lq][heads * dv] (ldgo) and
 * g_weights [heads * b][lq][lk] (NULL ok), with A the saved weights, per head:
 *   dA = g_weights + g_out_h v_h^T,  dS = A (dA - rowsum(A dA)),  dq_h = dS k_h,  dk_h = dS^T q_h,  dv_h = A^T g_out_h.
 * ds [heads * b][lq][lk] is scratch of the caller's (it receives dS).  Every element of dq, dk and dv (layouts of q, k, v
 * with their own leading dimensions) is written, nothing is accumulated; a fully masked query row sends exact zeros. */
int gh_mha_sdpa_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv,
                    const float* weights, const float* g_out, int ldgo, const float* g_weights /*NULL ok*/,
                    int b, int heads, int lq, int lk, int dk, int dv, float* ds /*scratch*/,
                    float* dq, int lddq, float* dk_out, int lddk, float* dv_out, int lddv, gh_stream_t stream);
/* y [rows][d] = LayerNorm(x + res) * gamma + beta over the last axis (:345 layer_norm(output + residual); :267 with
 * res = NULL), biased variance, eps inside the square root (nn.LayerNorm's default is 1e-5).  mean [rows] and
 * rstd [rows] are saved for the backward.  One wave per row; needs d <= 2048. */
int gh_add_layernorm_fwd(const float* x, const float* res /*NULL ok*/, const float* gamma, const float* beta, float eps,
                         int rows, int d, float* y, float* mean, float* rstd, gh_stream_t stream);
/* Backward from g [rows][d]: dx [rows][d] (also the gradient of res) is written; dgamma [d] and dbeta [d] are ACCUMULATED
 * (+=) from per-workgroup partials ([<= 256][2][d] floats on the stream workspace, which must be registered:
 * gh_set_stream_workspace / gh_set_workspace) summed by a second stage in workgroup order. */
int gh_add_layernorm_bwd(const float* x, const float* res /*NULL ok*/, const float* gamma, const float* mean,
                         const float* rstd, const float* g, int rows, int d, float* dx, float* dgamma /*ACCUMULATED*/,
                         float* dbeta /*ACCUMULATED*/, gh_stream_t stream);

/* ---- the LSTM sequence encoder's recurrence (get_amd/csrc/rnn_ops.hip): Models/BiDAF/wrapper.py:256-276 ----
 * What pack_padded_sequence + nn.LSTM + pad_packed_sequence + the two index gathers of :260-275 compute for ONE layer, both
 * directions in one launch, with torch.nn.LSTM's cell equations (gate order i, f, g, o; zero initial state):
 *   i, f, o = sigmoid(.), g = tanh(.) of gx[b][t] + h_{t-1} W_hh^T;  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
 * gx0 / gx1 [n][t_in][4h] (row pitch ldgx >= 4h): the input projection x W_ih^T + b_ih + b_hh of the forward / the reverse
 * direction (gx1, w_hh1: NULL when dirs == 1), a GEMM of the caller's.  w_hh [4h][h] as nn.LSTM stores it, 16-byte aligned.
 * lens [n] int32 on the device, clamped into [0, min(t_in, t_out)]; the reverse direction of sequence b walks t = len - 1 .. 0.
 * order [n] (NULL = identity): slot s of the launch processes row order[s] of every tensor -- a permutation sorted by length
 * gives the 16-sequence tiles similar lengths; an entry outside [0, n) is skipped.  Every tensor is indexed by the row b.
 * Out: y [n][t_out][ldy] columns [dir * h, (dir + 1) * h), exact zeros at t >= len; h_n, c_n [dirs][n][h] (the state after the
 * last step of the direction; zeros for an empty sequence -- where pack_padded_sequence raises).  gates [dirs][n][t_in][4h]
 * (post-activation), c [dirs][n][t_in][h] and h_prev [dirs][n][t_in][h] (the hidden state that ENTERED step t, zeros at t >= len)
 * are saved for the backward when all three are given (all NULL: inference).  Rows t >= len of gates and c are not written.
 * The sigmoid takes exp of non-positive arguments only: saturated pre-activations give exact 0 / 1, never NaN -- exactly 1 from
 * about +17 on, exactly 0 below ln(2^-126) = -87.34, where the value would be an fp32 denormal (every normal value is kept).
 * Limits: h <= 1024, t_in <= 4096, t_out <= 4096, dirs 1 or 2, any n; anything beyond is rejected and nothing is written. */
int gh_lstm_seq_fwd(const float* gx0, const float* gx1 /*NULL ok*/, int ldgx, const float* w_hh0, const float* w_hh1 /*NULL ok*/,
                    const int32_t* lens, const int32_t* order /*NULL ok*/, int n, int t_in, int t_out, int h, int dirs,
                    float* y, int ldy, float* gates /*NULL ok*/, float* c /*NULL ok*/, float* h_prev /*NULL ok*/,
                    float* h_n, float* c_n, gh_stream_t stream);
/* Backward of the above (autograd of torch.nn.LSTM's cell equations, wrapper.py:256-276) from g_y [n][t_out][ldgy] (NULL ok)
 * and g_hn [dirs][n][h] (NULL ok), walking time the other way:
 *   dh = g_y[t] + dh_rec (+ g_hn at the direction's last step);  dc += dh o (1 - tanh(c_t)^2);  di = dc g i (1 - i);
 *   df = dc c_{t-1} f (1 - f);  dg = dc i (1 - g^2);  do = dh tanh(c_t) o (1 - o);  dh_rec = dgates_t W_hh;  dc <- dc f
 * dgates [dirs][n][t_in][4h] is the gradient of gx: every element of every processed sequence is written, exact zeros at
 * t >= len (also in rows [t_out, t_in) when t_out < t_in).  The rows of a sequence that `order` skips (an entry outside [0, n)
 * where its row would have stood) are NOT written, as in the forward.  The caller forms dW_hh = dgates^T h_prev per direction
 * with gh_linear_bwd (dx = NULL, x = h_prev, g = dgates).  Same limits as the forward. */
int gh_lstm_seq_bwd(const float* w_hh0, const float* w_hh1 /*NULL ok*/, const int32_t* lens, const int32_t* order /*NULL ok*/,
                    int n, int t_in, int t_out, int h, int dirs, const float* g_y /*NULL ok*/, int ldgy,
                    const float* g_hn /*NULL ok*/, const float* gates, const float* c, float* dgates, gh_stream_t stream);

/* ---- the GRU sequence encoder's recurrence (get_amd/csrc/rnn_ops.hip): Models/BiDAF/wrapper.py:306-327 ----
 * What pack_padded_sequence + nn.GRU + pad_packed_sequence + the two index gathers of :310-326 compute for ONE layer, both
 * directions in one launch, with torch.nn.GRU's cell equations (gate order r, z, n; zero initial state):
 *   a = h_{t-1} W_hh^T + b_hh;  r = sigmoid(gx_r + a_r);  z = sigmoid(gx_z + a_z);  n = tanh(gx_n + r a_n);
 *   h_t = (1 - z) n + z h_{t-1}
 * gx0 / gx1 [n][t_in][3h] (row pitch ldgx >= 3h): the input projection x W_ih^T + b_ih ALONE of the forward / the reverse
 * direction (gx1, w_hh1, b_hh1: NULL when dirs == 1), a GEMM of the caller's.  b_hh cannot be folded into gx as for the LSTM:
 * its n third is multiplied by r.  w_hh [3h][h] as nn.GRU stores it, 16-byte aligned; b_hh0 / b_hh1 [3h] DEVICE pointers.
 * lens, order, the clamping, the row addressing and the reverse direction's walk are those of gh_lstm_seq_fwd.
 * Out: y [n][t_out][ldy] columns [dir * h, (dir + 1) * h), exact zeros at t >= len (also in rows [t_in, t_out)); h_n [dirs][n][h]
 * (the state after the last step of the direction; zeros for an empty sequence).  Saved for the backward when all three are
 * given (all NULL: inference): gates [dirs][n][t_in][3h] (post-activation r, z, n), an [dirs][n][t_in][h] (a_n, b_hn included)
 * and h_prev [dirs][n][t_in][h] (the hidden state that ENTERED step t, zeros at t >= len).  Rows t >= len of gates and an are
 * not written.  The sigmoid is the LSTM's: saturated pre-activations give exact 0 / 1 (1 from about +17 on, 0 below -87.34), never NaN.
 * Limits: h <= 1024, t_in <= 4096, t_out <= 4096, dirs 1 or 2, any n; anything beyond is rejected and nothing is written. */
int gh_gru_seq_fwd(const float* gx0, const float* gx1 /*NULL ok*/, int ldgx, const float* w_hh0, const float* w_hh1 /*NULL ok*/,
                   const float* b_hh0, const float* b_hh1 /*NULL ok*/, const int32_t* lens, const int32_t* order /*NULL ok*/,
                   int n, int t_in, int t_out, int h, int dirs, float* y, int ldy, float* gates /*NULL ok*/,
                   float* an /*NULL ok*/, float* h_prev /*NULL ok*/, float* h_n, gh_stream_t stream);
/* Backward of the above (autograd of torch.nn.GRU's cell equations) from g_y [n][t_out][ldgy] (NULL ok) and g_hn [dirs][n][h]
 * (NULL ok), walking time the other way.  With dh = g_y[t] + dh_carry (+ g_hn at the direction's last step):
 *   dn_pre = dh (1 - z) (1 - n^2);  dz_pre = dh (h_prev - n) z (1 - z);  dr_pre = dn_pre a_n r (1 - r);  da_n = dn_pre r;
 *   dh_carry = dh z + [dr_pre, dz_pre, da_n] W_hh
 * Two outputs, each [dirs][n][t_in][3h], every element of every processed sequence written, exact zeros at t >= len (the rows
 * of a sequence that `order` skips are NOT written, as in the forward):
 *   dgx = [dr_pre, dz_pre, dn_pre]   the gradient of gx (db_ih, dW_ih and dx follow from the input projection's backward)
 *   da  = [dr_pre, dz_pre, da_n]     the gradient of the recurrent pre-activations a
 * The caller forms dW_hh = da^T h_prev AND db_hh = colsum(da) per direction with ONE gh_linear_bwd (dx = NULL, x = h_prev,
 * g = da, dw, db).  No atomics: every element has one owner, two runs are bit-identical.  Same limits as the forward. */
int gh_gru_seq_bwd(const float* w_hh0, const float* w_hh1 /*NULL ok*/, const int32_t* lens, const int32_t* order /*NULL ok*/,
                   int n, int t_in, int t_out, int h, int dirs, const float* g_y /*NULL ok*/, int ldgy,
                   const float* g_hn /*NULL ok*/, const float* gates, const float* an, const float* h_prev, float* dgx,
                   float* da, gh_stream_t stream);

/* ---- the BiDAF model's own layers (get_amd/csrc/bidaf_ops.hip): Models/BiDAF/bidaf_model.py ----
 * The attention-flow layer, replacing :72-104: the q_len calls of the 1-wide att_weight_cq over c * q_i and their stack
 * (:75-83), the two expand adds (:87-89), both softmaxes (:92, :96), both bmm (:94, :98), the tiled expand (:100) and the
 * four-way cat (:104).
 *   c [b][lc][d] (row r of batch i at (i * lc + r) * ldc), q [b][lq][d] (ldq): read in place, e.g. column slices.
 *   w_c, w_q, w_cq [d]: the weights of the three Linear(d, 1); b_c, b_q, b_cq: their 1-element biases as DEVICE pointers.
 *   s[i][j] = c_i.w_c + q_j.w_q + (c_i * w_cq).q_j + (b_c + b_q + b_cq)
 *   a = softmax_j(s) (running maximum subtracted), c2q_i = sum_j a_ij q_j
 *   m_i = max_j s_ij, amax_i = the LOWEST j attaining it (torch.max's documented rule)
 *   beta = softmax_i(m) over ALL lc rows of the batch element, q2c = sum_i beta_i c_i
 *   x [b][lc][4d] (ldx >= 4d) = [c_i, c2q_i, c_i * c2q_i, c_i * q2c]
 * THERE IS NO MASK, as in the reference: c and q are LSTM outputs with exact-zero rows at t >= len, and those rows take part
 * in both softmaxes (a zero row of q scores c_i.w_c + bias, a zero row of c scores q_j.w_q + bias).
 * Saved for the backward: a [b][lc][lq], amax [b][lc] int32, beta [b][lc], q2c [b][d]; m [b][lc] is scratch (the row maxima
 * between the two launches).  c2q is re-read from x.
 * Limits: lc <= 1024, lq <= 1024, d <= 2048, any b with b * ceil(max(lc, lq) / 16) < 2^31; anything beyond them is rejected
 * with an error and nothing is written.  Rows that are 16-byte aligned (ld % 4 == 0, aligned base) move 16 bytes per lane,
 * every other shape takes single-float accesses.  No atomics: two runs are bit-identical. */
int gh_att_flow_fwd(const float* c, const float* q, int ldc, int ldq, const float* w_c, const float* w_q, const float* w_cq,
                    const float* b_c, const float* b_q, const float* b_cq, int b, int lc, int lq, int d, float* x, int ldx,
                    float* a, int32_t* amax, float* m /*scratch*/, float* beta, float* q2c, gh_stream_t stream);
/* Backward of the above (autograd of :72-104) from g_x [b][lc][4d] (ldg), slices g0 .. g3:
 *   dc2q = g1 + g2 * c;  dq2c = sum_i g3_i * c_i;  dbeta_i = dq2c.c_i;  dm_i = beta_i (dbeta_i - sum_k beta_k dbeta_k)
 *   dA_ij = dc2q_i.q_j;  dS_ij = a_ij (dA_ij - sum_j a_ij dA_ij) + dm_i [j = amax_i]
 *   dc_i = g0 + g2 * c2q + g3 * q2c + beta_i dq2c + dm_i w_c + w_cq * sum_j dS_ij q_j
 *   dq_j = sum_i a_ij dc2q_i + (sum_i dS_ij) w_q + w_cq * sum_i dS_ij c_i
 * ds [b][lc][lq], dm [b][lc] and dq2c [b][d] are scratch of the caller's.  Every element of dc (lddc) and dq (lddq) is
 * written, nothing is accumulated there.  dw_c, dw_q, dw_cq [d] are ACCUMULATED (+=) from per-batch-element (dw_c) and
 * per-(batch element, 16 query rows) partials, b * d * (1 + 2 ceil(lq / 16)) floats on the stream workspace, which must be
 * registered (gh_set_stream_workspace / gh_set_workspace), summed by a second stage in a fixed order.
 * The gradients of the three biases are mathematically zero (sum_j dS_ij = dm_i and sum_i dm_i = 0) and are not computed.
 * Same limits as the forward. */
int gh_att_flow_bwd(const float* c, const float* q, int ldc, int ldq, const float* w_c, const float* w_q, const float* w_cq,
                    const float* x, int ldx, const float* a, const int32_t* amax, const float* beta, const float* q2c,
                    const float* g_x, int ldg, int b, int lc, int lq, int d, float* ds /*scratch*/, float* dm /*scratch*/,
                    float* dq2c /*scratch*/, float* dc, int lddc, float* dq, int lddq, float* dw_c /*ACCUMULATED*/,
                    float* dw_q /*ACCUMULATED*/, float* dw_cq /*ACCUMULATED*/, gh_stream_t stream);
/* The gate of the highway network (:62, with the ReLU and Sigmoid of the nn.Sequential holders :22-24 folded in), elementwise
 * over [rows][d] contiguous tensors:  y = sigmoid(g_pre) relu(h_pre) + (1 - sigmoid(g_pre)) x.  h_pre and g_pre are the two
 * projections of the layer (GEMMs of the caller's).  The sigmoid takes exp of non-positive arguments only: saturated
 * pre-activations give exact 0 / 1 gates, never NaN. */
int gh_highway_fwd(const float* x, const float* h_pre, const float* g_pre, int rows, int d, float* y, gh_stream_t stream);
/* Backward from g [rows][d] in one launch: dh_pre = g s [h_pre > 0], dg_pre = g (relu(h_pre) - x) s (1 - s) and the direct
 * dx = g (1 - s), s = sigmoid(g_pre); every element of the three is written. */
int gh_highway_bwd(const float* x, const float* h_pre, const float* g_pre, const float* g, int rows, int d, float* dh_pre,
                   float* dg_pre, float* dx, gh_stream_t stream);

/* ---- the matchzoo/modules family (get_amd/csrc/match_ops.hip) ----
 * Soft alignment between two sequences, replacing matchzoo/modules/attention.py:50-63 (BidirectionalAttention: the bmm, both
 * masked_fill + softmax, both bmm and both masked_fill_) and :99-105 (MatchModule: the bmm, masked_fill, softmax, bmm and the
 * four-way cat).
 *   q [b][lq][d] (ldq), k [b][lk][d] (ldk), v [b][lk][dv] (ldv): read in place, e.g. column slices.
 *   key_fill [b][lk] uint8, nonzero = filled; row_zero [b][lq] uint8 or NULL; fill finite (a non-finite one is rejected).
 *   S_ij = q_i.k_j, then S_ij = fill where key_fill_j: the score is REPLACED by the constant and KEEPS its weight -- the
 *   reference's masked_fill(mask, -1e-7) as written, not an exclusion.  A = softmax_j(S) (running maximum subtracted),
 *   a [b][lq][lk] is always written; a sequence whose keys are all filled gets uniform weights 1 / lk, never NaN.
 *   o_i = sum_j A_ij v_j, then o_i = 0 where row_zero_i.
 *   fuse == 0: out [b][lq][dv] (ldo) = o.   fuse == 1 (needs dv == d, row_zero == NULL): out [b][lq][4d] = [q, o, q - o, q * o].
 * Limits: lq, lk <= 1024, d, dv <= 2048, b * ceil(max(lq, lk) / 16) < 2^31; anything beyond them is rejected with an error and
 * nothing is written.  Nothing is allocated.  No atomics: two runs are bit-identical. */
int gh_soft_align_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const uint8_t* key_fill,
                      const uint8_t* row_zero /*NULL ok*/, float fill, int fuse, int b, int lq, int lk, int d, int dv, float* a,
                      float* out, int ldo, gh_stream_t stream);
/* Backward of the above from g (ldg; [b][lq][dv], or [b][lq][4d] with slices g0 .. g3 when fuse):
 *   g_o = g, or g1 - g2 + g3 * q with fuse; g_o = 0 in the rows of row_zero
 *   dv_j = sum_i A_ij g_o,i (filled keys DO receive it);  dA_ij = g_o,i.v_j;  dS = A (dA - sum_j A dA), then dS_ij = 0 where
 *   key_fill_j (the fill is a constant);  dq_i = sum_j dS_ij k_j (+ g0 + g2 + g3 * o with fuse, o re-read from out);
 *   dk_j = sum_i dS_ij q_i.
 * ds [b][lq][lk] is scratch of the caller's; out is only read with fuse.  Every element of dq, dk and dvv is written. */
int gh_soft_align_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const uint8_t* key_fill,
                      const uint8_t* row_zero /*NULL ok*/, int fuse, const float* a, const float* out /*fuse only*/, int ldo,
                      const float* g, int ldg, int b, int lq, int lk, int d, int dv, float* ds /*scratch*/, float* dq, int lddq,
                      float* dk, int lddk, float* dvv, int lddv, gh_stream_t stream);
/* matchzoo/modules/attention.py:35-38 (Attention): s_l = x_l.w (x [b][l][d] contiguous, w [d], no bias), position l is excluded
 * according to mode -- the reference's mask = (x != m); masked_fill(mask == m, -inf) read literally: mode 0 (m == 0) excludes
 * s_l == 0, mode 1 (m == 1) excludes s_l != 1, mode 2 (any other m) excludes nothing -- and a [b][l] = the softmax over the
 * kept positions, exactly 0 at the excluded ones.  A sequence without a kept position is NaN in its own row, as in the
 * reference.  s_l is formed from products only, so an all-zero row scores exactly 0.  Limits: l <= 4096, d <= 2048. */
int gh_lin_att_fwd(const float* x, const float* w, int mode, int b, int l, int d, float* a, gh_stream_t stream);
/* Backward from g [b][l]: ds_l = a_l (g_l - sum_l a_l g_l), dx_l = ds_l w, dw = sum over the sequences of sum_l ds_l x_l:
 * part [b][d] (scratch of the caller's) holds the per-sequence sums, added in sequence order into dw (written, not +=). */
int gh_lin_att_bwd(const float* x, const float* w, const float* a, const float* g, int b, int l, int d, float* dx,
                   float* part /*scratch*/, float* dw, gh_stream_t stream);
/* matchzoo/modules/matching.py:46-50: out [b][l][r] = x_l.y_r (x [b][l][d] ldx, y [b][r][d] ldy); with normalize times
 * ix_l iy_r, i = 1 / max(||row||_2, 1e-12) (F.normalize), ix [b][l] and iy [b][r] written and saved.
 * Limits: l, r <= 1024, d <= 2048. */
int gh_match_dot_fwd(const float* x, const float* y, int ldx, int ldy, int normalize, int b, int l, int r, int d,
                     float* ix /*normalize only*/, float* iy /*normalize only*/, float* out, gh_stream_t stream);
/* Backward from g [b][l][r]: gs = g * ix * iy, dx_raw = gs y, dy_raw = gs^T x (dx [b][l][d], dy [b][r][d] contiguous).  With
 * normalize a row above the clamp gets dx = dx_raw - x (x.dx_raw) ix^2; a row with ||x|| <= 1e-12 keeps dx_raw (the gradient of
 * clamp_min is zero there), which is of the order 1e12 g, exactly as torch gives. */
int gh_match_dot_bwd(const float* x, const float* y, int ldx, int ldy, int normalize, const float* ix, const float* iy,
                     const float* g, int b, int l, int r, int d, float* dx, float* dy, gh_stream_t stream);
/* matchzoo/modules/matching.py:52-61: out [b][l][r][d] = x_l op y_r for op 0 mul, 1 plus, 2 minus; op 3 concat writes
 * [b][l][r][2d] = [x_l, y_r].  Written once from x [b][l][d] and y [b][r][d] (contiguous), without the reference's two repeat
 * copies.  64-bit offsets.  Limit: d <= 2048. */
int gh_match_bcast_fwd(const float* x, const float* y, int op, int b, int l, int r, int d, float* out, gh_stream_t stream);
/* Backward: dx_l = sum_r (g * y | g | g | g[:d]), dy_r = sum_l (g * x | g | -g | g[d:]); one owner per output element and a
 * fixed summation order. */
int gh_match_bcast_bwd(const float* x, const float* y, const float* g, int op, int b, int l, int r, int d, float* dx,
                       float* dy, gh_stream_t stream);
/* matchzoo/modules/gaussian_kernel.py:34-36: y = exp(-0.5 (x - mu)^2 / sigma^2) over n elements (y == x is fine);
 * sigma == 0 is rejected. */
int gh_gauss_kernel_fwd(const float* x, float mu, float sigma, long long n, float* y, gh_stream_t stream);
/* dx = -g y (x - mu) / sigma^2 from the saved y. */
int gh_gauss_kernel_bwd(const float* x, const float* y, const float* g, float mu, float sigma, long long n, float* dx,
                        gh_stream_t stream);

/* ---- a8  ragged helpers: Models/FCWithEvidences/basic_fc_model.py:80-121 ----
 * offsets[b+1] int32 prefix sum of evidence counts (device). */
/* has[b] (NULL ok) = 1.0 for claims with at least one evidence: row 0 of pad_right(x) is x's first row of the claim times has. */
int gh_seg_offsets(const int64_t* counts, int b, int32_t* offsets, int32_t* pair2claim, int b1, float* has,
                   gh_stream_t stream);
int gh_seg_broadcast(const float* src, const int32_t* pair2claim, float* dst, int b1, int x, gh_stream_t stream);
int gh_seg_sum(const float* src, const int32_t* offsets, float* dst, int b, int x, gh_stream_t stream);
int gh_seg_pad(const float* src, const int32_t* offsets, float* dst, int b, int n_max, int x, int dst_ld,
               gh_stream_t stream);
int gh_seg_unpad(const float* src, const int32_t* offsets, float* dst, int b, int n_max, int x, int src_ld,
                 gh_stream_t stream);
/* ---- evidence-level assembly: graph_based_semantic_structure.py:157-170,195-215 in one launch ----
 * right[b][slot][0:xa] = avg row of the claim's slot-th evidence (zeros beyond its count); right[b][slot][xa:xa+ds] =
 * table[max(sources[b][slot], 0)] (article-source embedding, -1 padding -> row 0; ds = 0: no table);
 * mask[b][slot] = (sum_r document[b][slot][r] >= 1).  sources/document are int32 or int64 (flag).
 * table_rows (ABI 9): rows of `table`; ids are clamped into [0, table_rows) -- nn.Embedding raises for an id beyond the table
 * (graph_based_semantic_structure.py:169), a device kernel cannot, so the event is COUNTED instead (gh_clamp_events). */
int gh_evd_assemble_fwd(const float* avg, const int32_t* offsets, const float* table, int table_rows, const void* sources, int sources_i64,
                        const void* document, int document_i64, int b, int n_max, int xa, int ds, int r,
                        float* right, float* mask, gh_stream_t stream);
/* Backward: d_avg[b1][xa] (NULL ok) = unpad(g[:, :, :xa]); d_table[s][ds] += the g[:, :, xa:] rows of the slots with source s,
 * summed in slot order (deterministic).  g [b][n_max][xa+ds] -- ds is g's row pitch as well: pass the real width even
 * when d_table is NULL (a frozen table just skips the table part).  At most 38 000 slots (b * n_max) per call.
 * EVERY row of d_avg is written (rows of a claim's evidences beyond its n_max-th receive zeros): the caller need not clear it. */
int gh_evd_assemble_bwd(const float* g, const int32_t* offsets, const void* sources, int sources_i64, int table_rows, int b, int n_max,
                        int xa, int ds, float* d_avg, float* d_table, gh_stream_t stream);
/* Out-of-range inputs the kernels clamped for memory safety where the reference would have RAISED (nn.Embedding /
 * nn.CrossEntropyLoss index errors): out_host[0] = labels outside [0, c) seen by gh_cross_entropy, [1] = claim-source ids,
 * [2] = article-source ids outside their table (other than the -1 padding id), [3] = ids outside [0, vocab) among the rows handed
 * to gh_embed_bwd (they contribute nothing there; the padding id is not counted) and among the word, position and token-type
 * ids of gh_bert_embed_fwd; counted on the CURRENT device since
 * the last reset.  Synchronises the device.  A training loop checks it once per epoch (or per step in debug runs): a non-zero
 * count means corrupt input data was trained on as if it were class / row 0 or the last one. */
int gh_clamp_events(int64_t* out4_host, int reset);
/* The same counters with the slots added since: out_host[0 .. n), 1 <= n <= GH_CLAMP_SLOTS.  [4] = labels outside [0, c) other than
 * the ignore index seen by gh_softmax_xent_fwd (the row is dropped from the loss).  Either call's reset clears every slot. */
#define GH_CLAMP_SLOTS 5
int gh_clamp_events_n(int64_t* out_host, int n, int reset);
/* masked mean over claim nodes (graph_based_semantic_structure.py:153): dst[b][h] = sum_l hid*mask / len */
int gh_masked_mean_fwd(const float* hid, const int32_t* ids, const float* lens, float* dst, int b, int l, int h,
                       gh_stream_t stream);
int gh_masked_mean_bwd(const float* g, const int32_t* ids, const float* lens, float* dhid, int b, int l, int h,
                       gh_stream_t stream);

/* ---- optimiser: torch.optim.Adam(weight_decay) semantics of Fitting/FittingFC/declare_fitter.py:58-61
 *      on one flat fp32 bucket (the same bucket the RCCL gradient all-reduce uses) ---- */
int gh_adam_step(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float grad_scale, gh_stream_t stream);

/* ---- the BERT fine-tuning optimiser on the same flat bucket (csrc/optim_ops.hip): pytorch_transformers/optimization.py ----
 * Global gradient norm, replacing the per-parameter norms, their stack and the host read of torch's clip_grad_norm_ that every
 * BERT recipe runs before optimization.py:130 AdamW.step:
 *     norm_out[0] = grad_scale * sqrt(sum_{i < count} g[i]^2)            (device memory; the host never reads it)
 * No floating-point atomics and a fixed order, so two calls on the same gradient give the same bits on any device:
 *   1. g is cut into chunks of GH_NORM_CHUNK elements, one partial each: gh_flat_grad_norm_partials (host only, no device
 *      call) says how many doubles `partials` must hold for `count`;
 *   2. in a chunk, lane t of 256 adds the squares of elements 4 t .. 4 t + 3, then of 1024 + 4 t .., in fp32 (one rounding per
 *      product and per sum); the 256 lane sums are combined in double: per 64 lanes a butterfly (xor 32, 16, .. 1), then the
 *      four sums in order;
 *   3. the partials are summed in double in index order in 256 contiguous runs of ceil(n / 256), the runs' sums in run order;
 *      root and scale in double, rounded once to fp32.
 * Two launches (one when count == 0, which writes 0).  g 16-byte aligned; count need not be a multiple of 4. */
#define GH_NORM_CHUNK 32768
int gh_flat_grad_norm_partials(int64_t count, int64_t* out_host);
int gh_flat_grad_norm(const float* g, int64_t count, float grad_scale, double* partials, int64_t n_partials, float* norm_out,
                      gh_stream_t stream);
/* AdamW.step, optimization.py:159-187, for the whole bucket in ONE launch, in place on p, m, v (g is only read), with the
 * hyperparameters of optimization.py:141 `group` per parameter.  The bucket is cut into blocks of GH_ADAMW_BLOCK elements (every
 * parameter slot of the bucket starts on one); block_seg[count / 64] names each block's entry of seg_table[n_seg], which the
 * host fills in double and rounds once: step_size = lr, or lr * sqrt(1 - beta2^t) / (1 - beta1^t) with bias correction (:170-174),
 * lr_wd = lr * weight_decay (:187), one_minus_beta = 1 - beta.  Per element, every operation rounded once to fp32, no FMA:
 *     gr = (g * grad_scale) * clip
 *     m  = beta1 * m + one_minus_beta1 * gr                              (:166)
 *     v  = beta2 * v + (one_minus_beta2 * gr) * gr                       (:167)
 *     p1 = p - (step_size * m) / (sqrt(v) + eps)                         (:168, :176: eps outside the bias correction)
 *     p  = p1 - lr_wd * p1   when lr_wd > 0, else p1                     (:186-187)
 * clip: norm NULL -> 1; else n = norm[0], read on the device (what gh_flat_grad_norm wrote: no host synchronisation):
 * n <= max_norm -> exactly 1, so that step equals the unclipped one bit for bit; else min(1, max_norm / (n + 1e-6)), the
 * coefficient of clip_grad_norm_.  The gradient itself is not rescaled in memory.
 * A block whose entry has skip != 0, or whose id is >= n_seg (checked in the kernel: a bad map cannot read outside the table),
 * is neither read nor written: padding between slots, and parameters without a gradient this step (:143-144).
 * Refused before any launch: count not a multiple of 64, p / g / m / v / seg_table not 16-byte aligned, n_seg beyond
 * GH_ADAMW_MAX_SEGMENTS (what the 16-bit ids can name), a norm with max_norm <= 0. */
#define GH_ADAMW_BLOCK 64
#define GH_ADAMW_MAX_SEGMENTS 65535
typedef struct {
  float step_size, lr_wd, beta1, beta2, eps, one_minus_beta1, one_minus_beta2;
  int32_t skip;
} gh_adamw_seg;
int gh_adamw_step(float* p, const float* g, float* m, float* v, int64_t count, const uint16_t* block_seg,
                  const gh_adamw_seg* seg_table, int n_seg, float grad_scale, const float* norm, float max_norm,
                  gh_stream_t stream);

/* ---- (e) the path's one exchange step: all-reduce(sum) of the flat fp32 gradient bucket over RCCL / xGMI with a
 *      communicator this library owns (SURVEY 8(b) `flat_allreduce`).  The reference has no distributed code -- its
 *      optimiser is single-process (Fitting/FittingFC/declare_fitter.py:58-61) -- so these calls mirror no reference
 *      interface; they exist so that a non-Python host can run data-parallel steps without
 *      torch.distributed:   rank 0: gh_comm_unique_id -> ship the 128 bytes to every rank by any channel ->
 *      every rank: hipSetDevice, gh_comm_init -> per step: gh_get_backward ..., gh_flat_allreduce(bucket),
 *      gh_adam_step(..., grad_scale = 1 / world).  librccl is dlopen'ed on first use (a copy the process already holds,
 *      e.g. torch's, is reused; $GET_AMD_RCCL overrides the search); nothing else in the library depends on it.
 *      Collectives are enqueued on `stream` and are in place; buffers are device pointers. ---- */
int gh_comm_unique_id(void* id128);                                  /* out: 128 bytes (ncclUniqueId) */
int gh_comm_init(const void* id128, int rank, int world, void** comm);   /* binds to the calling thread's current device */
int gh_comm_destroy(void* comm);
int gh_comm_info(void* comm, int* rank, int* world);                 /* either output may be NULL */
const char* gh_comm_library(void);                                   /* the librccl that was loaded; NULL + gh_last_error() if none */
int gh_flat_allreduce(void* comm, float* buf, int64_t count, gh_stream_t stream);
int gh_flat_broadcast(void* comm, float* buf, int64_t count, int root, gh_stream_t stream);

/* ==== a7  the whole model in two calls: Graph_basedSemantiStructure.forward (graph_based_semantic_structure.py:76-125) ====
 * gh_get_forward / gh_get_backward chain every kernel of the path -- claim cell + masked mean (:144-155), evidence cells
 * with the GSL refinement (:107; wrapper.py:165-172), word-level attention (:173-193), evidence-level assembly and
 * attention (:157-171, :195-221), head (:251-267, :69-74) -- on caller-provided buffers, so that a training step costs
 * the host two library calls instead of ~120 (the per-module entry points above remain the building blocks and the
 * API for callers that use the modules one by one).  Everything is fp32 unless model->storage asks for the bf16 storage
 * pipeline inside the evidence cells; widths: d % 4 == 0, h % 4 == 0, 4 <= d <= h <= 1024 (h > 320: the GSL scorer's projection
 * runs inside gh_scorer_gsl instead of the first cell's last epilogue); the word-embedding table is frozen (as
 * master_get.py:143 constructs it); the claim branch runs on `side_stream` (may equal `stream`) underneath the evidence
 * cells.  Pointers are device pointers; the structs themselves live on the host. */
typedef struct gh_cell_params {            /* one GGNN cell, Models/BiDAF/wrapper.py:177-183 */
  const float *w_p, *w_z0, *w_z1, *w_r0, *w_r1, *w_h0, *w_h1;          /* linear.weight as stored: w_p[h][din], others [h][h] */
  const float *b_z0, *b_z1, *b_r0, *b_r1, *b_h0, *b_h1;
  const float *wt_p, *wt_z0, *wt_z1, *wt_r0, *wt_r1, *wt_h0, *wt_h1;   /* transposes (gh_transpose_batch); backward only */
  float *dw_p, *dw_z0, *dw_z1, *dw_r0, *dw_r1, *dw_h0, *dw_h1;          /* gradients, ACCUMULATED (+=); backward only */
  float *db_z0, *db_z1, *db_r0, *db_r1, *db_h0, *db_h1;
} gh_cell_params;
typedef struct gh_cell_bf16 {              /* bf16 twins of one cell's matrices (bf16 storage mode; gh_weights_refresh makes them) */
  const void *w_p, *w_z0, *w_z1, *w_r0, *w_r1, *w_h0, *w_h1;            /* bf16 [h][din] / [h][h] */
  const void *wt_p, *wt_z0, *wt_z1, *wt_r0, *wt_r1, *wt_h0, *wt_h1;     /* bf16 transposes; backward only */
} gh_cell_bf16;
typedef struct gh_att_params {             /* ConcatNotEqualSelfAtt, thirdparty/two_branches_attention.py:112-148 */
  const float *w1, *w2, *w1t;              /* linear1.weight [ha][xl+dr], linear2.weight [heads][ha], linear1.weight^T */
  float *dw1, *dw2;                        /* ACCUMULATED */
} gh_att_params;
typedef struct gh_get_model {
  int d, h, word_heads, evd_heads, n_classes;       /* embedding width, hidden size, heads, output_size */
  int claim_src_dim, article_src_dim;               /* 0 = that source embedding is not used */
  int claim_src_rows, article_src_rows;             /* rows of the two source tables: claim-source ids are clamped into
                                                       [0, rows) (nn.Embedding raises there; a device kernel cannot) */
  const float* embedding;                           /* [vocab][d] word table (frozen) */
  gh_cell_params claim, cell1, cell2;               /* ggnn4claim_1, ggnn_with_gsl.feat_prop1 / feat_prop2 */
  const float* scorer_w;                            /* ggnn_with_gsl.word_scorer1.proj weight [h] */
  const float* scorer_gate;                         /* its six 1x1 linears packed as gh_scorer_gsl's gate[12] */
  gh_att_params att_word, att_evd;                  /* self_att_word, self_att_evd */
  const float *claim_src_table, *article_src_table; /* [.][claim_src_dim], [.][article_src_dim] or NULL */
  float *d_claim_src_table, *d_article_src_table;   /* ACCUMULATED; NULL = no gradient wanted */
  const float *out0_w, *out0_b, *out0_wt;           /* head: out.0 weight [h][e] (+ transpose [e][h]), bias */
  const float *out1_w, *out1_b, *out1_wt;           /* out.1 weight [n_classes][h] (+ transpose), bias */
  float *d_out0_w, *d_out0_b, *d_out1_w, *d_out1_b; /* ACCUMULATED */
  /* ABI 9 -- BASELINE configs[4]: storage = 1 runs the two EVIDENCE cells in the bf16 storage pipeline of
   * gh_ggnn_cell_fwd_bf16 / gh_ggnn_cell_bwd_bf16 (activations and weights bf16 in HBM, fp32 accumulation, fp32 cell outputs)
   * whenever d % 8 == 0, h % 8 == 0 and the batch has >= 8192 real node rows; everything else stays fp32.  0 = fp32 throughout. */
  int storage;
  const void* embedding16;                          /* bf16 copy of the word table (storage 1) */
  gh_cell_bf16 cell1_16, cell2_16;                  /* bf16 twins of cell1 / cell2 (storage 1) */
  const void *att_word_w1_16, *att_word_w1t_16;     /* bf16 twins of self_att_word.linear1.weight and of its transpose (storage 1; NULL ok:
                                                       the word attention's projections then round fp32 fragments in registers instead) */
} gh_get_model;
typedef struct gh_get_batch {
  int b, b1, l, r, n_max;                           /* claims, pairs, claim length, evidence length, evidence slots per claim */
  int m_real;                                       /* node-compact layout: total real evidence nodes (needs goff..maskf); < 0: padded layout */
  int collapsed;                                    /* node-compact evaluation: the first cell runs on m_real + 1 rows (gh_scorer_gsl pads_collapsed) */
  int k_keep;                                       /* GSL: int(rate * r) */
  const int32_t* q_ids;                             /* [b][l] claim node ids (int32) */
  const void* q_lens; int q_lens_kind;              /* [b] unique claim nodes; kind 0 = float32, 1 = int32, 2 = int64 */
  const uint64_t* q_bits; const float* q_dinv; const float* q_vals;      /* claim graphs (packed adjacency, see top) */
  const int32_t* d_ids;                             /* [b1][r] evidence node ids (padded indexing) */
  const uint64_t* d_bits; const float* d_dinv; const float* d_vals;      /* evidence graphs */
  const int32_t *goff, *rowg, *cids; const float* maskf;                 /* gh_ragged_plan outputs, or all NULL (padded layout) */
  const int64_t* counts;                            /* [b] evidences per claim (sum = b1) */
  int counts_fit;                                   /* (ignored since ABI 8: the backward always zero-fills d_avg) */
  const void* doc_sources; int doc_sources_i64;     /* [b][n_max], -1 = padding slot (article source ids) */
  const void* query_sources; int query_sources_i64; /* [b] claim source ids (claim_src_dim > 0) */
  const void* document; int document_i64;           /* [b][n_max][r] padded evidence node ids (slot mask only) */
  float drop_claim, drop_gnn;                       /* input dropout of the claim cell / of the three evidence-side cells (0 = eval) */
  uint32_t seed_claim, seed_cell1, seed_scorer, seed_cell2;
} gh_get_batch;
/* Buffer plan for (model, batch).  fwd_floats / bwd_floats = sizes (in floats) of the two activation arenas;
 * obs_floats = size of the OBSERVABLES buffer -- a few MB holding what a caller keeps after the step (ABI 7: a buffer of
 * its own, so that holding the logits / attention weights / keep-sets does not pin the multi-GB forward arena). */
typedef struct gh_get_plan {
  int64_t fwd_floats, bwd_floats, obs_floats;
  int64_t phi, word_w, evd_w, score, keep;          /* offsets (floats) of the observable results inside the observables buffer:
                                                       phi [b][n_classes]; word_w [rows][word_heads] (rows = m_real, or b1*r padded);
                                                       evd_w [b][n_max][evd_heads]; score [b1][r]; keep [b1][W] uint64 (8-byte aligned) */
} gh_get_plan;
int gh_get_plan_buffers(const gh_get_model* model, const gh_get_batch* batch, gh_get_plan* plan);
/* sizeof of {gh_get_model, gh_get_batch, gh_get_plan, gh_cell_params, gh_cell_bf16}: lets a binding verify its mirror of the structs. */
int gh_get_struct_sizes(int64_t* out5_host);
/* Forward into `arena_fwd` (plan.fwd_floats floats) and `obs` (plan.obs_floats floats); both 256-byte aligned and kept until
 * the backward has run (evaluation: the arena may be released as soon as the call has been issued and the stream drained). */
int gh_get_forward(const gh_get_model* model, const gh_get_batch* batch, float* arena_fwd, float* obs, gh_stream_t stream,
                   gh_stream_t side_stream);
/* Backward from g_phi [b][n_classes] (+ optional g_word_w / g_evd_w, shaped like the forward's weights outputs, or NULL).
 * phase 0: everything; 1: down to and including the second evidence cell -- every gradient outside the first evidence cell
 * and the claim branch is final in stream order when it returns (the data-parallel early all-reduce starts here);
 * 2: the rest (first evidence cell; joins the side stream).  Gradients are ACCUMULATED into model->d*. */
int gh_get_backward(const gh_get_model* model, const gh_get_batch* batch, const float* arena_fwd, const float* obs, float* arena_bwd,
                    const float* g_phi, const float* g_word_w, const float* g_evd_w, int phase,
                    gh_stream_t stream, gh_stream_t side_stream);
/* Mean cross-entropy of logits [b][c] against labels [b] (int64, clamped into [0, c): no ignore_index), fused with its gradient (losses.py:29-32 CrossEntropyLoss):
 * loss[0] = mean_b(logsumexp(phi_b) - phi_b[y_b]); dphi [b][c] = (softmax(phi_b) - onehot(y_b)) / b. */
int gh_cross_entropy(const float* phi, const int64_t* labels, int b, int c, float* loss, float* dphi, gh_stream_t stream);
/* Batch preparation in one call (interactions.py:334-351 for both sides + basic_fc_model.py:94-121's padded document):
 * graph build of the b claims and b1 evidences, node-compact plan (m_real must be known to the host; < 0 = skip the plan)
 * and the scatter of the evidence node ids into document[b][n_max][r] (slot[b1] = row of each pair; rows of unused slots
 * must be zero already and stay untouched). */
int gh_get_prepare(const int32_t* claim_tokens, const int32_t* claim_len, int b, int l,
                   const int32_t* evd_tokens, const int32_t* evd_len, int b1, int r, int window,
                   int32_t* q_ids, int32_t* q_n, uint64_t* q_bits, float* q_dinv,
                   int32_t* d_ids, int32_t* d_n, uint64_t* d_bits, float* d_dinv,
                   int m_real, int32_t* goff, int32_t* rowg, int32_t* src, int32_t* cids, float* maskf,
                   const int64_t* slot, int32_t* document, gh_stream_t stream);

/* ---- evaluation: the integers the fitter's metrics are exact functions of (Fitting/FittingFC/char_man_fitter_query_repr1.py:353
 *      and :358 `probs.argmax(dim=1)`, :360 `probs[:, 1]`, :362 and :381-401 `_computing_metrics`' sklearn calls) from logits
 *      phi [n] rows of c floats, ldphi >= c floats apart, and labels [n] (int64 when labels_i64, else int32).  No softmax is applied:
 *      the reference ranks by the raw logit.
 *   pred [n] (NULL ok): argmax of every row, the first index among equal maxima (a NaN counts as the maximum, as in torch.argmax).
 *   out [c*c + 8], written as a whole:
 *     out[t*c + p]  rows with label t and prediction p
 *     out[c*c + 0]  U2 = sum over rows i with label == pos_class and rows j with label != pos_class of
 *                   2 [s_i > s_j] + [s_i == s_j], s = phi[:, pos_class], IEEE comparison (-0.0 == 0.0, +-inf ordinary values):
 *                   AUC = U2 / (2 n_pos n_neg), the trapezoid area of roc_curve(pos_label = pos_class) + auc
 *     out[c*c + 1]  n_pos, rows with label == pos_class;  out[c*c + 2]  n_neg, rows with any other label in [0, c)
 *     out[c*c + 3]  rows whose label lies outside [0, c): left out of every other count
 *     out[c*c + 4]  rows (with a label in [0, c)) that hold a NaN among their c logits: left out of every other count
 *     out[c*c + 5 .. 7]  reserved, zero
 * Integer arithmetic throughout (64-bit integer atomic adds of per-workgroup sums into `out`, no floating-point atomics): the
 * result is exact and independent of tiling and launch geometry.  Limits: 2 <= c <= GH_CLS_MAX_CLASSES,
 * 1 <= n <= GH_CLS_MAX_ROWS (the launch grid and the 32-bit row index; n = 0 is rejected), 0 <= pos_class < c. */
#define GH_CLS_MAX_CLASSES 8
#define GH_CLS_MAX_ROWS (1 << 20)
int gh_cls_metrics(const float* phi, int ldphi, const void* labels, int labels_i64, int n, int c, int pos_class,
                   int32_t* pred, int64_t* out, gh_stream_t stream);

/* ---- ranking metrics: matchzoo/metrics/{precision, average_precision, mean_average_precision, mean_reciprocal_rank,
 *      discounted_cumulative_gain, normalized_discounted_cumulative_gain}.py for every group of a ragged batch in ONE launch.
 *   scores [n]      float, or double when scores_f64 (widened to double either way: equal values give equal results)
 *   labels [n]      double
 *   offsets [g+1]   int32 on the device, non-decreasing from 0 to n: group q is the items offsets[q] .. offsets[q+1] (the ragged
 *                   convention of gh_seg_offsets); an empty group is legal and scores 0 everywhere
 *   offsets_host    the same g + 1 values in HOST memory: the limits below are checked on them before anything is launched (the
 *                   kernel also skips a group whose device offsets leave [0, n] or the group limit, writing nothing for it)
 *   ks [nk]         int32 in HOST memory, the cut-offs k of precision@k, dcg@k and ndcg@k
 *   An item is relevant when label > threshold.
 *   rank [n]        0-based position of every item in the reference's ordering of its group, sorted(key=score, reverse=True)
 *                   (engine/base_metric.py:36-39; stable: ties to the lower index): #{j : s_j > s_i} + #{j < i : s_j == s_i} with
 *                   IEEE comparisons on values (-0.0 == 0.0, +-inf ordinary values).  A permutation of 0 .. len-1 per group.
 *   group_int [g][3 + nk], exact:
 *     [0] items of the group   [1] n_rel, its relevant items   [2] 1-based position of the first relevant item, 0 if none
 *     [3 + i] hits: relevant items at positions < ks[i]
 *   group_f64 [g][3 + 3 nk]:
 *     [0] AveragePrecision: (1/len) sum_{k=1..len} hits0(k) / k, hits0 counted at threshold 0 whatever `threshold` is
 *         (average_precision.py:41 builds Precision(k + 1) with the default threshold)
 *     [1] MeanAveragePrecision: sum over the relevant positions idx of (relevant items up to idx) / (idx + 1), over n_rel; 0 if none
 *     [2] MeanReciprocalRank: 1 / group_int[2]; 0 if none
 *     [3 + i] Precision@ks[i] = hits / ks[i]
 *     [3 + nk + i] DCG@ks[i] = sum over the relevant positions p < ks[i] of (2^label - 1) / ln(2 + p)
 *     [3 + 2 nk + i] NDCG@ks[i] = DCG / IDCG, 0 if IDCG == 0; IDCG is the DCG of the group ordered by label (stable likewise)
 *   nan_count [2]   NaN scores, NaN labels.  A NaN compares false with everything, as it does in Python's sort, whose result is
 *                   then unspecified: when either counter is nonzero the float outputs of the groups concerned mean nothing.
 * Every per-group float is summed by one wave in an order that depends on the group's length and k only (lane l adds the
 * positions l, l + 64, ..., then a butterfly over the lanes): no floating-point atomics, two runs are bit-identical.  Each term
 * is correct to a few ulp and non-negative, so a value differs from the reference's left-to-right sum by less than
 * 1024 * 4 * 2^-53 relative; a value that is 0 in the reference is exactly 0.
 * Limits: 1 <= g <= GH_RANK_MAX_GROUPS, 0 <= n <= GH_RANK_MAX_ITEMS, 1 <= nk <= GH_RANK_MAX_KS, every ks[i] >= 1, a finite or
 * infinite (not NaN) threshold, offsets_host[0] == 0, offsets_host[g] == n, non-decreasing, at most GH_RANK_MAX_GROUP items per
 * group (the four 8 KB LDS tiles of a workgroup).  A call that breaks one returns an error and nothing is written. */
#define GH_RANK_MAX_GROUP 1024
#define GH_RANK_MAX_KS 8
#define GH_RANK_MAX_GROUPS (1 << 24)
#define GH_RANK_MAX_ITEMS (1 << 30)
int gh_rank_metrics(const void* scores, int scores_f64, const double* labels, const int32_t* offsets, const int32_t* offsets_host,
                    int n, int g, double threshold, const int32_t* ks, int nk, int32_t* rank, int32_t* group_int, double* group_f64,
                    int32_t* nan_count, gh_stream_t stream);

/* ---- ranking losses on y [rows] rows of c floats, ld >= c floats apart: instance b is row b (num_neg + 1), its positive, and the
 *      num_neg rows behind it, its negatives.  fp32; every value is summed in a fixed order (two runs are bit-identical) and
 *      every gradient element has one writer.  dy is [rows][c], contiguous.
 * Limits (all four): 1 <= c <= ld, 1 <= rows <= GH_RANK_MAX_ROWS and rows a multiple of num_neg + 1 (the reference raises a
 * shape error otherwise), num_neg <= GH_RANK_MAX_NEG, num_neg >= 1 for the hinge loss and >= 0 for the cross-entropy.  A call
 * that breaks one returns an error and nothing is written.
 *
 * RankHingeLoss (matchzoo/losses/rank_hinge_loss.py:54-66), B = rows / (num_neg + 1):
 *   neg_mean [B] (saved for the backward) = mean of the instance's num_neg * c negative entries
 *   element (b, j) = max(0, margin - (y_pos[b][j] - neg_mean[b]))
 *   reduction 0 'none': elem [B][c] is written (part, loss unused, may be NULL);  1 'mean' / 2 'sum': loss[0] = the mean / sum of
 *   the B c elements, through part [B] (scratch: the per-instance sums; elem unused, may be NULL)
 *   backward: g is [B][c] (reduction 0) or one float; an element passes its gradient where margin - (y_pos - neg_mean) >= 0, as
 *   torch's clamp_min does. */
#define GH_RANK_MAX_ROWS (1 << 24)
#define GH_RANK_MAX_NEG 4095
int gh_rank_hinge_fwd(const float* y, int ld, int rows, int c, int num_neg, float margin, int reduction, float* neg_mean, float* elem,
                      float* part, float* loss, gh_stream_t stream);
int gh_rank_hinge_bwd(const float* y, int ld, int rows, int c, int num_neg, float margin, int reduction, const float* neg_mean,
                      const float* g, float* dy, gh_stream_t stream);
/* RankCrossEntropyLoss (matchzoo/losses/rank_cross_entropy_loss.py:29-38): the logits of instance b are its rows side by side,
 * [pos | neg_1 | ... | neg_num_neg], (num_neg + 1) c of them, the labels the same entries of y_true (rows ldt floats apart):
 *   loss[0] = -mean_b sum_j labels[b][j] * log_softmax(logits[b])[j], with log_softmax = x - max - log(sum exp(x - max)): finite
 *   where the reference's log(softmax(x)) underflows to -inf (a logit some 104 below its row maximum).
 *   lse [B] (saved for the backward) = the log-sum-exp of every instance; part [B] scratch.
 *   backward: g one float; dy = g / B * (softmax * sum_j labels - labels); the labels are constants. */
int gh_rank_ce_fwd(const float* y, int ld, const float* y_true, int ldt, int rows, int c, int num_neg, float* lse, float* part,
                   float* loss, gh_stream_t stream);
int gh_rank_ce_bwd(const float* y, int ld, const float* y_true, int ldt, int rows, int c, int num_neg, const float* lse, const float* g,
                   float* dy, gh_stream_t stream);

/* ---- pairwise interaction helpers (csrc/pair_ops.hip): added under ABI 10, nothing existing changes ----
 * Row operands take a leading dimension (floats between rows, batch i row r at (i * rows + r) * ld): column slices of a wider
 * tensor are read in place.  Outputs and gradients are contiguous.  One writer per output element, no floating-point atomics.
 *
 * torch_utils.py:311-329 (cosine_distance, which is the Euclidean distance): a [bn][l][d] lda, b [bn][r][d] ldb,
 *   out [bn][l][r] = sqrt(|inner| + eps), inner = (A2_l - 2 a_l.b_r) + B2_r in the reference's order of operations, so that
 *   coincident rows give rounding noise under the root, as there.  a2 [bn][l], b2 [bn][r] receive the squared row norms and
 *   sgn [bn][l][r] one byte per entry, sign(inner) in {-1, 0, 1}: the backward needs it and out does not hold it.
 *   Limits: l, r <= 1024, d <= 2048, eps finite and >= 0. */
int gh_pair_l2_fwd(const float* a, const float* b, int lda, int ldb, float eps, int bn, int l, int r, int d, float* a2, float* b2,
                   float* out, int8_t* sgn, gh_stream_t stream);
/* Backward from g [bn][l][r] with the forward's out and sgn: w = g 0.5 / out sgn (sign(0) = 0: such an entry sends nothing),
 * da_l = 2 a_l sum_r w_lr - 2 sum_r w_lr b_r, db_r = 2 b_r sum_l w_lr - 2 sum_l w_lr a_l; da [bn][l][d], db [bn][r][d]. */
int gh_pair_l2_bwd(const float* a, const float* b, int lda, int ldb, const float* out, const int8_t* sgn, const float* g, int bn, int l,
                   int r, int d, float* da, float* db, gh_stream_t stream);
/* torch_utils.py:332-348 (l1_distance): out [bn][l][r] = sum_k |a_lk - b_rk|, summed in k order, without the reference's
 * [bn][l][r][d] difference tensor.  Limits: l, r <= 1024, d <= 2048. */
int gh_pair_l1_fwd(const float* a, const float* b, int lda, int ldb, int bn, int l, int r, int d, float* out, gh_stream_t stream);
/* Backward from g [bn][l][r]: da_lk = sum_r g_lr sign(a_lk - b_rk) in r order, db_rk = -sum_l g_lr sign(a_lk - b_rk) in l order,
 * with sign(0) = 0 as the backward of torch's norm(p=1) has it. */
int gh_pair_l1_bwd(const float* a, const float* b, int lda, int ldb, const float* g, int bn, int l, int r, int d, float* da, float* db,
                   gh_stream_t stream);
/* torch_utils.py:292-308 (moving_average), :351-376 (_get_doc_context_copacrr) and layers.py:42-66 (MovingAverage):
 *   out [bn][lo][d], lo = l + left + right - w + 1 >= 1, out[t] = mask[t] / w * sum_{s = t - left}^{t - left + w - 1} x[s] over
 *   x [bn][l][d] ldx, the `left` rows before and the `right` rows behind the sequence counting as zeros (F.pad).  Every window
 *   is summed directly, in row order, never from a running prefix.  mask [bn][lo] fp32 or NULL; a row whose mask is 0 is an
 *   exact zero.  moving_average / MovingAverage: left = right = 0, mask = NULL; the context form of window c: left = c / 2,
 *   right = c - c / 2 - 1, w = c.  Limits: w, left, right <= 1024, l <= 2^20, d <= 2048. */
int gh_window_mean_fwd(const float* x, int ldx, const float* mask, int bn, int l, int d, int w, int left, int right, float* out,
                       gh_stream_t stream);
/* Backward from g [bn][lo][d] ldg: dx [bn][l][d], dx[s] = 1 / w * sum_{t = s + left - w + 1}^{s + left} mask[t] g[t] over the
 * existing t: the same window, reversed, over the masked g.  A row whose mask is 0 sends an exact zero. */
int gh_window_mean_bwd(const float* g, int ldg, const float* mask, int bn, int l, int d, int w, int left, int right, float* dx,
                       gh_stream_t stream);
/* matchzoo/preprocessors/units/matching_histogram.py:44-60 for a batch (data_generator/callbacks/histogram.py:37-65):
 *   table [v][d] ldt, inv_norm [v] or NULL (the products are then scaled by inv_norm[left id] inv_norm[right id]),
 *   ids_left [bn][lq], ids_right [bn][ld], len_right [bn] int32 (clamped into [0, ld]); out [bn][lq][bins] fp32.
 *   Entry (i, bin) starts from 1 and counts the right ids j < len_right of its sample with
 *   int((table[left_i].table[right_j] + 1) / 2 * (bins - 1)) == bin, truncated toward zero and clamped into [0, bins - 1];
 *   right ids at or beyond len_right are ignored, every left id counts.  mode 0 (CH) leaves the counts, 1 (NH) divides by the row
 *   total bins + len_right, 2 (LCH) takes the logarithm.  The rows are gathered through the ids, no gathered copy is written.
 *   An id outside [0, v) fails the call (flag: one int32 of device scratch; the verdict is read back before anything is read
 *   through an id, so the call synchronises the stream).  No backward.  Limits: lq, ld <= 1024, d <= 2048, bins <= 256. */
int gh_match_hist(const float* table, int ldt, const float* inv_norm, int v, int d, const int32_t* ids_left, const int32_t* ids_right,
                  const int32_t* len_right, int bn, int lq, int ld, int bins, int mode, float* out, int32_t* flag, gh_stream_t stream);

/* ---- embedding table: torch.nn.Embedding as Models/base_model.py:144-162 builds it (_make_default_embedding_layer with
 *      embedding_freeze, _make_entity_embedding_layer) and graph_based_semantic_structure.py:100,113,150,169 and
 *      Models/BiDAF/bidaf_model.py:128-129 look it up ----
 * Forward (ATen's embedding): out [m][d] = table[ids[i]] for a table [vocab][d]; any d >= 1, float4 copies where d % 4 == 0 and
 * both row sets are 16-byte aligned.  An id outside [0, vocab) is clamped into the table for memory safety (nn.Embedding
 * raises); the backward counts it. */
int gh_embed_fwd(const float* table, const int32_t* ids, float* out, int m, int d, int vocab, gh_stream_t stream);
/* Backward (ATen's embedding_dense_backward, and the zeros + index_add_ of a table gradient): dtable[t][:] += the sum of the
 * rows dx[i][:] with ids[i] == t, for dx [m][d] with the leading dimension ldx >= d (floats) and dtable [vocab][d], addressed in
 * 64 bits.  It ACCUMULATES; a row of dtable that no id names is neither read nor written.
 *   sorted_ids [m], perm [m] int32: the ids in ascending order and, for every sorted position, its row of dx; equal ids in
 *   ascending row order (a stable sort of the ids gives both).
 *   padding_idx: rows with that id contribute nothing (-1 = none).  So do rows whose id is outside [0, vocab); those are counted
 *   in slot [3] of gh_clamp_events (the padding id is not), and nothing is ever written through them.
 *   workspace: 2 * ceil(m / GH_EMBED_CHUNK) * d floats of scratch (workspace_floats says how many there are); nothing allocates.
 * The order of the additions is part of the contract, so that a host restatement (tests/embed_ref.py) gives the same bits and
 * two calls on the same inputs give the same table on any grid and device:
 *   1. the sorted positions 0 .. m-1 are cut into chunks of GH_EMBED_CHUNK;
 *   2. inside a chunk the rows of a run of equal ids are added one after the other in ascending sorted position, starting from
 *      the run's first row: the chunk's partial p_c of that id;
 *   3. a run that spans the chunks c_1 < .. < c_k is combined as ((p_1 + p_2) + ..) + p_k;
 *   4. the result is added to the table row once: dtable[t] = dtable[t] + (..).
 * These are fp32 additions in round-to-nearest, no FMA.  One writer per element of dtable and no floating-point atomics.
 * m == 0 is a no-op.  Calls that accumulate into one dtable must be ordered by their streams. */
#define GH_EMBED_CHUNK 128
int gh_embed_bwd(const float* dx, long long ldx, const int32_t* sorted_ids, const int32_t* perm, int m, int d, int vocab,
                 int padding_idx, float* dtable, float* workspace, long long workspace_floats, gh_stream_t stream);

/* ---- BERT encoder (csrc/bert_ops.hip): pytorch_transformers/modeling_bert.py, which matchzoo/modules/bert_module.py:22-30 wraps ----
 * Multi-head self-attention with an additive per-key bias, a temperature and dropout on the probabilities, replacing
 * BertSelfAttention.forward :203-228 (the three transpose_for_scores permutes, both matmul, the division by
 * sqrt(attention_head_size), the mask addition, the softmax, the dropout and the permute copy of the context):
 *   q [b][lq][heads * dh], k, v [b][lk][heads * dh], row r of batch i at (i * l + r) * ld, each with its own leading dimension
 *   (ld >= heads * dh): head h is the column slice [h * dh, (h + 1) * dh), read in place, so the three may be the column
 *   blocks of one [rows][3 * heads * dh] buffer.  bias [b][lk] fp32 or NULL (= zeros): the host forms (1 - mask) * -10000
 *   as :603 does.  P = softmax(scale q_h k_h^T + bias) over ALL lk keys, with the reference's roundings (the scaled score is
 *   rounded, then the bias is added) and the running maximum subtracted: a row whose keys all carry the bias -10000 is the
 *   softmax of its raw scores (on the 2^-10 grid fp32 has next to 10000), never zeros.
 *   out [b][lq][heads * dh] (ldo) = (P . keep / (1 - drop_p)) v_h; element (i, h, r, j) of P is kept iff
 *   drop_hash(seed, ((i * heads + h) * lq + r) * lk + j) >= drop_p * 2^32, the stateless rule of gh_feat_dropout over the
 *   element index of a [b * heads * lq][lk] tensor (drop_p > 0 needs b * heads * lq * lk < 2^32).  drop_p == 0 runs kernels
 *   that hold no hash at all.  lse [b][heads][lq] = max + log(sum exp(. - max)) of every row is the only state the backward
 *   needs besides q, k, v, bias and out: no [lq][lk] tensor is read or written in HBM in either direction.
 * Limits: 1 <= heads <= 16, lq <= 1024, lk <= 1024, dh <= 512, b * ceil(max(lq, lk) / 16) < 2^31; anything beyond them, a
 * NULL tensor or a leading dimension below heads * dh is rejected with an error and nothing is written. */
int gh_bert_attention_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* bias,
                          int b, int heads, int lq, int lk, int dh, float scale, float drop_p, uint32_t seed,
                          float* out, int ldo, float* lse, gh_stream_t stream);
/* Backward of the above (autograd of :203-228) from g_out [b][lq][heads * dh] (ldgo), with P recomputed from q, k, bias and
 * lse as exp(scale q_h k_h^T + bias - lse) and keep regenerated from (drop_p, seed), per head:
 *   delta = rowsum(g_out . out) ( = rowsum(P . keep / (1 - p) . dP), so it holds under dropout), dP = g_out v^T,
 *   dS = P . (keep / (1 - p) . dP - delta), dq = scale dS k, dk = scale dS^T q, dv = (P . keep / (1 - p))^T g_out.
 * delta [b][heads][lq] is caller-provided scratch of lse's size, written by the first launch and read by the second.  Every
 * element of dq [b][lq][heads * dh] (lddq), dk, dv [b][lk][heads * dh] (lddk, lddv) is written by one owner: two calls give
 * the same bits.  Limits and refusals as the forward. */
int gh_bert_attention_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* bias,
                          const float* out, int ldo, const float* lse, const float* g_out, int ldgo,
                          int b, int heads, int lq, int lk, int dh, float scale, float drop_p, uint32_t seed,
                          float* delta, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, gh_stream_t stream);
/* Elementwise activations over a contiguous [rows][n] tensor, 16 bytes per lane where the pointers are 16-byte aligned and
 * single floats for the last rows * n % 4 elements or an unaligned pointer (in place ok).  GH_ACT_GELU: x * 0.5 * (1 +
 * erf(x / sqrt(2))), the erf form of :120-126 that BertIntermediate :296 applies; GH_ACT_TANH: BertPooler's nn.Tanh :373.
 * The backward takes the saved pre-activation: dx = g * act'(x).  The linear layers' bias stays with gh_linear_*. */
#define GH_ACT_GELU 0
#define GH_ACT_TANH 1
int gh_act_fwd(const float* x, float* y, int rows, int n, int mode, gh_stream_t stream);
int gh_act_bwd(const float* x, const float* g, float* dx, int rows, int n, int mode, gh_stream_t stream);
/* BertEmbeddings.forward :156-169 without its dropout, in one pass over rows = batch * l tokens: sum[r] = word[ids[r]] +
 * pos[pos_ids[r]] + type[type_ids[r]] (added in that order) and y[r] = LayerNorm(sum[r]) * gamma + beta (biased variance,
 * eps inside the root), replacing three lookups, two additions and the LayerNorm.  pos_ids NULL: the column index r % l
 * (:159-160); type_ids NULL: row 0 of the type table (:161-162).  word [vocab][d], pos [npos][d], type [ntype][d], d <= 2048
 * (what gh_add_layernorm_bwd, which starts the backward on the saved `sum`, takes).  An id outside its table is clamped into
 * it for memory safety (nn.Embedding raises) and counted in slot [3] of gh_clamp_events.  Writes sum and y [rows][d], mean
 * and rstd [rows].  The table gradients are three gh_embed_bwd calls on the gradient gh_add_layernorm_bwd returns. */
int gh_bert_embed_fwd(const float* word, const float* pos, const float* type, const int32_t* ids, const int32_t* pos_ids,
                      const int32_t* type_ids, const float* gamma, const float* beta, float eps, int rows, int l, int d,
                      int vocab, int npos, int ntype, float* sum, float* y, float* mean, float* rstd, gh_stream_t stream);

/* ---- softmax cross-entropy with an ignore index (csrc/loss_ops.hip): the CrossEntropyLoss(ignore_index) every task model of
 *      pytorch_transformers/modeling_bert.py ends in (:698, :765, :822, :890, :996, :1056, :1142), up to the masked-LM loss over
 *      (B * L, vocab_size) logits ----
 * Logits: fp32, element (r, j) at x[r * ldx + j * cs], cs >= 1, ldx >= (c - 1) * cs + 1: a column slice of a wider tensor, or
 * one of the two columns of the question-answering head's (B, L, 2) output (cs = 2, ldx = 2 L), is read in place.  labels[rows]:
 * int64 (labels_i64 != 0) or int32.  A row is KEPT iff its label is not ignore_index and lies in [0, c); ignore_index is any
 * 64-bit value (-1, -100, c).  A label outside [0, c) that is not ignore_index makes torch raise; here the row is dropped like
 * an ignored one and counted in slot [4] of gh_clamp_events_n, and nothing is read or written through it.
 * Forward: lse[r] = log sum_j exp(x[r][j]) for EVERY row, by a running maximum m and sum s (one read of the logits, no exp
 * overflow), rounded to fp32, and lse_lo[r] = (m + log s) - lse[r], what that rounding dropped: at logits of 1e4 fp32 has a grid
 * of 2^-10, and probabilities formed from lse[r] alone would be off by a relative 5e-4.  row_loss[r] (scratch of `rows`
 * floats) = (m - x[r][label]) + log s for a kept row, 0 otherwise; then
 *     n_kept[0] = the number of kept rows,   loss[0] = (sum over kept rows of row_loss) / n_kept      (NaN when no row is kept)
 * summed without floating-point atomics in a fixed order: in double, in 256 contiguous runs of ceil(rows / 256) rows in row
 * order, the runs' sums in run order, rounded once to fp32.  Two calls give the same bits, and so do a strided view and its
 * contiguous copy (the float4, float2 and element-wise variants of a path share the order of every operation).  c = 1: loss 0.
 * Backward: dx[r * lddx + j * dcs] = (exp((x[r][j] - lse[r]) - lse_lo[r]) - [j == label_r]) * g[0] / n_kept[0] for a kept row and exactly 0
 * for every other row; g (the upstream gradient of the scalar loss) and n_kept are read on the device.  One read of the
 * logits, one write of dx, one writer per element; what lies between the rows or the elements of dx is not touched.  Only lse
 * and lse_lo, two floats per row, live between the two calls.
 * Paths by c: <= 32 one lane per row, <= 2048 one wave per row, wider one workgroup per row; the two wide paths with float4
 * accesses where cs (and dcs) == 1 and base and row stride are multiples of 16 bytes, float2 where they are multiples of 8 (a
 * contiguous matrix of 30522-wide rows: 30522 = 2 mod 4), element-wise otherwise; the three give the same bits.
 * Refused: NULL pointers, rows <= 0 (an empty input is the caller's to answer) or > 2^31 - 1, c <= 0, cs or dcs < 1, a row
 * stride below the span of a row. */
int gh_softmax_xent_fwd(const float* x, int64_t ldx, int cs, const void* labels, int labels_i64, int64_t ignore_index, int64_t rows,
                        int c, float* lse, float* lse_lo, float* row_loss, float* loss, int64_t* n_kept, gh_stream_t stream);
int gh_softmax_xent_bwd(const float* x, int64_t ldx, int cs, const void* labels, int labels_i64, int64_t ignore_index, int64_t rows,
                        int c, const float* lse, const float* lse_lo, const float* g, const int64_t* n_kept, float* dx, int64_t lddx,
                        int dcs, gh_stream_t stream);

/* Everything the forward / backward need that is DERIVED from weight matrices, for n matrices in one launch (after the
 * optimiser step): dst_t[i] = src[i]^T as fp32 [cols][rows] (the backward's dX operands), and -- bf16 storage mode, any of the
 * two arrays or any entry may be NULL -- dst_w16[i] = bf16(src[i]) [rows][cols], dst_t16[i] = bf16(src[i]^T) [cols][rows]. */
int gh_weights_refresh(int n, const void* const* src, void* const* dst_t, void* const* dst_w16, void* const* dst_t16,
                       const int* rows, const int* cols, gh_stream_t stream);

/* ---- measurement hook (bench.py): HIP events around every kernel launch on its own stream ----
 * rows of `out` (each {total ms, total algorithmic work, launches}; work = flops for GEMMs, bytes otherwise):
 * 0 activation-sized GEMM launches (>= 8192 rows) NT/NN, 1 same TN, 2 few-row GEMM launches NT/NN, 3 same TN, 4 spmm, 5 scorer_gsl,
 * 6 graph_build, 7 att_softmax_fwd, 8 att_softmax_bwd, 9 att_dpre, 10 gate_bwd_pre, 11 colsum, 12 adam */
#define GH_PROFILE_ROWS 13
int gh_profile_enable(int on);
/* Restrict the instrumentation to the rows whose bit is set in tag_mask (default: all).  Two events per launch cost
 * ~1.5 us of queue bubbles each, ~0.4 ms per bench step when every kernel is instrumented: bench.py times the step
 * with only the dominant kernel's row selected and collects the full table in an extra, untimed pass. */
int gh_profile_select(uint32_t tag_mask);
int gh_profile_collect(double* out_host, int rows);

/* GEMM launches since the last reset: out_host[0] on the float4 fast kernel, [1] on the generic (scalar-guarded) kernel,
 * [2] on the generic kernel with >= 1 GFLOP of work -- the last one should stay 0 in a healthy training step (a large
 * GEMM only falls back when an operand is misaligned or oddly shaped). */
int gh_gemm_path_counters(int64_t* out_host, int reset);

#ifdef __cplusplus
}
#endif
#endif /* GET_HIP_H */
