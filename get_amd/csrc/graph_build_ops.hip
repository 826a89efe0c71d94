// Graph construction and hand-over: the word-graph build of a text (one side or both sides of a batch), dense adjacency <-> packed
// bit rows + values, and the reference fitter's de-padding.  HBM-bound integer / bit work, one workgroup per graph.
#include "../../include/get_hip.h"
#include "common.h"

namespace gh {

// ------------------------------------------------------------------------------------------------
// a1  graph build (interactions.py:334-351).  One workgroup per text.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void graph_build_body(const int g, const int32_t* __restrict__ tokens, const int32_t* __restrict__ lengths, int R,
                                                 int window, int32_t* __restrict__ node_ids, int32_t* __restrict__ n_nodes,
                                                 uint64_t* __restrict__ bits, float* __restrict__ dinv) {
  __shared__ int tok[MAX_R];
  __shared__ int first[MAX_R];       // position of the first occurrence of tok[i]
  __shared__ int node_of[MAX_R];     // node index of position i
  __shared__ unsigned long long rows[MAX_R * MAX_W];
  __shared__ int total;
  const int tid = threadIdx.x;
  const int W = (R + 63) / 64;
  int len = lengths[g];
  len = len < 0 ? 0 : (len > R ? R : len);
  for (int i = tid; i < R; i += blockDim.x) tok[i] = (i < len) ? tokens[(size_t)g * R + i] : 0;
  for (int i = tid; i < R * W; i += blockDim.x) rows[i] = 0ull;
  __syncthreads();
  // first occurrence (words_list.sort(key=raw_text.index), :335-336)
  for (int i = tid; i < len; i += blockDim.x) {
    int f = i;
    const int t = tok[i];
    for (int j = 0; j < i; ++j)
      if (tok[j] == t) { f = j; break; }
    first[i] = f;
  }
  __syncthreads();
  // node index = number of first-occurrence positions before first[i]
  for (int i = tid; i < len; i += blockDim.x) {
    const int f = first[i];
    int c = 0;
    for (int j = 0; j < f; ++j) c += (first[j] == j);
    node_of[i] = c;
  }
  if (tid == 0) {
    int c = 0;
    for (int j = 0; j < len; ++j) c += (first[j] == j);
    total = c;
  }
  __syncthreads();
  // node list, zero padded (:349)
  for (int i = tid; i < R; i += blockDim.x) node_ids[(size_t)g * R + i] = 0;
  __syncthreads();
  for (int i = tid; i < len; i += blockDim.x)
    if (first[i] == i) node_ids[(size_t)g * R + node_of[i]] = tok[i];
  // window links over POSITIONS, accumulated on nodes (:342-344)
  for (int i = tid; i < len; i += blockDim.x) {
    const int ni = node_of[i];
    const int lo = max(i - window + 1, 0), hi = min(i + window, len);
    for (int j = lo; j < hi; ++j) {
      const int nj = node_of[j];
      atomicOr(&rows[ni * W + (nj >> 6)], 1ull << (nj & 63));
    }
  }
  __syncthreads();
  for (int i = tid; i < R; i += blockDim.x) {
    int deg = 0;
    for (int w = 0; w < W; ++w) {
      const unsigned long long m = rows[i * W + w];
      bits[((size_t)g * R + i) * W + w] = m;
      deg += __popcll(m);
    }
    // D^-1/2 with zero-degree rows -> 0 (interactions.py:14-16)
    dinv[(size_t)g * R + i] = deg > 0 ? (float)(1.0 / sqrt((double)deg)) : 0.f;
  }
  if (tid == 0) n_nodes[g] = total;
}
__global__ void __launch_bounds__(256)
graph_build_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ lengths, int R, int window,
                   int32_t* __restrict__ node_ids, int32_t* __restrict__ n_nodes, uint64_t* __restrict__ bits,
                   float* __restrict__ dinv) {
  graph_build_body(blockIdx.x, tokens, lengths, R, window, node_ids, n_nodes, bits, dinv);
}
// both sides of a batch in one launch (gh_get_prepare): workgroups [0, na) build the claims, the rest the evidences
struct GraphSide { const int32_t* tokens; const int32_t* lengths; int R; int32_t* node_ids; int32_t* n_nodes; uint64_t* bits; float* dinv; };
__global__ void __launch_bounds__(256)
graph_build2_kernel(const GraphSide a, const GraphSide b, int na, int window) {
  const bool first = (int)blockIdx.x < na;      // workgroup-uniform
  const GraphSide& s = first ? a : b;
  graph_build_body(first ? blockIdx.x : blockIdx.x - na, s.tokens, s.lengths, s.R, window, s.node_ids, s.n_nodes, s.bits, s.dinv);
}

// ------------------------------------------------------------------------------------------------
// dense (N,R,R) adjacency -> packed bits + fp32 values.  One wave per row, ballot builds the word.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
adj_pack_kernel(const T* __restrict__ adj, int R, uint64_t* __restrict__ bits, float* __restrict__ vals) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = (R + 63) / 64;
  for (int i = wave; i < R; i += 4) {
    const size_t rb = ((size_t)g * R + i) * R;
    for (int w = 0; w < W; ++w) {
      const int j = w * 64 + lane;
      float v = 0.f, vt = 0.f;
      if (j < R) {
        v = (float)adj[rb + j];
        vals[rb + j] = v;
        vt = (float)adj[((size_t)g * R + j) * R + i];
      }
      // the bit pattern is SYMMETRISED (A[i][j] != 0 or A[j][i] != 0): the transposed aggregation of the backward walks
      // row i's bits and reads vals[j][i], so an entry present only in A^T must have its bit too; the extra entries
      // carry the value 0 in `vals` and change no result
      const unsigned long long m = __ballot(v != 0.f || vt != 0.f);
      if (lane == 0) bits[((size_t)g * R + i) * W + w] = m;
    }
  }
}

// The reference fitter's de-padding (char_man_fitter_query_repr1.py:204-250: a Python loop over the claims slicing
// `[:evd_count]` out of the padded (B, n_max, R) ids and (B, n_max, R, R) float64 adjacency, two host syncs per claim) plus the
// packing of the adjacency and the node counts the node-compact plan needs, in ONE pass over the handed-over tensors:
// workgroup (claim c, slot j) with j < counts[c] is pair p = sum(counts[:c]) + j; it narrows the ids, counts the real nodes
// (id >= 1), packs its R x R block (as adj_pack_kernel) and checks what the node-compact layout assumes (ids prefix-shaped,
// no edge on a padding node).  It also recognises the adjacency convert_text produces (interactions.py:11-18: D^-1/2 A D^-1/2
// of a binary graph, A[i][j] = dinv[i] dinv[j] with dinv = 1 / sqrt(row degree)): such a block is fully described by its bit
// rows + dinv (the kernels' "normalised" mode, 2 KB instead of 40 KB per graph); only for other blocks, or when `force_vals`
// says that some graph of the batch needs them, the dense fp32 values are written.
// stats = {pairs, real nodes, pairs that violate the layout assumption, pairs that are NOT normalised graphs, reserved}.
template <typename TI>
__global__ void __launch_bounds__(256)
ref_depad_kernel(const int64_t* __restrict__ counts, int B, int n_max, int R, const TI* __restrict__ ids, const double* __restrict__ adj,
                 int32_t* __restrict__ d_ids, uint64_t* __restrict__ bits, float* __restrict__ vals, float* __restrict__ dinv,
                 int32_t* __restrict__ n_nodes, unsigned long long* __restrict__ stats, int force_vals) {
  const int c = blockIdx.x / n_max, j = blockIdx.x % n_max;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int red[4];
  __shared__ int s_real[256];
  __shared__ float s_dinv[256];
  __shared__ int s_bad, s_weighted;
  const long long cnt_c = counts[c];
  const int cc = cnt_c < 0 ? 0 : (cnt_c > n_max ? n_max : (int)cnt_c);
  if (j >= cc) return;
  // pair index: clamped counts of the claims before c (B is a few hundred at most)
  int part = 0;
  for (int i = tid; i < c; i += 256) { const long long v = counts[i]; part += v < 0 ? 0 : (v > n_max ? n_max : (int)v); }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) red[wave] = part;
  if (tid == 0) { s_bad = 0; s_weighted = 0; }
  __syncthreads();
  const int p = red[0] + red[1] + red[2] + red[3] + j;
  const size_t slot = (size_t)c * n_max + j;
  // ids -> int32, real-node flags, node count
  int real = 0;
  if (tid < R) {
    const long long id = (long long)ids[slot * R + tid];
    d_ids[(size_t)p * R + tid] = (int32_t)id;
    real = id >= 1 ? 1 : 0;
  }
  s_real[tid] = real;
  int nn = real;
  for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o);
  __syncthreads();                      // (red is re-used: every thread has read it)
  if (lane == 0) red[wave] = nn;
  __syncthreads();
  nn = red[0] + red[1] + red[2] + red[3];
  int bad = (tid < R && real != (tid < nn ? 1 : 0)) ? 1 : 0;
  // pass 1 over the block: bit rows (union of A's and A^T's patterns) and row degrees -> dinv as gh_graph_build computes it
  const int W = (R + 63) / 64;
  const double* ab = adj + slot * (size_t)R * R;
  for (int i = wave; i < R; i += 4) {
    int deg = 0;
    for (int w = 0; w < W; ++w) {
      const int jj = w * 64 + lane;
      double v = 0.0, vt = 0.0;
      if (jj < R) { v = ab[(size_t)i * R + jj]; vt = ab[(size_t)jj * R + i]; }
      const unsigned long long m = __ballot((float)v != 0.f || (float)vt != 0.f);
      if (lane == 0) bits[((size_t)p * R + i) * W + w] = m;
      deg += __popcll(m);
    }
    if (deg > 0 && !s_real[i]) bad = 1;     // a padding node with edges: the node-compact layout would drop them
    if (lane == 0) s_dinv[i] = deg > 0 ? (float)(1.0 / sqrt((double)deg)) : 0.f;
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid < R) dinv[(size_t)p * R + tid] = s_dinv[tid];
  // pass 2 (the block is in L2 now): is every entry dinv[i] dinv[j] (to fp32 rounding of the fitter's float64 product)?
  int weighted = 0;
  for (int i = wave; i < R; i += 4) {
    const float di = s_dinv[i];
    for (int w = 0; w < W; ++w) {
      const int jj = w * 64 + lane;
      if (jj < R) {
        const float v = (float)ab[(size_t)i * R + jj];
        const float e = di * s_dinv[jj];
        // (a pattern entry whose own value is 0 -- present on the transposed side only -- is not a normalised graph either)
        const bool on = v != 0.f || (float)ab[(size_t)jj * R + i] != 0.f;
        if (on && !(fabsf(v - e) <= 4e-7f * e)) weighted = 1;
      }
    }
  }
  if (weighted) s_weighted = 1;
  __syncthreads();
  if (s_weighted || force_vals) {
    for (int i = wave; i < R; i += 4)
      for (int jj = lane; jj < R; jj += 64) vals[((size_t)p * R + i) * R + jj] = (float)ab[(size_t)i * R + jj];
  }
  if (tid == 0) {
    n_nodes[p] = nn;
    atomicAdd(&stats[0], 1ull);
    atomicAdd(&stats[1], (unsigned long long)nn);
    if (s_bad) atomicAdd(&stats[2], 1ull);
    if (s_weighted) atomicAdd(&stats[3], 1ull);
  }
}

__global__ void __launch_bounds__(256)
adj_unpack_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
                  const uint64_t* __restrict__ keep, int R, float* __restrict__ adj) {
  const int g = blockIdx.x;
  const int W = (R + 63) / 64;
  for (int it = threadIdx.x; it < R * R; it += blockDim.x) {
    const int i = it / R, j = it % R;
    bool on = (bits[((size_t)g * R + i) * W + (j >> 6)] >> (j & 63)) & 1ull;
    if (on && keep) {
      const bool ki = (keep[(size_t)g * W + (i >> 6)] >> (i & 63)) & 1ull;
      const bool kj = (keep[(size_t)g * W + (j >> 6)] >> (j & 63)) & 1ull;
      on = ki || kj;
    }
    float v = 0.f;
    if (on) v = vals ? vals[((size_t)g * R + i) * R + j] : dinv[(size_t)g * R + i] * dinv[(size_t)g * R + j];
    adj[((size_t)g * R + i) * R + j] = v;
  }
}

}  // namespace gh

using namespace gh;

extern "C" int gh_graph_build(const int32_t* tokens, const int32_t* lengths, int n_texts, int fixed_length,
                              int window, int32_t* node_ids, int32_t* n_nodes, uint64_t* bits, float* dinv,
                              gh_stream_t stream) {
  GH_REQUIRE(fixed_length > 0 && fixed_length <= MAX_R, "graph_build: fixed_length %d not in [1,%d]", fixed_length, MAX_R);
  GH_REQUIRE(window >= 1, "graph_build: window %d < 1", window);
  if (n_texts <= 0) return 0;
  prof_begin((hipStream_t)stream, PROF_GRAPH_BUILD);
  hipLaunchKernelGGL(graph_build_kernel, dim3(n_texts), dim3(256), 0, (hipStream_t)stream, tokens, lengths,
                     fixed_length, window, node_ids, n_nodes, bits, dinv);
  prof_end(PROF_GRAPH_BUILD, (double)n_texts * (12.0 * fixed_length + 8.0 * fixed_length * words_for(fixed_length) + 8.0),
           (hipStream_t)stream);
  GH_LAUNCH_CHECK();
  return 0;
}

int gh::launch_graph_build2(const int32_t* ta, const int32_t* la, int na, int ra, int32_t* ida, int32_t* nna, uint64_t* ba, float* da,
                            const int32_t* tb, const int32_t* lb, int nb, int rb, int32_t* idb, int32_t* nnb, uint64_t* bb, float* db,
                            int window, hipStream_t s) {
  GH_REQUIRE(ra > 0 && ra <= MAX_R && rb > 0 && rb <= MAX_R, "graph_build: fixed lengths %d / %d not in [1,%d]", ra, rb, MAX_R);
  GH_REQUIRE(window >= 1, "graph_build: window %d < 1", window);
  if (na + nb <= 0) return 0;
  const GraphSide A = {ta, la, ra, ida, nna, ba, da}, B = {tb, lb, rb, idb, nnb, bb, db};
  prof_begin(s, PROF_GRAPH_BUILD);
  hipLaunchKernelGGL(graph_build2_kernel, dim3(na + nb), dim3(256), 0, s, A, B, na, window);
  prof_end(PROF_GRAPH_BUILD, (double)na * (12.0 * ra + 8.0 * ra * words_for(ra) + 8.0) + (double)nb * (12.0 * rb + 8.0 * rb * words_for(rb) + 8.0), s);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_adj_pack_f64(const double* adj, int n, int r, uint64_t* bits, float* vals, gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "adj_pack: r=%d not in [1,%d]", r, MAX_R);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(adj_pack_kernel<double>, dim3(n), dim3(256), 0, (hipStream_t)stream, adj, r, bits, vals);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_adj_pack_f32(const float* adj, int n, int r, uint64_t* bits, float* vals, gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "adj_pack: r=%d not in [1,%d]", r, MAX_R);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(adj_pack_kernel<float>, dim3(n), dim3(256), 0, (hipStream_t)stream, adj, r, bits, vals);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_ref_depad(const int64_t* counts, int b, int n_max, int r, const void* ids, int ids_i64, const double* adj,
                            int32_t* d_ids, uint64_t* bits, float* vals, float* dinv, int32_t* n_nodes, int64_t* stats, int force_vals,
                            gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "ref_depad: r=%d not in [1,%d]", r, MAX_R);
  GH_REQUIRE(b >= 0 && n_max > 0 && counts && ids && adj && d_ids && bits && vals && dinv && n_nodes && stats, "ref_depad: bad arguments");
  GH_CHECK_HIP(hipMemsetAsync(stats, 0, 5 * sizeof(int64_t), (hipStream_t)stream));
  if (b == 0) return 0;
  if (ids_i64)
    hipLaunchKernelGGL(ref_depad_kernel<int64_t>, dim3(b * n_max), dim3(256), 0, (hipStream_t)stream, counts, b, n_max, r,
                       (const int64_t*)ids, adj, d_ids, bits, vals, dinv, n_nodes, (unsigned long long*)stats, force_vals);
  else
    hipLaunchKernelGGL(ref_depad_kernel<int32_t>, dim3(b * n_max), dim3(256), 0, (hipStream_t)stream, counts, b, n_max, r,
                       (const int32_t*)ids, adj, d_ids, bits, vals, dinv, n_nodes, (unsigned long long*)stats, force_vals);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_adj_unpack(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep, int n,
                             int r, float* adj, gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "adj_unpack: r=%d not in [1,%d]", r, MAX_R);
  GH_REQUIRE(vals || dinv, "adj_unpack: need dinv or vals");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(adj_unpack_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, bits, dinv, vals, keep, r, adj);
  GH_LAUNCH_CHECK();
  return 0;
}
