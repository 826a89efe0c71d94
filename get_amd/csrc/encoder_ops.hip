// The wrapper module's other graph encoders (Models/BiDAF/wrapper.py:7-151): the GAT layer's masked edge-softmax
// aggregation over bit rows (forward and backward), the GCN normalisation, and the two elementwise passes the encoders
// need (stateless feature dropout; row scale with an optional ReLU mask).  The projections and weight gradients run on
// the library's grouped GEMMs (gh_linear_fwd / gh_linear_bwd), the GCN aggregation on the fp32 gh_spmm.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include <math.h>

namespace gh {
namespace {

constexpr int GAT_MAX_R = 256;           // one workgroup per graph, like every other gh_* graph kernel
constexpr int GAT_MAX_H = 8;
constexpr int GAT_MAX_F = 1024;          // per-head width: the backward keeps one head's row in registers (16 per lane)
constexpr int GAT_KF = GAT_MAX_F / 64;

struct GatArgs {
  const uint64_t* bits;
  const float* vals;
  const uint64_t* keep;
  int n, R, H, f;
  float alpha;                           // LeakyReLU slope
  unsigned head0;                        // layer * H: first head of this layer in the dropout key
  unsigned drop_seed, drop_thresh;
  float drop_scale;
  int drop;
};

// LDS image of one graph (dynamic shared memory, the same layout in both kernels):
//   rb[R][W] refined bit rows: edge (i,j) <=> bit && (keep_i || keep_j) && (vals == NULL || vals[i][j] > 0)   (wrapper.py:39)
//   cb[R][W] the same pattern transposed (backward only), over the rows that have at least one edge
//   per (node, head): s1, s2 (score halves), mx, rs (softmax max and 1 / sum), rr, ds1, ds2 (backward)
//   iso[R] row has no edge: the reference's -9e15 fill makes it uniform, 1/L over all L nodes
struct GatLds {
  unsigned long long *rb, *cb;
  float *s1, *s2, *mx, *rs, *rr, *ds1, *ds2, *colv;
  unsigned char* iso;
};

__host__ __device__ inline size_t gat_lds_bytes(int R, int H, int ncol) {
  const int W = (R + 63) / 64;
  return (size_t)2 * R * W * 8 + (size_t)7 * R * H * 4 + (size_t)ncol * 4 + (size_t)R;
}

__device__ inline GatLds gat_lds(unsigned char* base, int R, int H, int ncol) {
  const int W = (R + 63) / 64;
  GatLds L;
  L.rb = reinterpret_cast<unsigned long long*>(base);
  L.cb = L.rb + R * W;
  float* p = reinterpret_cast<float*>(L.cb + R * W);
  L.s1 = p; L.s2 = p + R * H; L.mx = p + 2 * R * H; L.rs = p + 3 * R * H; L.rr = p + 4 * R * H;
  L.ds1 = p + 5 * R * H; L.ds2 = p + 6 * R * H; L.colv = p + 7 * R * H;
  L.iso = reinterpret_cast<unsigned char*>(L.colv + ncol);
  return L;
}

__device__ inline void gat_load_rows(const GatArgs& A, int g, const GatLds& L) {
  const int R = A.R, W = (R + 63) >> 6;
  for (int t = threadIdx.x; t < R * W; t += blockDim.x) {
    const int i = t / W, w = t - i * W;
    unsigned long long word = A.bits[((size_t)g * R + i) * W + w];
    if (A.keep) {
      const bool ki = (A.keep[(size_t)g * W + (i >> 6)] >> (i & 63)) & 1ull;
      if (!ki) word &= A.keep[(size_t)g * W + w];
    }
    if (w == W - 1 && (R & 63)) word &= (1ull << (R & 63)) - 1ull;
    if (A.vals) {        // dense input: the reference masks with adj > 0, the packed pattern is adj != 0 (and its transpose)
      const float* vr = A.vals + ((size_t)g * R + i) * R + w * 64;
      unsigned long long b = word;
      while (b) {
        const int k = __builtin_ctzll(b);
        b &= b - 1ull;
        if (!(vr[k] > 0.f)) word &= ~(1ull << k);
      }
    }
    L.rb[i * W + w] = word;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    unsigned long long any = 0ull;
    for (int w = 0; w < W; ++w) any |= L.rb[i * W + w];
    L.iso[i] = any == 0ull;
  }
  __syncthreads();
}

// weight of entry (i,j) of head hd after softmax and dropout; *z = the LeakyReLU input (backward)
__device__ __forceinline__ float gat_weight(const GatArgs& A, const GatLds& L, int g, int i, int j, int hd, float* z) {
  const int t = i * A.H + hd;
  const float zz = L.s1[t] + L.s2[j * A.H + hd];
  const float e = zz > 0.f ? zz : A.alpha * zz;
  float p = expf(e - L.mx[t]) * L.rs[t];
  if (A.drop) {
    const unsigned idx = (((A.head0 + (unsigned)hd) * (unsigned)A.n + (unsigned)g) * (unsigned)A.R + (unsigned)i) * (unsigned)A.R + (unsigned)j;
    p = drop_hash(A.drop_seed, idx) >= A.drop_thresh ? p * A.drop_scale : 0.f;
  }
  *z = zz;
  return p;
}

// uniform row (no edge): 1/L, dropout applied as to any other entry
__device__ __forceinline__ float gat_uniform(const GatArgs& A, int g, int i, int j, int hd) {
  float p = 1.f / (float)A.R;
  if (A.drop) {
    const unsigned idx = (((A.head0 + (unsigned)hd) * (unsigned)A.n + (unsigned)g) * (unsigned)A.R + (unsigned)i) * (unsigned)A.R + (unsigned)j;
    p = drop_hash(A.drop_seed, idx) >= A.drop_thresh ? p * A.drop_scale : 0.f;
  }
  return p;
}

template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

// Scores, softmax statistics of every (row, head), scores and statistics saved for the backward.
__device__ inline void gat_scores_stats(const GatArgs& A, const GatLds& L, int g, const float* __restrict__ h,
                                        const float* __restrict__ a, float* __restrict__ s_out, float* __restrict__ stats) {
  const int R = A.R, H = A.H, f = A.f, F = H * f, W = (R + 63) >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float* hg = h + (size_t)g * R * F;
  for (int t = wave; t < R * H; t += nw) {                // s1 = h . a[:f], s2 = h . a[f:]  (wrapper.py:57-60)
    const int i = t / H, hd = t - i * H;
    const float* hr = hg + (size_t)i * F + (size_t)hd * f;
    const float* ar = a + (size_t)hd * 2 * f;
    float p1 = 0.f, p2 = 0.f;
    for (int c = lane; c < f; c += 64) {
      const float v = hr[c];
      p1 += v * ar[c];
      p2 += v * ar[f + c];
    }
    p1 = wave_sum(p1);
    p2 = wave_sum(p2);
    if (lane == 0) {
      L.s1[t] = p1;
      L.s2[t] = p2;
      s_out[((size_t)g * R * H + t) * 2] = p1;
      s_out[((size_t)g * R * H + t) * 2 + 1] = p2;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < R * H; t += blockDim.x) {
    const int i = t / H, hd = t - i * H;
    float m = 0.f, r = 1.f / (float)R;
    if (!L.iso[i]) {
      const float a1 = L.s1[t];
      m = -INFINITY;
      for (int w = 0; w < W; ++w) {
        unsigned long long b = L.rb[i * W + w];
        while (b) {
          const int j = w * 64 + __builtin_ctzll(b);
          b &= b - 1ull;
          const float z = a1 + L.s2[j * H + hd];
          m = fmaxf(m, z > 0.f ? z : A.alpha * z);
        }
      }
      float sum = 0.f;
      for (int w = 0; w < W; ++w) {
        unsigned long long b = L.rb[i * W + w];
        while (b) {
          const int j = w * 64 + __builtin_ctzll(b);
          b &= b - 1ull;
          const float z = a1 + L.s2[j * H + hd];
          sum += expf((z > 0.f ? z : A.alpha * z) - m);
        }
      }
      r = 1.f / sum;
    }
    L.mx[t] = m;
    L.rs[t] = r;
    stats[((size_t)g * R * H + t) * 2] = m;
    stats[((size_t)g * R * H + t) * 2 + 1] = r;
  }
  __syncthreads();
}

// sum_j P_ij h_j[col..col+V) of head hd (row i has edges, or a uniform row in training mode)
template <int V>
__device__ __forceinline__ void gat_row_sum(const GatArgs& A, const GatLds& L, int g, const float* __restrict__ hg, int i,
                                            int hd, int col, float (&acc)[V]) {
  const int R = A.R, W = (R + 63) >> 6, F = A.H * A.f;
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  if (!L.iso[i]) {
    for (int w = 0; w < W; ++w) {
      unsigned long long b = L.rb[i * W + w];
      while (b) {
        const int j = w * 64 + __builtin_ctzll(b);
        b &= b - 1ull;
        float z;
        const float p = gat_weight(A, L, g, i, j, hd, &z);
        float x[V];
        ldv<V>(hg + (size_t)j * F + col, x);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += p * x[v];
      }
    }
  } else {
    for (int j = 0; j < R; ++j) {
      const float p = gat_uniform(A, g, i, j, hd);
      float x[V];
      ldv<V>(hg + (size_t)j * F + col, x);
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] += p * x[v];
    }
  }
}

__device__ __forceinline__ float elu_(float x) { return x > 0.f ? x : expm1f(x); }

// Forward of one GAT layer's heads on one graph per workgroup (wrapper.py:27-53, 99-108).
// h [n*R][H*f] projected features (head-major columns); hp [n*R][H*f] the aggregated features before the activation;
// mode 1: out [n*R][H*f] = elu(hp) (hidden layer, heads concatenated); mode 2: out = hp (a lone concat=False layer);
// mode 0 (the GAT's output layer): out [n*R][f] = relu(sum_hd hp_hd / R).
template <int V>
__global__ void __launch_bounds__(256)
gat_aggregate_fwd_kernel(GatArgs A, const float* __restrict__ h, const float* __restrict__ a, int mode,
                         float* __restrict__ s_out, float* __restrict__ stats, float* __restrict__ hp, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int g = blockIdx.x, R = A.R, H = A.H, f = A.f, F = H * f;
  const GatLds L = gat_lds(dsm, R, H, 0);
  const float* hg = h + (size_t)g * R * F;
  const bool concat = mode != 0, elu = mode == 1;
  gat_load_rows(A, g, L);
  gat_scores_stats(A, L, g, h, a, s_out, stats);
  const int ncv = (concat ? F : f) / V;
  for (int it = threadIdx.x; it < R * ncv; it += blockDim.x) {
    const int i = it / ncv, c = (it - i * ncv) * V;
    if (L.iso[i] && !A.drop) continue;                   // evaluation mode: the uniform rows all hold the graph mean (below)
    const size_t row = (size_t)g * R + i;
    if (concat) {
      float acc[V], o[V];
      gat_row_sum<V>(A, L, g, hg, i, c / f, c, acc);
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = elu ? elu_(acc[v]) : acc[v];
      stv<V>(hp + row * F + c, acc);
      stv<V>(out + row * F + c, o);
    } else {
      float y[V];
#pragma unroll
      for (int v = 0; v < V; ++v) y[v] = 0.f;
      for (int hd = 0; hd < H; ++hd) {
        float acc[V];
        gat_row_sum<V>(A, L, g, hg, i, hd, hd * f + c, acc);
        stv<V>(hp + row * F + hd * f + c, acc);
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] += acc[v];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) { y[v] = y[v] / (float)R; y[v] = y[v] > 0.f ? y[v] : 0.f; }
      stv<V>(out + row * f + c, y);
    }
  }
  if (A.drop) return;
  // evaluation mode: every uniform row is sum_j h_j / L -- computed once per column, stored to each such row
  int any = 0;
  for (int i = 0; i < R; ++i) any |= L.iso[i];
  if (!any) return;
  for (int it = threadIdx.x; it < ncv; it += blockDim.x) {
    const int c = it * V;
    float y[V];
#pragma unroll
    for (int v = 0; v < V; ++v) y[v] = 0.f;
    for (int hd = 0; hd < (concat ? 1 : H); ++hd) {
      const int col = concat ? c : hd * f + c;
      float acc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = 0.f;
      const float p = 1.f / (float)R;
      for (int j = 0; j < R; ++j) {
        float x[V];
        ldv<V>(hg + (size_t)j * F + col, x);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += p * x[v];
      }
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) { o[v] = elu ? elu_(acc[v]) : acc[v]; y[v] += acc[v]; }
      for (int i = 0; i < R; ++i) {
        if (!L.iso[i]) continue;
        const size_t row = (size_t)g * R + i;
        stv<V>(hp + row * F + col, acc);
        if (concat) stv<V>(out + row * F + col, o);
      }
    }
    if (!concat) {
#pragma unroll
      for (int v = 0; v < V; ++v) { y[v] = y[v] / (float)R; y[v] = y[v] > 0.f ? y[v] : 0.f; }
      for (int i = 0; i < R; ++i)
        if (L.iso[i]) stv<V>(out + ((size_t)g * R + i) * f + c, y);
    }
  }
}

// gradient w.r.t. hp of head hd at row i, column c of the head (the activation's backward: elu, none, or relu then / L)
__device__ __forceinline__ float gat_dpre(const GatArgs& A, int mode, int g, int i, int hd, int c, const float* __restrict__ hp,
                                          const float* __restrict__ out, const float* __restrict__ gy) {
  const size_t row = (size_t)g * A.R + i;
  if (mode != 0) {
    const size_t o = row * A.H * A.f + (size_t)hd * A.f + c;
    const float x = hp[o], gv = gy[o];
    return (mode == 2 || x > 0.f) ? gv : gv * expf(x);
  }
  const size_t o = row * A.f + c;
  return out[o] > 0.f ? gy[o] / (float)A.R : 0.f;
}

// Backward of gat_aggregate_fwd_kernel, one graph per workgroup.  With P = dropout(softmax(e)) and dpre = the
// activation's backward, per head:
//   dh_j  = sum_i P_ij dpre_i + ds1_j a1 + ds2_j a2            (P^T g: transposed walk over the columns' bit rows)
//   dz_ij = P~_ij (mask_ij scale dpre_i . h_j - r_i) * leaky'(z_ij),   r_i = dpre_i . hp_i = sum_k P_ik dpre_i . h_k
//   ds1_i = sum_j dz_ij (row walk), ds2_j = sum_i dz_ij (column walk: LDS, a fixed order, no atomics)
//   da_part[g][hd] = (sum_i ds1_i h_i, sum_j ds2_j h_j)   -- reduced over the graphs by gat_da_reduce_kernel
// Uniform rows carry no gradient into the scores (their entries are the constant fill).
template <int V>
__global__ void __launch_bounds__(256)
gat_aggregate_bwd_kernel(GatArgs A, const float* __restrict__ h, const float* __restrict__ a, int mode,
                         const float* __restrict__ s_in, const float* __restrict__ stats, const float* __restrict__ hp,
                         const float* __restrict__ out, const float* __restrict__ gy, float* __restrict__ dh,
                         float* __restrict__ da_part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int g = blockIdx.x, R = A.R, H = A.H, f = A.f, F = H * f, W = (R + 63) >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const GatLds L = gat_lds(dsm, R, H, F);
  const float* hg = h + (size_t)g * R * F;
  gat_load_rows(A, g, L);
  for (int t = threadIdx.x; t < R * H; t += blockDim.x) {
    const size_t o = ((size_t)g * R * H + t) * 2;
    L.s1[t] = s_in[o];
    L.s2[t] = s_in[o + 1];
    L.mx[t] = stats[o];
    L.rs[t] = stats[o + 1];
  }
  for (int t = threadIdx.x; t < R * W; t += blockDim.x) {   // transposed pattern of the rows that have edges
    const int j = t / W, w = t - j * W;
    unsigned long long word = 0ull;
    for (int k = 0; k < 64; ++k) {
      const int i = w * 64 + k;
      if (i < R && !L.iso[i] && ((L.rb[i * W + (j >> 6)] >> (j & 63)) & 1ull)) word |= 1ull << k;
    }
    L.cb[j * W + w] = word;
  }
  __syncthreads();
  const int kq = (f + 63) / 64;
  // row walk: r_i and ds1_i, one wave per (row, head)
  for (int t = wave; t < R * H; t += nw) {
    const int i = t / H, hd = t - i * H;
    if (L.iso[i]) {
      if (lane == 0) { L.rr[t] = 0.f; L.ds1[t] = 0.f; }
      continue;
    }
    float dp[GAT_KF];
    float rpart = 0.f;
#pragma unroll
    for (int q = 0; q < GAT_KF; ++q) {
      const int c = lane + 64 * q;
      dp[q] = 0.f;
      if (q < kq && c < f) {
        dp[q] = gat_dpre(A, mode, g, i, hd, c, hp, out, gy);
        rpart += dp[q] * hp[((size_t)g * R + i) * F + (size_t)hd * f + c];
      }
    }
    const float ri = wave_sum(rpart);
    float ds = 0.f;
    for (int w = 0; w < W; ++w) {
      unsigned long long b = L.rb[i * W + w];
      while (b) {
        const int j = w * 64 + __builtin_ctzll(b);
        b &= b - 1ull;
        const float* hr = hg + (size_t)j * F + (size_t)hd * f;
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < GAT_KF; ++q) {
          const int c = lane + 64 * q;
          if (q < kq && c < f) part += dp[q] * hr[c];
        }
        const float dot = wave_sum(part);
        float z;
        const float p = gat_weight(A, L, g, i, j, hd, &z);              // P = P~ * mask * scale
        const float pt = expf((z > 0.f ? z : A.alpha * z) - L.mx[t]) * L.rs[t];
        const float ks = pt > 0.f ? p / pt : 0.f;                        // mask * scale (exact: scale or 0)
        float dz = pt * (ks * dot - ri);
        ds += z > 0.f ? dz : A.alpha * dz;
      }
    }
    if (lane == 0) { L.rr[t] = ri; L.ds1[t] = ds; }
  }
  __syncthreads();
  // column walk: ds2_j, one wave per (column, head), rows in ascending order
  for (int t = wave; t < R * H; t += nw) {
    const int j = t / H, hd = t - j * H;
    float hj[GAT_KF];
#pragma unroll
    for (int q = 0; q < GAT_KF; ++q) {
      const int c = lane + 64 * q;
      hj[q] = (q < kq && c < f) ? hg[(size_t)j * F + (size_t)hd * f + c] : 0.f;
    }
    float ds = 0.f;
    for (int w = 0; w < W; ++w) {
      unsigned long long b = L.cb[j * W + w];
      while (b) {
        const int i = w * 64 + __builtin_ctzll(b);
        b &= b - 1ull;
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < GAT_KF; ++q) {
          const int c = lane + 64 * q;
          if (q < kq && c < f) part += gat_dpre(A, mode, g, i, hd, c, hp, out, gy) * hj[q];
        }
        const float dot = wave_sum(part);
        const int ti = i * H + hd;
        float z;
        const float p = gat_weight(A, L, g, i, j, hd, &z);
        const float pt = expf((z > 0.f ? z : A.alpha * z) - L.mx[ti]) * L.rs[ti];
        const float ks = pt > 0.f ? p / pt : 0.f;
        float dz = pt * (ks * dot - L.rr[ti]);
        ds += z > 0.f ? dz : A.alpha * dz;
      }
    }
    if (lane == 0) L.ds2[t] = ds;
  }
  // evaluation mode: the uniform rows' share of P^T g is (1/L) sum_{uniform i} dpre_i, the same for every column j
  if (!A.drop) {
    for (int col = threadIdx.x; col < F; col += blockDim.x) {
      const int hd = col / f, c = col - hd * f;
      float s = 0.f;
      for (int i = 0; i < R; ++i)
        if (L.iso[i]) s += gat_dpre(A, mode, g, i, hd, c, hp, out, gy);
      L.colv[col] = s;
    }
  }
  __syncthreads();
  // dh
  for (int it = threadIdx.x; it < R * F; it += blockDim.x) {
    const int j = it / F, col = it - j * F, hd = col / f, c = col - hd * f;
    float acc = 0.f;
    for (int w = 0; w < W; ++w) {
      unsigned long long b = L.cb[j * W + w];
      while (b) {
        const int i = w * 64 + __builtin_ctzll(b);
        b &= b - 1ull;
        float z;
        acc += gat_weight(A, L, g, i, j, hd, &z) * gat_dpre(A, mode, g, i, hd, c, hp, out, gy);
      }
    }
    if (A.drop) {
      for (int i = 0; i < R; ++i)
        if (L.iso[i]) acc += gat_uniform(A, g, i, j, hd) * gat_dpre(A, mode, g, i, hd, c, hp, out, gy);
    } else {
      acc += L.colv[col] * (1.f / (float)R);
    }
    const float* ar = a + (size_t)hd * 2 * f;
    acc += L.ds1[j * H + hd] * ar[c] + L.ds2[j * H + hd] * ar[f + c];
    dh[((size_t)g * R + j) * F + col] = acc;
  }
  // this graph's share of da
  for (int col = threadIdx.x; col < F; col += blockDim.x) {
    const int hd = col / f, c = col - hd * f;
    float a1 = 0.f, a2 = 0.f;
    for (int i = 0; i < R; ++i) {
      const float x = hg[(size_t)i * F + col];
      a1 += L.ds1[i * H + hd] * x;
      a2 += L.ds2[i * H + hd] * x;
    }
    float* dp = da_part + ((size_t)g * H + hd) * 2 * f;
    dp[c] = a1;
    dp[f + c] = a2;
  }
}

// da[k] += sum_g part[g][k], k < K: 16 columns x 16 graph groups per workgroup, partial sums combined in a fixed order
__global__ void __launch_bounds__(256) gat_da_reduce_kernel(const float* __restrict__ part, float* __restrict__ da, int n, int K) {
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (k < K)
    for (int g = grp; g < n; g += 16) s += part[(size_t)g * K + k];
  red[grp][cl] = s;
  __syncthreads();
  if (grp == 0 && k < K) {
    float t = 0.f;
    for (int q = 0; q < 16; ++q) t += red[q][cl];
    da[k] += t;
  }
}

// Â = D^-1/2 A D^-1/2 with D the row sums of the adjacency VALUES (wrapper.py:125-135), as a per-row scale; one thread per row
__global__ void __launch_bounds__(256)
gcn_norm_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
                const uint64_t* __restrict__ keep, int n, int R, float* __restrict__ scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)n * R) return;
  const int g = (int)(idx / R), i = (int)(idx - (long long)g * R), W = (R + 63) >> 6;
  bool ki = true;
  if (keep) ki = (keep[(size_t)g * W + (i >> 6)] >> (i & 63)) & 1ull;
  float sum = 0.f;
  for (int w = 0; w < W; ++w) {
    unsigned long long b = bits[((size_t)g * R + i) * W + w];
    if (!ki) b &= keep[(size_t)g * W + w];
    if (w == W - 1 && (R & 63)) b &= (1ull << (R & 63)) - 1ull;
    while (b) {
      const int j = w * 64 + __builtin_ctzll(b);
      b &= b - 1ull;
      sum += vals ? vals[((size_t)g * R + i) * R + j] : dinv[(size_t)g * R + j];
    }
  }
  const float rowsum = vals ? sum : dinv[(size_t)g * R + i] * sum;
  const float s = rowsum == 0.f ? 0.f : 1.f / sqrtf(rowsum);           // pow(-0.5) with inf -> 0
  scale[idx] = vals ? s : dinv[(size_t)g * R + i] * s;
}

__global__ void __launch_bounds__(256)
feat_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long long count, unsigned seed, unsigned thresh, float scale) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (long long)gridDim.x * blockDim.x)
    y[e] = drop_hash(seed, (unsigned)e) >= thresh ? x[e] * scale : 0.f;
}

__global__ void __launch_bounds__(256)
scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ mask, float* __restrict__ y,
                  long long count, int cols) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (long long)gridDim.x * blockDim.x) {
    float v = x[e];
    if (s) v *= s[e / cols];
    if (mask && !(mask[e] > 0.f)) v = 0.f;
    y[e] = v;
  }
}

unsigned drop_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

int gat_check(int n, int r, int din, int heads, int f, int mode, int layer, float drop_p) {
  GH_REQUIRE(n > 0 && r > 0 && r <= GAT_MAX_R, "gat: graphs of r=%d nodes (supported: 1..%d), n=%d", r, GAT_MAX_R, n);
  GH_REQUIRE(heads >= 1 && heads <= GAT_MAX_H, "gat: %d heads (supported: 1..%d)", heads, GAT_MAX_H);
  GH_REQUIRE(f >= 1 && f <= GAT_MAX_F && din >= 1, "gat: head width %d (supported: 1..%d), input width %d", f, GAT_MAX_F, din);
  GH_REQUIRE(mode >= 0 && mode <= 2, "gat: mode %d not in {0: output layer, 1: elu, 2: no activation}", mode);
  GH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "gat: dropout p=%f not in [0,1)", drop_p);
  GH_REQUIRE(layer >= 0, "gat: layer %d < 0", layer);
  GH_REQUIRE(drop_p <= 0.f || (unsigned long long)(layer + 1) * heads * n * (unsigned long long)r * r < (1ull << 32),
             "gat: the attention dropout key (layer, head, graph, i, j) exceeds 32 bits");
  GH_REQUIRE((long long)n * r * heads * (long long)f < (1ll << 31), "gat: %d x %d rows of %d columns exceed 2^31 elements", n, r, heads * f);
  return 0;
}

GatArgs gat_args(const uint64_t* bits, const float* vals, const uint64_t* keep, int n, int r, int heads, int f, float alpha,
                 int layer, float drop_p, uint32_t drop_seed) {
  GatArgs A;
  A.bits = bits; A.vals = vals; A.keep = keep;
  A.n = n; A.R = r; A.H = heads; A.f = f; A.alpha = alpha;
  A.head0 = (unsigned)(layer * heads);
  A.drop = drop_p > 0.f;
  A.drop_seed = drop_seed;
  A.drop_thresh = drop_threshold(drop_p);
  A.drop_scale = A.drop ? 1.f / (1.f - drop_p) : 1.f;
  return A;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_gat_layer_fwd(const uint64_t* bits, const float* vals, const uint64_t* keep, const float* x, const float* w_lin,
                                const float* a, int n, int r, int din, int heads, int f, float alpha, int mode, int layer,
                                float drop_p, uint32_t drop_seed, float* h, float* s, float* stats, float* hp, float* out,
                                gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gat_check(n, r, din, heads, f, mode, layer, drop_p)) return rc;
  GH_REQUIRE(bits && x && w_lin && a && h && s && stats && hp && out, "gat_layer_fwd: NULL argument");
  const int F = heads * f, m = n * r;
  // all heads' projections in one GEMM: h = x W_cat, W_cat = [W_0 | W_1 | ...] handed over transposed ([F][din])
  if (int rc = gh_linear_fwd(x, w_lin, nullptr, h, m, din, F, stream)) return rc;
  const GatArgs A = gat_args(bits, vals, keep, n, r, heads, f, alpha, layer, drop_p, drop_seed);
  const size_t lds = gat_lds_bytes(r, heads, 0);
  const bool v4 = f % 4 == 0 && aligned16(h) && aligned16(hp) && aligned16(out);
  if (v4) {
    if (int rc = lds_opt_in((const void*)gat_aggregate_fwd_kernel<4>, lds, "gat_layer_fwd")) return rc;
    hipLaunchKernelGGL(gat_aggregate_fwd_kernel<4>, dim3(n), dim3(256), lds, st, A, h, a, mode, s, stats, hp, out);
  } else {
    if (int rc = lds_opt_in((const void*)gat_aggregate_fwd_kernel<1>, lds, "gat_layer_fwd")) return rc;
    hipLaunchKernelGGL(gat_aggregate_fwd_kernel<1>, dim3(n), dim3(256), lds, st, A, h, a, mode, s, stats, hp, out);
  }
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_gat_layer_bwd(const uint64_t* bits, const float* vals, const uint64_t* keep, const float* x, const float* w_cat,
                                const float* a, int n, int r, int din, int heads, int f, float alpha, int mode, int layer,
                                float drop_p, uint32_t drop_seed, const float* h, const float* s, const float* stats,
                                const float* hp, const float* out, const float* g, float* dh, float* da_part, float* dx,
                                float* dw_cat, float* da, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gat_check(n, r, din, heads, f, mode, layer, drop_p)) return rc;
  GH_REQUIRE(bits && x && a && h && s && stats && hp && out && g && dh && da_part && dw_cat && da,
             "gat_layer_bwd: NULL argument");
  GH_REQUIRE(dx == nullptr || w_cat != nullptr, "gat_layer_bwd: dx needs w_cat");
  const int F = heads * f, m = n * r;
  const GatArgs A = gat_args(bits, vals, keep, n, r, heads, f, alpha, layer, drop_p, drop_seed);
  const size_t lds = gat_lds_bytes(r, heads, F);
  if (int rc = lds_opt_in((const void*)gat_aggregate_bwd_kernel<1>, lds, "gat_layer_bwd")) return rc;
  hipLaunchKernelGGL(gat_aggregate_bwd_kernel<1>, dim3(n), dim3(256), lds, st, A, h, a, mode, s, stats, hp, out, g, dh, da_part);
  GH_LAUNCH_CHECK();
  const int K = heads * 2 * f;
  hipLaunchKernelGGL(gat_da_reduce_kernel, dim3((K + 15) / 16), dim3(256), 0, st, da_part, da, n, K);
  GH_LAUNCH_CHECK();
  // dx = dh W_cat^T; dW_cat += x^T dh (the TN GEMM with x and dh as its "g" and "x": dw[din][F])
  if (dx)
    if (int rc = gh_linear_bwd(nullptr, w_cat, nullptr, dh, m, din, F, dx, nullptr, nullptr, stream)) return rc;
  return gh_linear_bwd(dh, nullptr, nullptr, x, m, F, din, nullptr, dw_cat, nullptr, stream);
}

extern "C" int gh_gcn_norm(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep, int n, int r,
                           float* scale, gh_stream_t stream) {
  GH_REQUIRE(n > 0 && r > 0 && r <= GAT_MAX_R, "gcn_norm: graphs of r=%d nodes (supported: 1..%d)", r, GAT_MAX_R);
  GH_REQUIRE(bits && scale && (vals || dinv), "gcn_norm: need bits, scale and dinv or vals");
  const long long rows = (long long)n * r;
  hipLaunchKernelGGL(gcn_norm_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, dinv, vals, keep,
                     n, r, scale);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_feat_dropout(const float* x, float* y, int rows, int cols, float p, uint32_t seed, gh_stream_t stream) {
  GH_REQUIRE(rows > 0 && cols > 0 && x && y, "feat_dropout: bad arguments");
  GH_REQUIRE(p >= 0.f && p < 1.f, "feat_dropout: p=%f not in [0,1)", p);
  const long long count = (long long)rows * cols;
  GH_REQUIRE(count < (1ll << 32), "feat_dropout: %lld elements exceed the mask's 32-bit element index", count);
  const long long blocks = (count + 255) / 256;
  hipLaunchKernelGGL(feat_dropout_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     x, y, count, seed, drop_threshold(p), 1.f / (1.f - p));
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_scale_rows(const float* x, const float* scale, const float* mask, float* y, int rows, int cols,
                             gh_stream_t stream) {
  GH_REQUIRE(rows > 0 && cols > 0 && x && y, "scale_rows: bad arguments");
  const long long count = (long long)rows * cols;
  const long long blocks = (count + 255) / 256;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     x, scale, mask, y, count, cols);
  GH_LAUNCH_CHECK();
  return 0;
}
