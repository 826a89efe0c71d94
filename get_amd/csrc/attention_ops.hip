// The single-query attention ablations of thirdparty/two_branches_attention.py (Dot :9-38, BiLinear :41-70, BiLinearTanh
// :151-191) and thirdparty/self_attention.py (SelfAttentionICLR2017 :13-48, MultiHeadSelfAttentionICLR17OnWord :103-153):
//   gh_query_att_*  attention scored by a query vector, weighted sum of the scored tensor
//   gh_tanh_att_*   additive (tanh) attention with a bias on the hoisted branch and a weighted sum over a SEPARATE tensor
// One workgroup of four waves owns one sequence, so every reduction over l and over the feature axis stays inside it; the
// large operands (right; pre / t and values) are read from HBM once per direction and padded positions are never read.
// No floating-point atomics: the waves of a workgroup are merged through LDS in wave order, dW2 goes through per-sequence
// partials on the stream workspace and a fixed-order second stage.  The projections in front of these kernels run on the
// library's GEMMs (gh_linear_fwd / gh_linear_bwd).
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include <math.h>

namespace gh {
namespace {

constexpr int ATT_THREADS = 256;
constexpr int ATT_WAVES = ATT_THREADS / 64;
constexpr int QATT_MAX_L = 4096;         // raw scores of one sequence in LDS
constexpr int QATT_MAX_D = 2048;         // one row of `right` in a wave's registers (8 x float4 per lane)
constexpr int TATT_MAX_HEADS = 8;
constexpr int TATT_MAX_LH = 8192;        // l * heads scores of one sequence in LDS (32 KB)

// V consecutive floats of a row: V = 4 moves 16 bytes per lane (width % 4 == 0, 16-byte aligned operands), V = 1 is the
// scalar path for every other shape
template <int V> struct Pk { float v[V]; };
template <int V> __device__ __forceinline__ Pk<V> pk_zero() {
  Pk<V> r;
#pragma unroll
  for (int j = 0; j < V; ++j) r.v[j] = 0.f;
  return r;
}
template <int V> __device__ __forceinline__ Pk<V> pk_ld(const float* p) {
  Pk<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V> __device__ __forceinline__ void pk_st(float* p, const Pk<V>& a) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  else *p = a.v[0];
}
template <int V> __device__ __forceinline__ float pk_dot(const Pk<V>& a, const Pk<V>& b, float acc) {
#pragma unroll
  for (int j = 0; j < V; ++j) acc = fmaf(a.v[j], b.v[j], acc);
  return acc;
}

__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

// ============================================================================ query-vector attention
// Forward (two_branches_attention.py:29-37 / :61-69).  Wave w takes rows w, w + 4, ... of the sequence with an online
// softmax: a lane keeps its K x V columns of q and of the running weighted sum in registers, so a row of `right` is read
// once and used for its score and for the sum.  The four (max, sum, partial avg) triples are merged through LDS.
// LDS: sc[pad4(l)] raw scores | wm[8] wave maxima and sums | wacc[ATT_WAVES][d]
template <int V, int K>
__global__ void __launch_bounds__(ATT_THREADS)
query_att_fwd_kernel(const float* __restrict__ q, const float* __restrict__ right, const float* __restrict__ mask, int l,
                     int d, float* __restrict__ weights, float* __restrict__ avg) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sc = sm;
  float* wm = sm + pad4(l);
  float* wacc = wm + 2 * ATT_WAVES;
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, nu = d / V;
  const float* qb = q + (size_t)b * d;
  const float* rb = right + (size_t)b * l * d;
  const float* mb = mask + (size_t)b * l;
  Pk<V> qv[K], acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = lane + 64 * k;
    qv[k] = u < nu ? pk_ld<V>(qb + (size_t)u * V) : pk_zero<V>();
    acc[k] = pk_zero<V>();
  }
  float m = -INFINITY, sum = 0.f;
  // the wave's next unmasked row is in flight while the current one is reduced; padding rows are never read
  auto next_row = [&](int i) {
    while (i < l && mb[i] == 0.f) i += ATT_WAVES;
    return i;
  };
  auto load_row = [&](int i, Pk<V>* r) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int u = lane + 64 * k;
      r[k] = (i < l && u < nu) ? pk_ld<V>(rb + (size_t)i * d + (size_t)u * V) : pk_zero<V>();
    }
  };
  Pk<V> r[K], rn[K];
  int i = next_row(w);
  load_row(i, r);
  while (i < l) {
    const int nx = next_row(i + ATT_WAVES);
    load_row(nx, rn);
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) p = pk_dot<V>(r[k], qv[k], p);
    const float s = wave_sum(p);
    if (lane == 0) sc[i] = s;
    const float mn = fmaxf(m, s);
    const float f = expf(m - mn), e = expf(s - mn);   // m = -inf on the wave's first row: f = 0
    m = mn;
    sum = sum * f + e;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[k].v[j] = fmaf(acc[k].v[j], f, e * r[k].v[j]);
      r[k] = rn[k];
    }
    i = nx;
  }
  if (lane == 0) { wm[w] = m; wm[ATT_WAVES + w] = sum; }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = lane + 64 * k;
    if (u < nu) pk_st<V>(wacc + (size_t)w * d + (size_t)u * V, acc[k]);
  }
  __syncthreads();
  float M = -INFINITY;
#pragma unroll
  for (int ww = 0; ww < ATT_WAVES; ++ww) M = fmaxf(M, wm[ww]);
  float fw[ATT_WAVES], S = 0.f;
#pragma unroll
  for (int ww = 0; ww < ATT_WAVES; ++ww) {
    fw[ww] = wm[ww] == -INFINITY ? 0.f : expf(wm[ww] - M);
    S += wm[ATT_WAVES + ww] * fw[ww];
  }
  const bool none = !(M > -INFINITY);                // every position masked: the reference's softmax of all -inf is NaN
  const float inv = 1.f / S, nanv = __builtin_nanf("");
  for (int c = threadIdx.x; c < d; c += ATT_THREADS) {
    float a = 0.f;
#pragma unroll
    for (int ww = 0; ww < ATT_WAVES; ++ww) a = fmaf(wacc[(size_t)ww * d + c], fw[ww], a);
    avg[(size_t)b * d + c] = none ? nanv : a * inv;
  }
  for (int i = threadIdx.x; i < l; i += ATT_THREADS)
    weights[(size_t)b * l + i] = none ? nanv : (mb[i] == 0.f ? 0.f : expf(sc[i] - M) * inv);
}

// Backward.  dw_l = g_w_l + g_avg . right_l, c = sum_j w_j dw_j, ds_l = w_l (dw_l - c):
//   dright_l = w_l g_avg + ds_l q      needs only the scalars dw_l and c, not the row
//   dq = sum_l ds_l right_l = sum_l (w_l dw_l) right_l - c sum_l w_l right_l
// so one pass over `right` (rows of weight 0 skipped) yields dw_l and both sums, and a second pass writes dright from
// registers and LDS: right is read once, dright written once, every row of it (exact zeros where the weight is 0).
// LDS: dwl[pad4(l)] | red[8] | wacc[ATT_WAVES][d]
template <int V, int K>
__global__ void __launch_bounds__(ATT_THREADS)
query_att_bwd_kernel(const float* __restrict__ q, const float* __restrict__ right, const float* __restrict__ weights,
                     const float* __restrict__ g_avg, const float* __restrict__ g_w, int l, int d, float* __restrict__ dq,
                     float* __restrict__ dright) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dwl = sm;
  float* red = sm + pad4(l);
  float* wacc = red + 2 * ATT_WAVES;
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, nu = d / V;
  const float* rb = right + (size_t)b * l * d;
  const float* wb = weights + (size_t)b * l;
  Pk<V> qv[K], gv[K], sa[K], sv[K];                  // sa = sum (w dw) right, sv = sum w right
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = lane + 64 * k;
    qv[k] = u < nu ? pk_ld<V>(q + (size_t)b * d + (size_t)u * V) : pk_zero<V>();
    gv[k] = u < nu ? pk_ld<V>(g_avg + (size_t)b * d + (size_t)u * V) : pk_zero<V>();
    sa[k] = pk_zero<V>();
    sv[k] = pk_zero<V>();
  }
  float cpart = 0.f;
  auto next_row = [&](int i) {                       // rows of weight 0 (padding) are never read
    while (i < l && wb[i] == 0.f) i += ATT_WAVES;
    return i;
  };
  auto load_row = [&](int i, Pk<V>* r) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int u = lane + 64 * k;
      r[k] = (i < l && u < nu) ? pk_ld<V>(rb + (size_t)i * d + (size_t)u * V) : pk_zero<V>();
    }
  };
  Pk<V> r[K], rn[K];
  int i = next_row(w);
  load_row(i, r);
  while (i < l) {
    const int nx = next_row(i + ATT_WAVES);
    load_row(nx, rn);                                // in flight while row i is reduced
    const float wt = wb[i];
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) p = pk_dot<V>(r[k], gv[k], p);
    const float dw = wave_sum(p) + (g_w ? g_w[(size_t)b * l + i] : 0.f);
    if (lane == 0) dwl[i] = dw;
    const float wd = wt * dw;
    cpart += wd;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sa[k].v[j] = fmaf(wd, r[k].v[j], sa[k].v[j]);
        sv[k].v[j] = fmaf(wt, r[k].v[j], sv[k].v[j]);
      }
      r[k] = rn[k];
    }
    i = nx;
  }
  if (lane == 0) red[w] = cpart;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = lane + 64 * k;
    if (u < nu) pk_st<V>(wacc + (size_t)w * d + (size_t)u * V, sa[k]);
  }
  __syncthreads();
  float cc = 0.f;
#pragma unroll
  for (int ww = 0; ww < ATT_WAVES; ++ww) cc += red[ww];
  float ta[QATT_MAX_D / ATT_THREADS];
#pragma unroll
  for (int j = 0; j < QATT_MAX_D / ATT_THREADS; ++j) {
    const int c = threadIdx.x + ATT_THREADS * j;
    float a = 0.f;
    if (c < d)
#pragma unroll
      for (int ww = 0; ww < ATT_WAVES; ++ww) a += wacc[(size_t)ww * d + c];
    ta[j] = a;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = lane + 64 * k;
    if (u < nu) pk_st<V>(wacc + (size_t)w * d + (size_t)u * V, sv[k]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < QATT_MAX_D / ATT_THREADS; ++j) {
    const int c = threadIdx.x + ATT_THREADS * j;
    if (c < d) {
      float a = 0.f;
#pragma unroll
      for (int ww = 0; ww < ATT_WAVES; ++ww) a += wacc[(size_t)ww * d + c];
      dq[(size_t)b * d + c] = ta[j] - cc * a;
    }
  }
  float* db = dright + (size_t)b * l * d;
  for (int i = w; i < l; i += ATT_WAVES) {
    const float wt = wb[i];
    const float ds = wt == 0.f ? 0.f : wt * (dwl[i] - cc);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int u = lane + 64 * k;
      if (u >= nu) continue;
      Pk<V> o = pk_zero<V>();
      if (wt != 0.f)
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = fmaf(ds, qv[k].v[j], wt * gv[k].v[j]);
      pk_st<V>(db + (size_t)i * d + (size_t)u * V, o);
    }
  }
}

// ============================================================================ additive (tanh) attention
// Forward (two_branches_attention.py:181-190, self_attention.py:39-47 / :143-150).
//   phase 1  a wave per row: t = tanh(pre + u) (saved), e[c] = w2[c] . t per head -> LDS
//   phase 2  a wave per head: masked softmax over l in LDS, weights out
//   phase 3  column chunks of 64 lanes x V floats of `values`: wave w sums its rows w, w + 4, ... for all heads in
//            registers; waves 1..3 hand their sums to wave 0 through LDS, which adds them in wave order and stores
// Rows of weight 0 (padding) are never read; their t rows are not written.
// LDS: e[pad4(l * heads)] | macc[ATT_WAVES - 1][heads][64 * V]
template <int V>
__global__ void __launch_bounds__(ATT_THREADS)
tanh_att_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ u, const float* __restrict__ w2,
                    const float* __restrict__ mask, const float* __restrict__ values, int l, int ha, int heads, int dv,
                    float* __restrict__ t, float* __restrict__ weights, float* __restrict__ attended) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* e = sm;
  float* macc = sm + pad4(l * heads);
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* mb = mask + (size_t)b * l;
  const int nua = ha / V;
  for (int i = w; i < l; i += ATT_WAVES) {
    if (mb[i] == 0.f) continue;
    const size_t row = ((size_t)b * l + i) * ha;
    float p[TATT_MAX_HEADS];
#pragma unroll
    for (int c = 0; c < TATT_MAX_HEADS; ++c) p[c] = 0.f;
    for (int un = lane; un < nua; un += 64) {
      Pk<V> x = pk_ld<V>(pre + row + (size_t)un * V);
      if (u) {
        const Pk<V> uu = pk_ld<V>(u + (size_t)b * ha + (size_t)un * V);
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] += uu.v[j];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) x.v[j] = tanhf(x.v[j]);
      pk_st<V>(t + row + (size_t)un * V, x);
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) p[c] = pk_dot<V>(pk_ld<V>(w2 + (size_t)c * ha + (size_t)un * V), x, p[c]);
    }
#pragma unroll
    for (int c = 0; c < TATT_MAX_HEADS; ++c)
      if (c < heads) {
        const float s = wave_sum(p[c]);
        if (lane == 0) e[i * heads + c] = s;
      }
  }
  __syncthreads();
  const float nanv = __builtin_nanf("");
  for (int c = w; c < heads; c += ATT_WAVES) {
    float mx = -INFINITY;
    for (int i = lane; i < l; i += 64)
      if (mb[i] != 0.f) mx = fmaxf(mx, e[i * heads + c]);
    mx = wave_max(mx);
    const bool none = !(mx > -INFINITY);             // all masked: NaN weights, as the reference's softmax of all -inf
    float s = 0.f;
    for (int i = lane; i < l; i += 64)
      if (mb[i] != 0.f) s += expf(e[i * heads + c] - mx);
    const float inv = 1.f / wave_sum(s);
    for (int i = lane; i < l; i += 64) {
      const float wt = none ? nanv : (mb[i] != 0.f ? expf(e[i * heads + c] - mx) * inv : 0.f);
      e[i * heads + c] = wt;
      weights[((size_t)b * l + i) * heads + c] = wt;
    }
  }
  __syncthreads();
  const int nuv = dv / V;
  for (int c0 = 0; c0 < nuv; c0 += 64) {
    const int un = c0 + lane;
    const bool valid = un < nuv;
    Pk<V> acc[TATT_MAX_HEADS];
#pragma unroll
    for (int c = 0; c < TATT_MAX_HEADS; ++c) acc[c] = pk_zero<V>();
    for (int i = w; i < l; i += ATT_WAVES) {
      float wv[TATT_MAX_HEADS];
      bool any = false;
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c) {
        wv[c] = c < heads ? e[i * heads + c] : 0.f;
        any |= wv[c] != 0.f;
      }
      if (!any) continue;
      const Pk<V> x = valid ? pk_ld<V>(values + ((size_t)b * l + i) * dv + (size_t)un * V) : pk_zero<V>();
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[c].v[j] = fmaf(wv[c], x.v[j], acc[c].v[j]);
    }
    if (w > 0) {
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) pk_st<V>(macc + (((size_t)(w - 1) * heads + c) * 64 + lane) * V, acc[c]);
    }
    __syncthreads();
    if (w == 0 && valid) {
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) {
          Pk<V> o = acc[c];
          for (int ww = 0; ww < ATT_WAVES - 1; ++ww) {
            const Pk<V> x = pk_ld<V>(macc + (((size_t)ww * heads + c) * 64 + lane) * V);
#pragma unroll
            for (int j = 0; j < V; ++j) o.v[j] += x.v[j];
          }
          pk_st<V>(attended + ((size_t)b * heads + c) * dv + (size_t)un * V, o);
        }
    }
    __syncthreads();
  }
}

// Backward.  dwt[l][c] = g_w[l][c] + g_att[c] . values[l]; cc[c] = sum_l w dwt; de = w (dwt - cc);
//   dvalues[l] = sum_c w[l][c] g_att[c];  dpre[l] = (1 - t^2) sum_c de[l][c] w2[c];  du = sum_l dpre[l];
//   dw2_part[b][c] = sum_l de[l][c] t[l]   (the second stage adds the sequences in order)
//   phase 1  chunks of `values` columns with g_att's chunk in registers: dvalues chunk out, partial dwt into LDS (a row
//            belongs to one wave, so its LDS word has one writer)
//   phase 2  a wave per head: cc, de in place
//   phase 3  chunks of t columns with w2's chunk in registers: dpre out, du and dw2 partials per wave, merged like the
//            forward's sums
// Rows whose weights are all 0 are padding: dvalues / dpre rows are exact zeros and t is not read there.
// LDS: dwt[pad4(l * heads)] | macc[ATT_WAVES - 1][heads + 1][64 * V]
template <int V>
__global__ void __launch_bounds__(ATT_THREADS)
tanh_att_bwd_kernel(const float* __restrict__ t, const float* __restrict__ w2, const float* __restrict__ weights,
                    const float* __restrict__ values, const float* __restrict__ g_att, const float* __restrict__ g_w, int l,
                    int ha, int heads, int dv, float* __restrict__ dpre, float* __restrict__ du, float* __restrict__ dw2_part,
                    float* __restrict__ dvalues) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dwt = sm;
  float* macc = sm + pad4(l * heads);
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* wb = weights + (size_t)b * l * heads;
  for (int i = threadIdx.x; i < l * heads; i += ATT_THREADS) dwt[i] = g_w ? g_w[(size_t)b * l * heads + i] : 0.f;
  __syncthreads();
  const int nuv = dv / V;
  for (int c0 = 0; c0 < nuv; c0 += 64) {
    const int un = c0 + lane;
    const bool valid = un < nuv;
    Pk<V> g[TATT_MAX_HEADS];
#pragma unroll
    for (int c = 0; c < TATT_MAX_HEADS; ++c)
      g[c] = (valid && c < heads) ? pk_ld<V>(g_att + ((size_t)b * heads + c) * dv + (size_t)un * V) : pk_zero<V>();
    for (int i = w; i < l; i += ATT_WAVES) {
      float wv[TATT_MAX_HEADS];
      bool any = false;
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c) {
        wv[c] = c < heads ? wb[i * heads + c] : 0.f;
        any |= wv[c] != 0.f;
      }
      float* dvr = dvalues + ((size_t)b * l + i) * dv + (size_t)un * V;
      if (!any) {
        if (valid) pk_st<V>(dvr, pk_zero<V>());
        continue;
      }
      const Pk<V> x = valid ? pk_ld<V>(values + ((size_t)b * l + i) * dv + (size_t)un * V) : pk_zero<V>();
      Pk<V> o = pk_zero<V>();
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = fmaf(wv[c], g[c].v[j], o.v[j]);
      if (valid) pk_st<V>(dvr, o);
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) {
          const float p = wave_sum(pk_dot<V>(x, g[c], 0.f));
          if (lane == 0) dwt[i * heads + c] += p;
        }
    }
  }
  __syncthreads();
  for (int c = w; c < heads; c += ATT_WAVES) {
    float p = 0.f;
    for (int i = lane; i < l; i += 64) {
      const float wt = wb[i * heads + c];
      if (wt != 0.f) p = fmaf(wt, dwt[i * heads + c], p);
    }
    const float cc = wave_sum(p);
    for (int i = lane; i < l; i += 64) {
      const float wt = wb[i * heads + c];
      dwt[i * heads + c] = wt != 0.f ? wt * (dwt[i * heads + c] - cc) : 0.f;
    }
  }
  __syncthreads();
  const int nua = ha / V;
  for (int c0 = 0; c0 < nua; c0 += 64) {
    const int un = c0 + lane;
    const bool valid = un < nua;
    Pk<V> wr[TATT_MAX_HEADS], dwa[TATT_MAX_HEADS], dua = pk_zero<V>();
#pragma unroll
    for (int c = 0; c < TATT_MAX_HEADS; ++c) {
      wr[c] = (valid && c < heads) ? pk_ld<V>(w2 + (size_t)c * ha + (size_t)un * V) : pk_zero<V>();
      dwa[c] = pk_zero<V>();
    }
    for (int i = w; i < l; i += ATT_WAVES) {
      float de[TATT_MAX_HEADS];
      bool any = false;
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c) {
        de[c] = c < heads ? dwt[i * heads + c] : 0.f;
        any |= c < heads && wb[i * heads + c] != 0.f;
      }
      if (!valid) continue;
      const size_t at = ((size_t)b * l + i) * ha + (size_t)un * V;
      if (!any) {
        pk_st<V>(dpre + at, pk_zero<V>());
        continue;
      }
      const Pk<V> tt = pk_ld<V>(t + at);
      Pk<V> o = pk_zero<V>();
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = fmaf(de[c], wr[c].v[j], o.v[j]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o.v[j] *= 1.f - tt.v[j] * tt.v[j];
        dua.v[j] += o.v[j];
      }
      pk_st<V>(dpre + at, o);
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) dwa[c].v[j] = fmaf(de[c], tt.v[j], dwa[c].v[j]);
    }
    if (w > 0) {
      float* mw = macc + (size_t)(w - 1) * (heads + 1) * 64 * V;
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) pk_st<V>(mw + ((size_t)c * 64 + lane) * V, dwa[c]);
      pk_st<V>(mw + ((size_t)heads * 64 + lane) * V, dua);
    }
    __syncthreads();
    if (w == 0 && valid) {
      for (int ww = 0; ww < ATT_WAVES - 1; ++ww) {
        const float* mw = macc + (size_t)ww * (heads + 1) * 64 * V;
#pragma unroll
        for (int c = 0; c < TATT_MAX_HEADS; ++c)
          if (c < heads) {
            const Pk<V> x = pk_ld<V>(mw + ((size_t)c * 64 + lane) * V);
#pragma unroll
            for (int j = 0; j < V; ++j) dwa[c].v[j] += x.v[j];
          }
        const Pk<V> x = pk_ld<V>(mw + ((size_t)heads * 64 + lane) * V);
#pragma unroll
        for (int j = 0; j < V; ++j) dua.v[j] += x.v[j];
      }
#pragma unroll
      for (int c = 0; c < TATT_MAX_HEADS; ++c)
        if (c < heads) pk_st<V>(dw2_part + ((size_t)b * heads + c) * ha + (size_t)un * V, dwa[c]);
      if (du) pk_st<V>(du + (size_t)b * ha + (size_t)un * V, dua);
    }
    __syncthreads();
  }
}

// second stage of dW2: out[i] += sum_k part[k][i], k = 0 .. nb-1; 64 elements x 4 k-lanes per block, each lane walks its
// k = lane, lane + 4, ... in order, the four lane sums are added in lane order
__global__ void __launch_bounds__(256)
sum_partials_kernel(const float* __restrict__ part, int nb, int n, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63), kl = threadIdx.x >> 6;
  float acc = 0.f;
  if (i < n)
#pragma unroll 4
    for (int k = kl; k < nb; k += 4) acc += part[(size_t)k * n + i];
  red[kl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (kl == 0 && i < n) out[i] += ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

int query_check(const char* who, int b, int l, int d) {
  GH_REQUIRE(b > 0 && l > 0 && d > 0, "%s: b=%d l=%d d=%d must be positive", who, b, l, d);
  GH_REQUIRE(l <= QATT_MAX_L, "%s: sequence length l=%d exceeds the supported %d", who, l, QATT_MAX_L);
  GH_REQUIRE(d <= QATT_MAX_D, "%s: width d=%d exceeds the supported %d", who, d, QATT_MAX_D);
  return 0;
}

int tanh_check(const char* who, int b, int l, int ha, int heads, int dv) {
  GH_REQUIRE(b > 0 && l > 0 && ha > 0 && dv > 0, "%s: b=%d l=%d ha=%d dv=%d must be positive", who, b, l, ha, dv);
  GH_REQUIRE(heads >= 1 && heads <= TATT_MAX_HEADS, "%s: heads=%d (supported: 1..%d)", who, heads, TATT_MAX_HEADS);
  GH_REQUIRE((long long)l * heads <= TATT_MAX_LH, "%s: sequence length l=%d with heads=%d exceeds the supported l * heads <= %d", who,
             l, heads, TATT_MAX_LH);
  return 0;
}

// K = float4 (V = 4) or float (V = 1) units per lane that cover one row of d floats
#define GH_QATT_DISPATCH(KERNEL, ...)                                                                         \
  do {                                                                                                        \
    if (vec) {                                                                                                \
      const int nu = d / 4;                                                                                   \
      if (nu <= 64) hipLaunchKernelGGL((KERNEL<4, 1>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__);      \
      else if (nu <= 128) hipLaunchKernelGGL((KERNEL<4, 2>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__); \
      else if (nu <= 256) hipLaunchKernelGGL((KERNEL<4, 4>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<4, 8>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__);               \
    } else {                                                                                                  \
      if (d <= 256) hipLaunchKernelGGL((KERNEL<1, 4>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__);      \
      else hipLaunchKernelGGL((KERNEL<1, 32>), dim3(b), dim3(ATT_THREADS), lds, st, __VA_ARGS__);              \
    }                                                                                                         \
  } while (0)

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_query_att_fwd(const float* q, const float* right, const float* mask, int b, int l, int d, float* weights,
                                float* avg, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = query_check("query_att_fwd", b, l, d)) return rc;
  GH_REQUIRE(q && right && mask && weights && avg, "query_att_fwd: NULL argument");
  const bool vec = d % 4 == 0 && aligned16(q) && aligned16(right) && aligned16(avg);
  const size_t lds = ((size_t)pad4(l) + 2 * ATT_WAVES + (size_t)ATT_WAVES * d) * sizeof(float);
  GH_QATT_DISPATCH(query_att_fwd_kernel, q, right, mask, l, d, weights, avg);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_query_att_bwd(const float* q, const float* right, const float* weights, const float* g_avg, const float* g_w,
                                int b, int l, int d, float* dq, float* dright, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = query_check("query_att_bwd", b, l, d)) return rc;
  GH_REQUIRE(q && right && weights && g_avg && dq && dright, "query_att_bwd: NULL argument");
  const bool vec = d % 4 == 0 && aligned16(q) && aligned16(right) && aligned16(g_avg) && aligned16(dright);
  const size_t lds = ((size_t)pad4(l) + 2 * ATT_WAVES + (size_t)ATT_WAVES * d) * sizeof(float);
  GH_QATT_DISPATCH(query_att_bwd_kernel, q, right, weights, g_avg, g_w, l, d, dq, dright);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_tanh_att_fwd(const float* pre, const float* u, const float* w2, const float* mask, const float* values, int b,
                               int l, int ha, int heads, int dv, float* t, float* weights, float* attended,
                               gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = tanh_check("tanh_att_fwd", b, l, ha, heads, dv)) return rc;
  GH_REQUIRE(pre && w2 && mask && values && t && weights && attended, "tanh_att_fwd: NULL argument");
  const bool vec = ha % 4 == 0 && dv % 4 == 0 && aligned16(pre) && aligned16(u) && aligned16(w2) && aligned16(values) &&
                   aligned16(t) && aligned16(attended);
  const int V = vec ? 4 : 1;
  const size_t lds = ((size_t)pad4(l * heads) + (size_t)(ATT_WAVES - 1) * heads * 64 * V) * sizeof(float);
  if (vec)
    hipLaunchKernelGGL(tanh_att_fwd_kernel<4>, dim3(b), dim3(ATT_THREADS), lds, st, pre, u, w2, mask, values, l, ha, heads, dv, t,
                       weights, attended);
  else
    hipLaunchKernelGGL(tanh_att_fwd_kernel<1>, dim3(b), dim3(ATT_THREADS), lds, st, pre, u, w2, mask, values, l, ha, heads, dv, t,
                       weights, attended);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_tanh_att_bwd(const float* t, const float* w2, const float* weights, const float* values, const float* g_att,
                               const float* g_w, int b, int l, int ha, int heads, int dv, float* dpre, float* du, float* dw2,
                               float* dvalues, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = tanh_check("tanh_att_bwd", b, l, ha, heads, dv)) return rc;
  GH_REQUIRE(t && w2 && weights && values && g_att && dpre && dw2 && dvalues, "tanh_att_bwd: NULL argument");
  const Workspace wsp = workspace_for(st);
  const size_t need = (size_t)b * heads * ha * sizeof(float);
  GH_REQUIRE(wsp.p && need <= wsp.bytes,
             "tanh_att_bwd: the per-sequence dW2 partials need %zu bytes of stream workspace (gh_set_stream_workspace / gh_set_workspace)",
             need);
  const bool vec = ha % 4 == 0 && dv % 4 == 0 && aligned16(t) && aligned16(w2) && aligned16(values) && aligned16(g_att) &&
                   aligned16(dpre) && aligned16(du) && aligned16(dvalues) && aligned16(wsp.p);
  const int V = vec ? 4 : 1;
  const size_t lds = ((size_t)pad4(l * heads) + (size_t)(ATT_WAVES - 1) * (heads + 1) * 64 * V) * sizeof(float);
  if (vec)
    hipLaunchKernelGGL(tanh_att_bwd_kernel<4>, dim3(b), dim3(ATT_THREADS), lds, st, t, w2, weights, values, g_att, g_w, l, ha,
                       heads, dv, dpre, du, wsp.p, dvalues);
  else
    hipLaunchKernelGGL(tanh_att_bwd_kernel<1>, dim3(b), dim3(ATT_THREADS), lds, st, t, w2, weights, values, g_att, g_w, l, ha,
                       heads, dv, dpre, du, wsp.p, dvalues);
  const int n = heads * ha;
  hipLaunchKernelGGL(sum_partials_kernel, dim3((n + 63) / 64), dim3(256), 0, st, wsp.p, b, n, dw2);
  GH_LAUNCH_CHECK();
  return 0;
}
