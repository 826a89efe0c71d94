// Softmax cross-entropy with an ignore index over rows of any width (pytorch_transformers/modeling_bert.py: the CrossEntropyLoss
// every task model ends in, :698 :765 :822 :890 :996 :1056 :1142): gh_softmax_xent_fwd keeps one log-sum-exp per row (two floats) and the mean
// loss of the kept rows, gh_softmax_xent_bwd forms the gradient from the logits and that log-sum-exp alone.  No rows x c tensor
// lives between the two.  See include/get_hip.h for the contract of the entry points.
#include "../../include/get_hip.h"
#include "common.h"
#include <limits.h>

// The element-wise, float2 and float4 variants of a kernel promise the same bits (a strided view against its contiguous copy): they share
// every arithmetic statement, and nothing here may be contracted differently between two instantiations.
#pragma clang fp contract(off)

namespace gh {

// ---------------------------------------------------------------------------- dispatch on the row width c
//   c <= XENT_LANE_MAX_C   one lane per row (the B x 2 heads, 9 tags): 256 rows per workgroup
//   c <= XENT_WAVE_MAX_C   one wave per row (the 384- / 512-wide QA rows): 4 rows per workgroup
//   wider                  one workgroup per row (the 30522-wide vocabulary: 30 groups of four per lane)
// The wide paths read a group of four as one float4 where cs == 1 and base and row stride allow 16 bytes, as two float2 where
// they allow 8 (a contiguous 30522-wide matrix: 30522 = 2 mod 4 rules float4 out for every other row), else element by element
// (vec_width); all three hand lane t the elements 4 q .. 4 q + 3 of the groups q = t, t + lanes, .. in that order, so they agree
// bit for bit.
constexpr int XENT_LANE_MAX_C = 32;
constexpr int XENT_WAVE_MAX_C = 2048;
constexpr int XENT_THREADS = 256;
constexpr int XENT_WAVES = XENT_THREADS / 64;

__device__ __forceinline__ long long label_at(const void* labels, int i64, long long r) {
  return i64 ? (long long)static_cast<const int64_t*>(labels)[r] : (long long)static_cast<const int32_t*>(labels)[r];
}
// a row takes part iff its label is a class and not the ignore index (a label outside [0, c) drops the row: torch raises there)
__device__ __forceinline__ bool row_kept(long long label, long long ignore, int c) { return label != ignore && label >= 0 && label < c; }

// running (max, sum of exp(v - max)) of a lane
struct MaxSum { float m, s; };
__device__ __forceinline__ void ms_add(MaxSum& a, const float* v, int n) {
  float gm = v[0];
  for (int i = 1; i < n; ++i) gm = fmaxf(gm, v[i]);
  if (gm > a.m) {
    a.s = a.s * expf(a.m - gm);      // a.m == -inf: a.s is 0 and stays 0
    a.m = gm;
  }
  if (a.m == -INFINITY) return;      // nothing but -inf so far
  for (int i = 0; i < n; ++i) a.s = a.s + expf(v[i] - a.m);
}
__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b) {
  MaxSum r;
  r.m = fmaxf(a.m, b.m);
  if (r.m == -INFINITY) { r.s = 0.f; return r; }
  // the larger maximum's term first: both partners of a butterfly step form the same sum
  const float hi = a.m >= b.m ? a.s : b.s, lo = a.m >= b.m ? b.s : a.s, d = a.m >= b.m ? b.m - a.m : a.m - b.m;
  r.s = hi + lo * expf(d);
  return r;
}
__device__ __forceinline__ MaxSum ms_wave(MaxSum a) {
  for (int off = 32; off >= 1; off >>= 1) {
    MaxSum o;
    o.m = __shfl_xor(a.m, off, 64);
    o.s = __shfl_xor(a.s, off, 64);
    a = ms_merge(a, o);
  }
  return a;
}

template <int VEC>
__device__ __forceinline__ int load_group(const float* __restrict__ row, int cs, int c, int q, float* v) {
  const int j = 4 * q, n = c - j < 4 ? c - j : 4;
  if (VEC == 4 && n == 4) {
    const float4 w = *reinterpret_cast<const float4*>(row + j);
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  } else if (VEC == 2 && n == 4) {
    const float2 a = *reinterpret_cast<const float2*>(row + j), b = *reinterpret_cast<const float2*>(row + j + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
    for (int i = 0; i < n; ++i) v[i] = row[(long long)(j + i) * cs];
  }
  return n;
}

// (max, sum) of one row over `lanes` lanes, lane `t`
template <int VEC>
__device__ __forceinline__ MaxSum row_max_sum(const float* __restrict__ row, int cs, int c, int t, int lanes) {
  MaxSum a{-INFINITY, 0.f};
  const int groups = (c + 3) >> 2;
  float v[4];
#pragma unroll 4
  for (int q = t; q < groups; q += lanes) {
    const int n = load_group<VEC>(row, cs, c, q, v);
    ms_add(a, v, n);
  }
  return a;
}

__device__ __forceinline__ void finish_row(const float* __restrict__ row, int cs, int c, long long r, MaxSum a, const void* labels,
                                           int i64, long long ignore, float* __restrict__ lse, float* __restrict__ lse_lo,
                                           float* __restrict__ row_loss, unsigned int* __restrict__ clamped) {
  // lse = m + log s rounds at the size of m (2^-10 at 1e4: a relative 5e-4 in every probability formed from it alone), so what
  // the rounding dropped rides along: (m - lse) is exact where lse is within a factor 2 of m
  const float ls = logf(a.s), l = a.m + ls;
  const long long y = label_at(labels, i64, r);
  const bool kept = row_kept(y, ignore, c);
  lse[r] = l;
  lse_lo[r] = a.m == -INFINITY ? 0.f : (a.m - l) + ls;
  row_loss[r] = kept ? (a.m - row[y * cs]) + ls : 0.f;
  if (!kept && y != ignore) atomicAdd(clamped + 4, 1u);      // nn.CrossEntropyLoss raises there; counted, gh_clamp_events_n
}

// ---------------------------------------------------------------------------- forward
__global__ void __launch_bounds__(XENT_THREADS)
xent_fwd_lane_kernel(const float* __restrict__ x, long long ldx, int cs, const void* __restrict__ labels, int i64, long long ignore,
                     long long rows, int c, float* __restrict__ lse, float* __restrict__ lse_lo, float* __restrict__ row_loss,
                     unsigned int* __restrict__ clamped) {
  const long long r = (long long)blockIdx.x * XENT_THREADS + threadIdx.x;
  if (r >= rows) return;
  const float* row = x + r * ldx;
  MaxSum a{-INFINITY, 0.f};
  for (int j = 0; j < c; ++j) {
    const float v = row[(long long)j * cs];
    ms_add(a, &v, 1);
  }
  finish_row(row, cs, c, r, a, labels, i64, ignore, lse, lse_lo, row_loss, clamped);
}

template <int VEC>
__global__ void __launch_bounds__(XENT_THREADS)
xent_fwd_wave_kernel(const float* __restrict__ x, long long ldx, int cs, const void* __restrict__ labels, int i64, long long ignore,
                     long long rows, int c, float* __restrict__ lse, float* __restrict__ lse_lo, float* __restrict__ row_loss,
                     unsigned int* __restrict__ clamped) {
  const long long r = (long long)blockIdx.x * XENT_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;      // (whole waves leave: no barrier below)
  const float* row = x + r * ldx;
  const MaxSum a = ms_wave(row_max_sum<VEC>(row, cs, c, threadIdx.x & 63, 64));
  if ((threadIdx.x & 63) == 0) finish_row(row, cs, c, r, a, labels, i64, ignore, lse, lse_lo, row_loss, clamped);
}

template <int VEC>
__global__ void __launch_bounds__(XENT_THREADS)
xent_fwd_block_kernel(const float* __restrict__ x, long long ldx, int cs, const void* __restrict__ labels, int i64, long long ignore,
                      long long rows, int c, float* __restrict__ lse, float* __restrict__ lse_lo, float* __restrict__ row_loss,
                      unsigned int* __restrict__ clamped) {
  __shared__ float wave_m[XENT_WAVES], wave_s[XENT_WAVES];
  const long long r = blockIdx.x;
  const float* row = x + r * ldx;
  const MaxSum a = ms_wave(row_max_sum<VEC>(row, cs, c, threadIdx.x, XENT_THREADS));
  if ((threadIdx.x & 63) == 0) { wave_m[threadIdx.x >> 6] = a.m; wave_s[threadIdx.x >> 6] = a.s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    MaxSum t{wave_m[0], wave_s[0]};
    for (int w = 1; w < XENT_WAVES; ++w) t = ms_merge(t, MaxSum{wave_m[w], wave_s[w]});      // in wave order
    finish_row(row, cs, c, r, t, labels, i64, ignore, lse, lse_lo, row_loss, clamped);
  }
}

// One workgroup: lane t sums the losses of the rows [t * per, (t + 1) * per), per = ceil(rows / 256), in row order and counts the
// kept ones; lane 0 then sums the 256 lane sums in lane order.  All in double; the mean is rounded once to fp32 (0 / 0 = NaN).
__global__ void __launch_bounds__(XENT_THREADS)
xent_mean_kernel(const float* __restrict__ row_loss, const void* __restrict__ labels, int i64, long long ignore, long long rows, int c,
                 float* __restrict__ loss, int64_t* __restrict__ n_kept) {
  __shared__ double lane_sum[XENT_THREADS];
  __shared__ long long lane_cnt[XENT_THREADS];
  const long long per = (rows + XENT_THREADS - 1) / XENT_THREADS;
  const long long lo = per * threadIdx.x, hi = lo + per < rows ? lo + per : rows;
  double s = 0.0;
  long long n = 0;
  for (long long r = lo; r < hi; ++r) {
    if (row_kept(label_at(labels, i64, r), ignore, c)) { s += (double)row_loss[r]; ++n; }
  }
  lane_sum[threadIdx.x] = s;
  lane_cnt[threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    long long count = 0;
    for (int t = 0; t < XENT_THREADS; ++t) { total += lane_sum[t]; count += lane_cnt[t]; }
    loss[0] = (float)(total / (double)count);
    n_kept[0] = (int64_t)count;
  }
}

// ---------------------------------------------------------------------------- backward
// dx = (exp(x - lse) - [j == label]) * k, k = g / n_kept, for a kept row; zeros for any other.  lse = l + lo (finish_row).
__device__ __forceinline__ float xent_grad(float v, float l, float lo, bool hot, float k) {
  return (expf((v - l) - lo) - (hot ? 1.f : 0.f)) * k;
}

template <int VEC>
__device__ __forceinline__ void row_grad(const float* __restrict__ row, int cs, float* __restrict__ drow, int dcs, int c, long long y,
                                         bool kept, float l, float lo, float k, int t, int lanes) {
  const int groups = (c + 3) >> 2;
  float v[4];
#pragma unroll 4
  for (int q = t; q < groups; q += lanes) {
    const int j = 4 * q;
    int n = c - j < 4 ? c - j : 4;
    if (kept) n = load_group<VEC>(row, cs, c, q, v);
    for (int i = 0; i < n; ++i) v[i] = kept ? xent_grad(v[i], l, lo, j + i == y, k) : 0.f;
    if (VEC == 4 && n == 4) {
      *reinterpret_cast<float4*>(drow + j) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (VEC == 2 && n == 4) {
      *reinterpret_cast<float2*>(drow + j) = make_float2(v[0], v[1]);
      *reinterpret_cast<float2*>(drow + j + 2) = make_float2(v[2], v[3]);
    } else {
      for (int i = 0; i < n; ++i) drow[(long long)(j + i) * dcs] = v[i];
    }
  }
}

struct XentBwd {
  const float* x; long long ldx; int cs;
  const void* labels; int i64; long long ignore, rows; int c;
  const float* lse; const float* lse_lo; const float* g; const int64_t* n_kept;
  float* dx; long long lddx; int dcs;
};

__global__ void __launch_bounds__(XENT_THREADS) xent_bwd_lane_kernel(XentBwd a) {
  const long long r = (long long)blockIdx.x * XENT_THREADS + threadIdx.x;
  if (r >= a.rows) return;
  const long long y = label_at(a.labels, a.i64, r);
  const bool kept = row_kept(y, a.ignore, a.c);
  const float k = a.g[0] / (float)a.n_kept[0], l = a.lse[r], lo = a.lse_lo[r];
  const float* row = a.x + r * a.ldx;
  float* drow = a.dx + r * a.lddx;
  for (int j = 0; j < a.c; ++j) drow[(long long)j * a.dcs] = kept ? xent_grad(row[(long long)j * a.cs], l, lo, j == y, k) : 0.f;
}

template <int VEC, int LANES>      // LANES = 64: a wave per row; XENT_THREADS: a workgroup per row
__global__ void __launch_bounds__(XENT_THREADS) xent_bwd_wide_kernel(XentBwd a) {
  const long long r = LANES == 64 ? (long long)blockIdx.x * XENT_WAVES + (threadIdx.x >> 6) : (long long)blockIdx.x;
  if (r >= a.rows) return;
  const long long y = label_at(a.labels, a.i64, r);
  const bool kept = row_kept(y, a.ignore, a.c);
  const float k = a.g[0] / (float)a.n_kept[0], l = a.lse[r], lo = a.lse_lo[r];
  row_grad<VEC>(a.x + r * a.ldx, a.cs, a.dx + r * a.lddx, a.dcs, a.c, y, kept, l, lo, k, LANES == 64 ? (threadIdx.x & 63) : threadIdx.x, LANES);
}

// the widest access every row of a layout allows: 4 floats (base and row stride multiples of 16 bytes), 2 (of 8 bytes: the
// contiguous 30522-wide vocabulary, 30522 = 2 mod 4), else 1
inline int vec_width(const float* p, long long ld, int cs) {
  if (cs != 1) return 1;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0 && ld % 4 == 0) return 4;
  if ((a & 7) == 0 && ld % 2 == 0) return 2;
  return 1;
}

static int xent_check(const char* who, const float* x, long long ldx, int cs, const void* labels, long long rows, int c) {
  GH_REQUIRE(x != nullptr && labels != nullptr, "%s: NULL logits or labels", who);
  GH_REQUIRE(rows > 0 && rows <= INT_MAX, "%s: rows=%lld (1 .. 2^31 - 1; an empty input is the caller's to answer)", who, rows);
  GH_REQUIRE(c > 0, "%s: c=%d classes", who, c);
  GH_REQUIRE(cs >= 1, "%s: element stride %d (>= 1)", who, cs);
  GH_REQUIRE(ldx >= (long long)(c - 1) * cs + 1, "%s: row stride %lld is below the %lld floats a row of c=%d at element stride %d spans",
             who, ldx, (long long)(c - 1) * cs + 1, c, cs);
  return 0;
}

}  // namespace gh

using namespace gh;

extern "C" int gh_softmax_xent_fwd(const float* x, int64_t ldx, int cs, const void* labels, int labels_i64, int64_t ignore_index,
                                   int64_t rows, int c, float* lse, float* lse_lo, float* row_loss, float* loss, int64_t* n_kept,
                                   gh_stream_t stream) {
  if (int rc = xent_check("softmax_xent_fwd", x, ldx, cs, labels, rows, c)) return rc;
  GH_REQUIRE(lse && lse_lo && row_loss && loss && n_kept, "softmax_xent_fwd: NULL output");
  unsigned int* clamped = clamp_counter();
  GH_REQUIRE(clamped, "softmax_xent_fwd: cannot allocate the clamp counter");
  hipStream_t s = (hipStream_t)stream;
  const int vec = vec_width(x, ldx, cs);
  if (c <= XENT_LANE_MAX_C) {
    const unsigned grid = (unsigned)((rows + XENT_THREADS - 1) / XENT_THREADS);
    hipLaunchKernelGGL(xent_fwd_lane_kernel, dim3(grid), dim3(XENT_THREADS), 0, s, x, (long long)ldx, cs, labels, labels_i64,
                       (long long)ignore_index, (long long)rows, c, lse, lse_lo, row_loss, clamped);
  } else if (c <= XENT_WAVE_MAX_C) {
    const unsigned grid = (unsigned)((rows + XENT_WAVES - 1) / XENT_WAVES);
    auto kern = vec == 4 ? xent_fwd_wave_kernel<4> : vec == 2 ? xent_fwd_wave_kernel<2> : xent_fwd_wave_kernel<1>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(XENT_THREADS), 0, s, x, (long long)ldx, cs, labels, labels_i64, (long long)ignore_index,
                       (long long)rows, c, lse, lse_lo, row_loss, clamped);
  } else {
    auto kern = vec == 4 ? xent_fwd_block_kernel<4> : vec == 2 ? xent_fwd_block_kernel<2> : xent_fwd_block_kernel<1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(XENT_THREADS), 0, s, x, (long long)ldx, cs, labels, labels_i64,
                       (long long)ignore_index, (long long)rows, c, lse, lse_lo, row_loss, clamped);
  }
  GH_LAUNCH_CHECK();
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(XENT_THREADS), 0, s, row_loss, labels, labels_i64, (long long)ignore_index,
                     (long long)rows, c, loss, n_kept);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_softmax_xent_bwd(const float* x, int64_t ldx, int cs, const void* labels, int labels_i64, int64_t ignore_index,
                                   int64_t rows, int c, const float* lse, const float* lse_lo, const float* g, const int64_t* n_kept,
                                   float* dx, int64_t lddx, int dcs, gh_stream_t stream) {
  if (int rc = xent_check("softmax_xent_bwd", x, ldx, cs, labels, rows, c)) return rc;
  GH_REQUIRE(lse && lse_lo && g && n_kept && dx, "softmax_xent_bwd: NULL lse, lse_lo, g, n_kept or dx");
  GH_REQUIRE(dcs >= 1, "softmax_xent_bwd: element stride %d of dx (>= 1)", dcs);
  GH_REQUIRE(lddx >= (long long)(c - 1) * dcs + 1, "softmax_xent_bwd: row stride %lld of dx is below the %lld floats a row spans",
             (long long)lddx, (long long)(c - 1) * dcs + 1);
  hipStream_t s = (hipStream_t)stream;
  const XentBwd a{x, (long long)ldx, cs, labels, labels_i64, (long long)ignore_index, (long long)rows, c, lse, lse_lo, g, n_kept, dx,
                  (long long)lddx, dcs};
  const int vx = vec_width(x, ldx, cs), vd = vec_width(dx, lddx, dcs), vec = vx < vd ? vx : vd;
  if (c <= XENT_LANE_MAX_C) {
    hipLaunchKernelGGL(xent_bwd_lane_kernel, dim3((unsigned)((rows + XENT_THREADS - 1) / XENT_THREADS)), dim3(XENT_THREADS), 0, s, a);
  } else if (c <= XENT_WAVE_MAX_C) {
    auto kern = vec == 4 ? xent_bwd_wide_kernel<4, 64> : vec == 2 ? xent_bwd_wide_kernel<2, 64> : xent_bwd_wide_kernel<1, 64>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + XENT_WAVES - 1) / XENT_WAVES)), dim3(XENT_THREADS), 0, s, a);
  } else {
    auto kern = vec == 4 ? xent_bwd_wide_kernel<4, XENT_THREADS> : vec == 2 ? xent_bwd_wide_kernel<2, XENT_THREADS>
                                                                             : xent_bwd_wide_kernel<1, XENT_THREADS>;
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(XENT_THREADS), 0, s, a);
  }
  GH_LAUNCH_CHECK();
  return 0;
}
