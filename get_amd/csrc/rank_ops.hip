// Pair-wise ranking: the two matchzoo ranking losses and the six matchzoo ranking metrics.
//   gh_rank_metrics       matchzoo/metrics/{precision,average_precision,mean_average_precision,mean_reciprocal_rank,
//                         discounted_cumulative_gain,normalized_discounted_cumulative_gain}.py for ALL groups of a ragged batch
//                         in one launch, and the per-item rank inside each group (the segmented-sort primitive)
//   gh_rank_hinge_fwd/bwd matchzoo/losses/rank_hinge_loss.py:54-66
//   gh_rank_ce_fwd/bwd    matchzoo/losses/rank_cross_entropy_loss.py:29-38 (with a stable log-softmax)
//
// ---- metrics.  Workgroups of 256 threads (four waves); a group takes one of two DISPATCH PATHS, chosen by its length alone:
//   wave       0 <= len <= 64    workgroup b < ceil(g / 4): wave w owns group 4b + w, one item per lane, four groups side by side
//   workgroup  65 <= len <= 1024 workgroup ceil(g / 4) + q: all four waves own group q together, up to four items per thread
// The grid is ceil(g / 4) + g workgroups: a wave whose group is long, and a workgroup whose group is short, has nothing to do
// (a GET-style evaluation of 2000 short groups launches 2000 workgroups that read two offsets and end).
// Both paths run the same four phases over LDS tiles of the group (rank_group<64> / rank_group<256>):
//   1 load    scores (widened to fp64: exact, so fp32 and fp64 inputs of equal values rank alike) and labels into LDS
//   2 rank    by counting over the tile, every lane reading the same LDS address (a broadcast):
//             rank_i = #{j : s_j > s_i} + #{j < i : s_j == s_i}, IEEE comparisons on values -- the position of item i in Python's
//             stable sorted(key=score, reverse=True); the same count on the labels gives the ideal ordering of the NDCG.  The
//             ranks are a permutation of 0 .. len - 1: the labels are scattered to their positions in both orderings
//   3 terms   position r: prefix counts of the relevant labels up to r (ballot + popcount per 64 positions, integer sums over
//             the chunks in front: exact) give hits@k, n_rel, the first relevant position and the summands of AP and MAP; the
//             summands of DCG and IDCG come from the label at r
//   4 sums    every per-group float has ONE owning wave.  Lane l adds the summands r = l, l + 64, l + 128 ... in that order,
//             then a 64-lane xor butterfly adds the lanes: the order depends on the group's length (and k) only, not on the
//             path, the grid or the neighbouring groups, so two runs are bit-identical.  No floating-point atomics anywhere; the
//             only atomics are integer ones (the LDS minimum for the first relevant position and the two global NaN counters).
// A NaN score or label compares false with everything: such items are counted in nan_count and the float outputs of their group
// are unspecified (the caller raises); every write stays inside the group whatever the values are.
//
// ---- losses.  One wave per training instance (its positive row and num_neg negative rows, `c` columns each): lane-strided
// sequential sums and a butterfly, so every value is deterministic; the scalar reductions are a second, single-workgroup launch
// over the per-instance partial sums in a fixed order.  The backward kernels write every gradient element exactly once.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include <limits.h>
#include <math.h>

namespace gh {
namespace {

constexpr int RK_BLOCK = 256;                    // wave64 x 4
constexpr int RK_WAVES = RK_BLOCK / 64;          // groups per workgroup
constexpr int RK_MAX = GH_RANK_MAX_GROUP;        // items of a group: four LDS tiles of 8 KB
constexpr int RK_MAX_KS = GH_RANK_MAX_KS;
constexpr int RK_CHUNKS = RK_MAX / 64;           // 64-position chunks of the prefix counts
constexpr int RK_WAVE_LEN = 64;                  // longest group of the wave path
static_assert(RK_MAX == 4 * RK_BLOCK && RK_WAVES * RK_WAVE_LEN <= RK_MAX, "tile arithmetic");

struct RankKs { int k[RK_MAX_KS]; };

// integers a group keeps in LDS between the phases
struct RankCounts { int rel[RK_CHUNKS]; int rel0[RK_CHUNKS]; int first; int n_rel; };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of tile[0 .. limit): lane l adds l, l + 64, ... in order, then the butterfly (every lane ends with the result)
__device__ __forceinline__ double strided_sum(const double* tile, int limit, int lane) {
  double acc = 0.0;
  for (int r = lane; r < limit; r += 64) acc += tile[r];
  return wave_sum_f64(acc);
}

// math.pow(2., label) - 1.: exact for the integer labels of a graded relevance scale
__device__ __forceinline__ double rank_gain(double label) {
  const double p = (label == floor(label) && fabs(label) <= 1000.0) ? ldexp(1.0, (int)label) : exp2(label);
  return p - 1.0;
}

// One group of `len` items starting at item `base`, owned by NT threads (t = 0 .. NT - 1): one wave (NT = 64) or the workgroup
// (NT = 256).  Every thread of the workgroup calls this at the same time (the barriers are workgroup barriers); `live` is false
// for the callers that have no group to work on (len is then 0) and nothing is written for them.  a, b, c, d: this group's LDS
// tiles of at least max(len, 1) doubles; cnt: its integers.
template <int NT>
__device__ __forceinline__ void rank_group(const void* __restrict__ scores, int f64, const double* __restrict__ labels, int base, int len,
                                           bool live, double thr, const RankKs& ks, int nk, int t, double* a, double* b, double* c, double* d,
                                           RankCounts* cnt, int32_t* __restrict__ rank, int32_t* __restrict__ gi, double* __restrict__ gd,
                                           unsigned* nan_s, unsigned* nan_l) {
  constexpr int IPT = NT == RK_BLOCK ? RK_MAX / RK_BLOCK : 1;      // items per thread: 4 for the workgroup, 1 for a wave
  static_assert(NT == RK_BLOCK || NT == RK_WAVE_LEN, "a wave or the workgroup");
  const int lane = t & 63;
  const double nan = __builtin_nan("");
  // ---- 1 load
  for (int i = t; i < len; i += NT) {
    const double s = f64 ? static_cast<const double*>(scores)[base + i] : (double)static_cast<const float*>(scores)[base + i];
    const double l = labels[base + i];
    *nan_s += s != s;
    *nan_l += l != l;
    a[i] = s;
    b[i] = l;
    c[i] = 0.0;
    d[i] = 0.0;
  }
  if (t < RK_CHUNKS) cnt->rel[t] = cnt->rel0[t] = 0;
  if (t == 0) { cnt->first = INT_MAX; cnt->n_rel = 0; }
  __syncthreads();
  // ---- 2 rank by counting; an item beyond len is a NaN and counts nothing
  {
    double si[IPT], li[IPT];
    int gt[IPT], lgt[IPT];
#pragma unroll
    for (int m = 0; m < IPT; ++m) {
      const int i = m * NT + t;
      si[m] = i < len ? a[i] : nan;
      li[m] = i < len ? b[i] : nan;
      gt[m] = lgt[m] = 0;
    }
    for (int j = 0; j < len; ++j) {
      const double sj = a[j], lj = b[j];
#pragma unroll
      for (int m = 0; m < IPT; ++m) {
        const bool before = j < m * NT + t;
        gt[m] += (sj > si[m]) + ((sj == si[m]) & before);
        lgt[m] += (lj > li[m]) + ((lj == li[m]) & before);
      }
    }
#pragma unroll
    for (int m = 0; m < IPT; ++m) {
      const int i = m * NT + t;
      if (i < len) {                               // gt, lgt <= len - 1: item i itself adds nothing
        rank[base + i] = gt[m];
        c[gt[m]] = li[m];
        d[lgt[m]] = li[m];
      }
    }
  }
  __syncthreads();
  // ---- 3 terms: position r of both orderings
  double lab[IPT];
  int pc[IPT], pc0[IPT];
#pragma unroll
  for (int m = 0; m < IPT; ++m) {
    const int r = m * NT + t;
    lab[m] = r < len ? c[r] : nan;
    const unsigned long long rel = __ballot(lab[m] > thr), rel0 = __ballot(lab[m] > 0.0);
    const unsigned long long upto = (2ull << lane) - 1ull;      // lanes 0 .. lane
    pc[m] = __popcll(rel & upto);
    pc0[m] = __popcll(rel0 & upto);
    if (lane == 0 && r < len) {
      cnt->rel[r >> 6] = __popcll(rel);
      cnt->rel0[r >> 6] = __popcll(rel0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < IPT; ++m) {
    const int r = m * NT + t;
    if (r < len) {
      int n_le = pc[m], n0_le = pc0[m];            // relevant items at positions <= r, at `thr` and at 0
      for (int ch = 0; ch < (r >> 6); ++ch) { n_le += cnt->rel[ch]; n0_le += cnt->rel0[ch]; }
      const bool rel = lab[m] > thr;
      const double disc = log(2.0 + r);
      const double ideal = d[r];
      a[r] = n0_le / (r + 1.0);                    // AveragePrecision's Precision(r + 1) at the DEFAULT threshold 0 (average_precision.py:41)
      b[r] = rel ? n_le / (r + 1.0) : 0.0;
      c[r] = rel ? rank_gain(lab[m]) / disc : 0.0;
      d[r] = ideal > thr ? rank_gain(ideal) / disc : 0.0;
      if (rel) atomicMin(&cnt->first, r + 1);
      if (r == len - 1) cnt->n_rel = n_le;
      for (int kk = 0; kk < nk; ++kk)
        if (r == min(ks.k[kk], len) - 1) {
          gi[3 + kk] = n_le;
          gd[3 + kk] = n_le / (double)ks.k[kk];
        }
    }
  }
  __syncthreads();
  // ---- 4 sums, one owning wave each: AP, MAP, then per k the pair DCG / IDCG
  if (live) {
    const int n_rel = cnt->n_rel;
    constexpr int OWNERS = NT / 64;
    for (int q = t >> 6; q < 2 + nk; q += OWNERS) {
      if (q == 0) {
        const double s = strided_sum(a, len, lane);
        if (lane == 0) gd[0] = len ? s / len : 0.0;
      } else if (q == 1) {
        const double s = strided_sum(b, len, lane);
        if (lane == 0) gd[1] = n_rel ? s / n_rel : 0.0;
      } else {
        const int kk = q - 2, lim = min(ks.k[kk], len);
        const double dcg = strided_sum(c, lim, lane), idcg = strided_sum(d, lim, lane);
        if (lane == 0) {
          gd[3 + nk + kk] = dcg;
          gd[3 + 2 * nk + kk] = idcg != 0.0 ? dcg / idcg : 0.0;
        }
      }
    }
    if (t == 0) {
      const int first = cnt->first == INT_MAX ? 0 : cnt->first;
      gi[0] = len;
      gi[1] = n_rel;
      gi[2] = first;
      gd[2] = first ? 1.0 / first : 0.0;
      if (len == 0)
        for (int kk = 0; kk < nk; ++kk) { gi[3 + kk] = 0; gd[3 + kk] = 0.0; }
    }
  }
}

// offsets[q], offsets[q + 1] of a group the kernel may touch: inside [0, n], ordered, at most RK_MAX apart.  The entry point has
// checked the host copy already; this keeps every access in bounds should the device copy differ from it.
__device__ __forceinline__ bool group_bounds(const int32_t* __restrict__ offsets, int q, int g, int n, int* base, int* len) {
  if (q >= g) return false;
  const int o0 = offsets[q], o1 = offsets[q + 1];
  if (o0 < 0 || o1 < o0 || o1 > n || o1 - o0 > RK_MAX) return false;
  *base = o0;
  *len = o1 - o0;
  return true;
}

__global__ __launch_bounds__(RK_BLOCK) void rank_metrics_kernel(const void* __restrict__ scores, int f64, const double* __restrict__ labels,
                                                                const int32_t* __restrict__ offsets, int n, int g, double thr, RankKs ks, int nk,
                                                                int32_t* __restrict__ rank, int32_t* __restrict__ gi, double* __restrict__ gd,
                                                                unsigned int* __restrict__ nan_count) {
  __shared__ double ta[RK_MAX], tb[RK_MAX], tc[RK_MAX], td[RK_MAX];
  __shared__ RankCounts cnt[RK_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int ni = 3 + nk, nd = 3 + 3 * nk;
  unsigned nan_s = 0, nan_l = 0;
  const int wave_blocks = (g + RK_WAVES - 1) / RK_WAVES;
  if ((int)blockIdx.x < wave_blocks) {
    // ---- wave path: the short groups among this workgroup's four, side by side
    const int q = blockIdx.x * RK_WAVES + wave;
    int base = 0, len = 0;
    const bool live = group_bounds(offsets, q, g, n, &base, &len) && len <= RK_WAVE_LEN;
    if (!live) len = 0;
    const int off = wave * RK_WAVE_LEN;
    rank_group<64>(scores, f64, labels, base, len, live, thr, ks, nk, tid & 63, ta + off, tb + off, tc + off, td + off, &cnt[wave], rank,
                   gi + (size_t)(live ? q : 0) * ni, gd + (size_t)(live ? q : 0) * nd, &nan_s, &nan_l);
  } else {
    // ---- workgroup path: this workgroup's one group, if it is a long one (the condition is the same for every thread)
    const int q = blockIdx.x - wave_blocks;
    int base = 0, len = 0;
    if (!group_bounds(offsets, q, g, n, &base, &len) || len <= RK_WAVE_LEN) return;
    rank_group<RK_BLOCK>(scores, f64, labels, base, len, true, thr, ks, nk, tid, ta, tb, tc, td, &cnt[0], rank, gi + (size_t)q * ni,
                         gd + (size_t)q * nd, &nan_s, &nan_l);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nan_s += __shfl_xor(nan_s, o, 64);
    nan_l += __shfl_xor(nan_l, o, 64);
  }
  if ((tid & 63) == 0) {
    if (nan_s) atomicAdd(&nan_count[0], nan_s);
    if (nan_l) atomicAdd(&nan_count[1], nan_l);
  }
}

// ------------------------------------------------------------------------------------------------ losses
constexpr int RL_BLOCK = 256;
constexpr int RL_WAVES = RL_BLOCK / 64;

// entry e = r * c + j of instance b's rows r0 .. : row (b (num_neg + 1) + r0 + r), column j
__device__ __forceinline__ size_t inst_at(int b, int per, int r0, int e, int c, int ld) {
  return ((size_t)b * per + r0 + e / c) * ld + e % c;
}

__global__ __launch_bounds__(RL_BLOCK) void rank_hinge_fwd_kernel(const float* __restrict__ y, int ld, int nb, int num_neg, int c, float margin,
                                                                  float* __restrict__ neg_mean, float* __restrict__ elem, float* __restrict__ part) {
  const int b = blockIdx.x * RL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nb) return;
  const int per = num_neg + 1, count = num_neg * c;
  float acc = 0.f;
  for (int e = lane; e < count; e += 64) acc += y[inst_at(b, per, 1, e, c, ld)];
  const float nm = wave_sum(acc) / (float)count;
  acc = 0.f;
  for (int j = lane; j < c; j += 64) {
    const float v = fmaxf(margin - (y[inst_at(b, per, 0, j, c, ld)] - nm), 0.f);
    if (elem) elem[(size_t)b * c + j] = v;
    acc += v;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    neg_mean[b] = nm;
    if (part) part[b] = acc;
  }
}

// g_elem [nb][c] (reduction 'none') or g_one[0] * scale for every element
__global__ __launch_bounds__(RL_BLOCK) void rank_hinge_bwd_kernel(const float* __restrict__ y, int ld, int nb, int num_neg, int c, float margin,
                                                                  const float* __restrict__ neg_mean, const float* __restrict__ g_elem,
                                                                  const float* __restrict__ g_one, float scale, float* __restrict__ dy) {
  const int b = blockIdx.x * RL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nb) return;
  const int per = num_neg + 1, count = num_neg * c;
  const float nm = neg_mean[b];
  const float g1 = g_elem ? 0.f : g_one[0] * scale;
  float acc = 0.f;
  for (int j = lane; j < c; j += 64) {
    // the forward's expression again, bit for bit; clamp_min passes the gradient where its input is >= 0
    const float v = margin - (y[inst_at(b, per, 0, j, c, ld)] - nm);
    const float ge = g_elem ? g_elem[(size_t)b * c + j] : g1;
    const float m = v >= 0.f ? ge : 0.f;
    dy[inst_at(b, per, 0, j, c, c)] = -m;
    acc += m;
  }
  const float dneg = wave_sum(acc) / (float)count;
  for (int e = lane; e < count; e += 64) dy[inst_at(b, per, 1, e, c, c)] = dneg;
}

__global__ __launch_bounds__(RL_BLOCK) void rank_ce_fwd_kernel(const float* __restrict__ y, int ld, const float* __restrict__ yt, int ldt, int nb,
                                                               int num_neg, int c, float* __restrict__ lse, float* __restrict__ part) {
  const int b = blockIdx.x * RL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nb) return;
  const int per = num_neg + 1, width = per * c;
  float mx = -INFINITY;
  for (int e = lane; e < width; e += 64) mx = fmaxf(mx, y[inst_at(b, per, 0, e, c, ld)]);
  mx = wave_max(mx);
  float acc = 0.f;
  for (int e = lane; e < width; e += 64) acc += expf(y[inst_at(b, per, 0, e, c, ld)] - mx);
  const float l = mx + logf(wave_sum(acc));
  acc = 0.f;
  for (int e = lane; e < width; e += 64) acc += yt[inst_at(b, per, 0, e, c, ldt)] * (y[inst_at(b, per, 0, e, c, ld)] - l);
  acc = wave_sum(acc);
  if (lane == 0) {
    lse[b] = l;
    part[b] = -acc;
  }
}

__global__ __launch_bounds__(RL_BLOCK) void rank_ce_bwd_kernel(const float* __restrict__ y, int ld, const float* __restrict__ yt, int ldt, int nb,
                                                               int num_neg, int c, const float* __restrict__ lse, const float* __restrict__ g_one,
                                                               float* __restrict__ dy) {
  const int b = blockIdx.x * RL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nb) return;
  const int per = num_neg + 1, width = per * c;
  float acc = 0.f;
  for (int e = lane; e < width; e += 64) acc += yt[inst_at(b, per, 0, e, c, ldt)];
  const float lab_sum = wave_sum(acc), l = lse[b], ge = g_one[0] / (float)nb;
  for (int e = lane; e < width; e += 64)
    dy[inst_at(b, per, 0, e, c, c)] = ge * (lab_sum * expf(y[inst_at(b, per, 0, e, c, ld)] - l) - yt[inst_at(b, per, 0, e, c, ldt)]);
}

// out[0] = scale * sum(part[0 .. count)): one workgroup, thread t adds t, t + 256, ... in order, butterflies, then the four wave sums
__global__ __launch_bounds__(RL_BLOCK) void rank_total_kernel(const float* __restrict__ part, int count, float scale, float* __restrict__ out) {
  __shared__ float waves[RL_WAVES];
  float acc = 0.f;
  for (int i = threadIdx.x; i < count; i += RL_BLOCK) acc += part[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((waves[0] + waves[1]) + (waves[2] + waves[3])) * scale;
}

int loss_shape(const char* who, const void* y, int ld, int rows, int c, int num_neg, int min_neg) {
  GH_REQUIRE(y, "%s: NULL argument", who);
  GH_REQUIRE(c >= 1 && ld >= c, "%s: c = %d, ld = %d (1 <= c <= ld)", who, c, ld);
  GH_REQUIRE(num_neg >= min_neg && num_neg <= GH_RANK_MAX_NEG, "%s: num_neg = %d outside [%d, %d]", who, num_neg, min_neg, GH_RANK_MAX_NEG);
  GH_REQUIRE(rows >= 1 && rows <= GH_RANK_MAX_ROWS, "%s: rows = %d outside [1, %d]", who, rows, GH_RANK_MAX_ROWS);
  GH_REQUIRE(rows % (num_neg + 1) == 0, "%s: rows = %d is no multiple of num_neg + 1 = %d", who, rows, num_neg + 1);
  GH_REQUIRE((long long)(num_neg + 1) * c <= INT_MAX, "%s: (num_neg + 1) c = %lld does not fit an int", who, (long long)(num_neg + 1) * c);
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_rank_metrics(const void* scores, int scores_f64, const double* labels, const int32_t* offsets, const int32_t* offsets_host,
                               int n, int g, double threshold, const int32_t* ks, int nk, int32_t* rank, int32_t* group_int, double* group_f64,
                               int32_t* nan_count, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(g >= 1 && g <= GH_RANK_MAX_GROUPS, "rank_metrics: g = %d outside [1, %d]", g, GH_RANK_MAX_GROUPS);
  GH_REQUIRE(n >= 0 && n <= GH_RANK_MAX_ITEMS, "rank_metrics: n = %d outside [0, %d]", n, GH_RANK_MAX_ITEMS);
  GH_REQUIRE(nk >= 1 && nk <= GH_RANK_MAX_KS, "rank_metrics: nk = %d outside [1, %d]", nk, GH_RANK_MAX_KS);
  GH_REQUIRE(offsets && offsets_host && ks && group_int && group_f64 && nan_count, "rank_metrics: NULL argument");
  GH_REQUIRE(n == 0 || (scores && labels && rank), "rank_metrics: NULL argument");
  GH_REQUIRE(threshold == threshold, "rank_metrics: threshold is NaN");
  RankKs kv;
  for (int i = 0; i < RK_MAX_KS; ++i) kv.k[i] = 1;
  for (int i = 0; i < nk; ++i) {
    GH_REQUIRE(ks[i] >= 1, "rank_metrics: ks[%d] = %d < 1", i, ks[i]);
    kv.k[i] = ks[i];
  }
  GH_REQUIRE(offsets_host[0] == 0 && offsets_host[g] == n, "rank_metrics: offsets run from %d to %d, not from 0 to n = %d", offsets_host[0],
             offsets_host[g], n);
  for (int q = 0; q < g; ++q) {
    const long long len = (long long)offsets_host[q + 1] - offsets_host[q];
    GH_REQUIRE(len >= 0, "rank_metrics: offsets decrease at group %d", q);
    GH_REQUIRE(len <= GH_RANK_MAX_GROUP, "rank_metrics: group %d holds %lld items, more than %d", q, len, GH_RANK_MAX_GROUP);
  }
  GH_CHECK_HIP(hipMemsetAsync(nan_count, 0, 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(rank_metrics_kernel, dim3((g + RK_WAVES - 1) / RK_WAVES + g), dim3(RK_BLOCK), 0, st, scores, scores_f64 ? 1 : 0, labels, offsets, n, g,
                     threshold, kv, nk, rank, group_int, group_f64, reinterpret_cast<unsigned int*>(nan_count));
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_rank_hinge_fwd(const float* y, int ld, int rows, int c, int num_neg, float margin, int reduction, float* neg_mean, float* elem,
                                 float* part, float* loss, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = loss_shape("rank_hinge_fwd", y, ld, rows, c, num_neg, 1)) return rc;
  GH_REQUIRE(reduction >= 0 && reduction <= 2, "rank_hinge_fwd: reduction = %d (0 none, 1 mean, 2 sum)", reduction);
  GH_REQUIRE(neg_mean && (reduction == 0 ? elem != nullptr : (part && loss)), "rank_hinge_fwd: NULL argument");
  const int nb = rows / (num_neg + 1);
  hipLaunchKernelGGL(rank_hinge_fwd_kernel, dim3((nb + RL_WAVES - 1) / RL_WAVES), dim3(RL_BLOCK), 0, st, y, ld, nb, num_neg, c, margin, neg_mean,
                     reduction == 0 ? elem : nullptr, reduction == 0 ? nullptr : part);
  GH_LAUNCH_CHECK();
  if (reduction != 0) {
    const float scale = reduction == 1 ? (float)(1.0 / ((double)nb * c)) : 1.f;
    hipLaunchKernelGGL(rank_total_kernel, dim3(1), dim3(RL_BLOCK), 0, st, part, nb, scale, loss);
    GH_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gh_rank_hinge_bwd(const float* y, int ld, int rows, int c, int num_neg, float margin, int reduction, const float* neg_mean,
                                 const float* g, float* dy, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = loss_shape("rank_hinge_bwd", y, ld, rows, c, num_neg, 1)) return rc;
  GH_REQUIRE(reduction >= 0 && reduction <= 2, "rank_hinge_bwd: reduction = %d (0 none, 1 mean, 2 sum)", reduction);
  GH_REQUIRE(neg_mean && g && dy, "rank_hinge_bwd: NULL argument");
  const int nb = rows / (num_neg + 1);
  const float scale = reduction == 1 ? (float)(1.0 / ((double)nb * c)) : 1.f;
  hipLaunchKernelGGL(rank_hinge_bwd_kernel, dim3((nb + RL_WAVES - 1) / RL_WAVES), dim3(RL_BLOCK), 0, st, y, ld, nb, num_neg, c, margin, neg_mean,
                     reduction == 0 ? g : nullptr, reduction == 0 ? nullptr : g, scale, dy);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_rank_ce_fwd(const float* y, int ld, const float* y_true, int ldt, int rows, int c, int num_neg, float* lse, float* part,
                              float* loss, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = loss_shape("rank_ce_fwd", y, ld, rows, c, num_neg, 0)) return rc;
  GH_REQUIRE(y_true && ldt >= c && lse && part && loss, "rank_ce_fwd: NULL argument or ldt = %d < c = %d", ldt, c);
  const int nb = rows / (num_neg + 1);
  hipLaunchKernelGGL(rank_ce_fwd_kernel, dim3((nb + RL_WAVES - 1) / RL_WAVES), dim3(RL_BLOCK), 0, st, y, ld, y_true, ldt, nb, num_neg, c, lse, part);
  GH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_total_kernel, dim3(1), dim3(RL_BLOCK), 0, st, part, nb, (float)(1.0 / nb), loss);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_rank_ce_bwd(const float* y, int ld, const float* y_true, int ldt, int rows, int c, int num_neg, const float* lse, const float* g,
                              float* dy, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = loss_shape("rank_ce_bwd", y, ld, rows, c, num_neg, 0)) return rc;
  GH_REQUIRE(y_true && ldt >= c && lse && g && dy, "rank_ce_bwd: NULL argument or ldt = %d < c = %d", ldt, c);
  const int nb = rows / (num_neg + 1);
  hipLaunchKernelGGL(rank_ce_bwd_kernel, dim3((nb + RL_WAVES - 1) / RL_WAVES), dim3(RL_BLOCK), 0, st, y, ld, y_true, ldt, nb, num_neg, c, lse, g, dy);
  GH_LAUNCH_CHECK();
  return 0;
}
