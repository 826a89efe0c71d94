// On-device evaluation: the integers every classification metric of the reference's fitter is an exact function of
// (Fitting/FittingFC/char_man_fitter_query_repr1.py:353,358-362 predictions and scores, :381-401 the sklearn calls).
//   gh_cls_metrics    argmax predictions, the c x c confusion counts and the AUC pair count U2 of logits [n][c] against labels [n]
//
// One kernel on a two-dimensional grid: workgroup (x, y) owns the slab of CM_SLAB = 256 rows i = 256 x + thread and the span
// of CM_SPAN = 4096 rows j = 4096 y ...; it walks its span in LDS tiles of CM_TILE = 1024 scores.  A tile entry is the score
// phi[j][pos_class] of a NEGATIVE row and NaN for every other row (positives, rejected rows, rows beyond n); likewise the
// thread's own score is NaN unless its row is a positive.  An IEEE comparison with a NaN is false, so "i positive and j negative"
// needs no flag and no branch in the inner loop: two compares and two adds per pair, every lane reading the same LDS address
// (a broadcast) 16 bytes at a time.  The workgroups of the first span (y = 0) also write pred and count their slab's rows into
// the confusion matrix and the four row counters.
// Everything is integer arithmetic: 32-bit counters per span (at most 2 * 4096 per thread), widened to 64 bits for the wave and
// workgroup sums, which reach `out` (zeroed by a memset node in front of the launch) as 64-bit INTEGER atomic adds -- a sum of
// integers does not depend on the order of its terms, so the result is exact and the same for every tiling and launch geometry.
// There is no scratch buffer and no state between calls.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include <math.h>

namespace gh {
namespace {

constexpr int CM_SLAB = 256;             // rows i of a workgroup, one per thread (wave64 x 4)
constexpr int CM_TILE = 1024;            // scores j of one LDS tile (4 KB)
constexpr int CM_SPAN = 4096;            // rows j of a workgroup: n = 780 (one validation pass) is 4 workgroups, n = 65 536 is 4096
constexpr int CM_MAX_C = GH_CLS_MAX_CLASSES;
constexpr int CM_EXTRA = 8;              // out slots behind the confusion matrix
static_assert(CM_SPAN % CM_TILE == 0 && CM_TILE % CM_SLAB == 0 && CM_TILE % 16 == 0, "tile arithmetic");

enum RowKind : int { ROW_NEG = 0, ROW_POS = 1, ROW_BAD_LABEL = 2, ROW_NAN = 3 };

__device__ __forceinline__ long long load_label(const void* labels, int i64, int i) {
  return i64 ? static_cast<const long long*>(labels)[i] : (long long)static_cast<const int*>(labels)[i];
}

// Kind of row i (< n) and its score; *arg = torch.argmax of the row (first index among equal maxima; a NaN counts as the
// maximum, the first NaN wins), *label = its label when that lies in [0, c).  A label outside [0, c) is tested first: such a row
// is left out of the NaN count as well.
__device__ __forceinline__ int classify_row(const float* __restrict__ phi, int ldphi, const void* labels, int i64, int i, int c,
                                            int pos_class, float* score, int* arg, int* label) {
  const float* row = phi + (size_t)i * ldphi;
  float best = row[0];
  int at = 0;
  bool nan = best != best;
  float s = best;
  for (int k = 1; k < c; ++k) {
    const float v = row[k];
    if (k == pos_class) s = v;
    if (!(best != best) && (v > best || v != v)) { best = v; at = k; }
    nan |= v != v;
  }
  *score = s;
  *arg = at;
  const long long y = load_label(labels, i64, i);
  if (y < 0 || y >= c) return ROW_BAD_LABEL;
  *label = (int)y;
  if (nan) return ROW_NAN;
  return (int)y == pos_class ? ROW_POS : ROW_NEG;
}

__global__ __launch_bounds__(CM_SLAB) void cls_metrics_kernel(const float* __restrict__ phi, int ldphi, const void* __restrict__ labels,
                                                              int labels_i64, int n, int c, int pos_class, int32_t* __restrict__ pred,
                                                              unsigned long long* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tile[CM_TILE];
  __shared__ unsigned int counts[CM_MAX_C * CM_MAX_C + CM_EXTRA];
  __shared__ unsigned long long wave_u2[CM_SLAB / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * CM_SLAB + tid;
  const bool first_span = blockIdx.y == 0;
  const int cc = c * c;
  if (first_span) {
    for (int k = tid; k < cc + CM_EXTRA; k += CM_SLAB) counts[k] = 0;
    __syncthreads();
  }
  // ---- this thread's row
  float si = __builtin_nanf("");
  if (i < n) {
    float s;
    int arg, label = 0;
    const int kind = classify_row(phi, ldphi, labels, labels_i64, i, c, pos_class, &s, &arg, &label);
    if (kind == ROW_POS) si = s;
    if (first_span) {
      if (pred) pred[i] = arg;
      if (kind == ROW_POS || kind == ROW_NEG) {
        atomicAdd(&counts[label * c + arg], 1u);
        atomicAdd(&counts[cc + (kind == ROW_POS ? 1 : 2)], 1u);
      } else {
        atomicAdd(&counts[cc + (kind == ROW_BAD_LABEL ? 3 : 4)], 1u);
      }
    }
  }
  // ---- the span of j rows, tile by tile
  const int j_begin = blockIdx.y * CM_SPAN;
  const int j_end = min(n, j_begin + CM_SPAN);
  unsigned int gt = 0, eq = 0;
  for (int j0 = j_begin; j0 < j_end; j0 += CM_TILE) {
    __syncthreads();          // the previous tile has been read (and, the first time, `counts` has been updated)
    for (int t = tid; t < CM_TILE; t += CM_SLAB) {
      const int j = j0 + t;
      float sj = __builtin_nanf("");
      if (j < j_end) {
        float s;
        int arg, label;
        if (classify_row(phi, ldphi, labels, labels_i64, j, c, pos_class, &s, &arg, &label) == ROW_NEG) sj = s;
      }
      tile[t] = sj;
    }
    __syncthreads();
    if (__any(si == si)) {        // a wave without a positive row has nothing to count
      // 16 scores a step, the four 16-byte reads issued ahead of the compares: at one validation pass (n = 780, four
      // workgroups, one wave per SIMD) nothing else hides the LDS latency.  Entries up to the tile's end hold NaN.
      const int len = (min(CM_TILE, j_end - j0) + 15) & ~15;
      const f32x4* tile4 = reinterpret_cast<const f32x4*>(tile);
      for (int t = 0; t < len / 4; t += 4) {
        const f32x4 v[4] = {tile4[t], tile4[t + 1], tile4[t + 2], tile4[t + 3]};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          gt += (si > v[q].x) + (si > v[q].y) + (si > v[q].z) + (si > v[q].w);
          eq += (si == v[q].x) + (si == v[q].y) + (si == v[q].z) + (si == v[q].w);
        }
      }
    }
  }
  // ---- sums: 64-bit from here on
  unsigned long long u2 = 2ull * gt + eq;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u2 += __shfl_xor(u2, o, 64);
  if ((tid & 63) == 0) wave_u2[tid >> 6] = u2;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
    for (int w = 0; w < CM_SLAB / 64; ++w) total += wave_u2[w];
    if (total) atomicAdd(&out[cc], total);
  }
  if (first_span)
    for (int k = tid; k < cc + CM_EXTRA; k += CM_SLAB)
      if (k != cc && counts[k]) atomicAdd(&out[k], (unsigned long long)counts[k]);
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_cls_metrics(const float* phi, int ldphi, const void* labels, int labels_i64, int n, int c, int pos_class,
                              int32_t* pred, int64_t* out, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(c >= 2 && c <= GH_CLS_MAX_CLASSES, "cls_metrics: c = %d outside [2, %d]", c, GH_CLS_MAX_CLASSES);
  GH_REQUIRE(n >= 1 && n <= GH_CLS_MAX_ROWS, "cls_metrics: n = %d outside [1, %d]", n, GH_CLS_MAX_ROWS);
  GH_REQUIRE(phi && labels && out, "cls_metrics: NULL argument");
  GH_REQUIRE(ldphi >= c, "cls_metrics: ldphi = %d < c = %d", ldphi, c);
  GH_REQUIRE(pos_class >= 0 && pos_class < c, "cls_metrics: pos_class = %d outside [0, %d)", pos_class, c);
  GH_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)(c * c + CM_EXTRA), st));
  const dim3 grid((n + CM_SLAB - 1) / CM_SLAB, (n + CM_SPAN - 1) / CM_SPAN);
  hipLaunchKernelGGL(cls_metrics_kernel, grid, dim3(CM_SLAB), 0, st, phi, ldphi, labels, labels_i64 ? 1 : 0, n, c, pos_class, pred,
                     reinterpret_cast<unsigned long long*>(out));
  GH_LAUNCH_CHECK();
  return 0;
}
