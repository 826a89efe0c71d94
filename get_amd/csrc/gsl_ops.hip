// Fused word scorer + GSL top-k, and the top-k alone: one workgroup per graph, the keep set packed by ballot.
#include "../../include/get_hip.h"
#include "device_utils.h"

namespace gh {

// ------------------------------------------------------------------------------------------------
// top-k keep set from R scores held in LDS: rank by counting, ballot packs the 64-node words.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void topk_keep(const float* ss, int R, int k, uint64_t* keep_out, int tid) {
  // one thread per node (R <= 256 = blockDim); wave w produces word w
  bool kept = false;
  if (tid < R) {
    const float si = ss[tid];
    int rank = 0;
    for (int j = 0; j < R; ++j) {
      const float sj = ss[j];
      rank += (sj > si) || (sj == si && j < tid);
    }
    kept = rank < k;
  }
  const unsigned long long m = __ballot(kept);
  const int W = (R + 63) / 64;
  if ((tid & 63) == 0 && (tid >> 6) < W) keep_out[tid >> 6] = m;
}

// word scorer (GGNN 300->1, wrapper.py:167) + GSL top-k (:216-219), one workgroup per graph
__global__ void __launch_bounds__(256)
scorer_gsl_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
                  const int32_t* __restrict__ goff, const float* __restrict__ feat, const float* __restrict__ xs_in,
                  const float* __restrict__ w_p, const float* __restrict__ gate, int R, int H, int k, int pads_collapsed, float* __restrict__ score, uint64_t* __restrict__ keep, unsigned drop_thresh,
                  float drop_scale, unsigned drop_seed, int xs_parts, long long xs_stride) {
  __shared__ float xs[MAX_R];
  __shared__ float ss[MAX_R];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (R + 63) / 64;
  // node-compact layout: real node j < NR sits in feature row goff[g] + j; padding node j >= NR of graph g in row
  // goff[n] + (g*R - goff[g]) + (j - NR)  (all padding rows follow the real rows of the whole batch).  The padding
  // nodes still compete in the top-k with their own (bias- and dropout-driven) scores, as in wrapper.py:216-219.
  const int row0 = goff ? goff[g] : g * R;
  const int NR = goff ? goff[g + 1] - row0 : R;
  // pads_collapsed (evaluation mode: no dropout, so every padding row of the batch is the same vector): all padding
  // nodes read the single representative row goff[n]
  const int pad0 = goff ? goff[gridDim.x] + (pads_collapsed ? 0 : g * R - row0 - NR) : row0;
  // x_j = feat_j . w_p   (proj, no bias)
  const bool v4 = (H % 4 == 0) && ((reinterpret_cast<uintptr_t>(feat) & 15) == 0) && ((reinterpret_cast<uintptr_t>(w_p) & 15) == 0);
  if (xs_in) {      // projection already done by the producing cell's epilogue (gh_ggnn_cell_fwd score_x): one float per node
    if (tid < R) {      // (xs_parts > 1: one partial per column block of a wide cell output, added in block order)
      const unsigned xr = (unsigned)(tid < NR ? row0 + tid : (pads_collapsed ? pad0 : pad0 + tid));
      float v = xs_in[xr];
      for (int pp = 1; pp < xs_parts; ++pp) v += xs_in[(size_t)pp * xs_stride + xr];
      xs[tid] = v;
    }
  } else {
  for (int j = wave; j < R; j += 4) {
    float acc = 0.f;
    const unsigned frow = (unsigned)(j < NR ? row0 + j : (pads_collapsed ? pad0 : pad0 + j));
    const float* fg = feat + (size_t)frow * H;
    if (v4) {
      const float4* fr = reinterpret_cast<const float4*>(fg);
      const float4* wr = reinterpret_cast<const float4*>(w_p);
      for (int c = lane; c < H / 4; c += 64) {
        float4 a = fr[c];
        const float4 b = wr[c];
        if (drop_thresh) a = drop4(a, drop_seed, frow * (unsigned)H + 4u * c, drop_thresh, drop_scale);
        acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
      }
    } else {
      for (int c = lane; c < H; c += 64) {
        float a = fg[c];
        if (drop_thresh) a = drop_hash(drop_seed, frow * (unsigned)H + c) >= drop_thresh ? a * drop_scale : 0.f;
        acc += a * w_p[c];
      }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) xs[j] = acc;
  }
  }
  __syncthreads();
  if (tid < R) {
    const int i = tid;
    float a = 0.f;
    const float di = vals ? 0.f : dinv[(size_t)g * R + i];
    for (int w = 0; w < W; ++w) {
      unsigned long long m = bits[((size_t)g * R + i) * W + w];
      while (m) {
        const int j = (w << 6) + __builtin_ctzll(m);
        m &= m - 1;
        const float wt = vals ? vals[((size_t)g * R + i) * R + j] : di * dinv[(size_t)g * R + j];
        a += wt * xs[j];
      }
    }
    const float x = xs[i];
    const float z = 1.f / (1.f + expf(-((gate[0] * a + gate[1]) + (gate[2] * x + gate[3]))));
    const float r = 1.f / (1.f + expf(-((gate[4] * a + gate[5]) + (gate[6] * x + gate[7]))));
    const float hh = tanhf((gate[8] * a + gate[9]) + (gate[10] * (r * x) + gate[11]));
    const float sc = hh * z + x * (1.f - z);
    ss[i] = sc;
    score[(size_t)g * R + i] = sc;
  }
  __syncthreads();
  topk_keep(ss, R, k, keep + (size_t)g * W, tid);
}

__global__ void __launch_bounds__(256)
gsl_topk_kernel(const float* __restrict__ score, int R, int k, uint64_t* __restrict__ keep) {
  __shared__ float ss[MAX_R];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid < R) ss[tid] = score[(size_t)g * R + tid];
  __syncthreads();
  topk_keep(ss, R, k, keep + (size_t)g * ((R + 63) / 64), tid);
}

}  // namespace gh

using namespace gh;

extern "C" int gh_scorer_gsl(const uint64_t* bits, const float* dinv, const float* vals, const int32_t* goff,
                             int pads_collapsed, const float* feat, const float* score_x, const float* w_p, const float* gate, int n, int r, int h, int k, float* score,
                             uint64_t* keep, float drop_p, uint32_t drop_seed, gh_stream_t stream) {
  return scorer_gsl_impl(bits, dinv, vals, goff, pads_collapsed, feat, score_x, 1, 0, w_p, gate, n, r, h, k, score, keep, drop_p, drop_seed,
                         (hipStream_t)stream);
}

int gh::scorer_gsl_impl(const uint64_t* bits, const float* dinv, const float* vals, const int32_t* goff, int pads_collapsed, const float* feat,
                        const float* score_x, int score_parts, long long score_stride, const float* w_p, const float* gate, int n, int r, int h,
                        int k, float* score, uint64_t* keep, float drop_p, uint32_t drop_seed, hipStream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "scorer_gsl: r=%d not in [1,%d]", r, MAX_R);
  GH_REQUIRE(score_parts >= 1 && score_parts <= 16, "scorer_gsl: %d score partials", score_parts);
  GH_REQUIRE(vals || dinv, "scorer_gsl: need dinv or vals");
  if (n <= 0) return 0;
  prof_begin((hipStream_t)stream, PROF_SCORER_GSL);
  GH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "scorer_gsl: dropout p=%f not in [0,1)", drop_p);
  GH_REQUIRE(!(pads_collapsed && drop_p > 0.f), "scorer_gsl: collapsed padding rows are an evaluation-mode layout (no dropout)");
  GH_REQUIRE(drop_p <= 0.f || (long long)n * r * (long long)h < (1LL << 32), "scorer_gsl: %d rows x %d columns exceed the dropout mask's 32-bit element index", n * r, h);
  const double th = (double)drop_p * 4294967296.0;
  const unsigned thresh = drop_p > 0.f ? (th >= 4294967295.0 ? 4294967295u : (unsigned)th) : 0u;
  GH_REQUIRE((feat != nullptr) != (score_x != nullptr), "scorer_gsl: exactly one of feat / score_x");
  hipLaunchKernelGGL(scorer_gsl_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, bits, dinv, vals, goff, feat, score_x,
                     w_p, gate, r, h, k, (goff && pads_collapsed) ? 1 : 0, score, keep, thresh, 1.0f / (1.0f - drop_p), drop_seed,
                     score_parts, score_stride);
  prof_end(PROF_SCORER_GSL, (double)n * ((feat ? 4.0 * r * h : 4.0 * r) + 8.0 * r * words_for(r) + 8.0 * r + 8.0 * words_for(r)),
           (hipStream_t)stream);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_gsl_topk(const float* score, int n, int r, int k, uint64_t* keep, gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "gsl_topk: r=%d not in [1,%d]", r, MAX_R);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(gsl_topk_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, score, r, k, keep);
  GH_LAUNCH_CHECK();
  return 0;
}
