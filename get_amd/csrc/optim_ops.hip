// The BERT fine-tuning optimiser on the flat bucket (pytorch_transformers/optimization.py): the global gradient norm without
// floating-point atomics (gh_flat_grad_norm) and AdamW with per-parameter hyperparameters, clipping and skipped parameters in
// one launch (gh_adamw_step).  See include/get_hip.h for the contract of the entry points.
#include "../../include/get_hip.h"
#include "common.h"

// The header states the order and the rounding of every fp32 operation of both kernels (a host restatement in fp32 gives the same
// bits: tests/test_gpu_optim_paths.py), so nothing in this file may be contracted into an FMA; sqrtf and / are the correctly
// rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt; the Makefile passes no fast-math flag).
#pragma clang fp contract(off)

namespace gh {

// ---------------------------------------------------------------------------- global gradient norm
// One workgroup per GH_NORM_CHUNK elements, whatever the device: the number of partials and the order of every addition are a
// function of `count` alone.  A lane adds the squares of its float4s in fp32 in ascending address order (GH_NORM_CHUNK / 1024 = 32
// of them, 128 squares); the 256 lane sums are combined in double: a butterfly over the 64 lanes of a wave, then the four wave
// sums in wave order.
constexpr int NORM_THREADS = 256;
static_assert(GH_NORM_CHUNK % (NORM_THREADS * 4) == 0, "a chunk is a whole number of float4 rounds of the workgroup");

__global__ void __launch_bounds__(NORM_THREADS)
grad_sq_partials_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
  __shared__ double wave_sum[NORM_THREADS / 64];
  const size_t base = (size_t)blockIdx.x * GH_NORM_CHUNK;
  const size_t end = base + GH_NORM_CHUNK < n ? base + GH_NORM_CHUNK : n;
  float acc = 0.f;
  for (size_t i = base + 4 * (size_t)threadIdx.x; i < end; i += 4 * NORM_THREADS) {
    if (i + 4 <= end) {
      const float4 x = *reinterpret_cast<const float4*>(g + i);
      acc = acc + x.x * x.x;
      acc = acc + x.y * x.y;
      acc = acc + x.z * x.z;
      acc = acc + x.w * x.w;
    } else {      // the last, short float4 of a count that is no multiple of 4
      for (size_t j = i; j < end; ++j) acc = acc + g[j] * g[j];
    }
  }
  double s = (double)acc;
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// One workgroup: lane t sums the partials [t * per, (t + 1) * per), per = ceil(n_partials / 256), in index order; lane 0 then
// sums the 256 lane sums in lane order.  All in double; the root and the scale too.
__global__ void __launch_bounds__(NORM_THREADS)
grad_norm_final_kernel(const double* __restrict__ partials, long long n_partials, float grad_scale, float* __restrict__ norm_out) {
  __shared__ double lane_sum[NORM_THREADS];
  const long long per = (n_partials + NORM_THREADS - 1) / NORM_THREADS;
  const long long lo = per * threadIdx.x, hi = lo + per < n_partials ? lo + per : n_partials;
  double s = 0.0;
  for (long long i = lo; i < hi; ++i) s += partials[i];
  lane_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int t = 0; t < NORM_THREADS; ++t) total += lane_sum[t];
    norm_out[0] = (float)((double)grad_scale * sqrt(total));
  }
}

// ---------------------------------------------------------------------------- AdamW under a segment table
// A lane owns one float4; 16 lanes share a 64-element block and its segment.  Grid capped at ADAMW_GRID_CAP workgroups with a
// grid-stride loop: one pass covers ADAMW_GRID_CAP * 256 * 4 = 2 097 152 elements.
constexpr int ADAMW_THREADS = 256;
constexpr int ADAMW_GRID_CAP = 2048;
static_assert(sizeof(gh_adamw_seg) == 32, "two float4 loads per segment entry");

// Every operation is one fp32 rounding (contraction is off for this file), in the order the header states: two launches on the
// same inputs, and the clipped and unclipped step at clip = 1, agree bit for bit, and with an fp32 host restatement.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const gh_adamw_seg& s, float gscale, float clip) {
  const float gr = (g * gscale) * clip;
  m = s.beta1 * m + s.one_minus_beta1 * gr;
  v = s.beta2 * v + (s.one_minus_beta2 * gr) * gr;
  const float denom = sqrtf(v) + s.eps;
  const float p1 = p - (s.step_size * m) / denom;
  p = s.lr_wd > 0.f ? p1 - s.lr_wd * p1 : p1;
}

__global__ void __launch_bounds__(ADAMW_THREADS)
adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n4,
             const uint16_t* __restrict__ block_seg, const gh_adamw_seg* __restrict__ table, unsigned n_seg, float gscale,
             const float* __restrict__ norm, float max_norm) {
  float clip = 1.f;
  if (norm != nullptr) {
    const float nv = norm[0];
    if (nv > max_norm) clip = fminf(1.f, max_norm / (nv + 1e-6f));      // at or below max_norm: exactly 1
  }
  for (size_t q = (size_t)blockIdx.x * ADAMW_THREADS + threadIdx.x; q < n4; q += (size_t)gridDim.x * ADAMW_THREADS) {
    const unsigned id = block_seg[q >> 4];
    if (id >= n_seg) continue;                    // a bad map never reads outside the table
    const float4 lo = reinterpret_cast<const float4*>(table + id)[0], hi = reinterpret_cast<const float4*>(table + id)[1];
    gh_adamw_seg s;
    s.step_size = lo.x; s.lr_wd = lo.y; s.beta1 = lo.z; s.beta2 = lo.w;
    s.eps = hi.x; s.one_minus_beta1 = hi.y; s.one_minus_beta2 = hi.z; s.skip = __builtin_bit_cast(int32_t, hi.w);
    if (s.skip != 0) continue;                    // nothing of a skipped block is read or written
    float4 pw = reinterpret_cast<float4*>(p)[q], mw = reinterpret_cast<float4*>(m)[q], vw = reinterpret_cast<float4*>(v)[q];
    const float4 gw = reinterpret_cast<const float4*>(g)[q];
    adamw_element(pw.x, gw.x, mw.x, vw.x, s, gscale, clip);
    adamw_element(pw.y, gw.y, mw.y, vw.y, s, gscale, clip);
    adamw_element(pw.z, gw.z, mw.z, vw.z, s, gscale, clip);
    adamw_element(pw.w, gw.w, mw.w, vw.w, s, gscale, clip);
    reinterpret_cast<float4*>(m)[q] = mw;
    reinterpret_cast<float4*>(v)[q] = vw;
    reinterpret_cast<float4*>(p)[q] = pw;
  }
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace gh

using namespace gh;

extern "C" int gh_flat_grad_norm_partials(int64_t count, int64_t* out_host) {
  GH_REQUIRE(out_host != nullptr, "flat_grad_norm_partials: NULL out");
  GH_REQUIRE(count >= 0, "flat_grad_norm_partials: count=%lld is negative", (long long)count);
  out_host[0] = (count + GH_NORM_CHUNK - 1) / GH_NORM_CHUNK;
  return 0;
}

extern "C" int gh_flat_grad_norm(const float* g, int64_t count, float grad_scale, double* partials, int64_t n_partials,
                                 float* norm_out, gh_stream_t stream) {
  GH_REQUIRE(count >= 0, "flat_grad_norm: count=%lld is negative", (long long)count);
  GH_REQUIRE(norm_out != nullptr, "flat_grad_norm: NULL norm_out");
  const int64_t need = (count + GH_NORM_CHUNK - 1) / GH_NORM_CHUNK;
  GH_REQUIRE(need <= 0x7fffffff, "flat_grad_norm: count=%lld needs more partials than a grid has workgroups", (long long)count);
  GH_REQUIRE(n_partials >= need, "flat_grad_norm: %lld partials, count=%lld needs %lld (gh_flat_grad_norm_partials)",
             (long long)n_partials, (long long)count, (long long)need);
  GH_REQUIRE(need == 0 || (g != nullptr && partials != nullptr), "flat_grad_norm: NULL gradient or partials");
  GH_REQUIRE(aligned16(g) && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
             "flat_grad_norm: the gradient must be 16-byte and the partials 8-byte aligned");
  if (need > 0) {
    hipLaunchKernelGGL(grad_sq_partials_kernel, dim3((unsigned)need), dim3(NORM_THREADS), 0, (hipStream_t)stream, g, (size_t)count,
                       partials);
    GH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, partials, (long long)need, grad_scale,
                     norm_out);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_adamw_step(float* p, const float* g, float* m, float* v, int64_t count, const uint16_t* block_seg,
                             const gh_adamw_seg* seg_table, int n_seg, float grad_scale, const float* norm, float max_norm,
                             gh_stream_t stream) {
  GH_REQUIRE(count >= 0 && count % GH_ADAMW_BLOCK == 0, "adamw_step: count=%lld is not a multiple of %d", (long long)count,
             GH_ADAMW_BLOCK);
  GH_REQUIRE(n_seg >= 0 && n_seg <= GH_ADAMW_MAX_SEGMENTS, "adamw_step: a table of %d segments; the 16-bit block ids name at most %d",
             n_seg, GH_ADAMW_MAX_SEGMENTS);
  if (count == 0) return 0;
  GH_REQUIRE(p && g && m && v && block_seg, "adamw_step: NULL buffer");
  GH_REQUIRE(n_seg == 0 || seg_table, "adamw_step: NULL segment table");
  GH_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "adamw_step: p, g, m and v must be 16-byte aligned");
  GH_REQUIRE(aligned16(seg_table) && (reinterpret_cast<uintptr_t>(block_seg) & 1) == 0,
             "adamw_step: the segment table must be 16-byte and the block map 2-byte aligned");
  GH_REQUIRE(norm == nullptr || max_norm > 0.f, "adamw_step: max_norm=%g must be positive when a norm is given", (double)max_norm);
  const size_t n4 = (size_t)count / 4;
  const size_t blocks = (n4 + ADAMW_THREADS - 1) / ADAMW_THREADS;
  const int grid = (int)(blocks < (size_t)ADAMW_GRID_CAP ? blocks : (size_t)ADAMW_GRID_CAP);
  prof_begin((hipStream_t)stream, PROF_ADAM);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(ADAMW_THREADS), 0, (hipStream_t)stream, p, g, m, v, n4, block_seg, seg_table,
                     (unsigned)n_seg, grad_scale, norm, max_norm);
  prof_end(PROF_ADAM, 28.0 * (double)count, (hipStream_t)stream);
  GH_LAUNCH_CHECK();
  return 0;
}
