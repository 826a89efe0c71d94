// Kernels that run once per step over the parameters: the weight transposes with their optional bf16 twins (gh_transpose,
// gh_transpose_batch, gh_weights_refresh) and the fused flat Adam (gh_adam_step).
#include "../../include/get_hip.h"
#include "common.h"

namespace gh {

// ---------------------------------------------------------------------------- transpose
__global__ void __launch_bounds__(256)
transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int rows, int cols) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    if (r < rows && c < cols) tile[j][tx] = w[(size_t)r * cols + c];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;      // output row = c, output col = r
    if (r < rows && c < cols) wt[(size_t)c * rows + r] = tile[tx][j];
  }
}

struct TransposeBatch { const float* src[32]; float* dst[32]; int rows[32]; int cols[32]; int tile0[33]; int n;
                        unsigned short* w16[32]; unsigned short* t16[32]; };      // optional bf16 twins of src and of src^T (gh_weights_refresh)
__device__ __forceinline__ unsigned short bf16_rne(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);      // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__global__ void __launch_bounds__(256)
transpose_batch_kernel(const TransposeBatch B) {
  __shared__ float tile[32][33];
  int m = 0;
  while (m + 1 < B.n && (int)blockIdx.x >= B.tile0[m + 1]) ++m;
  const int rows = B.rows[m], cols = B.cols[m];
  const int t = blockIdx.x - B.tile0[m], tx_n = (cols + 31) / 32;
  const int bx = (t % tx_n) * 32, by = (t / tx_n) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* w = B.src[m];
  float* wt = B.dst[m];
  unsigned short* w16 = B.w16[m];
  unsigned short* t16 = B.t16[m];
  // float4-shaped matrices (every weight matrix of the path but the 2-row head): one 16-byte access per thread and direction instead
  // of four 4-byte ones (configs[4]: 86 us per step for the 14 cell matrices, the 41 MB head layer and their bf16 twins)
  const bool vec = rows % 4 == 0 && cols % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(wt)) & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(w16) | reinterpret_cast<uintptr_t>(t16)) & 7) == 0;
  if (vec) {
    const int q8 = threadIdx.x & 7, r8 = threadIdx.x >> 3;      // 32 rows x 8 float4 columns
    {
      const int r = by + r8, c = bx + 4 * q8;
      if (r < rows && c < cols) {
        const float4 v = *reinterpret_cast<const float4*>(w + (size_t)r * cols + c);
        tile[r8][4 * q8 + 0] = v.x; tile[r8][4 * q8 + 1] = v.y; tile[r8][4 * q8 + 2] = v.z; tile[r8][4 * q8 + 3] = v.w;
        if (w16) *reinterpret_cast<uint2*>(w16 + (size_t)r * cols + c) =
            make_uint2((unsigned)bf16_rne(v.x) | ((unsigned)bf16_rne(v.y) << 16), (unsigned)bf16_rne(v.z) | ((unsigned)bf16_rne(v.w) << 16));
      }
    }
    __syncthreads();
    {
      const int c = bx + r8, r = by + 4 * q8;      // output row = source column c, four consecutive source rows
      if (c < cols && r < rows) {
        const float4 v = make_float4(tile[4 * q8 + 0][r8], tile[4 * q8 + 1][r8], tile[4 * q8 + 2][r8], tile[4 * q8 + 3][r8]);
        if (wt) *reinterpret_cast<float4*>(wt + (size_t)c * rows + r) = v;
        if (t16) *reinterpret_cast<uint2*>(t16 + (size_t)c * rows + r) =
            make_uint2((unsigned)bf16_rne(v.x) | ((unsigned)bf16_rne(v.y) << 16), (unsigned)bf16_rne(v.z) | ((unsigned)bf16_rne(v.w) << 16));
      }
    }
    return;
  }
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    if (r < rows && c < cols) {
      const float v = w[(size_t)r * cols + c];
      tile[j][tx] = v;
      if (w16) w16[(size_t)r * cols + c] = bf16_rne(v);
    }
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;
    if (r < rows && c < cols) {
      const float v = tile[tx][j];
      if (wt) wt[(size_t)c * rows + r] = v;
      if (t16) t16[(size_t)c * rows + r] = bf16_rne(v);
    }
  }
}

// ---------------------------------------------------------------------------- flat Adam (torch.optim.Adam, L2 weight decay)
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            size_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float w = p[i];
    const float gr = g[i] * gscale + wd * w;
    const float mi = b1 * m[i] + (1.f - b1) * gr;
    const float vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi; v[i] = vi;
    // torch: denom = sqrt(v)/sqrt(bias_correction2) + eps ; p -= (lr / bias_correction1) * m / denom
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = w - (lr / bc1) * (mi / denom);
  }
}

}  // namespace gh

using namespace gh;

extern "C" int gh_transpose(const float* w, float* wt, int rows, int cols, gh_stream_t stream) {
  GH_REQUIRE(rows > 0 && cols > 0, "transpose: bad sizes %d x %d", rows, cols);
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, (hipStream_t)stream, w,
                     wt, rows, cols);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_weights_refresh(int n, const void* const* src, void* const* dst, void* const* dst_w16, void* const* dst_t16,
                                  const int* rows, const int* cols, gh_stream_t stream) {
  GH_REQUIRE(n >= 0 && (n == 0 || (src && rows && cols)), "weights_refresh: NULL arrays");
  for (int i0 = 0; i0 < n; i0 += 32) {
    TransposeBatch B;
    B.n = (n - i0 < 32) ? n - i0 : 32;
    int tiles = 0;
    for (int i = 0; i < B.n; ++i) {
      GH_REQUIRE(rows[i0 + i] > 0 && cols[i0 + i] > 0 && src[i0 + i], "weights_refresh: bad matrix at %d", i0 + i);
      B.src[i] = (const float*)src[i0 + i]; B.dst[i] = dst ? (float*)dst[i0 + i] : nullptr;
      B.w16[i] = dst_w16 ? (unsigned short*)dst_w16[i0 + i] : nullptr;
      B.t16[i] = dst_t16 ? (unsigned short*)dst_t16[i0 + i] : nullptr;
      B.rows[i] = rows[i0 + i]; B.cols[i] = cols[i0 + i];
      B.tile0[i] = tiles;
      tiles += ((rows[i0 + i] + 31) / 32) * ((cols[i0 + i] + 31) / 32);
    }
    B.tile0[B.n] = tiles;
    hipLaunchKernelGGL(transpose_batch_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, B);
    GH_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gh_transpose_batch(int n, const void* const* src, void* const* dst, const int* rows, const int* cols,
                                  gh_stream_t stream) {
  GH_REQUIRE(n == 0 || dst, "transpose_batch: NULL dst");
  return gh_weights_refresh(n, src, dst, nullptr, nullptr, rows, cols, stream);
}

extern "C" int gh_adam_step(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int step, float grad_scale,
                            gh_stream_t stream) {
  GH_REQUIRE(step >= 1, "adam_step: step=%d must be >= 1", step);
  if (count <= 0) return 0;
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int grid = (int)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
  prof_begin((hipStream_t)stream, PROF_ADAM);
  hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)count, lr, beta1,
                     beta2, eps, weight_decay, bc1, (float)sqrt(bc2), grad_scale);
  prof_end(PROF_ADAM, 28.0 * (double)count, (hipStream_t)stream);
  GH_LAUNCH_CHECK();
  return 0;
}
