// The LDS "score tile" toolkit of the attention files (mha_ops.hip, bidaf_ops.hip, match_ops.hip, pair_ops.hip, bert_ops.hip): one workgroup of
// TILE_THREADS holds a 16-row score tile S [16][n] in LDS, fills it with X Y^T over staged operand chunks and multiplies it
// into a second operand with the accumulators in registers.  Include after device_utils.h.
//
// The products run on v_mfma_f32_16x16x4_f32 (exact fp32) from operands staged in LDS.  Two layouts serve them:
//   KC  element (i, k) at i * pitch + k, pitch % 8 == 4    (pitch_kc; the reduction index k is contiguous: both operands of
//       X Y^T, and the score tile as the left operand of S B)
//   KM  element (k, j) at k * pitch + j, pitch % 32 == 16  (pitch_km; the reduction index is the row: the right operand B,
//       and 16-wide slabs [kk][16] of scores as transposed left operands)
// With those pitches the 64 lanes of an operand read (lane = 16 * (k & 3) + i) fall into 64 different banks.  Rows are
// zero-filled to a multiple of 16 and the depth to a multiple of 4 in LDS, so one code path serves every length and depth; a
// staging load moves 16 bytes per lane where the source rows are 16-byte aligned and whole, and single floats elsewhere.
// C/D lane map of a 16 x 16 tile: column = lane & 15, row = 4 (lane >> 4) + r for r = 0 .. 3 of the lane's f32x4.  Wave w owns
// the 16-column tiles w, w + 4, ... of a product, in every call.
#pragma once
#include "device_utils.h"

namespace gh {

constexpr int TILE_THREADS = 256;        // every kernel that uses this header runs workgroups of 4 waves
constexpr int TILE_WAVES = TILE_THREADS / 64;

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }
// LDS row pitch in floats of an operand whose reduction index is the row: a multiple of 16 that is 16 (mod 32)
__host__ __device__ inline int pitch_km(int n) { n = up16(n); return (n & 31) == 16 ? n : n + 16; }
// rows of a chunk with `pitch` floats per row: a multiple of 16, at least 16, at most the padded extent
__host__ __device__ inline int chunk_rows(int extent, int pitch, int budget) {
  int r = (budget / pitch) & ~15;
  if (r < 16) r = 16;
  const int e = up16(extent);
  return r < e ? r : e;
}

// LDS of a row-tiled kernel that walks its width in blocks of BLK columns: left [16][pa] | ss [16][ps] | chunk of CHUNK floats
// at most.  n = the length the scores run over, w = the widest depth; kc1 / kc2 = the chunk rows of the two products
struct TilePlan { int pa, ps, pk, pv, kc1, kc2, chunk; };
template <int BLK, int CHUNK> __host__ __device__ inline TilePlan tile_plan(int n, int w) {
  TilePlan p;
  p.pa = pitch_kc(imin(up4(w), BLK));
  p.ps = pitch_kc(up16(n));
  p.pk = p.pa;
  p.pv = pitch_km(imin(up16(w), BLK));
  p.kc1 = chunk_rows(n, p.pk, CHUNK);
  p.kc2 = chunk_rows(n, p.pv, CHUNK);
  const int c1 = p.kc1 * p.pk, c2 = p.kc2 * p.pv;
  p.chunk = c1 > c2 ? c1 : c2;
  return p;
}

__device__ __forceinline__ bool vec_ok(const float* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; }

// four floats from p (the first `n` of them exist), 16 bytes at once where `vec`
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, bool vec, int n) {
  if (vec && n >= 4) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}

// LDS [rows_pad][pitch] <- f(r, c) for r < rows, c < cols in steps of four columns, zero elsewhere; cols_pad % 4 == 0.
// f returns the four values of columns c .. c + 3 and must itself return zeros for the columns >= cols, as ld4 does.
template <class F>
__device__ __forceinline__ void stage_f(float* dst, int pitch, int rows_pad, int cols_pad, int rows, int cols, F f) {
  const int c4n = cols_pad >> 2;
  for (int idx = threadIdx.x; idx < rows_pad * c4n; idx += TILE_THREADS) {
    const int r = idx / c4n, c = (idx - r * c4n) << 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows && c < cols) v = f(r, c);
    *reinterpret_cast<float4*>(dst + r * pitch + c) = v;
  }
}

// rows x cols of a row-major source -> LDS [rows_pad][pitch], zero-filled beyond (rows, cols)
__device__ __forceinline__ void stage(float* dst, int pitch, int rows_pad, int cols_pad, const float* __restrict__ src, long long ld,
                                      int rows, int cols) {
  const bool vec = vec_ok(src, ld);
  stage_f(dst, pitch, rows_pad, cols_pad, rows, cols, [=](int r, int c) { return ld4(src + (size_t)r * ld + c, vec, cols - c); });
}

// LDS tile [16][pitch] (only the first `rows` rows and `cols` columns) -> row-major global, 16 bytes per lane where possible
__device__ __forceinline__ void unstage(float* __restrict__ dst, long long ld, const float* src, int pitch, int rows, int cols) {
  if (vec_ok(dst, ld) && (cols & 3) == 0) {
    const int c4n = cols >> 2;
    for (int idx = threadIdx.x; idx < rows * c4n; idx += TILE_THREADS) {
      const int r = idx / c4n, c = (idx - r * c4n) << 2;
      *reinterpret_cast<float4*>(dst + (size_t)r * ld + c) = *reinterpret_cast<const float4*>(src + r * pitch + c);
    }
  } else {
    for (int idx = threadIdx.x; idx < rows * cols; idx += TILE_THREADS) {
      const int r = idx / cols, c = idx - r * cols;
      dst[(size_t)r * ld + c] = src[r * pitch + c];
    }
  }
}

// S[16][key0 + ...] (+)= X Y^T for a chunk: X = xs [16][px] (KC), Y = ys [rows_pad][py] (KC), depth % 4 == 0.  A wave owns the
// same column tiles in every call, so `accumulate` re-reads what the same lane wrote for the previous depth block.
__device__ __forceinline__ void mma_scores(const float* xs, int px, const float* ys, int py, int rows_pad, int depth, float* ss, int ps,
                                           int key0, bool accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int jt = wave; jt < (rows_pad >> 4); jt += TILE_WAVES) {
    const float* xa = xs + l15 * px + qd;
    const float* yb = ys + (jt * 16 + l15) * py + qd;
    float* so = ss + (4 * qd) * ps + key0 + jt * 16 + l15;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc0[r] = so[r * ps];
    }
    int k0 = 0;
    for (; k0 + 8 <= depth; k0 += 8) {      // two accumulators: the dependent-accumulator latency exceeds the issue interval
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0], yb[k0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0 + 4], yb[k0 + 4], acc1, 0, 0, 0);
    }
    if (k0 < depth) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0], yb[k0], acc0, 0, 0, 0);
    acc0 += acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) so[r * ps] = acc0[r];
  }
}

// acc[t] += A B for the column tiles ct = wave + 4 t < ntiles: A element (i, k) at as[i * sai + k * sak], B = bs [kk][pb] (KM)
template <int NT>
__device__ __forceinline__ void mma_acc(const float* as, int sai, int sak, const float* bs, int pb, int kk, int ntiles, f32x4* acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const float* ap = as + l15 * sai + qd * sak;
  const float* bp = bs + qd * pb + wave * 16 + l15;
  for (int k0 = 0; k0 < kk; k0 += 4) {
    const float a = ap[k0 * sak];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (wave + TILE_WAVES * t < ntiles)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[k0 * pb + t * 16 * TILE_WAVES], acc[t], 0, 0, 0);
  }
}

// sum / maximum over the workgroup in a fixed order (lanes by butterfly, then the waves in order); every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < TILE_WAVES; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < TILE_WAVES; ++w) s = fmaxf(s, red[w]);
  return s;
}

// ss [16][ps] (+)= xs ys^T with ys = the `n` rows of `src` (ld), columns k0 .. k0 + nb, walked in chunks of `kc` rows through ch
__device__ __forceinline__ void scores_block(const float* xs, int px, float* ch, int pk, int kc, const float* __restrict__ src, long long ld,
                                             int n, int k0, int nb, float* ss, int ps, bool accumulate) {
  const int nb4 = up4(nb);
  for (int key0 = 0; key0 < n; key0 += kc) {
    const int nk = imin(kc, n - key0), rp = up16(nk);
    __syncthreads();
    stage(ch, pk, rp, nb4, src + (size_t)key0 * ld + k0, ld, nk, nb);
    __syncthreads();
    mma_scores(xs, px, ch, pk, rp, nb4, ss, ps, key0, accumulate);
  }
}

// acc += ss[:, 0:n] B with B = the `n` rows of `src` (ld), columns c0 .. c0 + nb, walked in chunks of `kc` rows through ch
template <int NT>
__device__ __forceinline__ void weighted_block(const float* ss, int ps, float* ch, int pv, int kc, const float* __restrict__ src, long long ld,
                                               int n, int c0, int nb, f32x4* acc) {
  const int nct = (nb + 15) >> 4;
  for (int key0 = 0; key0 < n; key0 += kc) {
    const int nk = imin(kc, n - key0), rp = up4(nk);
    __syncthreads();
    stage(ch, pv, rp, up16(nb), src + (size_t)key0 * ld + c0, ld, nk, nb);
    __syncthreads();
    mma_acc<NT>(ss + key0, ps, 1, ch, pv, rp, nct, acc);
  }
}

}  // namespace gh
