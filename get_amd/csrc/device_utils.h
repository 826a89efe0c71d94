// Device helpers with one copy for every kernel file: wave and 16-lane reductions, the bf16 pack / widen of the bf16 storage
// pipeline, the stateless dropout hash, the fast sigmoid / tanh, round-up and LDS-pitch arithmetic and the alignment test of the
// float4 paths.  Included by the GEMM kernels (gemm.hip.h, and through it gemm_ops.hip,
// cell_ops.hip, dense_ops.hip), the core streaming files (spmm_ops.hip, gsl_ops.hip, stream_ops.hip, concat_att_ops.hip, eval_ops.hip) and
// the drop-in kernel files (attention_ops.hip, encoder_ops.hip, mha_ops.hip, rnn_ops.hip, bidaf_ops.hip, match_ops.hip, pair_ops.hip, embed_ops.hip, bert_ops.hip).
// score_tile.hip.h builds on it: the LDS staging and MFMA helpers of the five files that keep a 16-row score tile in LDS
// (mha_ops.hip, bidaf_ops.hip, match_ops.hip, pair_ops.hip, bert_ops.hip).
#pragma once
#include "common.h"

namespace gh {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// stateless dropout: element idx of a tensor is kept iff drop_hash(seed, idx) >= thresh, and then scaled by 1/(1-p)
__host__ __device__ __forceinline__ unsigned drop_hash(unsigned seed, unsigned idx) {
  unsigned x = idx * 0x9E3779B1u + seed;
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float4 drop4(float4 v, unsigned seed, unsigned idx, unsigned thresh, float scale) {
  v.x = drop_hash(seed, idx + 0) >= thresh ? v.x * scale : 0.f;
  v.y = drop_hash(seed, idx + 1) >= thresh ? v.y * scale : 0.f;
  v.z = drop_hash(seed, idx + 2) >= thresh ? v.z * scale : 0.f;
  v.w = drop_hash(seed, idx + 3) >= thresh ? v.w * scale : 0.f;
  return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
  // tanh(x) = 1 - 2/(exp(2x)+1); exact to ~1e-7 abs, saturates cleanly for |x| large
  float e = __expf(2.0f * x);
  return 1.0f - 2.0f / (e + 1.0f);
}

// bf16 storage pipeline: two floats -> two bf16 in one word (v_cvt_pk_bf16_f32, RNE), four bf16 (8 bytes) <-> float4
__device__ __forceinline__ unsigned pack_bf2(float a, float b) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ float4 bf4_to_f4(uint2 u) {
  return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
}
__device__ __forceinline__ uint2 f4_to_bf4(float4 v) { return make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)); }

// 64-lane xor butterflies: every lane ends with the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the same within each aligned group of 16 lanes
__device__ __forceinline__ float sub16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float sub16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__host__ __device__ inline int up4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int up16(int n) { return (n + 15) & ~15; }
// LDS row pitch in floats of an operand read along k: a multiple of 4 that is 4 (mod 8)
__host__ __device__ inline int pitch_kc(int n) { n = up4(n); return (n & 7) == 4 ? n : n + 4; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace gh
