// Helpers shared by the drop-in kernel files (attention_ops.hip, encoder_ops.hip, mha_ops.hip, rnn_ops.hip, bidaf_ops.hip,
// match_ops.hip): wave and 16-lane reductions, round-up and LDS-pitch arithmetic, the alignment test of the float4 paths and
// the opt-in to more than 64 KB of LDS.  score_tile.hip.h builds on it: the LDS staging and MFMA helpers of the three files that
// keep a 16-row score tile in LDS (mha_ops.hip, bidaf_ops.hip, match_ops.hip).
#pragma once
#include "common.h"

namespace gh {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// Before a launch with `lds` bytes of dynamic shared memory: refuses more than the 160 KB of a CU and lifts the kernel's
// 64 KB default where it has to.  Returns 0, or the error code with the message set.
template <typename K> int lds_opt_in(K kernel, size_t lds, const char* who) {
  GH_REQUIRE(lds <= 160 * 1024, "%s: needs %zu bytes of LDS", who, lds);
  if (lds > 64 * 1024) GH_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return 0;
}

}  // namespace gh
