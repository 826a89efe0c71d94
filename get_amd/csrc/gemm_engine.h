// Between the two halves of the GEMM engine, and private to them: gemm_ops.hip (the kernels and their launchers) defines what is
// declared here, gemm_batch.hip (Batch's methods: the plans of gemm_plan.h turned into launches) calls it.  Nobody else includes it.
#pragma once
#include "common.h"
#include "gemm_types.h"

namespace gh {

// One launch on configuration `cfg` (any but CFG_TN_PP) with `grid` workgroups; fast: the launch meets the fast kernels'
// preconditions (gemm_plan.h fast_rule / gemm_grid -- the engine takes both as given and does not restate them).
hipError_t launch_gemm(GemmConfig cfg, const Launch& L, bool tn, bool fast, int grid, hipStream_t s);
// bf16 weight gradients on the 256 x 256 x 64 ping-pong tile: one workgroup per CU, work items dealt to the XCDs in runs (L.per each)
hipError_t launch_tn_pp(const Launch& L, hipStream_t s);

// out [I][J] (+=) the sum of ks partials [I][J] that lie `stride` floats apart
struct ReduceItem { const float* ws; float* out; int I, J, ldc, ks; long long stride; };
struct ReduceArgs { ReduceItem it[3 * GH_MAX_PROBLEMS]; int n; };     // the tiles of a launch's <= GH_MAX_PROBLEMS problems + up to two bias-gradient outputs each
// reduce_partials_kernel over R's items; max_elems: float4 elements of the largest one
hipError_t launch_reduce_partials(const ReduceArgs& R, int max_elems, hipStream_t s);

// Second half of an NT GEMM that was split over K: sum the partial tiles, then apply the problem's real epilogue
// (any of gemm.hip.h's row epilogues).  One wave per output row.
struct FinishItem {
  const float* ws; long long stride; int ks; int M, N, epi, accumulate, ldc;
  float* C; const float* bias; const float* bias2; float* out1; const float* in0; const float* in1;
  const float* u; const float* w2; float* e; int ldu, R, heads;
  const int32_t* rowg;
};
// Two shapes.  split = 1 (few-row products with many partials: the head's K = 3556 product has 45, and had 55 when this was measured): one WORKGROUP per output
// row, the four waves each sum a quarter of the partial tiles (eight 16-byte loads in flight per lane), the quarter sums meet
// in LDS in wave order (fixed summation order: deterministic) and wave 0 applies the epilogue -- one wave per row walked all
// `ks` partials alone, 14 dependent memory round trips = 18 us for the head; four waves need 4.  split = 0: one wave per
// row, four rows per workgroup (few partials, many rows).
struct FinishArgs { FinishItem it[GH_MAX_PROBLEMS]; int n; int split; };
// nt_finish_kernel on a grid of grid_x x F.n workgroups
hipError_t launch_nt_finish(const FinishArgs& F, int grid_x, hipStream_t s);

}  // namespace gh
