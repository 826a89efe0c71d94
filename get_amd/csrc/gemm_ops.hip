// The GEMM engine's kernels: every instantiation of the grouped MFMA GEMM kernels with launch_cfg / launch_tn_pp, the fp32x3 weight
// images, the split-K workspace registry, the reduce / finish / nn kernels and their launchers.  What runs on them is decided elsewhere:
// Batch's methods are in gemm_batch.hip and its arithmetic in gemm_plan.h, which this file does not include -- they reach the kernels
// through the launchers of gemm_engine.h.  gemm_batch.h is what the engine offers the layers (cell_ops.hip, dense_ops.hip).
#include "../../include/get_hip.h"
#include "gemm_batch.h"
#include "gemm_engine.h"
#include "device_utils.h"
#include "gemm_nt.hip.h"
#include "gemm_tn.hip.h"
#include "gemm_tn_pp.hip.h"
#include <stdlib.h>

namespace gh {

static bool wants_dropout(const Launch& L) {
  for (int i = 0; i < L.nprob; ++i)
    if (L.p[i].drop_mode) return true;
  return false;
}

// launches since the last reset: {fast kernel, generic kernel, generic kernel with >= 1 GFLOP of work}.  The generic
// kernel is the correctness net for odd shapes and unaligned operands; a LARGE GEMM landing on it is a performance
// bug upstream (e.g. a misaligned parameter view), which tests assert against through gh_gemm_path_counters.
static long long g_path_counts[3] = {0, 0, 0};
static int g_gemm_mode = 0;       // 0: fp32 MFMA everywhere (default); 1: bf16 MFMA in the big-tile NT/NN GEMMs; 2: fp32x3; 3: fp32x3 with pre-split weights (gh_set_gemm_mode)
// mode 3: replaces the B operands (weights) of an NT launch by their pre-split images (registry below); false = not every
// operand could be served, the launch runs the in-register split (MODE 3) instead
static bool x3p_substitute(Launch& L, hipStream_t s);

int gemm_mode() { return g_gemm_mode; }
long long generic_launches() { return g_path_counts[1]; }

// fast, grid: gemm_plan.h fast_rule / gemm_grid, computed by the caller (gemm_batch.hip)
template <int WM, int WN, int NI, int MI = 2>
static hipError_t launch_cfg(const Launch& L, bool tn, bool fast, int grid, hipStream_t s) {
  {
    double fl = 0.0;
    for (int i = 0; i < L.nprob; ++i)
      for (int j = 0; j < L.p[i].nseg; ++j) fl += 2.0 * L.p[i].M * L.p[i].N * (double)L.p[i].seg[j].K;
    g_path_counts[fast ? 0 : 1] += 1;
    if (!fast && fl >= 1e9) g_path_counts[2] += 1;
  }
  if (grid <= 0) return hipSuccess;
  // profiler row: by the SIZE of the launch, not by the tile configuration it runs on -- the activation-sized single-problem
  // launches that the occupancy rule moves to the 32-row tile belong with the big GEMMs (booked under
  // gemm_small they made gemm_big look better than the path is)
  int max_rows = 0;
  for (int i = 0; i < L.nprob; ++i) { const int rws = tn ? L.p[i].seg[0].K : L.p[i].M; if (rws > max_rows) max_rows = rws; }
  const int tag = (max_rows >= 8192 ? PROF_GEMM_BIG : PROF_GEMM_SMALL) + (tn ? 1 : 0);
  double flops = 0.0;
  if (prof_enabled()) {
    for (int i = 0; i < L.nprob; ++i)
      for (int j = 0; j < L.p[i].nseg; ++j) {
        int rows = L.p[i].M;       // segment 0 is skipped by the row tiles at or beyond seg0_rows: do not count it
        if (j == 0 && !tn && L.p[i].nseg > 1 && L.p[i].seg0_rows > 0) {
          const int bm = 16 * MI * WM, cut = ((L.p[i].seg0_rows + bm - 1) / bm) * bm;
          if (cut < rows) rows = cut;
        }
        flops += 2.0 * rows * L.p[i].N * (double)L.p[i].seg[j].K;
      }
    prof_begin(s, tag);
  }
  if (!fast && wants_dropout(L)) return hipErrorInvalidValue;     // fused dropout exists in the fast kernels only
  if (!fast && !tn)
    for (int i = 0; i < L.nprob; ++i)
      if ((L.p[i].epi == EPI_TANH_H && L.p[i].w2) || L.p[i].epi == EPI_GATE_PRE || (L.p[i].epi == EPI_ATT && L.p[i].e_atomic == 2))
        return hipErrorInvalidValue;   // so do the fused scorer projection, the fused gate head and the head scores of column blocks
  bool launched = false;
  bool any_elt = false, all_elt = true;
  for (int i = 0; i < L.nprob; ++i) { any_elt = any_elt || L.p[i].elt; all_elt = all_elt && L.p[i].elt; }
  if (any_elt) {      // bf16 storage pipeline: only on the 64x320 fast kernels, never mixed with fp32 problems
    if (!fast || !all_elt) return hipErrorInvalidValue;
    if constexpr (WM == 2 && WN == 2 && NI == 10) {
      if (tn) hipLaunchKernelGGL((gemm_tn_bf16_kernel<2, 2, 10, 4>), dim3(grid), dim3(256), 0, s, L);      // (128 x 320 tile)
      else hipLaunchKernelGGL((gemm_nt_kernel<2, 2, 10, 2, 2>), dim3(grid), dim3(256), 0, s, L);
      launched = true;
    } else if constexpr (WM == 2 && WN == 2 && NI == 8 && MI == 4) {      // 128 x 256 tile (NT only)
      if (tn) return hipErrorInvalidValue;
      constexpr int kLds = 3 * (128 + 256) * 64;          // three K-loop stages (the epilogue staging fits inside)
      if (lds_opt_in((const void*)gemm_nt_kernel<2, 2, 8, 4, 2>, kLds, "gemm_nt 128x256")) return hipErrorInvalidValue;
      hipLaunchKernelGGL((gemm_nt_kernel<2, 2, 8, 4, 2>), dim3(grid), dim3(256), kLds, s, L);
      launched = true;
    } else if constexpr (WM == 2 && WN == 4 && NI == 4 && MI == 8) {      // 256 x 256 x 64 tile, 8 waves, ping-pong K loop (NT only; gemm_nt_pp.hip.h)
      if (tn) return hipErrorInvalidValue;
      constexpr int kLds = 131072;                        // two K tiles of 64 KB (the epilogue staging fits inside)
      if (lds_opt_in((const void*)gemm_nt_kernel<2, 4, 4, 8, 2>, kLds, "gemm_nt 256x256")) return hipErrorInvalidValue;
      hipLaunchKernelGGL((gemm_nt_kernel<2, 4, 4, 8, 2>), dim3(grid), dim3(512), kLds, s, L);
      launched = true;
    } else return hipErrorInvalidValue;
  } else if (MI >= 4) {
    return hipErrorInvalidValue;          // the 128 x 256 / 256 x 256 tiles exist for the bf16 storage pipeline only
  }
  // (the rest of this function only exists for the MI = 2 configurations: as plain run-time branches the fp32 / fp32x3 / generic
  //  launches below were instantiated for the bf16-only tile shapes as well -- nine never-launched kernels, half of this file's build time)
  if constexpr (MI == 2) {
  if (launched) {
  } else if (fast && !tn) {
    // gh_set_gemm_mode(1): bf16 operand rounding in the activation-sized (64x320 tile) launches only
    if (g_gemm_mode == 1 && WM == 2 && WN == 2 && NI == 10) {
      if constexpr (WM == 2 && WN == 2 && NI == 10)
        hipLaunchKernelGGL((gemm_nt_kernel<2, 2, 10, 2, true>), dim3(grid), dim3(256), 0, s, L);
    } else if (g_gemm_mode == 1 && WM == 1 && WN == 4 && NI == 5) {
      // ... and in the few-row launches (32 x 320 tile): at h = 768 the evidence-level products (960 rows against 22 / 41 MB
      // weights) and the claim cell are 0.5 ms of fp32 MFMA time per step
      if constexpr (WM == 1 && WN == 4 && NI == 5)
        hipLaunchKernelGGL((gemm_nt_kernel<1, 4, 5, 2, true>), dim3(grid), dim3(256), 0, s, L);
    } else if (g_gemm_mode == 2 || g_gemm_mode == 3) {      // fp32x3 (experimental): fp32 values and results, products from 3-way bf16 splits on the bf16 MFMA
      Launch L2;
      bool pre = false;
      if (g_gemm_mode == 3) { L2 = L; pre = x3p_substitute(L2, s); }
      if (pre) {
        constexpr int kLds = 2 * (16 * 2 * WM * 64 + 16 * NI * WN * 112);      // two K-loop stages, B rows at the 112-byte pitch
        if (lds_opt_in((const void*)gemm_nt_kernel<WM, WN, NI, 2, 4>, kLds, "gemm_nt fp32x3p")) return hipErrorInvalidValue;
        hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, NI, 2, 4>), dim3(grid), dim3(WM * WN * 64), kLds, s, L2);
      } else
        hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, NI, 2, 3>), dim3(grid), dim3(WM * WN * 64), 0, s, L);
    } else
      hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, NI, 2>), dim3(grid), dim3(WM * WN * 64), 0, s, L);
    launched = true;
  } else if (fast && tn) {
    if constexpr (WM == 2 && WN == 2 && NI == 10) {        // weight gradients always take the 64x320 tile (Batch: big = tn || ...)
      if (g_gemm_mode == 1) hipLaunchKernelGGL((gemm_tn_kernel<2, 2, 10, true>), dim3(grid), dim3(256), 0, s, L);
      else hipLaunchKernelGGL((gemm_tn_kernel<2, 2, 10>), dim3(grid), dim3(256), 0, s, L);
      launched = true;
    }
  }
  if (!launched) {
    if (tn) hipLaunchKernelGGL((gemm_kernel<WM, WN, NI, true>), dim3(grid), dim3(WM * WN * 64), 0, s, L);
    else hipLaunchKernelGGL((gemm_kernel<WM, WN, NI, false>), dim3(grid), dim3(WM * WN * 64), 0, s, L);
  }
  }      // MI == 2
  if (!launched && MI != 2) return hipErrorInvalidValue;
  prof_end(tag, flops, s);
  return hipGetLastError();
}

// bf16 weight gradients on the 256 x 256 x 64 ping-pong tile: one workgroup per CU, work items dealt to the XCDs in runs (L.per each)
hipError_t launch_tn_pp(const Launch& L, hipStream_t s) {
  const int grid = 8 * L.per;
  if (grid <= 0) return hipSuccess;
  g_path_counts[0] += 1;
  const int tag = PROF_GEMM_BIG + 1;
  double flops = 0.0;
  if (prof_enabled()) {
    for (int i = 0; i < L.nprob; ++i) flops += 2.0 * L.p[i].M * L.p[i].N * (double)L.p[i].seg[0].K;
    prof_begin(s, tag);
  }
  constexpr int kLds = 131072;      // two K tiles of 64 KB
  if (lds_opt_in((const void*)gemm_tn_pp_kernel, kLds, "gemm_tn_pp")) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gemm_tn_pp_kernel, dim3(grid), dim3(512), kLds, s, L);
  prof_end(tag, flops, s);
  return hipGetLastError();
}

// Split-K scratch registered by the caller (gh_set_workspace); partial tiles are written with plain
// stores and summed by reduce_partials_kernel instead of cross-XCD fp32 atomics.
// Registry: one default buffer plus any number of per-stream buffers (two streams that both split K must not share
// one scratch area); looked up by the launch's stream on every call.
}  // namespace gh
#include <mutex>
#include <unordered_map>
#include <vector>
namespace gh {
// ---- fp32x3 with pre-split weights (gh_set_gemm_mode(3)) ---------------------------------------------
// Image of a weight view B[N][ldb] (K columns used): per row ceil(K / 16) K tiles of 96 bytes, each four groups of
// {hi[4], mid[4], lo[4]} bf16 -- the three pieces of four consecutive k (zeros beyond K).  gemm_nt_kernel MODE 4 DMAs a
// K tile of a row as six 16-byte chunks.  Images are made on first use (on the launching stream), re-made in one batched
// launch by gh_fp32x3_refresh after the optimiser step, and individually when found stale (gh_weights_changed without
// a refresh: correct, slow).
struct X3Item { const float* src; unsigned char* dst; int N, ldb, K, pitch; };
constexpr int X3_BATCH = 64;
struct X3Args { int n; X3Item it[X3_BATCH]; };
__global__ void __launch_bounds__(256) split3_kernel(const X3Args a) {
  const X3Item& it = a.it[blockIdx.y];
  const int G = it.pitch / 24;
  const long long total = (long long)it.N * G;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int row = (int)(idx / G), g = (int)(idx - (long long)row * G);
    const float* src = it.src + (size_t)row * it.ldb + 4 * g;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (4 * g + e < it.K) ? src[e] : 0.f;
    unsigned hi[2], mid[2], lo[2];
    hi[0] = pack_bf2(v[0], v[1]); hi[1] = pack_bf2(v[2], v[3]);
    const float r0 = v[0] - __builtin_bit_cast(float, hi[0] << 16), r1 = v[1] - __builtin_bit_cast(float, hi[0] & 0xffff0000u);
    const float r2 = v[2] - __builtin_bit_cast(float, hi[1] << 16), r3 = v[3] - __builtin_bit_cast(float, hi[1] & 0xffff0000u);
    mid[0] = pack_bf2(r0, r1); mid[1] = pack_bf2(r2, r3);
    const float q0 = r0 - __builtin_bit_cast(float, mid[0] << 16), q1 = r1 - __builtin_bit_cast(float, mid[0] & 0xffff0000u);
    const float q2 = r2 - __builtin_bit_cast(float, mid[1] << 16), q3 = r3 - __builtin_bit_cast(float, mid[1] & 0xffff0000u);
    lo[0] = pack_bf2(q0, q1); lo[1] = pack_bf2(q2, q3);
    uint2* dst = reinterpret_cast<uint2*>(it.dst + (size_t)row * it.pitch + (size_t)g * 24);
    dst[0] = make_uint2(hi[0], hi[1]); dst[1] = make_uint2(mid[0], mid[1]); dst[2] = make_uint2(lo[0], lo[1]);
  }
}
struct X3Key {
  const void* b; int ldb, K, N;
  bool operator==(const X3Key& o) const { return b == o.b && ldb == o.ldb && K == o.K && N == o.N; }
};
struct X3Hash {
  size_t operator()(const X3Key& k) const {
    size_t h = std::hash<const void*>()(k.b);
    h ^= std::hash<long long>()(((long long)k.ldb << 40) ^ ((long long)k.K << 20) ^ (long long)k.N) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
    return h;
  }
};
struct X3Ent { unsigned char* img; int pitch; long long epoch; };
static std::mutex g_x3_mu;
static std::unordered_map<X3Key, X3Ent, X3Hash> g_x3;
static std::unordered_multimap<size_t, unsigned char*> g_x3_pool;      // buffers of cleared images, by size (hipMalloc / hipFree are slow)
static long long g_x3_epoch = 0;

static void x3p_split(const X3Item* items, int n, hipStream_t s) {
  for (int i0 = 0; i0 < n; i0 += X3_BATCH) {
    X3Args a;
    a.n = n - i0 < X3_BATCH ? n - i0 : X3_BATCH;
    long long mx = 0;
    for (int i = 0; i < a.n; ++i) {
      a.it[i] = items[i0 + i];
      const long long t = (long long)a.it[i].N * (a.it[i].pitch / 24);
      if (t > mx) mx = t;
    }
    int gx = (int)((mx + 255) / 256);
    if (gx > 256) gx = 256;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(split3_kernel, dim3(gx, a.n), dim3(256), 0, s, a);
  }
}

static bool x3p_substitute(Launch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_x3_mu);
  X3Item todo[2 * GH_MAX_PROBLEMS];
  int nt = 0;
  for (int i = 0; i < L.nprob; ++i) {
    Problem& q = L.p[i];
    if (q.elt) return false;
    for (int j = 0; j < q.nseg; ++j) {
      Seg& g = q.seg[j];
      if (g.K <= 0 || g.gatherB) return false;
      const X3Key key{g.B, g.ldb, g.K, q.N};
      auto f = g_x3.find(key);
      if (f == g_x3.end()) {
        if (g_x3.size() >= 512) return false;      // views keep changing address (caller never clears): stop growing, in-register split instead
        X3Ent e;
        e.pitch = ((g.K + 15) / 16) * 96;
        e.epoch = -1;
        const size_t bytes = (size_t)q.N * e.pitch + 256;
        auto pf = g_x3_pool.find(bytes);
        if (pf != g_x3_pool.end()) { e.img = pf->second; g_x3_pool.erase(pf); }
        else if (hipMalloc((void**)&e.img, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        f = g_x3.emplace(key, e).first;
      }
      if (f->second.epoch != g_x3_epoch) {
        todo[nt++] = X3Item{g.B, f->second.img, q.N, g.ldb, g.K, f->second.pitch};
        f->second.epoch = g_x3_epoch;
      }
      g.B = reinterpret_cast<const float*>(f->second.img);
      g.ldb = f->second.pitch / 4;
    }
  }
  if (nt > 0) x3p_split(todo, nt, s);
  return true;
}
static std::mutex g_ws_mu;
static Workspace g_ws_default = {nullptr, 0, nullptr, 0};
// keyed by (device, stream): the default stream has handle 0 on EVERY device, so the stream alone does not identify a
// scratch area in a process that drives several devices
struct WsKey { int dev; hipStream_t s; bool operator==(const WsKey& o) const { return dev == o.dev && s == o.s; } };
struct WsKeyHash { size_t operator()(const WsKey& k) const { return std::hash<const void*>()((const void*)k.s) * 31u + (size_t)(k.dev + 1); } };
static std::unordered_map<WsKey, Workspace, WsKeyHash> g_ws_stream;
static int current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) d = 0; return d; }
static Workspace make_workspace(void* ptr, int64_t bytes) {
  // the last 1/16 of the buffer (16-byte aligned) serves the column-sum partials, the rest split-K tiles
  Workspace w = {nullptr, 0, nullptr, 0};
  if (!ptr || bytes < (1 << 20)) return w;
  const size_t tail = ((size_t)bytes / 16) & ~(size_t)15;
  w.p = (float*)ptr;
  w.bytes = ((size_t)bytes - tail) & ~(size_t)15;
  w.cs = (float*)((char*)ptr + w.bytes);
  w.cs_bytes = tail;
  return w;
}
Workspace workspace_for(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  auto it = g_ws_stream.find(WsKey{current_device(), s});
  return it != g_ws_stream.end() ? it->second : g_ws_default;
}


__global__ void __launch_bounds__(256)
reduce_partials_kernel(const ReduceArgs R) {
  const ReduceItem& it = R.it[blockIdx.y];
  const int J4 = it.J / 4;
  const size_t total = (size_t)it.I * J4;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / J4), j = 4 * (int)(e % J4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* p = it.ws + (size_t)i * it.J + j;
    int k = 0;
    for (; k + 8 <= it.ks; k += 8) {           // 8 independent 16-byte loads in flight, fixed summation order
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(k + u) * it.stride);
#pragma unroll
      for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
    for (; k < it.ks; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(p + (size_t)k * it.stride);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float* o = it.out + (size_t)i * it.ldc + j;     // += : gradients accumulate into the caller's buffer
    o[0] += acc.x; o[1] += acc.y; o[2] += acc.z; o[3] += acc.w;
  }
}

// Same reduction for FEW output elements and MANY partials (dW2 of the attention: 5 x 300 values, one partial per
// pair): one wave per float4 element, lanes stride over the partials, fixed-order shuffle tree.
__global__ void __launch_bounds__(256)
reduce_partials_wave_kernel(const ReduceArgs R) {
  const ReduceItem& it = R.it[blockIdx.y];
  const int J4 = it.J / 4;
  const int total = it.I * J4;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= total) return;
  const int i = e / J4, j = 4 * (e % J4);
  const float* p = it.ws + (size_t)i * it.J + j;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = lane; k < it.ks; k += 64) {
    const float4 v = *reinterpret_cast<const float4*>(p + (size_t)k * it.stride);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  for (int o = 32; o > 0; o >>= 1) {
    acc.x += __shfl_xor(acc.x, o); acc.y += __shfl_xor(acc.y, o); acc.z += __shfl_xor(acc.z, o); acc.w += __shfl_xor(acc.w, o);
  }
  if (lane == 0) {
    float* o = it.out + (size_t)i * it.ldc + j;
    o[0] += acc.x; o[1] += acc.y; o[2] += acc.z; o[3] += acc.w;
  }
}

// C [I][J] += sum_t A_t [I][K_t] . B_t [K_t][J] on weight-sized operands (gemm_batch.h NnArgs).  One workgroup of eight waves
// per 32 x 32 output tile; the 16-deep K chunks of the item's concatenated terms are dealt round-robin to the waves.  No LDS
// stage: with lane group q = lane / 16 taking k = k0 + 4 q + s in MFMA step s (any assignment of k to steps and groups is a valid
// contraction as long as A and B agree on it), a lane's four A values are ONE 16-byte load of its row and its B values four
// loads that 16 lanes coalesce, so a chunk is ten independent loads and sixteen v_mfma_f32_16x16x4_f32 per wave.  The eight
// partial tiles are added in wave order: fixed summation order, every output element has one writer.  (First version, FMAs on
// 4 x 4 register blocks over an LDS stage with two barriers per chunk: 184 us for the ten 300^3 products of a cell backward --
// launch-sized work is latency-bound, not FLOP-bound.)
constexpr int NN_T = 32, NN_K = 16, NN_WAVES = 8;
__global__ void __launch_bounds__(64 * NN_WAVES)
nn_accumulate_kernel(const NnArgs R_byval) {
  // (the item and term tables are indexed at run time: read them from the kernarg segment, as gemm_kernel does)
  (void)R_byval;
  const GH_KARG NnArgs& R = *(const GH_KARG NnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ float red[NN_WAVES][NN_T][NN_T];
  int item = 0;
  while (item + 1 < R.n && (int)blockIdx.x >= R.it[item + 1].tile0) ++item;
  const GH_KARG NnItem& it = R.it[item];
  const int I = it.I, J = it.J;
  const int tiles_j = (J + NN_T - 1) / NN_T;
  const int tile = (int)blockIdx.x - it.tile0;
  const int i0 = (tile / tiles_j) * NN_T, j0 = (tile % tiles_j) * NN_T;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l15 = lane & 15, q = lane >> 4;
  int total = 0;
  for (int t = 0; t < it.nterm; ++t) total += (it.t[t].K + NN_K - 1) / NN_K;
  // rows / columns beyond the matrix are clamped to its last one: their products land in accumulators that are never stored
  int row[2], col[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    row[m] = i0 + m * 16 + l15; if (row[m] > I - 1) row[m] = I - 1;
    col[m] = j0 + m * 16 + l15; if (col[m] > J - 1) col[m] = J - 1;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  int t = 0, base = 0;
  for (int c = w; c < total; c += NN_WAVES) {
    for (;;) {      // (c < total: the term is found before t runs off the table)
      const int nc = (it.t[t].K + NN_K - 1) / NN_K;
      if (c < base + nc) break;
      base += nc; ++t;
    }
    const GH_KARG NnTerm& tm = it.t[t];
    const float* A = tm.A;
    const float* B = tm.B;
    const int K = tm.K, lda = tm.lda, ldb = tm.ldb;
    const int kk = (c - base) * NN_K + 4 * q;
    float av[2][4], bv[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const float* ap = A + (size_t)row[mi] * lda + kk;
      if (tm.vec) {      // K % 4 == 0: the four values are inside the row together or not at all
        const float4 v = kk < K ? *reinterpret_cast<const float4*>(ap) : make_float4(0.f, 0.f, 0.f, 0.f);
        av[mi][0] = v.x; av[mi][1] = v.y; av[mi][2] = v.z; av[mi][3] = v.w;
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) av[mi][s] = kk + s < K ? ap[s] : 0.f;
      }
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int s = 0; s < 4; ++s) bv[ni][s] = kk + s < K ? B[(size_t)(kk + s) * ldb + col[ni]] : 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi][s], bv[ni][s], acc[mi][ni], 0, 0, 0);
  }
  // accumulator register `reg` of lane (q, l15) is element (4 q + reg, l15) of its 16 x 16 block
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) red[w][mi * 16 + 4 * q + reg][ni * 16 + l15] = acc[mi][ni][reg];
  __syncthreads();
  if (threadIdx.x >= NN_T * NN_T / 4) return;
  const int ri = threadIdx.x >> 3, rj = 4 * (threadIdx.x & 7);
  float4 sum = *reinterpret_cast<const float4*>(&red[0][ri][rj]);
#pragma unroll
  for (int v = 1; v < NN_WAVES; ++v) {
    const float4 p = *reinterpret_cast<const float4*>(&red[v][ri][rj]);
    sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
  }
  const int gi = i0 + ri, gj = j0 + rj;
  if (gi < I) {
    float* o = it.C + (size_t)gi * it.ldc + gj;
    const float sv[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (gj + e < J) o[e] += sv[e];      // += : gradients accumulate into the caller's buffer
  }
}

__global__ void __launch_bounds__(256)
nt_finish_kernel(const FinishArgs F) {
  const FinishItem& it = F.it[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool split = F.split != 0;
  const int row = split ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave;
  if (row >= it.M) return;           // (workgroup-uniform when split)
  const int N4 = it.N / 4;
  __shared__ float4 part[3][64];
  int kb = 0, ke = it.ks;
  if (split) { const int kq = (it.ks + 3) / 4; kb = wave * kq; ke = min(it.ks, kb + kq); }
  float pe[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) pe[c] = 0.f;
  for (int c0 = 0; c0 < N4; c0 += 64) {
    const int c4 = c0 + lane;
    const int col = 4 * c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < N4 && kb < ke) {
      const float* p = it.ws + (size_t)row * it.N + col;
      for (int k0 = kb; k0 < ke; k0 += 8) {            // eight partial tiles in flight, added in split order
        float4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const float4*>(p + (size_t)min(k0 + u, ke - 1) * it.stride);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + u < ke) { v.x += x[u].x; v.y += x[u].y; v.z += x[u].z; v.w += x[u].w; }
      }
    }
    if (split) {
      if (c0 > 0) __syncthreads();                     // wave 0 is done with the previous chunk's quarter sums
      if (wave > 0) part[wave - 1][lane] = v;
      __syncthreads();
      if (wave > 0) continue;
#pragma unroll
      for (int w = 0; w < 3; ++w) { const float4 q = part[w][lane]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    }
    if (c4 >= N4) continue;
    const size_t oo = (size_t)row * it.ldc + col;
    float* o = it.C + oo;
    if (it.bias) { const float4 b4 = *reinterpret_cast<const float4*>(it.bias + col); v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w; }
    if (it.bias2) { const float4 b4 = *reinterpret_cast<const float4*>(it.bias2 + col); v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w; }
    if (it.epi == EPI_ATT) {
      const float4 u4 = *reinterpret_cast<const float4*>(it.u + (size_t)(it.rowg ? it.rowg[row] : row / it.R) * it.ldu + col);
      const float4 t = make_float4(tanhf_(v.x + u4.x), tanhf_(v.y + u4.y), tanhf_(v.z + u4.z), tanhf_(v.w + u4.w));
      *reinterpret_cast<float4*>(o) = t;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < it.heads) {
          const float4 w = *reinterpret_cast<const float4*>(it.w2 + (size_t)c * it.N + col);
          pe[c] += t.x * w.x + t.y * w.y + t.z * w.z + t.w * w.w;
        }
    } else if (it.epi == EPI_SIGMOID_Z) {
      *reinterpret_cast<float4*>(o) = make_float4(sigmoidf_(v.x), sigmoidf_(v.y), sigmoidf_(v.z), sigmoidf_(v.w));
    } else if (it.epi == EPI_SIGMOID_R) {
      const float4 x = *reinterpret_cast<const float4*>(it.in0 + oo);
      const float4 r4 = make_float4(sigmoidf_(v.x), sigmoidf_(v.y), sigmoidf_(v.z), sigmoidf_(v.w));
      *reinterpret_cast<float4*>(o) = r4;
      *reinterpret_cast<float4*>(it.out1 + oo) = make_float4(r4.x * x.x, r4.y * x.y, r4.z * x.z, r4.w * x.w);
    } else if (it.epi == EPI_TANH_H) {
      const float4 z = *reinterpret_cast<const float4*>(it.in0 + oo);
      const float4 x = *reinterpret_cast<const float4*>(it.in1 + oo);
      const float4 h = make_float4(tanhf_(v.x), tanhf_(v.y), tanhf_(v.z), tanhf_(v.w));
      *reinterpret_cast<float4*>(o) = h;
      *reinterpret_cast<float4*>(it.out1 + oo) = make_float4(h.x * z.x + x.x * (1.f - z.x), h.y * z.y + x.y * (1.f - z.y),
                                                             h.z * z.z + x.z * (1.f - z.z), h.w * z.w + x.w * (1.f - z.w));
    } else if (it.epi == EPI_BWD_DRX) {
      const float4 x = *reinterpret_cast<const float4*>(it.in0 + oo);
      const float4 r4 = *reinterpret_cast<const float4*>(it.in1 + oo);
      float4 d = *reinterpret_cast<const float4*>(it.out1 + oo);
      *reinterpret_cast<float4*>(o) = make_float4(v.x * x.x * r4.x * (1.f - r4.x), v.y * x.y * r4.y * (1.f - r4.y),
                                                  v.z * x.z * r4.z * (1.f - r4.z), v.w * x.w * r4.w * (1.f - r4.w));
      d.x += v.x * r4.x; d.y += v.y * r4.y; d.z += v.z * r4.z; d.w += v.w * r4.w;
      *reinterpret_cast<float4*>(it.out1 + oo) = d;
    } else {
      if (it.accumulate) {
        const float4 c4v = *reinterpret_cast<const float4*>(o);
        v.x += c4v.x; v.y += c4v.y; v.z += c4v.z; v.w += c4v.w;
      }
      *reinterpret_cast<float4*>(o) = v;
      if (it.w2) {      // a second, few-column linear layer on the finished row (the head's out[1]): e = v . w2^T (+ in0 as its bias)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < it.heads) {
            const float4 w = *reinterpret_cast<const float4*>(it.w2 + (size_t)c * it.N + col);
            pe[c] += v.x * w.x + v.y * w.y + v.z * w.z + v.w * w.w;
          }
      }
    }
  }
  const bool proj = it.epi == EPI_STORE && it.w2 != nullptr;
  if ((it.epi == EPI_ATT || proj) && (!split || wave == 0)) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = pe[c];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && c < it.heads) it.e[(size_t)row * it.heads + c] = v + ((proj && it.in0) ? it.in0[c] : 0.f);
    }
  }
}


// ---- the launchers of gemm_engine.h ----------------------------------------------------------------------------------------
hipError_t launch_gemm(GemmConfig cfg, const Launch& L, bool tn, bool fast, int grid, hipStream_t s) {
  switch (cfg) {
    case CFG_32x320: return launch_cfg<1, 4, 5>(L, tn, fast, grid, s);
    case CFG_64x320: return launch_cfg<2, 2, 10>(L, tn, fast, grid, s);
    case CFG_64x160: return launch_cfg<2, 2, 5>(L, tn, fast, grid, s);
    case CFG_128x256: return launch_cfg<2, 2, 8, 4>(L, tn, fast, grid, s);
    case CFG_256x256: return launch_cfg<2, 4, 4, 8>(L, tn, fast, grid, s);
    default: return hipErrorInvalidValue;      // (CFG_TN_PP: launch_tn_pp)
  }
}
hipError_t launch_reduce_partials(const ReduceArgs& R, int max_elems, hipStream_t s) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((max_elems + 255) / 256, R.n), dim3(256), 0, s, R);
  return hipGetLastError();
}
hipError_t launch_nt_finish(const FinishArgs& F, int grid_x, hipStream_t s) {
  hipLaunchKernelGGL(nt_finish_kernel, dim3(grid_x, F.n), dim3(256), 0, s, F);
  return hipGetLastError();
}

// the layers' two direct uses of this file's kernels (gemm_batch.h)
int launch_att_finish(float* t, const float* u, const float* w2, float* e, const int32_t* urow, int M, int ha, int l, int heads, hipStream_t s) {
  FinishArgs F;
  F.n = 1; F.split = 0;
  F.it[0] = FinishItem{t, 0, 1, M, ha, EPI_ATT, 0, ha, t, nullptr, nullptr, nullptr, nullptr, nullptr, u, w2, e, ha, l, heads, urow};
  hipLaunchKernelGGL(nt_finish_kernel, dim3((M + 3) / 4, 1), dim3(256), 0, s, F);
  GH_LAUNCH_CHECK();
  return 0;
}
int launch_reduce_wave(const float* parts, int n_parts, float* out, int I, int J, hipStream_t s) {
  ReduceArgs R;
  R.n = 1;
  R.it[0] = ReduceItem{parts, out, I, J, J, n_parts, (long long)I * J};
  hipLaunchKernelGGL(reduce_partials_wave_kernel, dim3((I * (J / 4) + 3) / 4, 1), dim3(256), 0, s, R);
  GH_LAUNCH_CHECK();
  return 0;
}
int launch_nn_accumulate(NnArgs& R, hipStream_t s) {
  GH_REQUIRE(R.n > 0 && R.n <= NN_MAX_ITEMS, "nn_accumulate: %d items", R.n);
  int tiles = 0;
  for (int i = 0; i < R.n; ++i) {
    NnItem& it = R.it[i];
    GH_REQUIRE(it.C && it.I > 0 && it.J > 0 && it.ldc >= it.J && it.nterm > 0 && it.nterm <= NN_MAX_TERMS, "nn_accumulate: bad item %d", i);
    for (int t = 0; t < it.nterm; ++t)
      GH_REQUIRE(it.t[t].A && it.t[t].B && it.t[t].K > 0 && it.t[t].lda >= it.t[t].K && it.t[t].ldb >= it.J, "nn_accumulate: bad term %d of item %d", t, i);
    for (int t = 0; t < it.nterm; ++t)
      it.t[t].vec = (reinterpret_cast<uintptr_t>(it.t[t].A) & 15) == 0 && it.t[t].lda % 4 == 0 && it.t[t].K % 4 == 0;
    it.tile0 = tiles;
    tiles += ((it.I + NN_T - 1) / NN_T) * ((it.J + NN_T - 1) / NN_T);
  }
  hipLaunchKernelGGL(nn_accumulate_kernel, dim3(tiles), dim3(64 * NN_WAVES), 0, s, R);
  GH_LAUNCH_CHECK();
  return 0;
}

}  // namespace gh

using namespace gh;

extern "C" int gh_set_gemm_mode(int mode) {
  GH_REQUIRE(mode >= 0 && mode <= 3, "set_gemm_mode: %d is not 0 (fp32), 1 (bf16 operands in the big NT/NN GEMMs), 2 (fp32x3) or 3 (fp32x3, pre-split weights)", mode);
  g_gemm_mode = mode;
  return 0;
}

extern "C" int gh_weights_changed(void) {
  std::lock_guard<std::mutex> lk(g_x3_mu);
  ++g_x3_epoch;
  return 0;
}

extern "C" int gh_fp32x3_refresh(gh_stream_t stream) {
  std::lock_guard<std::mutex> lk(g_x3_mu);
  if (g_x3.empty()) return 0;
  std::vector<X3Item> items;
  items.reserve(g_x3.size());
  for (auto& kv : g_x3) {
    items.push_back(X3Item{(const float*)kv.first.b, kv.second.img, kv.first.N, kv.first.ldb, kv.first.K, kv.second.pitch});
    kv.second.epoch = g_x3_epoch;
  }
  x3p_split(items.data(), (int)items.size(), (hipStream_t)stream);
  GH_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gh_fp32x3_clear(void) {
  std::lock_guard<std::mutex> lk(g_x3_mu);
  if (g_x3.empty()) return 0;
  GH_CHECK_HIP(hipDeviceSynchronize());      // a launch on any stream may still read an image; the buffers go back to the pool
  for (auto& kv : g_x3) g_x3_pool.emplace((size_t)kv.first.N * kv.second.pitch + 256, kv.second.img);
  g_x3.clear();
  if (g_x3_pool.size() > 2048) {
    for (auto& kv : g_x3_pool) (void)hipFree(kv.second);
    g_x3_pool.clear();
  }
  return 0;
}

extern "C" int gh_gemm_path_counters(int64_t* out_host, int reset) {
  if (out_host)
    for (int i = 0; i < 3; ++i) out_host[i] = g_path_counts[i];
  if (reset) g_path_counts[0] = g_path_counts[1] = g_path_counts[2] = 0;
  return 0;
}

extern "C" int gh_set_workspace(void* ptr, int64_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  g_ws_default = make_workspace(ptr, bytes);
  return 0;
}

extern "C" int gh_set_stream_workspace(gh_stream_t stream, void* ptr, int64_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const WsKey key{current_device(), (hipStream_t)stream};      // the CURRENT device's `stream`
  if (!ptr) g_ws_stream.erase(key);
  else g_ws_stream[key] = make_workspace(ptr, bytes);
  return 0;
}

#ifdef GH_MEASURE
extern "C" int gh_debug_nt_phases(unsigned long long* out, int reset) {     // out: [16][4]
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nt_phase), 64 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_nt_phase)) != hipSuccess || hipMemset(p, 0, 64 * sizeof(unsigned long long)) != hipSuccess) return 1; }
  return 0;
}
#endif
