// The GEMM engine: every instantiation of the grouped MFMA GEMM kernels, the fp32x3 weight images, the split-K workspace with its
// reduce / finish kernels, and Batch's tile and split-K planning.  gemm_batch.h is what it offers the layers built on it
// (cell_ops.hip: GGNN cell; dense_ops.hip: concat attention, linear layers), which hold no kernel and compile in seconds.
#include "../../include/get_hip.h"
#include "gemm_batch.h"
#include "device_utils.h"
#include "gemm_nt.hip.h"
#include "gemm_tn.hip.h"
#include "gemm_tn_pp.hip.h"
#include <stdlib.h>

namespace gh {

static bool s_lds_bad(const Problem& p) { return p.seg[0].lda % 8 || p.seg[0].ldb % 8; }
// fast-path preconditions of gemm_nt.hip.h (NT: both operands contraction-contiguous) and gemm_tn.hip.h (TN); both LDS-DMA
// tool build: GH_FASTOK_DEBUG=1 names the rule that sent a launch to the generic kernel (seg >= 0: and that segment's sizes)
static void fast_why(int rule, int prob, const Problem* p = nullptr, int seg = -1) {
  static const bool dbg = measure_env("GH_FASTOK_DEBUG", 0) != 0;
  if (!dbg) return;
  fprintf(stderr, "gemm: generic kernel (fast_ok rule %d, problem %d)\n", rule, prob);
  if (p && seg >= 0) fprintf(stderr, "   seg %d lda %d M %d N %d K %d\n", seg, p->seg[seg].lda, p->M, p->N, p->seg[seg].K);
}
static bool fast_ok(const Launch& L, bool tn) {
  for (int i = 0; i < L.nprob; ++i) {
    const Problem& p = L.p[i];
    const int ns = tn ? 1 : p.nseg;
    for (int j = 0; j < ns; ++j) {
      const Seg& s = p.seg[j];
      if (!s.vecA || !s.vecB || s.gatherB || s.K < 4) { fast_why(1, i); return false; }
      if (tn && s.gatherA) { fast_why(2, i); return false; }
    }
    if (p.elt && tn && (p.M % 8 || p.N % 8 || s_lds_bad(p))) { fast_why(3, i); return false; }
    if (!tn) {  // operands are addressed through buffer descriptors: 31-bit byte offsets
      for (int j = 0; j < p.nseg; ++j) {
        if (4.0 * (double)p.seg[j].ldb * (double)p.N >= 2147483648.0) { fast_why(4, i); return false; }
        if (!p.seg[j].gatherA && 4.0 * (double)p.seg[j].lda * (double)p.M >= 2147483648.0) { fast_why(5, i, &p, j); return false; }   // (gathered tables: < 2 GB by contract)
      }
    }
    if (tn) {
      const Seg& s = p.seg[0];
      if (4.0 * (double)s.lda * (double)s.K >= 2147483648.0 || 4.0 * (double)s.ldb * (double)s.K >= 2147483648.0) { fast_why(6, i); return false; }
    }
    if (p.N % 4 || p.N < 4 || p.ldc % 4 || !aligned16(p.C)) { fast_why(7, i); return false; }
    if (tn && (p.M % 4 || p.M < 4)) { fast_why(8, i); return false; }
    if ((p.bias && !aligned16(p.bias)) || (p.bias2 && !aligned16(p.bias2)) || (p.out1 && !aligned16(p.out1)) || (p.in0 && !aligned16(p.in0)) || (p.in1 && !aligned16(p.in1)))
      { fast_why(9, i); return false; }
    if (p.epi == EPI_ATT && (!aligned16(p.u) || p.ldu % 4 || !aligned16(p.w2))) { fast_why(10, i); return false; }
    if (p.epi == EPI_TANH_H && p.w2 && !aligned16(p.w2)) { fast_why(11, i); return false; }
    if (p.epi == EPI_GATE_PRE && (tn || !p.in0 || !p.in1 || !p.in2 || !p.out1 || !p.out2 || !aligned16(p.in2) || !aligned16(p.out2) ||
                                  (p.gin && !aligned16(p.gin)))) { fast_why(12, i); return false; }
  }
  return true;
}
// bf16 weight-gradient GEMM on the 256 x 256 x 64 ping-pong tile (gemm_tn_pp.hip.h): K-chunk rows from which a batch of whole-output
// problems takes it (below: the 128 x 320 tile, gemm_tn_bf16_kernel<2, 2, 10, 4>)
constexpr int TN_PP_ROWS = 16384;
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

template <int WM, int WN, int NI, int MI = 2>
static hipError_t launch_cfg(const Launch& L, bool tn, hipStream_t s) {
  const bool fast = fast_ok(L, tn);
  {
    double fl = 0.0;
    for (int i = 0; i < L.nprob; ++i)
      for (int j = 0; j < L.p[i].nseg; ++j) fl += 2.0 * L.p[i].M * L.p[i].N * (double)L.p[i].seg[j].K;
    g_path_counts[fast ? 0 : 1] += 1;
    if (!fast && fl >= 1e9) g_path_counts[2] += 1;
  }
  const int n_outer = tn ? L.ksplit : L.m_tiles;
  const int n_inner = tn ? L.m_tiles * L.nprob : L.nprob * L.ksplit;
  const bool nt_few = !tn && L.m_tiles < 8 && fast;      // gemm_nt.hip.h: linear work decode for launches of fewer than 8 row tiles
  const int grid = nt_few ? n_outer * n_inner : 8 * ((n_outer + 7) / 8) * n_inner;
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
static hipError_t launch_tn_pp(const Launch& L, hipStream_t s) {
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

struct ReduceItem { const float* ws; float* out; int I, J, ldc, ks; long long stride; };
struct ReduceArgs { ReduceItem it[3 * GH_MAX_PROBLEMS]; int n; };     // tiles of <= 8 problems + up to two bias-gradient outputs each

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

// Second half of an NT GEMM that was split over K: sum the partial tiles, then apply the problem's real epilogue
// (any of gemm.hip.h's row epilogues).  One wave per output row.
struct FinishItem {
  const float* ws; long long stride; int ks; int M, N, epi, accumulate, ldc;
  float* C; const float* bias; const float* bias2; float* out1; const float* in0; const float* in1;
  const float* u; const float* w2; float* e; int ldu, R, heads;
  const int32_t* rowg;
};

// Two shapes.  split = 1 (few-row products with many partials: the head's K = 3556 product has 55): one WORKGROUP per output
// row, the four waves each sum a quarter of the partial tiles (eight 16-byte loads in flight per lane), the quarter sums meet
// in LDS in wave order (fixed summation order: deterministic) and wave 0 applies the epilogue -- one wave per row walked all
// `ks` partials alone, 14 dependent memory round trips = 18 us for the head; four waves need 4.  split = 0: one wave per
// row, four rows per workgroup (few partials, many rows).
struct FinishArgs { FinishItem it[GH_MAX_PROBLEMS]; int n; int split; };

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

// ---- Batch (declared in gemm_batch.h, with the comments on its knobs): tile choice, column blocks, split-K plans -------------
bool Batch::tn_pp_ok(const Problem& p) const {
  if (!tn || !p.elt || p.nseg != 1 || g_ws == nullptr || p.epi != EPI_ATOMIC) return false;
  const Seg& sg = p.seg[0];
  if (sg.gatherA || sg.gatherB || !sg.vecA || !sg.vecB || sg.K < TN_PP_ROWS) return false;
  if (p.M % 256 || p.N % 256 || p.ldc % 4 || (reinterpret_cast<uintptr_t>(p.C) & 15)) return false;
  return (size_t)sg.K * (size_t)sg.lda * 2 < ((size_t)1 << 31) && (size_t)sg.K * (size_t)sg.ldb * 2 < ((size_t)1 << 31);
}
Batch::Batch(bool tn_, int rows_hint, hipStream_t s_, bool wide_bf16, int site, int n_hint) : tn(tn_), s(s_) {
  const Workspace w = workspace_for(s_);
  g_ws = w.p; g_ws_bytes = w.bytes;
  big = tn_ || rows_hint >= 8192;      // 64x320 tile (2x2 waves) for the activation-sized GEMMs, 32x320 (1x4) for few-row ones
  bm = big ? 64 : 32;
  bn = 320;
  if (wide_bf16 && big && !tn_) { wide = true; bm = 128; bn = 256; }
  // 256 x 256 x 64 / 8 waves, one workgroup per CU, ping-pong K loop + software-pipelined epilogue (gemm_nt_pp.hip.h, round 6):
  // the default for activation-sized launches of the bf16 storage pipeline -- configs[4], B = 32: gemm_big 4.25 -> 3.09 ms per
  // step, 128.1 -> 148.6 K pairs/s.  (Round 3's 256 x 256 tile -- the 128 x 256 tile's K loop on 8 waves, 32-deep stages --
  // measured 0.200 against 0.207: not the tile size but the loop structure is the lever.)  Launches below 32 768 rows (fewer
  // than 1.5 workgroups per CU) keep the 128 x 256 tile.
  constexpr int tile256_rows = 32768;
  if (wide && rows_hint >= tile256_rows) { wide256 = true; bm = 256; }
  const bool less_pad = n_hint > 0 && (n_hint + 159) / 160 * 160 < (n_hint + 319) / 320 * 320;
  // launches whose 64 x 320 grid would not fill one round of 768 workgroup slots (realistic evidence counts: 14 208 rows = 222
  // row tiles) get twice the workgroups on 1024 slots: 99.0 -> 102.0 K pairs/s on the Snopes-histogram step at B = 32
  const bool thin = rows_hint <= 24576;
  if (site > 0 && big && !tn_ && !wide && g_gemm_mode == 0 && (((NARROW_DEFAULT >> (site - 1)) & 1) || less_pad || thin)) { narrow = true; bn = 160; }
  // (launches without a call-site id, e.g. the attention's t product with its head scores, keep the 64 x 320 tile)
  reset();
}
void Batch::reset() {
  L.nprob = 0; L.m_tiles = 0; L.ksplit = 1; L.kchunk = 0; k_total = 0; L.n_tiles = 0; L.per = 0;
  static const int dbg = measure_env("GH_DBG", 0);      // (tool build: DBG_* bits, gemm.hip.h)
  L.dbg = dbg;
  for (int i = 0; i < GH_MAX_PROBLEMS; ++i) cs_out[i] = cs_out2[i] = nullptr;
}

void Batch::add(const Problem& p) {
  // row reductions need whole rows -- except the scorer's single dot product, which two column blocks may add up (e_atomic)
  const bool scorer_blocks = p.epi == EPI_TANH_H && p.w2 && p.N > bn && narrow && p.N <= 2 * bn;
  const bool att_blocks = p.epi == EPI_ATT && p.N > bn && e_block_stride > 0;
  // ... or, with a partial buffer per block (e_block_stride), any number of them: the scorer kernel adds the partials in block order
  const bool scorer_parts = p.epi == EPI_TANH_H && p.w2 && p.N > bn && !scorer_blocks && e_block_stride > 0;
  if ((p.epi == EPI_ATT || (p.epi == EPI_TANH_H && p.w2)) && p.N > bn && !scorer_blocks && !att_blocks && !scorer_parts) { err = hipErrorInvalidValue; return; }
  if (tn) {
    const bool want = tn_pp_ok(p);
    if (L.nprob > 0 && want != tn_pp) flush();      // (a launch is one kernel: problems of the other kind start the next one)
    if (L.nprob == 0) tn_pp = want;
  }
  const int bn = tn_pp ? (1 << 30) : this->bn;
  for (int n0 = 0; n0 < p.N; n0 += bn) {
    Problem q = p;
    q.N = (p.N - n0 < bn) ? p.N - n0 : bn;
    auto adv = [](const float* ptr, size_t elems, bool bf) { return (const float*)((const char*)ptr + elems * (bf ? 2 : 4)); };
    for (int i = 0; i < q.nseg; ++i) {
      if (tn) {
        q.seg[i].B = adv(q.seg[i].B, (size_t)n0, q.elt);
        q.seg[i].vecB = q.elt ? (((reinterpret_cast<uintptr_t>(q.seg[i].B) & 15) == 0) && q.seg[i].ldb % 8 == 0 && q.N % 8 == 0)
                              : vec_ok(q.seg[i].B, q.seg[i].ldb, q.N);
      } else {
        q.seg[i].B = adv(q.seg[i].B, (size_t)n0 * q.seg[i].ldb, q.elt);       // B is [N][ldb]: a column block of C is a row block of B
      }
    }
    q.C = (float*)adv(q.C, (size_t)n0, q.io & 1);
    q.drop_col0 = p.drop_col0 + n0;
    if (q.bias) q.bias += n0;
    if (q.bias2) q.bias2 += n0;
    if (q.out1) q.out1 = (float*)adv(q.out1, (size_t)n0, q.io & 2);
    if (q.in0) q.in0 = adv(q.in0, (size_t)n0, q.io & 4);
    if (q.in1) q.in1 = adv(q.in1, (size_t)n0, q.io & 8);
    if (q.c32) q.c32 += n0;
    if (q.gin) q.gin += n0;
    if (q.in2) q.in2 = adv(q.in2, (size_t)n0, q.io & 16);
    if (q.out2) q.out2 = (float*)adv(q.out2, (size_t)n0, q.io & 32);
    if (scorer_blocks) { q.w2 += n0; q.e_atomic = 1; }
    if (scorer_parts) { q.w2 += n0; q.e = p.e + (size_t)(n0 / bn) * (size_t)e_block_stride; q.e_atomic = 2; }
    if (att_blocks) { q.w2 += n0; q.u += n0; q.e = p.e + (size_t)(n0 / bn) * (size_t)e_block_stride; q.e_atomic = 2; }      // (2: own partial buffer, plain stores)
    if (L.nprob == GH_MAX_PROBLEMS) flush();
    L.p[L.nprob++] = q;
    const int bm_eff = tn_pp ? 256 : (tn && q.elt) ? 128 : bm;      // (bf16 TN: the 128 x 320 tile; all problems of a TN launch share the storage mode)
    const int mt = (q.M + bm_eff - 1) / bm_eff;
    if (mt > L.m_tiles) L.m_tiles = mt;
    if (tn_pp && (q.N + 255) / 256 > L.n_tiles) L.n_tiles = (q.N + 255) / 256;
    if (q.seg[0].K > k_total) k_total = q.seg[0].K;
  }
}

void Batch::flush() {
  if (L.nprob == 0 || err != hipSuccess) { reset(); return; }
  if (tn) {
    const int n_inner = L.m_tiles * L.nprob;
    constexpr int target = 2304;
    int ks = (target + n_inner - 1) / n_inner;   // three resident rounds of 256 CUs x 3 workgroups (measured on the bench step: 1152 -> 2.06 ms,
                                                 // 1536 -> 1.95, 2304 -> 1.86, 3072 -> 1.84 but more partials to reduce; one round 20 % slower)
    // shortest K chunk: 256 rows (fp32).  bf16 storage, wide outputs (h = 768: 64 x 320 partial tiles of 80 KB each): a single
    // 768 x 768 product split into 64 chunks writes and re-reads more partial-tile bytes than it streams operands
    constexpr int min_rows16 = 4096;      // (A/B on configs[4]: 256 / 1024 / 2048 / 4096 rows = 106.76 / 106.72 / 106.81 / 107.17 K pairs/s)
    const int min_rows = L.p[0].elt ? min_rows16 : 256;
    const int ks_max = (k_total / min_rows > 1) ? k_total / min_rows : 1;
    if (ks > ks_max) ks = ks_max;
    if (ks < 1) ks = 1;
    // The K chunks are dealt round-robin to the 8 XCDs (chunk c runs on XCD c % 8, gemm_tn.hip.h): a chunk count that is
    // not a multiple of 8 leaves some XCDs one chunk (1 / 8 of their work at 65 chunks) more than the others.  Measured on
    // the bench step (A/B, one box): 65 chunks 158.6 K pairs/s, 72 chunks 159.9 K, 85 chunks 156.4 K.
    const int align = tn_pp ? 64 : L.p[0].elt ? 32 : 16;      // K tile of the kernel (bf16 storage: 32 rows, ping-pong tile: 64)
    if (tn_pp) {
      // one workgroup per CU: as many K chunks as fill ONE round of 256 workgroups when that occupies >= 85 % of them (h = 768: a
      // cell's 7 outputs = 63 tiles x 4 chunks = 252), else two rounds; chunks of at least 1024 rows.  The XCD rule does not apply:
      // the kernel deals its items to the XCDs in runs.
      const int tiles = L.nprob * L.m_tiles * L.n_tiles;
      const int ks1 = 256 / tiles > 0 ? 256 / tiles : 1, ks2 = 512 / tiles > 0 ? 512 / tiles : 1;
      const double e1 = tiles * ks1 / 256.0, e2 = tiles * ks2 / 512.0;
      ks = (e1 >= 0.85 || e1 >= e2) ? ks1 : ks2;
      const int kmax = k_total / 1024 > 1 ? k_total / 1024 : 1;
      if (ks > kmax) ks = kmax;
      // (the partial tiles must fit the workspace: fewer chunks otherwise)
      size_t out_bytes = 0;
      for (int i = 0; i < L.nprob; ++i) out_bytes += ((size_t)L.p[i].M * L.p[i].N + (cs_out[i] ? (size_t)L.p[i].M : 0)) * sizeof(float);
      while (ks > 1 && (size_t)ks * out_bytes > g_ws_bytes) --ks;
    } else
    if (ks >= 12) ks = ((ks + 4) / 8) * 8;
    int chunk = (k_total + ks - 1) / ks;
    chunk = ((chunk + align - 1) / align) * align;
    L.kchunk = chunk;
    L.ksplit = (k_total + chunk - 1) / chunk;
    if (tn_pp) L.per = (L.nprob * L.m_tiles * L.n_tiles * L.ksplit + 7) / 8;
    if (!tn_pp && L.ksplit >= 12 && L.ksplit % 8 != 0) {      // rounding the chunk up dropped a chunk or two: stretch the chunks to the multiple of 8 below
      const int k8 = (L.ksplit / 8) * 8;
      chunk = (((k_total + k8 - 1) / k8 + align - 1) / align) * align;
      if ((k_total + chunk - 1) / chunk % 8 == 0) { L.kchunk = chunk; L.ksplit = (k_total + chunk - 1) / chunk; }
    }
    // partial tiles -> workspace when it is big enough and every output is float4-shaped
    size_t need = 0;
    bool want_cs0 = false;
    for (int i = 0; i < L.nprob; ++i) want_cs0 = want_cs0 || cs_out[i] != nullptr;
    // (a single chunk also goes through the workspace when the ping-pong kernel runs it -- it only writes partial tiles -- or when
    //  bf16 operands want their bias gradient: that rides in the fused kernels' workspace path only)
    bool ws_ok = g_ws != nullptr && (L.ksplit > 1 || tn_pp || (want_cs0 && L.p[0].elt));
    bool any_cs = false;
    for (int i = 0; i < L.nprob && ws_ok; ++i) {
      if (L.p[i].N % 4) ws_ok = false;
      need += (size_t)L.ksplit * L.p[i].M * L.p[i].N * sizeof(float);
      if (cs_out[i]) { need += (size_t)L.ksplit * L.p[i].M * sizeof(float); any_cs = true; }
    }
    bool want_cs = false;
    for (int i = 0; i < L.nprob; ++i) want_cs = want_cs || cs_out[i] != nullptr;
    if (any_cs && !(ws_ok && need <= g_ws_bytes && fast_ok(L, true) && (g_gemm_mode != 1 || L.p[0].elt))) any_cs = false;
    if (want_cs && !any_cs) {
      // this launch cannot carry its column sums (no workspace, generic kernel): fp32 operands get them from the streaming
      // kernel right here, so that a Batch whose problems span several launches (h = 768: 21 column-block problems) never ends
      // up with some bias gradients fused and others missing; bf16 operands have no such kernel -- the caller is told
      for (int i = 0; i < L.nprob; ++i) {
        if (!cs_out[i]) continue;
        const Seg& sg = L.p[i].seg[0];
        if (L.p[i].elt || sg.lda != L.p[i].M) { colsum_missed = true; continue; }
        if (launch_colsum3(sg.A, nullptr, nullptr, cs_out[i], nullptr, nullptr, sg.K, L.p[i].M, s, cs_out2[i], nullptr, nullptr)) colsum_missed = true;
        else colsum_fused = true;
      }
    }
    if (ws_ok && need <= g_ws_bytes) {
      ReduceArgs R;
      R.n = L.nprob;
      float* w = g_ws;
      int max_elems = 0;
      for (int i = 0; i < L.nprob; ++i) {
        Problem& q = L.p[i];
        R.it[i] = ReduceItem{w, q.C, q.M, q.N, q.ldc, L.ksplit, (long long)q.M * q.N};
        q.C = w; q.ldc = q.N; q.epi = EPI_STORE; q.accumulate = 0; q.split_stride = (long long)q.M * q.N;
        w += (size_t)L.ksplit * q.M * q.N;
        if (q.M * (q.N / 4) > max_elems) max_elems = q.M * (q.N / 4);
      }
      ReduceArgs RC;          // bias-gradient partials [ksplit][M] behind the tiles, summed into one or two outputs
      RC.n = 0;
      int max_cs = 0;
      for (int i = 0; i < L.nprob && any_cs; ++i) {
        Problem& q = L.p[i];
        if (!cs_out[i]) continue;
        q.colsum = w; q.colsum_stride = q.M;
        RC.it[RC.n++] = ReduceItem{w, cs_out[i], 1, q.M, q.M, L.ksplit, (long long)q.M};
        if (cs_out2[i] && RC.n < GH_MAX_PROBLEMS) RC.it[RC.n++] = ReduceItem{w, cs_out2[i], 1, q.M, q.M, L.ksplit, (long long)q.M};
        w += (size_t)L.ksplit * q.M;
        if (q.M / 4 > max_cs) max_cs = q.M / 4;
      }
      hipError_t e = launch_any();
      if (e != hipSuccess) err = e;
      // one reduce launch: the bias-gradient partials ride behind the tiles (their workgroups beyond the first exit at once)
      for (int i = 0; i < RC.n; ++i) R.it[R.n++] = RC.it[i];
      if (max_cs > max_elems) max_elems = max_cs;
      hipLaunchKernelGGL(reduce_partials_kernel, dim3((max_elems + 255) / 256, R.n), dim3(256), 0, s, R);
      if (RC.n > 0) colsum_fused = true;
      e = hipGetLastError();
      if (e != hipSuccess) err = e;
      reset();
      return;
    }
  }
  if (tn && tn_pp) { err = hipErrorInvalidValue; reset(); return; }      // (the ping-pong kernel writes partial tiles only: no workspace, no launch)
  if (!tn && nt_split_plan()) return;
  hipError_t e = launch_any();
  if (e != hipSuccess) err = e;
  reset();
}

hipError_t Batch::launch_any() {
  if (tn && tn_pp) return launch_tn_pp(L, s);
  if (narrow && !tn && L.ksplit == 1 && !L.p[0].elt) return launch_cfg<2, 2, 5>(L, tn, s);
  if (big && !tn && L.ksplit == 1 && !L.p[0].elt) {
    // Occupancy-aware tile choice.  The chip holds 768 workgroups of either configuration (3 per CU); a grid of 64-row
    // tiles that ends in a thinly filled last round (e.g. 976 workgroups = 1.27 rounds, the node-compact single-problem
    // launches) runs faster on 32-row tiles (1937 workgroups = 2.52 rounds): measured 83 vs 78 TF at K = 300.
    const double r = (double)L.m_tiles * L.nprob / 768.0;
    const double frac = r - (double)(long long)r;
    if (g_gemm_mode != 1 && r < 3.0 && frac > 0.02 && frac < 0.45) {
      int mt = 0;
      for (int i = 0; i < L.nprob; ++i) { const int t = (L.p[i].M + 31) / 32; if (t > mt) mt = t; }
      L.m_tiles = mt;
      return launch_cfg<1, 4, 5>(L, tn, s);
    }
  }
  if (wide256) {
    // the ping-pong loop's preconditions (gemm_nt_pp.hip.h): whole 64-deep K tiles, no K split, no dropout inside the K loop
    bool ok = L.ksplit == 1;
    for (int i = 0; i < L.nprob; ++i) {
      if (L.p[i].drop_mode == 1) ok = false;
      for (int j = 0; j < L.p[i].nseg; ++j) if (L.p[i].seg[j].K % 64) ok = false;
    }
    if (ok) return launch_cfg<2, 4, 4, 8>(L, tn, s);
    int mt = 0;
    for (int i = 0; i < L.nprob; ++i) { const int t = (L.p[i].M + 127) / 128; if (t > mt) mt = t; }
    L.m_tiles = mt;
    return launch_cfg<2, 2, 8, 4>(L, tn, s);
  }
  if (wide) return launch_cfg<2, 2, 8, 4>(L, tn, s);
  return big ? launch_cfg<2, 2, 10>(L, tn, s) : launch_cfg<1, 4, 5>(L, tn, s);
}

// Few-row NT GEMMs (evidence level, head): too few row tiles to fill 256 CUs, so split K across
// workgroups, keep the partial tiles in the workspace and finish with nt_finish_kernel.
bool Batch::nt_split_plan() {
  const int blocks = L.m_tiles * L.nprob;
  constexpr int max_blocks = 96;
  if (g_ws == nullptr || blocks >= max_blocks || !fast_ok(L, false)) return false;
  int tmax = 0;          // K tiles over the concatenated segments (every problem of a launch is split alike)
  for (int i = 0; i < L.nprob; ++i) {
    const Problem& q = L.p[i];
    if (q.epi == EPI_ATOMIC || q.epi == EPI_GATE_PRE || q.drop_mode != 0 || (q.epi == EPI_TANH_H && q.w2) || q.seg0_rows > 0 || q.elt) return false;   // (fp32 problems only)
    int t = 0;
    for (int j = 0; j < q.nseg; ++j) t += (q.seg[j].K + 15) / 16;
    if (i > 0 && t != tmax) return false;
    tmax = t;
  }
  int ks = tmax / 4;
  // workgroups wanted: one per CU -- two for long contractions (>= 128 K tiles, e.g. the evidence-level attention at h = 768:
  // K = 6272), where a split-K workgroup is MFMA-bound rather than latency-bound (A/B configs[4] bf16: 256 / 512 / 768 =
  // 107.7 / 108.7 / 108.1 K pairs/s; headline and Snopes-count steps unchanged at any of them)
  const int tgt = tmax >= 128 ? 512 : 256;
  const int want = (tgt + blocks - 1) / blocks;
  if (ks > want) ks = want;
  if (ks < 2) return false;
  const int ct = (tmax + ks - 1) / ks;     // tiles per chunk
  ks = (tmax + ct - 1) / ct;
  if (ks < 2) return false;
  size_t need = 0;
  for (int i = 0; i < L.nprob; ++i) need += (size_t)ks * L.p[i].M * L.p[i].N * sizeof(float);
  if (need > g_ws_bytes) return false;
  FinishArgs F;
  F.n = L.nprob;
  float* w = g_ws;
  int max_m = 0;
  for (int i = 0; i < L.nprob; ++i) {
    Problem& q = L.p[i];
    F.it[i] = FinishItem{w, (long long)q.M * q.N, ks, q.M, q.N, q.epi, q.accumulate, q.ldc,
                         q.C, q.bias, q.bias2, q.out1, q.in0, q.in1, q.u, q.w2, q.e, q.ldu, q.R, q.heads, q.rowg};
    q.C = w; q.ldc = q.N; q.epi = EPI_STORE; q.accumulate = 0; q.bias = nullptr; q.bias2 = nullptr;
    q.split_stride = (long long)q.M * q.N;
    w += (size_t)ks * q.M * q.N;
    if (q.M > max_m) max_m = q.M;
  }
  L.ksplit = ks;
  L.kchunk = ct * 16;
  hipError_t e = launch_any();
  if (e != hipSuccess) err = e;
  // many partials over few rows: a workgroup per row (the four waves share the partials); otherwise a wave per row
  F.split = (ks >= 16 && max_m <= 8192) ? 1 : 0;      // (ks = 9, M = 960 -- the claim cell, the evidence-level attention -- measured equal or slower split)
  hipLaunchKernelGGL(nt_finish_kernel, dim3(F.split ? max_m : (max_m + 3) / 4, F.n), dim3(256), 0, s, F);
  split_done = true;
  e = hipGetLastError();
  if (e != hipSuccess) err = e;
  reset();
  return true;
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
