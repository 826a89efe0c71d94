// Bitmask aggregation (spmm): the bit-walk slab kernel, the edge-list slab kernel and the bf16 aggregation on the matrix pipe.
// Which of them a launch takes, and with what slabs, grid and LDS, is spmm_plan (spmm_plan.h): plain host arithmetic.
#include "../../include/get_hip.h"
#include "device_utils.h"
#include "spmm_plan.h"

namespace gh {

// ------------------------------------------------------------------------------------------------
// aggregation  y[g][i][:] (+)= sum_{j in N(i)} w_ij x[g][j][:]       (wrapper.py:192)
// grid (graph, column slab).  The slab of x is staged in LDS once (coalesced 16 B/lane reads of the
// feature rows), the refined neighbour bit-rows and dinv sit beside it, and every output float4
// walks its row's set bits with ctz -- each feature row leaves HBM exactly once per slab.
// ------------------------------------------------------------------------------------------------
// BF (with V = 4): x and y hold bf16 (the bf16 storage pipeline); the slab is widened to fp32 when it is staged
template <int V, bool BF = false>   // V = 4: float4 columns, V = 1: scalar columns
__global__ void __launch_bounds__(256)
spmm_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
            const uint64_t* __restrict__ keep, const int32_t* __restrict__ goff, const float* __restrict__ x,
            float* __restrict__ y, int R, int H, int slab, int transpose, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int W = (R + 63) / 64;
  float* xs = reinterpret_cast<float*>(dsm);                                  // [R][slab*V]
  const size_t xs_floats = (((size_t)R * slab * V) + 3) & ~(size_t)3;           // keep rb 16 B aligned
  unsigned long long* rb = reinterpret_cast<unsigned long long*>(xs + xs_floats);              // [R][W]
  float* dv = reinterpret_cast<float*>(rb + (size_t)R * W);                    // [R]
  const int g = blockIdx.x, tid = threadIdx.x;
  const int c0 = blockIdx.y * slab;                 // first column (in units of V floats)
  const int HV = H / V;
  const int ncol = min(slab, HV - c0);
  // node-compact layout: graph g owns feature rows [goff[g], goff[g+1]) -- its real nodes only; bit rows, dinv and
  // vals keep their padded [g][R] indexing (node i of graph g is feature row goff[g] + i)
  const int row0 = goff ? goff[g] : g * R;
  const int NR = goff ? goff[g + 1] - row0 : R;
  if (NR <= 0) return;
  const float* xg = x + (size_t)row0 * H;
  // Stage everything with ONE memory round trip: the slab (up to SL 16-byte loads per thread from a clamped
  // index -- unconditional, so no branch or per-load s_waitcnt), this thread's bit-row word and dinv entry
  // are all issued back to back; sched_barrier keeps them ahead of the first LDS write (the scheduler otherwise
  // pairs each load with its store: one HBM latency per element).  Out-of-range slots rewrite the last
  // element with its own value, which keeps the stores unconditional too.
  {
    constexpr int SL = 12;
    const int total = NR * ncol;
    // bit rows / dinv first (R*W <= 1024 and R <= 256 -> at most 4 + 1 per thread); consumed after the slab
    unsigned long long mw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mw[u] = bits[(size_t)g * R * W + min(tid + u * 256, R * W - 1)];
    const float dvv = vals ? 0.f : dinv[(size_t)g * R + min(tid, R - 1)];
    for (int base = tid; base < total; base += SL * 256) {
      float4 tmp[SL];
#pragma unroll
      for (int k = 0; k < SL; ++k) {
        const int it = min(base + k * 256, total - 1);
        const int i = it / ncol, c = it % ncol;
        if (BF) tmp[k] = bf4_to_f4(reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(x) + ((size_t)row0 + i) * H)[c0 + c]);
        else if (V == 4) tmp[k] = reinterpret_cast<const float4*>(xg + (size_t)i * H)[c0 + c];
        else tmp[k].x = xg[(size_t)i * H + c0 + c];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < SL; ++k) {
        const int it = min(base + k * 256, total - 1);
        const int i = it / ncol, c = it % ncol;
        if (V == 4) reinterpret_cast<float4*>(xs)[i * slab + c] = tmp[k];
        else xs[i * slab + c] = tmp[k].x;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = min(tid + u * 256, R * W - 1);
      unsigned long long m = mw[u];
      if (keep) {
        const int i = it / W, w = it % W;
        const bool ki = (keep[(size_t)g * W + (i >> 6)] >> (i & 63)) & 1ull;
        if (!ki) m &= keep[(size_t)g * W + w];          // edge survives iff keep(i) || keep(j)
      }
      rb[it] = m;
    }
    if (!vals) dv[min(tid, R - 1)] = dvv;
  }
  __syncthreads();
  const float* vg = vals ? vals + (size_t)g * R * R : nullptr;
  float* yg = y + (size_t)row0 * H;
  for (int it = tid; it < NR * ncol; it += 256) {
    const int i = it / ncol, c = it % ncol;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float di = vals ? 0.f : dv[i];
    for (int w = 0; w < W; ++w) {
      unsigned long long m = rb[i * W + w];
      while (m) {
        const int j = (w << 6) + __builtin_ctzll(m);
        m &= m - 1;
        const float wt = vg ? (transpose ? vg[(size_t)j * R + i] : vg[(size_t)i * R + j]) : di * dv[j];
        if (V == 4) {
          const float4 xv = reinterpret_cast<const float4*>(xs)[j * slab + c];
          acc.x += wt * xv.x; acc.y += wt * xv.y; acc.z += wt * xv.z; acc.w += wt * xv.w;
        } else {
          acc.x += wt * xs[j * slab + c];
        }
      }
    }
    if (BF) {
      uint2* o = reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(y) + ((size_t)row0 + i) * H) + c0 + c;
      if (accumulate) { const float4 p = bf4_to_f4(*o); acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
      *o = f4_to_bf4(acc);
    } else if (V == 4) {
      float4* o = reinterpret_cast<float4*>(yg + (size_t)i * H) + c0 + c;
      if (accumulate) { const float4 p = *o; acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
      *o = acc;
    } else {
      float* o = yg + (size_t)i * H + c0 + c;
      *o = accumulate ? *o + acc.x : acc.x;
    }
  }
}

// Edge-list variant of the slab kernel (the default for float4-shaped rows).  The bit-walk version above spends ~25
// VALU instructions per (output float4, neighbour) -- 64-bit ctz / clear-lowest-bit / weight product per lane -- and was
// VALU-issue-bound (1.4 G lane-instructions per launch at the bench shape = 35 us of a 47 us launch).  Here the
// refined bit rows of the graph are expanded ONCE per workgroup into an LDS edge list {j, w_ij} (row-start offsets by a
// workgroup scan of the popcounts), and every thread owns CPT float4 columns of one row, so the inner loop per
// neighbour is one 8-byte list read, one address mad and CPT x (ds_read_b128 + 4 FMA).  Graphs whose edge count
// exceeds the list capacity (dense hand-overs) fall back to the bit walk inside the same kernel.
#ifdef GH_MEASURE
__device__ unsigned g_spmm_phase[8192 * 8];     // tool build: s_memtime ticks per phase and workgroup (thread 0); ~0.5 ns per tick on the box (calibrated on the kernel time)
#define SPMM_T(i) do { if (threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (blockIdx.x < 8192) g_spmm_phase[blockIdx.x * 8 + i] = (unsigned)(t_ - tprev_); tprev_ = t_; } } while (0)
#else
#define SPMM_T(i) do { } while (0)
#endif
template <bool BF, int CPT>
__global__ void __launch_bounds__(256)
spmm_list_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
                 const uint64_t* __restrict__ keep, const int32_t* __restrict__ goff, const float* __restrict__ x,
                 float* __restrict__ y, int R, int H, int slab, int cap, int transpose, int accumulate, int n, int nslab, int split, int seq,
                 const ZeroFill zf) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  // zero-fill ranges handed over by the caller (a few hundred KB: the first workgroups' threads cover them)
  if (zf.n0 > 0 || zf.n1 > 0) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4, st = (long long)gridDim.x * 256 * 4;
    for (long long i = i0; i < zf.n0; i += st) *reinterpret_cast<float4*>(zf.p0 + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = i0; i < zf.n1; i += st) *reinterpret_cast<float4*>(zf.p1 + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int W = (R + 63) / 64;
  float4* xs = reinterpret_cast<float4*>(dsm);                                                // [R][slab] fp32 rows ...
  const uint2* xs16 = reinterpret_cast<const uint2*>(dsm);                                    // ... or (BF) bf16 rows, 8 B per float4 column
  uint2* ent = reinterpret_cast<uint2*>(dsm + (size_t)R * slab * (BF ? 8 : 16));              // [cap] {j, w}
  unsigned long long* rb = reinterpret_cast<unsigned long long*>(ent);                        // [R][W] refined bit rows (fallback only; cap >= R*W)
  int* st = reinterpret_cast<int*>(ent + cap);                                                // [R + 1] row starts
  float* dv = reinterpret_cast<float*>(st + R + 1);                                           // [R]
  uint2* itm = reinterpret_cast<uint2*>(dv + R + 1);                                          // [R] work items ((2R + 1) floats behind ent: + 1 for 8-byte alignment)
  __shared__ int wsum[4];
  __shared__ int wsum2[4];                                                                    // groups of hub rows | of mid rows << 16
  __shared__ int ctr[2];                                                                      // extra items, scratch slots
  // Work decode (1-D grid).  A workgroup owns `seq` consecutive slabs of one graph and walks them one after the other: bit
  // rows, scan and edge list are paid once per workgroup (measured: ~8 us of set-up latency chain against ~5 us of data
  // movement per fp32 slab at h = 300).  Workgroups go round-robin over the 8 XCDs, each with its own L2: the chunks of
  // one graph sit next to each other in ONE XCD's queue, so the 128-byte lines that straddle a slab boundary and the
  // graph's bit rows / dinv / keep words are fetched from HBM once and hit that L2 for the sibling workgroups.
  int g, sl;
  {
    const int nchunk = (nslab + seq - 1) / seq;
    const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
    sl = (j % nchunk) * seq;
    g = (j / nchunk) * 8 + xcd;
    if (g >= n) return;
  }
#ifdef GH_MEASURE
  unsigned long long tprev_ = __builtin_amdgcn_s_memtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int c0 = sl * slab;
  // exact n / d for n, d < 2^16 by one multiply-high (a runtime integer division costs ~20 VALU instructions)
  // (d = 1 has no 32-bit magic: magic_of wraps to 0, and fdiv returns n itself -- rows of one or two float4 columns, h = 4, 8)
  auto magic_of = [](int d) { return (unsigned)(0xFFFFFFFFu / (unsigned)d) + 1u; };
  auto fdiv = [](int n, unsigned magic) { return magic ? (int)__umulhi((unsigned)n, magic) : n; };
  const int H4 = H / 4;
  int ncol = min(slab, H4 - c0);
  const int row0 = goff ? goff[g] : g * R;
  const int NR = goff ? goff[g + 1] - row0 : R;
  if (NR <= 0) return;
  // ---- stage.  Issue order = completion order on the vector-memory counter: the few small loads of this thread's row
  // (bit words, keep words, dinv) go first, the slab's 16-byte loads after them, so the list is built from the former
  // while the latter are still in flight.  sched_barrier pins that order.
  const int trow = min(tid, R - 1);
  unsigned long long mrow[4] = {0ull, 0ull, 0ull, 0ull}, kwd[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < W) {
      mrow[w] = bits[((size_t)g * R + trow) * W + w];
      if (keep) kwd[w] = keep[(size_t)g * W + w];
    }
  const float dvv = vals ? 0.f : dinv[(size_t)g * R + trow];
  __builtin_amdgcn_sched_barrier(0);
  // LDS-DMA (buffer_load_dwordx4 ... lds): the LDS image is linear in (row, column), so a wave's 64 lanes land in 1 KB of
  // consecutive LDS; no staging registers, no ds_write.  fp32: one 16-byte chunk = one float4 column.  BF: the image
  // stays bf16 (half the LDS, twice the slab), one chunk = two columns (the launcher keeps slabs even).
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(reinterpret_cast<const char*>(x) + (size_t)row0 * H * (BF ? 2 : 4)), 0, 0x7fffffff, 0x00020000);
  auto dma_slab = [&]() __attribute__((always_inline)) {
    const int cpr = BF ? ncol / 2 : ncol;                 // chunks per row
    const int chunks = NR * cpr;
    const unsigned mg_cpr = magic_of(cpr);
    for (int base = 0; base < chunks; base += 256) {
      const int it = base + tid;
      if (it < chunks) {
        const int i = fdiv(it, mg_cpr), c = it - i * cpr;
        const int off = BF ? (i * H + (c0 + 2 * c) * 4) * 2 : (i * H + (c0 + c) * 4) * 4;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xs + base + wave * 64), 16, off, 0, 0, 0);
      }
    }
  };
#ifdef GH_MEASURE
  const bool dbg_noagg = (split & 256) != 0, dbg_nodma = (split & 512) != 0;      // tool build: one half of the kernel at a time
  split &= 255;
  if (!dbg_nodma)
#endif
  dma_slab();
  __builtin_amdgcn_sched_barrier(0);
  SPMM_T(0);        // loads issued
  // this thread's row (tid < NR): refined words, degree
  int deg = 0;
  {
    bool ki = true;
    if (keep) {
      unsigned long long kw = kwd[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) if ((trow >> 6) == w) kw = kwd[w];
      ki = (kw >> (trow & 63)) & 1ull;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned long long m = (w < W && tid < NR) ? mrow[w] : 0ull;
      if (!ki) m &= kwd[w];                                    // edge survives iff keep(i) || keep(j)
      mrow[w] = m;
      deg += __popcll(m);
    }
  }
  if (tid < R) dv[tid] = dvv;
  // exclusive scan of deg over the 256 threads (and, alongside, the totals of the 8-edge groups of hub / mid-degree rows)
  constexpr int GS = 8;
  const int grp = (deg + GS - 1) / GS;
  const bool hub = deg > 4 * GS, mid = deg > 2 * GS && !hub;
  int inc = deg, inc2 = hub ? grp : (mid ? grp << 16 : 0);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o), v2 = __shfl_up(inc2, o);
    if (lane >= o) { inc += v; inc2 += v2; }
  }
  if (lane == 63) { wsum[wave] = inc; wsum2[wave] = inc2; }
  if (tid < 2) ctr[tid] = 0;
  SPMM_T(1);        // row words arrived, scan
  __syncthreads();
  SPMM_T(2);        // barrier 1
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) if (w < wave) base += wsum[w];
  const int nnz = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  const int start = base + inc - deg;
  const bool listed = nnz <= cap;                 // workgroup-uniform
  if (tid <= R) st[tid] = (tid < NR) ? start : nnz;
  if (R >= 256 && tid == 0) st[R] = nnz;
  // Work items.  A word graph has a few hub nodes (frequent words: degree up to ~R/2 against a mean of ~6); with one thread per
  // (row, column group) the hub's threads run 8x longer than the rest and the workgroup waits for them.
  // NUMERICS (every row, split or not, every layout): a row's edges are summed in groups of GS = 8 -- each group from zero
  // in edge order, the group sums then added in group order.  SCHEDULING: a row with more than two groups may hand each
  // group to an item of its own; the group sums then travel through scratch slots in the part of the slab image that the
  // graph's R - NR absent rows leave unused and are added by a short second pass.  Which rows split (hubs first, then the
  // mid-degree rows, as far as the slots reach) never changes a result bit.
  const int spare = split ? (BF ? (R - NR) / 2 : (R - NR)) : 0;
  const int hm = wsum2[0] + wsum2[1] + wsum2[2] + wsum2[3];
  const bool split_hub = listed && (hm & 0xffff) > 0 && (hm & 0xffff) <= spare;
  const bool split_mid = listed && (hm >> 16) > 0 && (hm & 0xffff) + (hm >> 16) <= spare;
  if (tid < NR) {
    if (listed) {
      // item tid = the row itself (or its first group); a split row's further groups are appended behind the NR rows
      const bool sp = (hub && split_hub) || (mid && split_mid);
      const int pcs = sp ? grp : 1;
      int k0 = 0, s0 = 0;
      if (sp) { k0 = NR + atomicAdd(&ctr[0], pcs - 1) - 1; s0 = atomicAdd(&ctr[1], pcs); }
      for (int p = 0; p < pcs; ++p) {
        const int eb = start + p * GS, ee = sp ? min(start + deg, eb + GS) : start + deg;
        itm[p == 0 ? tid : k0 + p] = make_uint2((unsigned)tid | ((unsigned)p << 8) | ((unsigned)pcs << 14) | ((unsigned)s0 << 20),
                                                (unsigned)eb | ((unsigned)ee << 16));
      }
      const float di = dvv;
      int e = start;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (w < W) {
          unsigned long long m = mrow[w];
          while (m) {
            const int j = (w << 6) + __builtin_ctzll(m);
            m &= m - 1;
            const float wt = vals ? (transpose ? vals[((size_t)g * R + j) * R + tid] : vals[((size_t)g * R + tid) * R + j])
                                  : di * dv[j];
            ent[e++] = make_uint2((unsigned)j, __builtin_bit_cast(unsigned, wt));
          }
        }
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w) if (w < W) rb[tid * W + w] = mrow[w];
    }
  }
  SPMM_T(3);          // list build (thread 0's own row)
  const int sl_end = min(nslab, sl + seq);
  for (int s_ = sl; s_ < sl_end; ++s_) {
  if (s_ > sl) {                // next slab of this graph: every thread is done with the previous image and its scratch slots
    __syncthreads();
    c0 = s_ * slab;
    ncol = min(slab, H4 - c0);
#ifdef GH_MEASURE
    if (!dbg_nodma)
#endif
    dma_slab();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the slab has landed (LDS-DMA is tracked by vmcnt)
  SPMM_T(4);          // slab wait
  __syncthreads();
  SPMM_T(5);          // barrier 2 (the slowest list builder / DMA)
#ifdef GH_MEASURE
  if (dbg_noagg) continue;
#endif
  // ---- aggregate: thread = (item, column group q); columns q, q + TPR, ...
  const int TPR = (ncol + CPT - 1) / CPT;
  const unsigned mg_tpr = magic_of(TPR);
  const float* vg = vals ? vals + (size_t)g * R * R : nullptr;
  auto store_row = [&](int i, int q, const int* cc, const float4* acc) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      if (q + k * TPR >= ncol) break;
      float4 a = acc[k];
      if (BF) {
        uint2* o = reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(y) + ((size_t)row0 + i) * H) + c0 + cc[k];
        if (accumulate) { const float4 p = bf4_to_f4(*o); a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w; }
        *o = f4_to_bf4(a);
      } else {
        float4* o = reinterpret_cast<float4*>(y + ((size_t)row0 + i) * H) + c0 + cc[k];
        if (accumulate) { const float4 p = *o; a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w; }
        *o = a;
      }
    }
  };
  if (listed) {
    float4* scr = reinterpret_cast<float4*>(dsm + (size_t)NR * ncol * (BF ? 8 : 16));      // [slot][ncol] fp32 partial rows
    const int nitems = NR + ctr[0];
    const bool any_split = ctr[1] > 0;            // workgroup-uniform
    const int nit = nitems * TPR;
    for (int it = tid; it < nit; it += 256) {
      const int kk = fdiv(it, mg_tpr), q = it - kk * TPR;
      const uint2 im = itm[kk];
      const int i = im.x & 255, pcs = (im.x >> 14) & 63;
      int cc[CPT];
      float4 acc[CPT];
#pragma unroll
      for (int k = 0; k < CPT; ++k) { cc[k] = min(q + k * TPR, ncol - 1); acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
      const int e1 = im.y >> 16, e00 = im.y & 0xffff;
      const int slot0 = (int)(im.x >> 20) + (int)((im.x >> 8) & 63);
      float4 part[CPT];
#pragma unroll
      for (int k = 0; k < CPT; ++k) part[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e = e00; e < e1; e += 2) {
        const uint2 ea = ent[e];
        const bool two = e + 1 < e1;
        const uint2 eb = ent[two ? e + 1 : e];
        const float wa = __builtin_bit_cast(float, ea.y);
        const float wb = two ? __builtin_bit_cast(float, eb.y) : 0.f;
        float4 xa[CPT], xb[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          if (BF) { xa[k] = bf4_to_f4(xs16[ea.x * ncol + cc[k]]); xb[k] = bf4_to_f4(xs16[eb.x * ncol + cc[k]]); }
          else { xa[k] = xs[ea.x * ncol + cc[k]]; xb[k] = xs[eb.x * ncol + cc[k]]; }
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          part[k].x += wa * xa[k].x; part[k].y += wa * xa[k].y; part[k].z += wa * xa[k].z; part[k].w += wa * xa[k].w;
          part[k].x += wb * xb[k].x; part[k].y += wb * xb[k].y; part[k].z += wb * xb[k].z; part[k].w += wb * xb[k].w;
        }
        if ((((e - e00) & (GS - 2)) == GS - 2) || e + 2 >= e1) {        // the group's last pair: fold the group sum into the row sum
#pragma unroll
          for (int k = 0; k < CPT; ++k) {
            acc[k].x += part[k].x; acc[k].y += part[k].y; acc[k].z += part[k].z; acc[k].w += part[k].w;
            part[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      }
      if (pcs == 1) {
        store_row(i, q, cc, acc);
      } else {                     // a split row's item holds exactly one group: acc = 0 + part
#pragma unroll
        for (int k = 0; k < CPT; ++k)
          if (q + k * TPR < ncol) scr[slot0 * ncol + cc[k]] = acc[k];
      }
    }
    if (any_split) {
      __syncthreads();
      for (int it = tid; it < nit; it += 256) {
        const int kk = fdiv(it, mg_tpr), q = it - kk * TPR;
        const uint2 im = itm[kk];
        const int pcs = (im.x >> 14) & 63;
        if (pcs == 1 || ((im.x >> 8) & 63) != 0) continue;
        const int i = im.x & 255, s0 = (int)(im.x >> 20);
        int cc[CPT];
        float4 acc[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) { cc[k] = min(q + k * TPR, ncol - 1); acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        for (int p = 0; p < pcs; ++p) {
#pragma unroll
          for (int k = 0; k < CPT; ++k) {
            const float4 v = scr[(s0 + p) * ncol + cc[k]];
            acc[k].x += v.x; acc[k].y += v.y; acc[k].z += v.z; acc[k].w += v.w;
          }
        }
        store_row(i, q, cc, acc);
      }
    }
  } else {
    const int nit = NR * TPR;
    for (int it = tid; it < nit; it += 256) {
      const int i = fdiv(it, mg_tpr), q = it - i * TPR;
      int cc[CPT];
      float4 acc[CPT];
#pragma unroll
      for (int k = 0; k < CPT; ++k) { cc[k] = min(q + k * TPR, ncol - 1); acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
      const float di = vals ? 0.f : dv[i];
      for (int w = 0; w < W; ++w) {
        unsigned long long m = rb[i * W + w];
        while (m) {
          const int j = (w << 6) + __builtin_ctzll(m);
          m &= m - 1;
          const float wt = vg ? (transpose ? vg[(size_t)j * R + i] : vg[(size_t)i * R + j]) : di * dv[j];
#pragma unroll
          for (int k = 0; k < CPT; ++k) {
            const float4 xv = BF ? bf4_to_f4(xs16[j * ncol + cc[k]]) : xs[j * ncol + cc[k]];
            acc[k].x += wt * xv.x; acc[k].y += wt * xv.y; acc[k].z += wt * xv.z; acc[k].w += wt * xv.w;
          }
        }
      }
      store_row(i, q, cc, acc);
    }
  }
  }     // slabs
  SPMM_T(6);          // aggregate + stores issued (thread 0)
}

// ---------------------------------------------------------------------------------------------------------------------
// Aggregation of the bf16 storage pipeline ON THE MATRIX PIPE (round 6).  The edge-list kernel above is VALU-issue-bound on bf16 rows
// (PMC on configs[4]: 44 M wave VALU instructions per launch = 72 us of a 122 us launch; every (edge, four columns) item costs a list
// read, an address, four unpack instructions and two packed FMAs), while the same sum as a DENSE product  y_g = A_g x_g  per graph
// (A_g: <= 128 x 128 normalised adjacency, 7 % dense; x_g: the graph's rows) is 2 R^2 h flops = 15 MFLOP per graph at h = 768 -- a
// few microseconds of v_mfma_f32_16x16x32_bf16 even though 93 % of the products are with zeros.
//   * A never exists in memory: lane (l15, q) BUILDS its MFMA operand -- row i = 16 mi + l15, columns 32 ks + 8 q .. + 7 -- from the
//     row's refined bit words and the graph's d^-1/2 values (or the dense values), once per workgroup, in registers.  The fp32
//     weights are split THREE ways into bf16 (hi + mid + lo: w - hi and r1 - mid are exact in fp32, the remainder after lo is below
//     2^-24 |w|), so the products with the bf16 activations are exact to fp32 precision and the accumulation is fp32: the result is
//     the edge-list kernel's up to fp32 summation order, then rounded ONCE to bf16.
//   * x_g is the B operand, k-major as it sits in memory: slabs of 128 columns (256 B per row) by LDS-DMA, fragments by two
//     ds_read_b64_tr_b16 each, 32-byte units XOR-swizzled on the source side exactly as in gemm_tn_pp.hip.h (256-byte pitch).  Rows
//     between NR and the next multiple of 32 are DMA'd with the out-of-range offset (zeros: 0 x stale LDS could be NaN).
//   * Wave w owns the row tiles mi = w and w + 4 (R <= 128) and walks the slab's column tiles; only ceil(NR / 32) k-steps and
//     ceil(NR / 16) row tiles are computed, so the work follows NR^2 in the node-compact layout.
// Preconditions (launch_spmm): bf16 rows, R <= 128, h % 8 == 0, 16-byte aligned rows.
// (round 6, measured equal and removed, DESIGN 4.5: eight waves with one row tile each; 64-column slabs in two buffers with the next
//  slab's DMA under the current slab's MFMAs)
__global__ void __launch_bounds__(256, 2)
spmm_mfma_bf16_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ dinv, const float* __restrict__ vals,
                      const uint64_t* __restrict__ keep, const int32_t* __restrict__ goff, const unsigned short* __restrict__ x,
                      unsigned short* __restrict__ y, int R, int H, int transpose, int accumulate, int n, int nslab, int seq) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  constexpr int WAVES = 4, NT = 8 / WAVES, NTHR = WAVES * 64;      // row tiles per wave: wave w owns mi = w + WAVES t
  constexpr int SC = 128, PITCH = SC * 2, CPR = PITCH / 16;      // slab columns, bytes per row, 16-byte chunks per row
  __shared__ __attribute__((aligned(16))) unsigned char xs[128 * 256];      // [row][PITCH], rows 0 .. KR - 1 of a slab
  __shared__ float dv[128];
  constexpr unsigned OOB = 0x80000000u;
  int g, sl;
  {
    const int nchunk = (nslab + seq - 1) / seq;
    const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
    sl = (j % nchunk) * seq;
    g = (j / nchunk) * 8 + xcd;
    if (g >= n) return;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  // row-tile owner: rotated by the graph's position in its XCD queue.  In the node-compact layout most graphs have five row tiles (65 nodes
  // on average), i.e. ONE wave with two tiles, and wave w of every workgroup runs on SIMD w.  (Measured: no effect -- the tile loop is not
  // bound by the matrix pipe of one SIMD; kept because it costs nothing.)
  const int wv = (wave + (g >> 3)) % WAVES;
  const int W = (R + 63) / 64;                 // 1 or 2 words per bit row
  const int row0 = goff ? goff[g] : g * R;
  const int NR = goff ? goff[g + 1] - row0 : R;
  if (NR <= 0) return;
  const int nks = (NR + 31) >> 5;              // k-steps of 32 graph rows
  const int KR = nks * 32;

  // ---- the slab DMA (issued first: the operand build below runs under its flight)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)row0 * H), 0, 0x7fffffff, 0x00020000);
  auto dma_slab = [&](int c0) __attribute__((always_inline)) {
    const int chunks = KR * CPR;
    for (int base = 0; base < chunks; base += NTHR) {
      const int it = base + tid;                       // (chunks is a multiple of the workgroup size: no partial iteration)
      const int i = it / CPR, sl16 = it % CPR;
      const int fz = ((i & 3) << 1) | (((i >> 3) & 1) << 3);
      const int c = sl16 ^ fz;
      const int col = c0 + 8 * c;
      const unsigned off = (i < NR && col < H) ? (unsigned)(i * H + col) * 2u : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xs + (base + wave * 64) * 16), 16, off, 0, 0, 0);
    }
  };
  // Issue order = completion order on the vector-memory counter: the few small loads (bit rows, keep words, d^-1/2) go FIRST, the slab's
  // DMA after them, so that the operand build below waits for the former with a counted vmcnt while the latter is still in flight.
  const float dvv = (tid < 128 && !vals && tid < NR) ? dinv[(size_t)g * R + tid] : 0.f;
  unsigned long long mw0[NT], mw1[NT], kw0 = ~0ull, kw1 = ~0ull;
  if (keep) { kw0 = keep[(size_t)g * W]; if (W > 1) kw1 = keep[(size_t)g * W + 1]; }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = 16 * (wv + WAVES * t) + l15;
    mw0[t] = 0ull; mw1[t] = 0ull;
    if (i < NR) {
      mw0[t] = bits[((size_t)g * R + i) * W];
      if (W > 1) mw1[t] = bits[((size_t)g * R + i) * W + 1];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  dma_slab(sl * SC);
  __builtin_amdgcn_sched_barrier(0);

  // ---- d^-1/2 of the graph's nodes (pattern mode) for everybody
  if (tid < 128) dv[tid] = dvv;
  // (a bare barrier: __syncthreads() would also drain vmcnt, i.e. wait for the slab)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  // ---- A operands of this wave's row tiles, three bf16 pieces each: aF[t][ks][piece]
  uint4 aF[NT][4][3];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int mi = wv + WAVES * t;
    const int i = 16 * mi + l15;
    const bool live = i < NR;
    unsigned long long m0 = mw0[t], m1 = mw1[t];
    if (live && keep) {
      const bool ki = (((i < 64 ? kw0 : kw1) >> (i & 63)) & 1ull) != 0;
      if (!ki) { m0 &= kw0; m1 &= kw1; }                // edge survives iff keep(i) || keep(j)
    }
    const float di = live && !vals ? dv[i] : 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int j0 = 32 * ks + 8 * q;
      const unsigned byte = (unsigned)(((ks < 2 ? m0 : m1) >> ((32 * (ks & 1)) + 8 * q)) & 0xffull);
      float w[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool on = (byte >> b) & 1u;
        float v = 0.f;
        if (vals) { if (on) v = transpose ? vals[((size_t)g * R + (j0 + b)) * R + i] : vals[((size_t)g * R + i) * R + (j0 + b)]; }
        else v = on ? di * dv[j0 + b] : 0.f;
        w[b] = v;
      }
      unsigned hi[4], mid[4], lo[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float a0 = w[2 * b], a1 = w[2 * b + 1];
        const unsigned h2 = pack_bf2(a0, a1);
        const float r0 = a0 - __builtin_bit_cast(float, h2 << 16), r1 = a1 - __builtin_bit_cast(float, h2 & 0xffff0000u);
        const unsigned m2 = pack_bf2(r0, r1);
        const float s0 = r0 - __builtin_bit_cast(float, m2 << 16), s1 = r1 - __builtin_bit_cast(float, m2 & 0xffff0000u);
        hi[b] = h2; mid[b] = m2; lo[b] = pack_bf2(s0, s1);
      }
      aF[t][ks][0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      aF[t][ks][1] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
      aF[t][ks][2] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
  }
  const bool t0_live = 16 * wv < NR, t1_live = NT > 1 && 16 * (wv + WAVES) < NR;      // wave-uniform

  // ---- transpose-read base: lane (p = l15, g = q) points at row 8 q + (p >> 2) (+4: second read, +32 ks), four columns 4 (p & 3)
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)xs;
  const int f5 = (l15 >> 2) | ((q & 1) << 2);
  const unsigned rbase = lds0 + (unsigned)((8 * q + (l15 >> 2)) * PITCH + 8 * (l15 & 3));
  auto tr_read = [&](unsigned addr) __attribute__((always_inline)) {
    uint2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
  };

  const int sl_end = min(nslab, sl + seq);
  for (int s_ = sl; s_ < sl_end; ++s_) {
    const int c0 = s_ * SC;
    if (s_ > sl) {
      __syncthreads();                    // every wave is done with the previous slab's image
      dma_slab(c0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int ntile = (min(SC, H - c0) + 15) >> 4;
    // column tiles in pairs over two fragment sets: the next tile's transpose reads (and, accumulating, its y values) are in flight
    // while the current tile's MFMAs run
    auto load_b = [&](int ni, uint2* b0, uint2* b1) __attribute__((always_inline)) {
      const unsigned ad = rbase + (unsigned)(((ni ^ f5) & 7) << 5);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (ks < nks) { b0[ks] = tr_read(ad + ks * 32 * PITCH); b1[ks] = tr_read(ad + ks * 32 * PITCH + 4 * PITCH); }
        else { b0[ks] = make_uint2(0u, 0u); b1[ks] = make_uint2(0u, 0u); }
    };
    auto tile = [&](int ni, uint2* b0, uint2* b1, uint2* nb0, uint2* nb1) __attribute__((always_inline)) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b1[0]), "+v"(b1[1]), "+v"(b1[2]), "+v"(b1[3]) :: "memory");
      if (ni + 1 < ntile) load_b(ni + 1, nb0, nb1);
      // acc[r] = y[row 16 mi + l15][column c0 + 16 ni + 4 q + r]: four consecutive bf16 = one 8-byte access
      const int col = c0 + 16 * ni + 4 * q;
      const int i0r = 16 * wv + l15, i1r = i0r + 16 * WAVES;
      const bool ok0 = i0r < NR && col < H, ok1 = NT > 1 && i1r < NR && col < H;
      uint2* o0 = reinterpret_cast<uint2*>(y + ((size_t)row0 + i0r) * H + col);
      uint2* o1 = reinterpret_cast<uint2*>(y + ((size_t)row0 + i1r) * H + col);
      uint2 p0 = make_uint2(0u, 0u), p1 = make_uint2(0u, 0u);
      if (accumulate & 1) { if (ok0) p0 = *o0; if (ok1) p1 = *o1; }
      f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < nks) {
          const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, make_uint4(b0[ks].x, b0[ks].y, b1[ks].x, b1[ks].y));
          // (smallest pieces first: the fp32 accumulator sees lo + mid before hi)
          if (t0_live) {
#pragma unroll
            for (int pc = 2; pc >= 0; --pc) acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, __builtin_bit_cast(bf16x8_t, aF[0][ks][pc]), acc0, 0, 0, 0);
          }
          if constexpr (NT > 1) {
            if (t1_live) {
#pragma unroll
              for (int pc = 2; pc >= 0; --pc) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, __builtin_bit_cast(bf16x8_t, aF[NT - 1][ks][pc]), acc1, 0, 0, 0);
            }
          }
        }
      }
#ifdef GH_MEASURE
      if (accumulate & 256) {      // tool build: everything but the stores
        if (acc0[0] + acc1[0] == 12345.678f) *o0 = make_uint2(0u, 0u);
        return;
      }
#endif
      if (ok0) {
        float4 v = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]);
        if (accumulate & 1) { const float4 pv = bf4_to_f4(p0); v.x += pv.x; v.y += pv.y; v.z += pv.z; v.w += pv.w; }
        *o0 = f4_to_bf4(v);
      }
      if (ok1) {
        float4 v = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
        if (accumulate & 1) { const float4 pv = bf4_to_f4(p1); v.x += pv.x; v.y += pv.y; v.z += pv.z; v.w += pv.w; }
        *o1 = f4_to_bf4(v);
      }
    };
#ifdef GH_MEASURE
    if (accumulate & 512) continue;      // tool build: set-up + slab DMA only
#endif
    uint2 bA0[4], bA1[4], bB0[4], bB1[4];
    load_b(0, bA0, bA1);
    for (int ni = 0; ni < ntile; ni += 2) {
      tile(ni, bA0, bA1, bB0, bB1);
      if (ni + 1 < ntile) tile(ni + 1, bB0, bB1, bA0, bA1);
    }
  }
#endif
}

#ifdef GH_MEASURE
extern "C" int gh_debug_spmm_phases(unsigned* out, int reset) {     // out: [8192][8]
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_spmm_phase), 8192 * 8 * sizeof(unsigned)) != hipSuccess) return 1;
  if (reset) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_spmm_phase)) != hipSuccess || hipMemset(p, 0, 8192 * 8 * sizeof(unsigned)) != hipSuccess) return 1; }
  return 0;
}
#endif

int launch_spmm(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep, const int32_t* goff,
                int m_real, const float* x, float* y, int n, int r, int h, int transpose, int accumulate, hipStream_t s, int bf16,
                const ZeroFill* zfp, bool* zf_done) {
  if (zf_done) *zf_done = false;
  GH_REQUIRE(r > 0 && r <= MAX_R, "spmm: padded graph size %d not in [1,%d]", r, MAX_R);
  GH_REQUIRE(vals || dinv, "spmm: need dinv or vals");
  const bool v4 = (h % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && ((reinterpret_cast<uintptr_t>(y) & 15) == 0);
  GH_REQUIRE(!bf16 || v4, "spmm: the bf16 variant needs h %% 4 == 0 and 16-byte aligned rows");
  SpmmPlan p = spmm_plan(n, r, h, bf16 != 0, v4, goff != nullptr);
  // No shape reaches the 64 KB a launch may have without an opt-in (tools/spmm_plan_sweep.cpp, DESIGN.md 4.23: at most 57 352 B on the
  // edge list, 41 984 B on the bit walk): a slab rule that changes this fails here, not in the launch
  GH_REQUIRE(p.lds <= 64 * 1024, "spmm: %zu B of LDS for r=%d, h=%d (the slab rule keeps a launch under 64 KB)", p.lds, r, h);
  const dim3 grid(p.grid_x, p.grid_y);
  // algorithmic bytes: x in + y out (+ y in when accumulating) + bit rows + dinv (or the touched dense values)
  const double rows = goff ? (double)m_real : (double)n * r;
  const double alg_bytes = (2.0 + (accumulate ? 1.0 : 0.0)) * rows * h * (bf16 ? 2.0 : 4.0) +
                           (double)n * ((double)r * words_for(r) * 8.0 + (vals ? (double)r * r * 4.0 : (double)r * 4.0));
  const int ptag = few_rows_tag(n, PROF_SPMM);
  prof_begin(s, ptag);
  switch (p.kind) {
    case SPMM_MFMA_BF16: {
      const unsigned short* x16 = reinterpret_cast<const unsigned short*>(x);
      unsigned short* y16 = reinterpret_cast<unsigned short*>(y);
#ifdef GH_MEASURE
      static const int mdbg = measure_env("GH_SPMM_MFMA_NOSTORE", 0);
      if (mdbg) accumulate |= 256 * mdbg;
#endif
      hipLaunchKernelGGL(spmm_mfma_bf16_kernel, grid, dim3(256), 0, s, bits, dinv, vals, keep, goff, x16, y16, r, h, transpose, accumulate, n, p.nslab, p.seq);
      break;
    }
    case SPMM_LIST_F32:
    case SPMM_LIST_BF16: {
      const void* fn = bf16 ? (const void*)spmm_list_kernel<true, 3> : (const void*)spmm_list_kernel<false, 2>;
      // split = 1: hub rows may hand their edge groups to items of their own (tool build: GH_SPMM_DBG << 8 runs one half of the kernel)
      static const int split = 1 | (measure_env("GH_SPMM_DBG", 0) << 8);
      ZeroFill zf = {nullptr, 0, nullptr, 0};
      if (zfp && (zfp->n0 % 4 == 0) && (zfp->n1 % 4 == 0) && ((reinterpret_cast<uintptr_t>(zfp->p0) | reinterpret_cast<uintptr_t>(zfp->p1)) & 15) == 0) {
        zf = *zfp;
        if (zf_done) *zf_done = true;
      }
      void* args[] = {(void*)&bits, (void*)&dinv, (void*)&vals, (void*)&keep, (void*)&goff, (void*)&x, (void*)&y, (void*)&r, (void*)&h,
                      (void*)&p.slab, (void*)&p.cap, (void*)&transpose, (void*)&accumulate, (void*)&n, (void*)&p.nslab, (void*)&split, (void*)&p.seq,
                      (void*)&zf};
      (void)hipLaunchKernel(fn, grid, dim3(256), args, p.lds, s);
      break;
    }
    case SPMM_WALK_BF16:
      hipLaunchKernelGGL((spmm_kernel<4, true>), grid, dim3(256), p.lds, s, bits, dinv, vals, keep, goff, x, y, r, h, p.slab, transpose, accumulate);
      break;
    case SPMM_WALK_V4:
      hipLaunchKernelGGL(spmm_kernel<4>, grid, dim3(256), p.lds, s, bits, dinv, vals, keep, goff, x, y, r, h, p.slab, transpose, accumulate);
      break;
    default:
      hipLaunchKernelGGL(spmm_kernel<1>, grid, dim3(256), p.lds, s, bits, dinv, vals, keep, goff, x, y, r, h, p.slab, transpose, accumulate);
      break;
  }
  prof_end(ptag, alg_bytes, s);
  GH_LAUNCH_CHECK();
  return 0;
}
}  // namespace gh

using namespace gh;

extern "C" int gh_spmm(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                       const int32_t* goff, int m_real, const float* x, float* y, int n, int r, int h, int transpose,
                       int accumulate, gh_stream_t stream) {
  if (n <= 0) return 0;
  return launch_spmm(bits, dinv, vals, keep, goff, m_real, x, y, n, r, h, transpose, accumulate, (hipStream_t)stream, 0);
}

extern "C" int gh_spmm_bf16(const uint64_t* bits, const float* dinv, const float* vals, const uint64_t* keep,
                            const int32_t* goff, int m_real, const void* x16, void* y16, int n, int r, int h, int transpose,
                            int accumulate, gh_stream_t stream) {
  if (n <= 0) return 0;
  GH_REQUIRE(h % 8 == 0, "spmm_bf16: h must be a multiple of 8");
  return launch_spmm(bits, dinv, vals, keep, goff, m_real, (const float*)x16, (float*)y16, n, r, h, transpose, accumulate, (hipStream_t)stream, 1);
}
