// The arithmetic of launch_spmm (spmm_ops.hip) without its launches: which aggregation kernel a shape takes and with what slabs,
// grid and dynamic LDS.  Plain host C++ with no HIP call and no HIP include, so that tools/spmm_plan_sweep.cpp can walk it
// on the CPU.  Every tuning constant sits here next to the measurement that justifies it.
#pragma once
#include <stddef.h>

namespace gh {

enum SpmmKind {
  SPMM_MFMA_BF16,      // spmm_mfma_bf16_kernel: bf16 rows, r <= 128, h % 8 == 0
  SPMM_LIST_F32,       // spmm_list_kernel<false, 2>: float4-shaped fp32 rows
  SPMM_LIST_BF16,      // spmm_list_kernel<true, 3>: bf16 rows with an even number of float4 columns
  SPMM_WALK_BF16,      // spmm_kernel<4, true>
  SPMM_WALK_V4,        // spmm_kernel<4>
  SPMM_WALK_V1,        // spmm_kernel<1>: rows that are not float4-shaped
  SPMM_NKINDS
};

struct SpmmPlan {
  SpmmKind kind;
  int slab;               // columns per slab: float4 columns (bit walk V = 1: scalars; matrix pipe: bf16 elements)
  int nslab;              // slabs per row
  int seq;                // consecutive slabs of one graph that a workgroup walks (bit walk: 1, the grid's y is the slab)
  unsigned grid_x, grid_y;
  size_t lds;             // dynamic LDS bytes
  int cap;                // edge-list capacity (edge-list kinds only)
};

// n graphs of r (<= 256) padded nodes, h columns; bf16: x and y hold bf16; v4: h % 4 == 0 and 16-byte aligned rows (bf16 needs it);
// compact: node-compact layout (goff != NULL)
inline SpmmPlan spmm_plan(int n, int r, int h, bool bf16, bool v4, bool compact) {
  SpmmPlan p = {};
  const int W = (r + 63) / 64;
  const int V = v4 ? 4 : 1;
  const int hv = h / V;
  // slab: <= 32 float4 (or 128 scalars) per row, as even as possible
  // (sized so that a workgroup's slab stays under ~32 KB of LDS: four to five workgroups per CU, also at R = 200)
  // round 4, A/B on one box: many graphs of <= 128 nodes (the bench step's 960 x 100) run 0.4 % faster per STEP on 24 KB slabs (five
  // slabs of 15 float4 instead of four of 19), few graphs (218: the realistic step) 1 % slower
  const int cap_kb = (compact && n >= 512 && r <= 128 && !bf16) ? 24 : 32;      // (node-compact layout only: the padded 100-row graphs run 58 -> 69 us on 24 KB slabs)   // measured per step: 48 KB -> 0.314 ms, 32 -> 0.288, 24 -> 0.294, 16 -> 0.344 (R = 100); R = 200: 0.60 -> 0.43
  const int lds_cap = (cap_kb * 1024) / (r * (v4 ? 16 : 4));
  const int slab_max = v4 ? (lds_cap < 32 ? (lds_cap < 4 ? 4 : lds_cap) : 32) : (lds_cap < 128 ? (lds_cap < 16 ? 16 : lds_cap) : 128);
  const int nslab = (hv + slab_max - 1) / slab_max;
  const int slab = (hv + nslab - 1) / nslab;
  if (bf16 && r <= 128 && h % 8 == 0) {
    // bf16 rows: the aggregation as a dense product per graph on the matrix pipe (spmm_mfma_bf16_kernel), slabs of 128 columns,
    // three of them per workgroup (few-graph launches: one)
    constexpr int sc = 128, mseq = 3;
    const int ns = (h + sc - 1) / sc;
    int seq = n < 256 ? 1 : mseq;
    if (seq > ns) seq = ns;
    const int nchunk = (ns + seq - 1) / seq;
    p.kind = SPMM_MFMA_BF16;
    p.slab = sc; p.nslab = ns; p.seq = seq;
    p.grid_x = (unsigned)(((n + 7) / 8) * 8 * nchunk); p.grid_y = 1;
  } else if (v4 && r <= 256 && (!bf16 || hv % 2 == 0)) {
    // edge-list slab kernel, LDS-DMA staging -- 62 us vs 69 us for the bit-walk slab kernel on 960 x 100 x 300 Zipf word graphs,
    // 50 vs 61 us on hub-free graphs.  fp32 rows: two columns per thread.  bf16 rows: three -- a bf16 column is an 8-byte LDS read and
    // four unpack instructions in front of its FMAs, the per-edge overhead (list entry, address) weighs more than in fp32: 960 graphs
    // x h = 768, window 5: 148.6 / 126.9 / 120.0 / 122.2 / 126.2 us at 1 / 2 / 3 / 4 / 6 columns per thread (fewer, longer work items
    // per row beyond three: the last round of items is thinly filled).  LDS pitch = slab columns.
    // (removed, DESIGN 4.5: LDS-free gather variants -- thread-per-float4 / wave-per-row, measured equal or slower: with ~8K waves in
    //  flight their sliding-window working set (~49 MB) thrashes the 32 MB of L2 -- and a graph-per-workgroup pipeline over two LDS
    //  buffers, 74-85 us)
    const int cap = 10 * r;                        // edges per graph the list holds (a window-5 word graph has <= 9 R)
    int lslab = slab;
    int ns = nslab;
    if (bf16) {                                    // bf16 LDS image: 8 B per column -> twice the columns per slab, kept even
      int smax = (cap_kb * 1024) / (r * 8);
      smax = smax > 64 ? 64 : (smax < 4 ? 4 : smax);
      smax &= ~1;
      const int nsb = (hv + smax - 1) / smax;
      lslab = (((hv + nsb - 1) / nsb) + 1) & ~1;
      ns = (hv + lslab - 1) / lslab;
    }
    // Rows that are whole 128-byte lines (h = 768: 1536 B in bf16, 3072 B in fp32): slabs of whole lines.  The even split above
    // gives 40 bf16 columns = 320 B per row and slab -- 2.5 lines, every slab boundary inside a line that two workgroups fetch
    // (configs[4] bf16, A/B on one box: five slabs of 40 columns 0.675 ms of aggregation per step, four slabs of 48 columns =
    // 3 lines 0.607 ms; 64 columns = 51 KB of LDS per workgroup 0.91 ms).  Up to 40 KB of slab image per workgroup.
    {
      const int col_b = bf16 ? 8 : 16, per_line = 128 / col_b;            // float4 columns per 128-byte line
      constexpr int line_kb = 40;
      if (((size_t)h * (bf16 ? 2 : 4)) % 128 == 0 && hv % per_line == 0) {
        int best = 0;
        for (int c = per_line; c <= hv && (size_t)r * c * col_b <= (size_t)line_kb * 1024; c += per_line) best = c;
        if (best >= 2 * per_line) {
          const int nsl = (hv + best - 1) / best;
          int even = (((hv + nsl - 1) / nsl) + per_line - 1) / per_line * per_line;      // as even as whole lines allow
          lslab = even;
          ns = (hv + lslab - 1) / lslab;
        }
      }
    }
    // slabs per workgroup, measured inside the bench step (ms of aggregation per step at 1 / 2 / all slabs per workgroup):
    //   960 graphs, R = 100, h = 300 fp32 (4 slabs): 0.302 / 0.282 / 0.262;   640 graphs, R = 200 (8 slabs): 0.536 / 0.467 / 0.426;
    //   960 graphs, h = 768 bf16 image, window 5 (5 slabs): 0.634 / 0.620 / 0.698 -- long per-slab work: the whole graph in one
    //   workgroup leaves one thinly balanced round.  Few-graph launches (claim side) keep one slab per workgroup: latency.
    int seq = n < 256 ? 1 : (bf16 ? 2 : ns);
    if (seq > ns) seq = ns;
    p.kind = bf16 ? SPMM_LIST_BF16 : SPMM_LIST_F32;
    p.slab = lslab; p.nslab = ns; p.seq = seq; p.cap = cap;
    p.grid_x = (unsigned)(((n + 7) / 8) * 8 * ((ns + seq - 1) / seq)); p.grid_y = 1;
    p.lds = (size_t)r * lslab * (bf16 ? 8 : 16) + (size_t)cap * 8 + (size_t)(r + 1) * 4 + (size_t)r * 4 + 4 + (size_t)r * 8;   // + item table
  } else {
    p.kind = bf16 ? SPMM_WALK_BF16 : (v4 ? SPMM_WALK_V4 : SPMM_WALK_V1);
    p.slab = slab; p.nslab = nslab; p.seq = 1;
    p.grid_x = (unsigned)n; p.grid_y = (unsigned)nslab;
    p.lds = ((((size_t)r * slab * V) + 3) & ~(size_t)3) * 4 + (size_t)r * W * 8 + (size_t)r * 4;
  }
  return p;
}

}  // namespace gh
