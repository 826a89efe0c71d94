// Ragged claim <-> evidence helpers (gh_seg_*: offsets, broadcast, sum, pad, unpad), the masked mean of the claim vector
// (gh_masked_mean_*), the evidence-level assembly of the right operand and its mask (gh_evd_assemble_*) and the node-compact
// layout plan (gh_ragged_plan, launch_ragged_plan).
#include "../../include/get_hip.h"
#include "common.h"

namespace gh {

// ---------------------------------------------------------------------------- ragged helpers (basic_fc_model.py:80-121)
__global__ void __launch_bounds__(256)
seg_offsets_kernel(const int64_t* __restrict__ counts, int B, int32_t* __restrict__ offsets,
                   int32_t* __restrict__ pair2claim, int b1, float* __restrict__ has) {
  __shared__ int total;
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int b = 0; b < B; ++b) { offsets[b] = acc; acc += (int)counts[b]; }
    offsets[B] = acc;
    total = acc;
  }
  __syncthreads();
  __threadfence_block();
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int lo = min(offsets[b], b1), hi = min(offsets[b + 1], b1);
    for (int p = lo; p < hi; ++p) pair2claim[p] = b;
  }
  // counts that sum to less than b1 (a caller bug the reference reports as a shape error): the rows beyond the last
  // claim map to claim 0 instead of staying uninitialised -- no out-of-bounds gather downstream
  for (int p = total + threadIdx.x; p < b1; p += blockDim.x) pair2claim[p] = 0;
  if (has)
    for (int b = threadIdx.x; b < B; b += blockDim.x) has[b] = counts[b] > 0 ? 1.f : 0.f;
}

__global__ void __launch_bounds__(256)
seg_broadcast_kernel(const float* __restrict__ src, const int32_t* __restrict__ pair2claim, float* __restrict__ dst,
                     int b1, int X) {
  const int p = blockIdx.x;
  const float* s = src + (size_t)pair2claim[p] * X;
  for (int i = threadIdx.x; i < X; i += blockDim.x) dst[(size_t)p * X + i] = s[i];
}

__global__ void __launch_bounds__(256)
seg_sum_kernel(const float* __restrict__ src, const int32_t* __restrict__ offsets, float* __restrict__ dst, int X) {
  const int b = blockIdx.x;
  const int lo = offsets[b], hi = offsets[b + 1];
  // (few workgroups, a serial walk over <= n_max rows: eight row loads in flight per trip, added in row order)
  for (int i = threadIdx.x; i < X; i += blockDim.x) {
    float acc = 0.f;
    for (int p = lo; p < hi; p += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)min(p + u, hi - 1) * X + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) if (p + u < hi) acc += v[u];
    }
    dst[(size_t)b * X + i] = acc;
  }
}

// dst[b][slot][0:X] = src[offsets[b]+slot] for slot < count(b), else 0   (dst row pitch dst_ld >= X)
__global__ void __launch_bounds__(256)
seg_pad_kernel(const float* __restrict__ src, const int32_t* __restrict__ offsets, float* __restrict__ dst, int n_max,
               int X, int dst_ld) {
  const int b = blockIdx.x / n_max, slot = blockIdx.x % n_max;
  const int lo = offsets[b], cnt = min(offsets[b + 1] - lo, n_max);
  float* d = dst + ((size_t)b * n_max + slot) * dst_ld;
  if (slot < cnt) {
    const float* s = src + (size_t)(lo + slot) * X;
    for (int i = threadIdx.x; i < X; i += blockDim.x) d[i] = s[i];
  } else {
    for (int i = threadIdx.x; i < X; i += blockDim.x) d[i] = 0.f;
  }
}
__global__ void __launch_bounds__(256)
seg_unpad_kernel(const float* __restrict__ src, const int32_t* __restrict__ offsets, float* __restrict__ dst,
                 int n_max, int X, int src_ld) {
  const int b = blockIdx.x / n_max, slot = blockIdx.x % n_max;
  const int lo = offsets[b], cnt = min(offsets[b + 1] - lo, n_max);
  if (slot >= cnt) return;
  const float* s = src + ((size_t)b * n_max + slot) * src_ld;
  float* d = dst + (size_t)(lo + slot) * X;
  for (int i = threadIdx.x; i < X; i += blockDim.x) d[i] = s[i];
}

// claim vector: sum_l hid[b][l][:] [ids[b][l] > 0] / len[b]   (graph_based_semantic_structure.py:145,153)
__global__ void __launch_bounds__(256)
masked_mean_fwd_kernel(const float* __restrict__ hid, const int32_t* __restrict__ ids, const float* __restrict__ lens,
                       float* __restrict__ dst, int L, int H) {
  const int b = blockIdx.x;
  const float inv = 1.f / lens[b];
  for (int i = threadIdx.x; i < H; i += blockDim.x) {
    float acc = 0.f;
    for (int l = 0; l < L; l += 8) {
      float v[8];
      int id[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int lc = min(l + u, L - 1);
        id[u] = ids[b * L + lc];
        v[u] = hid[((size_t)b * L + lc) * H + i];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) if (l + u < L && id[u] > 0) acc += v[u];
    }
    dst[(size_t)b * H + i] = acc * inv;
  }
}
__global__ void __launch_bounds__(256)
masked_mean_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ ids, const float* __restrict__ lens,
                       float* __restrict__ dhid, int L, int H) {
  const int b = blockIdx.x / L, l = blockIdx.x % L;
  const float sc = (ids[b * L + l] > 0) ? 1.f / lens[b] : 0.f;
  for (int i = threadIdx.x; i < H; i += blockDim.x) dhid[((size_t)b * L + l) * H + i] = g[(size_t)b * H + i] * sc;
}

// ---------------------------------------------------------------------------- evidence-level assembly
// graph_based_semantic_structure.py:157-170,195-215 in one launch: right[b][slot] = [ pad_right(avg)[b][slot] |
// article_source_embs(max(src, 0)) ], mask[b][slot] = (sum_r document[b][slot][r] >= 1).  Replaces seg_pad +
// masked_fill + embedding + cat + sum/compare/cast (8 launches).  One workgroup per (claim, slot).
template <typename TS, typename TD>
__global__ void __launch_bounds__(256)
evd_assemble_fwd_kernel(const float* __restrict__ avg, const int32_t* __restrict__ offsets, const float* __restrict__ table,
                        const TS* __restrict__ sources, const TD* __restrict__ document, float* __restrict__ right,
                        float* __restrict__ mask, int n_max, int Xa, int Ds, int R, int table_rows, unsigned int* __restrict__ clamped) {
  const int b = blockIdx.x / n_max, slot = blockIdx.x % n_max;
  const int lo = offsets[b], cnt = min(offsets[b + 1] - lo, n_max);
  float* d = right + (size_t)blockIdx.x * (Xa + Ds);
  if (slot < cnt) {
    const float* sp = avg + (size_t)(lo + slot) * Xa;
    for (int i = threadIdx.x; i < Xa; i += blockDim.x) d[i] = sp[i];
  } else {
    for (int i = threadIdx.x; i < Xa; i += blockDim.x) d[i] = 0.f;
  }
  if (Ds > 0) {
    long long sid = (long long)sources[blockIdx.x];
    // -1 padding -> row 0 (:166-168).  Any other id outside the table would raise in nn.Embedding (:169); here it is clamped
    // for memory safety and counted (gh_clamp_events)
    if ((sid < -1 || sid >= table_rows) && threadIdx.x == 0) atomicAdd(clamped + 2, 1u);
    if (sid < 0) sid = 0;
    if (sid >= table_rows) sid = table_rows - 1;
    const float* tp = table + (size_t)sid * Ds;
    for (int i = threadIdx.x; i < Ds; i += blockDim.x) d[Xa + i] = tp[i];
  }
  if (threadIdx.x < 64) {                                        // slot mask: any node id >= 1 (ids are non-negative)
    long long acc = 0;
    const TD* dp = document + (size_t)blockIdx.x * R;
    for (int r = threadIdx.x; r < R; r += 64) acc += (long long)dp[r];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) mask[blockIdx.x] = acc >= 1 ? 1.f : 0.f;
  }
}

// backward: d_avg = unpad(g[:, :, :Xa]);  d_table[s] += sum over the slots with source s of g[:, :, Xa:], summed in
// slot order by the FIRST slot that holds s (deterministic: no float atomics, no sort)
template <typename TS>
__global__ void __launch_bounds__(256)
evd_assemble_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ offsets, const TS* __restrict__ sources,
                        float* __restrict__ d_avg, float* __restrict__ d_table, int n_slots, int n_max, int Xa, int Ds, int table_rows) {
  extern __shared__ __attribute__((aligned(16))) int sids[];
  const int me = blockIdx.x;
  const int b = me / n_max, slot = me % n_max;
  const int lo = offsets[b], cnt = min(offsets[b + 1] - lo, n_max);
  const float* gp = g + (size_t)me * (Xa + Ds);
  if (slot < cnt && d_avg) {
    float* d = d_avg + (size_t)(lo + slot) * Xa;
    for (int i = threadIdx.x; i < Xa; i += blockDim.x) d[i] = gp[i];
  }
  // pairs beyond the claim's n_max-th evidence have no slot: their gradient rows are zeros, written by the claim's last slot (the
  // caller's d_avg needs no fill in front of this kernel)
  if (slot == n_max - 1 && d_avg) {
    const size_t z0 = (size_t)(lo + n_max) * Xa, z1 = (size_t)offsets[b + 1] * Xa;
    for (size_t i = z0 + threadIdx.x; i < z1; i += blockDim.x) d_avg[i] = 0.f;
  }
  if (Ds <= 0 || !d_table) return;
  // Padding slots (slot >= the claim's evidence count) are masked out of the evidence-level softmax, so their gradient
  // rows are exact zeros: they neither own nor join a source row (-1 never matches).  Without this every padding slot
  // maps to source 0 and ONE workgroup walks hundreds of zero rows (177 us at the realistic evidence counts).
  for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
    const int bi = i / n_max;
    const bool real = (i - bi * n_max) < min(offsets[bi + 1] - offsets[bi], n_max);
    const long long v = (long long)sources[i];
    sids[i] = real ? (v < 0 ? 0 : (v >= table_rows ? table_rows - 1 : (int)v)) : -1;      // same clamp as the forward
  }
  __syncthreads();
  const int mine = sids[me];
  if (mine < 0) return;
  __shared__ int earlier;
  if (threadIdx.x == 0) earlier = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < me; i += blockDim.x)
    if (sids[i] == mine) earlier = 1;
  __syncthreads();
  if (earlier) return;                                            // an earlier slot owns this source's row
  // later slots with the same source as a bit mask (ballot per 64 slots), then summed in slot order
  const int nw = (n_slots + 63) / 64;
  unsigned long long* match = reinterpret_cast<unsigned long long*>(sids + ((n_slots + 1) & ~1));
  for (int w0 = (threadIdx.x >> 6); w0 < nw; w0 += (blockDim.x >> 6)) {
    const int j = w0 * 64 + (threadIdx.x & 63);
    const unsigned long long m = __ballot(j < n_slots && j >= me && sids[j] == mine);
    if ((threadIdx.x & 63) == 0) match[w0] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Ds; i += blockDim.x) {
    float acc = 0.f;
    for (int w0 = me >> 6; w0 < nw; ++w0) {
      unsigned long long m = match[w0];
      while (m) {
        const int j = (w0 << 6) + __builtin_ctzll(m);
        m &= m - 1;
        acc += g[(size_t)j * (Xa + Ds) + Xa + i];
      }
    }
    d_table[(size_t)mine * Ds + i] += acc;
  }
}


// ------------------------------------------------------------------------------------------------
// node-compact layout plan.  goff = exclusive prefix sum of the node counts (one workgroup, n <= a few
// thousand graphs), then one workgroup per graph fills the row maps.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
ragged_scan_kernel(const int32_t* __restrict__ n_nodes, int n, int R, int32_t* __restrict__ goff) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int sum = 0;
  for (int g = lo; g < hi; ++g) sum += min(max(n_nodes[g], 0), R);
  part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan of the per-thread sums
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int g = lo; g < hi; ++g) { goff[g] = run; run += min(max(n_nodes[g], 0), R); }
  if (tid == 1023) goff[n] = part[1023];
}

__global__ void __launch_bounds__(256)
ragged_fill_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ node_ids, int n, int R,
                   int32_t* __restrict__ rowg, int32_t* __restrict__ src, int32_t* __restrict__ cids,
                   float* __restrict__ maskf) {
  const int g = blockIdx.x;
  const int row0 = goff[g], NR = goff[g + 1] - row0;
  const int pad0 = goff[n] + g * R - row0 - NR;
  for (int j = threadIdx.x; j < R; j += 256) {
    const int row = j < NR ? row0 + j : pad0 + j;
    rowg[row] = g;
    src[row] = g * R + j;
    const int id = (cids || maskf) ? node_ids[(size_t)g * R + j] : 0;
    if (cids) cids[row] = id;
    if (maskf) maskf[row] = id >= 1 ? 1.f : 0.f;       // the word attention's mask (doc >= 1, graph_based_semantic_structure.py:180)
  }
}

// The plan in ONE launch for n <= 4096 graphs: every workgroup sums the node counts in front of its graph itself (n loads of
// 4 bytes out of L2, 960 at the bench shape) instead of waiting for a one-workgroup scan kernel; optionally it also scatters
// its graph's node ids into the padded `document` tensor (gh_get_prepare).
__global__ void __launch_bounds__(256)
ragged_plan1_kernel(const int32_t* __restrict__ n_nodes, const int32_t* __restrict__ node_ids, int n, int R,
                    int32_t* __restrict__ goff, int32_t* __restrict__ rowg, int32_t* __restrict__ src, int32_t* __restrict__ cids,
                    float* __restrict__ maskf, const int64_t* __restrict__ slot, int32_t* __restrict__ document) {
  __shared__ int red[2][4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0, all = 0;
  for (int i = tid; i < n; i += 256) {
    const int v = min(max(n_nodes[i], 0), R);
    all += v;
    if (i < g) before += v;
  }
  for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
  if (lane == 0) { red[0][wave] = before; red[1][wave] = all; }
  __syncthreads();
  const int row0 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const int total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const int NR = min(max(n_nodes[g], 0), R);
  if (tid == 0) { goff[g] = row0; if (g == n - 1) goff[n] = total; }
  const int pad0 = total + g * R - row0 - NR;
  const size_t dst = (slot && document) ? (size_t)slot[g] * R : 0;
  for (int j = tid; j < R; j += 256) {
    const int row = j < NR ? row0 + j : pad0 + j;
    rowg[row] = g;
    src[row] = g * R + j;
    const int id = (cids || maskf || document) ? node_ids[(size_t)g * R + j] : 0;
    if (cids) cids[row] = id;
    if (maskf) maskf[row] = id >= 1 ? 1.f : 0.f;
    if (slot && document) document[dst + j] = id;
  }
}

}  // namespace gh

using namespace gh;

extern "C" int gh_seg_offsets(const int64_t* counts, int b, int32_t* offsets, int32_t* pair2claim, int b1, float* has,
                              gh_stream_t stream) {
  GH_REQUIRE(b > 0, "seg_offsets: b=%d", b);
  hipLaunchKernelGGL(seg_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, b, offsets, pair2claim, b1, has);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_seg_broadcast(const float* src, const int32_t* pair2claim, float* dst, int b1, int x,
                                gh_stream_t stream) {
  if (b1 <= 0) return 0;
  hipLaunchKernelGGL(seg_broadcast_kernel, dim3(b1), dim3(256), 0, (hipStream_t)stream, src, pair2claim, dst, b1, x);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_seg_sum(const float* src, const int32_t* offsets, float* dst, int b, int x, gh_stream_t stream) {
  if (b <= 0) return 0;
  hipLaunchKernelGGL(seg_sum_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, src, offsets, dst, x);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_seg_pad(const float* src, const int32_t* offsets, float* dst, int b, int n_max, int x, int dst_ld,
                          gh_stream_t stream) {
  if (b <= 0) return 0;
  hipLaunchKernelGGL(seg_pad_kernel, dim3(b * n_max), dim3(256), 0, (hipStream_t)stream, src, offsets, dst, n_max, x, dst_ld);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_seg_unpad(const float* src, const int32_t* offsets, float* dst, int b, int n_max, int x, int src_ld,
                            gh_stream_t stream) {
  if (b <= 0) return 0;
  hipLaunchKernelGGL(seg_unpad_kernel, dim3(b * n_max), dim3(256), 0, (hipStream_t)stream, src, offsets, dst, n_max, x, src_ld);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_masked_mean_fwd(const float* hid, const int32_t* ids, const float* lens, float* dst, int b, int l,
                                  int h, gh_stream_t stream) {
  if (b <= 0) return 0;
  hipLaunchKernelGGL(masked_mean_fwd_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, hid, ids, lens, dst, l, h);
  GH_LAUNCH_CHECK();
  return 0;
}
extern "C" int gh_masked_mean_bwd(const float* g, const int32_t* ids, const float* lens, float* dhid, int b, int l,
                                  int h, gh_stream_t stream) {
  if (b <= 0) return 0;
  hipLaunchKernelGGL(masked_mean_bwd_kernel, dim3(b * l), dim3(256), 0, (hipStream_t)stream, g, ids, lens, dhid, l, h);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_ragged_plan(const int32_t* n_nodes, const int32_t* node_ids, int n, int r, int32_t* goff,
                              int32_t* rowg, int32_t* src, int32_t* cids, float* maskf, gh_stream_t stream) {
  GH_REQUIRE(r > 0 && r <= MAX_R, "ragged_plan: r=%d not in [1,%d]", r, MAX_R);
  GH_REQUIRE((cids == nullptr && maskf == nullptr) || (node_ids != nullptr), "ragged_plan: cids / maskf need node_ids");
  if (n <= 0) return 0;
  return launch_ragged_plan(n_nodes, node_ids, n, r, goff, rowg, src, cids, maskf, nullptr, nullptr, (hipStream_t)stream, nullptr);
}

// slot / document: also scatter the node ids of graph g into document[slot[g]][:] (the composite batch preparation)
int gh::launch_ragged_plan(const int32_t* n_nodes, const int32_t* node_ids, int n, int r, int32_t* goff, int32_t* rowg, int32_t* src,
                           int32_t* cids, float* maskf, const int64_t* slot, int32_t* document, hipStream_t s, bool* scattered) {
  if (scattered) *scattered = false;
  if (n <= 4096 && (node_ids || !(slot && document))) {
    hipLaunchKernelGGL(ragged_plan1_kernel, dim3(n), dim3(256), 0, s, n_nodes, node_ids, n, r, goff, rowg, src, cids, maskf, slot, document);
    GH_LAUNCH_CHECK();
    if (scattered) *scattered = slot && document;
    return 0;
  }
  hipLaunchKernelGGL(ragged_scan_kernel, dim3(1), dim3(1024), 0, s, n_nodes, n, r, goff);
  hipLaunchKernelGGL(ragged_fill_kernel, dim3(n), dim3(256), 0, s, goff, node_ids, n, r, rowg, src, cids, maskf);
  GH_LAUNCH_CHECK();
  return 0;      // (*scattered stays false: the document scatter, if any, is still the caller's)
}

extern "C" int gh_evd_assemble_fwd(const float* avg, const int32_t* offsets, const float* table, int table_rows, const void* sources,
                                   int sources_i64, const void* document, int document_i64, int b, int n_max, int xa, int ds,
                                   int r, float* right, float* mask, gh_stream_t stream) {
  GH_REQUIRE(b > 0 && n_max > 0 && xa > 0 && ds >= 0 && r > 0, "evd_assemble_fwd: bad sizes");
  GH_REQUIRE(ds == 0 || (table && sources), "evd_assemble_fwd: article-source width %d needs a table and source ids", ds);
  GH_REQUIRE(ds == 0 || table_rows > 0, "evd_assemble_fwd: table_rows must give the article-source table's row count");
  hipStream_t s = (hipStream_t)stream;
  unsigned int* cl = clamp_counter();
  GH_REQUIRE(cl, "evd_assemble_fwd: cannot allocate the clamp counter");
  const dim3 grid(b * n_max), blk(256);
#define GH_EA(TS, TD) hipLaunchKernelGGL((evd_assemble_fwd_kernel<TS, TD>), grid, blk, 0, s, avg, offsets, table, (const TS*)sources, \
                                         (const TD*)document, right, mask, n_max, xa, ds, r, table_rows, cl)
  if (sources_i64 && document_i64) GH_EA(int64_t, int64_t);
  else if (sources_i64) GH_EA(int64_t, int32_t);
  else if (document_i64) GH_EA(int32_t, int64_t);
  else GH_EA(int32_t, int32_t);
#undef GH_EA
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_evd_assemble_bwd(const float* g, const int32_t* offsets, const void* sources, int sources_i64, int table_rows, int b, int n_max,
                                   int xa, int ds, float* d_avg, float* d_table, gh_stream_t stream) {
  GH_REQUIRE(b > 0 && n_max > 0 && xa > 0 && ds >= 0, "evd_assemble_bwd: bad sizes");
  GH_REQUIRE(ds == 0 || !d_table || table_rows > 0, "evd_assemble_bwd: table_rows must give the article-source table's row count");
  const int n_slots = b * n_max;
  // every workgroup stages the source id of every slot (4 B) + a match bit per slot in LDS: 160 KB hold 38 000 slots,
  // i.e. 1266 claims x 30 evidence slots per call
  GH_REQUIRE(n_slots <= 38000, "evd_assemble_bwd: %d claim x evidence slots (max 38000 per call: split the batch)", n_slots);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds_bytes = (size_t)((n_slots + 1) & ~1) * 4 + (size_t)((n_slots + 63) / 64) * 8;
  // (38 000 slots need 156 752 B beside the kernel's static `earlier` flag)
  if (int rc = lds_opt_in(sources_i64 ? (const void*)evd_assemble_bwd_kernel<int64_t> : (const void*)evd_assemble_bwd_kernel<int32_t>, lds_bytes,
                          "evd_assemble_bwd"))
    return rc;
  if (sources_i64)
    hipLaunchKernelGGL((evd_assemble_bwd_kernel<int64_t>), dim3(n_slots), dim3(256), lds_bytes, s, g, offsets,
                       (const int64_t*)sources, d_avg, d_table, n_slots, n_max, xa, ds, table_rows);
  else
    hipLaunchKernelGGL((evd_assemble_bwd_kernel<int32_t>), dim3(n_slots), dim3(256), lds_bytes, s, g, offsets,
                       (const int32_t*)sources, d_avg, d_table, n_slots, n_max, xa, ds, table_rows);
  GH_LAUNCH_CHECK();
  return 0;
}
