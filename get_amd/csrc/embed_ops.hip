// The embedding table (torch.nn.Embedding, Models/base_model.py:144-162): the lookup and the gradient of a trainable table.
//   gh_embed_fwd   the row gather of stream_ops.hip (launch_gather_rows) without dropout, ids clamped into the table.
//   gh_embed_bwd   dtable[t] += the rows of dx whose id is t, as a segmented row sum over the ids in ascending (id, row) order.
//
// The order of every addition is fixed by the contract in include/get_hip.h (chunks of GH_EMBED_CHUNK sorted positions) and by
// nothing else: not by the grid, not by the device.  Two kernels:
//   embed_bwd_chunk_kernel   one workgroup per chunk, a thread per column (a float4 of columns where d % 4 == 0), the chunk's
//                            ids and rows in LDS.  It walks the rows in sorted order, EB_ROWS loads in flight, and adds the rows
//                            of a run of equal ids one after the other.  A run that lies inside the chunk is added to its table
//                            row at once -- no other workgroup has a row of that id.  The partial of a run that crosses a chunk
//                            edge goes to the workspace: slot 0 of the chunk when the run holds the chunk's first position, slot 1
//                            otherwise (at most one run can cross each edge).
//   embed_bwd_merge_kernel   one workgroup per chunk again; it works only where a crossing run STARTS in its chunk: the end of the
//                            run comes from a binary search over the sorted ids, the partials are added in chunk order (the loads
//                            batched, the additions sequential) and the sum is added to the table row once.  A token that is in
//                            every row therefore costs one partial per chunk in parallel and one short serial pass.
// One writer per table element, no floating-point atomics: two runs are bit-identical, and tests/embed_ref.py restates the
// result bit for bit.  Rows whose id is outside the table, or is the padding id, are skipped; nothing is written through them.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"

namespace gh {
namespace {

constexpr int EB_CHUNK = GH_EMBED_CHUNK;
constexpr int EB_ROWS = 8;              // rows requested before the first of them is added
constexpr int EB_MAX_THREADS = 256;

__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
template <typename V> __device__ __forceinline__ V vzero();
template <> __device__ __forceinline__ float vzero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ bool id_live(int id, int vocab, int padding_idx) { return id >= 0 && id < vocab && id != padding_idx; }

template <typename V>
__global__ void __launch_bounds__(EB_MAX_THREADS)
embed_bwd_chunk_kernel(const float* __restrict__ dx, long long ldx, const int32_t* __restrict__ sorted_ids,
                       const int32_t* __restrict__ perm, int m, int d, int vocab, int padding_idx, float* __restrict__ dtable,
                       float* __restrict__ ws, unsigned int* __restrict__ clamped) {
  constexpr int W = sizeof(V) / sizeof(float);
  __shared__ int s_id[EB_CHUNK];        // the id of a sorted position, -1 where the row contributes to no table row
  __shared__ int s_row[EB_CHUNK];       // its row of dx, -1 where perm names no row (read as zeros)
  const int s0 = blockIdx.x * EB_CHUNK, cnt = min(EB_CHUNK, m - s0);
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int id = sorted_ids[s0 + i], row = perm[s0 + i];
    const bool outside = id < 0 || id >= vocab;
    if (outside) atomicAdd(clamped + 3, 1u);        // nn.Embedding raises there; counted, gh_clamp_events
    s_id[i] = id_live(id, vocab, padding_idx) ? id : -1;
    s_row[i] = row >= 0 && row < m ? row : -1;
  }
  // the ids beyond both edges of the chunk (-1, which no live id equals, where the sorted index ends)
  const int before = s0 > 0 ? sorted_ids[s0 - 1] : -1;
  const int after = s0 + cnt < m ? sorted_ids[s0 + cnt] : -1;
  __syncthreads();
  for (int col = threadIdx.x * W; col < d; col += blockDim.x * W) {
    int cur = -1, start = 0;
    V acc = vzero<V>();
    // a run [start, end) of id `cur` is over: its sum goes to the table, or to the workspace when the run goes on beyond the chunk
    auto flush = [&](bool at_end) {
      if (cur < 0) return;
      const bool crosses = (start == 0 && before == cur) || (at_end && after == cur);
      if (crosses) {
        *reinterpret_cast<V*>(ws + ((size_t)blockIdx.x * 2 + (start == 0 ? 0 : 1)) * d + col) = acc;
      } else {
        V* p = reinterpret_cast<V*>(dtable + (size_t)cur * d + col);
        *p = vadd(*p, acc);
      }
    };
    for (int i0 = 0; i0 < cnt; i0 += EB_ROWS) {
      V v[EB_ROWS];
#pragma unroll
      for (int u = 0; u < EB_ROWS; ++u) {
        const int row = s_row[min(i0 + u, cnt - 1)];
        v[u] = *reinterpret_cast<const V*>(dx + (size_t)max(row, 0) * (size_t)ldx + col);      // (unconditional load, then the select)
        if (row < 0) v[u] = vzero<V>();
      }
#pragma unroll
      for (int u = 0; u < EB_ROWS; ++u) {
        const int i = i0 + u;
        if (i >= cnt) break;
        const int id = s_id[i];                     // the same for every thread of the workgroup
        if (id != cur) {
          flush(false);
          cur = id; start = i; acc = v[u];          // a run's sum starts from its first row
        } else {
          acc = vadd(acc, v[u]);
        }
      }
    }
    flush(true);
  }
}

template <typename V>
__global__ void __launch_bounds__(EB_MAX_THREADS)
embed_bwd_merge_kernel(const int32_t* __restrict__ sorted_ids, int m, int d, int vocab, int padding_idx, float* __restrict__ dtable,
                       const float* __restrict__ ws) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int c = blockIdx.x, s0 = c * EB_CHUNK, last = min(m, s0 + EB_CHUNK) - 1;
  if (last + 1 >= m) return;
  const int t = sorted_ids[last];
  if (!id_live(t, vocab, padding_idx) || sorted_ids[last + 1] != t) return;      // no run leaves this chunk
  const bool from_first = sorted_ids[s0] == t;
  if (from_first && s0 > 0 && sorted_ids[s0 - 1] == t) return;                   // the run started in an earlier chunk: merged there
  // first position behind the run: the smallest e in (last + 1, m] with sorted_ids[e] != t (e = m where there is none)
  int lo = last + 1, hi = m;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted_ids[mid] == t) lo = mid + 1; else hi = mid;
  }
  const int c_last = (lo - 1) / EB_CHUNK;           // > c: the run holds position last + 1
  for (int col = threadIdx.x * W; col < d; col += blockDim.x * W) {
    V tot = *reinterpret_cast<const V*>(ws + ((size_t)c * 2 + (from_first ? 0 : 1)) * d + col);
    for (int k0 = c + 1; k0 <= c_last; k0 += EB_ROWS) {
      V v[EB_ROWS];
#pragma unroll
      for (int u = 0; u < EB_ROWS; ++u) v[u] = *reinterpret_cast<const V*>(ws + (size_t)min(k0 + u, c_last) * 2 * d + col);
#pragma unroll
      for (int u = 0; u < EB_ROWS; ++u)
        if (k0 + u <= c_last) tot = vadd(tot, v[u]);
    }
    V* p = reinterpret_cast<V*>(dtable + (size_t)t * d + col);
    *p = vadd(*p, tot);
  }
}

template <typename V>
int launch_embed_bwd(const float* dx, long long ldx, const int32_t* sorted_ids, const int32_t* perm, int m, int d, int vocab,
                     int padding_idx, float* dtable, float* ws, unsigned int* clamped, hipStream_t s) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int chunks = (m + EB_CHUNK - 1) / EB_CHUNK;
  const int lanes = (d + W - 1) / W;
  const int threads = lanes >= EB_MAX_THREADS ? EB_MAX_THREADS : (lanes + 63) / 64 * 64;
  hipLaunchKernelGGL(embed_bwd_chunk_kernel<V>, dim3(chunks), dim3(threads), 0, s, dx, ldx, sorted_ids, perm, m, d, vocab, padding_idx,
                     dtable, ws, clamped);
  GH_LAUNCH_CHECK();
  if (chunks > 1) {
    hipLaunchKernelGGL(embed_bwd_merge_kernel<V>, dim3(chunks - 1), dim3(threads), 0, s, sorted_ids, m, d, vocab, padding_idx, dtable, ws);
    GH_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_embed_fwd(const float* table, const int32_t* ids, float* out, int m, int d, int vocab, gh_stream_t stream) {
  GH_REQUIRE(m >= 0 && d >= 1 && vocab >= 1, "embed_fwd: bad sizes (m=%d d=%d vocab=%d)", m, d, vocab);
  if (m == 0) return 0;
  GH_REQUIRE(table && ids && out, "embed_fwd: NULL table, ids or output");
  return launch_gather_rows(table, ids, out, m, d, (hipStream_t)stream, 0.f, 0, 0, vocab);
}

extern "C" int gh_embed_bwd(const float* dx, long long ldx, const int32_t* sorted_ids, const int32_t* perm, int m, int d, int vocab,
                            int padding_idx, float* dtable, float* workspace, long long workspace_floats, gh_stream_t stream) {
  GH_REQUIRE(m >= 0 && d >= 1 && vocab >= 1, "embed_bwd: bad sizes (m=%d d=%d vocab=%d)", m, d, vocab);
  if (m == 0) return 0;
  GH_REQUIRE(dx && sorted_ids && perm && dtable, "embed_bwd: NULL dx, sorted_ids, perm or dtable");
  GH_REQUIRE(ldx >= d, "embed_bwd: the leading dimension of dx (%lld) is below its width %d", ldx, d);
  GH_REQUIRE(padding_idx >= -1 && padding_idx < vocab, "embed_bwd: padding_idx %d is neither -1 nor a row of the %d-row table", padding_idx, vocab);
  const long long need = 2LL * ((m + GH_EMBED_CHUNK - 1) / GH_EMBED_CHUNK) * d;
  GH_REQUIRE(workspace && workspace_floats >= need, "embed_bwd: the workspace holds %lld floats, %lld are needed (2 ceil(m / %d) d)",
             workspace_floats, need, GH_EMBED_CHUNK);
  unsigned int* cl = clamp_counter();
  GH_REQUIRE(cl, "embed_bwd: cannot allocate the clamp counter");
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && aligned16(dx) && aligned16(dtable) && aligned16(workspace);
  if (vec) return launch_embed_bwd<float4>(dx, ldx, sorted_ids, perm, m, d, vocab, padding_idx, dtable, workspace, cl, (hipStream_t)stream);
  return launch_embed_bwd<float>(dx, ldx, sorted_ids, perm, m, d, vocab, padding_idx, dtable, workspace, cl, (hipStream_t)stream);
}
