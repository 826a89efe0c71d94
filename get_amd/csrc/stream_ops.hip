// Streaming (HBM-bound) and few-output companions of the GEMM layers, called by the fused entry points of cell_ops.hip,
// dense_ops.hip and model_ops.hip: the GGNN gate backward's elementwise head, column sums (bias gradients), the row gather
// with the forward's dropout mask, the linear layers with a handful of outputs and the one-launch head backward.
#include "../../include/get_hip.h"
#include "device_utils.h"

namespace gh {

// ---------------------------------------------------------------------------- GGNN gate backward (elementwise part)
// out = h z + xp (1 - z)  (wrapper.py:206):  dhp = g z (1-h^2) ; dzp = g (h-xp) z (1-z) ; dxp = g (1-z)
__global__ void __launch_bounds__(256)
gate_bwd_pre_kernel(const float4* __restrict__ g, const float4* __restrict__ z, const float4* __restrict__ hh,
                    const float4* __restrict__ xp, float4* __restrict__ dhp, float4* __restrict__ dzp,
                    float4* __restrict__ dxp, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 G = g[i], Z = z[i], Hh = hh[i], X = xp[i];
    float4 a, b, c;
#define GH_ONE(f)                                      \
    a.f = G.f * Z.f * (1.f - Hh.f * Hh.f);             \
    b.f = G.f * (Hh.f - X.f) * Z.f * (1.f - Z.f);      \
    c.f = G.f * (1.f - Z.f);
    GH_ONE(x) GH_ONE(y) GH_ONE(z) GH_ONE(w)
#undef GH_ONE
    dhp[i] = a; dzp[i] = b; dxp[i] = c;
  }
}
__global__ void __launch_bounds__(256)
gate_bwd_pre_scalar_kernel(const float* __restrict__ g, const float* __restrict__ z, const float* __restrict__ hh,
                           const float* __restrict__ xp, float* __restrict__ dhp, float* __restrict__ dzp,
                           float* __restrict__ dxp, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float G = g[i], Z = z[i], Hh = hh[i], X = xp[i];
    dhp[i] = G * Z * (1.f - Hh * Hh);
    dzp[i] = G * (Hh - X) * Z * (1.f - Z);
    dxp[i] = G * (1.f - Z);
  }
}

// bf16 storage pipeline: g fp32, every other stream bf16 (4 elements = 8 bytes per item)
__global__ void __launch_bounds__(256)
gate_bwd_pre_bf16_kernel(const float4* __restrict__ g, const uint2* __restrict__ z, const uint2* __restrict__ hh,
                         const uint2* __restrict__ xp, uint2* __restrict__ dhp, uint2* __restrict__ dzp,
                         uint2* __restrict__ dxp, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 G = g[i], Z = bf4_to_f4(z[i]), Hh = bf4_to_f4(hh[i]), X = bf4_to_f4(xp[i]);
    float4 a, b, c;
#define GH_ONE(f)                                      \
    a.f = G.f * Z.f * (1.f - Hh.f * Hh.f);             \
    b.f = G.f * (Hh.f - X.f) * Z.f * (1.f - Z.f);      \
    c.f = G.f * (1.f - Z.f);
    GH_ONE(x) GH_ONE(y) GH_ONE(z) GH_ONE(w)
#undef GH_ONE
    dhp[i] = f4_to_bf4(a); dzp[i] = f4_to_bf4(b); dxp[i] = f4_to_bf4(c);
  }
}

int launch_gate_bwd_pre(const float* g, const float* z, const float* hh, const float* xp, float* dhp, float* dzp,
                        float* dxp, size_t count, hipStream_t s, int bf16) {
  if (count == 0) return 0;
  if (bf16) {
    GH_REQUIRE(count % 4 == 0, "gate_bwd_pre: the bf16 variant needs a multiple of 4 elements");
    const size_t n4 = count / 4;
    const int grid = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    prof_begin(s, PROF_GATE_BWD_PRE);
    hipLaunchKernelGGL(gate_bwd_pre_bf16_kernel, dim3(grid), dim3(256), 0, s, (const float4*)g, (const uint2*)z, (const uint2*)hh,
                       (const uint2*)xp, (uint2*)dhp, (uint2*)dzp, (uint2*)dxp, n4);
    prof_end(PROF_GATE_BWD_PRE, (4.0 + 6.0 * 2.0) * (double)count, s);
    GH_LAUNCH_CHECK();
    return 0;
  }
  const uintptr_t al = (uintptr_t)g | (uintptr_t)z | (uintptr_t)hh | (uintptr_t)xp | (uintptr_t)dhp | (uintptr_t)dzp | (uintptr_t)dxp;
  if (count % 4 == 0 && (al & 15) == 0) {
    const size_t n4 = count / 4;
    const int grid = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    const int ptag = count < ((size_t)1 << 21) ? PROF_FEW_ROWS : PROF_GATE_BWD_PRE;      // (claim-side cells: 960 x 300)
    prof_begin(s, ptag);
    hipLaunchKernelGGL(gate_bwd_pre_kernel, dim3(grid), dim3(256), 0, s, (const float4*)g, (const float4*)z,
                       (const float4*)hh, (const float4*)xp, (float4*)dhp, (float4*)dzp, (float4*)dxp, n4);
    prof_end(ptag, 7.0 * 4.0 * (double)count, s);
  } else {
    const int grid = (int)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
    hipLaunchKernelGGL(gate_bwd_pre_scalar_kernel, dim3(grid), dim3(256), 0, s, g, z, hh, xp, dhp, dzp, dxp, count);
  }
  GH_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------- column sums (bias gradients), += via atomics
constexpr int CS_ROWS = 256;
__global__ void __launch_bounds__(256)
colsum_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
              float* __restrict__ oa, float* __restrict__ ob, float* __restrict__ oc, float* __restrict__ oa2,
              float* __restrict__ ob2, float* __restrict__ oc2, int m, int h) {
  const int r0 = blockIdx.x * CS_ROWS, r1 = min(m, r0 + CS_ROWS);
  for (int col = threadIdx.x; col < h; col += 256) {
    float sa = 0.f, sb = 0.f, sc = 0.f;
    for (int r = r0; r < r1; ++r) {
      sa += a[(size_t)r * h + col];
      if (b) sb += b[(size_t)r * h + col];
      if (c) sc += c[(size_t)r * h + col];
    }
    atomicAdd(oa + col, sa);
    if (b) atomicAdd(ob + col, sb);
    if (c) atomicAdd(oc + col, sc);
    if (oa2) atomicAdd(oa2 + col, sa);
    if (b && ob2) atomicAdd(ob2 + col, sb);
    if (c && oc2) atomicAdd(oc2 + col, sc);
  }
}
// workspace variant: float4 columns x RL row lanes per block, partial sums to scratch, one final pass.
constexpr int CS2_ROWS = 128;      // rows per block of activation-sized inputs; few-row inputs (claim cell at h = 768: 960 rows x 192 float4
                                   // columns, ONE row lane per block) take 16 -- eight blocks walked 128 rows each in 125 us
__global__ void colsum_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                      float* __restrict__ ws, int m, int h, int RL, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float4* red = reinterpret_cast<float4*>(dsm);          // [3][RL][h/4]
  const int n4 = h / 4;
  const int c4 = threadIdx.x % n4, rl = threadIdx.x / n4;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(m, r0 + rows_per_block);
  float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = sa, sc = sa;
  if (rl < RL) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += RL) {
      const size_t o = (size_t)r * n4 + c4;
      const float4 va = reinterpret_cast<const float4*>(a)[o];
      sa.x += va.x; sa.y += va.y; sa.z += va.z; sa.w += va.w;
      if (b) { const float4 v = reinterpret_cast<const float4*>(b)[o]; sb.x += v.x; sb.y += v.y; sb.z += v.z; sb.w += v.w; }
      if (c) { const float4 v = reinterpret_cast<const float4*>(c)[o]; sc.x += v.x; sc.y += v.y; sc.z += v.z; sc.w += v.w; }
    }
    red[(0 * RL + rl) * n4 + c4] = sa;
    red[(1 * RL + rl) * n4 + c4] = sb;
    red[(2 * RL + rl) * n4 + c4] = sc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * n4; i += blockDim.x) {
    const int arr = i / n4, cc = i % n4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < RL; ++k) {
      const float4 v = red[(arr * RL + k) * n4 + cc];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    reinterpret_cast<float4*>(ws)[((size_t)blockIdx.x * 3 + arr) * n4 + cc] = t;
  }
}
// 64 columns x 4 partial-row lanes per block; LDS tree over the lanes
__global__ void __launch_bounds__(256)
colsum_final_kernel(const float* __restrict__ ws, int nblk, int h, float* __restrict__ oa, float* __restrict__ ob,
                    float* __restrict__ oc, float* __restrict__ oa2, float* __restrict__ ob2, float* __restrict__ oc2) {
  __shared__ float red[4][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63), kl = threadIdx.x >> 6;
  float acc = 0.f;
  if (i < 3 * h) {
    const int arr = i / h, col = i % h;
#pragma unroll 4
    for (int k = kl; k < nblk; k += 4) acc += ws[((size_t)k * 3 + arr) * h + col];
  }
  red[kl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (kl == 0 && i < 3 * h) {
    const int arr = i / h, col = i % h;
    float* out = arr == 0 ? oa : (arr == 1 ? ob : oc);
    float* out2 = arr == 0 ? oa2 : (arr == 1 ? ob2 : oc2);
    const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (out) out[col] += v;
    if (out2) out2[col] += v;     // the same sum feeds a second bias (b?0 and b?1 share their gradient)
  }
}


int launch_colsum3(const float* a, const float* b, const float* c, float* oa, float* ob, float* oc, int m, int h,
                   hipStream_t s, float* oa2, float* ob2, float* oc2) {
  if (m <= 0) return 0;
  const uintptr_t al = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
  const int rpb = m <= 8192 ? 16 : CS2_ROWS;
  const int nblk = (m + rpb - 1) / rpb;
  const size_t need = (size_t)nblk * 3 * h * sizeof(float);
  const double bytes = 4.0 * (double)m * h * (1 + (b != nullptr) + (c != nullptr));
  const Workspace wsp = workspace_for(s);
  float* const g_cs_ws = wsp.cs;
  if (g_cs_ws && need <= wsp.cs_bytes && h % 4 == 0 && h / 4 <= 256 && (al & 15) == 0) {
    const int n4 = h / 4;
    const int RL = (256 / n4) > 0 ? (256 / n4) : 1;
    const int threads = ((n4 * RL + 63) / 64) * 64;
    prof_begin(s, PROF_COLSUM);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(threads), (size_t)3 * RL * h * sizeof(float), s, a, b, c,
                       g_cs_ws, m, h, RL, rpb);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((3 * h + 63) / 64), dim3(256), 0, s, g_cs_ws, nblk, h, oa, ob, oc, oa2, ob2, oc2);
    prof_end(PROF_COLSUM, bytes, s);
    GH_LAUNCH_CHECK();
    return 0;
  }
  prof_begin(s, PROF_COLSUM);
  hipLaunchKernelGGL(colsum_kernel, dim3((m + CS_ROWS - 1) / CS_ROWS), dim3(256), 0, s, a, b, c, oa, ob, oc, oa2, ob2, oc2, m, h);
  prof_end(PROF_COLSUM, bytes, s);
  GH_LAUNCH_CHECK();
  return 0;
}
int launch_colsum(const float* a, float* oa, int m, int h, hipStream_t s) {
  return launch_colsum3(a, nullptr, nullptr, oa, nullptr, nullptr, m, h, s, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------- row gather (embedding rows for the dW_proj GEMM)
// dst[r][:] = dropout(table[ids ? ids[r] : r][:]) -- the operand of the dW_proj GEMM, with the forward's mask
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids, float* __restrict__ dst, int m,
                   int d, unsigned drop_thresh, float drop_scale, unsigned drop_seed, int table_rows) {
  const int per = (d + 3) / 4;
  if (d % 4 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    // four independent id -> row chains per thread and trip (as gather_rows_bf16_kernel: one chain at a time left the kernel parked
    // on its loads 82 % of the time)
    const size_t total = (size_t)m * per, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t it0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it0 < total; it0 += 4 * stride) {
      int r[4], c[4], src[4];
      float4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t it = it0 + k * stride < total ? it0 + k * stride : it0;
        r[k] = (int)(it / per); c[k] = 4 * (int)(it % per);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) src[k] = ids ? ids[r[k]] : r[k];
      if (table_rows)      // (gh_embed_fwd: ids nobody has checked are clamped into the table)
#pragma unroll
        for (int k = 0; k < 4; ++k) src[k] = min(max(src[k], 0), table_rows - 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(table + (size_t)src[k] * d + c[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (it0 + k * stride >= total) break;
        float4 w = v[k];
        if (drop_thresh) w = drop4(w, drop_seed, (unsigned)r[k] * (unsigned)d + (unsigned)c[k], drop_thresh, drop_scale);
        *reinterpret_cast<float4*>(dst + (size_t)r[k] * d + c[k]) = w;
      }
    }
    return;
  }
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < (size_t)m * per; it += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(it / per), c = 4 * (int)(it % per);
    int src = ids ? ids[r] : r;
    if (table_rows) src = min(max(src, 0), table_rows - 1);
    const float* s = table + (size_t)src * d + c;
    float* o = dst + (size_t)r * d + c;
    // rows that are no multiple of 4 floats wide, or a base that is not 16-byte aligned: single floats only (a float4 access
    // needs both, and this loop is entered exactly when one of them fails)
    for (int k = 0; k < 4 && c + k < d; ++k) {
      float v = s[k];
      if (drop_thresh) v = drop_hash(drop_seed, (unsigned)r * (unsigned)d + (unsigned)(c + k)) >= drop_thresh ? v * drop_scale : 0.f;
      o[k] = v;
    }
  }
}
// bf16 storage pipeline: table rows and dst hold bf16
__global__ void __launch_bounds__(256)
gather_rows_bf16_kernel(const unsigned short* __restrict__ table, const int32_t* __restrict__ ids, unsigned short* __restrict__ dst,
                        int m, int d, unsigned drop_thresh, float drop_scale, unsigned drop_seed) {
  if (d % 8 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {      // 16-byte items (8 values)
    // four items per thread and trip, every load of the trip ahead of the first store: an item is a dependent id -> row chain, and
    // one chain per thread at a time left the kernel latency-bound (configs[4], 96 000 x 768: 117 us for 2 x 147 MB)
    const int per8 = d / 8;
    const size_t total = (size_t)m * per8, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t it0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it0 < total; it0 += 4 * stride) {
      int r[4], c[4];
      uint4 u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t it = it0 + k * stride < total ? it0 + k * stride : it0;      // (clamped duplicates are loaded, never stored)
        r[k] = (int)(it / per8); c[k] = 8 * (int)(it % per8);
      }
      int src[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) src[k] = ids ? ids[r[k]] : r[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = *reinterpret_cast<const uint4*>(table + (size_t)src[k] * d + c[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (it0 + k * stride >= total) break;
        float4 va = bf4_to_f4(make_uint2(u[k].x, u[k].y)), vb = bf4_to_f4(make_uint2(u[k].z, u[k].w));
        if (drop_thresh) {
          const unsigned idx = (unsigned)r[k] * (unsigned)d + (unsigned)c[k];
          va = drop4(va, drop_seed, idx, drop_thresh, drop_scale);
          vb = drop4(vb, drop_seed, idx + 4u, drop_thresh, drop_scale);
        }
        *reinterpret_cast<uint4*>(dst + (size_t)r[k] * d + c[k]) = make_uint4(pack_bf2(va.x, va.y), pack_bf2(va.z, va.w), pack_bf2(vb.x, vb.y), pack_bf2(vb.z, vb.w));
      }
    }
    return;
  }
  const int per = d / 4;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < (size_t)m * per; it += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(it / per), c = 4 * (int)(it % per);
    float4 v = bf4_to_f4(*reinterpret_cast<const uint2*>(table + (size_t)(ids ? ids[r] : r) * d + c));
    if (drop_thresh) v = drop4(v, drop_seed, (unsigned)r * (unsigned)d + (unsigned)c, drop_thresh, drop_scale);
    *reinterpret_cast<uint2*>(dst + (size_t)r * d + c) = f4_to_bf4(v);
  }
}

int launch_gather_rows(const float* table, const int32_t* ids, float* dst, int m, int d, hipStream_t s, float drop_p,
                       unsigned drop_seed, int bf16, int table_rows) {
  if (m <= 0) return 0;
  GH_REQUIRE(drop_p <= 0.f || (long long)m * (long long)d < (1LL << 32), "gather_rows: %d rows x %d columns exceed the dropout mask's 32-bit element index", m, d);
  if (bf16) {
    GH_REQUIRE(d % 4 == 0, "gather_rows: the bf16 variant needs d %% 4 == 0");
    GH_REQUIRE(table_rows == 0, "gather_rows: the bf16 variant does not clamp ids");
    const size_t n = (size_t)m * (d / 4);
    const double th = (double)drop_p * 4294967296.0;
    const unsigned thresh = drop_p > 0.f ? (th >= 4294967295.0 ? 4294967295u : (unsigned)th) : 0u;
    hipLaunchKernelGGL(gather_rows_bf16_kernel, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, s,
                       (const unsigned short*)table, ids, (unsigned short*)dst, m, d, thresh, 1.0f / (1.0f - drop_p), drop_seed);
    GH_LAUNCH_CHECK();
    return 0;
  }
  const size_t n = (size_t)m * ((d + 3) / 4);
  const double th = (double)drop_p * 4294967296.0;
  const unsigned thresh = drop_p > 0.f ? (th >= 4294967295.0 ? 4294967295u : (unsigned)th) : 0u;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, s,
                     table, ids, dst, m, d, thresh, 1.0f / (1.0f - drop_p), drop_seed, table_rows);
  GH_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------- linear layers with a handful of outputs
// y[m][n] = x[m][:] . w[n][:] + b[n]  for n <= 8 (the 2-class head, graph_based_semantic_structure.py:72): one wave per row
__global__ void __launch_bounds__(256)
tiny_linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                       float* __restrict__ y, int m, int k, int n) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;
  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;
  for (int i = lane; i < k; i += 64) {
    const float xv = x[(size_t)row * k + i];
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < n) acc[c] += xv * w[(size_t)c * k + i];
  }
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < n) {
      float v = acc[c];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) y[(size_t)row * n + c] = v + (bias ? bias[c] : 0.f);
    }
}
// dx[m][k] = g[m][:] . w[:][k] ;  dw[n][k] += sum_m g[m][n] x[m][k] ;  db[n] += sum_m g[m][n]   (w given as stored, [n][k])
__global__ void __launch_bounds__(256)
tiny_linear_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ g,
                       float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, int m, int k, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;            // column k index
  if (i < k) {
    float wc[8], dwc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { wc[c] = c < n ? w[(size_t)c * k + i] : 0.f; dwc[c] = 0.f; }
    for (int r0 = 0; r0 < m; r0 += 8) {
      float xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = x[(size_t)min(r0 + u, m - 1) * k + i];       // eight rows in flight
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + u;
        if (r >= m) break;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < n) { const float gv = g[(size_t)r * n + c]; d += gv * wc[c]; dwc[c] += gv * xv[u]; }
        if (dx) dx[(size_t)r * k + i] = d;
      }
    }
    if (dw)
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < n) dw[(size_t)c * k + i] += dwc[c];
  }
  if (db && blockIdx.x == 0 && threadIdx.x < n) {
    float acc = 0.f;
    for (int r = 0; r < m; ++r) acc += g[(size_t)r * n + threadIdx.x];
    db[threadIdx.x] += acc;
  }
}

int launch_tiny_linear_fwd(const float* x, const float* w, const float* bias, float* y, int m, int k, int n, hipStream_t s) {
  hipLaunchKernelGGL(tiny_linear_fwd_kernel, dim3((m + 3) / 4), dim3(256), 0, s, x, w, bias, y, m, k, n);
  GH_LAUNCH_CHECK();
  return 0;
}
int launch_tiny_linear_bwd(const float* x, const float* w, const float* g, float* dx, float* dw, float* db, int m, int k, int n,
                           hipStream_t s) {
  hipLaunchKernelGGL(tiny_linear_bwd_kernel, dim3((k + 63) / 64), dim3(64), 0, s, x, w, g, dx, dw, db, m, k, n);
  GH_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------- head backward in ONE launch (composite path)
// graph_based_semantic_structure.py:69-74: phi = out1(out0([left | att])) with no activation between.  Backward of both layers' inputs:
//   d_y0[b][k]   = sum_c g_phi[b][c] w1[c][k]                       (H values per claim; tiny: every workgroup makes its own copy in LDS)
//   d_in[b][j]   = sum_k d_y0[b][k] w0[k][j]                        (j < E = Xl + X1: the first Xl go to dx0, the rest to dx1)
//   dw1[c][k]   += sum_b g_phi[b][c] y0[b][k],  db1[c] += sum_b g_phi[b][c]
// It replaces tiny_linear_bwd (5 workgroups walking the claims serially), a 48-workgroup split-K GEMM and its finish kernel --
// 33 us of launch latency for 0.07 GFLOP.  One workgroup per 64 columns j: wave kg takes the k range [kg H/4, (kg+1) H/4), a lane one
// column, 32 claims at a time in registers; w0 is read once (coalesced along j), d_y0 comes from LDS as wave-uniform 16-byte reads.
// The weight gradients of out0 (d_y0^T [left | att]) stay with the side stream's TN launch, which reads the d_y0 this kernel writes.
// CPT = 4 (round 6): a lane owns FOUR consecutive columns (16-byte loads of w0: 256 contiguous bytes per k row and workgroup instead of
// 64).  At h = 768 the head's input is 13 K wide: 832 workgroups of 16 columns each fetched w0 (41 MB) in 64-byte pieces with two
// dependent round trips per thread -- 135 us on the critical path of the configs[4] step; 208 workgroups of 64 columns stream it.
// Used when the width gives >= 192 such workgroups; narrower heads (h = 300: 3556 columns) keep one column per lane.
template <int CPT>
__global__ void __launch_bounds__(256)
head_bwd_kernel(const float* __restrict__ g_phi, const float* __restrict__ y0, const float* __restrict__ w1, const float* __restrict__ w0,
                int B, int H, int C, int Xl, int E, float* __restrict__ d_y0, float* __restrict__ dw1, float* __restrict__ db1,
                float* __restrict__ dx0, int dx0_accumulate, float* __restrict__ dx1, int dy_floats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* dy = reinterpret_cast<float*>(dsm);                 // [32][H]; re-used as the partials [16][32][17] after the K loop
  float* w1s = dy + dy_floats;                               // [C][H]
  float* gs = w1s + (size_t)C * H;                           // [B][C]
  float* ys = gs + (size_t)B * C;                            // [nk][B]: y0 columns of this workgroup's share of dw1
  const int tid = threadIdx.x, col = tid & 15, kg = tid >> 4;       // 16 column groups x 16 k ranges per workgroup
  const int j = (blockIdx.x * 16 + col) * CPT;
  const int jc = min(j, E - CPT);
  const int H4 = H / 4;
  const int kq0 = (kg * H4) / 16, kq1 = ((kg + 1) * H4) / 16;     // this thread's range of float4 k-groups
  // everything small is staged once with independent loads (a per-element walk over g_phi / w1 / y0 in global memory put one
  // memory latency into every iteration: 37 us for this kernel)
  const int G = gridDim.x;
  const int nk = dw1 ? max(0, (H - (int)blockIdx.x + G - 1) / G) : 0;      // workgroup w owns the k with k % G == w
  for (int i = tid; i < C * H; i += 256) w1s[i] = w1[i];
  for (int i = tid; i < B * C; i += 256) gs[i] = g_phi[i];
  for (int i = tid; i < nk * B; i += 256) { const int kk = i / B, b = i - kk * B; ys[i] = y0[(size_t)b * H + blockIdx.x + kk * G]; }
  __syncthreads();
  for (int i = tid; i < nk * C; i += 256) {
    const int kk = i / C, c = i - kk * C;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += gs[b * C + c] * ys[kk * B + b];
    dw1[(size_t)c * H + blockIdx.x + kk * G] += acc;
  }
  if (db1 && blockIdx.x == 0 && tid < C) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += gs[b * C + tid];
    db1[tid] += acc;
  }
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int nb = min(32, B - b0);
    __syncthreads();                                         // (the previous chunk's partials are consumed)
    for (int i = tid; i < 32 * H; i += 256) {
      const int b = i / H, k = i - b * H;
      float v = 0.f;
      if (b < nb)
        for (int c = 0; c < C; ++c) v += gs[(b0 + b) * C + c] * w1s[c * H + k];
      dy[i] = v;
      if (blockIdx.x == 0 && b < nb) d_y0[(size_t)(b0 + b) * H + k] = v;
    }
    __syncthreads();
    float acc[32][CPT];
#pragma unroll
    for (int b = 0; b < 32; ++b)
#pragma unroll
      for (int c = 0; c < CPT; ++c) acc[b][c] = 0.f;
    // several k-groups (4 rows of w0 each) requested before any of them is used: one memory round trip per thread for H <= 512
    constexpr int U = CPT == 1 ? 8 : 4;
    for (int kq = kq0; kq < kq1; kq += U) {
      float wv[U][4][CPT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = 4 * min(kq + u, kq1 - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (CPT == 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(w0 + (size_t)(k + i) * E + jc);
            wv[u][i][0] = t4.x; wv[u][i][1] = t4.y; wv[u][i][2] = t4.z; wv[u][i][3] = t4.w;
          } else {
            wv[u][i][0] = w0[(size_t)(k + i) * E + jc];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (kq + u >= kq1) break;
        const int k = 4 * (kq + u);
#pragma unroll
        for (int b = 0; b < 32; ++b) {
          const float4 d4 = *reinterpret_cast<const float4*>(dy + b * H + k);
#pragma unroll
          for (int c = 0; c < CPT; ++c)
            acc[b][c] += d4.x * wv[u][0][c] + d4.y * wv[u][1][c] + d4.z * wv[u][2][c] + d4.w * wv[u][3][c];
        }
      }
    }
    __syncthreads();                                         // every wave is done with dy: it becomes the partial buffer
    float* red = dy;                                         // [16 k ranges][32][16 column groups + 1], one of a lane's CPT columns at a time
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      if (c > 0) __syncthreads();
#pragma unroll
      for (int b = 0; b < 32; ++b) red[(kg * 32 + b) * 17 + col] = acc[b][c];
      __syncthreads();
      for (int i = tid; i < 32 * 16; i += 256) {
        const int b = i >> 4, l = i & 15, jj = (blockIdx.x * 16 + l) * CPT + c;
        if (b >= nb || jj >= E) continue;
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) v += red[(r * 32 + b) * 17 + l];
        if (jj < Xl) {
          if (dx0) { float* o = dx0 + (size_t)(b0 + b) * Xl + jj; *o = dx0_accumulate ? *o + v : v; }
        } else if (dx1) {
          dx1[(size_t)(b0 + b) * (E - Xl) + (jj - Xl)] = v;
        }
      }
    }
  }
}

// LDS bytes of head_bwd_kernel for these sizes (0: does not fit -- the caller keeps the three-launch path)
static bool head_bwd_wide(int E, const float* w0) {      // four columns per lane: 16-byte rows and enough workgroups to fill the chip
  return E % 4 == 0 && (E + 63) / 64 >= 192 && (reinterpret_cast<uintptr_t>(w0) & 15) == 0;
}
size_t head_bwd_lds(int B, int H, int C, int E, const float* w0) {
  const int G = head_bwd_wide(E, w0) ? (E + 63) / 64 : (E + 15) / 16;
  const size_t dyf = (size_t)32 * H > (size_t)16 * 32 * 17 ? (size_t)32 * H : (size_t)16 * 32 * 17;
  const size_t fl = dyf + (size_t)C * H + (size_t)B * C + (size_t)((H + G - 1) / G) * B;
  return fl * 4 <= 160 * 1024 ? fl * 4 : 0;
}

int launch_head_bwd(const float* g_phi, const float* y0, const float* w1, const float* w0, int B, int H, int C, int Xl, int E,
                    float* d_y0, float* dw1, float* db1, float* dx0, int dx0_accumulate, float* dx1, hipStream_t s) {
  GH_REQUIRE(B > 0 && H > 0 && H % 4 == 0, "head_bwd: hidden width %d must be a multiple of 4", H);
  GH_REQUIRE(C >= 1 && C <= 8 && Xl >= 0 && Xl <= E && d_y0, "head_bwd: bad sizes (C=%d Xl=%d E=%d)", C, Xl, E);
  const size_t lds = head_bwd_lds(B, H, C, E, w0);
  GH_REQUIRE(lds > 0, "head_bwd: B=%d, H=%d do not fit the kernel's LDS staging", B, H);
  const bool wide = head_bwd_wide(E, w0);
  if (int rc = lds_opt_in(wide ? (const void*)head_bwd_kernel<4> : (const void*)head_bwd_kernel<1>, lds, "head_bwd")) return rc;
  const int dyf = 32 * H > 16 * 32 * 17 ? 32 * H : 16 * 32 * 17;
  if (wide)
    hipLaunchKernelGGL(head_bwd_kernel<4>, dim3((E + 63) / 64), dim3(256), lds, s, g_phi, y0, w1, w0, B, H, C, Xl, E, d_y0, dw1, db1, dx0,
                       dx0_accumulate, dx1, dyf);
  else
    hipLaunchKernelGGL(head_bwd_kernel<1>, dim3((E + 15) / 16), dim3(256), lds, s, g_phi, y0, w1, w0, B, H, C, Xl, E, d_y0, dw1, db1, dx0,
                       dx0_accumulate, dx1, dyf);
  GH_LAUNCH_CHECK();
  return 0;
}

}  // namespace gh
