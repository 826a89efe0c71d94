// The multi-head query/key/value attention of thirdparty/two_branches_attention.py (ScaledDotProductAttention :391-422 as
// MultiHeadAttentionOriginal :271-347 calls it) and the residual LayerNorm behind it (:345):
//   gh_mha_sdpa_*        weights = masked softmax(q_h k_h^T) (no temperature, :414-421), out_h = weights v_h, per head
//   gh_add_layernorm_*   y = LayerNorm(x + res) * gamma + beta over the last axis
// The heads are column slices of the projection GEMMs' outputs, read where they lie ([b][l][heads * d] with a leading
// dimension), and `out` is written in the layout `fc` consumes: none of the reference's permute copies exists here.
//
// All five products run on the MFMA from operands staged in LDS, in the KC / KM layouts of score_tile.hip.h: Q, K, gO and V
// are KC as "x^T" operands of the score products and KM as right operands of the second products; the 16-row score tile is the KC
// left operand of weights v / dS k, and 16-key slabs of weights / dS are the transposed left operands of the key-tiled kernel.
//
//   forward            one workgroup per (batch, head, 16-query tile): S = Q K^T into an LDS tile [16][lk] over key chunks,
//                      row softmax (running maximum subtracted, masked entries exactly 0, a fully masked row all 0), the
//                      weights written out, out = weights V over key chunks with the accumulators in registers.
//   backward, queries  same tiling: dA = g_w + gO V^T, dS = A (dA - rowsum(A dA)) (written to the caller's scratch), dq = dS K.
//   backward, keys     one workgroup per (batch, head, 16-key slab) walks the query chunks: dk = dS^T Q, dv = A^T gO.
// Every output element has one owner, nothing is accumulated in memory, no atomics: two runs are bit-identical.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include "score_tile.hip.h"
#include <math.h>

namespace gh {
namespace {

constexpr int MHA_THREADS = 256;
constexpr int MHA_WAVES = MHA_THREADS / 64;
static_assert(MHA_THREADS == TILE_THREADS, "score_tile.hip.h strides its loops by its own workgroup size");
constexpr int MHA_MAX_LQ = 1024;
constexpr int MHA_MAX_LK = 1024;         // one 16-row score tile [16][lk] in LDS (64 KB at the limit)
constexpr int MHA_MAX_D = 512;           // 32 column tiles of 16: 8 accumulators per wave
constexpr int MHA_MAX_HEADS = 16;
constexpr int MHA_NT = MHA_MAX_D / 16 / MHA_WAVES;      // column tiles per wave
constexpr int MHA_CHUNK = 9216;          // floats of one staged operand chunk (36 KB): >= 16 rows at the widest pitch (528)
constexpr int LN_MAX_D = 2048;           // per-wave dgamma / dbeta partials in LDS: 4 x 2 x d floats
constexpr int LN_MAX_WG = 256;

struct FwdPlan { int pq, ps, pk, pv, kc1, kc2, chunk; };      // pitches, key-chunk rows of the two products, chunk floats
__host__ __device__ inline FwdPlan fwd_plan(int lk, int da, int db) {
  // da: depth of the score product (KC operands), db: width of the second product (KM operand)
  FwdPlan p;
  p.pq = pitch_kc(da);
  p.ps = pitch_kc(up16(lk));
  p.pk = pitch_kc(da);
  p.pv = pitch_km(db);
  p.kc1 = chunk_rows(lk, p.pk, MHA_CHUNK);
  p.kc2 = chunk_rows(lk, p.pv, MHA_CHUNK);
  const int c1 = p.kc1 * p.pk, c2 = p.kc2 * p.pv;
  p.chunk = c1 > c2 ? c1 : c2;
  return p;
}
__host__ __device__ inline int fwd_lds_floats(const FwdPlan& p) { return 16 * p.pq + 16 * p.ps + p.chunk; }

struct KeyPlan { int pqm, pgm, qc; };
__host__ __device__ inline KeyPlan key_plan(int lq, int dk, int dv) {
  KeyPlan p;
  p.pqm = pitch_km(dk);
  p.pgm = pitch_km(dv);
  p.qc = chunk_rows(lq, p.pqm + p.pgm, MHA_CHUNK);
  return p;
}
__host__ __device__ inline int key_lds_floats(const KeyPlan& p) { return p.qc * (p.pqm + p.pgm + 32); }

// This file's own forms of score_tile.hip.h's `stage` and `mma_scores`, kept because the shared forms change these kernels'
// device code and that change was not measured: the tail tests here compare c + i with cols where ld4 compares
// cols - c with i, and the score store below indexes ss where the shared one, which also reloads, walks a hoisted pointer.
// rows x cols of a row-major source -> LDS [rows_pad][pitch], zero-filled beyond (rows, cols); cols_pad % 4 == 0
__device__ __forceinline__ void mha_stage(float* dst, int pitch, int rows_pad, int cols_pad, const float* __restrict__ src, long long ld,
                                          int rows, int cols) {
  const bool vec = vec_ok(src, ld);
  const int c4n = cols_pad >> 2;
  for (int idx = threadIdx.x; idx < rows_pad * c4n; idx += MHA_THREADS) {
    const int r = idx / c4n, c = (idx - r * c4n) << 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows && c < cols) {
      const float* p = src + (size_t)r * ld + c;
      if (vec && c + 4 <= cols) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v.x = p[0];
        if (c + 1 < cols) v.y = p[1];
        if (c + 2 < cols) v.z = p[2];
        if (c + 3 < cols) v.w = p[3];
      }
    }
    *reinterpret_cast<float4*>(dst + r * pitch + c) = v;
  }
}

// S[16][key0 + ...] = X Y^T for a chunk: X = xs [16][px] (KC), Y = ys [rows_pad][py] (KC), depth % 4 == 0; the whole depth in one call
__device__ __forceinline__ void mha_scores(const float* xs, int px, const float* ys, int py, int rows_pad, int depth, float* ss, int ps,
                                           int key0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int jt = wave; jt < (rows_pad >> 4); jt += MHA_WAVES) {
    const float* xa = xs + l15 * px + qd;
    const float* yb = ys + (jt * 16 + l15) * py + qd;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 8 <= depth; k0 += 8) {      // two accumulators: the dependent-accumulator latency exceeds the issue interval
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0], yb[k0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0 + 4], yb[k0 + 4], acc1, 0, 0, 0);
    }
    if (k0 < depth) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0], yb[k0], acc0, 0, 0, 0);
    acc0 += acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) ss[(4 * qd + r) * ps + key0 + jt * 16 + l15] = acc0[r];
  }
}

// rows row0 + 4 qd + r < row_end, columns ct * 16 + l15 < cols of a [..][ld] global tensor
__device__ __forceinline__ void store_acc(float* __restrict__ dst, long long ld, int rows, int cols, const f32x4* acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
#pragma unroll
  for (int t = 0; t < MHA_NT; ++t) {
    const int c = (wave + MHA_WAVES * t) * 16 + l15;
    if (c < cols) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * qd + r < rows) dst[(size_t)(4 * qd + r) * ld + c] = acc[t][r];
    }
  }
}

// ============================================================================ forward
// grid (b * ceil(lq / 16), heads).  LDS: qs [16][pq] | ss [16][ps] | chunk
__global__ __launch_bounds__(MHA_THREADS) void
mha_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
               long long ldv, const uint8_t* __restrict__ mask, int b, int lq, int lk, int dk, int dv, float* __restrict__ weights,
               float* __restrict__ out, long long ldo) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const FwdPlan P = fwd_plan(lk, dk, dv);
  float* qs = sm;
  float* ss = qs + 16 * P.pq;
  float* ch = ss + 16 * P.ps;
  const int nqt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nqt, q0 = (blockIdx.x - bi * nqt) << 4, h = blockIdx.y;
  const int nq = min(16, lq - q0);
  const int dk4 = up4(dk);

  mha_stage(qs, P.pq, 16, dk4, q + ((size_t)bi * lq + q0) * ldq + (size_t)h * dk, ldq, nq, dk);
  for (int key0 = 0; key0 < lk; key0 += P.kc1) {
    const int nk = min(P.kc1, lk - key0), rp = up16(nk);
    __syncthreads();
    mha_stage(ch, P.pk, rp, dk4, k + ((size_t)bi * lk + key0) * ldk + (size_t)h * dk, ldk, nk, dk);
    __syncthreads();
    mha_scores(qs, P.pq, ch, P.pk, rp, dk4, ss, P.ps, key0);
  }
  __syncthreads();
  {      // softmax: 16 lanes per row
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const bool live = row < nq;
    const uint8_t* mrow = mask + ((size_t)bi * lq + q0 + (live ? row : 0)) * lk;
    float* srow = ss + row * P.ps;
    float mx = -INFINITY;
    if (live)
      for (int c = sub; c < lk; c += 16)
        if (!mrow[c]) mx = fmaxf(mx, srow[c]);
    mx = sub16_max(mx);
    float sum = 0.f;
    if (live && mx > -INFINITY)
      for (int c = sub; c < lk; c += 16)
        if (!mrow[c]) sum += expf(srow[c] - mx);
    sum = sub16_sum(sum);
    const int lkp = up16(lk);
    for (int c = sub; c < lkp; c += 16) {
      float w = 0.f;
      if (live && c < lk && sum > 0.f && !mrow[c]) w = expf(srow[c] - mx) / sum;
      srow[c] = w;
    }
  }
  __syncthreads();
  unstage(weights + (((size_t)h * b + bi) * lq + q0) * lk, lk, ss, P.ps, nq, lk);

  f32x4 acc[MHA_NT];
#pragma unroll
  for (int t = 0; t < MHA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nct = (dv + 15) >> 4;
  for (int key0 = 0; key0 < lk; key0 += P.kc2) {
    const int nk = min(P.kc2, lk - key0), rp = up4(nk);
    __syncthreads();
    mha_stage(ch, P.pv, rp, up16(dv), v + ((size_t)bi * lk + key0) * ldv + (size_t)h * dv, ldv, nk, dv);
    __syncthreads();
    mma_acc<MHA_NT>(ss + key0, P.ps, 1, ch, P.pv, rp, nct, acc);
  }
  store_acc(out + ((size_t)bi * lq + q0) * ldo + (size_t)h * dv, ldo, nq, dv, acc);
}

// ============================================================================ backward, query-tiled: dS and dq
// grid (b * ceil(lq / 16), heads).  LDS: gs [16][pq] | ss [16][ps] | chunk   (fwd_plan(lk, dv, dk))
__global__ __launch_bounds__(MHA_THREADS) void
mha_bwd_q_kernel(const float* __restrict__ k, const float* __restrict__ v, long long ldk, long long ldv,
                 const float* __restrict__ weights, const float* __restrict__ g_out, long long ldgo, const float* __restrict__ g_w,
                 int b, int lq, int lk, int dk, int dv, float* __restrict__ ds, float* __restrict__ dq, long long lddq) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const FwdPlan P = fwd_plan(lk, dv, dk);
  float* gs = sm;
  float* ss = gs + 16 * P.pq;
  float* ch = ss + 16 * P.ps;
  const int nqt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nqt, q0 = (blockIdx.x - bi * nqt) << 4, h = blockIdx.y;
  const int nq = min(16, lq - q0);
  const int dv4 = up4(dv);
  const size_t wbase = (((size_t)h * b + bi) * lq + q0) * lk;

  mha_stage(gs, P.pq, 16, dv4, g_out + ((size_t)bi * lq + q0) * ldgo + (size_t)h * dv, ldgo, nq, dv);
  for (int key0 = 0; key0 < lk; key0 += P.kc1) {      // dA = gO V^T
    const int nk = min(P.kc1, lk - key0), rp = up16(nk);
    __syncthreads();
    mha_stage(ch, P.pk, rp, dv4, v + ((size_t)bi * lk + key0) * ldv + (size_t)h * dv, ldv, nk, dv);
    __syncthreads();
    mha_scores(gs, P.pq, ch, P.pk, rp, dv4, ss, P.ps, key0);
  }
  __syncthreads();
  {      // dS = A (dA - rowsum(A dA)), dA = g_w + gO V^T; exact zeros where the weight is 0
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const bool live = row < nq;
    const float* arow = weights + wbase + (size_t)(live ? row : 0) * lk;
    const float* grow = g_w ? g_w + wbase + (size_t)(live ? row : 0) * lk : nullptr;
    float* srow = ss + row * P.ps;
    float dot = 0.f;
    if (live)
      for (int c = sub; c < lk; c += 16) {
        const float a = arow[c];
        const float da = srow[c] + (grow ? grow[c] : 0.f);
        srow[c] = da;
        if (a != 0.f) dot = fmaf(a, da, dot);
      }
    dot = sub16_sum(dot);
    const int lkp = up16(lk);
    for (int c = sub; c < lkp; c += 16) {
      float d = 0.f;
      if (live && c < lk) {
        const float a = arow[c];
        if (a != 0.f) d = a * (srow[c] - dot);
      }
      srow[c] = d;
    }
  }
  __syncthreads();
  unstage(ds + wbase, lk, ss, P.ps, nq, lk);

  f32x4 acc[MHA_NT];
#pragma unroll
  for (int t = 0; t < MHA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nct = (dk + 15) >> 4;
  for (int key0 = 0; key0 < lk; key0 += P.kc2) {      // dq = dS K
    const int nk = min(P.kc2, lk - key0), rp = up4(nk);
    __syncthreads();
    mha_stage(ch, P.pv, rp, up16(dk), k + ((size_t)bi * lk + key0) * ldk + (size_t)h * dk, ldk, nk, dk);
    __syncthreads();
    mma_acc<MHA_NT>(ss + key0, P.ps, 1, ch, P.pv, rp, nct, acc);
  }
  store_acc(dq + ((size_t)bi * lq + q0) * lddq + (size_t)h * dk, lddq, nq, dk, acc);
}

// ============================================================================ backward, key-tiled: dk and dv
// grid (b * ceil(lk / 16), heads).  LDS: qc [qc][pqm] | gc [qc][pgm] | dst [qc][16] | wt [qc][16]
__global__ __launch_bounds__(MHA_THREADS) void
mha_bwd_k_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ weights, const float* __restrict__ ds,
                 const float* __restrict__ g_out, long long ldgo, int b, int lq, int lk, int dk, int dv, float* __restrict__ dkk,
                 long long lddk, float* __restrict__ dvv, long long lddv) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const KeyPlan P = key_plan(lq, dk, dv);
  float* qc = sm;
  float* gc = qc + P.qc * P.pqm;
  float* dst = gc + P.qc * P.pgm;
  float* wt = dst + P.qc * 16;
  const int nkt = (lk + 15) >> 4;
  const int bi = blockIdx.x / nkt, key0 = (blockIdx.x - bi * nkt) << 4, h = blockIdx.y;
  const int nk = min(16, lk - key0);
  const size_t wbase = ((size_t)h * b + bi) * lq * lk + key0;

  f32x4 acck[MHA_NT], accv[MHA_NT];
#pragma unroll
  for (int t = 0; t < MHA_NT; ++t) acck[t] = accv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nctk = (dk + 15) >> 4, nctv = (dv + 15) >> 4;
  for (int r0 = 0; r0 < lq; r0 += P.qc) {
    const int nr = min(P.qc, lq - r0), rp = up4(nr);
    __syncthreads();
    mha_stage(qc, P.pqm, rp, up16(dk), q + ((size_t)bi * lq + r0) * ldq + (size_t)h * dk, ldq, nr, dk);
    mha_stage(gc, P.pgm, rp, up16(dv), g_out + ((size_t)bi * lq + r0) * ldgo + (size_t)h * dv, ldgo, nr, dv);
    mha_stage(dst, 16, rp, 16, ds + wbase + (size_t)r0 * lk, lk, nr, nk);
    mha_stage(wt, 16, rp, 16, weights + wbase + (size_t)r0 * lk, lk, nr, nk);
    __syncthreads();
    mma_acc<MHA_NT>(dst, 1, 16, qc, P.pqm, rp, nctk, acck);      // dk = dS^T Q
    mma_acc<MHA_NT>(wt, 1, 16, gc, P.pgm, rp, nctv, accv);       // dv = A^T gO
  }
  store_acc(dkk + ((size_t)bi * lk + key0) * lddk + (size_t)h * dk, lddk, nk, dk, acck);
  store_acc(dvv + ((size_t)bi * lk + key0) * lddv + (size_t)h * dv, lddv, nk, dv, accv);
}

// ============================================================================ add + LayerNorm
// one wave per row; grid-stride over the rows
__global__ __launch_bounds__(MHA_THREADS) void
add_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                  const float* __restrict__ beta, float eps, int rows, int d, float* __restrict__ y, float* __restrict__ mean,
                  float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * MHA_WAVES + wave; r < rows; r += (long long)gridDim.x * MHA_WAVES) {
    const float* xr = x + r * d;
    const float* rr = res ? res + r * d : nullptr;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += xr[c] + (rr ? rr[c] : 0.f);
    const float mu = wave_sum(s) / (float)d;
    float s2 = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float z = xr[c] + (rr ? rr[c] : 0.f) - mu;
      s2 = fmaf(z, z, s2);
    }
    const float rs = 1.f / sqrtf(wave_sum(s2) / (float)d + eps);
    for (int c = lane; c < d; c += 64) {
      const float z = xr[c] + (rr ? rr[c] : 0.f) - mu;
      y[r * d + c] = fmaf(z * rs, gamma[c], beta[c]);
    }
    if (lane == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
  }
}

// dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = g gamma; per-workgroup dgamma / dbeta partials -> part[wg][2][d]
// LDS: pg[MHA_WAVES][d] | pb[MHA_WAVES][d]
__global__ __launch_bounds__(MHA_THREADS) void
add_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                  const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ g, int rows, int d,
                  float* __restrict__ dx, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* pg = sm + wave * d;
  float* pb = sm + (MHA_WAVES + wave) * d;
  for (int c = lane; c < d; c += 64) pg[c] = pb[c] = 0.f;
  for (long long r = (long long)blockIdx.x * MHA_WAVES + wave; r < rows; r += (long long)gridDim.x * MHA_WAVES) {
    const float* xr = x + r * d;
    const float* rr = res ? res + r * d : nullptr;
    const float* gr = g + r * d;
    const float mu = mean[r], rs = rstd[r];
    float c1 = 0.f, c2 = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float xh = (xr[c] + (rr ? rr[c] : 0.f) - mu) * rs;
      const float dxh = gr[c] * gamma[c];
      c1 += dxh;
      c2 = fmaf(dxh, xh, c2);
    }
    c1 = wave_sum(c1) / (float)d;
    c2 = wave_sum(c2) / (float)d;
    for (int c = lane; c < d; c += 64) {
      const float xh = (xr[c] + (rr ? rr[c] : 0.f) - mu) * rs;
      const float gv = gr[c];
      dx[r * d + c] = rs * (gv * gamma[c] - c1 - xh * c2);
      pg[c] = fmaf(gv, xh, pg[c]);
      pb[c] += gv;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < d; c += MHA_THREADS) {
    float sg = 0.f, sb = 0.f;
#pragma unroll
    for (int w = 0; w < MHA_WAVES; ++w) {
      sg += sm[w * d + c];
      sb += sm[(MHA_WAVES + w) * d + c];
    }
    part[((size_t)blockIdx.x * 2) * d + c] = sg;
    part[((size_t)blockIdx.x * 2 + 1) * d + c] = sb;
  }
}

// second stage: the workgroups' partials in workgroup order, added to dgamma | dbeta
__global__ __launch_bounds__(MHA_THREADS) void
add_ln_sum_kernel(const float* __restrict__ part, int nwg, int d, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * MHA_THREADS + threadIdx.x;
  if (c >= 2 * d) return;
  float s = 0.f;
  for (int w = 0; w < nwg; ++w) s += part[(size_t)w * 2 * d + c];
  if (c < d) dgamma[c] += s;
  else dbeta[c - d] += s;
}

int mha_check(const char* who, int b, int heads, int lq, int lk, int dk, int dv) {
  GH_REQUIRE(b >= 1 && heads >= 1 && lq >= 1 && lk >= 1 && dk >= 1 && dv >= 1, "%s: empty problem (b=%d heads=%d lq=%d lk=%d dk=%d dv=%d)",
             who, b, heads, lq, lk, dk, dv);
  GH_REQUIRE(heads <= MHA_MAX_HEADS, "%s: heads=%d exceeds the supported %d", who, heads, MHA_MAX_HEADS);
  GH_REQUIRE(lq <= MHA_MAX_LQ, "%s: lq=%d exceeds the supported %d", who, lq, MHA_MAX_LQ);
  GH_REQUIRE(lk <= MHA_MAX_LK, "%s: lk=%d exceeds the supported %d", who, lk, MHA_MAX_LK);
  GH_REQUIRE(dk <= MHA_MAX_D, "%s: dk=%d exceeds the supported %d", who, dk, MHA_MAX_D);
  GH_REQUIRE(dv <= MHA_MAX_D, "%s: dv=%d exceeds the supported %d", who, dv, MHA_MAX_D);
  GH_REQUIRE((long long)b * (((lq > lk ? lq : lk) + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_mha_sdpa_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const uint8_t* mask, int b,
                               int heads, int lq, int lk, int dk, int dv, float* weights, float* out, int ldo, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mha_check("mha_sdpa_fwd", b, heads, lq, lk, dk, dv)) return rc;
  GH_REQUIRE(q && k && v && mask && weights && out, "mha_sdpa_fwd: NULL argument");
  GH_REQUIRE(ldq >= heads * dk && ldk >= heads * dk && ldv >= heads * dv && ldo >= heads * dv,
             "mha_sdpa_fwd: a leading dimension is smaller than heads * width");
  const size_t lds = (size_t)fwd_lds_floats(fwd_plan(lk, dk, dv)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)mha_fwd_kernel, lds, "mha_sdpa_fwd")) return rc;
  hipLaunchKernelGGL(mha_fwd_kernel, dim3(b * ((lq + 15) / 16), heads), dim3(MHA_THREADS), lds, st, q, k, v, (long long)ldq,
                     (long long)ldk, (long long)ldv, mask, b, lq, lk, dk, dv, weights, out, (long long)ldo);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_mha_sdpa_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* weights,
                               const float* g_out, int ldgo, const float* g_weights, int b, int heads, int lq, int lk, int dk, int dv,
                               float* ds, float* dq, int lddq, float* dkk, int lddk, float* dvv, int lddv, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mha_check("mha_sdpa_bwd", b, heads, lq, lk, dk, dv)) return rc;
  GH_REQUIRE(q && k && v && weights && g_out && ds && dq && dkk && dvv, "mha_sdpa_bwd: NULL argument");
  GH_REQUIRE(ldq >= heads * dk && ldk >= heads * dk && lddq >= heads * dk && lddk >= heads * dk && ldv >= heads * dv &&
                 ldgo >= heads * dv && lddv >= heads * dv,
             "mha_sdpa_bwd: a leading dimension is smaller than heads * width");
  const size_t lds_q = (size_t)fwd_lds_floats(fwd_plan(lk, dv, dk)) * sizeof(float);
  const size_t lds_k = (size_t)key_lds_floats(key_plan(lq, dk, dv)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)mha_bwd_q_kernel, lds_q, "mha_sdpa_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)mha_bwd_k_kernel, lds_k, "mha_sdpa_bwd")) return rc;
  hipLaunchKernelGGL(mha_bwd_q_kernel, dim3(b * ((lq + 15) / 16), heads), dim3(MHA_THREADS), lds_q, st, k, v, (long long)ldk,
                     (long long)ldv, weights, g_out, (long long)ldgo, g_weights, b, lq, lk, dk, dv, ds, dq, (long long)lddq);
  hipLaunchKernelGGL(mha_bwd_k_kernel, dim3(b * ((lk + 15) / 16), heads), dim3(MHA_THREADS), lds_k, st, q, (long long)ldq, weights,
                     ds, g_out, (long long)ldgo, b, lq, lk, dk, dv, dkk, (long long)lddk, dvv, (long long)lddv);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_add_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps, int rows, int d,
                                    float* y, float* mean, float* rstd, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(rows >= 1 && d >= 1, "add_layernorm_fwd: empty problem (rows=%d d=%d)", rows, d);
  GH_REQUIRE(d <= LN_MAX_D, "add_layernorm_fwd: d=%d exceeds the supported %d", d, LN_MAX_D);
  GH_REQUIRE(x && gamma && beta && y && mean && rstd, "add_layernorm_fwd: NULL argument");
  const int nwg = (rows + MHA_WAVES - 1) / MHA_WAVES < 4096 ? (rows + MHA_WAVES - 1) / MHA_WAVES : 4096;
  hipLaunchKernelGGL(add_ln_fwd_kernel, dim3(nwg), dim3(MHA_THREADS), 0, st, x, res, gamma, beta, eps, rows, d, y, mean, rstd);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_add_layernorm_bwd(const float* x, const float* res, const float* gamma, const float* mean, const float* rstd,
                                    const float* g, int rows, int d, float* dx, float* dgamma, float* dbeta, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(rows >= 1 && d >= 1, "add_layernorm_bwd: empty problem (rows=%d d=%d)", rows, d);
  GH_REQUIRE(d <= LN_MAX_D, "add_layernorm_bwd: d=%d exceeds the supported %d", d, LN_MAX_D);
  GH_REQUIRE(x && gamma && mean && rstd && g && dx && dgamma && dbeta, "add_layernorm_bwd: NULL argument");
  const int nwg = (rows + MHA_WAVES - 1) / MHA_WAVES < LN_MAX_WG ? (rows + MHA_WAVES - 1) / MHA_WAVES : LN_MAX_WG;
  const Workspace wsp = workspace_for(st);
  const size_t need = (size_t)nwg * 2 * d * sizeof(float);
  GH_REQUIRE(wsp.p && need <= wsp.bytes,
             "add_layernorm_bwd: the per-workgroup dgamma / dbeta partials need %zu bytes of stream workspace (gh_set_stream_workspace / "
             "gh_set_workspace)", need);
  const size_t lds = (size_t)2 * MHA_WAVES * d * sizeof(float);
  hipLaunchKernelGGL(add_ln_bwd_kernel, dim3(nwg), dim3(MHA_THREADS), lds, st, x, res, gamma, mean, rstd, g, rows, d, dx, wsp.p);
  hipLaunchKernelGGL(add_ln_sum_kernel, dim3((2 * d + MHA_THREADS - 1) / MHA_THREADS), dim3(MHA_THREADS), 0, st, wsp.p, nwg, d, dgamma,
                     dbeta);
  GH_LAUNCH_CHECK();
  return 0;
}
