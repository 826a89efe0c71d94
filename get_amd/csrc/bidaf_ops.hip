// The two pieces of Models/BiDAF/bidaf_model.py that the other drop-ins do not cover:
//   gh_att_flow_*   the attention-flow layer (:72-104): trilinear scores, context-to-query and query-to-context attention and
//                   the four-way concatenation [c, c2q, c * c2q, c * q2c]
//   gh_highway_*    the gate of the highway network (:62): y = sigmoid(g_pre) relu(h_pre) + (1 - sigmoid(g_pre)) x
// There is NO mask, as in the reference: c and q are LSTM outputs with exact-zero rows at t >= len, and those rows take part
// in both softmaxes (a zero row of q scores c_i.w_c + bias, a zero row of c scores q_j.w_q + bias).
//
// The products run on the MFMA from operands staged in LDS: the KC / KM layouts, the staging and the MFMA helpers are those of
// score_tile.hip.h, which mha_ops.hip and match_ops.hip use as well.
// The width d is walked in blocks of AF_BLK = 640 columns (10 accumulators per wave; the project's 600 is one block).
//
//   forward, tiles     one workgroup per (batch element, 16 context rows).  The left operand is c_i * w_cq + w_q, so that one
//                      product gives (c_i * w_cq).q_j + q_j.w_q; c_i.w_c and the biases are added per row.  S [16][lq] sits
//                      in LDS over depth blocks and key chunks; row softmax (running maximum subtracted), row maximum and its
//                      LOWEST index; a is written out; c2q = a q over key chunks; x[:, 0:3d] is written.
//   forward, batch     one workgroup per (batch element, 256 columns): beta = softmax over ALL lc row maxima, q2c = sum_i
//                      beta_i c_i, x[:, 3d:4d] = c * q2c.  No workgroup waits on another: it is a second launch.
//   backward, batch    one workgroup per batch element: dq2c, dbeta, dm and the per-batch-element partial of dw_c.
//   backward, rows     forward tiling: dA = dc2q q^T, dS = a (dA - rowsum(a dA)) + dm [j = argmax] (to the caller's scratch),
//                      dc from dS q and the elementwise terms.
//   backward, keys     one workgroup per (batch element, 16 query rows) walks the context rows: dq = a^T dc2q + colsum(dS)
//                      w_q + w_cq * (dS^T c), and the per-tile partials of dw_q and dw_cq.
//   sums               the partials on the stream workspace, added to dw_c / dw_q / dw_cq in a fixed order.
// Every output element has one owner, there are no atomics: two runs are bit-identical.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include "score_tile.hip.h"
#include <math.h>

namespace gh {
namespace {

constexpr int AF_THREADS = 256;
constexpr int AF_WAVES = AF_THREADS / 64;
static_assert(AF_THREADS == TILE_THREADS, "score_tile.hip.h strides its loops by its own workgroup size");
constexpr int AF_MAX_LC = 1024;          // beta of one batch element in LDS; dA / dS tile [16][lq]
constexpr int AF_MAX_LQ = 1024;          // one 16-row score tile [16][lq] in LDS (64 KB at the limit)
constexpr int AF_MAX_D = 2048;           // dq2c of one batch element in LDS
constexpr int AF_BLK = 640;              // columns of one depth / column block
constexpr int AF_NT = AF_BLK / 16 / AF_WAVES;      // column tiles per wave: 10 accumulators
constexpr int AF_CHUNK = 16 * 656;       // floats of one staged operand chunk (41 KB): 16 rows at the widest pitch (656)

// LDS of the two row-tiled kernels: left [16][pa] | ss [16][ps] | chunk | 16 row scalars
__host__ __device__ inline TilePlan af_plan(int lq, int d) { return tile_plan<AF_BLK, AF_CHUNK>(lq, d); }
__host__ __device__ inline int tile_lds_floats(const TilePlan& p) { return 16 * p.pa + 16 * p.ps + p.chunk + 16; }

// LDS of the key-tiled kernel: cc [rc][pm] | gc [rc][pm] | dst [rc][16] | wt [rc][16] | 16 column sums
struct KeyPlan { int pm, rc; };
__host__ __device__ inline KeyPlan key_plan(int lc, int d) {
  KeyPlan p;
  p.pm = pitch_km(imin(up16(d), AF_BLK));
  p.rc = chunk_rows(lc, 2 * p.pm, AF_CHUNK);
  return p;
}
__host__ __device__ inline int key_lds_floats(const KeyPlan& p) { return p.rc * (2 * p.pm + 32) + 16; }

// g1 + g2 * c (the gradient that reaches c2q), columns k0 .. k0 + cols of rows row0 .. of one batch element
__device__ __forceinline__ void stage_dc2q(float* dst, int pitch, int rows_pad, int cols_pad, const float* __restrict__ g, long long ldg,
                                           const float* __restrict__ c, long long ldc, int d, int k0, int rows, int cols) {
  const float* g1 = g + d + k0;
  const float* g2 = g + 2 * (size_t)d + k0;
  const float* cb = c + k0;
  const bool v1 = vec_ok(g1, ldg), v2 = vec_ok(g2, ldg), vc = vec_ok(cb, ldc);
  stage_f(dst, pitch, rows_pad, cols_pad, rows, cols, [=](int r, int cc) {
    const float4 a = ld4(g1 + (size_t)r * ldg + cc, v1, cols - cc), b = ld4(g2 + (size_t)r * ldg + cc, v2, cols - cc);
    const float4 x = ld4(cb + (size_t)r * ldc + cc, vc, cols - cc);
    return make_float4(fmaf(b.x, x.x, a.x), fmaf(b.y, x.y, a.y), fmaf(b.z, x.z, a.z), fmaf(b.w, x.w, a.w));
  });
}

// ============================================================================ forward, row tiles
// grid b * ceil(lc / 16).  LDS: as [16][pa] | ss [16][ps] | chunk | rs [16]
__global__ __launch_bounds__(AF_THREADS) void
af_fwd_tile_kernel(const float* __restrict__ c, const float* __restrict__ q, long long ldc, long long ldq, const float* __restrict__ w_c,
                   const float* __restrict__ w_q, const float* __restrict__ w_cq, const float* __restrict__ b_c,
                   const float* __restrict__ b_q, const float* __restrict__ b_cq, int lc, int lq, int d, float* __restrict__ x,
                   long long ldx, float* __restrict__ a, int32_t* __restrict__ amax, float* __restrict__ m) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = af_plan(lq, d);
  float* as = sm;
  float* ss = as + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  float* rs = ch + P.chunk;
  const int nrt = (lc + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, lc - i0);
  const float* cb = c + ((size_t)bi * lc + i0) * ldc;
  const float* qb = q + (size_t)bi * lq * ldq;
  const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;

  {      // c_i . w_c + the three biases: 16 lanes per row
    float s = 0.f;
    if (row < ni)
      for (int k = sub; k < d; k += 16) s = fmaf(cb[(size_t)row * ldc + k], w_c[k], s);
    s = sub16_sum(s);
    if (sub == 0) rs[row] = s + (b_c[0] + b_q[0] + b_cq[0]);
  }
  for (int k0 = 0; k0 < d; k0 += AF_BLK) {      // S = (c * w_cq + w_q) q^T over depth blocks
    const int nb = min(AF_BLK, d - k0), nb4 = up4(nb);
    const float* cs = cb + k0;
    const bool vc = vec_ok(cs, ldc);
    __syncthreads();
    stage_f(as, P.pa, 16, nb4, ni, nb, [=](int r, int cc) {
      const float4 v = ld4(cs + (size_t)r * ldc + cc, vc, nb - cc);
      const float* wa = w_cq + k0 + cc;
      const float* wb = w_q + k0 + cc;
      const int n = nb - cc;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      o.x = fmaf(v.x, wa[0], wb[0]);
      if (n > 1) o.y = fmaf(v.y, wa[1], wb[1]);
      if (n > 2) o.z = fmaf(v.z, wa[2], wb[2]);
      if (n > 3) o.w = fmaf(v.w, wa[3], wb[3]);
      return o;
    });
    for (int key0 = 0; key0 < lq; key0 += P.kc1) {
      const int nk = min(P.kc1, lq - key0), rp = up16(nk);
      __syncthreads();
      stage(ch, P.pk, rp, nb4, qb + (size_t)key0 * ldq + k0, ldq, nk, nb);
      __syncthreads();
      mma_scores(as, P.pa, ch, P.pk, rp, nb4, ss, P.ps, key0, k0 > 0);
    }
  }
  __syncthreads();
  {      // softmax, row maximum and its lowest index: 16 lanes per row
    const bool live = row < ni;
    float* srow = ss + row * P.ps;
    const float add = rs[row];
    float mx = -INFINITY;
    int am = 0x7fffffff;
    if (live)
      for (int j = sub; j < lq; j += 16) {
        const float v = srow[j] + add;
        srow[j] = v;
        if (v > mx) {      // strict: the first index of a lane's columns wins
          mx = v;
          am = j;
        }
      }
    const float mxa = sub16_max(mx);
    int cand = (live && mx == mxa) ? am : 0x7fffffff;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    float sum = 0.f;
    if (live)
      for (int j = sub; j < lq; j += 16) sum += expf(srow[j] - mxa);
    sum = sub16_sum(sum);
    const int lqp = up16(lq);
    for (int j = sub; j < lqp; j += 16) {
      float w = 0.f;
      if (live && j < lq) w = expf(srow[j] - mxa) / sum;
      srow[j] = w;
    }
    if (live && sub == 0) {
      m[(size_t)bi * lc + i0 + row] = mxa;
      amax[(size_t)bi * lc + i0 + row] = cand < lq ? cand : 0;
    }
  }
  __syncthreads();
  unstage(a + ((size_t)bi * lc + i0) * lq, lq, ss, P.ps, ni, lq);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int c0 = 0; c0 < d; c0 += AF_BLK) {      // c2q = a q over column blocks
    const int nb = min(AF_BLK, d - c0), nct = (nb + 15) >> 4;
    f32x4 acc[AF_NT];
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < lq; key0 += P.kc2) {
      const int nk = min(P.kc2, lq - key0), rp = up4(nk);
      __syncthreads();
      stage(ch, P.pv, rp, up16(nb), qb + (size_t)key0 * ldq + c0, ldq, nk, nb);
      __syncthreads();
      mma_acc<AF_NT>(ss + key0, P.ps, 1, ch, P.pv, rp, nct, acc);
    }
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) {
      const int col = (wave + AF_WAVES * t) * 16 + l15;
      if (col < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) {
            const float cv = cb[(size_t)i * ldc + c0 + col];
            float* xr = x + ((size_t)bi * lc + i0 + i) * ldx + c0 + col;
            xr[0] = cv;
            xr[d] = acc[t][r];
            xr[2 * (size_t)d] = cv * acc[t][r];
          }
        }
      }
    }
  }
}

// ============================================================================ forward, per batch element
// grid (b, ceil(d / 256)): every workgroup forms beta of its batch element in the same order; column block 0 writes it
__global__ __launch_bounds__(AF_THREADS) void
af_fwd_batch_kernel(const float* __restrict__ c, long long ldc, const float* __restrict__ m, int lc, int d, float* __restrict__ x,
                    long long ldx, float* __restrict__ beta, float* __restrict__ q2c) {
  __shared__ float bs[AF_MAX_LC];
  __shared__ float red[AF_WAVES];
  const int bi = blockIdx.x, col = blockIdx.y * AF_THREADS + threadIdx.x;
  const float* mb = m + (size_t)bi * lc;
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < lc; i += AF_THREADS) mx = fmaxf(mx, mb[i]);
  mx = block_max(mx, red);
  float s = 0.f;
  for (int i = threadIdx.x; i < lc; i += AF_THREADS) {
    const float e = expf(mb[i] - mx);
    bs[i] = e;
    s += e;
  }
  s = block_sum(s, red);
  for (int i = threadIdx.x; i < lc; i += AF_THREADS) {
    const float w = bs[i] / s;
    bs[i] = w;
    if (blockIdx.y == 0) beta[(size_t)bi * lc + i] = w;
  }
  __syncthreads();
  if (col >= d) return;
  const float* cb = c + (size_t)bi * lc * ldc + col;
  float acc = 0.f;
  for (int i = 0; i < lc; ++i) acc = fmaf(bs[i], cb[(size_t)i * ldc], acc);
  q2c[(size_t)bi * d + col] = acc;
  float* xb = x + (size_t)bi * lc * ldx + 3 * (size_t)d + col;
  for (int i = 0; i < lc; ++i) xb[(size_t)i * ldx] = cb[(size_t)i * ldc] * acc;
}

// ============================================================================ backward, per batch element
// grid b: dq2c = sum_i g3_i * c_i, dbeta_i = dq2c . c_i, dm_i = beta_i (dbeta_i - sum_k beta_k dbeta_k), part_c = sum_i dm_i c_i
__global__ __launch_bounds__(AF_THREADS) void
af_bwd_batch_kernel(const float* __restrict__ c, long long ldc, const float* __restrict__ g, long long ldg, const float* __restrict__ beta,
                    int lc, int d, float* __restrict__ dq2c, float* __restrict__ dm, float* __restrict__ part_c) {
  __shared__ float dqs[AF_MAX_D];
  __shared__ float dbs[AF_MAX_LC];
  __shared__ float red[AF_WAVES];
  const int bi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* cb = c + (size_t)bi * lc * ldc;
  const float* g3 = g + (size_t)bi * lc * ldg + 3 * (size_t)d;
  for (int col = threadIdx.x; col < d; col += AF_THREADS) {
    float s = 0.f;
    for (int i = 0; i < lc; ++i) s = fmaf(g3[(size_t)i * ldg + col], cb[(size_t)i * ldc + col], s);
    dqs[col] = s;
    dq2c[(size_t)bi * d + col] = s;
  }
  __syncthreads();
  for (int i = wave; i < lc; i += AF_WAVES) {      // one wave per row
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(dqs[k], cb[(size_t)i * ldc + k], s);
    s = wave_sum(s);
    if (lane == 0) dbs[i] = s;
  }
  __syncthreads();
  const float* bb = beta + (size_t)bi * lc;
  float t = 0.f;
  for (int i = threadIdx.x; i < lc; i += AF_THREADS) t = fmaf(bb[i], dbs[i], t);
  t = block_sum(t, red);
  for (int i = threadIdx.x; i < lc; i += AF_THREADS) {
    const float v = bb[i] * (dbs[i] - t);
    dbs[i] = v;
    dm[(size_t)bi * lc + i] = v;
  }
  __syncthreads();
  for (int col = threadIdx.x; col < d; col += AF_THREADS) {
    float s = 0.f;
    for (int i = 0; i < lc; ++i) s = fmaf(dbs[i], cb[(size_t)i * ldc + col], s);
    part_c[(size_t)bi * d + col] = s;
  }
}

// ============================================================================ backward, row tiles: dS and dc
// grid b * ceil(lc / 16).  LDS as the forward's: gs [16][pa] | ss [16][ps] | chunk
__global__ __launch_bounds__(AF_THREADS) void
af_bwd_row_kernel(const float* __restrict__ c, const float* __restrict__ q, long long ldc, long long ldq, const float* __restrict__ w_c,
                  const float* __restrict__ w_cq, const float* __restrict__ x, long long ldx, const float* __restrict__ a,
                  const int32_t* __restrict__ amax, const float* __restrict__ beta, const float* __restrict__ q2c,
                  const float* __restrict__ g, long long ldg, const float* __restrict__ dm, const float* __restrict__ dq2c, int lc, int lq,
                  int d, float* __restrict__ ds, float* __restrict__ dc, long long lddc) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = af_plan(lq, d);
  float* gs = sm;
  float* ss = gs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nrt = (lc + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, lc - i0);
  const size_t r0 = (size_t)bi * lc + i0;
  const float* cb = c + r0 * ldc;
  const float* gb = g + r0 * ldg;
  const float* qb = q + (size_t)bi * lq * ldq;

  for (int k0 = 0; k0 < d; k0 += AF_BLK) {      // dA = dc2q q^T
    const int nb = min(AF_BLK, d - k0), nb4 = up4(nb);
    __syncthreads();
    stage_dc2q(gs, P.pa, 16, nb4, gb, ldg, cb, ldc, d, k0, ni, nb);
    for (int key0 = 0; key0 < lq; key0 += P.kc1) {
      const int nk = min(P.kc1, lq - key0), rp = up16(nk);
      __syncthreads();
      stage(ch, P.pk, rp, nb4, qb + (size_t)key0 * ldq + k0, ldq, nk, nb);
      __syncthreads();
      mma_scores(gs, P.pa, ch, P.pk, rp, nb4, ss, P.ps, key0, k0 > 0);
    }
  }
  __syncthreads();
  {      // dS = a (dA - rowsum(a dA)) + dm [j = argmax]
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const bool live = row < ni;
    const float* arow = a + (r0 + (live ? row : 0)) * lq;
    float* srow = ss + row * P.ps;
    float dot = 0.f;
    if (live)
      for (int j = sub; j < lq; j += 16) dot = fmaf(arow[j], srow[j], dot);
    dot = sub16_sum(dot);
    const int am = live ? amax[r0 + row] : -1;
    const float dmi = live ? dm[r0 + row] : 0.f;
    const int lqp = up16(lq);
    for (int j = sub; j < lqp; j += 16) {
      float v = 0.f;
      if (live && j < lq) {
        v = arow[j] * (srow[j] - dot);
        if (j == am) v += dmi;
      }
      srow[j] = v;
    }
  }
  __syncthreads();
  unstage(ds + r0 * lq, lq, ss, P.ps, ni, lq);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int c0 = 0; c0 < d; c0 += AF_BLK) {      // dS q, then dc
    const int nb = min(AF_BLK, d - c0), nct = (nb + 15) >> 4;
    f32x4 acc[AF_NT];
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < lq; key0 += P.kc2) {
      const int nk = min(P.kc2, lq - key0), rp = up4(nk);
      __syncthreads();
      stage(ch, P.pv, rp, up16(nb), qb + (size_t)key0 * ldq + c0, ldq, nk, nb);
      __syncthreads();
      mma_acc<AF_NT>(ss + key0, P.ps, 1, ch, P.pv, rp, nct, acc);
    }
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) {
      const int col = (wave + AF_WAVES * t) * 16 + l15;
      if (col < nb) {
        const int k = c0 + col;
        const float wc = w_c[k], wcq = w_cq[k], qc = q2c[(size_t)bi * d + k], dqc = dq2c[(size_t)bi * d + k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) {
            const float* gr = gb + (size_t)i * ldg + k;
            const float c2q = x[(r0 + i) * ldx + d + k];
            float v = gr[0];
            v = fmaf(gr[2 * (size_t)d], c2q, v);
            v = fmaf(gr[3 * (size_t)d], qc, v);
            v = fmaf(beta[r0 + i], dqc, v);
            v = fmaf(dm[r0 + i], wc, v);
            v = fmaf(wcq, acc[t][r], v);
            dc[(r0 + i) * lddc + k] = v;
          }
        }
      }
    }
  }
}

// ============================================================================ backward, key tiles: dq and the dw_q / dw_cq partials
// grid b * ceil(lq / 16).  LDS: cc [rc][pm] | gc [rc][pm] | dst [rc][16] | wt [rc][16] | sd [16]
// part [b * ceil(lq / 16)][2][d]: sum_j sd_j q_j | sum_j q_j * (dS^T c)_j over the tile's rows
__global__ __launch_bounds__(AF_THREADS) void
af_bwd_key_kernel(const float* __restrict__ c, const float* __restrict__ q, long long ldc, long long ldq, const float* __restrict__ w_q,
                  const float* __restrict__ w_cq, const float* __restrict__ a, const float* __restrict__ ds, const float* __restrict__ g,
                  long long ldg, int lc, int lq, int d, float* __restrict__ dq, long long lddq, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const KeyPlan P = key_plan(lc, d);
  float* cc = sm;
  float* gc = cc + P.rc * P.pm;
  float* dst = gc + P.rc * P.pm;
  float* wt = dst + P.rc * 16;
  float* sd = wt + P.rc * 16;
  const int nkt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nkt, j0 = (blockIdx.x - bi * nkt) << 4;
  const int nk = min(16, lq - j0);
  const float* cb = c + (size_t)bi * lc * ldc;
  const float* gb = g + (size_t)bi * lc * ldg;
  const float* qb = q + ((size_t)bi * lq + j0) * ldq;
  const size_t sbase = (size_t)bi * lc * lq + j0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;

  if (threadIdx.x < 16) {      // column sums of dS over ALL context rows, in row order
    float s = 0.f;
    if ((int)threadIdx.x < nk)
      for (int i = 0; i < lc; ++i) s += ds[sbase + (size_t)i * lq + threadIdx.x];
    sd[threadIdx.x] = s;
  }
  for (int c0 = 0; c0 < d; c0 += AF_BLK) {
    const int nb = min(AF_BLK, d - c0), nct = (nb + 15) >> 4;
    f32x4 accu[AF_NT], accv[AF_NT];
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) accu[t] = accv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < lc; i0 += P.rc) {
      const int nr = min(P.rc, lc - i0), rp = up4(nr);
      __syncthreads();
      stage(cc, P.pm, rp, up16(nb), cb + (size_t)i0 * ldc + c0, ldc, nr, nb);
      stage_dc2q(gc, P.pm, rp, up16(nb), gb + (size_t)i0 * ldg, ldg, cb + (size_t)i0 * ldc, ldc, d, c0, nr, nb);
      stage(dst, 16, rp, 16, ds + sbase + (size_t)i0 * lq, lq, nr, nk);
      stage(wt, 16, rp, 16, a + sbase + (size_t)i0 * lq, lq, nr, nk);
      __syncthreads();
      mma_acc<AF_NT>(dst, 1, 16, cc, P.pm, rp, nct, accu);      // u = dS^T c
      mma_acc<AF_NT>(wt, 1, 16, gc, P.pm, rp, nct, accv);       // a^T dc2q
    }
    // (sd was written before the first barrier above and is only read from here on)
#pragma unroll
    for (int t = 0; t < AF_NT; ++t) {
      if (wave + AF_WAVES * t < nct) {      // wave-uniform: the shuffles below see all 64 lanes
        const int col = (wave + AF_WAVES * t) * 16 + l15;
        const bool on = col < nb;
        const int k = c0 + (on ? col : 0);
        const float wq = w_q[k], wcq = w_cq[k];
        float pq = 0.f, pcq = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 4 * qd + r;
          if (on && j < nk) {
            const float qv = qb[(size_t)j * ldq + k];
            const float s = sd[j];
            dq[((size_t)bi * lq + j0 + j) * lddq + k] = fmaf(wcq, accu[t][r], fmaf(s, wq, accv[t][r]));
            pq = fmaf(s, qv, pq);
            pcq = fmaf(qv, accu[t][r], pcq);
          }
        }
        pq += __shfl_xor(pq, 16, 64);
        pq += __shfl_xor(pq, 32, 64);
        pcq += __shfl_xor(pcq, 16, 64);
        pcq += __shfl_xor(pcq, 32, 64);
        if (on && qd == 0) {
          float* pr = part + (size_t)blockIdx.x * 2 * d + k;
          pr[0] = pq;
          pr[d] = pcq;
        }
      }
    }
  }
}

// out0[col] (col < split) / out1[col - split] += the sum of part[row][col] over the rows: wave w adds its quarter of the rows in
// row order, the four wave sums are added in wave order.  grid ceil(ncols / 64)
__global__ __launch_bounds__(AF_THREADS) void
af_sum_rows_kernel(const float* __restrict__ part, int nrows, int ncols, int split, float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ float ws[AF_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
  const int per = (nrows + AF_WAVES - 1) / AF_WAVES;
  const int r1 = min(nrows, (wave + 1) * per);
  float s = 0.f;
  if (col < ncols)
    for (int r = wave * per; r < r1; ++r) s += part[(size_t)r * ncols + col];
  ws[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < ncols) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < AF_WAVES; ++w) tot += ws[w][lane];
    if (col < split) out0[col] += tot;
    else out1[col - split] += tot;
  }
}

// ============================================================================ highway gate
// exp of non-positive arguments only, as rnn_ops.hip forms it: s = sigmoid(v) and om = 1 - s; a saturated gate is exactly 1
// with om exactly 0, or below 1e-43 with om exactly 1
__device__ __forceinline__ void hw_gate(float v, float& s, float& om) {
  const float e = expf(-fabsf(v));
  const float t = 1.f / (1.f + e);
  s = v >= 0.f ? t : e * t;
  om = 1.f - s;
}
__device__ __forceinline__ float hw_fwd1(float x, float h, float gp) {
  float s, om;
  hw_gate(gp, s, om);
  return fmaf(s, fmaxf(h, 0.f), om * x);
}
__device__ __forceinline__ void hw_bwd1(float x, float h, float gp, float g, float& dh, float& dg, float& dx) {
  float s, om;
  hw_gate(gp, s, om);
  dh = h > 0.f ? g * s : 0.f;
  dg = g * (fmaxf(h, 0.f) - x) * (s * om);
  dx = g * om;
}

// n elements; `vec`: every pointer is 16-byte aligned -- the first n / 4 quads move 16 bytes per lane, the tail single floats
__global__ __launch_bounds__(AF_THREADS) void
highway_fwd_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ gp, long long n, int vec,
                   float* __restrict__ y) {
  const long long stride = (long long)gridDim.x * AF_THREADS, t0 = (long long)blockIdx.x * AF_THREADS + threadIdx.x;
  const long long n4 = vec ? n >> 2 : 0;
  for (long long i = t0; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(h)[i];
    const float4 p = reinterpret_cast<const float4*>(gp)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(hw_fwd1(a.x, b.x, p.x), hw_fwd1(a.y, b.y, p.y), hw_fwd1(a.z, b.z, p.z), hw_fwd1(a.w, b.w, p.w));
  }
  for (long long i = 4 * n4 + t0; i < n; i += stride) y[i] = hw_fwd1(x[i], h[i], gp[i]);
}

__global__ __launch_bounds__(AF_THREADS) void
highway_bwd_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ gp, const float* __restrict__ g,
                   long long n, int vec, float* __restrict__ dh, float* __restrict__ dg, float* __restrict__ dx) {
  const long long stride = (long long)gridDim.x * AF_THREADS, t0 = (long long)blockIdx.x * AF_THREADS + threadIdx.x;
  const long long n4 = vec ? n >> 2 : 0;
  for (long long i = t0; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(h)[i];
    const float4 p = reinterpret_cast<const float4*>(gp)[i], u = reinterpret_cast<const float4*>(g)[i];
    float4 o0, o1, o2;
    hw_bwd1(a.x, b.x, p.x, u.x, o0.x, o1.x, o2.x);
    hw_bwd1(a.y, b.y, p.y, u.y, o0.y, o1.y, o2.y);
    hw_bwd1(a.z, b.z, p.z, u.z, o0.z, o1.z, o2.z);
    hw_bwd1(a.w, b.w, p.w, u.w, o0.w, o1.w, o2.w);
    reinterpret_cast<float4*>(dh)[i] = o0;
    reinterpret_cast<float4*>(dg)[i] = o1;
    reinterpret_cast<float4*>(dx)[i] = o2;
  }
  for (long long i = 4 * n4 + t0; i < n; i += stride) hw_bwd1(x[i], h[i], gp[i], g[i], dh[i], dg[i], dx[i]);
}

int af_check(const char* who, int b, int lc, int lq, int d) {
  GH_REQUIRE(b >= 1 && lc >= 1 && lq >= 1 && d >= 1, "%s: empty problem (b=%d lc=%d lq=%d d=%d)", who, b, lc, lq, d);
  GH_REQUIRE(lc <= AF_MAX_LC, "%s: lc=%d exceeds the supported %d", who, lc, AF_MAX_LC);
  GH_REQUIRE(lq <= AF_MAX_LQ, "%s: lq=%d exceeds the supported %d", who, lq, AF_MAX_LQ);
  GH_REQUIRE(d <= AF_MAX_D, "%s: d=%d exceeds the supported %d", who, d, AF_MAX_D);
  GH_REQUIRE((long long)b * (((lc > lq ? lc : lq) + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  return 0;
}

int hw_grid(long long n) {
  const long long want = (n / 4 + AF_THREADS - 1) / AF_THREADS + 1;
  return (int)(want < 8192 ? want : 8192);
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_att_flow_fwd(const float* c, const float* q, int ldc, int ldq, const float* w_c, const float* w_q, const float* w_cq,
                               const float* b_c, const float* b_q, const float* b_cq, int b, int lc, int lq, int d, float* x, int ldx,
                               float* a, int32_t* amax, float* m, float* beta, float* q2c, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = af_check("att_flow_fwd", b, lc, lq, d)) return rc;
  GH_REQUIRE(c && q && w_c && w_q && w_cq && b_c && b_q && b_cq && x && a && amax && m && beta && q2c, "att_flow_fwd: NULL argument");
  GH_REQUIRE(ldc >= d && ldq >= d && (long long)ldx >= 4LL * d, "att_flow_fwd: a leading dimension is smaller than its row");
  const size_t lds = (size_t)tile_lds_floats(af_plan(lq, d)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)af_fwd_tile_kernel, lds, "att_flow_fwd")) return rc;
  hipLaunchKernelGGL(af_fwd_tile_kernel, dim3(b * ((lc + 15) / 16)), dim3(AF_THREADS), lds, st, c, q, (long long)ldc, (long long)ldq, w_c,
                     w_q, w_cq, b_c, b_q, b_cq, lc, lq, d, x, (long long)ldx, a, amax, m);
  hipLaunchKernelGGL(af_fwd_batch_kernel, dim3(b, (d + AF_THREADS - 1) / AF_THREADS), dim3(AF_THREADS), 0, st, c, (long long)ldc, m, lc, d,
                     x, (long long)ldx, beta, q2c);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_att_flow_bwd(const float* c, const float* q, int ldc, int ldq, const float* w_c, const float* w_q, const float* w_cq,
                               const float* x, int ldx, const float* a, const int32_t* amax, const float* beta, const float* q2c,
                               const float* g_x, int ldg, int b, int lc, int lq, int d, float* ds, float* dm, float* dq2c, float* dc,
                               int lddc, float* dq, int lddq, float* dw_c, float* dw_q, float* dw_cq, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = af_check("att_flow_bwd", b, lc, lq, d)) return rc;
  GH_REQUIRE(c && q && w_c && w_q && w_cq && x && a && amax && beta && q2c && g_x && ds && dm && dq2c && dc && dq && dw_c && dw_q && dw_cq,
             "att_flow_bwd: NULL argument");
  GH_REQUIRE(ldc >= d && ldq >= d && lddc >= d && lddq >= d && (long long)ldx >= 4LL * d && (long long)ldg >= 4LL * d,
             "att_flow_bwd: a leading dimension is smaller than its row");
  const int nkt = (lq + 15) / 16;
  const Workspace wsp = workspace_for(st);
  const size_t need = ((size_t)b * d + (size_t)b * nkt * 2 * d) * sizeof(float);
  GH_REQUIRE(wsp.p && need <= wsp.bytes,
             "att_flow_bwd: the dw_c / dw_q / dw_cq partials need %zu bytes of stream workspace (gh_set_stream_workspace / gh_set_workspace)",
             need);
  float* part_c = wsp.p;
  float* part_k = wsp.p + (size_t)b * d;
  const size_t lds_r = (size_t)tile_lds_floats(af_plan(lq, d)) * sizeof(float);
  const size_t lds_k = (size_t)key_lds_floats(key_plan(lc, d)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)af_bwd_row_kernel, lds_r, "att_flow_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)af_bwd_key_kernel, lds_k, "att_flow_bwd")) return rc;
  hipLaunchKernelGGL(af_bwd_batch_kernel, dim3(b), dim3(AF_THREADS), 0, st, c, (long long)ldc, g_x, (long long)ldg, beta, lc, d, dq2c, dm,
                     part_c);
  hipLaunchKernelGGL(af_bwd_row_kernel, dim3(b * ((lc + 15) / 16)), dim3(AF_THREADS), lds_r, st, c, q, (long long)ldc, (long long)ldq, w_c,
                     w_cq, x, (long long)ldx, a, amax, beta, q2c, g_x, (long long)ldg, dm, dq2c, lc, lq, d, ds, dc, (long long)lddc);
  hipLaunchKernelGGL(af_bwd_key_kernel, dim3(b * nkt), dim3(AF_THREADS), lds_k, st, c, q, (long long)ldc, (long long)ldq, w_q, w_cq, a, ds,
                     g_x, (long long)ldg, lc, lq, d, dq, (long long)lddq, part_k);
  hipLaunchKernelGGL(af_sum_rows_kernel, dim3((d + 63) / 64), dim3(AF_THREADS), 0, st, part_c, b, d, d, dw_c, dw_c);
  hipLaunchKernelGGL(af_sum_rows_kernel, dim3((2 * d + 63) / 64), dim3(AF_THREADS), 0, st, part_k, b * nkt, 2 * d, d, dw_q, dw_cq);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_highway_fwd(const float* x, const float* h_pre, const float* g_pre, int rows, int d, float* y, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(rows >= 1 && d >= 1, "highway_fwd: empty problem (rows=%d d=%d)", rows, d);
  GH_REQUIRE(x && h_pre && g_pre && y, "highway_fwd: NULL argument");
  const long long n = (long long)rows * d;
  const int vec = aligned16(x) && aligned16(h_pre) && aligned16(g_pre) && aligned16(y);
  hipLaunchKernelGGL(highway_fwd_kernel, dim3(hw_grid(n)), dim3(AF_THREADS), 0, st, x, h_pre, g_pre, n, vec, y);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_highway_bwd(const float* x, const float* h_pre, const float* g_pre, const float* g, int rows, int d, float* dh_pre,
                              float* dg_pre, float* dx, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(rows >= 1 && d >= 1, "highway_bwd: empty problem (rows=%d d=%d)", rows, d);
  GH_REQUIRE(x && h_pre && g_pre && g && dh_pre && dg_pre && dx, "highway_bwd: NULL argument");
  const long long n = (long long)rows * d;
  const int vec = aligned16(x) && aligned16(h_pre) && aligned16(g_pre) && aligned16(g) && aligned16(dh_pre) && aligned16(dg_pre) && aligned16(dx);
  hipLaunchKernelGGL(highway_bwd_kernel, dim3(hw_grid(n)), dim3(AF_THREADS), 0, st, x, h_pre, g_pre, g, n, vec, dh_pre, dg_pre, dx);
  GH_LAUNCH_CHECK();
  return 0;
}
