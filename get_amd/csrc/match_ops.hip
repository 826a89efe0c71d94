// The hot paths of the reference's matchzoo/modules family:
//   gh_soft_align_*    attention.py:50-63 (BidirectionalAttention) and :99-105 (MatchModule): softmax(fill(q k^T)) v between two
//                      sequences.  A filled key is NOT excluded: its score is REPLACED by the constant `fill` (the reference's
//                      masked_fill(mask, -1e-7)) and keeps its weight; its dS is zero because the fill is a constant.
//   gh_lin_att_*       attention.py:35-38 (Attention): softmax over the kept positions of x w
//   gh_match_dot_*     matching.py:46-50: x y^T, optionally of the L2-normalised rows
//   gh_match_bcast_*   matching.py:52-61: x_l (* | + | - | cat) y_r written once, without the reference's two repeat copies
//   gh_gauss_kernel_*  gaussian_kernel.py:34-36
//
// The products run on the MFMA from operands staged in LDS: the KC / KM layouts, the staging and the MFMA helpers are those of
// score_tile.hip.h, which bidaf_ops.hip and mha_ops.hip use as well.
// A width is walked in blocks of MT_BLK = 128 columns (two accumulators per wave; the project's 600 is five blocks): a narrow
// block leaves room for operand chunks of 64 rows, so that all four waves own a score tile per chunk, and for three workgroups
// per CU (53 KB of LDS at the project's shape), which overlap one another's staging and MFMA phases.
//
//   soft_align forward     one workgroup per (batch element, 16 query rows): S [16][lk] in LDS over depth blocks and key
//                          chunks, fill, row softmax (running maximum subtracted), A written out, o = A v over key chunks, the
//                          epilogue writes o (zero where row_zero) or the four-way [q, o, q - o, q * o].
//   soft_align backward    rows: forward tiling -- dA = g_o v^T, dS = A (dA - rowsum(A dA)), zero at filled keys, to the caller's
//                          scratch; dq = dS k plus the direct part.  keys: one workgroup per (batch element, 16 keys) walks the
//                          query rows: dk = dS^T q, dv = A^T g_o.
//   match_dot              forward: the score tile of soft_align, scaled by the two inverse norms.  backward: one kernel, run
//                          once per side, d_rows = (g * ix * iy) other, then the projection of F.normalize on its own rows.
// Every output element has one owner, there are no atomics: two runs are bit-identical.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include "score_tile.hip.h"
#include <math.h>

namespace gh {
namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
static_assert(MT_THREADS == TILE_THREADS, "score_tile.hip.h strides its loops by its own workgroup size");
constexpr int SA_MAX_L = 1024;           // one 16-row score tile [16][lk] in LDS (64 KB at the limit)
constexpr int SA_MAX_D = 2048;
constexpr int LA_MAX_L = 4096;           // the scores of one sequence in LDS
// columns of one depth / column block.  Measured at B = 960, lq / lk = 30 / 100, d = 600, forward + backward, both directions
// of BidirectionalAttention: 640 (one block, 16-row chunks, one workgroup per CU) 4.29 ms, 320 3.25 ms, 128 2.49 ms
constexpr int MT_BLK = 128;
constexpr int MT_NT = MT_BLK / 16 / MT_WAVES;      // column tiles per wave: 2 accumulators
constexpr int MT_CHUNK = 16 * 656;       // floats of one staged operand chunk (41 KB): 64 rows at this block's pitches (132, 144)

// LDS of the row-tiled kernels: left [16][pa] | ss [16][ps] | chunk.  n = the length the scores run over, w = the widest depth
__host__ __device__ inline TilePlan mt_plan(int n, int w) { return tile_plan<MT_BLK, MT_CHUNK>(n, w); }
__host__ __device__ inline int tile_lds_floats(const TilePlan& p) { return 16 * p.pa + 16 * p.ps + p.chunk; }

// LDS of the key-tiled kernel: mm [rc][pm] | st [rc][16]
struct KeyPlan { int pm, rc; };
__host__ __device__ inline KeyPlan key_plan(int n, int w) {
  KeyPlan p;
  p.pm = pitch_km(imin(up16(w), MT_BLK));
  p.rc = chunk_rows(n, p.pm + 16, MT_CHUNK);
  return p;
}
__host__ __device__ inline int key_lds_floats(const KeyPlan& p) { return p.rc * (p.pm + 16); }

// The gradient that reaches o, columns k0 .. k0 + cols of `rows` rows from the row the pointers stand on:
//   fuse == 0   g, zero where rz (NULL ok) marks the row
//   fuse == 1   g1 - g2 + g3 * q of the four d-wide slices of g
__device__ __forceinline__ void stage_go(float* dst, int pitch, int rows_pad, int cols_pad, const float* __restrict__ g, long long ldg,
                                         const float* __restrict__ q, long long ldq, const uint8_t* __restrict__ rz, int d, int fuse,
                                         int k0, int rows, int cols) {
  if (!fuse) {
    const float* gb = g + k0;
    const bool vg = vec_ok(gb, ldg);
    stage_f(dst, pitch, rows_pad, cols_pad, rows, cols, [=](int r, int cc) {
      if (rz && rz[r]) return make_float4(0.f, 0.f, 0.f, 0.f);
      return ld4(gb + (size_t)r * ldg + cc, vg, cols - cc);
    });
    return;
  }
  const float* g1 = g + d + k0;
  const float* g2 = g + 2 * (size_t)d + k0;
  const float* g3 = g + 3 * (size_t)d + k0;
  const float* qb = q + k0;
  const bool v1 = vec_ok(g1, ldg), v2 = vec_ok(g2, ldg), v3 = vec_ok(g3, ldg), vq = vec_ok(qb, ldq);
  stage_f(dst, pitch, rows_pad, cols_pad, rows, cols, [=](int r, int cc) {
    const int n = cols - cc;
    const float4 a = ld4(g1 + (size_t)r * ldg + cc, v1, n), b = ld4(g2 + (size_t)r * ldg + cc, v2, n);
    const float4 c = ld4(g3 + (size_t)r * ldg + cc, v3, n), x = ld4(qb + (size_t)r * ldq + cc, vq, n);
    return make_float4(fmaf(c.x, x.x, a.x - b.x), fmaf(c.y, x.y, a.y - b.y), fmaf(c.z, x.z, a.z - b.z), fmaf(c.w, x.w, a.w - b.w));
  });
}

// ============================================================================ soft_align forward
// grid b * ceil(lq / 16).  LDS: qs [16][pa] | ss [16][ps] | chunk
__global__ __launch_bounds__(MT_THREADS) void
sa_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
              long long ldv, const uint8_t* __restrict__ key_fill, const uint8_t* __restrict__ row_zero, float fill, int fuse, int lq,
              int lk, int d, int dv, float* __restrict__ a, float* __restrict__ out, long long ldo) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = mt_plan(lk, imax(d, dv));
  float* qs = sm;
  float* ss = qs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nrt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, lq - i0);
  const size_t r0 = (size_t)bi * lq + i0;
  const float* qb = q + r0 * ldq;
  const float* kb = k + (size_t)bi * lk * ldk;
  const float* vb = v + (size_t)bi * lk * ldv;
  const uint8_t* kf = key_fill + (size_t)bi * lk;

  for (int k0 = 0; k0 < d; k0 += MT_BLK) {      // S = q k^T over depth blocks
    const int nb = min(MT_BLK, d - k0);
    __syncthreads();
    stage(qs, P.pa, 16, up4(nb), qb + k0, ldq, ni, nb);
    scores_block(qs, P.pa, ch, P.pk, P.kc1, kb, ldk, lk, k0, nb, ss, P.ps, k0 > 0);
  }
  __syncthreads();
  {      // the fill and the row softmax: 16 lanes per row
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const bool live = row < ni;
    float* srow = ss + row * P.ps;
    float mx = -INFINITY;
    if (live)
      for (int j = sub; j < lk; j += 16) {
        const float s = kf[j] ? fill : srow[j];
        srow[j] = s;
        mx = fmaxf(mx, s);
      }
    mx = sub16_max(mx);
    float sum = 0.f;
    if (live)
      for (int j = sub; j < lk; j += 16) sum += expf(srow[j] - mx);
    sum = sub16_sum(sum);
    const int lkp = up16(lk);
    for (int j = sub; j < lkp; j += 16) {
      float w = 0.f;
      if (live && j < lk) w = expf(srow[j] - mx) / sum;
      srow[j] = w;
    }
  }
  __syncthreads();
  unstage(a + r0 * lk, lk, ss, P.ps, ni, lk);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const uint8_t* rz = row_zero ? row_zero + r0 : nullptr;
  for (int c0 = 0; c0 < dv; c0 += MT_BLK) {      // o = A v over column blocks
    const int nb = min(MT_BLK, dv - c0);
    f32x4 acc[MT_NT];
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    weighted_block<MT_NT>(ss, P.ps, ch, P.pv, P.kc2, vb, ldv, lk, c0, nb, acc);
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) {
      const int col = (wave + MT_WAVES * t) * 16 + l15;
      if (col < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) {
            float* xr = out + (r0 + i) * ldo + c0 + col;
            const float o = acc[t][r];
            if (fuse) {
              const float qv = qb[(size_t)i * ldq + c0 + col];
              xr[0] = qv;
              xr[d] = o;
              xr[2 * (size_t)d] = qv - o;
              xr[3 * (size_t)d] = qv * o;
            } else {
              xr[0] = (rz && rz[i]) ? 0.f : o;
            }
          }
        }
      }
    }
  }
}

// ============================================================================ soft_align backward, row tiles: dS and dq
// grid b * ceil(lq / 16).  LDS as the forward's: gs [16][pa] | ss [16][ps] | chunk
__global__ __launch_bounds__(MT_THREADS) void
sa_bwd_row_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
                  long long ldv, const uint8_t* __restrict__ key_fill, const uint8_t* __restrict__ row_zero, int fuse,
                  const float* __restrict__ a, const float* __restrict__ out, long long ldo, const float* __restrict__ g, long long ldg,
                  int lq, int lk, int d, int dv, float* __restrict__ ds, float* __restrict__ dq, long long lddq) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = mt_plan(lk, imax(d, dv));
  float* gs = sm;
  float* ss = gs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nrt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, lq - i0);
  const size_t r0 = (size_t)bi * lq + i0;
  const float* qb = q + r0 * ldq;
  const float* gb = g + r0 * ldg;
  const float* kb = k + (size_t)bi * lk * ldk;
  const float* vb = v + (size_t)bi * lk * ldv;
  const uint8_t* kf = key_fill + (size_t)bi * lk;
  const uint8_t* rz = row_zero ? row_zero + r0 : nullptr;

  for (int k0 = 0; k0 < dv; k0 += MT_BLK) {      // dA = g_o v^T
    const int nb = min(MT_BLK, dv - k0);
    __syncthreads();
    stage_go(gs, P.pa, 16, up4(nb), gb, ldg, qb, ldq, rz, d, fuse, k0, ni, nb);
    scores_block(gs, P.pa, ch, P.pk, P.kc1, vb, ldv, lk, k0, nb, ss, P.ps, k0 > 0);
  }
  __syncthreads();
  {      // dS = A (dA - rowsum(A dA)), zero at the filled keys
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const bool live = row < ni;
    const float* arow = a + (r0 + (live ? row : 0)) * lk;
    float* srow = ss + row * P.ps;
    float dot = 0.f;
    if (live)
      for (int j = sub; j < lk; j += 16) dot = fmaf(arow[j], srow[j], dot);
    dot = sub16_sum(dot);
    const int lkp = up16(lk);
    for (int j = sub; j < lkp; j += 16) {
      float w = 0.f;
      if (live && j < lk && !kf[j]) w = arow[j] * (srow[j] - dot);
      srow[j] = w;
    }
  }
  __syncthreads();
  unstage(ds + r0 * lk, lk, ss, P.ps, ni, lk);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int c0 = 0; c0 < d; c0 += MT_BLK) {      // dq = dS k (+ the direct part of the four-way epilogue)
    const int nb = min(MT_BLK, d - c0);
    f32x4 acc[MT_NT];
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    weighted_block<MT_NT>(ss, P.ps, ch, P.pv, P.kc2, kb, ldk, lk, c0, nb, acc);
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) {
      const int col = (wave + MT_WAVES * t) * 16 + l15;
      if (col < nb) {
        const int kx = c0 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) {
            float val = acc[t][r];
            if (fuse) {
              const float* gr = gb + (size_t)i * ldg + kx;
              const float o = out[(r0 + i) * ldo + d + kx];
              val += fmaf(gr[3 * (size_t)d], o, gr[0] + gr[2 * (size_t)d]);
            }
            dq[(r0 + i) * lddq + kx] = val;
          }
        }
      }
    }
  }
}

// ============================================================================ soft_align backward, key tiles: dk and dv
// grid b * ceil(lk / 16).  LDS: mm [rc][pm] | st [rc][16]
__global__ __launch_bounds__(MT_THREADS) void
sa_bwd_key_kernel(const float* __restrict__ q, long long ldq, const uint8_t* __restrict__ row_zero, int fuse, const float* __restrict__ a,
                  const float* __restrict__ ds, const float* __restrict__ g, long long ldg, int lq, int lk, int d, int dv,
                  float* __restrict__ dk, long long lddk, float* __restrict__ dvv, long long lddv) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const KeyPlan P = key_plan(lq, imax(d, dv));
  float* mm = sm;
  float* st = mm + P.rc * P.pm;
  const int nkt = (lk + 15) >> 4;
  const int bi = blockIdx.x / nkt, j0 = (blockIdx.x - bi * nkt) << 4;
  const int nk = min(16, lk - j0);
  const size_t q0 = (size_t)bi * lq;
  const size_t sbase = q0 * lk + j0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;

  for (int pass = 0; pass < 2; ++pass) {      // 0: dk = dS^T q over d, 1: dv = A^T g_o over dv
    const int w = pass ? dv : d;
    const float* tsrc = pass ? a : ds;
    float* dst = pass ? dvv : dk;
    const long long ldd = pass ? lddv : lddk;
    for (int c0 = 0; c0 < w; c0 += MT_BLK) {
      const int nb = min(MT_BLK, w - c0), nct = (nb + 15) >> 4;
      f32x4 acc[MT_NT];
#pragma unroll
      for (int t = 0; t < MT_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int i0 = 0; i0 < lq; i0 += P.rc) {
        const int nr = min(P.rc, lq - i0), rp = up4(nr);
        __syncthreads();
        if (pass)
          stage_go(mm, P.pm, rp, up16(nb), g + (q0 + i0) * ldg, ldg, q + (q0 + i0) * ldq, ldq, row_zero ? row_zero + q0 + i0 : nullptr, d,
                   fuse, c0, nr, nb);
        else
          stage(mm, P.pm, rp, up16(nb), q + (q0 + i0) * ldq + c0, ldq, nr, nb);
        stage(st, 16, rp, 16, tsrc + sbase + (size_t)i0 * lk, lk, nr, nk);
        __syncthreads();
        mma_acc<MT_NT>(st, 1, 16, mm, P.pm, rp, nct, acc);
      }
#pragma unroll
      for (int t = 0; t < MT_NT; ++t) {
        const int col = (wave + MT_WAVES * t) * 16 + l15;
        if (col < nb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 4 * qd + r;
            if (j < nk) dst[((size_t)bi * lk + j0 + j) * ldd + c0 + col] = acc[t][r];
          }
        }
      }
    }
  }
}

// ============================================================================ lin_att
__device__ __forceinline__ bool la_kept(float s, int mode) { return mode == 0 ? s != 0.f : (mode == 1 ? s == 1.f : true); }

// grid b.  One wave per position forms s_l = x_l . w from products only (an all-zero row scores exactly 0)
__global__ __launch_bounds__(MT_THREADS) void
la_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int mode, int l, int d, float* __restrict__ a) {
  __shared__ float sc[LA_MAX_L];
  __shared__ float red[MT_WAVES];
  const int bi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* xb = x + (size_t)bi * l * d;
  for (int i = wave; i < l; i += MT_WAVES) {
    float s = 0.f;
    for (int kx = lane; kx < d; kx += 64) s = fmaf(xb[(size_t)i * d + kx], w[kx], s);
    s = wave_sum(s);
    if (lane == 0) sc[i] = s;
  }
  __syncthreads();
  float mx = -INFINITY, cnt = 0.f;
  for (int i = threadIdx.x; i < l; i += MT_THREADS)
    if (la_kept(sc[i], mode)) {
      mx = fmaxf(mx, sc[i]);
      cnt += 1.f;
    }
  mx = block_max(mx, red);
  cnt = block_sum(cnt, red);
  float sum = 0.f;
  for (int i = threadIdx.x; i < l; i += MT_THREADS)
    if (la_kept(sc[i], mode)) sum += expf(sc[i] - mx);
  sum = block_sum(sum, red);
  float* ab = a + (size_t)bi * l;
  for (int i = threadIdx.x; i < l; i += MT_THREADS) {
    float o = la_kept(sc[i], mode) ? expf(sc[i] - mx) / sum : 0.f;
    if (cnt == 0.f) o = NAN;      // softmax over nothing, as the reference's row of -inf
    ab[i] = o;
  }
}

// grid b.  ds_l = a_l (g_l - sum a g); dx_l = ds_l w; part[bi] = sum_l ds_l x_l in position order
__global__ __launch_bounds__(MT_THREADS) void
la_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ a, const float* __restrict__ g, int l, int d,
              float* __restrict__ dx, float* __restrict__ part) {
  __shared__ float sc[LA_MAX_L];
  __shared__ float red[MT_WAVES];
  const int bi = blockIdx.x;
  const float* ab = a + (size_t)bi * l;
  const float* gb = g + (size_t)bi * l;
  float t = 0.f;
  for (int i = threadIdx.x; i < l; i += MT_THREADS) t = fmaf(ab[i], gb[i], t);
  t = block_sum(t, red);
  for (int i = threadIdx.x; i < l; i += MT_THREADS) sc[i] = ab[i] * (gb[i] - t);
  __syncthreads();
  const float* xb = x + (size_t)bi * l * d;
  float* dxb = dx + (size_t)bi * l * d;
  for (int col = threadIdx.x; col < d; col += MT_THREADS) {
    const float wc = w[col];
    float s = 0.f;
    for (int i = 0; i < l; ++i) {
      s = fmaf(sc[i], xb[(size_t)i * d + col], s);
      dxb[(size_t)i * d + col] = sc[i] * wc;
    }
    part[(size_t)bi * d + col] = s;
  }
}

// out[col] = the sum of part[row][col] over the rows, in row order
__global__ __launch_bounds__(MT_THREADS) void
sum_rows_kernel(const float* __restrict__ part, int nrows, int ncols, float* __restrict__ out) {
  const int col = blockIdx.x * MT_THREADS + threadIdx.x;
  if (col >= ncols) return;
  float s = 0.f;
  for (int r = 0; r < nrows; ++r) s += part[(size_t)r * ncols + col];
  out[col] = s;
}

// ============================================================================ match_dot
// inv[row] = 1 / max(||x_row||_2, 1e-12): one wave per row
__global__ __launch_bounds__(MT_THREADS) void
inv_norm_kernel(const float* __restrict__ x, long long ld, long long rows, int d, float* __restrict__ inv) {
  const long long row = (long long)blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * ld;
  float s = 0.f;
  for (int kx = lane; kx < d; kx += 64) s = fmaf(xr[kx], xr[kx], s);
  s = wave_sum(s);
  if (lane == 0) inv[row] = 1.f / fmaxf(sqrtf(s), 1e-12f);
}

// grid b * ceil(l / 16).  LDS: xs [16][pa] | ss [16][ps] | chunk
__global__ __launch_bounds__(MT_THREADS) void
md_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ldx, long long ldy, const float* __restrict__ ix,
              const float* __restrict__ iy, int l, int r, int d, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = mt_plan(r, d);
  float* xs = sm;
  float* ss = xs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nrt = (l + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, l - i0);
  const size_t r0 = (size_t)bi * l + i0;
  const float* xb = x + r0 * ldx;
  const float* yb = y + (size_t)bi * r * ldy;
  for (int k0 = 0; k0 < d; k0 += MT_BLK) {
    const int nb = min(MT_BLK, d - k0);
    __syncthreads();
    stage(xs, P.pa, 16, up4(nb), xb + k0, ldx, ni, nb);
    scores_block(xs, P.pa, ch, P.pk, P.kc1, yb, ldy, r, k0, nb, ss, P.ps, k0 > 0);
  }
  __syncthreads();
  if (ix) {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    if (row < ni) {
      const float sx = ix[r0 + row];
      const float* iyb = iy + (size_t)bi * r;
      for (int j = sub; j < r; j += 16) ss[row * P.ps + j] = ss[row * P.ps + j] * sx * iyb[j];
    }
    __syncthreads();
  }
  unstage(out + r0 * r, r, ss, P.ps, ni, r);
}

// The gradient of one side (rows `s` [b][ls][d], ld lds_) from the other (`o` [b][lo][d], ldo_):
//   gs_ij = g_ij is_i io_j  (g element (i, j) at g[i * lo + j], or at g[j * ls + i] when TRANS: the right side reads g^T)
//   d_i = sum_j gs_ij o_j;  with the norms and a row above the clamp (is_i < 1 / 1e-12f):  d_i -= s_i (s_i . d_i) is_i^2
// grid b * ceil(ls / 16).  LDS: ss [16][ps] | chunk
template <bool TRANS>
__global__ __launch_bounds__(MT_THREADS) void
md_bwd_kernel(const float* __restrict__ s, const float* __restrict__ o, long long lds_, long long ldo_, const float* __restrict__ is,
              const float* __restrict__ io, const float* __restrict__ g, int ls, int lo, int d, float* __restrict__ ds_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = mt_plan(lo, d);
  float* ss = sm;
  float* ch = ss + 16 * P.ps;
  const int nrt = (ls + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, ls - i0);
  const size_t r0 = (size_t)bi * ls + i0;
  const float* ob = o + (size_t)bi * lo * ldo_;
  const float* gb = g + (size_t)bi * ls * lo;
  const int lop = up16(lo);
  for (int idx = threadIdx.x; idx < 16 * lop; idx += MT_THREADS) {
    int i, j;
    if (TRANS) {
      j = idx >> 4;
      i = idx & 15;
    } else {
      i = idx / lop;
      j = idx - i * lop;
    }
    float val = 0.f;
    if (i < ni && j < lo) {
      val = TRANS ? gb[(size_t)j * ls + i0 + i] : gb[(size_t)(i0 + i) * lo + j];
      if (is) val = val * is[r0 + i] * io[(size_t)bi * lo + j];
    }
    ss[i * P.ps + j] = val;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int c0 = 0; c0 < d; c0 += MT_BLK) {
    const int nb = min(MT_BLK, d - c0);
    f32x4 acc[MT_NT];
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    weighted_block<MT_NT>(ss, P.ps, ch, P.pv, P.kc2, ob, ldo_, lo, c0, nb, acc);
#pragma unroll
    for (int t = 0; t < MT_NT; ++t) {
      const int col = (wave + MT_WAVES * t) * 16 + l15;
      if (col < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) ds_out[(r0 + i) * d + c0 + col] = acc[t][r];
        }
      }
    }
  }
  if (!is) return;
  __threadfence_block();
  __syncthreads();      // the rows this workgroup wrote above are re-read below, by other lanes
  const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const bool live = row < ni;
  const float* sr = s + (r0 + (live ? row : 0)) * lds_;
  float* dr = ds_out + (r0 + (live ? row : 0)) * d;
  const float inv = live ? is[r0 + row] : 0.f;
  float dot = 0.f;
  if (live)
    for (int kx = sub; kx < d; kx += 16) dot = fmaf(sr[kx], dr[kx], dot);
  dot = sub16_sum(dot);
  if (live && inv < 1.f / 1e-12f) {      // F.normalize's clamp_min: a row at or below 1e-12 (inv_norm_kernel's clamp) keeps the raw gradient
    const float c = dot * inv * inv;
    for (int kx = sub; kx < d; kx += 16) dr[kx] = fmaf(-sr[kx], c, dr[kx]);
  }
}

// ============================================================================ match_bcast
enum { BC_MUL = 0, BC_PLUS = 1, BC_MINUS = 2, BC_CONCAT = 3 };

__device__ __forceinline__ float bc1(float xv, float yv, int op) { return op == BC_MUL ? xv * yv : (op == BC_PLUS ? xv + yv : xv - yv); }

// out [b][l][r][dd] in units of W floats (W = 4: d % 4 == 0 and 16-byte aligned bases); 64-bit offsets
template <int W>
__global__ __launch_bounds__(MT_THREADS) void
bc_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int op, int l, int r, int d, long long total, float* __restrict__ out) {
  const int dd = op == BC_CONCAT ? 2 * d : d, cw = dd / W;
  const long long stride = (long long)gridDim.x * MT_THREADS;
  for (long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x; e < total; e += stride) {
    const long long row = e / cw;
    const int c = (int)(e - row * cw) * W;
    const long long xrow = row / r;
    const int rr = (int)(row - xrow * r);
    const long long yrow = (xrow / l) * r + rr;
    if (W == 4) {
      float4 o;
      if (op == BC_CONCAT) {
        o = c < d ? *reinterpret_cast<const float4*>(x + xrow * d + c) : *reinterpret_cast<const float4*>(y + yrow * d + (c - d));
      } else {
        const float4 u = *reinterpret_cast<const float4*>(x + xrow * d + c), w = *reinterpret_cast<const float4*>(y + yrow * d + c);
        o = make_float4(bc1(u.x, w.x, op), bc1(u.y, w.y, op), bc1(u.z, w.z, op), bc1(u.w, w.w, op));
      }
      *reinterpret_cast<float4*>(out + row * dd + c) = o;
    } else {
      float o;
      if (op == BC_CONCAT) o = c < d ? x[xrow * d + c] : y[yrow * d + (c - d)];
      else o = bc1(x[xrow * d + c], y[yrow * d + c], op);
      out[row * dd + c] = o;
    }
  }
}

// side 0: dx [b * l][d], element (xrow, k) = sum over rr of (g * y | g | g | g[:d]) in rr order
// side 1: dy [b * r][d], element (yrow, k) = sum over ll of (g * x | g | -g | g[d:]) in ll order
__global__ __launch_bounds__(MT_THREADS) void
bc_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, int op, int side, int l, int r, int d,
              long long total, float* __restrict__ dst) {
  const int dd = op == BC_CONCAT ? 2 * d : d;
  const long long stride = (long long)gridDim.x * MT_THREADS;
  for (long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x; e < total; e += stride) {
    const long long row = e / d;
    const int kx = (int)(e - row * d);
    float s = 0.f;
    if (side == 0) {
      const long long bi = row / l;
      const float* gp = g + row * r * dd + kx;
      const float* yp = y + bi * r * d + kx;
      for (int rr = 0; rr < r; ++rr) {
        const float gv = gp[(long long)rr * dd];
        s = op == BC_MUL ? fmaf(gv, yp[(long long)rr * d], s) : s + gv;
      }
    } else {
      const long long bi = row / r;
      const int rr = (int)(row - bi * r);
      const float* gp = g + (bi * l * r + rr) * dd + (op == BC_CONCAT ? d : 0) + kx;
      const float* xp = x + bi * l * d + kx;
      for (int ll = 0; ll < l; ++ll) {
        const float gv = gp[(long long)ll * r * dd];
        s = op == BC_MUL ? fmaf(gv, xp[(long long)ll * d], s) : (op == BC_MINUS ? s - gv : s + gv);
      }
    }
    dst[e] = s;
  }
}

// ============================================================================ gauss_kernel
__global__ __launch_bounds__(MT_THREADS) void
gk_fwd_kernel(const float* __restrict__ x, float mu, float s2, long long n, float* __restrict__ y) {
  const long long stride = (long long)gridDim.x * MT_THREADS;
  for (long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += stride) {
    const float t = x[i] - mu;
    y[i] = expf(-0.5f * (t * t) / s2);
  }
}
__global__ __launch_bounds__(MT_THREADS) void
gk_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, float mu, float s2, long long n,
              float* __restrict__ dx) {
  const long long stride = (long long)gridDim.x * MT_THREADS;
  for (long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += stride) dx[i] = -g[i] * y[i] * (x[i] - mu) / s2;
}

int flat_grid(long long n) {
  const long long want = (n + MT_THREADS - 1) / MT_THREADS;
  return (int)(want < 1 ? 1 : (want < 16384 ? want : 16384));
}

int sa_check(const char* who, int b, int lq, int lk, int d, int dv) {
  GH_REQUIRE(b >= 1 && lq >= 1 && lk >= 1 && d >= 1 && dv >= 1, "%s: empty problem (b=%d lq=%d lk=%d d=%d dv=%d)", who, b, lq, lk, d, dv);
  GH_REQUIRE(lq <= SA_MAX_L, "%s: lq=%d exceeds the supported %d", who, lq, SA_MAX_L);
  GH_REQUIRE(lk <= SA_MAX_L, "%s: lk=%d exceeds the supported %d", who, lk, SA_MAX_L);
  GH_REQUIRE(d <= SA_MAX_D, "%s: d=%d exceeds the supported %d", who, d, SA_MAX_D);
  GH_REQUIRE(dv <= SA_MAX_D, "%s: dv=%d exceeds the supported %d", who, dv, SA_MAX_D);
  GH_REQUIRE((long long)b * (((lq > lk ? lq : lk) + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  return 0;
}

int gk_check(const char* who, float mu, float sigma, long long n) {
  GH_REQUIRE(n >= 1, "%s: empty problem (n=%lld)", who, n);
  GH_REQUIRE(isfinite(mu) && isfinite(sigma), "%s: mu and sigma must be finite", who);
  GH_REQUIRE(sigma != 0.f, "%s: sigma == 0 (the kernel divides by sigma^2)", who);
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_soft_align_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const uint8_t* key_fill,
                                 const uint8_t* row_zero, float fill, int fuse, int b, int lq, int lk, int d, int dv, float* a, float* out,
                                 int ldo, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = sa_check("soft_align_fwd", b, lq, lk, d, dv)) return rc;
  GH_REQUIRE(q && k && v && key_fill && a && out, "soft_align_fwd: NULL argument");
  GH_REQUIRE(isfinite(fill), "soft_align_fwd: fill must be finite (a filled score keeps its weight; use a mask-excluding op for -inf)");
  GH_REQUIRE(fuse == 0 || fuse == 1, "soft_align_fwd: fuse=%d is neither 0 nor 1", fuse);
  GH_REQUIRE(!fuse || (dv == d && !row_zero), "soft_align_fwd: fuse needs dv == d (got %d, %d) and no row_zero", dv, d);
  GH_REQUIRE(ldq >= d && ldk >= d && ldv >= dv && (long long)ldo >= (fuse ? 4LL * d : (long long)dv),
             "soft_align_fwd: a leading dimension is smaller than its row");
  const size_t lds = (size_t)tile_lds_floats(mt_plan(lk, imax(d, dv))) * sizeof(float);
  if (int rc = lds_opt_in((const void*)sa_fwd_kernel, lds, "soft_align_fwd")) return rc;
  hipLaunchKernelGGL(sa_fwd_kernel, dim3(b * ((lq + 15) / 16)), dim3(MT_THREADS), lds, st, q, k, v, (long long)ldq, (long long)ldk,
                     (long long)ldv, key_fill, row_zero, fill, fuse, lq, lk, d, dv, a, out, (long long)ldo);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_soft_align_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const uint8_t* key_fill,
                                 const uint8_t* row_zero, int fuse, const float* a, const float* out, int ldo, const float* g, int ldg,
                                 int b, int lq, int lk, int d, int dv, float* ds, float* dq, int lddq, float* dk, int lddk, float* dvv,
                                 int lddv, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = sa_check("soft_align_bwd", b, lq, lk, d, dv)) return rc;
  GH_REQUIRE(q && k && v && key_fill && a && g && ds && dq && dk && dvv && (!fuse || out), "soft_align_bwd: NULL argument");
  GH_REQUIRE(fuse == 0 || fuse == 1, "soft_align_bwd: fuse=%d is neither 0 nor 1", fuse);
  GH_REQUIRE(!fuse || (dv == d && !row_zero), "soft_align_bwd: fuse needs dv == d (got %d, %d) and no row_zero", dv, d);
  const long long wo = fuse ? 4LL * d : (long long)dv;
  GH_REQUIRE(ldq >= d && ldk >= d && ldv >= dv && lddq >= d && lddk >= d && lddv >= dv && ldg >= wo && (!fuse || ldo >= wo),
             "soft_align_bwd: a leading dimension is smaller than its row");
  const size_t lds_r = (size_t)tile_lds_floats(mt_plan(lk, imax(d, dv))) * sizeof(float);
  const size_t lds_k = (size_t)key_lds_floats(key_plan(lq, imax(d, dv))) * sizeof(float);
  if (int rc = lds_opt_in((const void*)sa_bwd_row_kernel, lds_r, "soft_align_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)sa_bwd_key_kernel, lds_k, "soft_align_bwd")) return rc;
  hipLaunchKernelGGL(sa_bwd_row_kernel, dim3(b * ((lq + 15) / 16)), dim3(MT_THREADS), lds_r, st, q, k, v, (long long)ldq, (long long)ldk,
                     (long long)ldv, key_fill, row_zero, fuse, a, out, (long long)ldo, g, (long long)ldg, lq, lk, d, dv, ds, dq,
                     (long long)lddq);
  hipLaunchKernelGGL(sa_bwd_key_kernel, dim3(b * ((lk + 15) / 16)), dim3(MT_THREADS), lds_k, st, q, (long long)ldq, row_zero, fuse, a, ds, g,
                     (long long)ldg, lq, lk, d, dv, dk, (long long)lddk, dvv, (long long)lddv);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_lin_att_fwd(const float* x, const float* w, int mode, int b, int l, int d, float* a, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(b >= 1 && l >= 1 && d >= 1, "lin_att_fwd: empty problem (b=%d l=%d d=%d)", b, l, d);
  GH_REQUIRE(l <= LA_MAX_L, "lin_att_fwd: l=%d exceeds the supported %d", l, LA_MAX_L);
  GH_REQUIRE(d <= SA_MAX_D, "lin_att_fwd: d=%d exceeds the supported %d", d, SA_MAX_D);
  GH_REQUIRE(mode >= 0 && mode <= 2, "lin_att_fwd: mode=%d is not 0, 1 or 2", mode);
  GH_REQUIRE(x && w && a, "lin_att_fwd: NULL argument");
  hipLaunchKernelGGL(la_fwd_kernel, dim3(b), dim3(MT_THREADS), 0, st, x, w, mode, l, d, a);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_lin_att_bwd(const float* x, const float* w, const float* a, const float* g, int b, int l, int d, float* dx, float* part,
                              float* dw, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  GH_REQUIRE(b >= 1 && l >= 1 && d >= 1, "lin_att_bwd: empty problem (b=%d l=%d d=%d)", b, l, d);
  GH_REQUIRE(l <= LA_MAX_L, "lin_att_bwd: l=%d exceeds the supported %d", l, LA_MAX_L);
  GH_REQUIRE(d <= SA_MAX_D, "lin_att_bwd: d=%d exceeds the supported %d", d, SA_MAX_D);
  GH_REQUIRE(x && w && a && g && dx && part && dw, "lin_att_bwd: NULL argument");
  hipLaunchKernelGGL(la_bwd_kernel, dim3(b), dim3(MT_THREADS), 0, st, x, w, a, g, l, d, dx, part);
  hipLaunchKernelGGL(sum_rows_kernel, dim3((d + MT_THREADS - 1) / MT_THREADS), dim3(MT_THREADS), 0, st, part, b, d, dw);
  GH_LAUNCH_CHECK();
  return 0;
}

static int md_check(const char* who, int b, int l, int r, int d) {
  GH_REQUIRE(b >= 1 && l >= 1 && r >= 1 && d >= 1, "%s: empty problem (b=%d l=%d r=%d d=%d)", who, b, l, r, d);
  GH_REQUIRE(l <= SA_MAX_L, "%s: l=%d exceeds the supported %d", who, l, SA_MAX_L);
  GH_REQUIRE(r <= SA_MAX_L, "%s: r=%d exceeds the supported %d", who, r, SA_MAX_L);
  GH_REQUIRE(d <= SA_MAX_D, "%s: d=%d exceeds the supported %d", who, d, SA_MAX_D);
  GH_REQUIRE((long long)b * (((l > r ? l : r) + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  return 0;
}

extern "C" int gh_match_dot_fwd(const float* x, const float* y, int ldx, int ldy, int normalize, int b, int l, int r, int d, float* ix,
                                float* iy, float* out, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = md_check("match_dot_fwd", b, l, r, d)) return rc;
  GH_REQUIRE(x && y && out && (!normalize || (ix && iy)), "match_dot_fwd: NULL argument");
  GH_REQUIRE(ldx >= d && ldy >= d, "match_dot_fwd: a leading dimension is smaller than its row");
  const size_t lds = (size_t)tile_lds_floats(mt_plan(r, d)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)md_fwd_kernel, lds, "match_dot_fwd")) return rc;
  if (normalize) {
    const long long nx = (long long)b * l, ny = (long long)b * r;
    hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)((nx + MT_WAVES - 1) / MT_WAVES)), dim3(MT_THREADS), 0, st, x, (long long)ldx, nx, d, ix);
    hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)((ny + MT_WAVES - 1) / MT_WAVES)), dim3(MT_THREADS), 0, st, y, (long long)ldy, ny, d, iy);
  }
  hipLaunchKernelGGL(md_fwd_kernel, dim3(b * ((l + 15) / 16)), dim3(MT_THREADS), lds, st, x, y, (long long)ldx, (long long)ldy,
                     normalize ? ix : (const float*)nullptr, normalize ? iy : (const float*)nullptr, l, r, d, out);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_match_dot_bwd(const float* x, const float* y, int ldx, int ldy, int normalize, const float* ix, const float* iy,
                                const float* g, int b, int l, int r, int d, float* dx, float* dy, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = md_check("match_dot_bwd", b, l, r, d)) return rc;
  GH_REQUIRE(x && y && g && dx && dy && (!normalize || (ix && iy)), "match_dot_bwd: NULL argument");
  GH_REQUIRE(ldx >= d && ldy >= d, "match_dot_bwd: a leading dimension is smaller than its row");
  const size_t lds_x = (size_t)(tile_lds_floats(mt_plan(r, d))) * sizeof(float);
  const size_t lds_y = (size_t)(tile_lds_floats(mt_plan(l, d))) * sizeof(float);
  if (int rc = lds_opt_in((const void*)md_bwd_kernel<false>, lds_x, "match_dot_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)md_bwd_kernel<true>, lds_y, "match_dot_bwd")) return rc;
  const float* nx = normalize ? ix : nullptr;
  const float* ny = normalize ? iy : nullptr;
  hipLaunchKernelGGL(md_bwd_kernel<false>, dim3(b * ((l + 15) / 16)), dim3(MT_THREADS), lds_x, st, x, y, (long long)ldx, (long long)ldy, nx,
                     ny, g, l, r, d, dx);
  hipLaunchKernelGGL(md_bwd_kernel<true>, dim3(b * ((r + 15) / 16)), dim3(MT_THREADS), lds_y, st, y, x, (long long)ldy, (long long)ldx, ny,
                     nx, g, r, l, d, dy);
  GH_LAUNCH_CHECK();
  return 0;
}

static int bc_check(const char* who, int op, int b, int l, int r, int d) {
  GH_REQUIRE(b >= 1 && l >= 1 && r >= 1 && d >= 1, "%s: empty problem (b=%d l=%d r=%d d=%d)", who, b, l, r, d);
  GH_REQUIRE(op >= BC_MUL && op <= BC_CONCAT, "%s: op=%d is not mul (0), plus (1), minus (2) or concat (3)", who, op);
  GH_REQUIRE(d <= SA_MAX_D, "%s: d=%d exceeds the supported %d", who, d, SA_MAX_D);
  return 0;
}

extern "C" int gh_match_bcast_fwd(const float* x, const float* y, int op, int b, int l, int r, int d, float* out, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = bc_check("match_bcast_fwd", op, b, l, r, d)) return rc;
  GH_REQUIRE(x && y && out, "match_bcast_fwd: NULL argument");
  const long long total = (long long)b * l * r * (op == BC_CONCAT ? 2 * d : d);
  if ((d & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(out))
    hipLaunchKernelGGL(bc_fwd_kernel<4>, dim3(flat_grid(total / 4)), dim3(MT_THREADS), 0, st, x, y, op, l, r, d, total / 4, out);
  else
    hipLaunchKernelGGL(bc_fwd_kernel<1>, dim3(flat_grid(total)), dim3(MT_THREADS), 0, st, x, y, op, l, r, d, total, out);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_match_bcast_bwd(const float* x, const float* y, const float* g, int op, int b, int l, int r, int d, float* dx, float* dy,
                                  gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = bc_check("match_bcast_bwd", op, b, l, r, d)) return rc;
  GH_REQUIRE(x && y && g && dx && dy, "match_bcast_bwd: NULL argument");
  const long long nx = (long long)b * l * d, ny = (long long)b * r * d;
  hipLaunchKernelGGL(bc_bwd_kernel, dim3(flat_grid(nx)), dim3(MT_THREADS), 0, st, x, y, g, op, 0, l, r, d, nx, dx);
  hipLaunchKernelGGL(bc_bwd_kernel, dim3(flat_grid(ny)), dim3(MT_THREADS), 0, st, x, y, g, op, 1, l, r, d, ny, dy);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_gauss_kernel_fwd(const float* x, float mu, float sigma, long long n, float* y, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gk_check("gauss_kernel_fwd", mu, sigma, n)) return rc;
  GH_REQUIRE(x && y, "gauss_kernel_fwd: NULL argument");
  hipLaunchKernelGGL(gk_fwd_kernel, dim3(flat_grid(n)), dim3(MT_THREADS), 0, st, x, mu, (float)((double)sigma * (double)sigma), n, y);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_gauss_kernel_bwd(const float* x, const float* y, const float* g, float mu, float sigma, long long n, float* dx,
                                   gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gk_check("gauss_kernel_bwd", mu, sigma, n)) return rc;
  GH_REQUIRE(x && y && g && dx, "gauss_kernel_bwd: NULL argument");
  hipLaunchKernelGGL(gk_bwd_kernel, dim3(flat_grid(n)), dim3(MT_THREADS), 0, st, x, y, g, mu, (float)((double)sigma * (double)sigma), n, dx);
  GH_LAUNCH_CHECK();
  return 0;
}
