// The pairwise interaction helpers the sequence-matching baselines are assembled from:
//   gh_pair_l2_*       torch_utils.py:311-329 (cosine_distance, which is the Euclidean distance sqrt(|A2 - 2 a.b + B2| + eps))
//   gh_pair_l1_*       torch_utils.py:332-348 (l1_distance) without the (B,L,R,D) difference tensor
//   gh_window_mean_*   torch_utils.py:292-308 (moving_average), :351-376 (_get_doc_context_copacrr), layers.py:42-66 (MovingAverage)
//   gh_match_hist      matchzoo/preprocessors/units/matching_histogram.py:44-60 over a batch
//                      (data_generator/callbacks/histogram.py:37-65)
//
//   pair_l2 forward    the 16-row score tile of match_dot (score_tile.hip.h, exact fp32 MFMA) with the squared row norms from a
//                      one-wave-per-row launch; the epilogue turns the LDS tile into the distance in the reference's order of
//                      operations, (A2 - 2 dot) + B2, and saves the sign of that inner value as one byte per entry: it cannot be
//                      recovered from the output, and |.| has the gradient sign(inner), 0 at 0.
//   pair_l2 backward   one kernel, run once per side: w = g 0.5 / out sign into the LDS tile (read transposed for the right
//                      side), d_rows = 2 s rowsum(w) - 2 w other: one MFMA product and a row sum in a fixed order.
//   pair_l1 forward    VALU: a 32 x 64 output tile per workgroup over depth chunks of 64 staged in LDS, 2 x 4 outputs per lane.
//   pair_l1 backward   one kernel per side: a workgroup owns 16 whole rows of its side, a lane one column of four of them, and
//                      walks the other side's rows in chunks of 64: d_s = sum g sign(s - o), sign(0) = 0.
//   window_mean        a (rows + w - 1) x columns slab of the source in LDS, every window summed directly from it in row order;
//                      the backward is the same kernel on g (masked while it is staged) with the window reversed.
//   match_hist         one workgroup per (sample, 16 left ids): table rows gathered through the ids straight into the LDS
//                      operands of the score tile, integer counters in LDS.
// Every output element has one owner and there are no floating-point atomics: two runs are bit-identical.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include "score_tile.hip.h"
#include <math.h>

namespace gh {
namespace {

constexpr int PR_THREADS = 256;
static_assert(PR_THREADS == TILE_THREADS, "score_tile.hip.h strides its loops by its own workgroup size");
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_MAX_L = 1024;           // one 16-row score tile [16][r] in LDS, as the match family
constexpr int PR_MAX_D = 2048;
constexpr int PR_BLK = 128;              // the depth / column block and the chunk of match_ops.hip
constexpr int PR_NT = PR_BLK / 16 / PR_WAVES;
constexpr int PR_CHUNK = 16 * 656;
constexpr int WM_MAX_W = 1024;           // window rows: the slab of 16 columns then takes 67 KB of LDS
constexpr int WM_MAX_L = 1 << 20;
constexpr int WM_ROWS = 32;              // output rows of one workgroup
constexpr int MH_MAX_BINS = 256;         // 16 rows of integer counters: 16 KB of LDS beside the score tile

__host__ __device__ inline TilePlan pr_plan(int n, int w) { return tile_plan<PR_BLK, PR_CHUNK>(n, w); }
// LDS floats of the row-tiled kernels: left [16][pa] | ss [16][ps] | chunk | 16 row sums
__host__ __device__ inline int pr_lds_floats(const TilePlan& p) { return 16 * p.pa + 16 * p.ps + p.chunk + 16; }

// sq[row] = sum_k x[row][k]^2: one wave per row
__global__ __launch_bounds__(PR_THREADS) void
sq_norm_kernel(const float* __restrict__ x, long long ld, long long rows, int d, float* __restrict__ sq) {
  const long long row = (long long)blockIdx.x * PR_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * ld;
  float s = 0.f;
  for (int kx = lane; kx < d; kx += 64) s = fmaf(xr[kx], xr[kx], s);
  s = wave_sum(s);
  if (lane == 0) sq[row] = s;
}

// ============================================================================ pair_l2
// grid b * ceil(l / 16).  LDS: xs [16][pa] | ss [16][ps] | chunk
__global__ __launch_bounds__(PR_THREADS) void
pl2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ldx, long long ldy, const float* __restrict__ x2,
               const float* __restrict__ y2, float eps, int l, int r, int d, float* __restrict__ out, int8_t* __restrict__ sgn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = pr_plan(r, d);
  float* xs = sm;
  float* ss = xs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nrt = (l + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, l - i0);
  const size_t r0 = (size_t)bi * l + i0;
  const float* xb = x + r0 * ldx;
  const float* yb = y + (size_t)bi * r * ldy;
  for (int k0 = 0; k0 < d; k0 += PR_BLK) {
    const int nb = min(PR_BLK, d - k0);
    __syncthreads();
    stage(xs, P.pa, 16, up4(nb), xb + k0, ldx, ni, nb);
    scores_block(xs, P.pa, ch, P.pk, P.kc1, yb, ldy, r, k0, nb, ss, P.ps, k0 > 0);
  }
  __syncthreads();
  {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    if (row < ni) {
      const float xx = x2[r0 + row];
      const float* yy = y2 + (size_t)bi * r;
      int8_t* sg = sgn + (r0 + row) * r;
      for (int j = sub; j < r; j += 16) {
        const float inner = (xx - 2.f * ss[row * P.ps + j]) + yy[j];      // the reference's order: A2 - 2 dot + B2
        sg[j] = inner > 0.f ? 1 : (inner < 0.f ? -1 : 0);
        ss[row * P.ps + j] = sqrtf(fabsf(inner) + eps);
      }
    }
  }
  __syncthreads();
  unstage(out + r0 * r, r, ss, P.ps, ni, r);
}

// The gradient of one side (rows `s` [b][ls][d], ld lds_) from the other (`o` [b][lo][d], ldo_):
//   w_ij = g_ij 0.5 / out_ij sign_ij  (element (i, j) at [i * lo + j], or at [j * ls + i] when TRANS: the right side reads them transposed)
//   d_i = 2 s_i sum_j w_ij - 2 sum_j w_ij o_j
// grid b * ceil(ls / 16).  LDS: ss [16][ps] | chunk | rs [16]
template <bool TRANS>
__global__ __launch_bounds__(PR_THREADS) void
pl2_bwd_kernel(const float* __restrict__ s, const float* __restrict__ o, long long lds_, long long ldo_, const float* __restrict__ out,
               const int8_t* __restrict__ sgn, const float* __restrict__ g, int ls, int lo, int d, float* __restrict__ ds_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = pr_plan(lo, d);
  float* ss = sm;
  float* ch = ss + 16 * P.ps;
  float* rs = ch + P.chunk;
  const int nrt = (ls + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, ls - i0);
  const size_t r0 = (size_t)bi * ls + i0;
  const float* ob = o + (size_t)bi * lo * ldo_;
  const size_t e0 = (size_t)bi * ls * lo;
  const int lop = up16(lo);
  for (int idx = threadIdx.x; idx < 16 * lop; idx += PR_THREADS) {
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
      const size_t e = e0 + (TRANS ? (size_t)j * ls + i0 + i : (size_t)(i0 + i) * lo + j);
      val = g[e] * 0.5f / out[e] * (float)sgn[e];
    }
    ss[i * P.ps + j] = val;
  }
  __syncthreads();
  {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float t = 0.f;
    for (int j = sub; j < lop; j += 16) t += ss[row * P.ps + j];
    t = sub16_sum(t);
    if (sub == 0) rs[row] = t;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  for (int c0 = 0; c0 < d; c0 += PR_BLK) {
    const int nb = min(PR_BLK, d - c0);
    f32x4 acc[PR_NT];
#pragma unroll
    for (int t = 0; t < PR_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    weighted_block<PR_NT>(ss, P.ps, ch, P.pv, P.kc2, ob, ldo_, lo, c0, nb, acc);      // its first barrier publishes rs
#pragma unroll
    for (int t = 0; t < PR_NT; ++t) {
      const int col = (wave + PR_WAVES * t) * 16 + l15;
      if (col < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * qd + r;
          if (i < ni) ds_out[(r0 + i) * d + c0 + col] = 2.f * s[(r0 + i) * lds_ + c0 + col] * rs[i] - 2.f * acc[t][r];
        }
      }
    }
  }
}

// ============================================================================ pair_l1
constexpr int L1_TL = 32, L1_TR = 64, L1_DC = 64;      // output tile and depth chunk of the forward
constexpr int L1_P = 68;                               // pitch_kc(L1_DC)
constexpr int L1B_OC = 64, L1B_DC = 64;                // other-side rows and depth columns of one backward chunk
constexpr int L1B_PG = L1B_OC + 4;

// grid b * ceil(l / 32) * ceil(r / 64).  Lane (ty, tx) owns rows ty, ty + 16 and columns tx + 16 k, k < 4, of the tile
__global__ __launch_bounds__(PR_THREADS) void
pl1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ldx, long long ldy, int l, int r, int d,
               float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[L1_TL * L1_P];
  __shared__ __attribute__((aligned(16))) float ys[L1_TR * L1_P];
  const int ntl = (l + L1_TL - 1) / L1_TL, ntr = (r + L1_TR - 1) / L1_TR;
  const int bi = blockIdx.x / (ntl * ntr), rem = blockIdx.x - bi * ntl * ntr;
  const int l0 = (rem / ntr) * L1_TL, q0 = (rem % ntr) * L1_TR;
  const int nl = min(L1_TL, l - l0), nq = min(L1_TR, r - q0);
  const float* xb = x + ((size_t)bi * l + l0) * ldx;
  const float* yb = y + ((size_t)bi * r + q0) * ldy;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  float acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
  for (int k0 = 0; k0 < d; k0 += L1_DC) {
    const int nb = min(L1_DC, d - k0), nb4 = up4(nb);
    __syncthreads();
    stage(xs, L1_P, L1_TL, nb4, xb + k0, ldx, nl, nb);      // rows and columns beyond the operands are zeros on both sides: |0 - 0|
    stage(ys, L1_P, L1_TR, nb4, yb + k0, ldy, nq, nb);
    __syncthreads();
    for (int c = 0; c < nb4; c += 4) {
      float4 xv[2], yv[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const float4*>(xs + (ty + 16 * i) * L1_P + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) yv[k] = *reinterpret_cast<const float4*>(ys + (tx + 16 * k) * L1_P + c);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[i][k] += fabsf(xv[i].x - yv[k].x);
          acc[i][k] += fabsf(xv[i].y - yv[k].y);
          acc[i][k] += fabsf(xv[i].z - yv[k].z);
          acc[i][k] += fabsf(xv[i].w - yv[k].w);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int li = ty + 16 * i, qi = tx + 16 * k;
      if (li < nl && qi < nq) out[((size_t)bi * l + l0 + li) * r + q0 + qi] = acc[i][k];
    }
}

__device__ __forceinline__ float sign_times(float t, float g) { return t > 0.f ? g : (t < 0.f ? -g : 0.f); }

// d_s[i][k] = sum_j g_ij sign(s_ik - o_jk) in j order (g element (i, j) at [i * lo + j], or at [j * ls + i] when TRANS).
// grid b * ceil(ls / 16).  Wave w owns rows 4 w .. 4 w + 3 of the tile, lane c column c of the depth chunk
template <bool TRANS>
__global__ __launch_bounds__(PR_THREADS) void
pl1_bwd_kernel(const float* __restrict__ s, const float* __restrict__ o, long long lds_, long long ldo_, const float* __restrict__ g,
               int ls, int lo, int d, float* __restrict__ ds_out) {
  __shared__ __attribute__((aligned(16))) float os[L1B_OC * L1B_DC];
  __shared__ __attribute__((aligned(16))) float gs[16 * L1B_PG];
  const int nrt = (ls + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, ls - i0);
  const size_t r0 = (size_t)bi * ls + i0;
  const float* ob = o + (size_t)bi * lo * ldo_;
  const float* gb = g + (size_t)bi * ls * lo;
  const int wave = threadIdx.x >> 6, col = threadIdx.x & 63;
  for (int c0 = 0; c0 < d; c0 += L1B_DC) {
    const int nb = min(L1B_DC, d - c0);
    float sv[4], acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * wave + q;
      sv[q] = (i < ni && col < nb) ? s[(r0 + i) * lds_ + c0 + col] : 0.f;
      acc[q] = 0.f;
    }
    for (int j0 = 0; j0 < lo; j0 += L1B_OC) {
      const int nk = min(L1B_OC, lo - j0), nk4 = up4(nk);
      __syncthreads();
      stage(os, L1B_DC, nk4, L1B_DC, ob + (size_t)j0 * ldo_ + c0, ldo_, nk, nb);
      for (int idx = threadIdx.x; idx < 16 * L1B_OC; idx += PR_THREADS) {
        int i, j;
        if (TRANS) {
          j = idx >> 4;
          i = idx & 15;
        } else {
          i = idx >> 6;
          j = idx & 63;
        }
        float val = 0.f;      // zero beyond the rows of either side: those terms add +-0
        if (i < ni && j < nk) val = TRANS ? gb[(size_t)(j0 + j) * ls + i0 + i] : gb[(size_t)(i0 + i) * lo + j0 + j];
        gs[i * L1B_PG + j] = val;
      }
      __syncthreads();
      for (int j = 0; j < nk4; j += 4) {
        float4 gq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) gq[q] = *reinterpret_cast<const float4*>(gs + (4 * wave + q) * L1B_PG + j);
        const float o0 = os[(j + 0) * L1B_DC + col], o1 = os[(j + 1) * L1B_DC + col];
        const float o2 = os[(j + 2) * L1B_DC + col], o3 = os[(j + 3) * L1B_DC + col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[q] += sign_times(sv[q] - o0, gq[q].x);
          acc[q] += sign_times(sv[q] - o1, gq[q].y);
          acc[q] += sign_times(sv[q] - o2, gq[q].z);
          acc[q] += sign_times(sv[q] - o3, gq[q].w);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * wave + q;
      if (i < ni && col < nb) ds_out[(r0 + i) * d + c0 + col] = acc[q];
    }
  }
}

// ============================================================================ window_mean
// dst[b][t][:] = 1 / w * sum_{k < w} src[b][t + off + k][:], rows outside [0, n_in) count as zeros.  mask (NULL ok) multiplies
// the output rows ([b][n_out]), or with mask_in the source rows while they are staged ([b][n_in]: the backward); a row whose
// mask is 0 is an exact zero.
// grid b * ceil(n_out / WM_ROWS) * ceil(d / cb).  LDS: slab [WM_ROWS + w - 1][cb]
__global__ __launch_bounds__(PR_THREADS) void
wm_kernel(const float* __restrict__ src, long long ld, int n_in, int n_out, int off, int w, const float* __restrict__ mask, int mask_in,
          int d, int cb, float* __restrict__ dst, long long ldd) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nrt = (n_out + WM_ROWS - 1) / WM_ROWS, nct = (d + cb - 1) / cb;
  const int bi = blockIdx.x / (nrt * nct), rem = blockIdx.x - bi * nrt * nct;
  const int t0 = (rem / nct) * WM_ROWS, c0 = (rem % nct) * cb;
  const int nt = min(WM_ROWS, n_out - t0), nc = min(cb, d - c0);
  const int c4n = cb >> 2, nslab = nt + w - 1;
  const float* sb = src + (size_t)bi * n_in * ld + c0;
  const bool vs = vec_ok(sb, ld);
  for (int idx = threadIdx.x; idx < nslab * c4n; idx += PR_THREADS) {
    const int k = idx / c4n, c = (idx - k * c4n) << 2;
    const int row = t0 + off + k;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0 && row < n_in && c < nc) {
      const float m = (mask && mask_in) ? mask[(size_t)bi * n_in + row] : 1.f;
      if (m != 0.f) {
        v = ld4(sb + (size_t)row * ld + c, vs, nc - c);
        if (mask && mask_in) v = make_float4(v.x * m, v.y * m, v.z * m, v.w * m);
      }
    }
    *reinterpret_cast<float4*>(sm + k * cb + c) = v;
  }
  __syncthreads();
  float* db = dst + ((size_t)bi * n_out + t0) * ldd + c0;
  const bool vd = vec_ok(db, ldd);
  const float wf = (float)w;
  for (int idx = threadIdx.x; idx < nt * c4n; idx += PR_THREADS) {
    const int t = idx / c4n, c = (idx - t * c4n) << 2;
    if (c >= nc) continue;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* p = sm + t * cb + c;
    for (int k = 0; k < w; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(p + k * cb);
      a.x += v.x;
      a.y += v.y;
      a.z += v.z;
      a.w += v.w;
    }
    a = make_float4(a.x / wf, a.y / wf, a.z / wf, a.w / wf);
    if (mask && !mask_in) {
      const float m = mask[(size_t)bi * n_out + t0 + t];
      a = m != 0.f ? make_float4(a.x * m, a.y * m, a.z * m, a.w * m) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float* q = db + (size_t)t * ldd + c;
    const int n = nc - c;
    if (vd && n >= 4) {
      *reinterpret_cast<float4*>(q) = a;
    } else {
      q[0] = a.x;
      if (n > 1) q[1] = a.y;
      if (n > 2) q[2] = a.z;
      if (n > 3) q[3] = a.w;
    }
  }
}

// columns of one slab: the widest of 64, 32, 16 whose slab stays within 64 KB (16 at the longest window: 67 KB, opted in)
int wm_cols(int w, int d) {
  int cb = 64;
  while (cb > 16 && (size_t)(WM_ROWS + w - 1) * cb * sizeof(float) > 65536) cb >>= 1;
  while (cb > 16 && (cb >> 1) >= d) cb >>= 1;
  return cb;
}

int wm_launch(const char* who, const float* src, long long ld, int n_in, int n_out, int off, int w, const float* mask, int mask_in, int b,
              int d, float* dst, long long ldd, hipStream_t st) {
  const int cb = wm_cols(w, d);
  const size_t lds = (size_t)(WM_ROWS + w - 1) * cb * sizeof(float);
  const long long grid = (long long)b * ((n_out + WM_ROWS - 1) / WM_ROWS) * ((d + cb - 1) / cb);
  GH_REQUIRE(grid <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  if (int rc = lds_opt_in((const void*)wm_kernel, lds, who)) return rc;
  hipLaunchKernelGGL(wm_kernel, dim3((unsigned)grid), dim3(PR_THREADS), lds, st, src, ld, n_in, n_out, off, w, mask, mask_in, d, cb, dst,
                     ldd);
  GH_LAUNCH_CHECK();
  return 0;
}

int wm_check(const char* who, int b, int l, int d, int w, int left, int right) {
  GH_REQUIRE(b >= 1 && l >= 1 && d >= 1, "%s: empty problem (b=%d l=%d d=%d)", who, b, l, d);
  GH_REQUIRE(w >= 1 && w <= WM_MAX_W, "%s: window=%d is outside 1 .. %d", who, w, WM_MAX_W);
  GH_REQUIRE(left >= 0 && right >= 0 && left <= WM_MAX_W && right <= WM_MAX_W, "%s: left=%d / right=%d padding rows are outside 0 .. %d",
             who, left, right, WM_MAX_W);
  GH_REQUIRE(l <= WM_MAX_L, "%s: l=%d exceeds the supported %d", who, l, WM_MAX_L);
  GH_REQUIRE(d <= PR_MAX_D, "%s: d=%d exceeds the supported %d", who, d, PR_MAX_D);
  GH_REQUIRE(l + left + right - w + 1 >= 1, "%s: the window %d is longer than the padded sequence %d (an empty result is the caller's)", who,
             w, l + left + right);
  return 0;
}

// ============================================================================ match_hist
// flag[0] = 1 where a left id, or a right id below its sample's length, lies outside [0, v)
__global__ __launch_bounds__(PR_THREADS) void
mh_check_kernel(const int32_t* __restrict__ idl, const int32_t* __restrict__ idr, const int32_t* __restrict__ lenr, int b, int lq, int ldoc,
                int v, int32_t* __restrict__ flag) {
  const long long nl = (long long)b * lq, total = nl + (long long)b * ldoc;
  const long long stride = (long long)gridDim.x * PR_THREADS;
  bool bad = false;
  for (long long e = (long long)blockIdx.x * PR_THREADS + threadIdx.x; e < total; e += stride) {
    if (e < nl) {
      bad |= idl[e] < 0 || idl[e] >= v;
    } else {
      const long long f = e - nl;
      const int bi = (int)(f / ldoc), j = (int)(f - (long long)bi * ldoc);
      if (j < lenr[bi]) bad |= idr[f] < 0 || idr[f] >= v;
    }
  }
  if (bad) atomicOr(flag, 1);
}

// rows of the table through ids (count of them) -> LDS [rows_pad][pitch], zeros beyond (count, cols) and for an id outside the table
__device__ __forceinline__ void stage_gather(float* dst, int pitch, int rows_pad, int cols_pad, const float* __restrict__ table, long long ldt,
                                             int v, const int32_t* __restrict__ ids, int k0, int rows, int cols) {
  const bool vec = vec_ok(table + k0, ldt);
  stage_f(dst, pitch, rows_pad, cols_pad, rows, cols, [=](int r, int c) {
    const int id = ids[r];
    if (id < 0 || id >= v) return make_float4(0.f, 0.f, 0.f, 0.f);
    return ld4(table + (size_t)id * ldt + k0 + c, vec, cols - c);
  });
}

// grid b * ceil(lq / 16).  LDS: xs [16][pa] | ss [16][ps] | chunk | 16 floats | counters int [16][bins]
__global__ __launch_bounds__(PR_THREADS) void
mh_kernel(const float* __restrict__ table, long long ldt, const float* __restrict__ inv, int v, int d, const int32_t* __restrict__ idl,
          const int32_t* __restrict__ idr, const int32_t* __restrict__ lenr, int lq, int ldoc, int bins, int mode, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = pr_plan(ldoc, d);
  float* xs = sm;
  float* ss = xs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  int* hist = reinterpret_cast<int*>(ch + P.chunk + 16);
  const int nrt = (lq + 15) >> 4;
  const int bi = blockIdx.x / nrt, i0 = (blockIdx.x - bi * nrt) << 4;
  const int ni = min(16, lq - i0);
  const int n = min(max(lenr[bi], 0), ldoc);
  const int32_t* il = idl + (size_t)bi * lq + i0;
  const int32_t* ir = idr + (size_t)bi * ldoc;
  for (int idx = threadIdx.x; idx < 16 * bins; idx += PR_THREADS) hist[idx] = 0;
  for (int k0 = 0; k0 < d && n > 0; k0 += PR_BLK) {
    const int nb = min(PR_BLK, d - k0), nb4 = up4(nb);
    __syncthreads();
    stage_gather(xs, P.pa, 16, nb4, table, ldt, v, il, k0, ni, nb);
    for (int key0 = 0; key0 < n; key0 += P.kc1) {
      const int nk = imin(P.kc1, n - key0), rp = up16(nk);
      __syncthreads();
      stage_gather(ch, P.pk, rp, nb4, table, ldt, v, ir + key0, k0, nk, nb);
      __syncthreads();
      mma_scores(xs, P.pa, ch, P.pk, rp, nb4, ss, P.ps, key0, k0 > 0);
    }
  }
  __syncthreads();
  {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    if (row < ni) {
      const int idq = il[row];
      const float sq = (inv && idq >= 0 && idq < v) ? inv[idq] : 1.f;
      for (int j = sub; j < n; j += 16) {
        float val = ss[row * P.ps + j];
        if (inv) {
          const int idk = ir[j];
          val = val * sq * ((idk >= 0 && idk < v) ? inv[idk] : 1.f);
        }
        const float f = (val + 1.f) * 0.5f * (float)(bins - 1);
        int bin = f >= 0.f ? (f < (float)bins ? (int)f : bins - 1) : 0;      // truncation toward zero; NaN goes to bin 0
        if (bin > bins - 1) bin = bins - 1;
        atomicAdd(&hist[row * bins + bin], 1);      // integer counters in LDS: the order of the adds does not show
      }
    }
  }
  __syncthreads();
  const float total = (float)(bins + n);
  for (int idx = threadIdx.x; idx < ni * bins; idx += PR_THREADS) {
    const float c = (float)(hist[idx] + 1);
    out[((size_t)bi * lq + i0) * bins + idx] = mode == 0 ? c : (mode == 1 ? c / total : logf(c));
  }
}

int pr_check(const char* who, int b, int l, int r, int d) {
  GH_REQUIRE(b >= 1 && l >= 1 && r >= 1 && d >= 1, "%s: empty problem (b=%d l=%d r=%d d=%d)", who, b, l, r, d);
  GH_REQUIRE(l <= PR_MAX_L, "%s: l=%d exceeds the supported %d", who, l, PR_MAX_L);
  GH_REQUIRE(r <= PR_MAX_L, "%s: r=%d exceeds the supported %d", who, r, PR_MAX_L);
  GH_REQUIRE(d <= PR_MAX_D, "%s: d=%d exceeds the supported %d", who, d, PR_MAX_D);
  GH_REQUIRE((long long)b * ((l + 15) / 16) * ((r + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_pair_l2_fwd(const float* a, const float* b, int lda, int ldb, float eps, int bn, int l, int r, int d, float* a2, float* b2,
                              float* out, int8_t* sgn, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = pr_check("pair_l2_fwd", bn, l, r, d)) return rc;
  GH_REQUIRE(a && b && a2 && b2 && out && sgn, "pair_l2_fwd: NULL argument");
  GH_REQUIRE(lda >= d && ldb >= d, "pair_l2_fwd: a leading dimension is smaller than its row");
  GH_REQUIRE(isfinite(eps) && eps >= 0.f, "pair_l2_fwd: eps must be finite and >= 0");
  const size_t lds = (size_t)pr_lds_floats(pr_plan(r, d)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)pl2_fwd_kernel, lds, "pair_l2_fwd")) return rc;
  const long long na = (long long)bn * l, nb = (long long)bn * r;
  hipLaunchKernelGGL(sq_norm_kernel, dim3((unsigned)((na + PR_WAVES - 1) / PR_WAVES)), dim3(PR_THREADS), 0, st, a, (long long)lda, na, d, a2);
  hipLaunchKernelGGL(sq_norm_kernel, dim3((unsigned)((nb + PR_WAVES - 1) / PR_WAVES)), dim3(PR_THREADS), 0, st, b, (long long)ldb, nb, d, b2);
  hipLaunchKernelGGL(pl2_fwd_kernel, dim3(bn * ((l + 15) / 16)), dim3(PR_THREADS), lds, st, a, b, (long long)lda, (long long)ldb,
                     (const float*)a2, (const float*)b2, eps, l, r, d, out, sgn);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_pair_l2_bwd(const float* a, const float* b, int lda, int ldb, const float* out, const int8_t* sgn, const float* g, int bn,
                              int l, int r, int d, float* da, float* db, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = pr_check("pair_l2_bwd", bn, l, r, d)) return rc;
  GH_REQUIRE(a && b && out && sgn && g && da && db, "pair_l2_bwd: NULL argument");
  GH_REQUIRE(lda >= d && ldb >= d, "pair_l2_bwd: a leading dimension is smaller than its row");
  const size_t lds_a = (size_t)pr_lds_floats(pr_plan(r, d)) * sizeof(float);
  const size_t lds_b = (size_t)pr_lds_floats(pr_plan(l, d)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)pl2_bwd_kernel<false>, lds_a, "pair_l2_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)pl2_bwd_kernel<true>, lds_b, "pair_l2_bwd")) return rc;
  hipLaunchKernelGGL(pl2_bwd_kernel<false>, dim3(bn * ((l + 15) / 16)), dim3(PR_THREADS), lds_a, st, a, b, (long long)lda, (long long)ldb, out,
                     sgn, g, l, r, d, da);
  hipLaunchKernelGGL(pl2_bwd_kernel<true>, dim3(bn * ((r + 15) / 16)), dim3(PR_THREADS), lds_b, st, b, a, (long long)ldb, (long long)lda, out,
                     sgn, g, r, l, d, db);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_pair_l1_fwd(const float* a, const float* b, int lda, int ldb, int bn, int l, int r, int d, float* out, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = pr_check("pair_l1_fwd", bn, l, r, d)) return rc;
  GH_REQUIRE(a && b && out, "pair_l1_fwd: NULL argument");
  GH_REQUIRE(lda >= d && ldb >= d, "pair_l1_fwd: a leading dimension is smaller than its row");
  const int grid = bn * ((l + L1_TL - 1) / L1_TL) * ((r + L1_TR - 1) / L1_TR);
  hipLaunchKernelGGL(pl1_fwd_kernel, dim3(grid), dim3(PR_THREADS), 0, st, a, b, (long long)lda, (long long)ldb, l, r, d, out);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_pair_l1_bwd(const float* a, const float* b, int lda, int ldb, const float* g, int bn, int l, int r, int d, float* da,
                              float* db, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = pr_check("pair_l1_bwd", bn, l, r, d)) return rc;
  GH_REQUIRE(a && b && g && da && db, "pair_l1_bwd: NULL argument");
  GH_REQUIRE(lda >= d && ldb >= d, "pair_l1_bwd: a leading dimension is smaller than its row");
  hipLaunchKernelGGL(pl1_bwd_kernel<false>, dim3(bn * ((l + 15) / 16)), dim3(PR_THREADS), 0, st, a, b, (long long)lda, (long long)ldb, g, l, r,
                     d, da);
  hipLaunchKernelGGL(pl1_bwd_kernel<true>, dim3(bn * ((r + 15) / 16)), dim3(PR_THREADS), 0, st, b, a, (long long)ldb, (long long)lda, g, r, l,
                     d, db);
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_window_mean_fwd(const float* x, int ldx, const float* mask, int bn, int l, int d, int w, int left, int right, float* out,
                                  gh_stream_t stream) {
  if (int rc = wm_check("window_mean_fwd", bn, l, d, w, left, right)) return rc;
  GH_REQUIRE(x && out, "window_mean_fwd: NULL argument");
  GH_REQUIRE(ldx >= d, "window_mean_fwd: a leading dimension is smaller than its row");
  const int lo = l + left + right - w + 1;
  return wm_launch("window_mean_fwd", x, ldx, l, lo, -left, w, mask, 0, bn, d, out, d, (hipStream_t)stream);
}

extern "C" int gh_window_mean_bwd(const float* g, int ldg, const float* mask, int bn, int l, int d, int w, int left, int right, float* dx,
                                  gh_stream_t stream) {
  if (int rc = wm_check("window_mean_bwd", bn, l, d, w, left, right)) return rc;
  GH_REQUIRE(g && dx, "window_mean_bwd: NULL argument");
  GH_REQUIRE(ldg >= d, "window_mean_bwd: a leading dimension is smaller than its row");
  const int lo = l + left + right - w + 1;
  // dx_s = 1 / w * sum of the masked g_t over t = s + left - w + 1 .. s + left: the forward's window, reversed
  return wm_launch("window_mean_bwd", g, ldg, lo, l, left - w + 1, w, mask, 1, bn, d, dx, d, (hipStream_t)stream);
}

extern "C" int gh_match_hist(const float* table, int ldt, const float* inv_norm, int v, int d, const int32_t* ids_left,
                             const int32_t* ids_right, const int32_t* len_right, int bn, int lq, int ld, int bins, int mode, float* out,
                             int32_t* flag, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = pr_check("match_hist", bn, lq, ld, d)) return rc;
  GH_REQUIRE(table && ids_left && ids_right && len_right && out && flag, "match_hist: NULL argument");
  GH_REQUIRE(v >= 1 && ldt >= d, "match_hist: the table has v=%d rows of ldt=%d floats for d=%d", v, ldt, d);
  GH_REQUIRE(bins >= 1 && bins <= MH_MAX_BINS, "match_hist: bins=%d is outside 1 .. %d", bins, MH_MAX_BINS);
  GH_REQUIRE(mode >= 0 && mode <= 2, "match_hist: mode=%d is not CH (0), NH (1) or LCH (2)", mode);
  const size_t lds = (size_t)pr_lds_floats(pr_plan(ld, d)) * sizeof(float) + (size_t)16 * bins * sizeof(int);
  if (int rc = lds_opt_in((const void*)mh_kernel, lds, "match_hist")) return rc;
  // the ids are checked on the device before anything is read through them; the verdict is read back (this call synchronises)
  GH_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
  const long long n_ids = (long long)bn * lq + (long long)bn * ld;
  const long long want = (n_ids + PR_THREADS - 1) / PR_THREADS;
  hipLaunchKernelGGL(mh_check_kernel, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(PR_THREADS), 0, st, ids_left, ids_right, len_right, bn,
                     lq, ld, v, flag);
  GH_LAUNCH_CHECK();
  int32_t bad = 0;
  GH_CHECK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  GH_CHECK_HIP(hipStreamSynchronize(st));
  GH_REQUIRE(!bad, "match_hist: an id lies outside the table's rows [0, %d)", v);
  hipLaunchKernelGGL(mh_kernel, dim3(bn * ((lq + 15) / 16)), dim3(PR_THREADS), lds, st, table, (long long)ldt, inv_norm, v, d, ids_left,
                     ids_right, len_right, lq, ld, bins, mode, out);
  GH_LAUNCH_CHECK();
  return 0;
}
