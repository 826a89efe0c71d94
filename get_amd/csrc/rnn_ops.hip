// The recurrence of the LSTM sequence encoder (Models/BiDAF/wrapper.py:256-276, torch.nn.LSTM's cell equations):
//   gh_lstm_seq_fwd   h_t, c_t over t from gx = x W_ih^T + b_ih + b_hh (a GEMM of the caller's) and W_hh
//   gh_lstm_seq_bwd   dgates over t, walking time the other way
// and of the GRU sequence encoder (wrapper.py:306-327, torch.nn.GRU's cell equations) in the same layout, further down:
//   gh_gru_seq_fwd    h_t over t from gx = x W_ih^T + b_ih, W_hh and b_hh (b_hn sits inside the product with r: it cannot be folded)
//   gh_gru_seq_bwd    the gradients of gx and of the recurrent pre-activations over t, walking time the other way
// Only the sequential part lives here: the input projection, its gradients and dW_hh = dgates^T h_prev are activation-sized GEMMs
// of gh_linear_* (dense_ops.hip).  Both directions of a layer run in one launch (grid y).
//
// One workgroup of 8 waves owns a tile of 16 sequences (the M of v_mfma_f32_16x16x4_f32, exact fp32) and all 4h gate columns of
// its direction.  Tiles are independent: no workgroup waits for another, every loop's trip count comes from the clamped lengths.
// Sequence slot i of tile b is row order[16 b + i] of every tensor (order == NULL: the identity), so neither the sorted gather
// of the inputs nor the restoring gather of the outputs exists.
//
//   forward    h_{t-1} of the tile sits in LDS ([16][pitch], two buffers: one barrier per step), c_{t-1} in c_n, read back by the lane that wrote it.  Wave w owns
//              the hidden units 16 (w + 8 j) ... + 15 with their four gates: four accumulators over k = 0 .. h, W_hh streamed as
//              16 bytes per lane along k (row u of gate g is the B operand's column), so lane (u, q) feeds the four MFMAs of a
//              16-deep k step from ONE 16-byte load per gate and ONE 16-byte LDS read of h_{t-1}.  The lane that holds the
//              pre-activations of (sequence, unit) applies the gates, updates c and writes y, the saved tensors and h_t.
//   backward   dh_rec and dc of the tile stay in registers of the lane that owns (sequence, unit); per step and per chunk of
//              256 units the lanes form dgates ([16][4][256] in LDS and the caller's dgates), then every wave adds
//              dgates_chunk W_hh[chunk rows] to its 32-unit column groups, W_hh as stored as the k-major operand (8 bytes per lane).
// Every output element has one owner, nothing is accumulated in memory, no atomics: two runs are bit-identical.
//
// The GRU kernels are the LSTM's with three gates and another cell, written out a second time ON PURPOSE.  One
// kernel<Cell> pair for both was built and measured: with the same registers, occupancy and MFMA count its
// forward ran 2.2 - 2.7 % and the LSTM's backward 0.6 % slower, from a few dozen scalar instructions that moved, and its results
// kept the parent's bits only while each cell's per-element block stayed whole.  The host side below (rnn_check, rnn_launch) is
// shared.  Whoever merges the kernels compares the ISA with this file's first and measures against it.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include <math.h>

namespace gh {
namespace {

constexpr int RNN_THREADS = 512;
constexpr int RNN_WAVES = RNN_THREADS / 64;
constexpr int RNN_TILE = 16;                                 // sequences per workgroup
constexpr int RNN_MAX_H = 1024;
constexpr int RNN_MAX_T = 4096;
constexpr int RNN_GW = 32;                                   // units of a backward column group
constexpr int RNN_CHUNK = RNN_GW * RNN_WAVES;                // units whose dgates are staged at once (backward)
constexpr int RNN_BWD_NP = RNN_MAX_H / RNN_CHUNK;            // column groups per wave (backward)
constexpr int RNN_BWD_PF = 2;                                // k steps (of 4) whose operands are fetched ahead (backward)
constexpr int RNN_DG_PITCH = 4 * RNN_CHUNK + 4;              // [16][4][256] + 4: rows start 4 banks apart

__host__ __device__ inline int rnn_pitch(int h) { return pitch_kc(up16(h)); }      // LDS row pitch of the h_{t-1} / w_hh tiles

// never overflows: exp of a non-positive argument only.  Saturates to EXACT 0 / 1 (include/get_hip.h): towards -inf the value
// e s is e itself once s == 1, and fp32 denormals are kept on gfx950, so below ln(2^-126) = -87.34 it would be a denormal
// (3.8e-44 at -100); such a result is sent to 0.  Every normal result is the one the plain expression gives, bit for bit.
// The compare and select cost the forward 0.5 - 1.4 %; testing x instead of e measured the same.
__device__ __forceinline__ float rnn_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  const float s = 1.f / (1.f + e);
  return x >= 0.f ? s : (e < 1.17549435e-38f ? 0.f : e * s);
}

// s_len[i] = clamped length, s_row[i] = tensor row of sequence slot i of this tile (-1: no such sequence)
__device__ __forceinline__ int tile_setup(int* s_len, int* s_row, const int32_t* __restrict__ lens, const int32_t* __restrict__ order,
                                          int n, int tcap) {
  if (threadIdx.x < RNN_TILE) {
    const long long slot = (long long)blockIdx.x * RNN_TILE + threadIdx.x;
    int b = -1, len = 0;
    if (slot < n) {
      b = order ? order[slot] : (int)slot;
      if (b < 0 || b >= n) b = -1;
    }
    if (b >= 0) len = min(max(lens[b], 0), tcap);
    s_len[threadIdx.x] = len;
    s_row[threadIdx.x] = b;
  }
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < RNN_TILE; ++i) tmax = max(tmax, s_len[i]);
  return tmax;
}

// rows [t0, t1) x `cols` floats of a [..][t][ld] tensor, starting at `base` (row 0 of the sequence), set to zero
__device__ __forceinline__ void zero_rows(float* __restrict__ base, long long ld, int t0, int t1, int cols) {
  const long long count = (long long)(t1 - t0) * cols;
  for (long long idx = threadIdx.x; idx < count; idx += RNN_THREADS) {
    const long long r = idx / cols;
    base[(t0 + r) * ld + (idx - r * cols)] = 0.f;
  }
}

// W_hh[row][k .. k + 3], zeros beyond h
__device__ __forceinline__ float4 load_w4(const float* __restrict__ row, int k, int h, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k < h) {
    if (vec) {
      v = *reinterpret_cast<const float4*>(row + k);
    } else {
      v.x = row[k];
      if (k + 1 < h) v.y = row[k + 1];
      if (k + 2 < h) v.z = row[k + 2];
      if (k + 3 < h) v.w = row[k + 3];
    }
  }
  return v;
}

// W_hh[row][j], W_hh[row][j + 1], zeros beyond h
__device__ __forceinline__ float2 load_w2(const float* __restrict__ row, int j, int h, bool vec) {
  float2 v = make_float2(0.f, 0.f);
  if (j < h) {
    if (vec) {
      v = *reinterpret_cast<const float2*>(row + j);
    } else {
      v.x = row[j];
      if (j + 1 < h) v.y = row[j + 1];
    }
  }
  return v;
}

// operands of RNN_BWD_PF k steps of the backward product from k = k0 on: a[e] = dgates (LDS), b[e][q] = two columns of W_hh's row
// for each of the wave's column groups; zeros beyond the chunk's `ucp` rows (nothing is read there)
__device__ __forceinline__ void bwd_operands(float* a, float2 (*b)[RNN_BWD_NP], const float* ap, const float* __restrict__ wg, int k0,
                                             int ucp, int qd, int wave, int l15, int h, bool vec) {
#pragma unroll
  for (int e = 0; e < RNN_BWD_PF; ++e) {
    const int k = k0 + 4 * e;
    const bool kok = k + qd < ucp;
    a[e] = k < ucp ? ap[k] : 0.f;
    const float* wrow = wg + (size_t)(kok ? k : 0) * h;
#pragma unroll
    for (int q = 0; q < RNN_BWD_NP; ++q) {
      const int grp = q * RNN_WAVES + wave;
      b[e][q] = (kok && grp * RNN_GW < h) ? load_w2(wrow, grp * RNN_GW + 2 * l15, h, vec) : make_float2(0.f, 0.f);
    }
  }
}

// ============================================================================ forward
// grid (ceil(n / 16), dirs).  LDS: hs [2][16][pitch] | s_len [16] | s_row [16]
__global__ __launch_bounds__(RNN_THREADS) void
lstm_fwd_kernel(const float* __restrict__ gx0, const float* __restrict__ gx1, long long ldgx, const float* __restrict__ w0,
                const float* __restrict__ w1, const int32_t* __restrict__ lens, const int32_t* __restrict__ order, int n, int t_in, int t_out,
                int h, float* __restrict__ y, long long ldy, float* __restrict__ gates, float* __restrict__ cs, float* __restrict__ hprev,
                float* __restrict__ hn, float* __restrict__ cn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int pitch = rnn_pitch(h);
  float* hs = sm;
  int* s_len = reinterpret_cast<int*>(sm + 2 * RNN_TILE * pitch);
  int* s_row = s_len + RNN_TILE;
  const int dir = blockIdx.y;
  const float* __restrict__ gx = dir ? gx1 : gx0;
  const float* __restrict__ w = dir ? w1 : w0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const bool vec = (h & 3) == 0;
  const int h4 = 4 * h;
  const int kp = up16(h), nut = kp >> 4;

  const int tmax = tile_setup(s_len, s_row, lens, order, n, min(t_in, t_out));
  for (int idx = threadIdx.x; idx < 2 * RNN_TILE * pitch; idx += RNN_THREADS) hs[idx] = 0.f;
  // what no step writes: y beyond the length, h_prev of the first step and beyond the length, the state of an empty sequence
  for (int i = 0; i < RNN_TILE; ++i) {
    const int b = s_row[i], len = s_len[i];
    if (b < 0) continue;
    zero_rows(y + (size_t)b * t_out * ldy + (size_t)dir * h, ldy, len, t_out, h);
    const size_t sr = ((size_t)dir * n + b) * t_in;
    if (hprev) {
      zero_rows(hprev + sr * h, h, len, t_in, h);
      if (len > 0) zero_rows(hprev + sr * h, h, dir ? len - 1 : 0, dir ? len : 1, h);
    }
    // h_n / c_n carry the running state: every step rewrites them, the lane that owns (sequence, unit) reads its own c back
    for (int u = threadIdx.x; u < h; u += RNN_THREADS) hn[((size_t)dir * n + b) * h + u] = cn[((size_t)dir * n + b) * h + u] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < tmax; ++s) {
    const int t = dir ? tmax - 1 - s : s;
    const float* cur = hs + (s & 1) * RNN_TILE * pitch;
    float* nxt = hs + ((s & 1) ^ 1) * RNN_TILE * pitch;
    for (int ut = wave; ut < nut; ut += RNN_WAVES) {
      const int u = ut * 16 + l15;
      const bool uok = u < h;
      // the input projection's share of the four pre-activations, fetched ahead of the k loop
      float px[4][4], cp[4];
      bool act[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r, b = s_row[i];
        act[r] = b >= 0 && t < s_len[i] && uok;
        const float* p = gx + ((size_t)(act[r] ? b : 0) * t_in + (act[r] ? t : 0)) * ldgx + (uok ? u : 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) px[g][r] = act[r] ? p[g * h] : 0.f;
        cp[r] = act[r] ? cn[((size_t)dir * n + b) * h + u] : 0.f;
      }
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* wrow = w + (size_t)(uok ? u : 0) * h;
      const float* ap = cur + l15 * pitch + 4 * qd;
      // operands of the next 16-deep k step are requested before this step's MFMAs are issued: the loads' latency is
      // spent under 16 MFMAs instead of in front of them
      float4 a4 = *reinterpret_cast<const float4*>(ap);
      float4 b4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) b4[g] = uok ? load_w4(wrow + (size_t)g * h * h, 4 * qd, h, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k0 = 0; k0 < kp; k0 += 16) {
        const int kn = k0 + 16;
        float4 an = a4, bn[4];
        if (kn < kp) an = *reinterpret_cast<const float4*>(ap + kn);
#pragma unroll
        for (int g = 0; g < 4; ++g) bn[g] = uok ? load_w4(wrow + (size_t)g * h * h, kn + 4 * qd, h, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4[g].x, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4[g].y, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4[g].z, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4[g].w, acc[g], 0, 0, 0);
        a4 = an;
#pragma unroll
        for (int g = 0; g < 4; ++g) b4[g] = bn[g];
      }
      // C/D map: column (unit) = lane & 15, row (sequence) = 4 (lane >> 4) + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r;
        float hv = 0.f;
        if (act[r]) {
          const int b = s_row[i], len = s_len[i];
          const float ig = rnn_sigmoid(acc[0][r] + px[0][r]);
          const float fg = rnn_sigmoid(acc[1][r] + px[1][r]);
          const float gg = tanhf(acc[2][r] + px[2][r]);
          const float og = rnn_sigmoid(acc[3][r] + px[3][r]);
          const float cv = fg * cp[r] + ig * gg;
          hv = og * tanhf(cv);
          y[((size_t)b * t_out + t) * ldy + (size_t)dir * h + u] = hv;
          const size_t sq = (size_t)dir * n + b;
          if (gates) {
            const size_t sr = sq * t_in + t;
            float* gp = gates + sr * h4 + u;
            gp[0] = ig;
            gp[h] = fg;
            gp[2 * h] = gg;
            gp[3 * h] = og;
            cs[sr * h + u] = cv;
            if (dir ? t >= 1 : t + 1 < len) hprev[(dir ? sr - 1 : sr + 1) * h + u] = hv;
          }
          hn[sq * h + u] = hv;
          cn[sq * h + u] = cv;
        }
        if (uok) nxt[i * pitch + u] = hv;
      }
    }
    __syncthreads();
  }
}

// ============================================================================ backward
// grid (ceil(n / 16), dirs).  LDS: dgs [16][RNN_DG_PITCH] | s_len [16] | s_row [16]
__global__ __launch_bounds__(RNN_THREADS) void
lstm_bwd_kernel(const float* __restrict__ w0, const float* __restrict__ w1, const int32_t* __restrict__ lens,
                const int32_t* __restrict__ order, int n, int t_in, int t_out, int h, const float* __restrict__ gy, long long ldgy,
                const float* __restrict__ ghn, const float* __restrict__ gates, const float* __restrict__ cs, float* __restrict__ dgates) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dgs = sm;
  int* s_len = reinterpret_cast<int*>(sm + RNN_TILE * RNN_DG_PITCH);
  int* s_row = s_len + RNN_TILE;
  const int dir = blockIdx.y;
  const float* __restrict__ w = dir ? w1 : w0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const bool vec = (h & 1) == 0;
  const int h4 = 4 * h;

  const int tmax = tile_setup(s_len, s_row, lens, order, n, min(t_in, t_out));
  for (int idx = threadIdx.x; idx < RNN_TILE * RNN_DG_PITCH; idx += RNN_THREADS) dgs[idx] = 0.f;
  for (int i = 0; i < RNN_TILE; ++i) {
    const int b = s_row[i];
    if (b >= 0) zero_rows(dgates + ((size_t)dir * n + b) * t_in * h4, h4, s_len[i], t_in, h4);
  }
  __syncthreads();

  // lane (l15, qd) of wave w owns, for p < RNN_BWD_NP: sequences 4 qd + r, units 32 (8 p + w) + 2 l15 + cc
  f32x4 dh[RNN_BWD_NP][2], dc[RNN_BWD_NP][2];
#pragma unroll
  for (int p = 0; p < RNN_BWD_NP; ++p)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) dh[p][cc] = dc[p][cc] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < tmax; ++s) {
    const int t = dir ? s : tmax - 1 - s;
    f32x4 acc[RNN_BWD_NP][2];
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) acc[p][0] = acc[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) {
      const int u0 = p * RNN_CHUNK;                 // first unit of the chunk
      if (u0 >= h) continue;
      // ---- dgates of the chunk's units from dh = g_y + dh_rec (+ g_hn at the sequence's last forward step) and dc
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r, b = s_row[i], len = s_len[i];
        const bool live = b >= 0 && t < len;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const int uu = wave * RNN_GW + 2 * l15 + cc, u = u0 + uu;
          float di = 0.f, df = 0.f, dg = 0.f, d_og = 0.f, dcn = 0.f;
          if (live && u < h) {
            const size_t sq = (size_t)dir * n + b, sr = sq * t_in + t;
            const float* gp = gates + sr * h4 + u;
            const float ig = gp[0], fg = gp[h], gg = gp[2 * h], og = gp[3 * h];
            const float cv = cs[sr * h + u];
            const bool first = dir ? t == len - 1 : t == 0;      // the step that started from the zero state
            const float cprev = first ? 0.f : cs[(dir ? sr + 1 : sr - 1) * h + u];
            float dhv = dh[p][cc][r];
            if (gy) dhv += gy[((size_t)b * t_out + t) * ldgy + (size_t)dir * h + u];
            if (ghn && (dir ? t == 0 : t == len - 1)) dhv += ghn[sq * h + u];
            const float tc = tanhf(cv);
            const float dcv = dc[p][cc][r] + dhv * og * (1.f - tc * tc);
            di = dcv * gg * ig * (1.f - ig);
            df = dcv * cprev * fg * (1.f - fg);
            dg = dcv * ig * (1.f - gg * gg);
            d_og = dhv * tc * og * (1.f - og);
            dcn = dcv * fg;
            float* dp = dgates + sr * h4 + u;
            dp[0] = di;
            dp[h] = df;
            dp[2 * h] = dg;
            dp[3 * h] = d_og;
          }
          dc[p][cc][r] = dcn;
          float* ds = dgs + i * RNN_DG_PITCH + uu;
          ds[0] = di;
          ds[RNN_CHUNK] = df;
          ds[2 * RNN_CHUNK] = dg;
          ds[3 * RNN_CHUNK] = d_og;
        }
      }
      __syncthreads();
      // ---- dh_rec[.][units of this wave's groups] += dgates_chunk W_hh[rows of the chunk]
      const int ucp = min(RNN_CHUNK, h - u0);
      for (int g = 0; g < 4; ++g) {
        const float* ap = dgs + l15 * RNN_DG_PITCH + g * RNN_CHUNK + qd;
        const float* wg = w + ((size_t)g * h + u0 + qd) * h;
        // blocks of RNN_BWD_PF k steps; the next block's operands are requested before this block's MFMAs are issued
        float a[RNN_BWD_PF];
        float2 b2[RNN_BWD_PF][RNN_BWD_NP];
        bwd_operands(a, b2, ap, wg, 0, ucp, qd, wave, l15, h, vec);
        for (int k0 = 0; k0 < ucp; k0 += 4 * RNN_BWD_PF) {
          float an[RNN_BWD_PF];
          float2 bn[RNN_BWD_PF][RNN_BWD_NP];
          bwd_operands(an, bn, ap, wg, k0 + 4 * RNN_BWD_PF, ucp, qd, wave, l15, h, vec);
#pragma unroll
          for (int e = 0; e < RNN_BWD_PF; ++e)
#pragma unroll
            for (int q = 0; q < RNN_BWD_NP; ++q)
              if ((q * RNN_WAVES + wave) * RNN_GW < h) {
                acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b2[e][q].x, acc[q][0], 0, 0, 0);
                acc[q][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b2[e][q].y, acc[q][1], 0, 0, 0);
              }
#pragma unroll
          for (int e = 0; e < RNN_BWD_PF; ++e) {
            a[e] = an[e];
#pragma unroll
            for (int q = 0; q < RNN_BWD_NP; ++q) b2[e][q] = bn[e][q];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) {
      dh[p][0] = acc[p][0];
      dh[p][1] = acc[p][1];
    }
  }
}

// the limits of all four entries (the messages are those of both recurrences)
int rnn_check(const char* who, int n, int t_in, int t_out, int h, int dirs) {
  GH_REQUIRE(n >= 1 && t_in >= 1 && t_out >= 1 && h >= 1, "%s: empty problem (n=%d t_in=%d t_out=%d h=%d)", who, n, t_in, t_out, h);
  GH_REQUIRE(dirs == 1 || dirs == 2, "%s: dirs=%d is neither 1 nor 2", who, dirs);
  GH_REQUIRE(h <= RNN_MAX_H, "%s: h=%d exceeds the supported %d", who, h, RNN_MAX_H);
  GH_REQUIRE(t_in <= RNN_MAX_T, "%s: t_in=%d exceeds the supported %d", who, t_in, RNN_MAX_T);
  GH_REQUIRE(t_out <= RNN_MAX_T, "%s: t_out=%d exceeds the supported %d", who, t_out, RNN_MAX_T);
  return 0;
}

// ============================================================================ GRU
// torch.nn.GRU's cell, gate order r, z, n:  a = h_{t-1} W_hh^T + b_hh;  r = sigmoid(gx_r + a_r);  z = sigmoid(gx_z + a_z);
// n = tanh(gx_n + r a_n);  h_t = (1 - z) n + z h_{t-1}.  The layout is the LSTM's with three gates and no cell state: what differs
// is that b_hh is the kernel's (b_hn is multiplied by r), that the owning lane reads h_{t-1} once more for the convex update, and
// that the backward has two gradient rows per step (of gx and of a: they differ in the n third by the factor r).
constexpr int RNN_DA_PITCH = 3 * RNN_CHUNK + 4;              // [16][3][256] + 4: rows start 4 banks apart

// ---------------------------------------------------------------------------- forward
// grid (ceil(n / 16), dirs).  LDS: hs [2][16][pitch] | s_len [16] | s_row [16]
__global__ __launch_bounds__(RNN_THREADS) void
gru_fwd_kernel(const float* __restrict__ gx0, const float* __restrict__ gx1, long long ldgx, const float* __restrict__ w0,
               const float* __restrict__ w1, const float* __restrict__ bh0, const float* __restrict__ bh1, const int32_t* __restrict__ lens,
               const int32_t* __restrict__ order, int n, int t_in, int t_out, int h, float* __restrict__ y, long long ldy,
               float* __restrict__ gates, float* __restrict__ ans, float* __restrict__ hprev, float* __restrict__ hn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int pitch = rnn_pitch(h);
  float* hs = sm;
  int* s_len = reinterpret_cast<int*>(sm + 2 * RNN_TILE * pitch);
  int* s_row = s_len + RNN_TILE;
  const int dir = blockIdx.y;
  const float* __restrict__ gx = dir ? gx1 : gx0;
  const float* __restrict__ w = dir ? w1 : w0;
  const float* __restrict__ bh = dir ? bh1 : bh0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const bool vec = (h & 3) == 0;
  const int h3 = 3 * h;
  const int kp = up16(h), nut = kp >> 4;

  const int tmax = tile_setup(s_len, s_row, lens, order, n, min(t_in, t_out));
  for (int idx = threadIdx.x; idx < 2 * RNN_TILE * pitch; idx += RNN_THREADS) hs[idx] = 0.f;
  // what no step writes: y beyond the length, h_prev of the first step and beyond the length, the state of an empty sequence
  for (int i = 0; i < RNN_TILE; ++i) {
    const int b = s_row[i], len = s_len[i];
    if (b < 0) continue;
    zero_rows(y + (size_t)b * t_out * ldy + (size_t)dir * h, ldy, len, t_out, h);
    const size_t sr = ((size_t)dir * n + b) * t_in;
    if (hprev) {
      zero_rows(hprev + sr * h, h, len, t_in, h);
      if (len > 0) zero_rows(hprev + sr * h, h, dir ? len - 1 : 0, dir ? len : 1, h);
    }
    for (int u = threadIdx.x; u < h; u += RNN_THREADS) hn[((size_t)dir * n + b) * h + u] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < tmax; ++s) {
    const int t = dir ? tmax - 1 - s : s;
    const float* cur = hs + (s & 1) * RNN_TILE * pitch;
    float* nxt = hs + ((s & 1) ^ 1) * RNN_TILE * pitch;
    for (int ut = wave; ut < nut; ut += RNN_WAVES) {
      const int u = ut * 16 + l15;
      const bool uok = u < h;
      // the input projection's share of the three pre-activations and the unit's recurrent biases, fetched ahead of the k loop
      float px[3][4], bu[3];
      bool act[4];
#pragma unroll
      for (int g = 0; g < 3; ++g) bu[g] = uok ? bh[g * h + u] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r, b = s_row[i];
        act[r] = b >= 0 && t < s_len[i] && uok;
        const float* p = gx + ((size_t)(act[r] ? b : 0) * t_in + (act[r] ? t : 0)) * ldgx + (uok ? u : 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) px[g][r] = act[r] ? p[g * h] : 0.f;
      }
      f32x4 acc[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* wrow = w + (size_t)(uok ? u : 0) * h;
      const float* ap = cur + l15 * pitch + 4 * qd;
      // operands of the next 16-deep k step are requested before this step's MFMAs are issued
      float4 a4 = *reinterpret_cast<const float4*>(ap);
      float4 b4[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) b4[g] = uok ? load_w4(wrow + (size_t)g * h * h, 4 * qd, h, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k0 = 0; k0 < kp; k0 += 16) {
        const int kn = k0 + 16;
        float4 an = a4, bn[3];
        if (kn < kp) an = *reinterpret_cast<const float4*>(ap + kn);
#pragma unroll
        for (int g = 0; g < 3; ++g) bn[g] = uok ? load_w4(wrow + (size_t)g * h * h, kn + 4 * qd, h, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4[g].x, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4[g].y, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4[g].z, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4[g].w, acc[g], 0, 0, 0);
        a4 = an;
#pragma unroll
        for (int g = 0; g < 3; ++g) b4[g] = bn[g];
      }
      // C/D map: column (unit) = lane & 15, row (sequence) = 4 (lane >> 4) + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r;
        float hv = 0.f;
        if (act[r]) {
          const int b = s_row[i], len = s_len[i];
          const float hp = cur[i * pitch + u];              // h_{t-1}, from the buffer the A operand was read from
          const float av = acc[2][r] + bu[2];
          const float rg = rnn_sigmoid(px[0][r] + (acc[0][r] + bu[0]));
          const float zg = rnn_sigmoid(px[1][r] + (acc[1][r] + bu[1]));
          const float ng = tanhf(px[2][r] + rg * av);
          hv = (1.f - zg) * ng + zg * hp;
          y[((size_t)b * t_out + t) * ldy + (size_t)dir * h + u] = hv;
          const size_t sq = (size_t)dir * n + b;
          if (gates) {
            const size_t sr = sq * t_in + t;
            float* gp = gates + sr * h3 + u;
            gp[0] = rg;
            gp[h] = zg;
            gp[2 * h] = ng;
            ans[sr * h + u] = av;
            if (dir ? t >= 1 : t + 1 < len) hprev[(dir ? sr - 1 : sr + 1) * h + u] = hv;
          }
          hn[sq * h + u] = hv;
        }
        if (uok) nxt[i * pitch + u] = hv;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------- backward
// grid (ceil(n / 16), dirs).  LDS: das [16][RNN_DA_PITCH] | s_len [16] | s_row [16]
__global__ __launch_bounds__(RNN_THREADS) void
gru_bwd_kernel(const float* __restrict__ w0, const float* __restrict__ w1, const int32_t* __restrict__ lens,
               const int32_t* __restrict__ order, int n, int t_in, int t_out, int h, const float* __restrict__ gy, long long ldgy,
               const float* __restrict__ ghn, const float* __restrict__ gates, const float* __restrict__ ans,
               const float* __restrict__ hprev, float* __restrict__ dgx, float* __restrict__ da) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* das = sm;
  int* s_len = reinterpret_cast<int*>(sm + RNN_TILE * RNN_DA_PITCH);
  int* s_row = s_len + RNN_TILE;
  const int dir = blockIdx.y;
  const float* __restrict__ w = dir ? w1 : w0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
  const bool vec = (h & 1) == 0;
  const int h3 = 3 * h;

  const int tmax = tile_setup(s_len, s_row, lens, order, n, min(t_in, t_out));
  for (int idx = threadIdx.x; idx < RNN_TILE * RNN_DA_PITCH; idx += RNN_THREADS) das[idx] = 0.f;
  for (int i = 0; i < RNN_TILE; ++i) {
    const int b = s_row[i];
    if (b < 0) continue;
    zero_rows(dgx + ((size_t)dir * n + b) * t_in * h3, h3, s_len[i], t_in, h3);
    zero_rows(da + ((size_t)dir * n + b) * t_in * h3, h3, s_len[i], t_in, h3);
  }
  __syncthreads();

  // lane (l15, qd) of wave w owns, for p < RNN_BWD_NP: sequences 4 qd + r, units 32 (8 p + w) + 2 l15 + cc
  f32x4 dh[RNN_BWD_NP][2];
#pragma unroll
  for (int p = 0; p < RNN_BWD_NP; ++p) dh[p][0] = dh[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < tmax; ++s) {
    const int t = dir ? s : tmax - 1 - s;
    // the next step's dh: the direct part dh z is added by the owning lane when it forms its chunk's gradients, the product
    // [dr_pre, dz_pre, da_n] W_hh by the MFMAs of every chunk
    f32x4 acc[RNN_BWD_NP][2];
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) acc[p][0] = acc[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) {
      const int u0 = p * RNN_CHUNK;                 // first unit of the chunk
      if (u0 >= h) continue;
      // ---- both gradient rows of the chunk's units from dh = g_y + dh_carry (+ g_hn at the sequence's last forward step)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * qd + r, b = s_row[i], len = s_len[i];
        const bool live = b >= 0 && t < len;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const int uu = wave * RNN_GW + 2 * l15 + cc, u = u0 + uu;
          float dr = 0.f, dz = 0.f, dan = 0.f;
          if (live && u < h) {
            const size_t sq = (size_t)dir * n + b, sr = sq * t_in + t;
            const float* gp = gates + sr * h3 + u;
            const float rg = gp[0], zg = gp[h], ng = gp[2 * h];
            const float av = ans[sr * h + u], hp = hprev[sr * h + u];
            float dhv = dh[p][cc][r];
            if (gy) dhv += gy[((size_t)b * t_out + t) * ldgy + (size_t)dir * h + u];
            if (ghn && (dir ? t == 0 : t == len - 1)) dhv += ghn[sq * h + u];
            const float dnp = dhv * (1.f - zg) * (1.f - ng * ng);
            dz = dhv * (hp - ng) * zg * (1.f - zg);
            dr = dnp * av * rg * (1.f - rg);
            dan = dnp * rg;
            acc[p][cc][r] += dhv * zg;
            float* xp = dgx + sr * h3 + u;
            xp[0] = dr;
            xp[h] = dz;
            xp[2 * h] = dnp;
            float* rp = da + sr * h3 + u;
            rp[0] = dr;
            rp[h] = dz;
            rp[2 * h] = dan;
          }
          float* ds = das + i * RNN_DA_PITCH + uu;
          ds[0] = dr;
          ds[RNN_CHUNK] = dz;
          ds[2 * RNN_CHUNK] = dan;
        }
      }
      __syncthreads();
      // ---- dh_carry[.][units of this wave's groups] += da_chunk W_hh[rows of the chunk]
      const int ucp = min(RNN_CHUNK, h - u0);
      for (int g = 0; g < 3; ++g) {
        const float* ap = das + l15 * RNN_DA_PITCH + g * RNN_CHUNK + qd;
        const float* wg = w + ((size_t)g * h + u0 + qd) * h;
        // blocks of RNN_BWD_PF k steps; the next block's operands are requested before this block's MFMAs are issued
        float a[RNN_BWD_PF];
        float2 b2[RNN_BWD_PF][RNN_BWD_NP];
        bwd_operands(a, b2, ap, wg, 0, ucp, qd, wave, l15, h, vec);
        for (int k0 = 0; k0 < ucp; k0 += 4 * RNN_BWD_PF) {
          float an[RNN_BWD_PF];
          float2 bn[RNN_BWD_PF][RNN_BWD_NP];
          bwd_operands(an, bn, ap, wg, k0 + 4 * RNN_BWD_PF, ucp, qd, wave, l15, h, vec);
#pragma unroll
          for (int e = 0; e < RNN_BWD_PF; ++e)
#pragma unroll
            for (int q = 0; q < RNN_BWD_NP; ++q)
              if ((q * RNN_WAVES + wave) * RNN_GW < h) {
                acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b2[e][q].x, acc[q][0], 0, 0, 0);
                acc[q][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b2[e][q].y, acc[q][1], 0, 0, 0);
              }
#pragma unroll
          for (int e = 0; e < RNN_BWD_PF; ++e) {
            a[e] = an[e];
#pragma unroll
            for (int q = 0; q < RNN_BWD_NP; ++q) b2[e][q] = bn[e][q];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < RNN_BWD_NP; ++p) {
      dh[p][0] = acc[p][0];
      dh[p][1] = acc[p][1];
    }
  }
}

// What the four entries do after their own checks: the w_hh alignment (last of the checks, as it always was), then one
// workgroup per tile and direction with `lds_floats` of dynamic LDS plus the s_len / s_row tail.
template <class K, class... A>
int rnn_launch(K kernel, const char* who, const float* w_hh0, const float* w_hh1, size_t lds_floats, int n, int dirs,
               gh_stream_t stream, A... args) {
  GH_REQUIRE(aligned16(w_hh0) && aligned16(w_hh1), "%s: w_hh must be 16-byte aligned", who);
  const size_t lds = (lds_floats + 2 * RNN_TILE) * sizeof(float);
  if (int rc = lds_opt_in((const void*)kernel, lds, who)) return rc;
  hipLaunchKernelGGL(kernel, dim3((n + RNN_TILE - 1) / RNN_TILE, dirs), dim3(RNN_THREADS), lds, (hipStream_t)stream, args...);
  GH_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_lstm_seq_fwd(const float* gx0, const float* gx1, int ldgx, const float* w_hh0, const float* w_hh1, const int32_t* lens,
                               const int32_t* order, int n, int t_in, int t_out, int h, int dirs, float* y, int ldy, float* gates,
                               float* c, float* h_prev, float* h_n, float* c_n, gh_stream_t stream) {
  if (int rc = rnn_check("lstm_seq_fwd", n, t_in, t_out, h, dirs)) return rc;
  GH_REQUIRE(gx0 && w_hh0 && lens && y && h_n && c_n && (dirs == 1 || (gx1 && w_hh1)), "lstm_seq_fwd: NULL argument");
  GH_REQUIRE((gates != nullptr) == (c != nullptr) && (gates != nullptr) == (h_prev != nullptr),
             "lstm_seq_fwd: gates, c and h_prev are saved together or not at all");
  GH_REQUIRE(ldgx >= 4 * h && ldy >= dirs * h, "lstm_seq_fwd: a leading dimension is smaller than its row");
  return rnn_launch(lstm_fwd_kernel, "lstm_seq_fwd", w_hh0, w_hh1, (size_t)2 * RNN_TILE * rnn_pitch(h), n, dirs, stream, gx0, gx1,
                    (long long)ldgx, w_hh0, w_hh1, lens, order, n, t_in, t_out, h, y, (long long)ldy, gates, c, h_prev, h_n, c_n);
}

extern "C" int gh_lstm_seq_bwd(const float* w_hh0, const float* w_hh1, const int32_t* lens, const int32_t* order, int n, int t_in,
                               int t_out, int h, int dirs, const float* g_y, int ldgy, const float* g_hn, const float* gates,
                               const float* c, float* dgates, gh_stream_t stream) {
  if (int rc = rnn_check("lstm_seq_bwd", n, t_in, t_out, h, dirs)) return rc;
  GH_REQUIRE(w_hh0 && lens && gates && c && dgates && (dirs == 1 || w_hh1), "lstm_seq_bwd: NULL argument");
  GH_REQUIRE(!g_y || ldgy >= dirs * h, "lstm_seq_bwd: ldgy is smaller than dirs * h");
  return rnn_launch(lstm_bwd_kernel, "lstm_seq_bwd", w_hh0, w_hh1, (size_t)RNN_TILE * RNN_DG_PITCH, n, dirs, stream, w_hh0, w_hh1, lens,
                    order, n, t_in, t_out, h, g_y, (long long)ldgy, g_hn, gates, c, dgates);
}

extern "C" int gh_gru_seq_fwd(const float* gx0, const float* gx1, int ldgx, const float* w_hh0, const float* w_hh1, const float* b_hh0,
                              const float* b_hh1, const int32_t* lens, const int32_t* order, int n, int t_in, int t_out, int h, int dirs,
                              float* y, int ldy, float* gates, float* an, float* h_prev, float* h_n, gh_stream_t stream) {
  if (int rc = rnn_check("gru_seq_fwd", n, t_in, t_out, h, dirs)) return rc;
  GH_REQUIRE(gx0 && w_hh0 && b_hh0 && lens && y && h_n && (dirs == 1 || (gx1 && w_hh1 && b_hh1)), "gru_seq_fwd: NULL argument");
  GH_REQUIRE((gates != nullptr) == (an != nullptr) && (gates != nullptr) == (h_prev != nullptr),
             "gru_seq_fwd: gates, an and h_prev are saved together or not at all");
  GH_REQUIRE(ldgx >= 3 * h && ldy >= dirs * h, "gru_seq_fwd: a leading dimension is smaller than its row");
  return rnn_launch(gru_fwd_kernel, "gru_seq_fwd", w_hh0, w_hh1, (size_t)2 * RNN_TILE * rnn_pitch(h), n, dirs, stream, gx0, gx1,
                    (long long)ldgx, w_hh0, w_hh1, b_hh0, b_hh1, lens, order, n, t_in, t_out, h, y, (long long)ldy, gates, an, h_prev, h_n);
}

extern "C" int gh_gru_seq_bwd(const float* w_hh0, const float* w_hh1, const int32_t* lens, const int32_t* order, int n, int t_in,
                              int t_out, int h, int dirs, const float* g_y, int ldgy, const float* g_hn, const float* gates,
                              const float* an, const float* h_prev, float* dgx, float* da, gh_stream_t stream) {
  if (int rc = rnn_check("gru_seq_bwd", n, t_in, t_out, h, dirs)) return rc;
  GH_REQUIRE(w_hh0 && lens && gates && an && h_prev && dgx && da && (dirs == 1 || w_hh1), "gru_seq_bwd: NULL argument");
  GH_REQUIRE(!g_y || ldgy >= dirs * h, "gru_seq_bwd: ldgy is smaller than dirs * h");
  return rnn_launch(gru_bwd_kernel, "gru_seq_bwd", w_hh0, w_hh1, (size_t)RNN_TILE * RNN_DA_PITCH, n, dirs, stream, w_hh0, w_hh1, lens,
                    order, n, t_in, t_out, h, g_y, (long long)ldgy, g_hn, gates, an, h_prev, dgx, da);
}
