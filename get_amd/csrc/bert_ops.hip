// The BERT encoder of pytorch_transformers/modeling_bert.py (BertEmbeddings :142-171, BertSelfAttention :174-231, the erf-GELU
// :120-126 of BertIntermediate, the tanh of BertPooler :362-375):
//   gh_bert_attention_*   P = softmax(scale q_h k_h^T + bias), out_h = (P . keep / (1 - p)) v_h per head, the probabilities never
//                         in HBM: the forward saves lse = max + log(sum) per query row, the backward recomputes the score tiles
//   gh_act_*              erf-GELU and tanh, elementwise
//   gh_bert_embed_fwd     word[ids] + pos[pos_ids] + type[type_ids] and its LayerNorm in one pass
// The heads are column slices of the projection GEMMs' outputs, read where they lie ([b][l][heads * dh] with a leading
// dimension, so q, k and v may be the three column blocks of one [rows][3 H] buffer).
//
// The attention keeps the tiling of mha_ops.hip and runs every product on the exact-fp32 MFMA through score_tile.hip.h:
//   forward            one workgroup per (batch, head, 16-query tile): S = Q K^T into an LDS tile [16][lk] over key chunks, the
//                      row softmax of scale S + bias (running maximum subtracted), lse written, the dropout mask applied to
//                      the tile, out = tile V over key chunks with the accumulators in registers.
//   backward, queries  same tiling: delta = rowsum(gO . out) (written for the key-tiled kernel), dP = gO V^T into the tile, then
//                      per key chunk S = Q K^T into a small second tile and the tile becomes scale dS, dS = P (keep / (1 - p) dP
//                      - delta) with P = exp(scale S + bias - lse); dq = tile K.
//   backward, keys     one workgroup per (batch, head, 16-key slab) walks the query chunks: the transposed slabs K Q^T and V gO^T
//                      [16][chunk] become scale dS^T and (P . keep / (1 - p))^T in place; dk = scale dS^T Q, dv = P^T gO.
// The staged Q and gO chunks of the key-tiled kernel serve both as the KC operand of the slab products and as the right operand
// of the two accumulations (one image, KC pitch).  Dropout is the stateless rule of device_utils.h over the element index
// ((batch * heads + head) * lq + i) * lk + j; drop_p == 0 instantiates kernels without a hash.
// Every output element has one owner, nothing is accumulated in memory, no floating-point atomics: two runs are bit-identical.
#include "../../include/get_hip.h"
#include "common.h"
#include "device_utils.h"
#include "score_tile.hip.h"
#include <math.h>

namespace gh {
namespace {

constexpr int BA_THREADS = TILE_THREADS;
constexpr int BA_WAVES = TILE_WAVES;
constexpr int BA_MAX_LQ = 1024;
constexpr int BA_MAX_LK = 1024;          // one 16-row score tile [16][lk] in LDS (64 KB at the limit)
constexpr int BA_MAX_D = 512;            // 32 column tiles of 16: 8 accumulators per wave
constexpr int BA_MAX_HEADS = 16;
constexpr int BA_NT = BA_MAX_D / 16 / BA_WAVES;        // column tiles per wave
constexpr int BA_CHUNK = 9216;           // floats of one staged operand chunk (36 KB), as mha_ops.hip
constexpr int BA_BWD_KC = 64;            // key rows per recomputed score chunk of the query-tiled backward (the second tile [16][68])
constexpr int LN_MAX_D = 2048;           // gh_add_layernorm_bwd, which the embedding's backward runs, takes no more

// forward and query-tiled backward: xs [16][pa] | ss [16][ps] | (backward: s2 [16][p2]) | chunk
__host__ __device__ inline TilePlan att_plan(int lk, int dh) { return tile_plan<BA_MAX_D, BA_CHUNK>(lk, dh); }
__host__ __device__ inline int fwd_lds_floats(const TilePlan& p) { return 16 * p.pa + 16 * p.ps + p.chunk; }
__host__ __device__ inline int bwd_kc(const TilePlan& p) { return imin(p.kc1, BA_BWD_KC); }
__host__ __device__ inline int bwd_q_lds_floats(const TilePlan& p) { return 16 * p.pa + 16 * p.ps + 16 * pitch_kc(bwd_kc(p)) + p.chunk; }

// key-tiled backward: ks [16][pq] | vs [16][pq] | qi [qc][pq] | gi [qc][pq] | st [16][pst] | pt [16][pst]
struct KeyPlan { int pq, qc, pst; };
__host__ __device__ inline KeyPlan key_plan(int lq, int dh) {
  KeyPlan p;
  p.pq = pitch_kc(up16(dh));
  p.qc = chunk_rows(lq, 2 * p.pq + 32, BA_CHUNK);
  p.pst = pitch_kc(p.qc);
  return p;
}
__host__ __device__ inline int key_lds_floats(const KeyPlan& p) { return 32 * p.pq + 2 * p.qc * p.pq + 32 * p.pst; }

// rows row0 + 4 qd + r < rows, columns ct * 16 + l15 < cols of a [..][ld] global tensor
__device__ __forceinline__ void store_acc(float* __restrict__ dst, long long ld, int rows, int cols, const f32x4* acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, qd = lane >> 4;
#pragma unroll
  for (int t = 0; t < BA_NT; ++t) {
    const int c = (wave + BA_WAVES * t) * 16 + l15;
    if (c < cols) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * qd + r < rows) dst[(size_t)(4 * qd + r) * ld + c] = acc[t][r];
    }
  }
}

// scale s + bias with the reference's two roundings (scores / sqrt(dh), then + mask: modeling_bert.py:209-211), never fused:
// next to a bias of -10000 the sum lies on a grid of 2^-10, and one rounding instead of two lands on another grid point
__device__ __forceinline__ float biased(float s, float scale, float bias) { return __fadd_rn(__fmul_rn(s, scale), bias); }

// ============================================================================ forward
// grid (b * ceil(lq / 16), heads).  LDS: qs [16][pa] | ss [16][ps] | chunk
template <bool DROP>
__global__ __launch_bounds__(BA_THREADS) void
bert_att_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
                    long long ldv, const float* __restrict__ bias, int lq, int lk, int dh, float scale, unsigned seed, unsigned thresh,
                    float keep_scale, float* __restrict__ out, long long ldo, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = att_plan(lk, dh);
  float* qs = sm;
  float* ss = qs + 16 * P.pa;
  float* ch = ss + 16 * P.ps;
  const int nqt = (lq + 15) >> 4, heads = gridDim.y;
  const int bi = blockIdx.x / nqt, q0 = (blockIdx.x - bi * nqt) << 4, h = blockIdx.y;
  const int nq = min(16, lq - q0);

  stage(qs, P.pa, 16, up4(dh), q + ((size_t)bi * lq + q0) * ldq + (size_t)h * dh, ldq, nq, dh);
  scores_block(qs, P.pa, ch, P.pk, P.kc1, k + (size_t)bi * lk * ldk + (size_t)h * dh, ldk, lk, 0, dh, ss, P.ps, false);
  __syncthreads();
  {      // softmax: 16 lanes per row; the rows beyond nq hold zero scores and are computed along (nothing of them is stored)
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const float* brow = bias ? bias + (size_t)bi * lk : nullptr;
    float* srow = ss + row * P.ps;
    float mx = -INFINITY;
    for (int c = sub; c < lk; c += 16) {
      const float s = biased(srow[c], scale, brow ? brow[c] : 0.f);
      srow[c] = s;
      mx = fmaxf(mx, s);
    }
    mx = sub16_max(mx);
    float sum = 0.f;
    for (int c = sub; c < lk; c += 16) {
      const float e = expf(srow[c] - mx);
      srow[c] = e;
      sum += e;
    }
    sum = sub16_sum(sum);
    const float inv = 1.f / sum;
    const size_t rowi = ((size_t)bi * heads + h) * lq + q0 + row;
    if (sub == 0 && row < nq) lse[rowi] = mx + logf(sum);
    const unsigned idx0 = (unsigned)rowi * (unsigned)lk;      // (32 bits by the entry's guard)
    const int lkp = up16(lk);
    for (int c = sub; c < lkp; c += 16) {
      float w = 0.f;
      if (c < lk) {
        w = srow[c] * inv;
        if (DROP) w = drop_hash(seed, idx0 + (unsigned)c) >= thresh ? w * keep_scale : 0.f;
      }
      srow[c] = w;
    }
  }

  f32x4 acc[BA_NT];
#pragma unroll
  for (int t = 0; t < BA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  weighted_block<BA_NT>(ss, P.ps, ch, P.pv, P.kc2, v + (size_t)bi * lk * ldv + (size_t)h * dh, ldv, lk, 0, dh, acc);
  store_acc(out + ((size_t)bi * lq + q0) * ldo + (size_t)h * dh, ldo, nq, dh, acc);
}

// ============================================================================ backward, query-tiled: delta and dq
// grid (b * ceil(lq / 16), heads).  LDS: xs [16][pa] | ss [16][ps] | s2 [16][p2] | chunk
template <bool DROP>
__global__ __launch_bounds__(BA_THREADS) void
bert_att_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
                      long long ldv, const float* __restrict__ bias, const float* __restrict__ out, long long ldo,
                      const float* __restrict__ lse, const float* __restrict__ g_out, long long ldgo, int lq, int lk, int dh,
                      float scale, unsigned seed, unsigned thresh, float keep_scale, float* __restrict__ delta,
                      float* __restrict__ dq, long long lddq) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TilePlan P = att_plan(lk, dh);
  const int kc = bwd_kc(P), p2 = pitch_kc(kc);
  float* xs = sm;
  float* ss = xs + 16 * P.pa;
  float* s2 = ss + 16 * P.ps;
  float* ch = s2 + 16 * p2;
  const int nqt = (lq + 15) >> 4, heads = gridDim.y;
  const int bi = blockIdx.x / nqt, q0 = (blockIdx.x - bi * nqt) << 4, h = blockIdx.y;
  const int nq = min(16, lq - q0);
  const int dh4 = up4(dh);
  const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;       // 16 lanes per query row in the elementwise passes
  const bool live = row < nq;
  const size_t rowi = ((size_t)bi * heads + h) * lq + q0 + (live ? row : 0);

  stage(xs, P.pa, 16, dh4, g_out + ((size_t)bi * lq + q0) * ldgo + (size_t)h * dh, ldgo, nq, dh);
  __syncthreads();
  float dl = 0.f;
  if (live) {      // delta = rowsum(gO . out) = rowsum(P . keep / (1 - p) . dP)
    const float* orow = out + ((size_t)bi * lq + q0 + row) * ldo + (size_t)h * dh;
    for (int c = sub; c < dh; c += 16) dl = fmaf(xs[row * P.pa + c], orow[c], dl);
  }
  dl = sub16_sum(dl);
  if (live && sub == 0) delta[rowi] = dl;
  const float lrow = live ? lse[rowi] : 0.f;
  // dP = gO V^T
  scores_block(xs, P.pa, ch, P.pk, P.kc1, v + (size_t)bi * lk * ldv + (size_t)h * dh, ldv, lk, 0, dh, ss, P.ps, false);
  __syncthreads();
  stage(xs, P.pa, 16, dh4, q + ((size_t)bi * lq + q0) * ldq + (size_t)h * dh, ldq, nq, dh);
  const float* brow = bias ? bias + (size_t)bi * lk : nullptr;
  const unsigned idx0 = (unsigned)rowi * (unsigned)lk;
  for (int key0 = 0; key0 < lk; key0 += kc) {      // S chunk = Q K^T, and the tile becomes scale dS
    const int nk = imin(kc, lk - key0), rp = up16(nk);
    __syncthreads();
    stage(ch, P.pk, rp, dh4, k + ((size_t)bi * lk + key0) * ldk + (size_t)h * dh, ldk, nk, dh);
    __syncthreads();
    mma_scores(xs, P.pa, ch, P.pk, rp, dh4, s2, p2, 0, false);
    __syncthreads();
    float* srow = ss + row * P.ps + key0;
    for (int c = sub; c < rp; c += 16) {
      float d = 0.f;
      if (live && c < nk) {
        const float p = expf(biased(s2[row * p2 + c], scale, brow ? brow[key0 + c] : 0.f) - lrow);
        float kf = 1.f;      // keep / (1 - p)
        if (DROP) kf = drop_hash(seed, idx0 + (unsigned)(key0 + c)) >= thresh ? keep_scale : 0.f;
        d = scale * p * (kf * srow[c] - dl);
      }
      srow[c] = d;
    }
  }

  f32x4 acc[BA_NT];
#pragma unroll
  for (int t = 0; t < BA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  weighted_block<BA_NT>(ss, P.ps, ch, P.pv, P.kc2, k + (size_t)bi * lk * ldk + (size_t)h * dh, ldk, lk, 0, dh, acc);      // dq = scale dS K
  store_acc(dq + ((size_t)bi * lq + q0) * lddq + (size_t)h * dh, lddq, nq, dh, acc);
}

// ============================================================================ backward, key-tiled: dk and dv
// grid (b * ceil(lk / 16), heads).  LDS: ks [16][pq] | vs [16][pq] | qi [qc][pq] | gi [qc][pq] | st [16][pst] | pt [16][pst]
template <bool DROP>
__global__ __launch_bounds__(BA_THREADS) void
bert_att_bwd_k_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ldq, long long ldk,
                      long long ldv, const float* __restrict__ bias, const float* __restrict__ lse, const float* __restrict__ delta,
                      const float* __restrict__ g_out, long long ldgo, int lq, int lk, int dh, float scale, unsigned seed,
                      unsigned thresh, float keep_scale, float* __restrict__ dkk, long long lddk, float* __restrict__ dvv,
                      long long lddv) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const KeyPlan P = key_plan(lq, dh);
  float* ks = sm;
  float* vs = ks + 16 * P.pq;
  float* qi = vs + 16 * P.pq;
  float* gi = qi + P.qc * P.pq;
  float* st = gi + P.qc * P.pq;
  float* pt = st + 16 * P.pst;
  const int nkt = (lk + 15) >> 4, heads = gridDim.y;
  const int bi = blockIdx.x / nkt, key0 = (blockIdx.x - bi * nkt) << 4, h = blockIdx.y;
  const int nk = min(16, lk - key0);
  const int dh4 = up4(dh), dh16 = up16(dh);
  const size_t row0 = ((size_t)bi * heads + h) * lq;

  stage(ks, P.pq, 16, dh4, k + ((size_t)bi * lk + key0) * ldk + (size_t)h * dh, ldk, nk, dh);
  stage(vs, P.pq, 16, dh4, v + ((size_t)bi * lk + key0) * ldv + (size_t)h * dh, ldv, nk, dh);
  f32x4 acck[BA_NT], accv[BA_NT];
#pragma unroll
  for (int t = 0; t < BA_NT; ++t) acck[t] = accv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nct = (dh + 15) >> 4;
  for (int r0 = 0; r0 < lq; r0 += P.qc) {
    const int nr = imin(P.qc, lq - r0), rp = up16(nr);
    __syncthreads();
    stage(qi, P.pq, rp, dh16, q + ((size_t)bi * lq + r0) * ldq + (size_t)h * dh, ldq, nr, dh);
    stage(gi, P.pq, rp, dh16, g_out + ((size_t)bi * lq + r0) * ldgo + (size_t)h * dh, ldgo, nr, dh);
    __syncthreads();
    mma_scores(ks, P.pq, qi, P.pq, rp, dh4, st, P.pst, 0, false);      // st[key][row] = S^T
    mma_scores(vs, P.pq, gi, P.pq, rp, dh4, pt, P.pst, 0, false);      // pt[key][row] = dP^T
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * rp; idx += BA_THREADS) {
      const int i = idx / rp, r = idx - i * rp;
      float d = 0.f, w = 0.f;
      if (i < nk && r < nr) {
        const size_t rowi = row0 + r0 + r;
        w = expf(biased(st[i * P.pst + r], scale, bias ? bias[(size_t)bi * lk + key0 + i] : 0.f) - lse[rowi]);
        float kf = 1.f;      // keep / (1 - p)
        if (DROP) kf = drop_hash(seed, (unsigned)rowi * (unsigned)lk + (unsigned)(key0 + i)) >= thresh ? keep_scale : 0.f;
        d = scale * w * (kf * pt[i * P.pst + r] - delta[rowi]);
        w *= kf;
      }
      st[i * P.pst + r] = d;
      pt[i * P.pst + r] = w;
    }
    __syncthreads();
    mma_acc<BA_NT>(st, P.pst, 1, qi, P.pq, rp, nct, acck);      // dk = scale dS^T Q
    mma_acc<BA_NT>(pt, P.pst, 1, gi, P.pq, rp, nct, accv);      // dv = (P . keep / (1 - p))^T gO
  }
  store_acc(dkk + ((size_t)bi * lk + key0) * lddk + (size_t)h * dh, lddk, nk, dh, acck);
  store_acc(dvv + ((size_t)bi * lk + key0) * lddv + (size_t)h * dh, lddv, nk, dh, accv);
}

// ============================================================================ activations
constexpr float INV_SQRT2 = 0.70710678118654752440f;
constexpr float INV_SQRT_2PI = 0.39894228040143267794f;

template <int MODE> __device__ __forceinline__ float act_f(float x) {
  if (MODE == GH_ACT_GELU) return x * 0.5f * (1.f + erff(x * INV_SQRT2));
  return tanhf(x);
}
// d act / dx at the saved pre-activation x
template <int MODE> __device__ __forceinline__ float act_d(float x) {
  if (MODE == GH_ACT_GELU) return 0.5f * (1.f + erff(x * INV_SQRT2)) + x * INV_SQRT_2PI * expf(-0.5f * x * x);
  const float t = tanhf(x);
  return 1.f - t * t;
}

// y = act(x) (g == NULL) or y = g act'(x); float4 body where `vec`, the last count % 4 elements (or all of them) one by one
template <int MODE, bool BWD>
__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ y,
                                                  long long count, int vec) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = vec ? count >> 2 : 0;
  for (long long i = t0; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i];
    float4 o;
    if (BWD) {
      const float4 gg = reinterpret_cast<const float4*>(g)[i];
      o = make_float4(gg.x * act_d<MODE>(a.x), gg.y * act_d<MODE>(a.y), gg.z * act_d<MODE>(a.z), gg.w * act_d<MODE>(a.w));
    } else {
      o = make_float4(act_f<MODE>(a.x), act_f<MODE>(a.y), act_f<MODE>(a.z), act_f<MODE>(a.w));
    }
    reinterpret_cast<float4*>(y)[i] = o;
  }
  for (long long i = 4 * n4 + t0; i < count; i += stride) y[i] = BWD ? g[i] * act_d<MODE>(x[i]) : act_f<MODE>(x[i]);
}

template <bool BWD> int launch_act(const char* who, const float* x, const float* g, float* y, int rows, int n, int mode, hipStream_t st) {
  GH_REQUIRE(rows >= 1 && n >= 1, "%s: empty problem (rows=%d n=%d)", who, rows, n);
  GH_REQUIRE(mode == GH_ACT_GELU || mode == GH_ACT_TANH, "%s: mode %d is neither GH_ACT_GELU nor GH_ACT_TANH", who, mode);
  GH_REQUIRE(x && y && (!BWD || g), "%s: NULL argument", who);
  const long long count = (long long)rows * n;
  const int vec = aligned16(x) && aligned16(y) && (!BWD || aligned16(g));
  const long long work = vec ? count / 4 + 3 : count, blocks = (work + 255) / 256;
  const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
  if (mode == GH_ACT_GELU) hipLaunchKernelGGL((act_kernel<GH_ACT_GELU, BWD>), grid, dim3(256), 0, st, x, g, y, count, vec);
  else hipLaunchKernelGGL((act_kernel<GH_ACT_TANH, BWD>), grid, dim3(256), 0, st, x, g, y, count, vec);
  GH_LAUNCH_CHECK();
  return 0;
}

// ============================================================================ embedding sum + LayerNorm
// one wave per row; grid-stride over the rows (add_ln_fwd_kernel of mha_ops.hip with the three table rows as its input)
__device__ __forceinline__ int clamp_id(int id, int n, int lane, unsigned int* clamped) {
  if (id >= 0 && id < n) return id;
  if (lane == 0) atomicAdd(clamped + 3, 1u);      // nn.Embedding raises there; counted, gh_clamp_events
  return id < 0 ? 0 : n - 1;
}

__global__ __launch_bounds__(BA_THREADS) void
bert_embed_fwd_kernel(const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                      const int32_t* __restrict__ ids, const int32_t* __restrict__ pos_ids, const int32_t* __restrict__ type_ids,
                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int rows, int l, int d, int vocab,
                      int npos, int ntype, float* __restrict__ sum, float* __restrict__ y, float* __restrict__ mean,
                      float* __restrict__ rstd, unsigned int* __restrict__ clamped) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * BA_WAVES + wave; r < rows; r += (long long)gridDim.x * BA_WAVES) {
    const float* wr = word + (size_t)clamp_id(ids[r], vocab, lane, clamped) * d;
    const float* pr = pos + (size_t)clamp_id(pos_ids ? pos_ids[r] : (int)(r % l), npos, lane, clamped) * d;
    const float* tr = type + (size_t)(type_ids ? clamp_id(type_ids[r], ntype, lane, clamped) : 0) * d;
    float* sr = sum + r * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float e = wr[c] + pr[c] + tr[c];      // (the reference's order: words + positions, then + token types, :168)
      sr[c] = e;
      s += e;
    }
    const float mu = wave_sum(s) / (float)d;
    float s2 = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float z = wr[c] + pr[c] + tr[c] - mu;
      s2 = fmaf(z, z, s2);
    }
    const float rs = 1.f / sqrtf(wave_sum(s2) / (float)d + eps);
    for (int c = lane; c < d; c += 64) {
      const float z = wr[c] + pr[c] + tr[c] - mu;
      y[r * d + c] = fmaf(z * rs, gamma[c], beta[c]);
    }
    if (lane == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
  }
}

unsigned drop_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

int att_check(const char* who, int b, int heads, int lq, int lk, int dh, float scale, float drop_p) {
  GH_REQUIRE(b >= 1 && heads >= 1 && lq >= 1 && lk >= 1 && dh >= 1, "%s: empty problem (b=%d heads=%d lq=%d lk=%d dh=%d)", who, b, heads,
             lq, lk, dh);
  GH_REQUIRE(heads <= BA_MAX_HEADS, "%s: heads=%d exceeds the supported %d", who, heads, BA_MAX_HEADS);
  GH_REQUIRE(lq <= BA_MAX_LQ, "%s: lq=%d exceeds the supported %d", who, lq, BA_MAX_LQ);
  GH_REQUIRE(lk <= BA_MAX_LK, "%s: lk=%d exceeds the supported %d", who, lk, BA_MAX_LK);
  GH_REQUIRE(dh <= BA_MAX_D, "%s: dh=%d exceeds the supported %d", who, dh, BA_MAX_D);
  GH_REQUIRE((long long)b * (((lq > lk ? lq : lk) + 15) / 16) <= 0x7fffffffLL, "%s: b=%d is too large", who, b);
  GH_REQUIRE(isfinite(scale), "%s: scale=%f is not finite", who, scale);
  GH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: dropout p=%f not in [0,1)", who, drop_p);
  GH_REQUIRE(drop_p <= 0.f || (long long)b * heads * lq * (long long)lk < (1LL << 32),
             "%s: b * heads * lq * lk = %lld elements exceed the dropout mask's 32-bit element index", who,
             (long long)b * heads * lq * (long long)lk);
  return 0;
}

template <bool DROP>
int launch_att_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* bias, const float* out, int ldo,
                   const float* lse, const float* g_out, int ldgo, int b, int heads, int lq, int lk, int dh, float scale, float drop_p,
                   uint32_t seed, float* delta, float* dq, int lddq, float* dkk, int lddk, float* dvv, int lddv, hipStream_t st) {
  const size_t lds_q = (size_t)bwd_q_lds_floats(att_plan(lk, dh)) * sizeof(float);
  const size_t lds_k = (size_t)key_lds_floats(key_plan(lq, dh)) * sizeof(float);
  if (int rc = lds_opt_in((const void*)bert_att_bwd_q_kernel<DROP>, lds_q, "bert_attention_bwd")) return rc;
  if (int rc = lds_opt_in((const void*)bert_att_bwd_k_kernel<DROP>, lds_k, "bert_attention_bwd")) return rc;
  const unsigned thresh = DROP ? drop_threshold(drop_p) : 0u;
  const float keep_scale = DROP ? 1.f / (1.f - drop_p) : 1.f;
  hipLaunchKernelGGL(bert_att_bwd_q_kernel<DROP>, dim3(b * ((lq + 15) / 16), heads), dim3(BA_THREADS), lds_q, st, q, k, v, (long long)ldq,
                     (long long)ldk, (long long)ldv, bias, out, (long long)ldo, lse, g_out, (long long)ldgo, lq, lk, dh, scale, seed,
                     thresh, keep_scale, delta, dq, (long long)lddq);
  hipLaunchKernelGGL(bert_att_bwd_k_kernel<DROP>, dim3(b * ((lk + 15) / 16), heads), dim3(BA_THREADS), lds_k, st, q, k, v, (long long)ldq,
                     (long long)ldk, (long long)ldv, bias, lse, delta, g_out, (long long)ldgo, lq, lk, dh, scale, seed, thresh,
                     keep_scale, dkk, (long long)lddk, dvv, (long long)lddv);
  GH_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" int gh_bert_attention_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* bias, int b,
                                     int heads, int lq, int lk, int dh, float scale, float drop_p, uint32_t seed, float* out, int ldo,
                                     float* lse, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = att_check("bert_attention_fwd", b, heads, lq, lk, dh, scale, drop_p)) return rc;
  GH_REQUIRE(q && k && v && out && lse, "bert_attention_fwd: NULL argument");
  GH_REQUIRE(ldq >= heads * dh && ldk >= heads * dh && ldv >= heads * dh && ldo >= heads * dh,
             "bert_attention_fwd: a leading dimension is smaller than heads * dh = %d", heads * dh);
  const size_t lds = (size_t)fwd_lds_floats(att_plan(lk, dh)) * sizeof(float);
  const dim3 grid(b * ((lq + 15) / 16), heads);
  if (drop_p > 0.f) {
    if (int rc = lds_opt_in((const void*)bert_att_fwd_kernel<true>, lds, "bert_attention_fwd")) return rc;
    hipLaunchKernelGGL(bert_att_fwd_kernel<true>, grid, dim3(BA_THREADS), lds, st, q, k, v, (long long)ldq, (long long)ldk, (long long)ldv,
                       bias, lq, lk, dh, scale, seed, drop_threshold(drop_p), 1.f / (1.f - drop_p), out, (long long)ldo, lse);
  } else {
    if (int rc = lds_opt_in((const void*)bert_att_fwd_kernel<false>, lds, "bert_attention_fwd")) return rc;
    hipLaunchKernelGGL(bert_att_fwd_kernel<false>, grid, dim3(BA_THREADS), lds, st, q, k, v, (long long)ldq, (long long)ldk,
                       (long long)ldv, bias, lq, lk, dh, scale, 0u, 0u, 1.f, out, (long long)ldo, lse);
  }
  GH_LAUNCH_CHECK();
  return 0;
}

extern "C" int gh_bert_attention_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* bias,
                                     const float* out, int ldo, const float* lse, const float* g_out, int ldgo, int b, int heads, int lq,
                                     int lk, int dh, float scale, float drop_p, uint32_t seed, float* delta, float* dq, int lddq,
                                     float* dkk, int lddk, float* dvv, int lddv, gh_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = att_check("bert_attention_bwd", b, heads, lq, lk, dh, scale, drop_p)) return rc;
  GH_REQUIRE(q && k && v && out && lse && g_out && delta && dq && dkk && dvv, "bert_attention_bwd: NULL argument");
  GH_REQUIRE(ldq >= heads * dh && ldk >= heads * dh && ldv >= heads * dh && ldo >= heads * dh && ldgo >= heads * dh && lddq >= heads * dh &&
                 lddk >= heads * dh && lddv >= heads * dh,
             "bert_attention_bwd: a leading dimension is smaller than heads * dh = %d", heads * dh);
  if (drop_p > 0.f)
    return launch_att_bwd<true>(q, k, v, ldq, ldk, ldv, bias, out, ldo, lse, g_out, ldgo, b, heads, lq, lk, dh, scale, drop_p, seed, delta,
                                dq, lddq, dkk, lddk, dvv, lddv, st);
  return launch_att_bwd<false>(q, k, v, ldq, ldk, ldv, bias, out, ldo, lse, g_out, ldgo, b, heads, lq, lk, dh, scale, 0.f, 0u, delta, dq,
                               lddq, dkk, lddk, dvv, lddv, st);
}

extern "C" int gh_act_fwd(const float* x, float* y, int rows, int n, int mode, gh_stream_t stream) {
  return launch_act<false>("act_fwd", x, nullptr, y, rows, n, mode, (hipStream_t)stream);
}

extern "C" int gh_act_bwd(const float* x, const float* g, float* dx, int rows, int n, int mode, gh_stream_t stream) {
  return launch_act<true>("act_bwd", x, g, dx, rows, n, mode, (hipStream_t)stream);
}

extern "C" int gh_bert_embed_fwd(const float* word, const float* pos, const float* type, const int32_t* ids, const int32_t* pos_ids,
                                 const int32_t* type_ids, const float* gamma, const float* beta, float eps, int rows, int l, int d,
                                 int vocab, int npos, int ntype, float* sum, float* y, float* mean, float* rstd, gh_stream_t stream) {
  GH_REQUIRE(rows >= 1 && l >= 1 && d >= 1 && vocab >= 1 && npos >= 1 && ntype >= 1,
             "bert_embed_fwd: bad sizes (rows=%d l=%d d=%d vocab=%d npos=%d ntype=%d)", rows, l, d, vocab, npos, ntype);
  GH_REQUIRE(d <= LN_MAX_D, "bert_embed_fwd: d=%d exceeds the supported %d", d, LN_MAX_D);
  GH_REQUIRE(word && pos && type && ids && gamma && beta && sum && y && mean && rstd, "bert_embed_fwd: NULL argument");
  unsigned int* cl = clamp_counter();
  GH_REQUIRE(cl, "bert_embed_fwd: cannot allocate the clamp counter");
  const int nwg = (rows + BA_WAVES - 1) / BA_WAVES < 4096 ? (rows + BA_WAVES - 1) / BA_WAVES : 4096;
  hipLaunchKernelGGL(bert_embed_fwd_kernel, dim3(nwg), dim3(BA_THREADS), 0, (hipStream_t)stream, word, pos, type, ids, pos_ids, type_ids,
                     gamma, beta, eps, rows, l, d, vocab, npos, ntype, sum, y, mean, rstd, cl);
  GH_LAUNCH_CHECK();
  return 0;
}
