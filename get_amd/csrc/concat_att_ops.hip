// The streaming kernels of the concat attention (two_branches_attention.py) around its GEMMs: masked softmax + weighted reduce
// forward, its per-pair and row-balanced backward, and the backward through the tanh layer (att_dpre), each with its launcher.
// dense_ops.hip's att_fwd_impl / att_bwd_impl chain them with the GEMMs.
#include "../../include/get_hip.h"
#include "device_utils.h"

namespace gh {

// ---------------------------------------------------------------------------- concat attention: masked softmax + weighted reduce
// bf16 storage mode (R16): `right` is the producing cell's bf16 output (four values per 8-byte load, widened at the point of use --
// the loads stay in flight as raw words), so that no fp32 copy of that output has to exist
template <bool R16> struct RightVec { typedef float4 T; };
template <> struct RightVec<true> { typedef uint2 T; };
__device__ __forceinline__ float4 right_widen(const float4 v) { return v; }
__device__ __forceinline__ float4 right_widen(const uint2 v) { return bf4_to_f4(v); }
// e [b][l][C] -> weights = softmax over l (two_branches_attention.py:142-146), attended[b][d][c] = sum_l right[b][l][d] w[l][c] (:147)
template <int CT, bool R16 = false>     // compile-time bound on the number of heads (accumulator registers); R16: right holds bf16
__global__ void __launch_bounds__(256, 4)
att_softmax_fwd_kernel(float* __restrict__ e, const float* __restrict__ mask, const float* __restrict__ right,
                       const int32_t* __restrict__ goff, int Lmax, int Dr, int C, float* __restrict__ weights,
                       float* __restrict__ attended, const float* __restrict__ e_parts, int n_parts, long long part_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* ws = reinterpret_cast<float*>(dsm);   // [Lmax][C]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // node-compact layout: pair b owns rows [goff[b], goff[b+1]) of e / mask / right / weights
  const int row0 = goff ? goff[b] : b * Lmax;
  const int L = goff ? goff[b + 1] - row0 : Lmax;
  const float* mb = mask + (size_t)row0;
  const int NT = blockDim.x, NWV = NT >> 6;
  // The right tile is what the kernel streams (L rows x Dr floats per pair): the first batch of this wave's rows is
  // requested BEFORE the softmax (its latency hides behind the exp / shuffle work), and every later batch before the
  // previous one is consumed -- RB rows = RB KB per wave in flight instead of the one-row-at-a-time walk that kept the
  // kernel latency-bound at 1.9 TB/s.
  // A workgroup takes 128 float4 columns (two per lane): at Dr = 300 that is the WHOLE row -- the 64-column slabs
  // left a second workgroup per pair reading 176-byte runs (11 float4) whose 128-byte lines the first one fetches too.
  // All 960 pairs of the bench shape should be resident at once (4 workgroups per CU -> <= 128 VGPRs), and a wave should
  // need as few memory round trips as possible for its ~16 rows: RB = 6 rows x 2 chunks in flight per trip, single
  // buffered (the math between two trips is far shorter than a round trip, so a second buffer only costs registers).
  constexpr int RB = CT <= 2 ? 8 : CT <= 5 ? 6 : 4, NCH = 2;   // (8 x 2 chunks + 40 accumulators spill at 128 VGPRs)
  const int D4 = Dr / 4;
  int dcl[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) dcl[h] = min(blockIdx.y * (64 * NCH) + lane + 64 * h, D4 - 1);
  typedef typename RightVec<R16>::T RV;
  const RV* rb = R16 ? reinterpret_cast<const RV*>(reinterpret_cast<const unsigned short*>(right) + (size_t)row0 * Dr)
                     : reinterpret_cast<const RV*>(right + (size_t)row0 * Dr);
  RV zero4;
  __builtin_memset(&zero4, 0, sizeof(RV));
  // (unconditional loads from clamped rows / columns: a `cond ? load : 0` select makes the compiler route the load
  // through a flat pointer to a zero in scratch; clamped duplicates are loaded twice and never consumed)
  RV rv[RB][NCH];
  if (L > 0) {
#pragma unroll
    for (int u = 0; u < RB; ++u)
#pragma unroll
      for (int h = 0; h < NCH; ++h) rv[u][h] = rb[(size_t)min(wave + u * NWV, L - 1) * D4 + dcl[h]];
  } else {
#pragma unroll
    for (int u = 0; u < RB; ++u)
#pragma unroll
      for (int h = 0; h < NCH; ++h) rv[u][h] = zero4;
  }
  // scores staged in LDS (read twice below).  n_parts > 0: the producing GEMM left one partial per column block of the hidden
  // layer (wide rows, h = 768): summed here in block order, and the sum is written back as the layer's `e` output
  float* eb = ws + (size_t)Lmax * C + (size_t)NWV * 64 * (4 * C + 1);      // [Lmax][C], behind the weights and the reduce partials
  for (int i = tid; i < L * C; i += NT) {
    float v;
    if (n_parts > 0) {
      v = 0.f;
      for (int p = 0; p < n_parts; ++p) v += e_parts[(size_t)p * part_stride + (size_t)row0 * C + i];
      if (blockIdx.y == 0) e[(size_t)row0 * C + i] = v;
    } else {
      v = e[(size_t)row0 * C + i];
    }
    eb[i] = v;
  }
  __syncthreads();
  for (int c = wave; c < C; c += NWV) {
    float mx = -INFINITY;
    for (int l = lane; l < L; l += 64)
      if (mb[l] != 0.f) mx = fmaxf(mx, eb[l * C + c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float p = (mb[l] != 0.f) ? expf(eb[l * C + c] - mx) : 0.f;
      ws[l * C + c] = p;
      sum += p;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;          // all-masked row: 0/0 = NaN, as the reference's softmax of -inf
    for (int l = lane; l < L; l += 64) ws[l * C + c] = (sum > 0.f) ? ws[l * C + c] * inv : NAN;
  }
  __syncthreads();
  if (blockIdx.y == 0)
    for (int i = tid; i < L * C; i += NT) weights[(size_t)row0 * C + i] = ws[i];
  // attended[d][c] = sum_l right[l][d] w[l][c]: the waves take every NWV-th row (16-byte coalesced reads), partial sums
  // meet in LDS, one column chunk after the other
  // [NWV][64 lanes][4 C + 1] floats.  The odd pitch keeps the 4 C partial stores of a wave conflict-free (at the pitch 4 C the
  // 64 lanes of a store sat 4 C floats apart: 32-way bank conflicts at C = 8, 4-way at C = 5 -- PMC on configs[4]:
  // SQ_LDS_BANK_CONFLICT 87 % of the kernel's LDS cycles) and the reduce below still reads consecutive words
  float* part = ws + Lmax * C;
  const int PP = 4 * C + 1;
  float acc[NCH][4][CT];
#pragma unroll
  for (int h = 0; h < NCH; ++h)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[h][k][c] = 0.f;
  for (int l0 = wave; l0 < L; l0 += RB * NWV) {
    if (l0 != wave) {
#pragma unroll
      for (int u = 0; u < RB; ++u)
#pragma unroll
        for (int h = 0; h < NCH; ++h) rv[u][h] = rb[(size_t)min(l0 + u * NWV, L - 1) * D4 + dcl[h]];
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int l = l0 + u * NWV;
      if (l < L) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) {
            const float w = ws[l * C + c];
#pragma unroll
            for (int h = 0; h < NCH; ++h) {
              const float4 r4 = right_widen(rv[u][h]);
              acc[h][0][c] += r4.x * w; acc[h][1][c] += r4.y * w; acc[h][2][c] += r4.z * w; acc[h][3][c] += r4.w * w;
            }
          }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    if (h > 0) __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) part[(wave * 64 + lane) * PP + k * C + c] = acc[h][k][c];
    __syncthreads();
    for (int i = tid; i < 64 * 4 * C; i += NT) {
      const int ln = i / (4 * C), rem = i % (4 * C);     // rem = k*C + c -> output offset within the float4 column group
      const int dd = (blockIdx.y * (64 * NCH) + 64 * h + ln) * 4 + rem / C;
      if (dd < Dr) {
        float v = 0.f;
        for (int w = 0; w < NWV; ++w) v += part[(w * 64 + ln) * PP + rem];
        if (L == 0) v = NAN;                      // no rows at all: the reference's softmax over an all -inf column
        attended[((size_t)b * Dr + dd) * C + rem % C] = v;
      }
    }
  }
}

int launch_att_softmax_fwd(float* e, const float* mask, const float* right, const int32_t* goff, int m_real,
                           int b, int l, int dr, int heads, float* weights, float* attended, hipStream_t s,
                           const float* e_parts, int n_parts, long long part_stride, const void* right16) {
  GH_REQUIRE(right || right16, "att_softmax_fwd: no right operand");
  if (right16) {
    GH_REQUIRE(dr % 4 == 0 && (reinterpret_cast<uintptr_t>(right16) & 7) == 0, "att_softmax_fwd: bf16 right rows must be 8-byte shaped (dr=%d)", dr);
    right = reinterpret_cast<const float*>(right16);
  }
  GH_REQUIRE(dr % 4 == 0 && (right16 || (reinterpret_cast<uintptr_t>(right) & 15) == 0), "att_softmax_fwd: right rows must be float4-shaped (dr=%d)", dr);
  const int nthr = 256;      // (8 waves per pair measured no faster: the kernel is not parallelism-bound)
  const size_t lds = ((size_t)2 * l * heads + (nthr / 64) * 64 * (4 * heads + 1)) * 4;
  GH_REQUIRE(lds <= 64 * 1024, "att_softmax_fwd: sequence %d x heads %d too large", l, heads);
  GH_REQUIRE(heads >= 1 && heads <= 8, "att_softmax_fwd: %d heads (1..8 supported)", heads);
  static const void* const fns[3][2] = {{(const void*)att_softmax_fwd_kernel<2>, (const void*)att_softmax_fwd_kernel<2, true>},
                                        {(const void*)att_softmax_fwd_kernel<5>, (const void*)att_softmax_fwd_kernel<5, true>},
                                        {(const void*)att_softmax_fwd_kernel<8>, (const void*)att_softmax_fwd_kernel<8, true>}};
  const void* fn = fns[heads <= 2 ? 0 : heads <= 5 ? 1 : 2][right16 ? 1 : 0];
  const int ptag = few_rows_tag(b, PROF_ATT_SOFTMAX_FWD);
  prof_begin(s, ptag);
  void* args[] = {(void*)&e, (void*)&mask, (void*)&right, (void*)&goff, (void*)&l, (void*)&dr, (void*)&heads, (void*)&weights,
                  (void*)&attended, (void*)&e_parts, (void*)&n_parts, (void*)&part_stride};
  (void)hipLaunchKernel(fn, dim3(b, (dr / 4 + 127) / 128), dim3(nthr), args, lds, s);
  const double rows = goff ? (double)m_real : (double)b * l;
  prof_end(ptag, (right16 ? 2.0 : 4.0) * rows * dr + 4.0 * (2.0 * rows * heads + rows + (double)b * dr * heads), s);
  GH_LAUNCH_CHECK();
  return 0;
}

// Sum over the 64 lanes of a wave on the VALU's DPP path (row shifts + row broadcasts, gfx9 wave64): six VALU
// instructions, no LDS crossbar traffic -- __shfl_xor compiles to ds_bpermute_b32 (an LDS instruction plus a wait per
// step), which made the five head reductions per row the largest cost of the word-level softmax backward.  The total
// lands in lane 63 (returned to every lane through readlane).
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));   // row_shr:1
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));   // row_shr:2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xe, true));   // row_shr:4, banks 1-3
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xc, true));   // row_shr:8, banks 2-3
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, true));   // row_bcast:15 -> rows 1, 3
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, true));   // row_bcast:31 -> rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// backward of the softmax/reduce: dw[l][c] = sum_d right[l][d] g_att[d][c] (+ g_w) ; de = w (dw - sum_l w dw) ;
// dright[l][d] = sum_c w[l][c] g_att[d][c]  (first contribution; the GEMM adds dpre W1r on top)
template <int CT>     // compile-time bound on the number of heads
__global__ void __launch_bounds__(512)
att_softmax_bwd_kernel(const float* __restrict__ right, const float* __restrict__ weights,
                       const float* __restrict__ g_att, const float* __restrict__ g_w,
                       const int32_t* __restrict__ goff, int Lmax, int Dr, int C,
                       float* __restrict__ de, float* __restrict__ dright) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* ga = reinterpret_cast<float*>(dsm);   // [C][Dr]: head-major, so a lane's four g values are one 16-byte read and
                                               // consecutive lanes hit consecutive banks ([Dr][C] was an 8-way conflict)
  float* ws = ga + (size_t)Dr * C;             // [Lmax][C]
  float* dw = ws + (size_t)Lmax * C;           // [Lmax][C]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = goff ? goff[b] : b * Lmax;
  const int L = goff ? goff[b + 1] - row0 : Lmax;
  const int NT = blockDim.x, NWV = NT >> 6;
  const int D4 = Dr / 4;
  constexpr int NCH = 2;                         // float4 columns per lane on the register path (Dr <= 512)
  const bool reg_path = D4 <= 64 * NCH;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int dcl[NCH];                                  // clamped column of this lane (loads stay unconditional)
#pragma unroll
  for (int h = 0; h < NCH; ++h) dcl[h] = min(lane + 64 * h, D4 - 1);
  // two rows per wave and trip; the first trip's rows are requested before g_att / the weights are staged
  float4 na[NCH], nb[NCH];
  if (reg_path && L > 0) {
    const float4* ra_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + min(wave, L - 1)) * Dr);
    const float4* rb_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + min(wave + NWV, L - 1)) * Dr);
#pragma unroll
    for (int h = 0; h < NCH; ++h) { na[h] = ra_[dcl[h]]; nb[h] = rb_[dcl[h]]; }
  }
  for (int i = tid; i < Dr * C; i += NT) ga[(i % C) * Dr + i / C] = g_att[(size_t)b * Dr * C + i];
  for (int i = tid; i < L * C; i += NT) ws[i] = weights[(size_t)row0 * C + i];
  __syncthreads();
  if (reg_path) {
    // word level (Dr = H): this lane's g_att columns are loop invariants ([CT][NCH] float4 out of LDS once), the row
    // dot products are reduced on the DPP path -- per row no LDS instruction is left but the C weight broadcasts
    float4 gq[CT][NCH];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        gq[c][h] = reinterpret_cast<const float4*>(ga + (size_t)min(c, C - 1) * Dr)[dcl[h]];
        if (c >= C || lane + 64 * h >= D4) gq[c][h] = zero4;          // clamped duplicates contribute nothing
      }
    for (int l = wave; l < L; l += 2 * NWV) {
      const int lb = l + NWV;
      const bool has_b = lb < L;
      float4 ca[NCH], cb[NCH];
#pragma unroll
      for (int h = 0; h < NCH; ++h) { ca[h] = na[h]; cb[h] = nb[h]; }
      if (l + 2 * NWV < L) {                     // next trip's rows in flight while this trip is consumed
        const float4* ra_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + l + 2 * NWV) * Dr);
        const float4* rb_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + min(l + 3 * NWV, L - 1)) * Dr);
#pragma unroll
        for (int h = 0; h < NCH; ++h) { na[h] = ra_[dcl[h]]; nb[h] = rb_[dcl[h]]; }
      }
      float4 aa[NCH], ab[NCH];
#pragma unroll
      for (int h = 0; h < NCH; ++h) { aa[h] = zero4; ab[h] = zero4; }
      float pa[CT], pb[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        pa[c] = 0.f; pb[c] = 0.f;
        if (c < C) {
          const float wa = ws[l * C + c], wb = ws[(has_b ? lb : l) * C + c];
#pragma unroll
          for (int h = 0; h < NCH; ++h) {
            const float4 q = gq[c][h];
            aa[h].x += wa * q.x; aa[h].y += wa * q.y; aa[h].z += wa * q.z; aa[h].w += wa * q.w;
            ab[h].x += wb * q.x; ab[h].y += wb * q.y; ab[h].z += wb * q.z; ab[h].w += wb * q.w;
            pa[c] += ca[h].x * q.x + ca[h].y * q.y + ca[h].z * q.z + ca[h].w * q.w;
            pb[c] += cb[h].x * q.x + cb[h].y * q.y + cb[h].z * q.z + cb[h].w * q.w;
          }
        }
      }
      float4* da_ = reinterpret_cast<float4*>(dright + ((size_t)row0 + l) * Dr);
      float4* db_ = reinterpret_cast<float4*>(dright + ((size_t)row0 + (has_b ? lb : l)) * Dr);
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        const int d4 = lane + 64 * h;
        if (d4 < D4) { da_[d4] = aa[h]; if (has_b) db_[d4] = ab[h]; }
      }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          const float va = wave_sum_dpp(pa[c]), vb = wave_sum_dpp(pb[c]);
          if (lane == 0) {
            dw[l * C + c] = va + (g_w ? g_w[((size_t)row0 + l) * C + c] : 0.f);
            if (has_b) dw[lb * C + c] = vb + (g_w ? g_w[((size_t)row0 + lb) * C + c] : 0.f);
          }
        }
    }
  } else {
    // wide rows (evidence level: Dr = H * heads + source width): two rows per wave in flight, columns walked in a loop
    for (int l = wave; l < L; l += 2 * NWV) {
      const int lb = l + NWV;
      const bool has_b = lb < L;
      const int lbc = has_b ? lb : l;
      float pa[CT], pb[CT], wa[CT], wb[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        pa[c] = 0.f; pb[c] = 0.f;
        wa[c] = (c < C) ? ws[l * C + c] : 0.f;
        wb[c] = (c < C) ? ws[lbc * C + c] : 0.f;
      }
      const float4* ra_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + l) * Dr);
      const float4* rb_ = reinterpret_cast<const float4*>(right + ((size_t)row0 + lbc) * Dr);
      float4* da_ = reinterpret_cast<float4*>(dright + ((size_t)row0 + l) * Dr);
      float4* db_ = reinterpret_cast<float4*>(dright + ((size_t)row0 + lbc) * Dr);
      for (int d4 = lane; d4 < D4; d4 += 64) {
        const float4 rva = ra_[d4];
        const float4 rvb = rb_[d4];
        float4 aa = zero4, ab = zero4;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) {
            const float4 gq = reinterpret_cast<const float4*>(ga + (size_t)c * Dr)[d4];
            aa.x += wa[c] * gq.x; aa.y += wa[c] * gq.y; aa.z += wa[c] * gq.z; aa.w += wa[c] * gq.w;
            ab.x += wb[c] * gq.x; ab.y += wb[c] * gq.y; ab.z += wb[c] * gq.z; ab.w += wb[c] * gq.w;
            pa[c] += rva.x * gq.x + rva.y * gq.y + rva.z * gq.z + rva.w * gq.w;
            pb[c] += rvb.x * gq.x + rvb.y * gq.y + rvb.z * gq.z + rvb.w * gq.w;
          }
        da_[d4] = aa;
        if (has_b) db_[d4] = ab;
      }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          const float va = wave_sum_dpp(pa[c]), vb = wave_sum_dpp(pb[c]);
          if (lane == 0) {
            dw[l * C + c] = va + (g_w ? g_w[((size_t)row0 + l) * C + c] : 0.f);
            if (has_b) dw[lb * C + c] = vb + (g_w ? g_w[((size_t)row0 + lb) * C + c] : 0.f);
          }
        }
    }
  }
  __syncthreads();
  for (int c = wave; c < C; c += NWV) {
    float sum = 0.f;
    for (int l = lane; l < L; l += 64) sum += ws[l * C + c] * dw[l * C + c];
    sum = wave_sum(sum);
    for (int l = lane; l < L; l += 64)
      de[((size_t)row0 + l) * C + c] = ws[l * C + c] * (dw[l * C + c] - sum);
  }
}


// Row-balanced first half of the same backward for the word level (Dr <= 512): one workgroup per PAIR left 960 workgroups
// of 158 VGPRs for 768 resident slots -- 1.25 rounds, 2.0 TB/s.  Here every WAVE owns an equal run of consecutive rows
// of the whole batch (pair boundaries are crossed by reloading the pair's g_att columns, 4 C floats per lane and chunk,
// contiguous in g_att's [Dr][C] layout), writes dright rows and the raw dw[row][c] = right[row] . g_att[pair][:, c] (+ g_w);
// the per-pair part of the softmax backward (de = w (dw - sum_l w dw)) moves into att_dpre_kernel's prologue, which
// stages those few values per pair anyway.  <= 128 VGPRs: 16 waves per CU, three rows in flight per wave.
template <int CT, bool R16 = false>      // exact number of heads; R16: right holds bf16
__global__ void __launch_bounds__(256, CT <= 5 ? 4 : 3)
att_rows_bwd_kernel(const float* __restrict__ right, const float* __restrict__ weights, const float* __restrict__ g_att,
                    const float* __restrict__ g_w, const int32_t* __restrict__ rowg, int Lmax, int Dr, int C, int M,
                    int rows_per_wave, float* __restrict__ dw_out, float* __restrict__ dright, int D4h) {
  // Rows wider than 512 floats (h = 768): blockIdx.y selects a column range of D4h float4 columns; every range writes its dright
  // columns and its PARTIAL dw (dw_out + range * M * C; att_dpre's prologue adds the ranges in order), g_w rides with range 0.
  constexpr int NCH = 2;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int r0 = gw * rows_per_wave, r1 = min(M, r0 + rows_per_wave);
  if (r0 >= r1) return;
  const int D4 = Dr / 4;
  const int col0 = blockIdx.y * D4h;
  const int ncol = min(D4h, D4 - col0);           // float4 columns of this range
  dw_out += (size_t)blockIdx.y * (size_t)M * CT;
  if (blockIdx.y > 0) g_w = nullptr;
  int dcl[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) dcl[h] = col0 + min(lane + 64 * h, ncol - 1);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  typedef typename RightVec<R16>::T RV;
  const RV* rp = reinterpret_cast<const RV*>(right);
  // this wave's softmax weights and pair ids, staged once into its private LDS region: a per-row global load in the
  // loop (weights[l][c], rowg[l]) put one unhidden memory latency into every iteration
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* wl = reinterpret_cast<float*>(dsm) + (size_t)(threadIdx.x >> 6) * rows_per_wave * (2 * CT + 1);
  int* pl = reinterpret_cast<int*>(wl + (size_t)rows_per_wave * CT);
  float* dwl = wl + (size_t)rows_per_wave * (CT + 1);      // this wave's dw values: written out in one coalesced pass at the end
  const int nr = r1 - r0;
  for (int i = lane; i < nr * CT; i += 64) wl[i] = weights[(size_t)r0 * CT + i];
  for (int i = lane; i < nr; i += 64) pl[i] = rowg ? rowg[r0 + i] : (r0 + i) / Lmax;
  // three rows in flight (loads unconditional from clamped rows; duplicates are never consumed)
  RV ra[NCH], rb[NCH], rc[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    ra[h] = rp[(size_t)r0 * D4 + dcl[h]];
    rb[h] = rp[(size_t)min(r0 + 1, r1 - 1) * D4 + dcl[h]];
    rc[h] = rp[(size_t)min(r0 + 2, r1 - 1) * D4 + dcl[h]];
  }
  float4 gq[CT][NCH];
  int cur = -1;
  // one row: `buf` holds it (requested three rows ago); its slot is re-requested for row l + 3 right away.  The three slots
  // keep their roles (the loop is unrolled by three): rotating them through register moves would make every iteration wait
  // for ALL outstanding loads -- a move out of a register that a load is still filling waits for that load.
  auto step = [&](int l, RV (&buf)[NCH]) __attribute__((always_inline)) {
    if (l >= r1) return;
    const int pair = pl[l - r0];
    if (pair != cur) {          // wave-uniform: this pair's g_att columns, 4 C consecutive floats per lane and chunk
      cur = pair;
      const float4* gp = reinterpret_cast<const float4*>(g_att + (size_t)pair * Dr * CT);
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        float G[4 * CT];
#pragma unroll
        for (int j = 0; j < CT; ++j) {
          const float4 v = gp[(size_t)dcl[h] * CT + j];
          G[4 * j] = v.x; G[4 * j + 1] = v.y; G[4 * j + 2] = v.z; G[4 * j + 3] = v.w;
        }
        const bool live = lane + 64 * h < ncol;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          // element (d = 4 d4 + k, c) sits at G[k * C + c] (the kernel is instantiated for the exact head count: C == CT)
          gq[c][h] = live ? make_float4(G[0 * CT + c], G[1 * CT + c], G[2 * CT + c], G[3 * CT + c]) : zero4;
      }
    }
    float4 cu[NCH];
#pragma unroll
    for (int h = 0; h < NCH; ++h) cu[h] = right_widen(buf[h]);
    if (l + 3 < r1) {
#pragma unroll
      for (int h = 0; h < NCH; ++h) buf[h] = rp[(size_t)(l + 3) * D4 + dcl[h]];
    }
    float4 aa[NCH];
#pragma unroll
    for (int h = 0; h < NCH; ++h) aa[h] = zero4;
    float pa[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      pa[c] = 0.f;
      const float wv = wl[(l - r0) * CT + c];
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        const float4 q = gq[c][h];
        aa[h].x += wv * q.x; aa[h].y += wv * q.y; aa[h].z += wv * q.z; aa[h].w += wv * q.w;
        pa[c] += cu[h].x * q.x + cu[h].y * q.y + cu[h].z * q.z + cu[h].w * q.w;
      }
    }
    float4* dp = reinterpret_cast<float4*>(dright + (size_t)l * Dr);
#pragma unroll
    for (int h = 0; h < NCH; ++h)
      if (lane + 64 * h < ncol) dp[col0 + lane + 64 * h] = aa[h];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const float v = wave_sum_dpp(pa[c]);
      if (lane == 0) dwl[(l - r0) * CT + c] = v;
    }
  };
  for (int l = r0; l < r1; l += 3) {
    step(l, ra);
    step(l + 1, rb);
    step(l + 2, rc);
  }
  if (g_w) {
    for (int i = lane; i < nr * CT; i += 64) dw_out[(size_t)r0 * CT + i] = dwl[i] + g_w[(size_t)r0 * CT + i];
  } else {
    for (int i = lane; i < nr * CT; i += 64) dw_out[(size_t)r0 * CT + i] = dwl[i];
  }
}
int launch_att_softmax_bwd(const float* right, const float* weights, const float* g_att, const float* g_w,
                           const int32_t* goff, int m_real, int b, int l, int dr, int heads, float* de, float* dright,
                           hipStream_t s, const int32_t* rowg, float* dw_tmp, int* dw_written, const void* right16) {
  GH_REQUIRE(right || right16, "att_softmax_bwd: no right operand");
  GH_REQUIRE(dr % 4 == 0 && (reinterpret_cast<uintptr_t>(right) & 15) == 0 && (reinterpret_cast<uintptr_t>(right16) & 7) == 0 &&
             (reinterpret_cast<uintptr_t>(dright) & 15) == 0, "att_softmax_bwd: right rows must be float4-shaped (dr=%d)", dr);
  if (dw_written) *dw_written = 0;
  // many pairs, rows that fit two float4 chunks per lane, 16-byte aligned g_att rows: the row-balanced kernel; de is then
  // finished by att_dpre's prologue (launch_att_dpre with dw_in)
  // (rows wider than 512 floats: ceil(dr / 512) column ranges, each a grid row of its own; *dw_written = the number of ranges.
  //  Up to 16 ranges: the evidence level at h = 768 has 6272-float rows over only 32 claims -- the per-pair kernel below, one workgroup
  //  per claim, streamed 1.5 MB per workgroup in 90 us)
  if (dw_tmp && dw_written && dr / 4 <= 16 * 128 && (goff == nullptr || rowg != nullptr) &&
      (reinterpret_cast<uintptr_t>(g_att) & 15) == 0 && heads >= 1 && heads <= 8) {
    const int M = goff ? m_real : b * l;
    if (M <= 0) return 0;
    const int waves = 256 * 4 * 4;                       // 16 waves per CU
    int rpw = (M + waves - 1) / waves < 4 ? 4 : (M + waves - 1) / waves;
    if (rpw > 256) rpw = 256;                            // (LDS staging of a wave's weights: more waves instead of longer runs)
    const int nwg = ((M + rpw - 1) / rpw + 3) / 4;
    const size_t lds_rows = (size_t)4 * rpw * (2 * heads + 1) * 4;
    const int ptag = few_rows_tag(b, PROF_ATT_SOFTMAX_BWD);
    static const void* const fns[8] = {(const void*)att_rows_bwd_kernel<1>, (const void*)att_rows_bwd_kernel<2>,
                                       (const void*)att_rows_bwd_kernel<3>, (const void*)att_rows_bwd_kernel<4>,
                                       (const void*)att_rows_bwd_kernel<5>, (const void*)att_rows_bwd_kernel<6>,
                                       (const void*)att_rows_bwd_kernel<7>, (const void*)att_rows_bwd_kernel<8>};
    static const void* const fns16[8] = {(const void*)att_rows_bwd_kernel<1, true>, (const void*)att_rows_bwd_kernel<2, true>,
                                         (const void*)att_rows_bwd_kernel<3, true>, (const void*)att_rows_bwd_kernel<4, true>,
                                         (const void*)att_rows_bwd_kernel<5, true>, (const void*)att_rows_bwd_kernel<6, true>,
                                         (const void*)att_rows_bwd_kernel<7, true>, (const void*)att_rows_bwd_kernel<8, true>};
    const void* fn = right16 ? fns16[heads - 1] : fns[heads - 1];
    if (right16) right = reinterpret_cast<const float*>(right16);
    int Mv = M, rpwv = rpw;
    const int ranges = (dr / 4 + 127) / 128;
    int d4h = (dr / 4 + ranges - 1) / ranges;
    void* args[] = {(void*)&right, (void*)&weights, (void*)&g_att, (void*)&g_w, (void*)&rowg, (void*)&l, (void*)&dr, (void*)&heads,
                    (void*)&Mv, (void*)&rpwv, (void*)&dw_tmp, (void*)&dright, (void*)&d4h};
    if (int rc = lds_opt_in(fn, lds_rows, "att_rows_bwd")) return rc;      // (256 rows per wave x 8 heads: 69 632 B)
    prof_begin(s, ptag);
    (void)hipLaunchKernel(fn, dim3(nwg, ranges), dim3(256), args, lds_rows, s);
    prof_end(ptag, (right16 ? 6.0 : 8.0) * M * dr + 4.0 * (3.0 * M * heads + (double)b * dr * heads), s);
    GH_LAUNCH_CHECK();
    *dw_written = ranges;
    return 0;
  }
  GH_REQUIRE(right, "att_softmax_bwd: the per-pair kernel (few pairs / no row map) reads an fp32 right operand");
  const size_t lds = ((size_t)dr * heads + 2 * (size_t)l * heads) * 4;
  GH_REQUIRE(heads >= 1 && heads <= 8, "att_softmax_bwd: %d heads (1..8 supported)", heads);
  const void* fn = heads <= 2 ? (const void*)att_softmax_bwd_kernel<2> : heads <= 5 ? (const void*)att_softmax_bwd_kernel<5>
                                                                                   : (const void*)att_softmax_bwd_kernel<8>;
  if (int rc = lds_opt_in(fn, lds, "att_softmax_bwd")) return rc;
  prof_begin(s, few_rows_tag(b, PROF_ATT_SOFTMAX_BWD));
  // few pairs (evidence level: one workgroup per claim): eight waves share the rows of a pair
  void* args[] = {(void*)&right, (void*)&weights, (void*)&g_att, (void*)&g_w, (void*)&goff, (void*)&l, (void*)&dr, (void*)&heads,
                  (void*)&de, (void*)&dright};
  (void)hipLaunchKernel(fn, dim3(b), dim3(b < 512 ? 512 : 256), args, lds, s);
  const double rows = goff ? (double)m_real : (double)b * l;
  prof_end(few_rows_tag(b, PROF_ATT_SOFTMAX_BWD), 4.0 * (2.0 * rows * dr + 3.0 * rows * heads + (double)b * dr * heads), s);
  GH_LAUNCH_CHECK();
  return 0;
}

// dpre[m][n] = (sum_c de[m][c] w2[c][n]) (1 - t[m][n]^2) ; du[b][n] = sum_l dpre[b*L+l][n] ;
// dw2 partial [b][c][n] = sum_l de[m][c] t[m][n]   (summed over b by reduce_partials afterwards).
// One workgroup per (pair, column slab of S4 float4): threads = (float4 column of the slab, row lane); row lanes take
// every RL-th row.  Slabs triple the number of workgroups (2880 at the bench shape) and cut a thread's serial row walk
// to a third -- the one-workgroup-per-pair version was latency-bound at 2.0 TB/s.
__global__ void att_dpre_kernel(const float* __restrict__ de, const float* __restrict__ w2, const float* __restrict__ t,
                                const int32_t* __restrict__ goff, int Lmax, int Ha, int C, int RL, int S4,
                                float* __restrict__ dpre, float* __restrict__ du, float* __restrict__ dw2_part,
                                const float* __restrict__ dw_in, const float* __restrict__ wts, float* __restrict__ de_out,
                                unsigned short* __restrict__ dpre16,        // dpre16 != NULL: dpre is written THERE as bf16 (RNE) instead
                                long long dw_range_stride, int dw_ranges) { // dw_ranges > 1: dw_in holds that many column-range partials, dw_range_stride floats apart
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float4* red = reinterpret_cast<float4*>(dsm);           // [RL][1 + C][S4]
  const int b = blockIdx.x;
  const int row0 = goff ? goff[b] : b * Lmax;
  const int L = goff ? goff[b + 1] - row0 : Lmax;
  const int n4 = Ha / 4;
  float* des = reinterpret_cast<float*>(red + (size_t)RL * (1 + C) * S4);       // [L][C]: read once, not once per thread and row
  const int s0 = blockIdx.y * S4;                          // first float4 column of this slab
  const int sw = min(S4, n4 - s0);
  const int cl = threadIdx.x % S4, rl = threadIdx.x / S4;
  const int c4 = s0 + cl;
  const bool act = rl < RL && cl < sw;
  // RB rows per thread and trip with all loads ahead of the math; the first trip's rows are requested before `de` is
  // staged (loads unconditional from clamped rows / columns; clamped duplicates are never consumed)
  constexpr int RB = 4;
  const int c4c = min(c4, n4 - 1);
  const float4* tb = reinterpret_cast<const float4*>(t + (size_t)row0 * Ha) + c4c;
  float4 nxt[RB];
  if (L > 0) {
#pragma unroll
    for (int u = 0; u < RB; ++u) nxt[u] = tb[(size_t)min(rl + u * RL, L - 1) * n4];
  }
  if (dw_in) {
    // second half of the softmax backward, per pair (att_rows_bwd_kernel left the raw dw): de = w (dw - sum_l w dw)
    float* wl = des + (size_t)Lmax * C;                    // [L][C] softmax weights
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) {
      float v = dw_in[(size_t)row0 * C + i];
      for (int rg = 1; rg < dw_ranges; ++rg) v += dw_in[(size_t)rg * (size_t)dw_range_stride + (size_t)row0 * C + i];
      des[i] = v; wl[i] = wts[(size_t)row0 * C + i];
    }
    __syncthreads();
    float* sums = wl + (size_t)Lmax * C;                   // [C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    for (int c = wave; c < C; c += nwv) {
      float sm = 0.f;
      for (int l = lane; l < L; l += 64) sm += wl[l * C + c] * des[l * C + c];
      for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
      if (lane == 0) sums[c] = sm;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) {
      const float v = wl[i] * (des[i] - sums[i % C]);
      des[i] = v;
      if (de_out && blockIdx.y == 0) de_out[(size_t)row0 * C + i] = v;
    }
  } else {
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) des[i] = de[(size_t)row0 * C + i];
  }
  float4 wc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    wc[c] = reinterpret_cast<const float4*>(w2 + (size_t)min(c, C - 1) * Ha)[c4c];
    if (c >= C || !act) wc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 dw[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) dw[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (act) {
    for (int l0 = rl; l0 < L; l0 += RB * RL) {
      float4 cur[RB];
#pragma unroll
      for (int u = 0; u < RB; ++u) cur[u] = nxt[u];
      if (l0 + RB * RL < L) {
#pragma unroll
        for (int u = 0; u < RB; ++u) nxt[u] = tb[(size_t)min(l0 + (RB + u) * RL, L - 1) * n4];
      }
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        const int l = l0 + u * RL;
        if (l >= L) break;
        const size_t m = (size_t)row0 + l;
        const float4 tv = cur[u];
        float4 dt = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < C) {
            const float e = des[l * C + c];
            dt.x += e * wc[c].x; dt.y += e * wc[c].y; dt.z += e * wc[c].z; dt.w += e * wc[c].w;
            dw[c].x += e * tv.x; dw[c].y += e * tv.y; dw[c].z += e * tv.z; dw[c].w += e * tv.w;
          }
        const float4 dp = make_float4(dt.x * (1.f - tv.x * tv.x), dt.y * (1.f - tv.y * tv.y), dt.z * (1.f - tv.z * tv.z),
                                      dt.w * (1.f - tv.w * tv.w));
        if (dpre16) {
          reinterpret_cast<uint2*>(dpre16 + m * Ha)[c4] = f4_to_bf4(dp);
        } else {
          reinterpret_cast<float4*>(dpre + m * Ha)[c4] = dp;
        }
        acc.x += dp.x; acc.y += dp.y; acc.z += dp.z; acc.w += dp.w;
      }
    }
  }
  if (rl < RL) {
    red[(rl * (1 + C) + 0) * S4 + cl] = acc;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < C) red[(rl * (1 + C) + 1 + c) * S4 + cl] = dw[c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (1 + C) * sw; i += blockDim.x) {
    const int which = i / sw, cc = i % sw;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < RL; ++k) {
      const float4 x = red[(k * (1 + C) + which) * S4 + cc];
      v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
    }
    if (which == 0) reinterpret_cast<float4*>(du + (size_t)b * Ha)[s0 + cc] = v;
    else if (dw2_part) reinterpret_cast<float4*>(dw2_part + ((size_t)b * C + (which - 1)) * Ha)[s0 + cc] = v;
  }
}

int launch_att_dpre(const float* de, const float* w2, const float* t, const int32_t* goff, int m_real, int b, int l,
                    int ha, int heads, float* dpre, float* du, float* dw2_part, hipStream_t s, const float* dw_in,
                    const float* weights, float* de_out, void* dpre16, long long dw_range_stride, int dw_ranges) {
  GH_REQUIRE(ha % 4 == 0 && ha / 4 <= 256, "att_dpre: attention hidden %d must be a multiple of 4 and <= 1024", ha);
  const int n4 = ha / 4;
  // column slabs of <= 32 float4 (512 B of a row per lane group: whole 128-byte lines), ~3 slabs at ha = 300; few pairs
  // (evidence level) keep one slab per 64 columns
  // whole rows per workgroup up to 512 floats: a column slab makes every row a short run (400 B at three slabs) that
  // straddles 128-byte lines shared with the neighbouring slab's workgroup -- measured 3.1 / 3.6 / 3.9 / 4.3 TB/s at
  // 5 / 3 / 2 / 1 slabs once the row batches are prefetched
  // (round 5: 3 / 5 / 8 slabs for the few-pair launches -- evidence level, 32 workgroups of 30 rows -- measured: no effect on the step)
  const int nsl = (n4 + 127) / 128;
  const int S4 = (n4 + nsl - 1) / nsl;
  const int RL = (256 / S4) > 0 ? (256 / S4) : 1;
  const int threads = ((S4 * RL + 63) / 64) * 64;
  GH_REQUIRE(!dw_in || weights, "att_dpre: dw_in needs the softmax weights");
  const size_t lds = (size_t)RL * (1 + heads) * S4 * 16 + (size_t)l * heads * 4 * (dw_in ? 2 : 1) + (dw_in ? 64 : 0);
  prof_begin(s, few_rows_tag(b, PROF_ATT_DPRE));
  hipLaunchKernelGGL(att_dpre_kernel, dim3(b, nsl), dim3(threads), lds, s, de, w2, t, goff, l, ha, heads, RL, S4, dpre, du, dw2_part,
                     dw_in, weights, de_out, (unsigned short*)dpre16, dw_range_stride, dw_ranges);
  const double rows = goff ? (double)m_real : (double)b * l;
  prof_end(few_rows_tag(b, PROF_ATT_DPRE), 4.0 * (2.0 * rows * ha + rows * heads + (double)b * ha), s);
  GH_LAUNCH_CHECK();
  return 0;
}

}  // namespace gh
