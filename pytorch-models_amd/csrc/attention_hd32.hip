// attention_hd32.hip - pm_attention_hd32_bf16: flash-style softmax(q k^T / sqrt(32)) v for head dim 32 on the bf16 MFMA
// (DETR's attentions, reference pytorch_models/image/detr.py:64-87 over transformer.py:36-53: d_model 256, 8 heads; encoder
// self-attention over the H*W image tokens, decoder self-attention over 100 queries, cross-attention 100 x H*W).
// No bias, no causal mask.  Addressing as pm_attention_bf16: q / k / v / o are base + b*stride_b + token*stride_t + h*32.
//
// Workgroup = 4 waves = 64 queries of one (batch, head); wave w owns queries 16 w .. 16 w + 15 and walks the keys in tiles of 64.
// The layout is the one of pm_window_attention_bf16 (maxvit.hip) with a running maximum / sum added:
//   S^T = K Q^T : MFMA 16x16x32, k = the 32 head dims in ONE step.  A = 16 key rows, B = the wave's 16 query rows, both 16-byte
//                 fragments read straight from global (the K rows of a tile are read by all four waves: L1 / L2 hits).  The
//                 accumulator of key block kb has the QUERY on the lane (l & 15) and keys 16 kb + 4 (l >> 4) + i.
//   softmax     : online, fp32, in the log2 domain.  Tile maximum in-lane over 16 keys, then across the four 16-lane groups
//                 (xor 16, 32); keys >= Lk are -inf (P = 0).  Lk >= 1 and there is no mask, so the first tile always has a
//                 finite maximum and no row is ever dead.  The row sum accumulates the fp32 P, the matrix product takes P
//                 rounded to bf16 (rounding is unbiased, the sum stays the exact normaliser of the unrounded weights).
//   O^T += V^T P^T : the S^T accumulators of key blocks (2c, 2c + 1), converted to bf16, ARE the B operand of k-chunk c
//                 (element j of lane group g = key 16 (2c + (j >> 2)) + 4 g + (j & 3)).  The A operand V^T needs, per lane, 8
//                 keys of ONE dim: the workgroup writes the V tile transposed into LDS (dim-major rows of 64 keys, padded to
//                 68) and a fragment is two 8-byte LDS reads.  Rows of keys >= Lk are written as zeros (0 x NaN is NaN).
//   O^T has the query on the lane: rescaling by 2^(m_old - m_new) and the final division are per lane, 8-byte stores of 4 dims.
// The next tile's K fragments and V chunk are requested before the current tile's arithmetic (register prefetch); the V tile in
// LDS is double-buffered, one barrier per tile.
#include "common.h"

namespace {

constexpr int A32_WAVES = 4;
constexpr int A32_QB = 16 * A32_WAVES;  // queries per workgroup
constexpr int A32_KT = 64;              // keys per tile
constexpr int A32_VLD = 68;             // bf16 per dim row of the transposed V tile (64 keys + 4: 8-byte aligned, skews banks)

__global__ __launch_bounds__(64 * A32_WAVES) void attention_hd32_kernel(
    const bf16* __restrict__ Q, int64_t q_sb, int64_t q_st, const bf16* __restrict__ K, int64_t k_sb, int64_t k_st,
    const bf16* __restrict__ V, int64_t v_sb, int64_t v_st, bf16* __restrict__ O, int64_t o_sb, int64_t o_st, int H, int Lq,
    int Lk, float scale_log2) {
  __shared__ __attribute__((aligned(16))) bf16 vt[2][32 * A32_VLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.x * A32_QB + wave * 16;
  const bf16* Qb = Q + (int64_t)b * q_sb + h * 32;
  const bf16* Kb = K + (int64_t)b * k_sb + h * 32;
  const bf16* Vb = V + (int64_t)b * v_sb + h * 32;

  // the wave's query fragment: row q0 + i16 (clamped: rows >= Lq are computed and never stored), dims 8 g .. 8 g + 7
  const int qi = q0 + i16;
  const int qic = qi < Lq ? qi : Lq - 1;
  const bf16x8 qf = *(const bf16x8*)(Qb + (int64_t)qic * q_st + g * 8);

  const int ntiles = (Lk + A32_KT - 1) / A32_KT;
  // V chunk of this thread: key tid >> 2 of the tile, dims 8 (tid & 3) .. + 7
  const int vkey = tid >> 2, vch = tid & 3;
  bf16x8 kf[4], vreg;
  auto load_tile = [&](int t) {
    const int k0 = t * A32_KT;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      int key = k0 + 16 * kb + i16;
      key = key < Lk ? key : Lk - 1;  // clamped rows score -inf below
      kf[kb] = *(const bf16x8*)(Kb + (int64_t)key * k_st + g * 8);
    }
    const int key = k0 + vkey;
    if (key < Lk) {
      vreg = *(const bf16x8*)(Vb + (int64_t)key * v_st + vch * 8);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) vreg[e] = (bf16)0.f;
    }
  };
  auto store_v = [&](int buf) {
    bf16* d = vt[buf] + vkey;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[(vch * 8 + e) * A32_VLD] = vreg[e];
  };

  f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float m_run = -INFINITY, l_run = 0.f;

  load_tile(0);
  store_v(0);
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    bf16x8 kc[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) kc[kb] = kf[kb];
    __syncthreads();  // tile t's V is in vt[buf]; everyone is done reading vt[buf ^ 1] (tile t - 1)
    if (t + 1 < ntiles) load_tile(t + 1);

    f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[kb], qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    const int k0 = t * A32_KT;
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = s[kb][i] * scale_log2;
        if (k0 + 16 * kb + 4 * g + i >= Lk) v = -INFINITY;
        s[kb][i] = v;
        m = fmaxf(m, v);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float m_new = fmaxf(m_run, m);  // finite: every tile holds at least one key < Lk
    const float alpha = exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = exp2f(s[kb][i] - m_new);
        s[kb][i] = p;
        sum += p;
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = m_new;
    bf16x8 pf[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[c][j] = (bf16)s[2 * c][j];
        pf[c][4 + j] = (bf16)s[2 * c + 1][j];
      }
    }
    const bf16* vb = vt[buf];
#pragma unroll
    for (int db = 0; db < 2; ++db) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[db][i] *= alpha;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16* row = vb + (16 * db + i16) * A32_VLD + 32 * c + 4 * g;
        const bf16x4 lo = *(const bf16x4*)row, hi = *(const bf16x4*)(row + 16);
        const bf16x8 va = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pf[c], o[db], 0, 0, 0);
      }
    }
    if (t + 1 < ntiles) store_v(buf ^ 1);  // vt[buf ^ 1] was last read in iteration t - 1, before this iteration's barrier
  }
  if (qi < Lq) {
    const float inv = 1.0f / l_run;
    bf16* orow = O + (int64_t)b * o_sb + (int64_t)qi * o_st + h * 32 + 4 * g;
#pragma unroll
    for (int db = 0; db < 2; ++db)
      *(bf16x4*)(orow + 16 * db) = bf16x4{(bf16)(o[db][0] * inv), (bf16)(o[db][1] * inv), (bf16)(o[db][2] * inv), (bf16)(o[db][3] * inv)};
  }
}

bool a32_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

extern "C" int pm_attention_hd32_bf16(const void* q, int64_t q_stride_b, int64_t q_stride_t, const void* k, int64_t k_stride_b,
                                      int64_t k_stride_t, const void* v, int64_t v_stride_b, int64_t v_stride_t, void* o,
                                      int64_t o_stride_b, int64_t o_stride_t, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                                      void* stream) {
  if (!q || !k || !v || !o || B < 0 || H <= 0 || Lq < 1 || Lk < 1) return PM_EINVAL;
  if (Lq > (1 << 24) || Lk > (1 << 24) || B * H > 65535) return PM_EUNSUPPORTED;
  const int64_t strides[] = {q_stride_b, q_stride_t, k_stride_b, k_stride_t, v_stride_b, v_stride_t};
  for (int64_t s : strides)
    if (s % 8) return PM_EALIGN;  // 16-byte fragment loads
  if (o_stride_b % 4 || o_stride_t % 4) return PM_EALIGN;
  if (o_stride_t < H * 32) return PM_EINVAL;
  if (!a32_aligned(q, 16) || !a32_aligned(k, 16) || !a32_aligned(v, 16) || !a32_aligned(o, 8)) return PM_EALIGN;
  if (B == 0) return PM_OK;
  const float scale_log2 = 0.17677669529663687f * 1.4426950408889634f;  // 1 / sqrt(32) * log2(e)
  const dim3 grid((unsigned)((Lq + A32_QB - 1) / A32_QB), (unsigned)(B * H));
  hipLaunchKernelGGL(attention_hd32_kernel, grid, dim3(64 * A32_WAVES), 0, (hipStream_t)stream, (const bf16*)q, q_stride_b,
                     q_stride_t, (const bf16*)k, k_stride_b, k_stride_t, (const bf16*)v, v_stride_b, v_stride_t, (bf16*)o,
                     o_stride_b, o_stride_t, (int)H, (int)Lq, (int)Lk, scale_log2);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
