// varlen.hip - the row movers of variable-length (packed) encoder batches.
// A ragged batch of B right-padded sequences runs as ONE (T_total, d) matrix, T_total = sum(len_b); sequence b owns rows
// cu[b] .. cu[b + 1] (cu_seqlens: int32 (B + 1) on the device, cu[0] = 0, non-decreasing).  Every row-wise operator (GEMM, LayerNorm)
// takes that matrix as it is; the attention that knows the boundaries is pm_attention_varlen_bf16 (attention_bf16.hip).  What is
// left lives here: the token embedding straight into packed rows, pack / unpack / zero-tail between the padded (B, L, d) and the
// packed layout, and the per-sequence mean.  All of them are HBM-bound copies: one wave per row, 16-byte accesses, the rows of a
// sequence past its length cost one compare.  No kernel reads a padded row.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// row (b, t) of the padded side, or "none" when the wave has nothing to do; len = cu[b + 1] - cu[b] clamped to [0, L]
struct VRow {
  int b, t, len, row0;
};
__device__ __forceinline__ VRow vrow(const int* __restrict__ cu, int64_t rows, int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  VRow v{-1, 0, 0, 0};
  if (row >= rows) return v;
  v.b = (int)(row / L);
  v.t = (int)(row % L);
  v.row0 = cu[v.b];
  const int n = cu[v.b + 1] - v.row0;
  v.len = n < 0 ? 0 : (n > L ? L : n);
  return v;
}

// out[cu[b] + t] = emb[tok[b, t]] + pos[t] for t < len_b: embed_kernel's arithmetic (embed.hip) on packed output rows
template <bool YF32, typename ET>
__global__ __launch_bounds__(256) void embed_varlen_kernel(const int64_t* __restrict__ tok, const ET* __restrict__ E,
                                                           const float* __restrict__ pos, const int* __restrict__ cu,
                                                           void* __restrict__ out, int64_t rows, int L, int d, int V) {
  const int lane = threadIdx.x & 63;
  const VRow w = vrow(cu, rows, L);
  if (w.b < 0 || w.t >= w.len) return;
  int64_t t = tok[(int64_t)w.b * L + w.t];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);  // ops.embed_tokens_varlen raises on ids outside [0, V) at valid positions; a raw caller's bad id cannot fault
  const int64_t orow = (int64_t)w.row0 + w.t;
  for (int c = lane; c < d / 8; c += 64) {
    float e[8];
    if constexpr (sizeof(ET) == 2) {
      const bf16x8 ev = *(const bf16x8*)(E + t * d + c * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = (float)ev[i];
    } else {
      const f32x4 e0 = *(const f32x4*)(E + t * d + c * 8), e1 = *(const f32x4*)(E + t * d + c * 8 + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { e[i] = e0[i]; e[4 + i] = e1[i]; }
    }
    f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0;
    if (pos) {
      p0 = *(const f32x4*)(pos + (int64_t)w.t * d + c * 8);
      p1 = *(const f32x4*)(pos + (int64_t)w.t * d + c * 8 + 4);
    }
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = e[i] + p0[i]; v[4 + i] = e[4 + i] + p1[i]; }
    if constexpr (YF32) {
      *(f32x4*)((float*)out + orow * d + c * 8) = f32x4{v[0], v[1], v[2], v[3]};
      *(f32x4*)((float*)out + orow * d + c * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
      bf16x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (bf16)v[i];
      *(bf16x8*)((bf16*)out + orow * d + c * 8) = o;
    }
  }
}

// MODE 0: packed[cu[b] + t] = padded[b, t] (t < len_b).  1: padded[b, t] = t < len_b ? packed[cu[b] + t] : 0.  2: padded[b, t] = 0
// for t >= len_b.  Rows are nch 16-byte chunks; strides in bytes.
template <int MODE>
__global__ __launch_bounds__(256) void rows_kernel(char* __restrict__ padded, int64_t psb, int64_t pst, char* __restrict__ packed,
                                                   int64_t kst, const int* __restrict__ cu, int64_t rows, int L, int nch) {
  const int lane = threadIdx.x & 63;
  const VRow w = vrow(cu, rows, L);
  if (w.b < 0) return;
  const bool live = w.t < w.len;
  if (MODE == 0 && !live) return;
  if (MODE == 2 && live) return;
  char* pr = padded + (int64_t)w.b * psb + (int64_t)w.t * pst;
  char* kr = packed + ((int64_t)w.row0 + w.t) * kst;  // dereferenced for live rows only
  for (int c = lane; c < nch; c += 64) {
    if constexpr (MODE == 0) {
      *(u32x4*)(kr + c * 16) = *(const u32x4*)(pr + c * 16);
    } else {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (MODE == 1 && live) v = *(const u32x4*)(kr + c * 16);
      *(u32x4*)(pr + c * 16) = v;
    }
  }
}

// out[b, :] = mean of rows cu[b] .. cu[b + 1] of x: a lane owns 16 bytes of columns and adds the rows IN ORDER in fp32 (no
// atomics, no tree whose shape depends on the launch): the result is a function of the sequence's rows alone.  Length 0 -> zeros.
template <typename XT>
__global__ __launch_bounds__(64) void segment_mean_kernel(const XT* __restrict__ x, int64_t xst, const int* __restrict__ cu,
                                                          float* __restrict__ out, int d) {
  constexpr int W = 16 / sizeof(XT);
  const int b = blockIdx.y;
  const int c = (blockIdx.x * 64 + threadIdx.x) * W;
  if (c >= d) return;
  const int row0 = cu[b], n = cu[b + 1] - row0;
  float acc[W];
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.f;
  const XT* p = x + (int64_t)row0 * xst + c;
  for (int t = 0; t < n; ++t, p += xst) {
    if constexpr (sizeof(XT) == 2) {
      const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += (float)v[i];
    } else {
      const f32x4 v = *(const f32x4*)p;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += v[i];
    }
  }
  const float nf = n > 0 ? (float)n : 1.f;
#pragma unroll
  for (int i = 0; i < W; i += 4)
    *(f32x4*)(out + (int64_t)b * d + c + i) = f32x4{acc[i] / nf, acc[i + 1] / nf, acc[i + 2] / nf, acc[i + 3] / nf};
}

int rows_launch(int mode, void* padded, int64_t psb, int64_t pst, void* packed, int64_t kst, const int32_t* cu, int64_t B, int64_t L,
                int64_t d, int64_t eb, void* stream) {
  if (!padded || !packed || !cu || B < 0 || L < 0 || d <= 0 || (eb != 2 && eb != 4)) return PM_EINVAL;
  if (pst < d || kst < d || psb < 0) return PM_EINVAL;
  if ((d * eb) % 16) return PM_EUNSUPPORTED;
  if (((psb | pst | kst) * eb) % 16) return PM_EALIGN;
  if (((uintptr_t)padded | (uintptr_t)packed) & 15) return PM_EALIGN;
  if ((uintptr_t)cu & 3) return PM_EALIGN;
  if (B == 0 || L == 0) return PM_OK;
  const int64_t rows = B * L, nblk = (rows + 3) / 4;
  if (nblk > 0x7fffffff || L > 0x7fffffff || d * eb / 16 > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_ROWS(M_)                                                                                                   \
  hipLaunchKernelGGL((rows_kernel<M_>), dim3((unsigned)nblk), dim3(256), 0, st, (char*)padded, psb * eb, pst * eb,     \
                     (char*)packed, kst * eb, (const int*)cu, rows, (int)L, (int)(d * eb / 16))
  if (mode == 0) PM_ROWS(0);
  else if (mode == 1) PM_ROWS(1);
  else PM_ROWS(2);
#undef PM_ROWS
  PM_CHECK_LAUNCH();
  return PM_OK;
}

}  // namespace

extern "C" int pm_embed_tokens_varlen(const int64_t* tokens, const void* emb, int emb_dtype, const float* pos,
                                      const int32_t* cu_seqlens, void* out, int out_dtype, int64_t B, int64_t L, int64_t d,
                                      int64_t V, void* stream) {
  if (!tokens || !emb || !cu_seqlens || !out || B < 0 || L < 0 || d <= 0 || V <= 0) return PM_EINVAL;
  if ((emb_dtype != PM_BF16 && emb_dtype != PM_F32) || (out_dtype != PM_BF16 && out_dtype != PM_F32)) return PM_EINVAL;
  if (emb_dtype == PM_F32 && out_dtype != PM_F32) return PM_EUNSUPPORTED;  // an fp32 table makes fp32 rows, as pm_embed_tokens_f32
  if (d % 8) return PM_EUNSUPPORTED;
  if (((uintptr_t)emb | (uintptr_t)pos | (uintptr_t)out) & 15) return PM_EALIGN;
  if ((uintptr_t)cu_seqlens & 3) return PM_EALIGN;
  if (B == 0 || L == 0) return PM_OK;
  const int64_t rows = B * L, nblk = (rows + 3) / 4;
  if (nblk > 0x7fffffff || L > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_EMBV(YF_, ET_)                                                                                             \
  hipLaunchKernelGGL((embed_varlen_kernel<YF_, ET_>), dim3((unsigned)nblk), dim3(256), 0, st, tokens, (const ET_*)emb, \
                     pos, (const int*)cu_seqlens, out, rows, (int)L, (int)d, (int)V)
  if (emb_dtype == PM_F32) PM_EMBV(true, float);
  else if (out_dtype == PM_F32) PM_EMBV(true, bf16);
  else PM_EMBV(false, bf16);
#undef PM_EMBV
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_rows_pack(const void* x, int64_t x_stride_b, int64_t x_stride_t, const int32_t* cu_seqlens, void* out,
                            int64_t out_stride_t, int64_t B, int64_t L, int64_t d, int64_t elem_bytes, void* stream) {
  return rows_launch(0, const_cast<void*>(x), x_stride_b, x_stride_t, out, out_stride_t, cu_seqlens, B, L, d, elem_bytes, stream);
}

extern "C" int pm_rows_unpack(const void* x, int64_t x_stride_t, const int32_t* cu_seqlens, void* out, int64_t out_stride_b,
                              int64_t out_stride_t, int64_t B, int64_t L, int64_t d, int64_t elem_bytes, void* stream) {
  return rows_launch(1, out, out_stride_b, out_stride_t, const_cast<void*>(x), x_stride_t, cu_seqlens, B, L, d, elem_bytes, stream);
}

extern "C" int pm_rows_zero_tail(void* x, int64_t x_stride_b, int64_t x_stride_t, const int32_t* cu_seqlens, int64_t B, int64_t L,
                                 int64_t d, int64_t elem_bytes, void* stream) {
  return rows_launch(2, x, x_stride_b, x_stride_t, x, x_stride_t, cu_seqlens, B, L, d, elem_bytes, stream);
}

extern "C" int pm_segment_mean(const void* x, int64_t x_stride_t, int x_dtype, const int32_t* cu_seqlens, float* out, int64_t B,
                               int64_t d, void* stream) {
  if (!x || !cu_seqlens || !out || B < 0 || d <= 0 || x_stride_t < d) return PM_EINVAL;
  if (x_dtype != PM_BF16 && x_dtype != PM_F32) return PM_EINVAL;
  const int64_t eb = x_dtype == PM_BF16 ? 2 : 4, w = 16 / eb;
  if (d % w) return PM_EUNSUPPORTED;
  if ((x_stride_t * eb) % 16) return PM_EALIGN;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return PM_EALIGN;
  if ((uintptr_t)cu_seqlens & 3) return PM_EALIGN;
  if (B == 0) return PM_OK;
  if (B > 65535 || d > 0x7fffffff) return PM_EINVAL;
  const dim3 grid((unsigned)((d / w + 63) / 64), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == PM_BF16)
    hipLaunchKernelGGL((segment_mean_kernel<bf16>), grid, dim3(64), 0, st, (const bf16*)x, x_stride_t, (const int*)cu_seqlens, out, (int)d);
  else
    hipLaunchKernelGGL((segment_mean_kernel<float>), grid, dim3(64), 0, st, (const float*)x, x_stride_t, (const int*)cu_seqlens, out, (int)d);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
