// convnext.hip - the ConvNeXt-specific stages (reference: pytorch_models/image/convnext.py), NHWC rows, fp32 arithmetic,
// bf16 or f32 at the edges:
//  * pm_dwconv7_ln        Conv2d(C, C, 7, padding 3, groups C) + bias, then LayerNorm over C (every block, convnext.py:22-25);
//  * pm_ln_space_to_depth LayerNorm + the 2 x 2 / stride-2 patch gather of the downsample (convnext.py:47-52), so that its
//                         Conv2d(C, 2C, 2, 2) is one GEMM with K = 4C;
//  * pm_convnext_stem     Conv2d(3, d, 4, 4) + bias + LayerNorm on fp32 NCHW images (convnext.py:41);
//  * pm_mean_ln           AdaptiveAvgPool2d(1) + LayerNorm of the head (convnext.py:67-68).
// The pointwise MLP runs on the tile GEMMs (linear_bf16*.hip / linear_f32.hip).
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ f32x4 ld4(const T* p);
template <>
__device__ __forceinline__ f32x4 ld4<float>(const float* p) {
  return *(const f32x4*)p;
}
template <>
__device__ __forceinline__ f32x4 ld4<bf16>(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(bf16* p, f32x4 v) {
  *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16* p) { return (float)*p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16* p, float v) { *p = (bf16)v; }

template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WIDTH);
  return v;
}

// ------------------------------------------------------------------------------------------------ depthwise 7 x 7 + LayerNorm
// A workgroup owns `sblk` strips of SW consecutive pixels of one image row, every channel of them.
// Phase 1: work item (strip, channel quad) - a thread slides the 7 x 7 window along its strip: per kernel row it loads SW + 6
//   input quads once and uses each for up to 7 outputs (12.25 quad loads per output quad at SW = 8 instead of 49); the halo
//   rows come from L1 / L2 (neighbouring workgroups read the same rows).  The conv outputs (+ bias) go to LDS as f32.
// Phase 2: 16 lanes per pixel - two-pass mean / variance over the pixel's C values in LDS, then the normalised row and the
//   zero columns C .. ldy - 1 (the bf16 GEMM behind it needs K % 64 == 0) are written once.
constexpr int DW_THREADS = 256;

template <typename TX, typename TY, int SW>
__global__ __launch_bounds__(DW_THREADS) void dwconv7_ln_kernel(const TX* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, TY* __restrict__ y,
                                                                int64_t ldy, int H, int W, int C, int spr, int64_t nstrips,
                                                                int sblk) {
  extern __shared__ f32x4 dw_lds[];  // (sblk * SW pixels, C / 4 quads)
  const int C4 = C >> 2;
  const int64_t s0 = (int64_t)blockIdx.x * sblk;
  const int items = sblk * C4;
  for (int it = threadIdx.x; it < items; it += DW_THREADS) {
    const int sl = it / C4, q = it - sl * C4;
    const int64_t s = s0 + sl;
    if (s >= nstrips) break;  // items are ordered by strip
    const int64_t row = s / spr;  // n * H + h
    const int w0 = (int)(s - row * spr) * SW;
    const int h = (int)(row % H);
    const TX* ximg = x + (row - h) * W * C + q * 4;
    const f32x4 b = *(const f32x4*)(bias + q * 4);
    f32x4 acc[SW];
#pragma unroll
    for (int j = 0; j < SW; ++j) acc[j] = b;
#pragma unroll
    for (int kr = 0; kr < 7; ++kr) {
      const int ih = h + kr - 3;
      if (ih < 0 || ih >= H) continue;
      const TX* xr = ximg + (int64_t)ih * W * C;
      f32x4 in[SW + 6];
#pragma unroll
      for (int j = 0; j < SW + 6; ++j) {
        const int iw = w0 + j - 3;
        in[j] = (iw >= 0 && iw < W) ? ld4(xr + (int64_t)iw * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kc = 0; kc < 7; ++kc) {
        const f32x4 wq = *(const f32x4*)(w + (kr * 7 + kc) * C + q * 4);
#pragma unroll
        for (int j = 0; j < SW; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[j + kc][e], wq[e], acc[j][e]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SW; ++j) dw_lds[(sl * SW + j) * C4 + q] = acc[j];
  }
  __syncthreads();

  const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int ldy4 = (int)(ldy >> 2);
  const float inv_c = 1.0f / (float)C;
  for (int p = grp; p < sblk * SW; p += DW_THREADS / 16) {  // uniform over each 16-lane group
    const int sl = p / SW, j = p - sl * SW;
    const int64_t s = s0 + sl;
    if (s >= nstrips) break;
    const int64_t row = s / spr;
    const int wcol = (int)(s - row * spr) * SW + j;
    if (wcol >= W) continue;
    const f32x4* v = dw_lds + p * C4;
    float sum = 0.f;
    for (int q = l16; q < C4; q += 16) {
      const f32x4 a = v[q];
      sum += (a[0] + a[1]) + (a[2] + a[3]);
    }
    const float mean = group_sum<16>(sum) * inv_c;
    float sq = 0.f;
    for (int q = l16; q < C4; q += 16) {
      const f32x4 a = v[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) sq = fmaf(a[e] - mean, a[e] - mean, sq);
    }
    const float rstd = rsqrtf(group_sum<16>(sq) * inv_c + eps);
    TY* yr = y + (row * W + wcol) * ldy;
    for (int q = l16; q < ldy4; q += 16) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (q < C4) {
        const f32x4 a = v[q], g = *(const f32x4*)(gamma + q * 4), bb = *(const f32x4*)(beta + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf((a[e] - mean) * rstd, g[e], bb[e]);
      }
      st4(yr + q * 4, o);
    }
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm + space-to-depth
// One wave per output row (n, i, j): the four pixels (2i, 2j), (2i, 2j + 1), (2i + 1, 2j), (2i + 1, 2j + 1) normalised and laid
// side by side (the Conv2d(C, 2C, 2, 2) weight permuted to (Cout, kh, kw, Cin) is then the GEMM's (N, K) operand), zeros after.
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void ln_s2d_kernel(const TX* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, TY* __restrict__ y, int64_t ldy,
                                                     int64_t M, int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const int Wo = W >> 1, Ho = H >> 1;
  const int jo = (int)(r % Wo);
  const int64_t t = r / Wo;
  const int io = (int)(t % Ho);
  const int64_t n = t / Ho;
  const float inv_c = 1.0f / (float)C;
  TY* yr = y + r * ldy;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const TX* xp = x + ((n * H + 2 * io + (k >> 1)) * W + 2 * jo + (k & 1)) * ldx;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += ld1(xp + c);
    const float mean = group_sum<64>(sum) * inv_c;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float d = ld1(xp + c) - mean;
      sq = fmaf(d, d, sq);
    }
    const float rstd = rsqrtf(group_sum<64>(sq) * inv_c + eps);
    for (int c = lane; c < C; c += 64) st1(yr + k * C + c, fmaf((ld1(xp + c) - mean) * rstd, gamma[c], beta[c]));
  }
  for (int64_t c = 4 * (int64_t)C + lane; c < ldy; c += 64) st1(yr + c, 0.f);
}

// ------------------------------------------------------------------------------------------------ stem: 4 x 4 patchify + LN
// One wave per SP consecutive output pixels of an image row; lane l owns channels l, l + 64, ... (NCH of them).  The SP patches
// (48 floats each) are staged through LDS and read back as broadcasts; the weight is the derived (48, d) transpose, so a k step
// reads one coalesced row of it for all SP pixels.  fp32 fma in k order on the VALU (~7 GFLOP at ConvNeXt-T, batch 256, 224^2).
constexpr int STEM_SP = 8;

template <typename TY, int NCH>
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ img, const float* __restrict__ wt,
                                                   const float* __restrict__ bias, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, TY* __restrict__ y, int64_t ldy,
                                                   int64_t ngroups, int Hi, int Wi, int d) {
  __shared__ float patch[4][STEM_SP * 48];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t g0 = (int64_t)blockIdx.x * 4 + wv;
  const bool live = g0 < ngroups;
  const int64_t g = live ? g0 : ngroups - 1;
  const int Ho = Hi >> 2, Wo = Wi >> 2, gpr = (Wo + STEM_SP - 1) / STEM_SP;
  const int jo0 = (int)(g % gpr) * STEM_SP;
  const int64_t t = g / gpr;
  const int io = (int)(t % Ho);
  const int64_t n = t / Ho;
  float* pw = patch[wv];
  for (int e = lane; e < STEM_SP * 48; e += 64) {
    const int p = e / 48, k = e - p * 48;
    const int ci = k >> 4, kh = (k >> 2) & 3, kw = k & 3;
    const int jo = jo0 + p < Wo ? jo0 + p : Wo - 1;  // a ragged group repeats its last pixel (not stored)
    pw[e] = img[((n * 3 + ci) * Hi + 4 * io + kh) * (int64_t)Wi + 4 * jo + kw];
  }
  __syncthreads();
  if (!live) return;
  float acc[STEM_SP][NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    const float b = c < d ? bias[c] : 0.f;
#pragma unroll
    for (int p = 0; p < STEM_SP; ++p) acc[p][i] = b;
  }
#pragma unroll 4
  for (int k = 0; k < 48; ++k) {
    float wk[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      wk[i] = c < d ? wt[k * d + c] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < STEM_SP; ++p) {
      const float v = pw[p * 48 + k];
#pragma unroll
      for (int i = 0; i < NCH; ++i) acc[p][i] = fmaf(v, wk[i], acc[p][i]);
    }
  }
  const float inv_d = 1.0f / (float)d;
#pragma unroll
  for (int p = 0; p < STEM_SP; ++p) {
    if (jo0 + p >= Wo) break;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) sum += lane + 64 * i < d ? acc[p][i] : 0.f;
    const float mean = group_sum<64>(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const float dv = acc[p][i] - mean;
      sq = lane + 64 * i < d ? fmaf(dv, dv, sq) : sq;
    }
    const float rstd = rsqrtf(group_sum<64>(sq) * inv_d + eps);
    TY* yr = y + ((n * Ho + io) * Wo + jo0 + p) * ldy;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < d) st1(yr + c, fmaf((acc[p][i] - mean) * rstd, gamma[c], beta[c]));
    }
    for (int64_t c = d + lane; c < ldy; c += 64) st1(yr + c, 0.f);
  }
}

// ------------------------------------------------------------------------------------------------ head: mean over pixels + LN
// One workgroup per image: per-channel means over the HW rows into LDS (coalesced across channels), then a two-pass LayerNorm.
template <int T>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = group_sum<64>(v);
  __syncthreads();  // red is reused between calls
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < T / 64; ++i) s += red[i];
  return s;
}

template <typename TX, typename TY>
__global__ __launch_bounds__(256) void mean_ln_kernel(const TX* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, TY* __restrict__ y, int HW,
                                                      int C) {
  extern __shared__ float mln_lds[];  // C means, then 4 partial sums
  float* red = mln_lds + C;
  const int64_t n = blockIdx.x;
  const TX* xi = x + n * HW * ldx;
  const float inv_hw = 1.0f / (float)HW, inv_c = 1.0f / (float)C;
  float part = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int r = 0; r < HW; ++r) s += ld1(xi + (int64_t)r * ldx + c);
    s *= inv_hw;
    mln_lds[c] = s;
    part += s;
  }
  const float mean = block_sum<256>(part, red) * inv_c;
  float sq = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float dv = mln_lds[c] - mean;
    sq = fmaf(dv, dv, sq);
  }
  const float rstd = rsqrtf(block_sum<256>(sq, red) * inv_c + eps);
  for (int c = threadIdx.x; c < C; c += 256) st1(y + n * C + c, fmaf((mln_lds[c] - mean) * rstd, gamma[c], beta[c]));
}

bool aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

extern "C" int pm_dwconv7_ln(const void* x, int x_dtype, const float* w, const float* bias, const float* gamma, const float* beta,
                             float eps, void* y, int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                             void* stream) {
  if (!x || !w || !bias || !gamma || !beta || !y || N < 0 || H <= 0 || W <= 0 || C <= 0 || ldy < C) return PM_EINVAL;
  if ((x_dtype != PM_BF16 && x_dtype != PM_F32) || (y_dtype != PM_BF16 && y_dtype != PM_F32)) return PM_EINVAL;
  if (C % 4 || ldy % 4 || C > 4096 || H > (1 << 20) || W > (1 << 20)) return PM_EUNSUPPORTED;
  const int xs = x_dtype == PM_F32 ? 16 : 8, ys = y_dtype == PM_F32 ? 16 : 8;
  if (!aligned(x, xs) || !aligned(y, ys) || !aligned(w, 16) || !aligned(bias, 16) || !aligned(gamma, 16) || !aligned(beta, 16))
    return PM_EALIGN;
  if (N == 0) return PM_OK;
  const int SW = C <= 2048 ? 8 : 4;
  const int spr = (int)((W + SW - 1) / SW);
  const int64_t nstrips = N * H * spr;
  const int C4 = (int)(C / 4);
  // about one work item per thread, at most 32 KiB of LDS (64 KiB for one strip of a wide C): 4-5 workgroups per CU
  int sblk = (DW_THREADS + C4 - 1) / C4;
  const int cap = (int)(8192 / (SW * C));
  sblk = sblk < cap ? sblk : cap;
  sblk = sblk < 1 ? 1 : sblk;
  const int64_t nblk = (nstrips + sblk - 1) / sblk;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  const size_t lds = (size_t)sblk * SW * C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define PM_DWGO(TX, TY, S)                                                                                                   \
  hipLaunchKernelGGL((dwconv7_ln_kernel<TX, TY, S>), dim3((unsigned)nblk), dim3(DW_THREADS), lds, st, (const TX*)x, w, bias, \
                     gamma, beta, eps, (TY*)y, ldy, (int)H, (int)W, (int)C, spr, nstrips, sblk)
#define PM_DWSW(TX, TY) \
  if (SW == 8)          \
    PM_DWGO(TX, TY, 8); \
  else                  \
    PM_DWGO(TX, TY, 4)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_DWSW(float, float); else PM_DWSW(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_DWSW(bf16, float); else PM_DWSW(bf16, bf16);
  }
#undef PM_DWSW
#undef PM_DWGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_ln_space_to_depth(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps,
                                    void* y, int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                                    void* stream) {
  if (!x || !gamma || !beta || !y || N < 0 || H <= 0 || W <= 0 || C <= 0 || ldx < C || ldy < 4 * C) return PM_EINVAL;
  if ((x_dtype != PM_BF16 && x_dtype != PM_F32) || (y_dtype != PM_BF16 && y_dtype != PM_F32)) return PM_EINVAL;
  if (H % 2 || W % 2 || H > (1 << 20) || W > (1 << 20) || C > (1 << 24)) return PM_EUNSUPPORTED;
  const int64_t M = N * (H / 2) * (W / 2);
  if (M == 0) return PM_OK;
  const int64_t nblk = (M + 3) / 4;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_S2DGO(TX, TY)                                                                                               \
  hipLaunchKernelGGL((ln_s2d_kernel<TX, TY>), dim3((unsigned)nblk), dim3(256), 0, st, (const TX*)x, ldx, gamma, beta, eps, \
                     (TY*)y, ldy, M, (int)H, (int)W, (int)C)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_S2DGO(float, float); else PM_S2DGO(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_S2DGO(bf16, float); else PM_S2DGO(bf16, bf16);
  }
#undef PM_S2DGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_convnext_stem(const float* imgs, const float* wt, const float* bias, const float* gamma, const float* beta,
                                float eps, void* y, int64_t ldy, int y_dtype, int64_t N, int64_t Himg, int64_t Wimg, int64_t d,
                                void* stream) {
  if (!imgs || !wt || !bias || !gamma || !beta || !y || N < 0 || d <= 0 || ldy < d) return PM_EINVAL;
  if (y_dtype != PM_BF16 && y_dtype != PM_F32) return PM_EINVAL;
  if (Himg < 4 || Wimg < 4 || Himg > (1 << 20) || Wimg > (1 << 20) || d > 384) return PM_EUNSUPPORTED;
  const int64_t Ho = Himg / 4, Wo = Wimg / 4;
  const int64_t ngroups = N * Ho * ((Wo + STEM_SP - 1) / STEM_SP);
  if (ngroups == 0) return PM_OK;
  const int64_t nblk = (ngroups + 3) / 4;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nch = (int)((d + 63) / 64);
#define PM_STEMGO(TY, K)                                                                                                     \
  hipLaunchKernelGGL((stem_kernel<TY, K>), dim3((unsigned)nblk), dim3(256), 0, st, imgs, wt, bias, gamma, beta, eps, (TY*)y, \
                     ldy, ngroups, (int)Himg, (int)Wimg, (int)d)
#define PM_STEMNCH(TY)                 \
  switch (nch) {                       \
    case 1: PM_STEMGO(TY, 1); break;   \
    case 2: PM_STEMGO(TY, 2); break;   \
    case 3: PM_STEMGO(TY, 3); break;   \
    case 4: PM_STEMGO(TY, 4); break;   \
    case 5: PM_STEMGO(TY, 5); break;   \
    default: PM_STEMGO(TY, 6); break;  \
  }
  if (y_dtype == PM_F32) {
    PM_STEMNCH(float)
  } else {
    PM_STEMNCH(bf16)
  }
#undef PM_STEMNCH
#undef PM_STEMGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_mean_ln(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps, void* y,
                          int y_dtype, int64_t N, int64_t HW, int64_t C, void* stream) {
  if (!x || !gamma || !beta || !y || N < 0 || HW <= 0 || C <= 0 || ldx < C) return PM_EINVAL;
  if ((x_dtype != PM_BF16 && x_dtype != PM_F32) || (y_dtype != PM_BF16 && y_dtype != PM_F32)) return PM_EINVAL;
  if (C > 16000 || HW > (1 << 30) || N > 0x7fffffff) return PM_EUNSUPPORTED;
  if (N == 0) return PM_OK;
  const size_t lds = (size_t)(C + 4) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define PM_MLNGO(TX, TY)                                                                                                     \
  hipLaunchKernelGGL((mean_ln_kernel<TX, TY>), dim3((unsigned)N), dim3(256), lds, st, (const TX*)x, ldx, gamma, beta, eps, \
                     (TY*)y, (int)HW, (int)C)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_MLNGO(float, float); else PM_MLNGO(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_MLNGO(bf16, float); else PM_MLNGO(bf16, bf16);
  }
#undef PM_MLNGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}
