// resnet.hip - the ResNet bottleneck backbone of DETR (reference: pytorch_models/image/detr.py:11-61), NHWC bf16 rows:
//  * pm_conv_bf16     implicit-GEMM convolution on the bf16 MFMA: 3 x 3 pad 1 or 1 x 1 pad 0, stride 1 or 2, Cin % 64 == 0,
//                     eval BatchNorm folded into weight and bias by the caller, epilogue relu?(acc + bias [+ resid]) - the
//                     ReLU AFTER the residual add, which is what Bottleneck.forward needs (detr.py:33);
//  * pm_resnet_stem   MaxPool2d(3, 2, 1)(relu(bn(Conv2d(3, 64, 7, 2, 3)))) from f32 NCHW images (detr.py:40-45): fp32 fma on
//                     the VALU into a bf16 NHWC map, then a 3 x 3 / 2 max over it (two kernels, see below).
// The plain 1 x 1 + ReLU convolutions are rows x weights and run on pm_linear_bf16.
//
// pm_conv_bf16.  GEMM view: rows = the N*Ho*Wo output pixels, columns = Cout, K = (kh, kw, Cin) in the weight's own order
// (Cout, kh, kw, Cin), cut into steps of 64 channels of ONE tap (Cin % 64 == 0), so a K step of a pixel row is 128 contiguous
// bytes of the NHWC input at (oh*stride + kh - pad, ow*stride + kw - pad) - or zeros outside the image.  Nothing like an im2col
// buffer exists: every thread gathers its 16-byte chunks of the pixel tile from global into registers (zero where the tap falls
// outside), and writes them to LDS behind the arithmetic of the current step.
//   tile        128 pixels x BN channels (BN = 128, or 64 when Cout <= 64) x 64 of K, 4 waves as 2 (pixels) x 2 (channels);
//   LDS         two stages of (128 + BN) rows of 128 bytes, 16-byte chunks XOR-swizzled (swz_pos, common.h): the 16-row x
//               4-chunk fragment reads of MFMA 16x16x32 are conflict-free; one barrier per K step;
//   MFMA        16x16x32 with A = 16 weight rows, B = 16 pixel rows: the accumulator holds the PIXEL on the lane (l & 15) and
//               4 consecutive channels 4 (l >> 4) + r, so bias / residual / ReLU / rounding happen in place on 8-byte cells;
//   epilogue    Cout % 8 == 0: the cells live in LDS - the residual tile comes in and the output tile leaves as 16-byte chunks
//               of whole row segments; otherwise straight from the accumulators (8-byte stores, element-wise if Cout % 4 != 0);
//   edges       pixel rows >= M gather zeros and are not stored; weight rows >= Cout are clamped and not stored.
#include "common.h"

namespace {

constexpr int CV_BM = 128, CV_BK = 64;

__device__ __forceinline__ bf16x8 cv_read(const char* tile, int row, int chunk) {
  return *(const bf16x8*)(tile + row * 128 + swz_pos(row, chunk) * 16);
}

template <int BN, bool RES, bool RELU>
__global__ __launch_bounds__(256) void conv_bf16_kernel(const bf16* __restrict__ X, const bf16* __restrict__ Wt,
                                                        const float* __restrict__ bias, const bf16* __restrict__ resid,
                                                        bf16* __restrict__ Y, int M, int H, int W, int Cin, int Ho, int Wo,
                                                        int Cout, int ksz, int stride, int pad, int tiles_n) {
  constexpr int STAGE = (CV_BM + BN) * 128;
  constexpr int NBJ = BN / 32;   // 16-channel blocks per wave
  constexpr int BROWS = BN / 32;  // weight rows staged per thread
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int tn = blockIdx.x % tiles_n, tm = blockIdx.x / tiles_n;
  const int cpt = Cin / CV_BK;          // K steps per tap
  const int nk = ksz * ksz * cpt;
  const int64_t Ktot = (int64_t)ksz * ksz * Cin;

  // staging geometry: this thread's chunk (tid & 7) of pixel rows (tid >> 3) + 32 i and of weight rows (tid >> 3) + 32 i
  const int srow = tid >> 3, chunk = tid & 7;
  int ih0[4], iw0[4];
  int64_t pix0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = tm * CV_BM + srow + 32 * i;
    if (m < M) {
      const int n = m / (Ho * Wo), rem = m - n * (Ho * Wo);
      const int oh = rem / Wo, ow = rem - oh * Wo;
      ih0[i] = oh * stride - pad;
      iw0[i] = ow * stride - pad;
      pix0[i] = (int64_t)n * H * W;
    } else {
      ih0[i] = -(1 << 24);  // every tap falls outside: zeros
      iw0[i] = 0;
      pix0[i] = 0;
    }
  }
  const bf16* wrow[BROWS];
#pragma unroll
  for (int i = 0; i < BROWS; ++i) {
    int n = tn * BN + srow + 32 * i;
    n = n < Cout ? n : Cout - 1;
    wrow[i] = Wt + (int64_t)n * Ktot + chunk * 8;
  }
  bf16x8 areg[4], breg[BROWS];
  auto load_regs = [&](int kt) {
    const int tap = kt / cpt, c0 = (kt - tap * cpt) * CV_BK;
    const int kh = tap / ksz, kw = tap - kh * ksz;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ih = ih0[i] + kh, iw = iw0[i] + kw;
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
        areg[i] = *(const bf16x8*)(X + (pix0[i] + (int64_t)ih * W + iw) * Cin + c0 + chunk * 8);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) areg[i][e] = (bf16)0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) breg[i] = *(const bf16x8*)(wrow[i] + (int64_t)kt * CV_BK);
  };
  auto write_lds = [&](int stage) {
    char* at = smem + stage * STAGE;
    char* bt = at + CV_BM * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 32 * i;
      *(bf16x8*)(at + r * 128 + swz_pos(r, chunk) * 16) = areg[i];
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      const int r = srow + 32 * i;
      *(bf16x8*)(bt + r * 128 + swz_pos(r, chunk) * 16) = breg[i];
    }
  };

  f32x4 acc[4][NBJ];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < NBJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  load_regs(0);
  write_lds(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();  // stage kt & 1 is complete; nobody still reads the other stage (step kt - 1)
    if (kt + 1 < nk) load_regs(kt + 1);
    const char* at = smem + (kt & 1) * STAGE;
    const char* bt = at + CV_BM * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[NBJ], b[4];
#pragma unroll
      for (int j = 0; j < NBJ; ++j) a[j] = cv_read(bt, wn * (BN / 2) + 16 * j + i16, 4 * ks + g);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = cv_read(at, wm * 64 + 16 * i + i16, 4 * ks + g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < NBJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[i][j], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) write_lds((kt + 1) & 1);
  }

  if ((Cout & 7) == 0) {
    // Epilogue through LDS: the residual tile comes in and the output tile goes out as 16-byte chunks of whole row segments
    // (BN * 2 bytes contiguous per pixel); in between, each lane finishes its own 8-byte cells (4 channels of one pixel) in
    // place, in the accumulator layout.  Rows of EP_LD bytes: the 8-byte cell accesses of a half wave fall on distinct banks.
    constexpr int EP_LD = BN * 2 + 16;
    constexpr int CPR = BN / 8;  // 16-byte chunks per tile row
    static_assert(CV_BM * EP_LD <= 2 * STAGE, "the epilogue tile fits in the K loop's LDS");
    __syncthreads();  // the last K step's fragment reads are done
    if (RES) {
      for (int c = tid; c < CV_BM * CPR; c += 256) {
        const int r = c / CPR, q = c - r * CPR;
        const int m = tm * CV_BM + r, ch = tn * BN + q * 8;
        if (m < M && ch < Cout) *(bf16x8*)(smem + r * EP_LD + q * 16) = *(const bf16x8*)(resid + (int64_t)m * Cout + ch);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wm * 64 + 16 * i + i16;
#pragma unroll
      for (int j = 0; j < NBJ; ++j) {
        const int cl = wn * (BN / 2) + 16 * j + 4 * g;
        const int ch = tn * BN + cl;
        if (tm * CV_BM + r >= M || ch >= Cout) continue;
        f32x4 v = acc[i][j];
        if (bias) {
          const f32x4 bv = *(const f32x4*)(bias + ch);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bv[e];
        }
        bf16x4* cell = (bf16x4*)(smem + r * EP_LD + cl * 2);
        if (RES) {
          const bf16x4 rv = *cell;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
        }
        if (RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        *cell = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
      }
    }
    __syncthreads();
    for (int c = tid; c < CV_BM * CPR; c += 256) {
      const int r = c / CPR, q = c - r * CPR;
      const int m = tm * CV_BM + r, ch = tn * BN + q * 8;
      if (m < M && ch < Cout) *(bf16x8*)(Y + (int64_t)m * Cout + ch) = *(const bf16x8*)(smem + r * EP_LD + q * 16);
    }
    return;
  }
  // Cout % 8 != 0: straight from the accumulators (8-byte stores, or element-wise when Cout % 4 != 0)
  const bool vec = (Cout & 3) == 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = tm * CV_BM + wm * 64 + 16 * i + i16;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NBJ; ++j) {
      const int ch = tn * BN + wn * (BN / 2) + 16 * j + 4 * g;
      if (ch >= Cout) continue;
      const int64_t off = (int64_t)m * Cout + ch;
      f32x4 v = acc[i][j];
      if (vec) {
        if (bias) {
          const f32x4 bv = *(const f32x4*)(bias + ch);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bv[r];
        }
        if (RES) {
          const bf16x4 rv = *(const bf16x4*)(resid + off);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
        }
        if (RELU) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        *(bf16x4*)(Y + off) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (ch + r < Cout) {
            float u = v[r] + (bias ? bias[ch + r] : 0.f);
            if (RES) u += (float)resid[off + r];
            if (RELU) u = fmaxf(u, 0.f);
            Y[off + r] = (bf16)u;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stem: conv 7 x 7 / 2 + BN + ReLU
// Thread = one output pixel x SC_CH channels; the channel group is blockIdx.y, i.e. uniform over the workgroup, so the weights
// of a tap are scalar loads shared by every lane and the inner loop is one image load + SC_CH v_fma with a scalar operand.
// Lanes are neighbouring output columns: their 7-wide input windows overlap, the loads hit the L1.  SC_CH = 64 (all channels in
// one thread): the image value and its bounds test are paid once per 64 fma.
constexpr int SC_CH = 64;
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ imgs, const float* __restrict__ wt,
                                                        const float* __restrict__ shift, bf16* __restrict__ y, int64_t npix,
                                                        int Himg, int Wimg, int Hc, int Wc) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int cg = blockIdx.y;
  const int ow = (int)(p % Wc);
  const int64_t t = p / Wc;
  const int oh = (int)(t % Hc);
  const int64_t n = t / Hc;
  float acc[SC_CH];
#pragma unroll
  for (int e = 0; e < SC_CH; ++e) acc[e] = shift[cg * SC_CH + e];
  const float* wg = wt + cg * SC_CH;
  for (int c = 0; c < 3; ++c) {
    const float* plane = imgs + (n * 3 + c) * (int64_t)Himg * Wimg;
    for (int kh = 0; kh < 7; ++kh) {
      const int ih = 2 * oh + kh - 3;
      const bool rv = ih >= 0 && ih < Himg;
      const float* row = plane + (int64_t)(rv ? ih : 0) * Wimg;
      float xv[7];
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const int iw = 2 * ow + kw - 3;
        xv[kw] = (rv && iw >= 0 && iw < Wimg) ? row[iw] : 0.f;
      }
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const float* w = wg + ((c * 7 + kh) * 7 + kw) * 64;
#pragma unroll
        for (int e = 0; e < SC_CH; ++e) acc[e] = fmaf(xv[kw], w[e], acc[e]);
      }
    }
  }
  bf16* o = y + p * 64 + cg * SC_CH;
#pragma unroll
  for (int q = 0; q < SC_CH / 8; ++q) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)fmaxf(acc[8 * q + e], 0.f);
    *(bf16x8*)(o + 8 * q) = v;
  }
}

// MaxPool2d(3, 2, 1) on the bf16 NHWC map (rounding to bf16 is monotonic: the max of the rounded values is the rounded max).
__global__ __launch_bounds__(256) void stem_pool_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int64_t nitems, int Hc,
                                                        int Wc, int Hp, int Wp) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  const int c8 = (int)(it & 7);
  const int64_t p = it >> 3;
  const int pw = (int)(p % Wp);
  const int64_t t = p / Wp;
  const int ph = (int)(t % Hp);
  const int64_t n = t / Hp;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * ph + kh - 1;
    if (ih < 0 || ih >= Hc) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = 2 * pw + kw - 1;
      if (iw < 0 || iw >= Wc) continue;
      const bf16x8 v = *(const bf16x8*)(x + ((n * Hc + ih) * (int64_t)Wc + iw) * 64 + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
    }
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16)m[e];
  *(bf16x8*)(y + p * 64 + c8 * 8) = o;
}

bool rn_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

template <int BN>
int conv_launch(const bf16* x, const bf16* w, const float* bias, const bf16* resid, bf16* y, int M, int H, int W, int Cin, int Ho,
                int Wo, int Cout, int ksz, int stride, int pad, int relu, hipStream_t st) {
  const int tiles_n = (Cout + BN - 1) / BN;
  const int64_t nblk = (int64_t)((M + CV_BM - 1) / CV_BM) * tiles_n;
  if (nblk > 0x7fffffff) return PM_EINVAL;
#define PM_CVGO(RES, RELU)                                                                                                  \
  hipLaunchKernelGGL((conv_bf16_kernel<BN, RES, RELU>), dim3((unsigned)nblk), dim3(256), 0, st, x, w, bias, resid, y, M, H, W, \
                     Cin, Ho, Wo, Cout, ksz, stride, pad, tiles_n)
  if (resid) {
    if (relu) PM_CVGO(true, true);
    else PM_CVGO(true, false);
  } else {
    if (relu) PM_CVGO(false, true);
    else PM_CVGO(false, false);
  }
#undef PM_CVGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

}  // namespace

extern "C" int pm_conv_bf16(const void* x, int64_t N, int64_t H, int64_t W, int64_t Cin, const void* w, const float* bias,
                            const void* resid, void* y, int64_t Cout, int64_t ksize, int64_t stride, int relu, void* stream) {
  if (!x || !w || !y || N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return PM_EINVAL;
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || Cin % 64) return PM_EUNSUPPORTED;
  if (H > (1 << 20) || W > (1 << 20) || Cin > (1 << 16) || Cout > (1 << 16)) return PM_EUNSUPPORTED;
  const int64_t pad = ksize == 3 ? 1 : 0;
  const int64_t Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
  const int64_t M = N * Ho * Wo;
  if (M >= (1LL << 31) - CV_BM || N * H * W >= (1LL << 31)) return PM_EUNSUPPORTED;
  if (!rn_aligned(x, 16) || !rn_aligned(w, 16) || (bias && !rn_aligned(bias, 16)) || (resid && !rn_aligned(resid, 16)) ||
      !rn_aligned(y, 16))
    return PM_EALIGN;
  if (M == 0) return PM_OK;
  hipStream_t st = (hipStream_t)stream;
  if (Cout <= 64)
    return conv_launch<64>((const bf16*)x, (const bf16*)w, bias, (const bf16*)resid, (bf16*)y, (int)M, (int)H, (int)W, (int)Cin,
                           (int)Ho, (int)Wo, (int)Cout, (int)ksize, (int)stride, (int)pad, relu, st);
  return conv_launch<128>((const bf16*)x, (const bf16*)w, bias, (const bf16*)resid, (bf16*)y, (int)M, (int)H, (int)W, (int)Cin,
                          (int)Ho, (int)Wo, (int)Cout, (int)ksize, (int)stride, (int)pad, relu, st);
}

extern "C" int pm_resnet_stem(const float* imgs, const float* wt, const float* shift, void* conv_map, void* y, int64_t N,
                              int64_t Himg, int64_t Wimg, void* stream) {
  if (!imgs || !wt || !shift || !conv_map || !y || N < 0 || Himg <= 0 || Wimg <= 0) return PM_EINVAL;
  if (Himg > (1 << 20) || Wimg > (1 << 20)) return PM_EUNSUPPORTED;
  if (!rn_aligned(conv_map, 16) || !rn_aligned(y, 16)) return PM_EALIGN;
  const int64_t Hc = (Himg - 1) / 2 + 1, Wc = (Wimg - 1) / 2 + 1;
  const int64_t Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  const int64_t npix = N * Hc * Wc, nitems = N * Hp * Wp * 8;
  if (npix == 0) return PM_OK;
  const int64_t nb1 = (npix + 255) / 256, nb2 = (nitems + 255) / 256;
  if (nb1 > 0x7fffffff || nb2 > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)nb1, 64 / SC_CH), dim3(256), 0, st, imgs, wt, shift, (bf16*)conv_map, npix,
                     (int)Himg, (int)Wimg, (int)Hc, (int)Wc);
  PM_CHECK_LAUNCH();
  hipLaunchKernelGGL(stem_pool_kernel, dim3((unsigned)nb2), dim3(256), 0, st, (const bf16*)conv_map, (bf16*)y, nitems, (int)Hc,
                     (int)Wc, (int)Hp, (int)Wp);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
