// maxvit.hip - the MaxViT-specific stages (reference: pytorch_models/image/maxvit.py), NHWC rows, fp32 arithmetic, bf16 or f32
// at the edges:
//  * pm_window_attention_bf16  softmax(q k^T / sqrt(32) + bias[h]) v over the 7 x 7 blocks / dilated grids of an NHWC image,
//                              read straight out of the packed QKV rows (maxvit.py:70-91 block / grid, 94-112 RelativeMHA);
//  * pm_dwconv3_bn_act         the MBConv depthwise 3 x 3 (stride 1 or 2, the reference's padding) + folded BatchNorm +
//                              GELU-tanh, optionally gated per (image, channel) and / or emitting per-row channel sums
//                              (maxvit.py:27-31, 52 and the squeeze-excitation's pool, 36);
//  * pm_se_gate                mean -> Conv1x1 + SiLU -> Conv1x1 + sigmoid of the squeeze-excitation (maxvit.py:34-44);
//  * pm_maxvit_stem            Conv2d(3, s, 3, 2) + BatchNorm + GELU-tanh on fp32 NCHW images (maxvit.py:150-153);
//  * pm_im2col3x3_nhwc         pad-1 3 x 3 patches, so the stem's second Conv2d(s, s, 3) is one GEMM (maxvit.py:154);
//  * pm_avgpool2x2_nhwc        the MBConv shortcut's AvgPool2d(2) (maxvit.py:59-60).
// The 1 x 1 convolutions, projections and MLPs run on the GEMMs (linear_bf16*.hip / linear_f32.hip).
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ f32x4 mv_ld4(const T* p);
template <>
__device__ __forceinline__ f32x4 mv_ld4<float>(const float* p) {
  return *(const f32x4*)p;
}
template <>
__device__ __forceinline__ f32x4 mv_ld4<bf16>(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void mv_st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void mv_st4(bf16* p, f32x4 v) {
  *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
__device__ __forceinline__ void mv_st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void mv_st1(bf16* p, float v) { *p = (bf16)v; }

__device__ __forceinline__ float gelu_tanh(float x) { return apply_act<PM_ACT_GELU_TANH, true>(x); }

bool mv_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// ------------------------------------------------------------------------------------------------ window attention, head dim 32
// One wave per (window, head); heads are the fastest index of the wave id, so the four waves of a workgroup fetch the same
// tokens' rows for four heads at once (grid-mode tokens are scattered pixels, but each token row of 3d bf16 is >= 384 B).
// L = ws * ws <= 64 tokens, one padded key tile of 64:
//   S^T = K Q^T : MFMA 16x16x32 (k = the 32 head dims in one step), A = 16 key rows, B = 16 query rows, both 16-byte fragments
//                 read straight from global.  The accumulator has the QUERY on the lane (l & 15) and keys 4(l >> 4) + i.
//   softmax     : in-lane over 16 keys, then across the four 16-lane groups (xor 16, 32); keys >= L are -inf (P = 0).
//   O^T = V^T P^T: the S^T accumulators of key blocks (2c, 2c + 1), converted to bf16, ARE the B operand of k-chunk c
//                 (element j of lane group g = key 16(2c + (j >> 2)) + 4g + (j & 3)); the A operand V^T takes the same keys
//                 from a row-major V image in LDS whose rows >= L are zero (a P = 0 times a NaN would still be a NaN).
//   O^T has the query on the lane again: one division by the lane's row sum, 8-byte stores of 4 dims.
constexpr int WA_WAVES = 4;

template <bool GRID>
__device__ __forceinline__ int64_t wa_pixel_row(int t, int ws, int64_t n, int wy, int wx, int nWy, int nWx, int Himg, int Wimg) {
  const int r = t / ws, c = t - r * ws;
  const int py = GRID ? r * nWy + wy : wy * ws + r;
  const int px = GRID ? c * nWx + wx : wx * ws + c;
  return (n * Himg + py) * (int64_t)Wimg + px;
}

template <bool GRID>
__global__ __launch_bounds__(64 * WA_WAVES) void window_attn_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                                    const bf16* __restrict__ V, int64_t ld, bf16* __restrict__ O,
                                                                    int64_t ldo, const float* __restrict__ bias, int64_t nwork,
                                                                    int H, int Himg, int Wimg, int ws, float scale_log2) {
  __shared__ __attribute__((aligned(16))) bf16 vlds[WA_WAVES][64 * 32];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * WA_WAVES + wave;
  const bool live = gw < nwork;
  const int64_t gwc = live ? gw : nwork - 1;
  const int h = (int)(gwc % H);
  const int64_t win = gwc / H;
  const int nWy = Himg / ws, nWx = Wimg / ws;
  const int wx = (int)(win % nWx);
  const int64_t t1 = win / nWx;
  const int wy = (int)(t1 % nWy);
  const int64_t n = t1 / nWy;
  const int L = ws * ws;
  const int i16 = lane & 15, g = lane >> 4;
  const int hoff = h * 32;

  // V image: token t at row t (64 B), rows >= L zero
  bf16* vw = vlds[wave];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = (lane >> 2) + 16 * i, ch = lane & 3;
    bf16x8 val;
    if (t < L) {
      const int64_t row = wa_pixel_row<GRID>(t, ws, n, wy, wx, nWy, nWx, Himg, Wimg);
      val = *(const bf16x8*)(V + row * ld + hoff + ch * 8);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) val[e] = (bf16)0.f;
    }
    *(bf16x8*)(vw + t * 32 + ch * 8) = val;
  }
  // K and Q fragments (row t = 16 b + (lane & 15), dims 8 g .. 8 g + 7), zero past L
  bf16x8 kf[4], qf[4];
  int64_t qrow[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int t = 16 * b + i16;
    if (t < L) {
      const int64_t row = wa_pixel_row<GRID>(t, ws, n, wy, wx, nWy, nWx, Himg, Wimg);
      qrow[b] = row;
      kf[b] = *(const bf16x8*)(K + row * ld + hoff + g * 8);
      qf[b] = *(const bf16x8*)(Q + row * ld + hoff + g * 8);
    } else {
      qrow[b] = -1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        kf[b][e] = (bf16)0.f;
        qf[b][e] = (bf16)0.f;
      }
    }
  }
  __syncthreads();
  // V^T fragments: dim block db (rows 16 db + (lane & 15)), k-chunk c
  const short* vs = (const short*)vw;
  bf16x8 va[2][2];
#pragma unroll
  for (int db = 0; db < 2; ++db) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = 16 * (2 * c + (j >> 2)) + 4 * g + (j & 3);
        va[db][c][j] = __builtin_bit_cast(bf16, vs[key * 32 + 16 * db + i16]);
      }
    }
  }
  if (!live) return;
  const float* bh = bias ? bias + (int64_t)h * L * L : nullptr;
  constexpr float LOG2E = 1.4426950408889634f;

#pragma unroll 1
  for (int qb = 0; qb < 4; ++qb) {
    const int qi = 16 * qb + i16;
    if (16 * qb >= L) break;  // wave-uniform
    f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb], qf[qb], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * kb + 4 * g + i;
        float v = s[kb][i] * scale_log2;
        if (key >= L) v = -INFINITY;
        else if (bh && qi < L) v = fmaf(bh[qi * L + key], LOG2E, v);
        s[kb][i] = v;
        m = fmaxf(m, v);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (m == -INFINITY) m = 0.f;  // a bias row of -inf only: p = exp2(-inf) = 0 for every key, and the row is zeros (below)
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = exp2f(s[kb][i] - m);
        s[kb][i] = p;
        sum += p;
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    bf16x8 pf[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[c][j] = (bf16)s[2 * c][j];
        pf[c][4 + j] = (bf16)s[2 * c + 1][j];
      }
    }
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // dead row -> zeros, as F.scaled_dot_product_attention on the CPU
    const int64_t orow = qrow[qb];
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[db][0], pf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[db][1], pf[1], o, 0, 0, 0);
      if (orow >= 0)
        *(bf16x4*)(O + orow * ldo + hoff + 16 * db + 4 * g) =
            bf16x4{(bf16)(o[0] * inv), (bf16)(o[1] * inv), (bf16)(o[2] * inv), (bf16)(o[3] * inv)};
    }
  }
}

// ------------------------------------------------------------------------------------------------ depthwise 3 x 3 + BN + GELU-tanh
// Work item = (image, output row, channel quad): the thread walks the output row left to right with a rolling 3 x 3 window of
// input quads (stride 1: one new column per pixel; stride 2: two), so every input quad is loaded once per output row that
// needs it; neighbouring lanes take neighbouring quads (coalesced pixel rows).  Because a thread owns a whole output row of its
// channels, the per-row channel sums of the squeeze-excitation's pool come out of registers with no cross-thread reduction,
// deterministically: psum[(n * Ho + oh) * C + c].  Stride 2 is the reference's F.pad(x, (0, 1, 0, 1)) + padding 0, i.e.
// inputs (2 oh + kh, 2 ow + kw), zero past the bottom / right edge; stride 1 is padding 1.
template <typename TX, typename TY, int STRIDE>
__global__ __launch_bounds__(256) void dwconv3_kernel(const TX* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* __restrict__ gate, float* __restrict__ psum,
                                                      TY* __restrict__ y, int64_t nitems, int H, int W, int Ho, int Wo, int C) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  const int C4 = C >> 2;
  const int q = (int)(it % C4);
  const int64_t row = it / C4;  // n * Ho + oh
  const int oh = (int)(row % Ho);
  const int64_t n = row / Ho;
  const int c0 = q * 4;
  f32x4 wk[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wk[k] = *(const f32x4*)(w + k * C + c0);
  const f32x4 sc = *(const f32x4*)(scale + c0), sh = *(const f32x4*)(shift + c0);
  f32x4 gt = {1.f, 1.f, 1.f, 1.f};
  if (gate) gt = *(const f32x4*)(gate + n * C + c0);
  const TX* xr[3];
  bool rv[3];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = STRIDE == 1 ? oh + kh - 1 : 2 * oh + kh;
    rv[kh] = ih >= 0 && ih < H;
    xr[kh] = x + ((n * H + (rv[kh] ? ih : 0)) * (int64_t)W) * C + c0;
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto ld = [&](int kh, int iw) -> f32x4 { return (rv[kh] && iw >= 0 && iw < W) ? mv_ld4(xr[kh] + (int64_t)iw * C) : zero; };
  f32x4 col[3][3];  // [kh][kw]
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) col[kh][kw] = ld(kh, STRIDE == 1 ? kw - 1 : kw);
  }
  TY* yr = y ? y + (row * (int64_t)Wo) * C + c0 : nullptr;
  f32x4 tot = zero;
  for (int ow = 0;;) {
    f32x4 acc = zero;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(col[kh][kw][e], wk[kh * 3 + kw][e], acc[e]);
      }
    }
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = gelu_tanh(fmaf(acc[e], sc[e], sh[e]));
      tot[e] += v[e];
    }
    if (yr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= gt[e];
      mv_st4(yr + (int64_t)ow * C, v);
    }
    if (++ow >= Wo) break;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      if (STRIDE == 1) {
        col[kh][0] = col[kh][1];
        col[kh][1] = col[kh][2];
        col[kh][2] = ld(kh, ow + 1);
      } else {
        col[kh][0] = col[kh][2];
        col[kh][1] = ld(kh, 2 * ow + 1);
        col[kh][2] = ld(kh, 2 * ow + 2);
      }
    }
  }
  if (psum) *(f32x4*)(psum + row * C + c0) = tot;
}

// ------------------------------------------------------------------------------------------------ squeeze-excitation gate
// One workgroup per image: the per-row partial sums are added in row order (deterministic), FC1 is one wave per hidden unit
// (coalesced weight rows, a 64-lane reduction), FC2 one thread per channel.
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ psum, int ntiles, float inv_hw,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ gate, int C, int R) {
  extern __shared__ float se_lds[];  // C means, then R hidden values
  float* hid = se_lds + C;
  const int64_t n = blockIdx.x;
  const float* ps = psum + n * (int64_t)ntiles * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int t = 0; t < ntiles; ++t) s += ps[(int64_t)t * C + c];
    se_lds[c] = s * inv_hw;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int r = wv; r < R; r += 4) {
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d = fmaf(w1[(int64_t)r * C + c], se_lds[c], d);
    d = wave_sum(d) + b1[r];
    if (lane == 0) hid[r] = d / (1.0f + expf(-d));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float z = b2[c];
    for (int r = 0; r < R; ++r) z = fmaf(w2[(int64_t)c * R + r], hid[r], z);
    gate[n * C + c] = 1.0f / (1.0f + expf(-z));
  }
}

// ------------------------------------------------------------------------------------------------ stem: 3 x 3 / stride 2 + BN + GELU
// As pm_convnext_stem: one wave per SP consecutive output pixels of an image row, lane l owns channels l, l + 64, ...; the SP
// patches (27 floats each, zero past the bottom / right edge) are staged in LDS and read back as broadcasts.
constexpr int MSTEM_SP = 8;

template <typename TY, int NCH>
__global__ __launch_bounds__(256) void mstem_kernel(const float* __restrict__ img, const float* __restrict__ wt,
                                                    const float* __restrict__ shift, TY* __restrict__ y, int64_t ldy,
                                                    int64_t ngroups, int Hi, int Wi, int Ho, int Wo, int d) {
  __shared__ float patch[4][MSTEM_SP * 27];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t g0 = (int64_t)blockIdx.x * 4 + wv;
  const bool live = g0 < ngroups;
  const int64_t g = live ? g0 : ngroups - 1;
  const int gpr = (Wo + MSTEM_SP - 1) / MSTEM_SP;
  const int jo0 = (int)(g % gpr) * MSTEM_SP;
  const int64_t t = g / gpr;
  const int io = (int)(t % Ho);
  const int64_t n = t / Ho;
  float* pw = patch[wv];
  for (int e = lane; e < MSTEM_SP * 27; e += 64) {
    const int p = e / 27, k = e - p * 27;
    const int ci = k / 9, kh = (k / 3) % 3, kw = k % 3;
    const int jo = jo0 + p < Wo ? jo0 + p : Wo - 1;
    const int ih = 2 * io + kh, iw = 2 * jo + kw;
    pw[e] = (ih < Hi && iw < Wi) ? img[((n * 3 + ci) * Hi + ih) * (int64_t)Wi + iw] : 0.f;
  }
  __syncthreads();
  if (!live) return;
  float acc[MSTEM_SP][NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    const float b = c < d ? shift[c] : 0.f;
#pragma unroll
    for (int p = 0; p < MSTEM_SP; ++p) acc[p][i] = b;
  }
#pragma unroll 3
  for (int k = 0; k < 27; ++k) {
    float wk[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      wk[i] = c < d ? wt[k * d + c] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < MSTEM_SP; ++p) {
      const float v = pw[p * 27 + k];
#pragma unroll
      for (int i = 0; i < NCH; ++i) acc[p][i] = fmaf(v, wk[i], acc[p][i]);
    }
  }
#pragma unroll
  for (int p = 0; p < MSTEM_SP; ++p) {
    if (jo0 + p >= Wo) break;
    TY* yr = y + ((n * Ho + io) * Wo + jo0 + p) * ldy;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < d) mv_st1(yr + c, gelu_tanh(acc[p][i]));
    }
    for (int64_t c = d + lane; c < ldy; c += 64) mv_st1(yr + c, 0.f);
  }
}

// ------------------------------------------------------------------------------------------------ im2col 3 x 3, pad 1
// Work item = (pixel, quad of output columns); columns (kh * 3 + kw) * C + c, then zeros up to ldy.
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void im2col3_kernel(const TX* __restrict__ x, TY* __restrict__ y, int64_t ldy, int64_t nitems,
                                                      int H, int W, int C) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  const int Q = (int)(ldy >> 2);
  const int qc = (int)(it % Q);
  const int64_t pix = it / Q;
  const int col = qc * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (col < 9 * C) {
    const int k = col / C, c = col - k * C;
    const int wq = (int)(pix % W);
    const int64_t t = pix / W;
    const int hq = (int)(t % H);
    const int64_t n = t / H;
    const int ih = hq + k / 3 - 1, iw = wq + k % 3 - 1;
    if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = mv_ld4(x + ((n * H + ih) * (int64_t)W + iw) * C + c);
  }
  mv_st4(y + pix * ldy + col, v);
}

// ------------------------------------------------------------------------------------------------ 2 x 2 average pool
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void avgpool2_kernel(const TX* __restrict__ x, TY* __restrict__ y, int64_t nitems, int H, int W,
                                                       int C) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  const int C4 = C >> 2;
  const int q = (int)(it % C4);
  const int64_t op = it / C4;
  const int Wo = W >> 1, Ho = H >> 1;
  const int jo = (int)(op % Wo);
  const int64_t t = op / Wo;
  const int io = (int)(t % Ho);
  const int64_t n = t / Ho;
  const TX* p = x + ((n * H + 2 * io) * (int64_t)W + 2 * jo) * C + q * 4;
  const f32x4 a = mv_ld4(p), b = mv_ld4(p + C), c = mv_ld4(p + (int64_t)W * C), d = mv_ld4(p + (int64_t)W * C + C);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = ((a[e] + b[e]) + (c[e] + d[e])) * 0.25f;
  mv_st4(y + op * C + q * 4, o);
}

bool dt_ok(int dt) { return dt == PM_BF16 || dt == PM_F32; }

}  // namespace

extern "C" int pm_window_attention_bf16(const void* q, const void* k, const void* v, int64_t ld, void* o, int64_t ldo,
                                        const float* bias, int64_t N, int64_t Himg, int64_t Wimg, int64_t n_heads, int64_t ws,
                                        int mode, void* stream) {
  if (!q || !k || !v || !o || N < 0 || Himg <= 0 || Wimg <= 0 || n_heads <= 0 || ws <= 0) return PM_EINVAL;
  if (mode != 0 && mode != 1) return PM_EINVAL;
  if (ws * ws > 64 || Himg % ws || Wimg % ws || Himg > (1 << 20) || Wimg > (1 << 20) || n_heads > 1024) return PM_EUNSUPPORTED;
  if (ld < 32 * n_heads || ldo < 32 * n_heads) return PM_EINVAL;
  if (ld % 8 || ldo % 4) return PM_EALIGN;
  if (!mv_aligned(q, 16) || !mv_aligned(k, 16) || !mv_aligned(v, 16) || !mv_aligned(o, 8) || (bias && !mv_aligned(bias, 4)))
    return PM_EALIGN;
  const int64_t nwork = N * (Himg / ws) * (Wimg / ws) * n_heads;
  if (nwork == 0) return PM_OK;
  const int64_t nblk = (nwork + WA_WAVES - 1) / WA_WAVES;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  const float scale_log2 = 1.4426950408889634f / sqrtf(32.0f);
  hipStream_t st = (hipStream_t)stream;
#define PM_WAGO(G)                                                                                                      \
  hipLaunchKernelGGL((window_attn_kernel<G>), dim3((unsigned)nblk), dim3(64 * WA_WAVES), 0, st, (const bf16*)q,         \
                     (const bf16*)k, (const bf16*)v, ld, (bf16*)o, ldo, bias, nwork, (int)n_heads, (int)Himg, (int)Wimg, \
                     (int)ws, scale_log2)
  if (mode == 1) PM_WAGO(true); else PM_WAGO(false);
#undef PM_WAGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_dwconv3_bn_act(const void* x, int x_dtype, const float* w, const float* scale, const float* shift,
                                 const float* gate, float* psum, void* y, int y_dtype, int64_t N, int64_t H, int64_t W,
                                 int64_t C, int stride, void* stream) {
  if (!x || !w || !scale || !shift || (!y && !psum) || N < 0 || H <= 0 || W <= 0 || C <= 0) return PM_EINVAL;
  if (!dt_ok(x_dtype) || (y && !dt_ok(y_dtype)) || (stride != 1 && stride != 2)) return PM_EINVAL;
  if (C % 4 || C > (1 << 16) || H > (1 << 20) || W > (1 << 20)) return PM_EUNSUPPORTED;
  if (stride == 2 && (H < 2 || W < 2)) return PM_EUNSUPPORTED;
  const int xs = x_dtype == PM_F32 ? 16 : 8, ys = y_dtype == PM_F32 ? 16 : 8;
  if (!mv_aligned(x, xs) || (y && !mv_aligned(y, ys)) || !mv_aligned(w, 16) || !mv_aligned(scale, 16) ||
      !mv_aligned(shift, 16) || (gate && !mv_aligned(gate, 16)) || (psum && !mv_aligned(psum, 16)))
    return PM_EALIGN;
  const int64_t Ho = stride == 1 ? H : (H - 2) / 2 + 1, Wo = stride == 1 ? W : (W - 2) / 2 + 1;
  const int64_t nitems = N * Ho * (C / 4);
  if (nitems == 0) return PM_OK;
  const int64_t nblk = (nitems + 255) / 256;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_DW3GO(TX, TY, S)                                                                                                    \
  hipLaunchKernelGGL((dwconv3_kernel<TX, TY, S>), dim3((unsigned)nblk), dim3(256), 0, st, (const TX*)x, w, scale, shift, gate, \
                     psum, (TY*)y, nitems, (int)H, (int)W, (int)Ho, (int)Wo, (int)C)
#define PM_DW3S(TX, TY)      \
  if (stride == 1)           \
    PM_DW3GO(TX, TY, 1);     \
  else                       \
    PM_DW3GO(TX, TY, 2)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_DW3S(float, float); else PM_DW3S(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_DW3S(bf16, float); else PM_DW3S(bf16, bf16);
  }
#undef PM_DW3S
#undef PM_DW3GO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_se_gate(const float* psum, int64_t ntiles, int64_t hw, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* gate, int64_t N, int64_t C, int64_t R, void* stream) {
  if (!psum || !w1 || !b1 || !w2 || !b2 || !gate || N < 0 || ntiles <= 0 || hw <= 0 || C <= 0 || R <= 0) return PM_EINVAL;
  if (C > 16384 || R > 4096 || ntiles > (1 << 20) || N > 0x7fffffff) return PM_EUNSUPPORTED;
  const size_t lds = (size_t)(C + R) * sizeof(float);
  if (lds > 64 * 1024) return PM_EUNSUPPORTED;  // the default dynamic-LDS limit, which this kernel never raises
  if (N == 0) return PM_OK;
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)N), dim3(256), lds, (hipStream_t)stream, psum, (int)ntiles,
                     1.0f / (float)hw, w1, b1, w2, b2, gate, (int)C, (int)R);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_maxvit_stem(const float* imgs, const float* wt, const float* shift, void* y, int64_t ldy, int y_dtype,
                              int64_t N, int64_t Himg, int64_t Wimg, int64_t d, void* stream) {
  if (!imgs || !wt || !shift || !y || N < 0 || d <= 0 || ldy < d || !dt_ok(y_dtype)) return PM_EINVAL;
  if (Himg < 2 || Wimg < 2 || Himg > (1 << 20) || Wimg > (1 << 20) || d > 256) return PM_EUNSUPPORTED;
  const int64_t Ho = (Himg - 2) / 2 + 1, Wo = (Wimg - 2) / 2 + 1;
  const int64_t ngroups = N * Ho * ((Wo + MSTEM_SP - 1) / MSTEM_SP);
  if (ngroups == 0) return PM_OK;
  const int64_t nblk = (ngroups + 3) / 4;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nch = (int)((d + 63) / 64);
#define PM_MSGO(TY, K)                                                                                                      \
  hipLaunchKernelGGL((mstem_kernel<TY, K>), dim3((unsigned)nblk), dim3(256), 0, st, imgs, wt, shift, (TY*)y, ldy, ngroups, \
                     (int)Himg, (int)Wimg, (int)Ho, (int)Wo, (int)d)
#define PM_MSNCH(TY)                  \
  switch (nch) {                      \
    case 1: PM_MSGO(TY, 1); break;    \
    case 2: PM_MSGO(TY, 2); break;    \
    case 3: PM_MSGO(TY, 3); break;    \
    default: PM_MSGO(TY, 4); break;   \
  }
  if (y_dtype == PM_F32) {
    PM_MSNCH(float)
  } else {
    PM_MSNCH(bf16)
  }
#undef PM_MSNCH
#undef PM_MSGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_im2col3x3_nhwc(const void* x, int x_dtype, void* y, int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W,
                                 int64_t C, void* stream) {
  if (!x || !y || N < 0 || H <= 0 || W <= 0 || C <= 0 || ldy < 9 * C || !dt_ok(x_dtype) || !dt_ok(y_dtype)) return PM_EINVAL;
  if (C % 4 || ldy % 4 || C > (1 << 16) || H > (1 << 20) || W > (1 << 20)) return PM_EUNSUPPORTED;
  if (!mv_aligned(x, x_dtype == PM_F32 ? 16 : 8) || !mv_aligned(y, y_dtype == PM_F32 ? 16 : 8)) return PM_EALIGN;
  const int64_t nitems = N * H * W * (ldy / 4);
  if (nitems == 0) return PM_OK;
  const int64_t nblk = (nitems + 255) / 256;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_I2CGO(TX, TY)                                                                                                       \
  hipLaunchKernelGGL((im2col3_kernel<TX, TY>), dim3((unsigned)nblk), dim3(256), 0, st, (const TX*)x, (TY*)y, ldy, nitems, \
                     (int)H, (int)W, (int)C)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_I2CGO(float, float); else PM_I2CGO(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_I2CGO(bf16, float); else PM_I2CGO(bf16, bf16);
  }
#undef PM_I2CGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_avgpool2x2_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                                  void* stream) {
  if (!x || !y || N < 0 || H <= 0 || W <= 0 || C <= 0 || !dt_ok(x_dtype) || !dt_ok(y_dtype)) return PM_EINVAL;
  if (H % 2 || W % 2 || C % 4 || C > (1 << 20) || H > (1 << 20) || W > (1 << 20)) return PM_EUNSUPPORTED;
  if (!mv_aligned(x, x_dtype == PM_F32 ? 16 : 8) || !mv_aligned(y, y_dtype == PM_F32 ? 16 : 8)) return PM_EALIGN;
  const int64_t nitems = N * (H / 2) * (W / 2) * (C / 4);
  if (nitems == 0) return PM_OK;
  const int64_t nblk = (nitems + 255) / 256;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_APGO(TX, TY)                                                                                                         \
  hipLaunchKernelGGL((avgpool2_kernel<TX, TY>), dim3((unsigned)nblk), dim3(256), 0, st, (const TX*)x, (TY*)y, nitems, (int)H, \
                     (int)W, (int)C)
  if (x_dtype == PM_F32) {
    if (y_dtype == PM_F32) PM_APGO(float, float); else PM_APGO(float, bf16);
  } else {
    if (y_dtype == PM_F32) PM_APGO(bf16, float); else PM_APGO(bf16, bf16);
  }
#undef PM_APGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}
