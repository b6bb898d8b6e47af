// encodec.hip - the kernels of EnCodec (reference: pytorch_models/audio/encodec.py), everything fp32 on the exact-product
// f32 MFMA (v_mfma_f32_16x16x4_f32, as linear_f32.hip): the encoder ends in an argmin, so bf16 operands give another codec.
// Activations are TIME-MAJOR (B, T, C): the im2col row of output frame t is then the k * Cin contiguous floats that start
// at frame t * stride - left, so the convolutions are implicit GEMMs without an im2col buffer.
//
//  pm_conv1d_f32        Conv1d with the reflect padding taken as mirrored indices, an optional ELU on the operand as it is
//                       loaded, bias and an optional residual in the epilogue; the same kernel in its zero-padding / "up"
//                       mode is ConvTranspose1d(kernel 2 s, stride s): row j = [x[j-1], x[j]] against a repacked
//                       (s * Cout, 2 * Cin) matrix, whose (T + 1, s * Cout) output IS the time-major result, trimmed on
//                       the way out (Unpad1d).
//  pm_lstm_f32          the stacked LSTM: one pm_linear_f32 for layer 0's input projections of all frames, then ONE LAUNCH
//                       PER STEP of a kernel in which a workgroup owns the four gates of four hidden units (its 16 rows of
//                       W_hh are one MFMA A tile; the cell update is the epilogue); two layers run as a wavefront, layer 1 at
//                       frame t - 1 beside layer 0 at frame t (T + 1 launches).  No grid barrier, no flag.
//  pm_rvq_encode_f32    all stages of the residual vector quantizer in one pass over the latent rows.
//  pm_rvq_decode_f32    sum of the chosen codebook rows, time-major.
//  pm_groupnorm1_f32    GroupNorm(1, C) over a whole clip (per-thread fp32 mean and centred squares, combined in fp64), in place.
//  pm_encodec_scale_f32 / pm_scale_clips_f32   the 48 kHz variant's per-clip input scale and its division / multiplication.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ convolution
constexpr int CBM = 128, CBK = 16, CPITCH = 20;  // rows of a tile, K step, floats per LDS row (linear_f32.hip's pitch)

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }

// Tile 128 frames x (16 NT) output columns x 16; four waves, wave w owns frames 32 w .. 32 w + 31 and every column
// (2 x NT MFMA tiles).  A workgroup never crosses a clip, so the mirrored index needs one reflection.
template <int NT>
__global__ __launch_bounds__(256) void conv1d_f32_kernel(const float* __restrict__ X, int64_t x_bs, const float* __restrict__ W,
                                                         const float* __restrict__ bias, const float* __restrict__ resid,
                                                         float* __restrict__ Y, int Tin, int Cin, int Cout, int N, int K,
                                                         int stride, int left, int zero_pad, int elu, int up, int trim, int Mr,
                                                         int Tout, int tiles_m, int tiles_n) {
  constexpr int BN = 16 * NT;
  constexpr int WCH = NT >= 4 ? NT / 4 : 1;  // 16-byte chunks of the weight tile per thread
  constexpr int STAGE = (CBM + BN) * CPITCH;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tn = blockIdx.x % tiles_n, rest = blockIdx.x / tiles_n;
  const int tm = rest % tiles_m, b = rest / tiles_m;
  const int m0 = tm * CBM, n0 = tn * BN;
  const float* xb = X + (int64_t)b * x_bs;
  const bool vec = (Cin & 3) == 0;  // then K % 4 == 0 and a 4-float chunk never straddles a tap
  const int nk = (K + CBK - 1) / CBK;

  const int srow = tid >> 2, sk = (tid & 3) * 4;
  int f0[2];  // first source frame of the thread's two rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int t = m0 + srow + i * 64;
    t = t < Mr ? t : Mr - 1;
    f0[i] = t * stride - left;
  }
  int wrow[WCH];
#pragma unroll
  for (int j = 0; j < WCH; ++j) {
    int gn = n0 + ((tid + j * 256) >> 2);
    wrow[j] = gn < N ? gn : N - 1;
  }
  int tap = sk / Cin, ci = sk - tap * Cin;  // position of this thread's chunk; advanced by 16 per K step

  auto frame = [&](int f, bool& ok) {
    ok = true;
    if (zero_pad) {
      ok = f >= 0 && f < Tin;
      return ok ? f : 0;
    }
    f = f < 0 ? -f : f;
    return f >= Tin ? 2 * (Tin - 1) - f : f;
  };

  f32x4 xr[2], wr[WCH];
  auto fetch = [&](int kt) {
    const int kk = kt * CBK + sk;
    if (vec) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (kk < K) {
          bool ok;
          const int f = frame(f0[i] + tap, ok);
          if (ok) v = *(const f32x4*)(xb + (int64_t)f * Cin + ci);
          if (elu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = elu1(v[e]);
          }
        }
        xr[i] = v;
      }
#pragma unroll
      for (int j = 0; j < WCH; ++j) {
        wr[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kk < K && tid + j * 256 < BN * 4) wr[j] = *(const f32x4*)(W + (int64_t)wrow[j] * K + kk);
      }
      ci += CBK;
      while (ci >= Cin) {
        ci -= Cin;
        ++tap;
      }
    } else {  // Cin not a multiple of 4 (the first convolution: one or two audio channels): element-wise
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = 0.f;
          if (kk + e < K) {
            const int tp = (kk + e) / Cin;
            bool ok;
            const int f = frame(f0[i] + tp, ok);
            if (ok) v = xb[(int64_t)f * Cin + (kk + e - tp * Cin)];
            if (elu) v = elu1(v);
          }
          xr[i][e] = v;
        }
      }
#pragma unroll
      for (int j = 0; j < WCH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          wr[j][e] = (kk + e < K && tid + j * 256 < BN * 4) ? W[(int64_t)wrow[j] * K + kk + e] : 0.f;
    }
  };
  auto put = [&](int buf) {
    float* xs = smem + buf * STAGE;
    float* ws = xs + CBM * CPITCH;
#pragma unroll
    for (int i = 0; i < 2; ++i) *(f32x4*)(xs + (srow + i * 64) * CPITCH + sk) = xr[i];
#pragma unroll
    for (int j = 0; j < WCH; ++j)
      if (tid + j * 256 < BN * 4) *(f32x4*)(ws + ((tid + j * 256) >> 2) * CPITCH + sk) = wr[j];
  };

  f32x4 acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  fetch(0);
  put(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) fetch(kt + 1);
    const float* xs = smem + (kt & 1) * STAGE;
    const float* ws = xs + CBM * CPITCH;
#pragma unroll
    for (int ss = 0; ss < CBK / 4; ++ss) {
      float a[NT], bb[2];
#pragma unroll
      for (int j = 0; j < NT; ++j) a[j] = ws[(j * 16 + fr) * CPITCH + ss * 4 + fq];
#pragma unroll
      for (int i = 0; i < 2; ++i) bb[i] = xs[(wave * 32 + i * 16 + fr) * CPITCH + ss * 4 + fq];
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bb[i], acc[j][i], 0, 0, 0);
    }
    if (kt + 1 < nk) put((kt + 1) & 1);
    __syncthreads();
  }

  // The epilogue may store an accumulator to memory as it is (no bias, no residual): the explicit wait of lstm_step_kernel, for
  // the same reason (the compiler guards VALU reads of an MFMA result, not stores), tied to every accumulator.
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(acc[j][i]));

  // D[row = column 4 fq + r][col = frame fr].  Column n of the product is output channel n % Cout of output frame
  // m * up + n / Cout - trim (up = 1, trim = 0: a plain convolution).
  const bool v4 = (Cout & 3) == 0;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + j * 16 + fq * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + wave * 32 + i * 16 + fr;
      if (m >= Mr || n >= N) continue;
      if (v4) {
        const int rr = n / Cout, c = n - rr * Cout;
        const int o = m * up + rr - trim;
        if (o < 0 || o >= Tout) continue;
        const int64_t at = ((int64_t)b * Tout + o) * Cout + c;
        f32x4 v = acc[j][i];
        if (bias) v += *(const f32x4*)(bias + c);
        if (resid) v += *(const f32x4*)(resid + at);
        *(f32x4*)(Y + at) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n + r >= N) continue;
          const int rr = (n + r) / Cout, c = n + r - rr * Cout;
          const int o = m * up + rr - trim;
          if (o < 0 || o >= Tout) continue;
          const int64_t at = ((int64_t)b * Tout + o) * Cout + c;
          float v = acc[j][i][r] + (bias ? bias[c] : 0.f);
          if (resid) v += resid[at];
          Y[at] = v;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ LSTM step
__device__ __forceinline__ float sigmoid1(float v) { return 1.0f / (1.0f + expf(-v)); }

// What one layer does in one launch: frame t of the sequence.  The gates' input part is either xp (B, T, 4H), the projections of
// all frames from one GEMM (bias included), or - xin != NULL - computed here from the layer's input row xin[b, t] and Win, + bias.
struct LstmRole {
  const float* xp;
  const float* xin;
  const float* Win;
  const float* bias;
  const float* Whh;
  float* hseq;
  float* cst;
  const float* xres;
  float* y;
  int t;  // outside [0, T): the role is idle in this launch
};

// acc += W[16 rows of this lane's tile][kbeg .. kbeg + kq) . h[16 batch rows][same k]: 8 K steps per group, all 16 loads of a
// group in flight before its MFMAs.  A lane loads 4 consecutive k of its row and feeds them to 4 MFMAs: the k order inside the
// MFMAs is permuted the same way for both operands.
__device__ __forceinline__ void lstm_mma(f32x4& acc, const float* wp, const float* hp, int kq) {
  for (int i0 = 0; i0 < kq; i0 += 128) {
    f32x4 a4[8], b4[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = i0 + 16 * j < kq;  // wave-uniform
      a4[j] = in ? *(const f32x4*)(wp + i0 + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
      b4[j] = in ? *(const f32x4*)(hp + i0 + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j][e], b4[j][e], acc, 0, 0, 0);
  }
}

// One launch = one time step.  Workgroups 0 .. H/4 - 1 serve role r0, the next H/4 role r1 (the wavefront: layer 1 at frame
// t - 1 beside layer 0 at frame t; the plain form launches H/4 workgroups with r0 only).  Workgroup g of a role owns hidden units
// 4 g .. 4 g + 3: the A tile's row a is gate (a & 3) of unit (a >> 2), so that lane (fq, fr) of the accumulator holds the four
// gates (i, f, g, o) of unit fq for batch row fr and the cell update needs no exchange; c stays with its owner.  The four waves
// split K; wave 0 adds the partial products in a fixed order, so a batch row does not depend on its neighbours.  h_t goes straight
// into hseq (B, T, H), where the next launch reads it.  No wait on another workgroup anywhere.
__global__ __launch_bounds__(256) void lstm_step_kernel(LstmRole r0, LstmRole r1, int B, int T, int H) {
  __shared__ f32x4 red[4][64];
  const int nb = H >> 2;
  const bool second = (int)blockIdx.x >= nb;
  const LstmRole r = second ? r1 : r0;
  const int t = r.t;
  if (t < 0 || t >= T) return;  // uniform for the workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int u0 = ((int)blockIdx.x - (second ? nb : 0)) * 4;
  const int64_t wrow = ((int64_t)(fr & 3) * H + u0 + (fr >> 2)) * H;
  const int kq = H >> 2, koff = wave * kq + fq * 4;
  for (int bt = 0; bt < B; bt += 16) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int bb = bt + fr < B ? bt + fr : B - 1;
    if (r.xin) lstm_mma(acc, r.Win + wrow + koff, r.xin + ((int64_t)bb * T + t) * H + koff, kq);
    if (t > 0) lstm_mma(acc, r.Whh + wrow + koff, r.hseq + ((int64_t)bb * T + (t - 1)) * H + koff, kq);
    // DO NOT REMOVE, and do not let a store read an MFMA accumulator directly.  With -amdgpu-mfma-vgpr-form the compiler puts
    // its own wait states in front of VALU reads of an accumulator, but it put NONE in front of the LDS store below: the
    // store took the accumulator without the last products (step 0, which has no recurrent term, was exact; every later step
    // was off by the last k of each wave's range: 0.04 at T = 2, 0.66 at T = 300).  The shape of the loop does not matter;
    // this wait does.  32 wait states cover the 8 passes of v_mfma_f32_16x16x4_f32 several times over.
    asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc));
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
      const f32x4 s = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
      const int bq = bt + fr, u = u0 + fq;
      if (bq < B) {
        const float* xr = r.xp ? r.xp + ((int64_t)bq * T + t) * 4 * H + u : r.bias + u;
        const float gi = sigmoid1(s[0] + xr[0]);
        const float gf = sigmoid1(s[1] + xr[H]);
        const float gg = tanhf(s[2] + xr[2 * H]);
        const float go = sigmoid1(s[3] + xr[3 * H]);
        const int64_t ci = (int64_t)bq * H + u;
        const float cn = t > 0 ? fmaf(gf, r.cst[ci], gi * gg) : gi * gg;
        const float h = go * tanhf(cn);
        r.cst[ci] = cn;
        const int64_t at = ((int64_t)bq * T + t) * H + u;
        r.hseq[at] = h;
        if (r.y) r.y[at] = r.xres ? r.xres[at] + h : h;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ RVQ
constexpr int RVQ_D = 128, RVQ_N = 1024, RVQ_PITCH = 132;

// 16 latent rows per workgroup, every stage without leaving the kernel.  Per stage wave w scans entries 256 w .. 256 w + 255
// in increasing order (16 MFMA tiles of 16 entries; the residual's fragments stay in registers), d = |e|^2 - 2 r.e, strict "<"
// keeps the lowest index on exact ties; lanes, then waves, are combined on (d, index).
__global__ __launch_bounds__(256) void rvq_encode_kernel(const float* __restrict__ Z, const float* __restrict__ E,
                                                         const float* __restrict__ E2, int64_t* __restrict__ codes, int M,
                                                         int nq) {
  __shared__ __attribute__((aligned(16))) float r[16 * RVQ_PITCH];
  __shared__ float bd[4][16];
  __shared__ int bi[4][16];
  __shared__ int best[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * 16;
  for (int e = tid; e < 16 * (RVQ_D / 4); e += 256) {
    const int row = e >> 5, ch = e & 31;
    const int m = m0 + row < M ? m0 + row : M - 1;
    *(f32x4*)(r + row * RVQ_PITCH + ch * 4) = *(const f32x4*)(Z + (int64_t)m * RVQ_D + ch * 4);
  }
  __syncthreads();
  for (int q = 0; q < nq; ++q) {
    const float* Eq = E + (int64_t)q * RVQ_N * RVQ_D;
    const float* E2q = E2 + (int64_t)q * RVQ_N;
    f32x4 rf[RVQ_D / 16];
#pragma unroll
    for (int c = 0; c < RVQ_D / 16; ++c) rf[c] = *(const f32x4*)(r + fr * RVQ_PITCH + c * 16 + fq * 4);
    float bestd = __builtin_inff();
    int besti = wave * 256 + 4 * fq;
    for (int tile = 0; tile < 16; ++tile) {
      const int code0 = wave * 256 + tile * 16;
      const float* erow = Eq + (int64_t)(code0 + fr) * RVQ_D + fq * 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < RVQ_D / 16; ++c) {
        const f32x4 a4 = *(const f32x4*)(erow + c * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], rf[c][e], acc, 0, 0, 0);
      }
      const f32x4 n2 = *(const f32x4*)(E2q + code0 + 4 * fq);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float d = fmaf(-2.0f, acc[rr], n2[rr]);
        if (d < bestd) {
          bestd = d;
          besti = code0 + 4 * fq + rr;
        }
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float od = __shfl_xor(bestd, o, 64);
      const int oi = __shfl_xor(besti, o, 64);
      if (od < bestd || (od == bestd && oi < besti)) {
        bestd = od;
        besti = oi;
      }
    }
    if (fq == 0) {
      bd[wave][fr] = bestd;
      bi[wave][fr] = besti;
    }
    __syncthreads();
    if (tid < 16) {
      float d0 = bd[0][tid];
      int i0 = bi[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (bd[w][tid] < d0) {  // later waves hold higher indices: strict "<" keeps the lowest on ties
          d0 = bd[w][tid];
          i0 = bi[w][tid];
        }
      best[tid] = i0;
      if (m0 + tid < M) codes[(int64_t)q * M + m0 + tid] = i0;
    }
    __syncthreads();
    for (int e = tid; e < 16 * (RVQ_D / 4); e += 256) {
      const int row = e >> 5, ch = e & 31;
      f32x4* p = (f32x4*)(r + row * RVQ_PITCH + ch * 4);
      *p = *p - *(const f32x4*)(Eq + (int64_t)best[row] * RVQ_D + ch * 4);
    }
    __syncthreads();
  }
}

// out (B * T, 128) = sum over the stages, in stage order, of the chosen rows; an index outside the codebook is clamped into it.
__global__ __launch_bounds__(256) void rvq_decode_kernel(const int64_t* __restrict__ codes, int64_t sb, int64_t sq, int64_t st,
                                                         const float* __restrict__ E, float* __restrict__ out, int64_t M, int T,
                                                         int nq) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = g >> 5;
  const int ch = (int)(g & 31);
  if (m >= M) return;
  const int64_t b = m / T, t = m - b * T;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < nq; ++q) {
    int64_t idx = codes[b * sb + q * sq + t * st];
    idx = idx < 0 ? 0 : (idx >= RVQ_N ? RVQ_N - 1 : idx);
    const f32x4 v = *(const f32x4*)(E + ((int64_t)q * RVQ_N + idx) * RVQ_D + ch * 4);
    s = q == 0 ? v : s + v;
  }
  *(f32x4*)(out + m * RVQ_D + ch * 4) = s;
}

// ------------------------------------------------------------------------------------------------ GroupNorm(1, C), scale
constexpr int GN_CHUNK = 16384;  // floats per workgroup: 64 per thread in fp32 around the thread's own mean, everything above in fp64
constexpr int GN_PER = GN_CHUNK / 256;

__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const double s = sh[0];
  __syncthreads();
  return s;
}

// Statistics of one chunk as (mean, M2 = sum (x - mean)^2), the two doubles of the chunk.  This kernel used to store the fp32 sums
// S = sum x and SS = sum x^2 of 64 values per thread and gn_apply_kernel formed SS / n - mean^2: at |mean| / sigma = 4096 the fp32
// SS carries an error of about 64 u mean^2 per value, a thousand times the variance, and the output was no normalisation at all
// (tests/encodec_cases.py, the offset family, found it).  Now a thread keeps its 64 values in registers, takes their fp32 mean p as a
// pivot and sums d = sum (x - p) and q = sum (x - p)^2 in fp32 (small numbers whatever the clip's mean); its exact-arithmetic
// statistics are mean_t = p + d / n_t and M2_t = q - d^2 / n_t, formed in fp64, and threads, then chunks, are combined in fp64 with
// Chan's formula M2 = sum (M2_i + n_i (mean_i - mean)^2).
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int64_t n,
                                                       int nchunk) {
  __shared__ double sh[256];
  const int64_t b = blockIdx.y, beg = (int64_t)blockIdx.x * GN_CHUNK;
  const int64_t end = beg + GN_CHUNK < n ? beg + GN_CHUNK : n;
  const float* xb = x + b * n;
  float v[GN_PER];
  float s = 0.f;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < GN_PER; ++j) {
    const int64_t i = beg + threadIdx.x + j * 256;
    const bool in = i < end;
    v[j] = in ? xb[i] : 0.f;
    s += v[j];
    cnt += in;
  }
  const float p = cnt ? s / (float)cnt : 0.f;
  float d = 0.f, q = 0.f;
#pragma unroll
  for (int j = 0; j < GN_PER; ++j) {
    const float c = beg + threadIdx.x + j * 256 < end ? v[j] - p : 0.f;
    d += c;
    q = fmaf(c, c, q);
  }
  const double nt = (double)cnt;
  const double mean_t = cnt ? (double)p + (double)d / nt : 0.0;
  const double m2_t = cnt ? (double)q - (double)d * (double)d / nt : 0.0;
  const double mean = block_sum_f64(nt * mean_t, sh) / (double)(end - beg);
  const double dm = mean_t - mean;
  const double M2 = block_sum_f64(m2_t + nt * dm * dm, sh);
  if (threadIdx.x == 0) {
    part[(b * nchunk + blockIdx.x) * 2] = mean;
    part[(b * nchunk + blockIdx.x) * 2 + 1] = M2 > 0.0 ? M2 : 0.0;
  }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(float* __restrict__ x, const double* __restrict__ part,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ resid, int64_t n, int C, int nchunk, float eps) {
  __shared__ double sh[256];
  const int64_t b = blockIdx.y;
  auto count = [&](int i) { return (double)(i + 1 < nchunk ? (int64_t)GN_CHUNK : n - (int64_t)i * GN_CHUNK); };
  double s = 0.0;
  for (int i = threadIdx.x; i < nchunk; i += 256) s += count(i) * part[(b * nchunk + i) * 2];
  const double mean = block_sum_f64(s, sh) / (double)n;
  double m2 = 0.0;
  for (int i = threadIdx.x; i < nchunk; i += 256) {
    const double dm = part[(b * nchunk + i) * 2] - mean;
    m2 += part[(b * nchunk + i) * 2 + 1] + count(i) * dm * dm;
  }
  const double var = block_sum_f64(m2, sh) / (double)n;
  const float mu = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)eps));
  const int64_t beg = (int64_t)blockIdx.x * GN_CHUNK;
  const int64_t end = beg + GN_CHUNK < n ? beg + GN_CHUNK : n;
  float* xb = x + b * n;
  int c = (int)((beg + threadIdx.x) % C);  // one 64-bit remainder per thread; then the channel advances by 256 % C
  const int cstep = 256 % C;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256, c = c + cstep >= C ? c + cstep - C : c + cstep) {
    float v = fmaf((xb[i] - mu) * rstd, gamma[c], beta[c]);
    if (resid) v += resid[b * n + i];
    xb[i] = v;
  }
}

// scale[b] = sqrt(mean_t(mean_c(x[b, c, t])^2)) + 1e-8, x (B, C, T)
__global__ __launch_bounds__(1024) void encodec_scale_kernel(const float* __restrict__ x, float* __restrict__ scale, int C,
                                                             int64_t T) {
  __shared__ double sh[1024];
  const float* xb = x + (int64_t)blockIdx.x * C * T;
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += 1024) {
    float m = 0.f;
    for (int c = 0; c < C; ++c) m += xb[c * T + t];
    m = m / (float)C;
    s += (double)m * (double)m;
  }
  const double S = block_sum_f64(s, sh);
  if (threadIdx.x == 0) scale[blockIdx.x] = sqrtf((float)(S / (double)T)) + 1e-8f;
}

__global__ __launch_bounds__(256) void scale_clips_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          float* __restrict__ y, int64_t n, int divide) {
  const int64_t b = blockIdx.y;
  const float s = scale[b];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[b * n + i] = divide ? x[b * n + i] / s : x[b * n + i] * s;
}

int conv_nt(int64_t N) { return N <= 16 ? 1 : N <= 32 ? 2 : N <= 64 ? 4 : 8; }

}  // namespace

extern "C" int pm_conv1d_f32_supported(int64_t Tin, int64_t Cin, int64_t Cout, int64_t k, int64_t stride, int64_t left,
                                       int64_t right, int zero_pad, int64_t up) {
  if (Tin < 1 || Cin < 1 || Cout < 1 || k < 1 || stride < 1 || left < 0 || right < 0 || up < 1) return 0;
  if (Tin + left + right < k) return 0;
  if (!zero_pad && (left >= Tin || right >= Tin)) return 0;  // one reflection only, as F.pad(mode="reflect") itself demands
  if (Tin * Cin >= (1ll << 31) || k * Cin >= (1ll << 31) || up * Cout >= (1ll << 31)) return 0;
  if (((Tin + left + right - k) / stride + 1) * up * stride >= (1ll << 31)) return 0;
  return 1;
}

extern "C" int pm_conv1d_f32(const float* x, int64_t x_batch_stride, const float* w, const float* bias, const float* resid,
                             float* y, int64_t B, int64_t Tin, int64_t Cin, int64_t Cout, int64_t k, int64_t stride,
                             int64_t left, int64_t right, int zero_pad, int elu, int64_t up, int64_t trim, int64_t Tout,
                             void* stream) {
  if (!x || !w || !y || B < 0 || Tout < 1 || trim < 0) return PM_EINVAL;
  if (!pm_conv1d_f32_supported(Tin, Cin, Cout, k, stride, left, right, zero_pad, up)) return PM_EUNSUPPORTED;
  if (B == 0) return PM_OK;
  if (x_batch_stride < Tin * Cin) return PM_EINVAL;
  const int64_t Mr = (Tin + left + right - k) / stride + 1, N = up * Cout, K = k * Cin;
  if (trim + Tout > Mr * up || (resid && (up != 1 || trim != 0))) return PM_EINVAL;  // every frame of y is written
  if ((Cin & 3) == 0 && ((x_batch_stride & 3) || (((uintptr_t)x | (uintptr_t)w) & 15))) return PM_EALIGN;
  if ((Cout & 3) == 0 && ((((uintptr_t)y | (uintptr_t)bias | (uintptr_t)resid) & 15))) return PM_EALIGN;
  const int nt = conv_nt(N);
  const int64_t tiles_m = (Mr + CBM - 1) / CBM, tiles_n = (N + 16 * nt - 1) / (16 * nt);
  const int64_t nblk = B * tiles_m * tiles_n;
  if (nblk > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define PM_CONVGO(NT)                                                                                                      \
  hipLaunchKernelGGL((conv1d_f32_kernel<NT>), dim3((unsigned)nblk), dim3(256), 0, st, x, x_batch_stride, w, bias, resid, y, \
                     (int)Tin, (int)Cin, (int)Cout, (int)N, (int)K, (int)stride, (int)left, zero_pad, elu, (int)up, (int)trim, \
                     (int)Mr, (int)Tout, (int)tiles_m, (int)tiles_n)
  switch (nt) {
    case 1: PM_CONVGO(1); break;
    case 2: PM_CONVGO(2); break;
    case 4: PM_CONVGO(4); break;
    default: PM_CONVGO(8); break;
  }
#undef PM_CONVGO
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int64_t pm_lstm_workspace_floats(int64_t B, int64_t T, int64_t H) { return B * T * 6 * H + 2 * B * H; }

extern "C" int pm_lstm_f32(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* bias,
                           int64_t n_layers, float* work, float* y, int flags, int64_t B, int64_t T, int64_t H,
                           void* stream) {
  if (!x || !w_ih || !w_hh || !bias || !work || !y || n_layers < 1 || B < 0 || T < 1 || (flags & ~3)) return PM_EINVAL;
  if (H < 64 || H % 64 || H > 16384) return PM_EUNSUPPORTED;  // four waves x K steps of 16
  if (B == 0) return PM_OK;
  if (B >= (1ll << 31) || T >= (1ll << 31) || B * T * 4 * H >= (1ll << 40)) return PM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)work | (uintptr_t)y) & 15) return PM_EALIGN;
  for (int64_t l = 0; l < n_layers; ++l)
    if (!w_ih[l] || !w_hh[l] || !bias[l] || (((uintptr_t)w_ih[l] | (uintptr_t)w_hh[l]) & 15)) return PM_EINVAL;
  const bool residual = flags & 1;
  float* xp = work;
  float* hbuf[2] = {work + B * T * 4 * H, work + B * T * 5 * H};
  float* cbuf[2] = {work + B * T * 6 * H, work + B * T * 6 * H + B * H};
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)(H / 4);
  const LstmRole idle = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, -1};
  if (n_layers == 2 && !(flags & 2)) {
    // the wavefront: launch s runs layer 0 at frame s beside layer 1 at frame s - 1, which multiplies [h0, h1_prev] with
    // [W_ih; W_hh] itself (K = 2 H): T + 1 launches and one GEMM instead of 2 T launches and two GEMMs
    const int rc = pm_linear_f32(x, H, 0, 0, w_ih[0], H, bias[0], nullptr, 0, 0, xp, 4 * H, B * T, 4 * H, H, PM_ACT_NONE, stream);
    if (rc != PM_OK) return rc;
    LstmRole r0 = {xp, nullptr, nullptr, nullptr, w_hh[0], hbuf[0], cbuf[0], nullptr, nullptr, 0};
    LstmRole r1 = {nullptr, hbuf[0], w_ih[1], bias[1], w_hh[1], hbuf[1], cbuf[1], residual ? x : nullptr, y, -1};
    for (int64_t s = 0; s <= T; ++s) {
      r0.t = (int)s;  // == T in the last launch: idle
      r1.t = (int)s - 1;
      hipLaunchKernelGGL(lstm_step_kernel, dim3(2 * nb), dim3(256), 0, st, r0, r1, (int)B, (int)T, (int)H);
    }
    PM_CHECK_LAUNCH();
    return PM_OK;
  }
  const float* in = x;
  for (int64_t l = 0; l < n_layers; ++l) {  // plain passes: per layer one GEMM and T launches
    const int rc = pm_linear_f32(in, H, 0, 0, w_ih[l], H, bias[l], nullptr, 0, 0, xp, 4 * H, B * T, 4 * H, H, PM_ACT_NONE, stream);
    if (rc != PM_OK) return rc;
    const bool last = l + 1 == n_layers;
    LstmRole r0 = {xp, nullptr, nullptr, nullptr, w_hh[l], hbuf[l & 1], cbuf[0], last && residual ? x : nullptr, last ? y : nullptr, 0};
    for (int64_t t = 0; t < T; ++t) {
      r0.t = (int)t;
      hipLaunchKernelGGL(lstm_step_kernel, dim3(nb), dim3(256), 0, st, r0, idle, (int)B, (int)T, (int)H);
    }
    PM_CHECK_LAUNCH();
    in = hbuf[l & 1];
  }
  return PM_OK;
}

extern "C" int pm_rvq_encode_f32(const float* z, const float* codebooks, const float* norms, int64_t* codes, int64_t M,
                                 int64_t n_q, int64_t dim, int64_t codebook_size, void* stream) {
  if (!z || !codebooks || !norms || !codes || M < 0 || n_q < 1) return PM_EINVAL;
  if (dim != RVQ_D || codebook_size != RVQ_N) return PM_EUNSUPPORTED;
  if (M == 0) return PM_OK;
  if (M >= (1ll << 31) - 16) return PM_EINVAL;
  if (((uintptr_t)z | (uintptr_t)codebooks | (uintptr_t)norms) & 15) return PM_EALIGN;
  hipLaunchKernelGGL(rvq_encode_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, (hipStream_t)stream, z, codebooks, norms,
                     codes, (int)M, (int)n_q);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_rvq_decode_f32(const int64_t* codes, int64_t stride_b, int64_t stride_q, int64_t stride_t,
                                 const float* codebooks, float* out, int64_t B, int64_t T, int64_t n_q, int64_t dim,
                                 int64_t codebook_size, void* stream) {
  if (!codes || !codebooks || !out || B < 0 || T < 0 || n_q < 1) return PM_EINVAL;
  if (dim != RVQ_D || codebook_size != RVQ_N) return PM_EUNSUPPORTED;
  const int64_t M = B * T;
  if (M == 0) return PM_OK;
  if (T >= (1ll << 31) || M * 32 / 256 + 1 > 0x7fffffff) return PM_EINVAL;
  if (((uintptr_t)codebooks | (uintptr_t)out) & 15) return PM_EALIGN;
  hipLaunchKernelGGL(rvq_decode_kernel, dim3((unsigned)((M * 32 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes,
                     stride_b, stride_q, stride_t, codebooks, out, M, (int)T, (int)n_q);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int64_t pm_groupnorm1_workspace_doubles(int64_t B, int64_t n) { return B * ((n + GN_CHUNK - 1) / GN_CHUNK) * 2; }

extern "C" int pm_groupnorm1_f32(float* x, const float* gamma, const float* beta, const float* resid, double* work, int64_t B,
                                 int64_t n, int64_t C, float eps, void* stream) {
  if (!x || !gamma || !beta || !work || B < 0 || n < 1 || C < 1 || n % C) return PM_EINVAL;
  if (B == 0) return PM_OK;
  const int64_t nchunk = (n + GN_CHUNK - 1) / GN_CHUNK;
  if (B > 65535 || nchunk > 0x7fffffff || C >= (1ll << 31)) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, st, x, work, n, (int)nchunk);
  hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, st, x, work, gamma, beta, resid, n,
                     (int)C, (int)nchunk, eps);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_encodec_scale_f32(const float* x, float* scale, int64_t B, int64_t C, int64_t T, void* stream) {
  if (!x || !scale || B < 0 || C < 1 || T < 1 || C >= (1ll << 31)) return PM_EINVAL;
  if (B == 0) return PM_OK;
  if (B > 0x7fffffff) return PM_EINVAL;
  hipLaunchKernelGGL(encodec_scale_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, x, scale, (int)C, T);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_scale_clips_f32(const float* x, const float* scale, float* y, int64_t B, int64_t n, int divide, void* stream) {
  if (!x || !scale || !y || B < 0 || n < 1) return PM_EINVAL;
  if (B == 0) return PM_OK;
  if (B > 65535) return PM_EINVAL;
  int64_t gx = (n + 255) / 256;
  gx = gx > 1024 ? 1024 : gx;
  hipLaunchKernelGGL(scale_clips_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, scale, y, n,
                     divide);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
