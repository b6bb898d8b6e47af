// cls_tail.hip - the last encoder layer of a class-token ViT, computed for the class-token row only.
//
// Of the last layer's output only token 0 of each image is read (ViT.forward with ClassTokenPooling), and everything behind
// that layer's attention is row-wise, so the layer needs ONE query per image and head.  With W'k, W'v the k / v weights with
// sa_norm's gamma folded in, c_v = W_v beta + b_v, x_j the stored token rows and (mean_j, rstd_j) their sa_norm statistics:
//
//   scores   q_h . k_j = rstd_j (u_h . x_j - mean_j sum(u_h)) + const_h      u_h = W'k,h^T q_h  (a d-vector; softmax drops const_h)
//   output   o_h = W'v,h ctx_h + c_v,h                                       ctx_h = sum_j p_hj rstd_j (x_j - mean_j)
//
// so neither K nor V is ever projected: two small per-head GEMMs (pm_cls_head_gemm) and one pass over the residual stream
// (pm_cls_attend).
//
//  * pm_cls_attend   one workgroup (4 waves) per image.  The image's rows stream through LDS in blocks of 32 (LDS-DMA, double
//    buffered, [64-column panel][row][128 B] with the XOR swizzle of swz_pos riding on the SOURCE addresses).  Per block:
//      A  S[h][j] = u_h . x_j on the matrix pipe, heads padded to 16 (mfma 16x16x32: A = u fragments held in registers, wave w
//         owns the K steps w, w+4, ..; B = row fragments, ds_read_b128); the four waves' partial sums meet in LDS, summed in
//         wave order;
//      B  online softmax per head (16 lanes per head): s = scale rstd_j (S - mean_j sum(u_h)), running max / sum, and the
//         block's weights w_hj = bf16(exp(s - m) rstd_j);
//      C  ctx^T[c][h] += sum_j x[j][c] w[h][j] (mfma 16x16x32, A = the block's rows read TRANSPOSED with ds_read_b64_tr_b16,
//         B = w; wave w owns the 16-column tiles w, w+4, ..; the accumulator has the head on the lane, so the rescale is one
//         factor per lane), and in the softmax lanes cm_h += sum_j w_hj mean_j.
//    Result ctx_h = (acc_h - cm_h) / l_h.  This is the RAW-ROW form: the rows are weighted as stored and the mean enters once, as
//    cm.  Both sums use the SAME bf16-rounded weights, so their difference is sum_j w_hj (x_j - mean_j) up to fp32 accumulation
//    error - a row whose |mean| is 4x its std costs two bits of an fp32 sum, nothing of the bf16 result (tests/test_hip_cls_tail.py).
//    A normalised copy of x would add a rounding point and an LDS pass instead.
//    Without statistics (stats == NULL) the kernel computes mean and rstd of each row from the block in LDS (two passes, fp32).
//    A workgroup owns a whole image and sums in a fixed order: the result does not depend on the batch size or position.
//  * pm_cls_head_gemm   y[:, g] = x[:, g] W[g]^T (+ bias) for G groups in one launch: 16 rows x 64 features per workgroup,
//    the K steps dealt to the 4 waves and summed in wave order through LDS; operands straight from global memory (L2-resident).
//    Rows are independent lanes of the MFMA: a row's sum does not depend on M or on the row's position.
#include "common.h"

namespace {

constexpr int CT_JB = 32;        // rows per block = one K step of the context MFMA
constexpr int CT_THREADS = 256;  // 4 waves, one per SIMD
constexpr int CT_MAX_D = 1024;   // u fragments (8 per wave) and context tiles (16 per wave) live in registers
constexpr int CT_SIDE_BYTES = 4 * 16 * CT_JB * 4 + 16 * CT_JB * 2 + CT_JB * 2 * 4 + 16 * 4 + 4 * 16 * 4 + 16 * 2 * 4;

// LDS-DMA hidden from hipcc, as in attention_bf16.hip: with the builtin form every later ds_read_b64_tr_b16 is ordered behind a
// vmcnt(0), and the next block's prefetch would never overlap this block's arithmetic.  The completion is counted by hand: the
// vmcnt(0) in front of the barrier at the top of a block.
__device__ __forceinline__ void ct_glds16(const void* gsrc, unsigned lds_dst_wave_base) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst_wave_base);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(dst)
               : "memory");
}

__device__ __forceinline__ bf16x8 ct_tr_pair(const unsigned char* p0, const unsigned char* p1) {
  union { s16x4 h[2]; bf16x8 v; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((PM_LDS s16x4*)p0);
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((PM_LDS s16x4*)p1);
  return u.v;
}

__device__ __forceinline__ float sum16(float v) {  // over the 16 lanes of an aligned group, the same bits in every lane
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float max16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(CT_THREADS) void cls_attend_kernel(const bf16* __restrict__ x, int64_t x_rs, int64_t x_bs,
                                                                const float* __restrict__ stats, const bf16* __restrict__ u,
                                                                bf16* __restrict__ ctx, int L, int d, int H, float scale, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // in a scalar register: the guards on a wave's K steps / tiles are scalar branches
  const int n = blockIdx.x;
  const int P = d >> 6, nks = d >> 5, nct = d >> 4;
  const int XB = 64 * d;  // bytes of one block of rows
  float* sc = (float*)(smem + 2 * XB);  // [wave][head][row]: partial scores
  bf16* wt = (bf16*)(sc + 4 * 16 * CT_JB);  // [head][row]: the block's weights
  float* st = (float*)(wt + 16 * CT_JB);    // [row][mean, rstd]
  float* al = st + CT_JB * 2;               // [head]: rescale factor of the block
  float* su = al + 16;                      // [wave][head]: partial sums of u
  float* fin = su + 4 * 16;                 // [head][cm, l]
  const unsigned lds0 = (unsigned)(uintptr_t)(PM_LDS unsigned char*)smem;
  const bf16* xn = x + (int64_t)n * x_bs;
  const int nblk = (L + CT_JB - 1) / CT_JB;

  // rows past L are served by row L - 1 (finite values; their weights are exact zeros)
  auto stage = [&](int b) {
    const unsigned buf = lds0 + (b & 1) * XB;
    for (int pc = wv; pc < 4 * P; pc += 4) {
      const int p = pc >> 2, rg = pc & 3;
      const int r = rg * 8 + (lane >> 3), c = swz_pos(r, lane & 7);
      const int j = min(b * CT_JB + r, L - 1);
      ct_glds16(xn + (int64_t)j * x_rs + p * 64 + c * 8, buf + p * 4096 + rg * 1024);
    }
  };
  // the block's given statistics travel one block ahead in a register, requested BEFORE the block's LDS-DMA pieces: a load
  // requested behind them would be waited for together with them (vmcnt counts in order) and the prefetch would hide nothing
  f32x2 stn = {0.f, 1.f};
  if (stats && tid < CT_JB) stn = *(const f32x2*)(stats + ((int64_t)n * L + min(tid, L - 1)) * 2);
  stage(0);

  // u fragments of this wave's K steps (A operand: head fr, columns 32 ks + 8 fq ..), and the heads' sums of u
  bf16x8 uf[8];
  {
    const bf16* up = u + ((int64_t)n * H + min(fr, H - 1)) * d + fq * 8;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int ks = wv + 4 * t;
      bf16x8 v = *(const bf16x8*)(up + min(ks, nks - 1) * 32);
      if (ks >= nks || fr >= H)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (bf16)0.0f;
      uf[t] = v;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (float)v[e];
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (fq == 0) su[wv * 16 + fr] = s;
  }

  f32x4 acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // softmax lanes: head sh, rows sj and sj + 16 of a block
  const int sh = tid >> 4, sj = tid & 15;
  float m_run = -INFINITY, l_run = 0.f, cm_run = 0.f, su_h = 0.f;

  for (int b = 0; b < nblk; ++b) {
    const unsigned char* buf = smem + (b & 1) * XB;
    const int j0 = b * CT_JB;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of block b have landed
    __syncthreads();                                   // everyone's have; and everyone is done with the other buffer
    if (stats && tid < CT_JB) {
      *(f32x2*)(st + 2 * tid) = stn;
      if (b + 1 < nblk) stn = *(const f32x2*)(stats + ((int64_t)n * L + min(j0 + CT_JB + tid, L - 1)) * 2);
    }
    if (b + 1 < nblk) stage(b + 1);
    if (b == 0) su_h = su[sh] + su[16 + sh] + su[32 + sh] + su[48 + sh];

    // ---- no statistics given: from the rows in LDS (wave w takes rows 8w .. 8w+7)
    if (!stats) {
      for (int rr = 0; rr < 8; ++rr) {
        const int r = wv * 8 + rr;
        float s = 0.f;
        for (int c = lane; c < d / 8; c += 64) {
          const bf16x8 v = *(const bf16x8*)(buf + (c >> 3) * 4096 + r * 128 + swz_pos(r, c & 7) * 16);
#pragma unroll
          for (int e = 0; e < 8; ++e) s += (float)v[e];
        }
        const float mean = wave_sum(s) / (float)d;
        float q = 0.f;
        for (int c = lane; c < d / 8; c += 64) {
          const bf16x8 v = *(const bf16x8*)(buf + (c >> 3) * 4096 + r * 128 + swz_pos(r, c & 7) * 16);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dv = (float)v[e] - mean;
            q = fmaf(dv, dv, q);
          }
        }
        const float var = wave_sum(q) / (float)d;
        if (lane == 0) {
          st[2 * r] = mean;
          st[2 * r + 1] = rsqrtf(var + eps);
        }
      }
    }

    // ---- A: partial scores of this wave's K steps
    {
      f32x4 sa[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int ks = wv + 4 * t;
        if (ks < nks) {
          const unsigned char* pb = buf + (ks >> 1) * 4096;
          const int ch = (ks & 1) * 4 + fq;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            const int row = jt * 16 + fr;
            const bf16x8 bx = *(const bf16x8*)(pb + row * 128 + swz_pos(row, ch) * 16);
            sa[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(uf[t], bx, sa[jt], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(wv * 16 + fq * 4 + i) * CT_JB + jt * 16 + fr] = sa[jt][i];
    }
    __syncthreads();

    // ---- B: online softmax, the block's weights
    {
      float s[2], mean[2], rstd[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int j = sj + 16 * r;
        const float dot = ((sc[sh * CT_JB + j] + sc[(16 + sh) * CT_JB + j]) + sc[(32 + sh) * CT_JB + j]) + sc[(48 + sh) * CT_JB + j];
        mean[r] = st[2 * j];
        rstd[r] = st[2 * j + 1];
        s[r] = j0 + j < L ? scale * rstd[r] * (dot - mean[r] * su_h) : -INFINITY;
      }
      const float m_new = fmaxf(m_run, max16(fmaxf(s[0], s[1])));  // finite: row j0 of a block is always a real row
      const float alpha = __expf(m_run - m_new);
      const float p0 = __expf(s[0] - m_new), p1 = __expf(s[1] - m_new);
      const bf16 w0 = (bf16)(p0 * rstd[0]), w1 = (bf16)(p1 * rstd[1]);
      l_run = fmaf(l_run, alpha, sum16(p0 + p1));
      cm_run = fmaf(cm_run, alpha, sum16(fmaf((float)w0, mean[0], (float)w1 * mean[1])));
      m_run = m_new;
      wt[sh * CT_JB + sj] = w0;
      wt[sh * CT_JB + sj + 16] = w1;
      if (sj == 0) al[sh] = alpha;
    }
    __syncthreads();

    // ---- C: ctx^T[c][h] = alpha_h ctx^T[c][h] + sum_j x[j][c] w[h][j]
    {
      const bf16x8 wf = *(const bf16x8*)(wt + fr * CT_JB + fq * 8);  // B operand: head fr, rows 8 fq ..
      const float a = al[fr];
      // transposed read (cdna_hip_programming.md T10): lane 4q+p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a
      // 4 x 16 block and receives column (lane & 15); the group fq takes rows 8 fq .. 8 fq + 3 and 8 fq + 4 .. + 7
      const int q = fr >> 2, p = fr & 3;
      const int r0 = 8 * fq + q, r1 = r0 + 4;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int ct = wv + 4 * t;
        if (ct < nct) {  // wave-uniform: EXEC stays all ones for the transposed reads
          const unsigned char* pb = buf + (ct >> 2) * 4096;
          const int ch = (ct & 3) * 2 + (p >> 1);
          const bf16x8 xf = ct_tr_pair(pb + r0 * 128 + swz_pos(r0, ch) * 16 + (p & 1) * 8,
                                       pb + r1 * 128 + swz_pos(r1, ch) * 16 + (p & 1) * 8);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, wf, acc[t] * a, 0, 0, 0);
        }
      }
    }
  }

  if (sj == 0) {
    fin[2 * sh] = cm_run;
    fin[2 * sh + 1] = l_run;
  }
  __syncthreads();
  if (fr < H) {  // D[channel 4 fq + i of the tile][head fr]
    const float cm = fin[2 * fr], inv = 1.0f / fin[2 * fr + 1];
    bf16* cp = ctx + ((int64_t)n * H + fr) * d + fq * 4;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int ct = wv + 4 * t;
      if (ct < nct) {
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)((acc[t][i] - cm) * inv);
        *(bf16x4*)(cp + ct * 16) = o;
      }
    }
  }
}

// y[m][g][n] = sum_k x[m][g][k] w[g][n][k] (+ bias[g][n]).  Workgroup: rows m0 .. m0+15, features n0 .. n0+63 of group g.
__global__ __launch_bounds__(256) void cls_head_gemm_kernel(const bf16* __restrict__ x, int64_t ldx, int64_t xg,
                                                            const bf16* __restrict__ w, const float* __restrict__ bias,
                                                            bf16* __restrict__ y, int64_t ldy, int64_t yg, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float red[4][16][68];  // [wave][row][feature], rows padded
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 64, g = blockIdx.z;
  const bf16* xp = x + (int64_t)min(m0 + fr, M - 1) * ldx + (int64_t)g * xg + fq * 8;  // B operand: row fr
  const bf16* wp = w + ((int64_t)g * N + n0 + fr) * K + fq * 8;                         // A operand: feature fr of a 16-tile
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nks = K >> 5;
  for (int ks = wv; ks < nks; ks += 4) {
    const bf16x8 b = *(const bf16x8*)(xp + ks * 32);
    bf16x8 a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = *(const bf16x8*)(wp + (int64_t)j * 16 * K + ks * 32);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b, acc[j], 0, 0, 0);
  }
  // D[feature 4 fq + i][row fr]
#pragma unroll
  for (int j = 0; j < 4; ++j) *(f32x4*)&red[wv][fr][j * 16 + fq * 4] = acc[j];
  __syncthreads();
  const int row = tid >> 4, c4 = (tid & 15) * 4;
  if (m0 + row < M) {
    f32x4 v = ((*(const f32x4*)&red[0][row][c4] + *(const f32x4*)&red[1][row][c4]) + *(const f32x4*)&red[2][row][c4]) +
              *(const f32x4*)&red[3][row][c4];
    if (bias) v += *(const f32x4*)(bias + (int64_t)g * N + n0 + c4);
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (bf16)v[i];
    *(bf16x4*)(y + (int64_t)(m0 + row) * ldy + (int64_t)g * yg + n0 + c4) = o;
  }
}

inline bool ct_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int pm_cls_attend_supported(int64_t L, int64_t d, int64_t H) {
  return L >= 1 && L <= (1 << 20) && d >= 64 && d % 64 == 0 && d <= CT_MAX_D && H >= 1 && H <= 16 ? 1 : 0;
}

extern "C" int pm_cls_attend(const void* x, int64_t x_row_stride, int64_t x_batch_stride, const float* stats, const void* u,
                             void* ctx, int64_t N, int64_t L, int64_t d, int64_t H, float scale, float eps, void* stream) {
  if (!x || !u || !ctx || N < 0 || L < 1 || d < 64 || d % 64 || H < 1 || H > 16 || x_row_stride < d) return PM_EINVAL;
  if (d > CT_MAX_D || L > (1 << 20) || N > 0x7fffffff) return PM_EUNSUPPORTED;
  if (!ct_al(x, 16) || !ct_al(u, 16) || !ct_al(ctx, 8) || !ct_al(stats, 8) || x_row_stride % 8 || x_batch_stride % 8) return PM_EALIGN;
  if (N == 0) return PM_OK;
  const size_t lds = (size_t)(2 * 64 * d + CT_SIDE_BYTES);
  if (lds > 64 * 1024) {
    static bool raised = false;  // (outside any stream capture: captures follow a warm-up; setting it twice is harmless)
    if (!raised) {
      if (hipFuncSetAttribute((const void*)cls_attend_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * CT_MAX_D + CT_SIDE_BYTES) !=
          hipSuccess)
        return PM_ELAUNCH;
      raised = true;
    }
  }
  hipLaunchKernelGGL(cls_attend_kernel, dim3((unsigned)N), dim3(CT_THREADS), lds, (hipStream_t)stream, (const bf16*)x, x_row_stride,
                     x_batch_stride, stats, (const bf16*)u, (bf16*)ctx, (int)L, (int)d, (int)H, scale, eps);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_cls_head_gemm(const void* x, int64_t ldx, int64_t x_group_stride, const void* w, const float* bias, void* y,
                                int64_t ldy, int64_t y_group_stride, int64_t M, int64_t N, int64_t K, int64_t G, void* stream) {
  if (!x || !w || !y || M < 0 || N < 64 || N % 64 || K < 32 || K % 32 || G < 1) return PM_EINVAL;
  if (G > 65535 || N / 64 > 65535 || M > (1 << 24) || K > (1 << 20)) return PM_EUNSUPPORTED;
  if (!ct_al(x, 16) || !ct_al(w, 16) || !ct_al(y, 8) || !ct_al(bias, 16) || ldx % 8 || x_group_stride % 8 || ldy % 4 || y_group_stride % 4)
    return PM_EALIGN;
  if (M == 0) return PM_OK;
  const dim3 grid((unsigned)((M + 15) / 16), (unsigned)(N / 64), (unsigned)G);
  hipLaunchKernelGGL(cls_head_gemm_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, x_group_stride, (const bf16*)w,
                     bias, (bf16*)y, ldy, y_group_stride, (int)M, (int)N, (int)K);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
