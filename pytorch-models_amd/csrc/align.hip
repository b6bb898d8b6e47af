// align.hip - Whisper token timestamps: cross-attention alignment matrix and dynamic time warping.
//
// For the selected (layer, head) pairs a = 0 .. A - 1 of a teacher-forced decoder pass, with q_t (L rows) and k_f (S rows) the
// 64-wide head slices of the cross-attention projections of one clip, len <= L tokens and F <= S frames:
//   p[a, t, f] = softmax_{f < F}(q_t . k_f / 8)                                        t < len
//   n[a, t, f] = (p - mean_t p) / std_t p      (biased std over t < len; a column whose rows are all equal - std exactly 0 - gives 0)
//   m[t, f]    = 1 / A  sum_a  median7_f(n[a, t, :])   (reflect padding at 0 and F - 1)
//   start[t]   = first frame of token row t on the DTW path through -m[skip_first : len - skip_last, 0 : F]
// The (A, L, F) probabilities never exist in memory.  Three kernels, no atomics, every clip's outputs bit-identical wherever
// the clip sits in the batch and whatever the batch size is:
//
// align_lse_kernel     one wave per 16 token rows of one (clip, head): k streams through the bf16 MFMA 16 frames at a time
//                      (A operand = 16 frames, B operand = 16 tokens, two K steps of 32), each lane folds its 4 logits per
//                      tile into a running (max, sum) and the 4 lanes of a token merge once at the end.  Writes lse only.
// align_matrix_kernel  one workgroup per (clip, tile of MT_W = 26 frames): it computes the 32 columns f0 - 3 .. f0 + 28 (the
//                      tile plus the 3-frame halo of the median on each side) for ALL len rows and loops over the heads of
//                      the launch: logits again on the MFMA -> p = exp(logit - lse) into LDS (448 x 33 floats) -> column mean
//                      and a true two-pass variance from LDS -> normalised in place -> median of 7 as a register sorting
//                      network -> per-thread register accumulators (a thread owns rows tid and tid + 256 of the tile).  One
//                      write of m at the end: `first` overwrites (and writes the zeros outside len and F), else adds.
//                      The deviations are scaled by an exact power of two taken from the column mean before they are squared,
//                      so a column of probabilities around 1e-37 (one frame 80 above the rest) neither underflows to std = 0
//                      nor loses a bit.
// align_dtw_kernel     one workgroup of 448 threads per clip, thread r = token row r of the window.  Anti-diagonal d holds
//                      the cells (r, d - r); a thread keeps cost[r][j - 1] in a register, reads cost[r - 1][j] from LDS (its
//                      neighbour's value of the previous diagonal) and remembers the one before as cost[r - 1][j - 1]: one
//                      barrier per diagonal.  Every 32 diagonals the workgroup reloads the skewed band x[r][d0 - r + s] it
//                      will need into LDS (coalesced along the rows) and each thread stores its 32 two-bit trace codes as ONE
//                      8-byte word: no global access inside the 32 barriers in between.  Thread 0 then walks the trace back
//                      (at most N + M moves by construction, whatever the matrix holds) and the workgroup writes start.
//                      The additions and strict comparisons are those of the published recurrence, one fp32 add per cell.
#include <float.h>

#include "common.h"

namespace {

constexpr int AL_MAXL = 448;   // token rows a workgroup of the matrix / DTW kernels holds (Whisper's decoder length)
constexpr int MT_W = 26;       // output frames per matrix tile
constexpr int MT_C = 32;       // computed columns per tile: MT_W + 2 * 3
constexpr int MT_PS = 33;      // LDS row stride (floats) of the probability tile
constexpr int DT_T = 32;       // diagonals per DTW block
constexpr int DT_PS = 33;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float al_exp(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }
__device__ __forceinline__ int al_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ bf16x8 al_ld8(const bf16* p) { return *(const bf16x8*)p; }

// logits of 16 frames x 16 tokens: D[frame 4 (lane >> 4) + r][token lane & 15]
__device__ __forceinline__ f32x4 al_qk(const bf16x8 (&kf)[2], const bf16x8 (&qf)[2]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0], qf[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1], qf[1], acc, 0, 0, 0);
  return acc;
}

__global__ __launch_bounds__(256) void align_lse_kernel(const bf16* __restrict__ Q, int64_t ldq, int64_t qbs,
                                                        const bf16* __restrict__ K, int64_t ldk, int64_t kbs,
                                                        const int* __restrict__ heads, const int* __restrict__ lengths,
                                                        const int* __restrict__ frames, float* __restrict__ lse, int L, int S,
                                                        int nh, int H) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.z, a = blockIdx.y;
  const int h = al_clamp(heads[a], 0, H - 1);
  const int len = al_clamp(lengths[b], 1, L), F = al_clamp(frames[b], 1, S);
  const int row0 = blockIdx.x * 64 + wave * 16;
  if (row0 >= len) return;  // (no barrier in this kernel)
  const int qrow = row0 + fr < len ? row0 + fr : len - 1;
  const bf16* qp = Q + (int64_t)b * qbs + (int64_t)qrow * ldq + h * 64 + fq * 8;
  const bf16x8 qf[2] = {al_ld8(qp), al_ld8(qp + 32)};
  const bf16* kb = K + (int64_t)b * kbs + h * 64 + fq * 8;
  float m = -FLT_MAX, s = 0.f;
  for (int f0 = 0; f0 < F; f0 += 16) {
    const int frow = f0 + fr < F ? f0 + fr : F - 1;
    const bf16* kp = kb + (int64_t)frow * ldk;
    const bf16x8 kf[2] = {al_ld8(kp), al_ld8(kp + 32)};
    const f32x4 acc = al_qk(kf, qf);
    float x[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      x[r] = f0 + fq * 4 + r < F ? acc[r] * 0.125f : -INFINITY;
      tmax = fmaxf(tmax, x[r]);
    }
    const float mn = fmaxf(m, tmax);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) sum += al_exp(x[r] - mn);
    s = s * al_exp(m - mn) + sum;
    m = mn;
  }
#pragma unroll
  for (int mask = 16; mask <= 32; mask <<= 1) {
    const float mo = __shfl_xor(m, mask, 64), so = __shfl_xor(s, mask, 64);
    const float mn = fmaxf(m, mo);
    s = s * al_exp(m - mn) + so * al_exp(mo - mn);
    m = mn;
  }
  if (fq == 0 && row0 + fr < len) lse[((int64_t)b * nh + a) * L + row0 + fr] = m + logf(s);
}

#define AL_SORT2(A, B)            \
  {                               \
    const float lo_ = fminf(A, B); \
    B = fmaxf(A, B);              \
    A = lo_;                      \
  }
// median of 7: the 13-exchange selection network (checked on all 128 zero-one inputs by tests/test_align_cases_cpu.py)
__device__ __forceinline__ float al_med7(float p0, float p1, float p2, float p3, float p4, float p5, float p6) {
  AL_SORT2(p0, p5) AL_SORT2(p0, p3) AL_SORT2(p1, p6) AL_SORT2(p2, p4) AL_SORT2(p0, p1) AL_SORT2(p3, p5) AL_SORT2(p2, p6)
  AL_SORT2(p2, p3) AL_SORT2(p3, p6) AL_SORT2(p4, p5) AL_SORT2(p1, p4) AL_SORT2(p1, p3) AL_SORT2(p3, p4)
  return p3;
}
#undef AL_SORT2

__global__ __launch_bounds__(256) void align_matrix_kernel(const bf16* __restrict__ Q, int64_t ldq, int64_t qbs,
                                                           const bf16* __restrict__ K, int64_t ldk, int64_t kbs,
                                                           const int* __restrict__ heads, const int* __restrict__ lengths,
                                                           const int* __restrict__ frames, const float* __restrict__ lse,
                                                           float* __restrict__ Mo, int64_t ldm, int64_t mbs, int L, int S, int nh,
                                                           int H, float inv_heads, int first) {
  __shared__ float P[AL_MAXL * MT_PS];
  __shared__ int bad_tile;  // a column of this tile holds a NaN probability (a NaN in q, k or lse): see the store below
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.y, f0 = blockIdx.x * MT_W;
  if (tid == 0) bad_tile = 0;  // (the first barrier of the head loop is in front of every other write and every read of it: the
                               // launcher refuses nh < 1, so the loop runs at least once)
  const int len = al_clamp(lengths[b], 1, L), F = al_clamp(frames[b], 1, S);
  const int nout = al_clamp((F < f0 + MT_W ? F : f0 + MT_W) - f0, 0, MT_W);  // frames of this tile below F
  const int wcols = (S < f0 + MT_W ? S : f0 + MT_W) - f0;                     // frames of this tile below S

  if (nout > 0) {
    float acc[2][MT_W];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int o = 0; o < MT_W; ++o) acc[rr][o] = 0.f;
    const bool interior = f0 >= 3 && f0 + MT_W + 3 <= F;
    const bf16* qb = Q + (int64_t)b * qbs + fq * 8;
    const bf16* kb = K + (int64_t)b * kbs + fq * 8;

    for (int a = 0; a < nh; ++a) {
      const int h = al_clamp(heads[a], 0, H - 1);
      // ---- 1: p = exp(logit - lse) of rows [0, len) x columns f0 - 3 + [0, 32) into LDS (frames outside [0, F) are clamped:
      // their columns are computed and never read)
      bf16x8 kf[2][2];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int frow = al_clamp(f0 - 3 + jt * 16 + fr, 0, F - 1);
        const bf16* kp = kb + (int64_t)frow * ldk + h * 64;
        kf[jt][0] = al_ld8(kp);
        kf[jt][1] = al_ld8(kp + 32);
      }
      const float* lse_a = lse + ((int64_t)b * nh + a) * L;
      for (int rb = wave; rb * 16 < len; rb += 4) {
        const int trow = rb * 16 + fr;  // <= 447
        const int qrow = trow < len ? trow : len - 1;
        const bf16* qp = qb + (int64_t)qrow * ldq + h * 64;
        const bf16x8 qf[2] = {al_ld8(qp), al_ld8(qp + 32)};
        const float ls = lse_a[qrow];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          const f32x4 d = al_qk(kf[jt], qf);
#pragma unroll
          for (int r = 0; r < 4; ++r) P[trow * MT_PS + jt * 16 + fq * 4 + r] = al_exp(d[r] * 0.125f - ls);
        }
      }
      __syncthreads();
      // ---- 2: column statistics over t < len, 8 threads per column, and the normalisation in place
      {
        const int c = tid >> 3, part = tid & 7;
        float sum = 0.f, vmax = 0.f, vmin = FLT_MAX;  // (p >= 0; part 0 always has a row)
        for (int t = part; t < len; t += 8) {
          const float v = P[t * MT_PS + c];
          sum += v;
          vmax = fmaxf(vmax, v);
          vmin = fminf(vmin, v);
        }
#pragma unroll
        for (int mask = 1; mask <= 4; mask <<= 1) {
          sum += __shfl_xor(sum, mask, 64);
          vmax = fmaxf(vmax, __shfl_xor(vmax, mask, 64));
          vmin = fminf(vmin, __shfl_xor(vmin, mask, 64));
        }
        const bool flat = vmax == vmin;  // all rows equal: the std is exactly 0 whatever the rounding of the mean
        if (part == 0 && sum != sum) bad_tile = 1;  // (every writer writes 1)
        const float mean = sum / (float)len;
        // exact power-of-two scale 2^(127 - e) of the deviations, e the biased exponent of the mean (p <= 1, so e <= 127)
        int e = (__float_as_int(mean) >> 23) & 255;
        e = e < 1 ? 1 : (e > 253 ? 253 : e);
        const float scale = __int_as_float((254 - e) << 23);
        float ss = 0.f;
        for (int t = part; t < len; t += 8) {
          const float dv = (P[t * MT_PS + c] - mean) * scale;
          ss += dv * dv;
        }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
        const float sd = sqrtf(ss / (float)len);
        for (int t = part; t < len; t += 8) {
          const float dv = (P[t * MT_PS + c] - mean) * scale;
          P[t * MT_PS + c] = (sd > 0.f && !flat) ? dv / sd : 0.f;
        }
      }
      __syncthreads();
      // ---- 3: median of 7 along the frames, into the thread's accumulators
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int t = tid + rr * 256;
        if (t < len) {
          const float* row = P + t * MT_PS;
          if (interior) {
            float v[MT_C];
#pragma unroll
            for (int c = 0; c < MT_C; ++c) v[c] = row[c];
#pragma unroll
            for (int o = 0; o < MT_W; ++o) acc[rr][o] += al_med7(v[o], v[o + 1], v[o + 2], v[o + 3], v[o + 4], v[o + 5], v[o + 6]);
          } else {
#pragma unroll
            for (int o = 0; o < MT_W; ++o) {
              if (o < nout) {
                float w[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                  int f = f0 + o + i - 3;
                  f = f < 0 ? -f : f;
                  f = f > F - 1 ? 2 * (F - 1) - f : f;
                  f = al_clamp(f, 0, F - 1);  // (F >= 4 never needs it)
                  w[i] = row[al_clamp(f - (f0 - 3), 0, MT_C - 1)];
                }
                acc[rr][o] += al_med7(w[0], w[1], w[2], w[3], w[4], w[5], w[6]);
              }
            }
          }
        }
      }
      __syncthreads();
    }
    // the tile's result through LDS, so that the store below runs along the frames.  The normalisation (sd > 0 is false for a NaN
    // deviation) and the median's min / max exchanges both drop a NaN; a tile that met one reports NaN instead of looking healthy
    const bool bad = bad_tile != 0;  // (behind the head loop's last barrier)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int t = tid + rr * 256;
      if (t < len) {
#pragma unroll
        for (int o = 0; o < MT_W; ++o) P[t * MT_PS + o] = bad ? __builtin_nanf("") : acc[rr][o] * inv_heads;
      }
    }
    __syncthreads();
  }
  if (nout == 0 && !first) return;
  float* mo = Mo + (int64_t)b * mbs + f0;
  for (int idx = tid; idx < L * wcols; idx += 256) {
    const int t = idx / wcols, o = idx - t * wcols;
    float* dst = mo + (int64_t)t * ldm + o;
    if (t < len && o < nout) {
      const float v = P[t * MT_PS + o];
      *dst = first ? v : *dst + v;
    } else if (first) {
      *dst = 0.f;
    }
  }
}

__global__ __launch_bounds__(AL_MAXL) void align_dtw_kernel(const float* __restrict__ Mg, int64_t ldm, int64_t mbs,
                                                            const int* __restrict__ lengths, const int* __restrict__ frames,
                                                            int* __restrict__ start, uint2* ws, int L, int S, int nblk,
                                                            int skip_first, int skip_last) {
  __shared__ float Xs[AL_MAXL * DT_PS];
  __shared__ float Cs[2 * AL_MAXL];
  const int tid = threadIdx.x, r = tid;
  const int b = blockIdx.x;
  const int len = al_clamp(lengths[b], 1, L), M = al_clamp(frames[b], 1, S);
  const int N = len - skip_first - skip_last;
  int* srow = start + (int64_t)b * L;
  if (N <= 0) {  // uniform: nothing is aligned
    for (int t = tid; t < L; t += AL_MAXL) srow[t] = -1;
    return;
  }
  const float* mg = Mg + (int64_t)b * mbs + (int64_t)skip_first * ldm;
  uint2* wsb = ws + (int64_t)b * nblk * L;
  const int nsteps = N + M - 1;
  float left = INFINITY, upprev = INFINITY;
  for (int blk = 0, d0 = 0; d0 < nsteps; ++blk, d0 += DT_T) {
    // the skewed band of this block: Xs[row][s] = x[row][d0 + s - row] = -m
    for (int idx = tid; idx < N * DT_T; idx += AL_MAXL) {
      const int rr = idx >> 5, s = idx & 31, j = d0 + s - rr;
      if (j >= 0 && j < M) Xs[rr * DT_PS + s] = -mg[(int64_t)rr * ldm + j];
    }
    __syncthreads();
    unsigned lo = 0, hi = 0;
    const int send = nsteps - d0 < DT_T ? nsteps - d0 : DT_T;
    for (int s = 0; s < send; ++s) {
      const int d = d0 + s, j = d - r;
      if (r < N && j >= 0 && j < M) {
        const float c1 = r == 0 ? INFINITY : Cs[((d - 1) & 1) * AL_MAXL + r - 1];
        const float c0 = j == 0 ? (r == 0 ? 0.f : INFINITY) : (r == 0 ? INFINITY : upprev);
        const float c2 = j == 0 ? INFINITY : left;
        float c;
        unsigned t;
        if (c0 < c1 && c0 < c2) {
          c = c0;
          t = 0;
        } else if (c1 < c0 && c1 < c2) {
          c = c1;
          t = 1;
        } else {
          c = c2;
          t = 2;
        }
        const float cost = Xs[r * DT_PS + s] + c;
        Cs[(d & 1) * AL_MAXL + r] = cost;
        left = cost;
        upprev = c1;
        if (s < 16) lo |= t << (2 * s);
        else hi |= t << (2 * (s - 16));
      }
      __syncthreads();
    }
    if (r < N) wsb[(int64_t)blk * L + r] = make_uint2(lo, hi);
  }
  __syncthreads();  // the trace words of every wave are visible to thread 0
  int* st = (int*)Xs;
  for (int t = tid; t < N; t += AL_MAXL) st[t] = -1;
  __syncthreads();
  if (tid == 0) {
    int i = N, j = M, cb = -1, cr = -1;
    uint2 w = make_uint2(0u, 0u);
    for (int it = 0; it < N + M && (i > 0 || j > 0); ++it) {
      unsigned t;
      if (i > 0 && j > 0) {
        st[i - 1] = j - 1;  // j only falls along a row: the last write is the row's first frame
        const int d = i + j - 2, blk = d >> 5, s = d & 31;
        if (blk != cb || i != cr) {
          w = wsb[(int64_t)blk * L + i - 1];
          cb = blk;
          cr = i;
        }
        t = ((s < 16 ? w.x >> (2 * s) : w.y >> (2 * (s - 16)))) & 3u;
      } else {
        t = i == 0 ? 2u : 1u;
      }
      if (t == 0) {
        --i;
        --j;
      } else if (t == 1) {
        --i;
      } else {
        --j;
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < L; t += AL_MAXL) {
    const int rel = t - skip_first;
    srow[t] = (rel >= 0 && rel < N) ? st[rel] : -1;
  }
}

int al_check_qk(const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk, int64_t kbs, const int32_t* heads,
                const int32_t* lengths, const int32_t* frames, int64_t B, int64_t L, int64_t S, int64_t nh, int64_t H) {
  if (!q || !k || !heads || !lengths || !frames || B < 0 || L <= 0 || S <= 0 || nh <= 0 || H <= 0) return PM_EINVAL;
  if (ldq < H * 64 || ldk < H * 64 || qbs < 0 || kbs < 0) return PM_EINVAL;
  if (B > 65535 || nh > 65535 || L > (1 << 24) || S > (1 << 24) || H > (1 << 16)) return PM_EINVAL;
  if (ldq % 8 || ldk % 8 || qbs % 8 || kbs % 8) return PM_EALIGN;
  if (((uintptr_t)q | (uintptr_t)k) & 15) return PM_EALIGN;
  if (((uintptr_t)heads | (uintptr_t)lengths | (uintptr_t)frames) & 3) return PM_EALIGN;
  return PM_OK;
}

}  // namespace

extern "C" int64_t pm_align_ws_bytes(int64_t B, int64_t L, int64_t S) {
  if (B <= 0 || L <= 0 || S <= 0) return 0;
  return B * L * ((L + S - 1 + DT_T - 1) / DT_T) * 8;
}

extern "C" int pm_align_lse_bf16(const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk,
                                 int64_t k_batch_stride, const int32_t* heads, const int32_t* lengths, const int32_t* frames,
                                 float* lse, int64_t B, int64_t L, int64_t S, int64_t n_sel, int64_t n_heads, void* stream) {
  const int rc = al_check_qk(q, ldq, q_batch_stride, k, ldk, k_batch_stride, heads, lengths, frames, B, L, S, n_sel, n_heads);
  if (rc != PM_OK) return rc;
  if (!lse) return PM_EINVAL;
  if ((uintptr_t)lse & 3) return PM_EALIGN;
  if (B == 0) return PM_OK;
  hipLaunchKernelGGL(align_lse_kernel, dim3((unsigned)((L + 63) / 64), (unsigned)n_sel, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)q, ldq, q_batch_stride, (const bf16*)k, ldk, k_batch_stride, heads, lengths, frames, lse, (int)L,
                     (int)S, (int)n_sel, (int)n_heads);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_align_matrix_bf16(const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk,
                                    int64_t k_batch_stride, const int32_t* heads, const int32_t* lengths, const int32_t* frames,
                                    const float* lse, float* m, int64_t ldm, int64_t m_batch_stride, int64_t B, int64_t L, int64_t S,
                                    int64_t n_sel, int64_t n_heads, float inv_heads, int first, void* stream) {
  const int rc = al_check_qk(q, ldq, q_batch_stride, k, ldk, k_batch_stride, heads, lengths, frames, B, L, S, n_sel, n_heads);
  if (rc != PM_OK) return rc;
  if (!lse || !m || ldm < S || m_batch_stride < 0) return PM_EINVAL;
  if (L > AL_MAXL) return PM_EUNSUPPORTED;
  if (((uintptr_t)lse | (uintptr_t)m) & 3) return PM_EALIGN;
  if (B == 0) return PM_OK;
  hipLaunchKernelGGL(align_matrix_kernel, dim3((unsigned)((S + MT_W - 1) / MT_W), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)q, ldq, q_batch_stride, (const bf16*)k, ldk, k_batch_stride, heads, lengths, frames, lse, m, ldm,
                     m_batch_stride, (int)L, (int)S, (int)n_sel, (int)n_heads, inv_heads, first);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_align_dtw_f32(const float* m, int64_t ldm, int64_t m_batch_stride, const int32_t* lengths, const int32_t* frames,
                                int32_t* start, void* ws, int64_t B, int64_t L, int64_t S, int64_t skip_first, int64_t skip_last,
                                void* stream) {
  if (!m || !lengths || !frames || !start || !ws || B < 0 || L <= 0 || S <= 0 || skip_first < 0 || skip_last < 0) return PM_EINVAL;
  if (ldm < S || m_batch_stride < 0 || S > (1 << 24) || B > (1 << 24) || skip_first > (1 << 24) || skip_last > (1 << 24)) return PM_EINVAL;
  if (L > AL_MAXL) return PM_EUNSUPPORTED;
  if (((uintptr_t)m | (uintptr_t)lengths | (uintptr_t)frames | (uintptr_t)start) & 3) return PM_EALIGN;
  if ((uintptr_t)ws & 7) return PM_EALIGN;
  if (B == 0) return PM_OK;
  const int nblk = (int)((L + S - 1 + DT_T - 1) / DT_T);
  hipLaunchKernelGGL(align_dtw_kernel, dim3((unsigned)B), dim3(AL_MAXL), 0, (hipStream_t)stream, m, ldm, m_batch_stride, lengths, frames,
                     start, (uint2*)ws, (int)L, (int)S, nblk, (int)skip_first, (int)skip_last);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
