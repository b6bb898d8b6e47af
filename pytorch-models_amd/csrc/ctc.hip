// ctc.hip - CTC heads of the wav2vec2 family: vocabulary projection + log-softmax, best-path decoding, the forward (alpha)
// recursion and the Viterbi forced alignment.  Four entry points, no atomics: a clip's outputs are bit-identical wherever the
// clip sits in the batch and whatever the batch size is.  Every id and length is clamped on the device.
//
// ctc_head_kernel   a workgroup owns 64 hidden rows (4 waves x 16) and ALL V <= 256 columns.  K runs in chunks of 256 (V <= 64)
//                   or 64: the workgroup copies the chunk of w into LDS (rows at and beyond V and the K tail as zeros), every lane
//                   loads its own 16-byte pieces of h straight from global memory (h is read exactly once; a chunk's 8 or 2
//                   loads are issued together, the next chunk's under the MFMAs of this one), and the bf16 MFMA
//                   16x16x32 takes w as the A operand and h as the B operand, so that a lane holds, for ITS row (lane & 15),
//                   the columns 16 j + 4 (lane >> 4) + r of every column tile j.  The row reduction is then the lane's own
//                   columns in ascending order and two cross-lane exchanges (lane ^ 16, lane ^ 32): the maximum with its
//                   LOWEST index, S = sum exp(x - max) with exp(d) = v_exp_f32(d * log2 e), lse = max + logf(S),
//                   logp = x - lse.  One kernel, no workspace.  Columns V .. ldl are not written.
// ctc_greedy_kernel one workgroup per clip, 256 frames at a time: a frame emits when its arg-max is not the blank and differs
//                   from the frame before it (inside the clip); the emit flags are scanned with a ballot per wave and the four
//                   wave totals through LDS (one barrier per 256 frames).  path_logp: thread i adds the frames i, i + 256, ..
//                   in ascending order, a wave folds its 64 partials with the xor butterfly (32, 16, .. 1) and thread 0 adds the
//                   four wave sums in wave order.
// ctc_rec_kernel    <VIT = false> the alpha recursion in log space, <VIT = true> the same recursion with max in place of the
//                   merge plus two bits of back-pointer per (frame, state).  One workgroup of 256 threads per clip; thread i
//                   owns the extended states 4 i .. 4 i + 3 = (blank, label 2 i, blank, label 2 i + 1) in registers for the
//                   whole clip, so the only value that crosses threads is state 4 i - 1 of the frame before: one float through
//                   a double-buffered LDS slot, ONE barrier per frame.  The emissions logp[t, label] are gathered 16 frames
//                   ahead: loaded into registers at the start of a block of 16 frames, stored to the other half of a
//                   double-buffered LDS tile (16 frames x (U + 1) columns, the blank last) in front of the block's last
//                   barrier.  No global access depends on the chain.
//                   merge(a, b, c) = m + log(exp(a - m) + exp(b - m) + exp(c - m)), m the maximum, terms in the order
//                   (stay, s - 1, s - 2), exp as above, log(S) = v_log_f32(S) * ln 2; m = -inf gives -inf (no inf - inf).
//                   Viterbi: stay if it is not below the others, else s - 1 if it is not below s - 2, else s - 2; the score
//                   is that maximum plus the emission, one fp32 add.  The 16 codes of a (block, state) are one 32-bit word, a
//                   thread's four words one 16-byte store per block; thread 0 walks them back (T - 1 moves) and the workgroup
//                   writes start / stop.
#include <float.h>

#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

constexpr int CH_ROWS = 64;   // hidden rows per workgroup of the head kernel
constexpr int CH_KC = 64;     // K chunk staged in LDS when V > 64 (256 below; the LDS row stride is the chunk + 8 bf16)
constexpr int CH_MAXV = 256;

constexpr int CT_THREADS = 256;
constexpr int CT_FB = 16;     // frames per block of the recursion kernels (= codes per back-pointer word)
constexpr int CT_UP = 512;    // columns of the emission tile: U <= 511 labels and the blank
constexpr int CT_MAXU = 511;

__device__ __forceinline__ float ct_exp(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }
__device__ __forceinline__ int ct_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bf16x8 ct_ld8(const bf16* p) { return *(const bf16x8*)p; }
__device__ __forceinline__ bf16x8 ct_zero8() { return __builtin_bit_cast(bf16x8, f32x4{0.f, 0.f, 0.f, 0.f}); }

template <int NT>
__global__ __launch_bounds__(256) void ctc_head_kernel(const bf16* __restrict__ H, int64_t ldh, const bf16* __restrict__ W, int64_t ldw,
                                                       const float* __restrict__ bias, float* __restrict__ logp, int64_t ldl,
                                                       int* __restrict__ best, float* __restrict__ best_logp, int M, int V, int K,
                                                       int vec) {
  // K chunk per barrier pair: 256 while all V rows of it stay small in LDS (V <= 64: 33 KiB), else 64
  constexpr int KC = NT <= 4 ? 256 : CH_KC, NF = KC / 32, SEGS = KC / 8, WS = KC + 8;
  __shared__ __attribute__((aligned(16))) bf16 Ws[NT * 16 * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int m = blockIdx.x * CH_ROWS + wave * 16 + fr;
  const bf16* hp = H + (int64_t)(m < M ? m : M - 1) * ldh + fq * 8;  // rows beyond M: clamped here, never written

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's pieces of h for one chunk: NF loads of 16 bytes in flight at once, the next chunk's under the MFMAs of this one
  bf16x8 hf[NF], hn[NF];
#pragma unroll
  for (int s = 0; s < NF; ++s) hf[s] = s * 32 + fq * 8 < K ? ct_ld8(hp + s * 32) : ct_zero8();
  for (int k0 = 0; k0 < K; k0 += KC) {
    for (int idx = tid; idx < NT * 16 * SEGS; idx += 256) {
      const int row = idx / SEGS, seg = idx % SEGS, kk = k0 + seg * 8;
      *(bf16x8*)(Ws + row * WS + seg * 8) = (row < V && kk < K) ? ct_ld8(W + (int64_t)row * ldw + kk) : ct_zero8();
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NF; ++s) hn[s] = k0 + KC + s * 32 + fq * 8 < K ? ct_ld8(hp + k0 + KC + s * 32) : ct_zero8();
#pragma unroll
    for (int s = 0; s < NF; ++s)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bf16x8 wf = *(const bf16x8*)(Ws + (j * 16 + fr) * WS + s * 32 + fq * 8);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, hf[s], acc[j], 0, 0, 0);
      }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NF; ++s) hf[s] = hn[s];
  }

  // ---- the lane's columns 16 j + 4 fq + r of its row, ascending: bias, the maximum and its lowest index
  float mx = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = j * 16 + fq * 4 + r;
      const float x = v < V ? acc[j][r] + (bias ? bias[v] : 0.f) : -INFINITY;
      acc[j][r] = x;
      if (x > mx) {
        mx = x;
        bi = v;
      }
    }
#pragma unroll
  for (int mask = 16; mask <= 32; mask <<= 1) {
    const float mo = __shfl_xor(mx, mask, 64);
    const int io = __shfl_xor(bi, mask, 64);
    if (mo > mx || (mo == mx && io < bi)) {
      mx = mo;
      bi = io;
    }
  }
  if ((unsigned)bi >= (unsigned)V) bi = 0;  // a row without a maximum (NaN): any valid index
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) s += ct_exp(acc[j][r] - mx);
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const float lse = mx + logf(s);
  if (m >= M) return;
  float* out = logp + (int64_t)m * ldl;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int v0 = j * 16 + fq * 4;
    if (vec && v0 + 3 < V) {
      *(f32x4*)(out + v0) = f32x4{acc[j][0] - lse, acc[j][1] - lse, acc[j][2] - lse, acc[j][3] - lse};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (v0 + r < V) out[v0 + r] = acc[j][r] - lse;
    }
  }
  if (fq == 0) {
    best[m] = bi;
    if (best_logp) best_logp[m] = mx - lse;
  }
}

__global__ __launch_bounds__(256) void ctc_greedy_kernel(const int* __restrict__ best, const int* __restrict__ cu,
                                                         const float* __restrict__ blp, int* __restrict__ ids, int* __restrict__ n,
                                                         int* __restrict__ start, float* __restrict__ path, int Tmax, int blank,
                                                         int total) {
  __shared__ int wtot[2][4];
  __shared__ float wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int r0 = ct_clamp(cu[b], 0, total);
  int T = ct_clamp(cu[b + 1] - r0, 0, total - r0);
  T = T < Tmax ? T : Tmax;
  int* idrow = ids + (int64_t)b * Tmax;
  int* strow = start + (int64_t)b * Tmax;
  int base = 0;
  float acc = 0.f;
  for (int c0 = 0, it = 0; c0 < T; c0 += 256, ++it) {
    const int f = c0 + tid;
    int id = blank;
    bool flag = false;
    if (f < T) {
      id = best[r0 + f];
      flag = id != blank && (f == 0 || id != best[r0 + f - 1]);
      if (blp) acc += blp[r0 + f];
    }
    const unsigned long long mask = __ballot(flag);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[it & 1][wave] = __popcll(mask);
    __syncthreads();
    int off = base, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wtot[it & 1][w];
      off += w < wave ? c : 0;
      all += c;
    }
    if (flag) {
      idrow[off + pre] = id;
      strow[off + pre] = f;
    }
    base += all;
  }
  for (int pos = base + tid; pos < Tmax; pos += 256) {
    idrow[pos] = -1;
    strow[pos] = -1;
  }
  if (tid == 0) n[b] = base;
  if (blp) {  // (uniform)
    acc = wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) path[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// one step of one state: (stay, s - 1, s - 2) -> the merged / best predecessor; code = the Viterbi back-pointer
template <bool VIT>
__device__ __forceinline__ float ct_step(float a, float b, float c, unsigned& code) {
  if constexpr (VIT) {
    // NaN ranks above everything (x != x), as in torch.max: a NaN emission reaches the score instead of losing every comparison
    if ((a >= b || a != a) && (a >= c || a != a)) {
      code = 0u;
      return a;
    }
    if (b >= c || b != b) {
      code = 1u;
      return b;
    }
    code = 2u;
    return c;
  } else {
    code = 0u;
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    const float s = (ct_exp(a - m) + ct_exp(b - m)) + ct_exp(c - m);
    return m + __builtin_amdgcn_logf(s) * LN2;
  }
}

template <bool VIT>
__global__ __launch_bounds__(CT_THREADS) void ctc_rec_kernel(const float* __restrict__ logp, int64_t ldl, const int* __restrict__ cu,
                                                             const int* __restrict__ targets, int64_t ldt,
                                                             const int* __restrict__ tlen, float* __restrict__ out,
                                                             int* __restrict__ start, int* __restrict__ stop, uint4* ws, int Umax,
                                                             int V, int blank, int total, int Tmax, int nblk, int nthr) {
  __shared__ float E[2][CT_FB][CT_UP];
  __shared__ int col[CT_UP];
  __shared__ float Nb[2][CT_THREADS];
  __shared__ int sst[VIT ? CT_UP : 1], ssp[VIT ? CT_UP : 1];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int r0 = ct_clamp(cu[b], 0, total);
  int T = ct_clamp(cu[b + 1] - r0, 0, total - r0);
  T = T < Tmax ? T : Tmax;
  const int ucap = Umax < CT_MAXU ? Umax : CT_MAXU;
  const int U = ct_clamp(tlen[b], 0, ucap), S = 2 * U + 1;
  for (int u = tid; u < CT_UP; u += CT_THREADS) {
    col[u] = u < U ? ct_clamp(targets[(int64_t)b * ldt + u], 0, V - 1) : blank;  // column U (and beyond): the blank
    if constexpr (VIT) {
      sst[u] = -1;
      ssp[u] = -1;
    }
  }
  __syncthreads();
  const int l0 = col[2 * tid], l1 = col[2 * tid + 1];
  const bool sk1 = tid > 0 && 2 * tid < U && l0 != col[tid > 0 ? 2 * tid - 1 : 0];
  const bool sk3 = 2 * tid + 1 < U && l1 != l0;
  const bool ok0 = 4 * tid < S, ok1 = 4 * tid + 1 < S, ok2 = 4 * tid + 2 < S, ok3 = 4 * tid + 3 < S;
  const float* lrow = logp + (int64_t)r0 * ldl;

  float stg[2 * CT_FB];
  // emissions of block blk into registers: frame i >> 1, column tid + 256 (i & 1)
#define CT_LOAD(BLK)                                                            \
  {                                                                             \
    _Pragma("unroll") for (int i = 0; i < 2 * CT_FB; ++i) {                     \
      const int t_ = (BLK) * CT_FB + (i >> 1), u_ = tid + CT_THREADS * (i & 1); \
      stg[i] = (t_ < T && u_ <= U) ? lrow[(int64_t)t_ * ldl + col[u_]] : 0.f;   \
    }                                                                           \
  }
#define CT_STORE(BUF)                                                                                           \
  {                                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 2 * CT_FB; ++i) E[BUF][i >> 1][tid + CT_THREADS * (i & 1)] = stg[i]; \
  }

  float a0 = -INFINITY, a1 = -INFINITY, a2 = -INFINITY, a3 = -INFINITY;
  if (T > 0) {  // (uniform)
    CT_LOAD(0)
    CT_STORE(0)
  }
  __syncthreads();
  for (int blk = 0; blk * CT_FB < T; ++blk) {
    const int buf = blk & 1;
    const bool more = (blk + 1) * CT_FB < T;
    if (more) CT_LOAD(blk + 1)
    const int nf = T - blk * CT_FB < CT_FB ? T - blk * CT_FB : CT_FB;
    unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
    for (int f = 0; f < nf; ++f) {
      const int t = blk * CT_FB + f;
      const float e0 = E[buf][f][2 * tid], e1 = E[buf][f][2 * tid + 1], eb = E[buf][f][U];
      if (t == 0) {
        a0 = tid == 0 ? eb : -INFINITY;
        a1 = (tid == 0 && U > 0) ? e0 : -INFINITY;
      } else {
        const float p3 = tid > 0 ? Nb[(t - 1) & 1][tid - 1] : -INFINITY;
        unsigned c0, c1, c2, c3;
        const float n0 = ct_step<VIT>(a0, p3, -INFINITY, c0) + eb;
        const float n1 = ct_step<VIT>(a1, a0, sk1 ? p3 : -INFINITY, c1) + e0;
        const float n2 = ct_step<VIT>(a2, a1, -INFINITY, c2) + eb;
        const float n3 = ct_step<VIT>(a3, a2, sk3 ? a1 : -INFINITY, c3) + e1;
        a0 = ok0 ? n0 : -INFINITY;
        a1 = ok1 ? n1 : -INFINITY;
        a2 = ok2 ? n2 : -INFINITY;
        a3 = ok3 ? n3 : -INFINITY;
        if constexpr (VIT) {
          w0 |= c0 << (2 * f);
          w1 |= c1 << (2 * f);
          w2 |= c2 << (2 * f);
          w3 |= c3 << (2 * f);
        }
      }
      Nb[t & 1][tid] = a3;
      if (f == nf - 1 && more) CT_STORE(buf ^ 1)
      __syncthreads();
    }
    if constexpr (VIT) {
      if (tid < nthr) ws[((int64_t)b * nblk + blk) * nthr + tid] = make_uint4(w0, w1, w2, w3);
    }
  }
#undef CT_LOAD
#undef CT_STORE

  float* fin = &E[0][0][0];  // the last barrier of the loop is behind every read of E
  fin[4 * tid] = a0;
  fin[4 * tid + 1] = a1;
  fin[4 * tid + 2] = a2;
  fin[4 * tid + 3] = a3;
  __syncthreads();  // (and the trace words of every wave are visible to thread 0)
  if constexpr (!VIT) {
    if (tid == 0) {
      unsigned c;
      out[b] = T > 0 ? ct_step<false>(fin[2 * U], U > 0 ? fin[2 * U - 1] : -INFINITY, -INFINITY, c) : -INFINITY;
    }
  } else {
    if (tid == 0) {
      int s = 2 * U;
      if (U > 0 && fin[2 * U - 1] > fin[2 * U]) s = 2 * U - 1;
      const float score = T > 0 ? fin[s] : -INFINITY;
      const bool feasible = score > -INFINITY;
      out[b] = feasible ? score : -INFINITY;
      if (feasible) {
        int cb = -1, co = -1;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        for (int t = T - 1; t >= 0; --t) {
          if (s & 1) {
            const int u = (s - 1) >> 1;  // < U
            if (ssp[u] < 0) ssp[u] = t + 1;
            sst[u] = t;  // t only falls: the last write is the token's first frame
          }
          if (t == 0) break;
          const int owner = s >> 2, k = s & 3, tb = t >> 4;
          if (tb != cb || owner != co) {
            w = ws[((int64_t)b * nblk + tb) * nthr + owner];
            cb = tb;
            co = owner;
          }
          const unsigned word = k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w));
          s -= (int)((word >> (2 * (t & 15))) & 3u);
          s = s < 0 ? 0 : s;
        }
      }
    }
    __syncthreads();
    for (int u = tid; u < Umax; u += CT_THREADS) {
      const bool live = u < U;
      start[(int64_t)b * Umax + u] = live ? sst[u] : -1;
      stop[(int64_t)b * Umax + u] = live ? ssp[u] : -1;
    }
  }
}

int ct_check_rec(const float* logp, int64_t ldl, const int32_t* cu, const int32_t* targets, int64_t ldt, const int32_t* tlen,
                 const float* out, int64_t total, int64_t B, int64_t Umax, int64_t V, int64_t blank) {
  if (!logp || !cu || !tlen || !out || total < 0 || B < 0 || Umax < 0 || V < 1 || blank < 0 || blank >= V) return PM_EINVAL;
  if ((Umax > 0 && !targets) || ldl < V || ldt < Umax) return PM_EINVAL;
  if (Umax > CT_MAXU) return PM_EUNSUPPORTED;
  if (total > 0x7fffffff || B > 0x7fffffff || V > 0x7fffffff) return PM_EINVAL;
  if (((uintptr_t)logp | (uintptr_t)cu | (uintptr_t)targets | (uintptr_t)tlen | (uintptr_t)out) & 3) return PM_EALIGN;
  return PM_OK;
}

}  // namespace

extern "C" int pm_ctc_head_bf16(const void* h, int64_t ldh, const void* w, int64_t ldw, const float* bias, float* logp, int64_t ldl,
                                int32_t* best, float* best_logp, int64_t M, int64_t V, int64_t K, void* stream) {
  if (!h || !w || !logp || !best || M < 0 || K <= 0) return PM_EINVAL;
  if (V < 2 || V > CH_MAXV || K % 8 != 0) return PM_EUNSUPPORTED;
  if (ldh < K || ldw < K || ldl < V) return PM_EINVAL;
  if (ldh % 8 || ldw % 8) return PM_EALIGN;
  if (((uintptr_t)h | (uintptr_t)w) & 15) return PM_EALIGN;
  if (((uintptr_t)bias | (uintptr_t)logp | (uintptr_t)best | (uintptr_t)best_logp) & 3) return PM_EALIGN;
  if (M > (1 << 30) || K > (1 << 30)) return PM_EINVAL;
  if (M == 0) return PM_OK;
  const int vec = (ldl % 4 == 0 && ((uintptr_t)logp & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((M + CH_ROWS - 1) / CH_ROWS));
  hipStream_t st = (hipStream_t)stream;
#define CT_HEAD(NT)                                                                                                               \
  hipLaunchKernelGGL(ctc_head_kernel<NT>, grid, dim3(256), 0, st, (const bf16*)h, ldh, (const bf16*)w, ldw, bias, logp, ldl, best, \
                     best_logp, (int)M, (int)V, (int)K, vec)
  if (V <= 16) CT_HEAD(1);
  else if (V <= 32) CT_HEAD(2);
  else if (V <= 64) CT_HEAD(4);
  else if (V <= 128) CT_HEAD(8);
  else CT_HEAD(16);
#undef CT_HEAD
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_ctc_greedy(const int32_t* best, const int32_t* cu_frames, const float* best_logp, int32_t* ids, int32_t* n,
                             int32_t* start, float* path_logp, int64_t total_frames, int64_t B, int64_t Tmax, int64_t blank,
                             void* stream) {
  if (!cu_frames || !ids || !n || !start || total_frames < 0 || B < 0 || Tmax < 0 || (total_frames > 0 && !best)) return PM_EINVAL;
  if ((best_logp == nullptr) != (path_logp == nullptr)) return PM_EINVAL;
  if (total_frames > 0x7fffffff || B > 0x7fffffff || Tmax > 0x7fffffff || blank < -0x7fffffff || blank > 0x7fffffff) return PM_EINVAL;
  if (((uintptr_t)best | (uintptr_t)cu_frames | (uintptr_t)best_logp | (uintptr_t)ids | (uintptr_t)n | (uintptr_t)start |
       (uintptr_t)path_logp) & 3)
    return PM_EALIGN;
  if (B == 0) return PM_OK;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, best, cu_frames, best_logp, ids, n, start,
                     path_logp, (int)Tmax, (int)blank, (int)total_frames);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_ctc_forward_f32(const float* logp, int64_t ldl, const int32_t* cu_frames, const int32_t* targets, int64_t ldt,
                                  const int32_t* target_lengths, float* loglik, int64_t total_frames, int64_t B, int64_t Umax,
                                  int64_t V, int64_t blank, void* stream) {
  const int rc = ct_check_rec(logp, ldl, cu_frames, targets, ldt, target_lengths, loglik, total_frames, B, Umax, V, blank);
  if (rc != PM_OK) return rc;
  if (B == 0) return PM_OK;
  hipLaunchKernelGGL(ctc_rec_kernel<false>, dim3((unsigned)B), dim3(CT_THREADS), 0, (hipStream_t)stream, logp, ldl, cu_frames, targets,
                     ldt, target_lengths, loglik, (int*)nullptr, (int*)nullptr, (uint4*)nullptr, (int)Umax, (int)V, (int)blank,
                     (int)total_frames, (int)total_frames, 0, 0);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int64_t pm_ctc_ws_bytes(int64_t B, int64_t Tmax, int64_t Umax) {
  if (B <= 0 || Tmax <= 0 || Umax < 0) return 0;
  return B * ((Tmax + CT_FB - 1) / CT_FB) * ((2 * Umax + 1 + 3) / 4) * 16;
}

extern "C" int pm_ctc_viterbi_f32(const float* logp, int64_t ldl, const int32_t* cu_frames, const int32_t* targets, int64_t ldt,
                                  const int32_t* target_lengths, int32_t* start, int32_t* stop, float* score, void* ws,
                                  int64_t total_frames, int64_t B, int64_t Tmax, int64_t Umax, int64_t V, int64_t blank,
                                  void* stream) {
  const int rc = ct_check_rec(logp, ldl, cu_frames, targets, ldt, target_lengths, score, total_frames, B, Umax, V, blank);
  if (rc != PM_OK) return rc;
  if (Tmax < 0 || Tmax > 0x7fffffff || (Umax > 0 && (!start || !stop)) || (Tmax > 0 && B > 0 && !ws)) return PM_EINVAL;
  if (((uintptr_t)start | (uintptr_t)stop) & 3) return PM_EALIGN;
  if ((uintptr_t)ws & 15) return PM_EALIGN;
  if (B == 0) return PM_OK;
  hipLaunchKernelGGL(ctc_rec_kernel<true>, dim3((unsigned)B), dim3(CT_THREADS), 0, (hipStream_t)stream, logp, ldl, cu_frames, targets,
                     ldt, target_lengths, score, start, stop, (uint4*)ws, (int)Umax, (int)V, (int)blank, (int)total_frames, (int)Tmax,
                     (int)((Tmax + CT_FB - 1) / CT_FB), (int)((2 * Umax + 1 + 3) / 4));
  PM_CHECK_LAUNCH();
  return PM_OK;
}
