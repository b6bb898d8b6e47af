// lm_score.hip - teacher-forced scoring against a vocabulary without the (M, V) logits matrix.
//
// For x[m, v] = sum_k h[m, k] w[v, k] (bf16 operands, fp32 accumulation on the MFMA) the kernel returns per row
//   lse[m] = log sum_v exp(x[m, v]),  logprob[m] = x[m, targets[m]] - lse[m],  argmax[m] = lowest index of max_v x[m, v]
// and never stores a logit: the accumulators of each 128 x 128 tile are folded in registers into per-row running values
// (m, s, best value, best index, target logit).  Memory is O(M): one 20-byte partial per (row, vocabulary chunk).
//
// Shape.  The vocabulary is cut into chunks of LS_NC = 2048 columns (a constant of the build), the grid is
// (row blocks of 128) x (chunks), chunk-major under xcd_remap so that the workgroups of one XCD walk the row blocks of ONE
// weight chunk (2048 x 768 bf16 = 3 MB against the 4 MB L2).  A workgroup is linear_bf16.hip's 128 x 128 x 64 kernel -
// 4 waves as 2 x 2, LDS-DMA staging with the swizzle on the source address, a double buffer, the K tail from the zero page -
// run over the up to 16 tiles of its chunk as ONE stream of K steps: the first K step of the next tile is in flight while
// the finished tile is folded.  The weight tile is the MFMA's A operand, so an accumulator lane holds, for each of its 4 rows
// (tokens m = .. + 16 i + (lane & 15)), 16 columns per tile: 4 j x 4 r at n = .. + 16 j + 4 (lane >> 4) + r.
//
// Fold (per lane, per row, per tile; registers only): tile maximum of the 16 values, running maximum m' = max(m, tmax),
// s = s exp(m - m') + sum exp(x - m'), with exp(d) = exp2(d * log2 e) on v_exp_f32; the arg-max index is searched only
// when the tile maximum beats the lane's best (strictly: columns ascend within a lane, so the lowest index wins a tie);
// the target's logit is picked up by the one lane that owns that column.  Columns at or beyond V are set to -inf BEFORE
// the fold: they enter neither the maximum nor the sum.  A lane's state starts at m = -FLT_MAX (finite: no inf - inf).
// Once per chunk the 4 lanes of a row (lane ^ 16, lane ^ 32: two cross-lane exchanges of registers, no LDS memory) and then
// the 2 waves that share the row (through LDS, one write and one read) merge, and 128 threads write the chunk's partials.
// A second kernel, one thread per row, merges a row's chunks in chunk order with the same rescaling and writes the outputs.
// No atomics; chunk boundaries, lane ownership and merge order depend on V alone, so a row's outputs are bit-identical
// wherever the row sits in the batch and whatever M is.
#include <float.h>

#include "common.h"

namespace {

constexpr int LS_NC = 2048;  // columns per vocabulary chunk
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * BK * 2;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __attribute__((aligned(16))) const unsigned short ls_zero_page[8] = {0, 0, 0, 0, 0, 0, 0, 0};

__device__ __forceinline__ float ls_exp(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }

__device__ __forceinline__ void ls_stage(const bf16* __restrict__ G, const int64_t (&off)[4], const int (&kc)[4], int k0, int K,
                                         char* tile, int wave) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const void* src = (k0 + kc[i] < K) ? (const void*)(G + off[i] + k0) : (const void*)ls_zero_page;
    glds16(src, tile + (wave * 32 + i * 8) * 128);
  }
}

__device__ __forceinline__ bf16x8 ls_frag(const char* tile, int row, int chunk) {
  return *(const bf16x8*)(tile + row * 128 + swz_pos(row, chunk) * 16);
}

// running values of one row over a set of columns
struct RowState {
  float m, s, bv, tg;
  int bi;
};

// a <- a merged with b.  Symmetric up to the order of one commutative add; on equal best values the lower index wins.
__device__ __forceinline__ void ls_merge(RowState& a, const RowState& b) {
  const float mn = fmaxf(a.m, b.m);
  a.s = a.s * ls_exp(a.m - mn) + b.s * ls_exp(b.m - mn);
  a.m = mn;
  if (b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi)) {
    a.bv = b.bv;
    a.bi = b.bi;
  }
  a.tg = fmaxf(a.tg, b.tg);
}

__device__ __forceinline__ RowState ls_xor(const RowState& a, int mask) {
  RowState o;
  o.m = __shfl_xor(a.m, mask, 64);
  o.s = __shfl_xor(a.s, mask, 64);
  o.bv = __shfl_xor(a.bv, mask, 64);
  o.tg = __shfl_xor(a.tg, mask, 64);
  o.bi = __shfl_xor(a.bi, mask, 64);
  return o;
}

// ws: five planes of (chunks x M) 4-byte values: m, s, best value, target logit, best index
__global__ __launch_bounds__(256, 2) void lm_score_kernel(const bf16* __restrict__ H, int64_t ldh, const bf16* __restrict__ W,
                                                          int64_t ldw, const int64_t* __restrict__ targets, float* __restrict__ ws,
                                                          int M, int V, int K, int row_blocks, int nchunks) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk_id = wg / row_blocks, rb = wg - chunk_id * row_blocks;  // chunk-major: neighbours share the weight chunk
  const int m0 = rb * BM, c0 = chunk_id * LS_NC;
  const int cols = V - c0 < LS_NC ? V - c0 : LS_NC;
  const int ntiles = (cols + BN - 1) / BN;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  int64_t hoff[4];
  int kc[4], rt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rt[i] = wave * 32 + i * 8 + (lane >> 3);
    const int chunk = swz_pos(rt[i], lane & 7);
    kc[i] = chunk * 8;
    int gm = m0 + rt[i];
    gm = gm < M ? gm : M - 1;  // rows beyond M: clamped here, never written
    hoff[i] = (int64_t)gm * ldh + chunk * 8;
  }
  // this lane's 4 rows and their targets; a target outside [0, V) matches no column
  int tcol[4];
  RowState st[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    const int64_t t = m < M ? targets[m] : -1;
    tcol[i] = (t >= 0 && t < V) ? (int)t : -1;
    st[i] = RowState{-FLT_MAX, 0.f, -INFINITY, -INFINITY, 0x7fffffff};
  }

  f32x4 acc[4][4];  // [column subtile j][row subtile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + BK - 1) / BK;
  const int P = ntiles * nk;  // K steps of all tiles of the chunk: one stream
  int64_t woff[4];
  // staging side: step pp = (tile pp_t, K step pp_k) goes into buffer pp & 1
  int pp_t = 0, pp_k = 0;
#define LS_STAGE_NEXT(BUF)                                                   \
  {                                                                          \
    if (pp_k == 0) {                                                         \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                        \
        int gn = c0 + pp_t * BN + rt[i];                                     \
        gn = gn < V ? gn : V - 1; /* rows beyond V: clamped, masked below */ \
        woff[i] = (int64_t)gn * ldw + kc[i];                                 \
      }                                                                      \
    }                                                                        \
    char* dst_ = smem + (BUF) * 2 * TILE_BYTES;                              \
    ls_stage(H, hoff, kc, pp_k * BK, K, dst_, wave);                         \
    ls_stage(W, woff, kc, pp_k * BK, K, dst_ + TILE_BYTES, wave);            \
    if (++pp_k == nk) {                                                      \
      pp_k = 0;                                                              \
      ++pp_t;                                                                \
    }                                                                        \
  }

  LS_STAGE_NEXT(0);
  wait_vmcnt0();
  __syncthreads();

  int kt = 0, tile = 0;
  for (int pc = 0; pc < P; ++pc) {
    const char* hcur = smem + (pc & 1) * 2 * TILE_BYTES;
    const char* wcur = hcur + TILE_BYTES;
    if (pc + 1 < P) LS_STAGE_NEXT((pc + 1) & 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = ls_frag(wcur, wn * 64 + j * 16 + fr, s * 4 + fq);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = ls_frag(hcur, wm * 64 + i * 16 + fr, s * 4 + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[j][i], 0, 0, 0);
    }
    if (++kt == nk) {
      // ---- tile finished: fold D[column 16 j + 4 fq + r][row 16 i + fr] into the running values; the next tile's first
      // K step is already in flight
      kt = 0;
      const int nb = c0 + tile * BN + wn * 64 + fq * 4;  // this lane's column of (j = 0, r = 0)
      ++tile;
      if (nb - fq * 4 + 64 > V) {  // the vocabulary ends inside this wave's 64 columns: exclude what lies beyond
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (nb + j * 16 + r >= V) {
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[j][i][r] = -INFINITY;
            }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float tmax = acc[0][i][0];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, acc[j][i][r]);
        if (tmax > st[i].bv) {  // a new best: its lowest column (descending scan, the last hit stays)
          int idx = 0;
#pragma unroll
          for (int j = 3; j >= 0; --j)
#pragma unroll
            for (int r = 3; r >= 0; --r)
              if (acc[j][i][r] == tmax) idx = j * 16 + r;
          st[i].bv = tmax;
          st[i].bi = nb + idx;
        }
        const int d = tcol[i] - nb;
        if ((unsigned)d < 64u && (d & 12) == 0) {  // the target is one of this lane's 16 columns: j = d >> 4, r = d & 3
          float tv = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (d == j * 16 + r) tv = acc[j][i][r];
          st[i].tg = tv;
        }
        const float mn = fmaxf(st[i].m, tmax);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) sum += ls_exp(acc[j][i][r] - mn);
        st[i].s = st[i].s * ls_exp(st[i].m - mn) + sum;
        st[i].m = mn;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    wait_vmcnt0();
    __syncthreads();
  }
#undef LS_STAGE_NEXT

  // ---- once per chunk: the 4 lanes of a row, then the 2 waves of a row (LDS is free: the loop ended on a barrier)
  float* part = (float*)smem;  // [wn][128 rows][5]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    RowState o = ls_xor(st[i], 16);
    ls_merge(st[i], o);
    o = ls_xor(st[i], 32);
    ls_merge(st[i], o);
    if (fq == 0) {
      float* p = part + (wn * BM + wm * 64 + i * 16 + fr) * 5;
      p[0] = st[i].m;
      p[1] = st[i].s;
      p[2] = st[i].bv;
      p[3] = st[i].tg;
      p[4] = __int_as_float(st[i].bi);
    }
  }
  __syncthreads();
  if (tid < BM && m0 + tid < M) {
    const float* p0 = part + tid * 5;
    const float* p1 = part + (BM + tid) * 5;
    RowState a{p0[0], p0[1], p0[2], p0[3], __float_as_int(p0[4])};
    const RowState b{p1[0], p1[1], p1[2], p1[3], __float_as_int(p1[4])};
    ls_merge(a, b);
    const int64_t plane = (int64_t)nchunks * M;
    const int64_t o = (int64_t)chunk_id * M + m0 + tid;
    ws[o] = a.m;
    ws[plane + o] = a.s;
    ws[2 * plane + o] = a.bv;
    ws[3 * plane + o] = a.tg;
    ((int*)ws)[4 * plane + o] = a.bi;
  }
}

// one thread per row: the row's chunks in chunk order
__global__ __launch_bounds__(256) void lm_score_merge_kernel(const float* __restrict__ ws, const int64_t* __restrict__ targets,
                                                            float* __restrict__ logprob, float* __restrict__ lse,
                                                            int32_t* __restrict__ argmax, int M, int V, int nchunks) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int64_t plane = (int64_t)nchunks * M;
  RowState a{-FLT_MAX, 0.f, -INFINITY, -INFINITY, 0x7fffffff};
  for (int c = 0; c < nchunks; ++c) {
    const int64_t o = (int64_t)c * M + m;
    const RowState b{ws[o], ws[plane + o], ws[2 * plane + o], ws[3 * plane + o], ((const int*)ws)[4 * plane + o]};
    ls_merge(a, b);
  }
  const float l = a.m + logf(a.s);
  const int64_t t = targets[m];
  logprob[m] = (t >= 0 && t < V) ? a.tg - l : 0.f;
  if (lse) lse[m] = l;
  if (argmax) argmax[m] = (unsigned)a.bi < (unsigned)V ? a.bi : 0;  // a row without a maximum (NaN): any valid index
}

}  // namespace

extern "C" int64_t pm_lm_score_ws_bytes(int64_t M, int64_t V) {
  if (M <= 0 || V <= 0) return 0;
  return 20 * M * ((V + LS_NC - 1) / LS_NC);
}

extern "C" int pm_lm_score_bf16(const void* h, int64_t ldh, const void* w, int64_t ldw, const int64_t* targets, float* logprob,
                                float* lse, int32_t* argmax, void* ws, int64_t M, int64_t V, int64_t K, void* stream) {
  if (!h || !w || !targets || !logprob || !ws || M < 0 || V <= 0 || K <= 0) return PM_EINVAL;
  if (K % 8 != 0) return PM_EUNSUPPORTED;  // 16-byte chunks; a K tail below 64 is fed from the zero page
  if (ldh < K || ldw < K) return PM_EINVAL;
  if (ldh % 8 || ldw % 8) return PM_EALIGN;
  if (((uintptr_t)h | (uintptr_t)w) & 15) return PM_EALIGN;
  if (((uintptr_t)targets & 7) || (((uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)argmax | (uintptr_t)ws) & 3)) return PM_EALIGN;
  if (M > (1 << 30) || V > (1 << 30) || K > (1 << 30)) return PM_EINVAL;
  if (M == 0) return PM_OK;
  const int64_t row_blocks = (M + BM - 1) / BM, nchunks = (V + LS_NC - 1) / LS_NC;
  if (row_blocks * nchunks > 0x7fffffff) return PM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lm_score_kernel, dim3((unsigned)(row_blocks * nchunks)), dim3(256), 0, st, (const bf16*)h, ldh, (const bf16*)w,
                     ldw, targets, (float*)ws, (int)M, (int)V, (int)K, (int)row_blocks, (int)nchunks);
  PM_CHECK_LAUNCH();
  hipLaunchKernelGGL(lm_score_merge_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const float*)ws, targets, logprob,
                     lse, argmax, (int)M, (int)V, (int)nchunks);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
