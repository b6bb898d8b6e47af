// decode_beam.hip - the three kernels a fixed-shape beam search adds to the tail of the decode step (decode.hip): rows are
// r = b * W + w (clip b, beam w), W <= 8.  New capability: the reference decodes nothing for Whisper (README.md:86) and its
// generic generators follow one hypothesis (text/generator.py:23-35).  Semantics: DESIGN.md, "Beam search".
//   dec_beam_topw    one workgroup per row : log-sum-exp of the row's logits and its W best continuations
//   dec_beam_select  one workgroup per clip: the W best of the clip's W x W candidates, token histories re-gathered,
//                                            then the tail of pm_dec_next_token (next x rows, ticketed position advance)
//   dec_beam_reorder one launch, all layers: self-attention K / V rows re-gathered from their parents, in place
#include "common.h"

namespace {

constexpr int BM_MAXW = 8;
constexpr int TW_THREADS = 1024, TW_WAVES = TW_THREADS / 64, TW_LOADS = 8;  // dec_beam_topw: one 16-wave workgroup per row
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;  // one 16-byte unit of a cache row

// Row r's candidates: cand_score / cand_tok (rows, W).  A live row: its W largest logits in the order (value descending,
// index ascending) as score[r] + (logit - lse).  ONE pass over the row: every thread keeps the W best of the elements it visits
// (a sorted list in registers; an element that does not beat the list's last entry - nearly all of them - costs one compare),
// then W rounds of a block-wide arg-max over the lists' heads, the winner's owner popping its list: the global W best are in
// the union of the threads' W best.  (The rounds of dec_sample_topk_kernel re-read the row once per round: W + 1 = 6 dependent
// passes over 51865 logits were 254 us per step at 40 rows, this form with 256 threads and 4 loads in flight 88 us - both passes
// are load-latency bound, hence 16 waves with 8 loads each in flight; DESIGN.md has the figures.)  Round 0's winner is the row
// maximum the log-sum-exp needs: a second pass sums exp(x - max).
// A finished row: (score[r], eos) and W - 1 padding entries (token -1: never selected).  A row at -inf (beams 1.. of the first
// generated position): every continuation is at -inf, the tie rule orders them by token id -> tokens 0 .. W - 1.
template <int W>
__global__ __launch_bounds__(TW_THREADS) void dec_beam_topw_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                            const float* __restrict__ scores, const int* __restrict__ finished,
                                                            int eos, const int* __restrict__ pos_ptr, int P,
                                                            float* __restrict__ cand_score, int* __restrict__ cand_tok) {
  __shared__ float wv[TW_WAVES];
  __shared__ int wi[TW_WAVES];
  __shared__ float ws[TW_WAVES];
  constexpr int NONE = 0x7fffffff;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (*pos_ptr + 1 < P) return;  // the prompt is still being forced: dec_beam_select keeps every row as it is
  const float s = scores[r];
  float* cs = cand_score + (int64_t)r * W;
  int* ct = cand_tok + (int64_t)r * W;
  if (eos >= 0 && finished[r]) {
    if (tid < W) { cs[tid] = tid == 0 ? s : -INFINITY; ct[tid] = tid == 0 ? eos : -1; }
    return;
  }
  if (s == -INFINITY) {
    if (tid < W) { cs[tid] = -INFINITY; ct[tid] = tid; }
    return;
  }
  const float* row = logits + (int64_t)r * ldl;
  float lv[W];
  int li[W];
#pragma unroll
  for (int k = 0; k < W; ++k) { lv[k] = -INFINITY; li[k] = NONE; }
  // TW_LOADS loads in flight per trip (clamped index, the repeats dropped below), as dec_argmax_reduce_kernel does
  for (int i0 = tid; i0 < V; i0 += TW_LOADS * TW_THREADS) {
    float vl[TW_LOADS];
#pragma unroll
    for (int j = 0; j < TW_LOADS; ++j) vl[j] = row[min(i0 + TW_THREADS * j, V - 1)];
#pragma unroll
    for (int j = 0; j < TW_LOADS; ++j) {
      const int i = i0 + TW_THREADS * j;
      float cv = vl[j];
      int ci = i;
      if (i < V && (cv > lv[W - 1] || (cv == lv[W - 1] && ci < li[W - 1]))) {
#pragma unroll
        for (int k = 0; k < W; ++k) {  // sorted insert: the entry that loses at slot k moves on to slot k + 1
          const bool b = cv > lv[k] || (cv == lv[k] && ci < li[k]);
          const float tv = b ? lv[k] : cv;
          const int ti = b ? li[k] : ci;
          lv[k] = b ? cv : lv[k];
          li[k] = b ? ci : li[k];
          cv = tv;
          ci = ti;
        }
      }
    }
  }
  float lse = 0.f;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
    __syncthreads();
    bv = wv[0];
    bi = wi[0];
#pragma unroll
    for (int w = 1; w < TW_WAVES; ++w)
      if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
    if (bi != NONE && li[0] == bi) {  // the winner's owner pops it
#pragma unroll
      for (int q = 0; q + 1 < W; ++q) { lv[q] = lv[q + 1]; li[q] = li[q + 1]; }
      lv[W - 1] = -INFINITY;
      li[W - 1] = NONE;
    }
    if (k == 0) {  // lse = max + log(sum exp(x - max)): ceil(V / 1024) terms per thread in order, a 6-level tree, 15 adds
      float se = 0.f;
      if (bv > -INFINITY)
        for (int i0 = tid; i0 < V; i0 += TW_LOADS * TW_THREADS) {
          float vl[TW_LOADS];
#pragma unroll
          for (int j = 0; j < TW_LOADS; ++j) vl[j] = row[min(i0 + TW_THREADS * j, V - 1)];
#pragma unroll
          for (int j = 0; j < TW_LOADS; ++j)
            if (i0 + TW_THREADS * j < V) se += expf(vl[j] - bv);
        }
      se = wave_sum(se);
      if (lane == 0) ws[wave] = se;
      __syncthreads();
      float tot = ws[0];
#pragma unroll
      for (int w = 1; w < TW_WAVES; ++w) tot += ws[w];
      lse = bv + logf(tot);
    }
    if (tid == 0) {
      cs[k] = bv > -INFINITY ? s + (bv - lse) : -INFINITY;
      // fewer than W comparable logits (NaN compares with nothing): the lowest id no earlier round of this row took, at -inf -
      // the row's W candidates stay distinct (some id in 0 .. k is free: k earlier rounds, k + 1 <= W <= V ids)
      int tok = bi;
      if (bi == NONE) {
        tok = 0;
        for (int c = k; c >= 0; --c) {
          bool used = false;
          for (int j = 0; j < k; ++j) used = used || ct[j] == c;
          if (!used) tok = c;
        }
      }
      ct[k] = tok;
    }
    __syncthreads();
  }
}

// Clip b's W survivors.  Every candidate's rank = the number of candidates before it in the order (score descending, parent
// ascending, token ascending; padding last) - a strict total order, so ranks 0 .. W - 1 are the survivors, best first.
// Then, with the parents known: scores / finished / parents, the token histories tokens[b, j, 0..t] = tokens[b, parent_j, 0..t]
// in place (each thread owns one position: loads it from all W parents, then stores all W), the new token, and
// pm_dec_next_token's tail.  While t + 1 < P: identity parents, the forced prompt token, scores and flags untouched.
__global__ __launch_bounds__(256) void dec_beam_select_kernel(const float* __restrict__ cand_score, const int* __restrict__ cand_tok,
                                                              int W, float* scores, int* finished, int* __restrict__ parents,
                                                              int eos, int64_t* tokens, int Ttot, const int64_t* __restrict__ prompt,
                                                              int P, int64_t* __restrict__ tok_cur, const bf16* __restrict__ E,
                                                              const float* __restrict__ pos_tab, float* __restrict__ x, int d,
                                                              int V, int* ticket, int* pos_rw) {
  __shared__ float c_s[BM_MAXW * BM_MAXW];
  __shared__ int c_t[BM_MAXW * BM_MAXW];
  __shared__ int old_fin[BM_MAXW];
  __shared__ int s_par[BM_MAXW];
  __shared__ int s_tok[BM_MAXW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int t = *pos_rw, t1 = t + 1;
  const int r0 = b * W;
  const bool forced = t1 < P;
  if (tid < W) {  // identity and the forced token; the ranking below overwrites both for a generated position
    s_par[tid] = tid;
    s_tok[tid] = forced ? (int)prompt[(int64_t)(r0 + tid) * P + t1] : 0;
  }
  if (!forced) {
    const int n = W * W;
    if (tid < n) { c_s[tid] = cand_score[(int64_t)r0 * W + tid]; c_t[tid] = cand_tok[(int64_t)r0 * W + tid]; }
    if (tid < W) old_fin[tid] = finished[r0 + tid];
    __syncthreads();
    if (tid < n) {
      const float ms = c_s[tid];
      const int mt = c_t[tid];
      int rank = 0;
      if (mt < 0) rank = n;  // padding of a finished row
      else
        for (int o = 0; o < n; ++o) {  // o / W = parent, ascending with o: equal scores of another row -> the lower o is first
          const float os = c_s[o];
          const int ot = c_t[o];
          // NaN scores come first and tie with each other (torch.topk's order): the order stays total, so no two candidates
          // share a rank, and a NaN hypothesis stays visible in `scores` instead of racing the best finite one for slot 0
          const bool on = os != os, mn = ms != ms;
          const bool gt = mn ? false : (on || os > ms), eq = mn ? on : os == ms;
          const bool before = ot >= 0 && (gt || (eq && (o / W < tid / W || (o / W == tid / W && ot < mt))));
          rank += before ? 1 : 0;
        }
      if (rank < W) {
        const int par = tid / W;
        s_par[rank] = par;
        s_tok[rank] = mt;
        scores[r0 + rank] = ms;
        finished[r0 + rank] = (old_fin[par] != 0 || (eos >= 0 && mt == eos)) ? 1 : 0;
      }
    }
  }
  __syncthreads();
  bool ident = true;
  for (int j = 0; j < W; ++j) ident = ident && s_par[j] == j;
  if (!ident) {
    for (int i = tid; i <= t && i < Ttot; i += 256) {
      int64_t v[BM_MAXW] = {};
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j)
        if (j < W) v[j] = tokens[(int64_t)(r0 + s_par[j]) * Ttot + i];
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j)
        if (j < W) tokens[(int64_t)(r0 + j) * Ttot + i] = v[j];
    }
  }
  if (tid < W) {
    parents[r0 + tid] = s_par[tid];
    tok_cur[r0 + tid] = s_tok[tid];
    if (t1 < Ttot) tokens[(int64_t)(r0 + tid) * Ttot + t1] = s_tok[tid];
  }
  // the next step's input rows x[r] = E[token] + pos[t + 1]; the last workgroup to get here moves the position
  const int nch = d / 8;
  for (int c = tid; c < W * nch; c += 256) {
    const int j = c / nch, cc = c - j * nch;
    int64_t id = s_tok[j];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    const bf16x8 e = *(const bf16x8*)(E + id * d + cc * 8);
    const f32x4 p0 = *(const f32x4*)(pos_tab + (int64_t)t1 * d + cc * 8), p1 = *(const f32x4*)(pos_tab + (int64_t)t1 * d + cc * 8 + 4);
    f32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o0[i] = (float)e[i] + p0[i]; o1[i] = (float)e[4 + i] + p1[i]; }
    *(f32x4*)(x + (int64_t)(r0 + j) * d + cc * 8) = o0;
    *(f32x4*)(x + (int64_t)(r0 + j) * d + cc * 8 + 4) = o1;
  }
  __syncthreads();
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int n = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == (int)gridDim.x - 1) {
      __hip_atomic_store(pos_rw, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// cache[b, j, h, 0..t, :] = cache[b, parent_j, h, 0..t, :] for every cache of the table (K and V of every layer), in place:
// a thread owns one 16-byte unit of a clip's row image, loads it from all W parent rows, then stores the rows that moved.
// No other thread reads or writes that unit of that clip, so no second buffer is needed although `parents` is no permutation.
// It runs after dec_beam_select moved the position: t = *pos_ptr - 1 is the position this step appended.  Grid: (units of a
// full row / 256, clips, caches); only the units of positions 0..t do anything.
template <int W>
__global__ __launch_bounds__(256) void dec_beam_reorder_kernel(const uint64_t* __restrict__ table, const int* __restrict__ parents,
                                                               const int* __restrict__ pos_ptr, int H, int Tmax,
                                                               int upp) {  // upp: 16-byte units per position (64 elements)
  const int b = blockIdx.y;
  int par[W];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    par[j] = min(max(parents[b * W + j], 0), W - 1);
    ident = ident && par[j] == j;
  }
  if (ident) return;  // a converged beam, and the whole prompt phase
  int t = *pos_ptr - 1;
  if (t < 0) return;
  if (t >= Tmax) t = Tmax - 1;
  const int per_head = (t + 1) * upp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * per_head) return;
  const int h = idx / per_head, u = idx - h * per_head;
  const int64_t row_units = (int64_t)H * Tmax * upp;
  u32x4* base = (u32x4*)table[blockIdx.z] + (int64_t)b * W * row_units + (int64_t)h * Tmax * upp + u;
  u32x4 v[W];
#pragma unroll
  for (int j = 0; j < W; ++j) v[j] = base[(int64_t)par[j] * row_units];
#pragma unroll
  for (int j = 0; j < W; ++j)
    if (par[j] != j) base[(int64_t)j * row_units] = v[j];
}

}  // namespace

extern "C" int pm_dec_beam_topw(const float* logits, int64_t ldl, int64_t V, int64_t W, const float* scores,
                                const int32_t* finished, int64_t eos, const int32_t* pos_ptr, int64_t P, float* cand_score,
                                int32_t* cand_tok, int64_t rows, void* stream) {
  if (!logits || !scores || !finished || !pos_ptr || !cand_score || !cand_tok) return PM_EINVAL;
  if (V <= 0 || ldl < V || W < 1 || W > BM_MAXW || W > V || rows <= 0 || rows % W || P <= 0 || eos >= V) return PM_EINVAL;
#define PM_BM_TOPW(W_)                                                                                                        \
  case W_:                                                                                                                    \
    hipLaunchKernelGGL(dec_beam_topw_kernel<W_>, dim3((unsigned)rows), dim3(TW_THREADS), 0, (hipStream_t)stream, logits, ldl, (int)V, \
                       scores, (const int*)finished, eos < 0 ? -1 : (int)eos, (const int*)pos_ptr, (int)P, cand_score,        \
                       (int*)cand_tok);                                                                                       \
    break;
  switch ((int)W) {
    PM_BM_TOPW(1) PM_BM_TOPW(2) PM_BM_TOPW(3) PM_BM_TOPW(4) PM_BM_TOPW(5) PM_BM_TOPW(6) PM_BM_TOPW(7) PM_BM_TOPW(8)
  }
#undef PM_BM_TOPW
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_dec_beam_select(const float* cand_score, const int32_t* cand_tok, int64_t W, float* scores, int32_t* finished,
                                  int32_t* parents, int64_t eos, int64_t* tokens, int64_t Ttot, int32_t* pos_ptr,
                                  const int64_t* prompt, int64_t P, int64_t* tok_cur, const void* emb, const float* pos, float* x,
                                  int64_t d, int64_t V, int32_t* ticket, int64_t B, void* stream) {
  if (!cand_score || !cand_tok || !scores || !finished || !parents || !tokens || !pos_ptr || !prompt || !tok_cur) return PM_EINVAL;
  if (!emb || !pos || !x || !ticket || W < 1 || W > BM_MAXW || W > V || B <= 0 || P <= 0 || Ttot < P || d <= 0 || V <= 0 || eos >= V)
    return PM_EINVAL;
  if (d % 8) return PM_EUNSUPPORTED;
  if (((uintptr_t)emb | (uintptr_t)pos | (uintptr_t)x) & 15) return PM_EALIGN;
  hipLaunchKernelGGL(dec_beam_select_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, cand_score,
                     (const int*)cand_tok, (int)W, scores, (int*)finished, (int*)parents, eos < 0 ? -1 : (int)eos, tokens, (int)Ttot,
                     prompt, (int)P, tok_cur, (const bf16*)emb, pos, x, (int)d, (int)V, (int*)ticket, (int*)pos_ptr);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_dec_beam_reorder(const void* table, int64_t n_caches, const int32_t* parents, const int32_t* pos_ptr, int64_t B,
                                   int64_t W, int64_t H, int64_t Tmax, int kv_f32, void* stream) {
  if (!table || !parents || !pos_ptr || n_caches <= 0 || n_caches > 65535 || B <= 0 || B > 65535) return PM_EINVAL;
  if (W < 1 || W > BM_MAXW || H <= 0 || Tmax <= 0) return PM_EINVAL;
  const int upp = kv_f32 ? 16 : 8;
  const int64_t units = H * Tmax * upp;
  if (units > (int64_t)1 << 30) return PM_EUNSUPPORTED;
  const dim3 grid((unsigned)((units + 255) / 256), (unsigned)B, (unsigned)n_caches);
#define PM_BM_REORDER(W_)                                                                                                   \
  case W_:                                                                                                                  \
    hipLaunchKernelGGL(dec_beam_reorder_kernel<W_>, grid, dim3(256), 0, (hipStream_t)stream, (const uint64_t*)table,        \
                       (const int*)parents, (const int*)pos_ptr, (int)H, (int)Tmax, upp);                                   \
    break;
  switch ((int)W) {
    PM_BM_REORDER(1) PM_BM_REORDER(2) PM_BM_REORDER(3) PM_BM_REORDER(4) PM_BM_REORDER(5) PM_BM_REORDER(6) PM_BM_REORDER(7)
    PM_BM_REORDER(8)
  }
#undef PM_BM_REORDER
  PM_CHECK_LAUNCH();
  return PM_OK;
}
