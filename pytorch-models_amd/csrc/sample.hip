// The sampling tail of a decode step (pm_dec_sample / pm_dec_sample_ragged): temperature, top-k or the whole vocabulary,
// nucleus (top-p) cut, the emitted token's log-probability - then the tail of pm_dec_next_token (prompt forcing, the next
// step's embedding row, ticketed position advance), restated here so that csrc/decode.hip does not move.
//
// Per row b at cache position t, l[0..V) = the fp32 logits after the rules (finite or -inf), m = max l:
//   logprob  = l[tok] - (m + log sum_i exp(l_i - m))                 (always at temperature 1)
//   T == 0   : tok = lowest index with l == m
//   weights  : w_i = exp((l_i - m) / T), -inf -> 0
//   survivors: the k first tokens in the order (logit descending, index ascending), or (k = 0) all tokens
//   nucleus  : top_p < 1: tau = the largest logit VALUE among the survivors for which mass(survivors with l >= tau) >= top_p * W
//              (W = the survivors' mass); the nucleus is every survivor with l >= tau - ties at the boundary are all kept
//   draw     : u from the counter-based generator of pm_dec_sample_topk keyed by (seed, t, b); the first nucleus element whose
//              running mass exceeds u * M (M = the nucleus mass); running order = the sorted order (k >= 1) or ascending index
//              (k = 0); if rounding leaves u * M above every running sum: the last nucleus element of positive weight
//
// One workgroup of 16 waves per row (at most 64 rows step at once: the launch is latency-bound, and a row of 50k logits is
// ~50 elements per thread).  Wave w owns the contiguous segment [w * S, (w + 1) * S) of the row, S = ceil(V / 16), and reads
// it 64 consecutive elements at a time.  EVERY reduction has one fixed order: per lane in index order, then a shfl_down
// tree whose lane 0 holds the result, then the 16 waves in order - no floating-point atomics.  So (a) token and log-prob are
// bit-identical run to run, graph replay or eager launches, and (b) a sum over {l >= c} is monotone in c (adding non-negative
// terms in a fixed order is monotone under rounding), which makes the bisection for tau well defined.
//
// k = 0 does not fit a row in LDS (Whisper: 51865 floats), so its passes re-read the row from cache: one for (m, sum, arg-max)
// together, one for W, then the search for tau on the order-preserving integer image of a float, 16 candidates per pass (4
// bits of the 32 per pass = 8 passes), one pass for the 16 waves' nucleus masses, and the walk of the one wave that holds the
// pick (a 64-wide scan per 64 elements).
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int SP_WAVES = 16;
constexpr int SP_THREADS = 64 * SP_WAVES;
constexpr int SP_MAXK = 64;
constexpr int SP_CAND = 16;

__device__ __forceinline__ float sp_uniform(uint64_t seed, int t, int b) {  // pm_dec_sample_topk's: splitmix64 finaliser -> [0, 1)
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1) + 0xBF58476D1CE4E5B9ull * (uint64_t)(b + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ int sp_ragged_pos(int t, const int* __restrict__ key_start, int b) {
  const int l = t - key_start[b];
  return l < 0 ? 0 : (l < t ? l : t);  // a negative start cannot index past the cache position
}

// the order-preserving image of a float in the unsigned integers, and back (-inf -> 0x007FFFFF, +FLT_MAX -> 0xFF7FFFFF)
__device__ __forceinline__ uint32_t sp_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// w = exp((l - m) / T): l - m and the quotient may overflow to -inf (weight 0); 0 / T = 0 for every T > 0, so the maximum has weight 1
__device__ __forceinline__ float sp_weight(float l, float m, float T) { return l == -INFINITY ? 0.f : expf((l - m) / T); }

struct SpShared {
  float f[SP_WAVES][SP_CAND];
  int i[SP_WAVES];
  float topv[SP_MAXK];
  float cum[SP_MAXK];
  int topi[SP_MAXK];
  int64_t next;
};

// sums over the row of w_i * [l_i >= c_j] for NC candidates: per lane in index order, shfl_down tree, lane 0 of every wave to sh.f;
// the caller adds the waves in order after the barrier at the end
template <int NC>
__device__ __forceinline__ void sp_mass_pass(const float* __restrict__ row, int lo, int hi, float m, float T, const float (&c)[NC],
                                             SpShared& sh, int lane, int wave) {
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
#pragma unroll 2
  for (int i = lo + lane; i < hi; i += 64) {
    const float l = row[i];
    const float w = sp_weight(l, m, T);
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] += l >= c[j] ? w : 0.f;
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_down(acc[j], o, 64);
  }
  __syncthreads();  // the previous pass's sums have been read by everyone
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NC; ++j) sh.f[wave][j] = acc[j];
  }
  __syncthreads();
}

__global__ __launch_bounds__(SP_THREADS) void dec_sample_kernel(const float* __restrict__ logits, int64_t ldl, int V, int k, float T,
                                                                float top_p, uint64_t seed, const int64_t* __restrict__ prompt,
                                                                int P, int64_t* __restrict__ tok_cur,
                                                                int64_t* __restrict__ tokens_out, int Ttot,
                                                                float* __restrict__ logprobs, const bf16* __restrict__ E,
                                                                const float* __restrict__ pos_tab, float* __restrict__ x, int d,
                                                                int* ticket, int* pos_rw, const int* __restrict__ key_start) {
  __shared__ SpShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (int64_t)b * ldl;
  const int t = *pos_rw;  // the token just consumed sits at position t; this step decides position t + 1
  const int t1 = t + 1;
  const int seg = (V + SP_WAVES - 1) / SP_WAVES;
  const int lo = min(wave * seg, V), hi = min(lo + seg, V);

  // ---- pass 1: running maximum, running sum of exp(l - max) and the arg-max (lowest index on ties) TOGETHER, four elements per
  // rescale.  -inf entries add nothing; a lane that has seen only -inf keeps (max -inf, sum 0).
  float mt = -INFINITY, st = 0.f;
  int bi = 0x7fffffff;
  bool bad = false;  // a NaN logit: no comparison below sees it, so the sum is made to carry it
  for (int i0 = lo + lane; i0 < hi; i0 += 4 * 64) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + 64 * j < hi ? row[i0 + 64 * j] : -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= v[j] != v[j];
    float mn = mt;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + 64 * j;
      if (i < hi && (v[j] > mn || (v[j] == mn && i < bi))) { mn = v[j]; bi = i; }
    }
    if (mn > -INFINITY) {
      float s = st * expf(mt - mn);  // mt == -inf: st is 0 and exp(-inf) is 0
#pragma unroll
      for (int j = 0; j < 4; ++j) s += expf(v[j] - mn);  // -inf - finite = -inf -> 0
      st = s;
      mt = mn;
    }
  }
  // NaN * exp(.) stays NaN through every merge that forms a sum: lse, and with it the log-prob, is NaN.  A merge of two parts at
  // -inf forms none, so a row of NaN and -inf only ends with m = -inf and reports the log-prob -inf, as a row of -inf does.
  if (bad) st = __builtin_nanf("");
  auto merge = [&](float om, float os, int oi) {  // (max, sum, index) of two disjoint parts; the part with the lower indices is `this`
    const float mn = fmaxf(mt, om);
    if (om > mt || (om == mt && oi < bi)) bi = oi;
    if (mn > -INFINITY) st = st * expf(mt - mn) + os * expf(om - mn);
    mt = mn;
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_down(mt, o, 64), os = __shfl_down(st, o, 64);
    const int oi = __shfl_down(bi, o, 64);
    merge(om, os, oi);
  }
  if (lane == 0) { sh.f[wave][0] = mt; sh.f[wave][1] = st; sh.i[wave] = bi; }
  __syncthreads();
  mt = sh.f[0][0];
  st = sh.f[0][1];
  bi = sh.i[0];
#pragma unroll
  for (int w = 1; w < SP_WAVES; ++w) merge(sh.f[w][0], sh.f[w][1], sh.i[w]);
  const float m = mt;
  const float lse = m + logf(st);  // m == -inf (a row of -inf only): -inf, and the log-prob below is reported as -inf
  const int amax = bi == 0x7fffffff ? 0 : bi;  // a row of NaN has no maximum: a valid id.  Every thread holds (m, lse, amax), from
                                               // the same operations in the same order

  int pick = amax;
  if (T > 0.f && k >= 1) {
    // ---- the k first tokens in (logit descending, index ascending): round 0 is the arg-max above, each further round takes the best
    // element AFTER the previous winner in that order (dec_sample_topk_kernel's selection: nothing is masked or sorted)
    const int kk = min(k, V);
    float pv = m;
    int pi = amax;
    if (tid == 0) { sh.topv[0] = m; sh.topi[0] = amax; }
    for (int r = 1; r < kk; ++r) {
      float bv = -INFINITY;
      int bx = 0x7fffffff;
#pragma unroll 4
      for (int i = lo + lane; i < hi; i += 64) {
        const float v = row[i];
        const bool after = v < pv || (v == pv && i > pi);
        if (after && (v > bv || (v == bv && i < bx))) { bv = v; bx = i; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_down(bv, o, 64);
        const int oi = __shfl_down(bx, o, 64);
        if (ov > bv || (ov == bv && oi < bx)) { bv = ov; bx = oi; }
      }
      __syncthreads();
      if (lane == 0) { sh.f[wave][0] = bv; sh.i[wave] = bx; }
      __syncthreads();
      bv = sh.f[0][0];
      bx = sh.i[0];
#pragma unroll
      for (int w = 1; w < SP_WAVES; ++w)
        if (sh.f[w][0] > bv || (sh.f[w][0] == bv && sh.i[w] < bx)) { bv = sh.f[w][0]; bx = sh.i[w]; }
      if (tid == 0) { sh.topv[r] = bv; sh.topi[r] = bx; }
      pv = bv;
      pi = bx;
    }
    __syncthreads();
    if (tid == 0) {
      // running masses in the sorted order (at T = 1 these are pm_dec_sample_topk's sums, term for term)
      float sum = 0.f;
      for (int r = 0; r < kk; ++r) { sum += sp_weight(sh.topv[r], m, T); sh.cum[r] = sum; }
      int nend = kk - 1;  // the nucleus is sorted positions 0 .. nend
      if (top_p < 1.f) {
        const float need = top_p * sum;
        for (int r = 0; r < kk;) {
          int e = r;  // the last position of the tie group that starts at r
          while (e + 1 < kk && sh.topv[e + 1] == sh.topv[r]) ++e;
          if (sh.cum[e] >= need) { nend = e; break; }
          r = e + 1;
        }
      }
      const float u = sp_uniform(seed, t, b) * sh.cum[nend];
      int pk = -1, lastpos = 0;
      for (int r = 0; r <= nend; ++r) {
        if (pk < 0 && u < sh.cum[r]) pk = r;
        if (sh.cum[r] > (r ? sh.cum[r - 1] : 0.f)) lastpos = r;
      }
      sh.i[0] = sh.topi[pk < 0 ? lastpos : pk];
    }
    __syncthreads();
    pick = sh.i[0];
  } else if (T > 0.f) {
    // ---- the whole vocabulary.  tau = -inf keeps everything (top_p == 1)
    float tau = -INFINITY;
    if (top_p < 1.f) {
      const float all[1] = {-INFINITY};
      sp_mass_pass<1>(row, lo, hi, m, T, all, sh, lane, wave);
      float W = 0.f;
#pragma unroll
      for (int w = 0; w < SP_WAVES; ++w) W += sh.f[w][0];
      const float need = top_p * W;
      // the largest key c in [klo, khi] with mass(l >= unkey(c)) >= need: true at klo (the mass is W), monotone in c.  Were c not
      // the image of a logit of the row, c + 1 would select the same set: so tau is a logit value, and its weight is positive.
      uint32_t klo = sp_key(-INFINITY), khi = sp_key(m);
      while (klo < khi) {
        const uint64_t span = (uint64_t)khi - klo;
        // candidate j = klo + ceil(span (j + 1) / 16): non-decreasing, the first above klo, the last = khi; the same in every lane
        auto cand = [&](int j) { return klo + (uint32_t)((span * (uint64_t)(j + 1) + SP_CAND - 1) / SP_CAND); };
        float c[SP_CAND];
#pragma unroll
        for (int j = 0; j < SP_CAND; ++j) c[j] = sp_unkey(__builtin_amdgcn_readfirstlane(cand(j)));
        sp_mass_pass<SP_CAND>(row, lo, hi, m, T, c, sh, lane, wave);
        float s = 0.f;  // lane j < 16 of every wave adds candidate j's wave sums, in wave order
#pragma unroll
        for (int w = 0; w < SP_WAVES; ++w) s += sh.f[w][lane & (SP_CAND - 1)];
        const uint64_t ok = __ballot(lane < SP_CAND && s >= need);  // monotone: true for a prefix of the candidates
        const int best = ok ? 63 - __builtin_clzll(ok) : -1;
        uint32_t nlo = klo, nhi = khi;
        if (best < 0) nhi = cand(0) - 1;
        else {
          nlo = cand(best);
          if (best + 1 < SP_CAND) nhi = cand(best + 1) - 1;  // candidate best + 1 fails, so it lies above candidate best
          if (nhi < nlo) nhi = nlo;
        }
        klo = __builtin_amdgcn_readfirstlane(nlo);
        khi = __builtin_amdgcn_readfirstlane(nhi);
      }
      tau = sp_unkey(klo);
    }
    // ---- the nucleus mass of every wave's segment, M = their sum in wave order, and the wave that holds the pick
    const float cut[1] = {tau};
    sp_mass_pass<1>(row, lo, hi, m, T, cut, sh, lane, wave);
    float M = 0.f;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) M += sh.f[w][0];
    const float target = sp_uniform(seed, t, b) * M;
    int wt = -1, wlast = 0;
    float base = 0.f, run = 0.f;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) {
      const float nxt = run + sh.f[w][0];
      if (wt < 0 && target < nxt) { wt = w; base = run; }
      if (sh.f[w][0] > 0.f) wlast = w;
      run = nxt;
    }
    const bool beyond = wt < 0;  // rounding left the target at or above M: the last nucleus element of positive weight
    if (beyond) wt = wlast;
    if (wave == wt) {
      float running = base;
      int found = -1, lastpos = -1;
      for (int i0 = lo; i0 < hi && found < 0; i0 += 64) {
        const int i = i0 + lane;
        const float l = i < hi ? row[i] : -INFINITY;
        const float w = l >= tau ? sp_weight(l, m, T) : 0.f;
        float s = w;  // inclusive scan over the lanes, in a fixed order
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float up = __shfl_up(s, o, 64);
          if (lane >= o) s += up;
        }
        const float c = running + s;
        const uint64_t hit = __ballot(!beyond && w > 0.f && target < c);
        if (hit) found = i0 + __builtin_ctzll(hit);
        const uint64_t posw = __ballot(w > 0.f);
        if (posw) lastpos = i0 + 63 - __builtin_clzll(posw);
        running = __shfl(c, 63, 64);
      }
      if (lane == 0) sh.i[0] = found >= 0 ? found : (lastpos >= 0 ? lastpos : amax);
    }
    __syncthreads();
    pick = sh.i[0];
  }

  // ---- the tail of pm_dec_next_token: prompt forcing, tok_cur / tokens_out, the next step's row, the ticketed advance
  if (tid == 0) {
    const int64_t next = t1 < P ? prompt[(int64_t)b * P + t1] : (int64_t)pick;
    tok_cur[b] = next;
    if (t1 < Ttot) {
      tokens_out[(int64_t)b * Ttot + t1] = next;
      if (logprobs) {
        const int64_t id = next < 0 ? 0 : (next >= V ? V - 1 : next);
        logprobs[(int64_t)b * Ttot + t1] = m == -INFINITY ? -INFINITY : row[id] - lse;
      }
    }
    sh.next = next;
  }
  __syncthreads();
  const int tp = key_start ? sp_ragged_pos(t1, key_start, b) : t1;
  int64_t id = sh.next;
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  for (int c = tid; c < d / 8; c += SP_THREADS) {
    const bf16x8 e = *(const bf16x8*)(E + id * d + c * 8);
    const f32x4 p0 = *(const f32x4*)(pos_tab + (int64_t)tp * d + c * 8), p1 = *(const f32x4*)(pos_tab + (int64_t)tp * d + c * 8 + 4);
    f32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o0[i] = (float)e[i] + p0[i]; o1[i] = (float)e[4 + i] + p1[i]; }
    *(f32x4*)(x + (int64_t)b * d + c * 8) = o0;
    *(f32x4*)(x + (int64_t)b * d + c * 8 + 4) = o1;
  }
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int n = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == (int)gridDim.x - 1) {  // every workgroup read the position before it took its ticket
      __hip_atomic_store(pos_rw, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

int dec_sample_impl(const float* logits, int64_t ldl, int64_t V, int64_t topk, float temperature, float top_p, uint64_t seed,
                    int32_t* pos_ptr, const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot,
                    float* logprobs, const void* emb, const float* pos, const int32_t* key_start, float* x, int64_t d, int32_t* ticket,
                    int64_t B, void* stream) {
  if (!logits || !pos_ptr || !prompt || !tok_cur || !tokens_out || !emb || !pos || !x || !ticket) return PM_EINVAL;
  if (V <= 0 || V > (1 << 30) || ldl < V || topk < 0 || topk > SP_MAXK || P <= 0 || B <= 0 || Ttot < P || d <= 0 || d % 8) return PM_EINVAL;
  if (!(temperature >= 0.f) || !(temperature <= FLT_MAX)) return PM_EINVAL;  // NaN fails both comparisons
  if (!(top_p > 0.f) || !(top_p <= 1.f)) return PM_EINVAL;
  if (((uintptr_t)emb | (uintptr_t)pos | (uintptr_t)x) & 15) return PM_EALIGN;
  if (((uintptr_t)logits | (uintptr_t)logprobs) & 3) return PM_EALIGN;
  hipLaunchKernelGGL(dec_sample_kernel, dim3((unsigned)B), dim3(SP_THREADS), 0, (hipStream_t)stream, logits, ldl, (int)V, (int)topk,
                     temperature, top_p, seed, prompt, (int)P, tok_cur, tokens_out, (int)Ttot, logprobs, (const bf16*)emb, pos, x,
                     (int)d, (int*)ticket, (int*)pos_ptr, (const int*)key_start);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

}  // namespace

extern "C" int pm_dec_sample(const float* logits, int64_t ldl, int64_t V, int64_t topk, float temperature, float top_p,
                             uint64_t seed, int32_t* pos_ptr, const int64_t* prompt, int64_t P, int64_t* tok_cur,
                             int64_t* tokens_out, int64_t Ttot, float* logprobs, const void* emb, const float* pos, float* x,
                             int64_t d, int32_t* ticket, int64_t B, void* stream) {
  return dec_sample_impl(logits, ldl, V, topk, temperature, top_p, seed, pos_ptr, prompt, P, tok_cur, tokens_out, Ttot, logprobs, emb,
                         pos, nullptr, x, d, ticket, B, stream);
}

extern "C" int pm_dec_sample_ragged(const float* logits, int64_t ldl, int64_t V, int64_t topk, float temperature, float top_p,
                                    uint64_t seed, int32_t* pos_ptr, const int64_t* prompt, int64_t P, int64_t* tok_cur,
                                    int64_t* tokens_out, int64_t Ttot, float* logprobs, const void* emb, const float* pos,
                                    const int32_t* key_start, float* x, int64_t d, int32_t* ticket, int64_t B, void* stream) {
  if (!key_start) return PM_EINVAL;
  return dec_sample_impl(logits, ldl, V, topk, temperature, top_p, seed, pos_ptr, prompt, P, tok_cur, tokens_out, Ttot, logprobs, emb,
                         pos, key_start, x, d, ticket, B, stream);
}
