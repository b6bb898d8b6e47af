// Repetition controls and eos bookkeeping of a decode step: two latency-bound launches that sit in the
// captured step next to pm_dec_whisper_rules, so that csrc/decode.hip, csrc/sample.hip and csrc/decode_beam.hip do not move.
//
// pm_dec_controls   between the vocabulary projection and the rules / the token tail.  Row b at cache position t (= *pos_ptr; the
//   token being chosen sits at t + 1; nothing happens while t + 1 < P): its history h = tokens[b, s .. t], s = key_start[b] of a
//   ragged batch (the padding in front of it is not history) or 0, m = t - s + 1 ids, prompt included.
//     penalty (r != 1)   for every DISTINCT id v of h, once: l[v] = l[v] > 0 ? l[v] / r : l[v] * r
//     no-repeat (n >= 1) for every 0 <= i <= m - n with h[i .. i + n - 2] == h[m - n + 1 .. m - 1]: l[h[i + n - 1]] = -inf
//                        (n = 1: every id of h; m < n - 1: nothing)
//     minimum length     while t + 1 - P < min_new_tokens: l[eos] = -inf
//   One workgroup of 256 threads per row (at most 64 rows step at once: the launch is latency-bound, as csrc/sample.hip argues).
//   "Once" is decided by a V-bit set in LDS: a thread ORs its id's bit in with an LDS atomic and the one that finds it clear owns
//   the id - linear in m, no first-occurrence scan.  Which thread owns an id depends on scheduling; what it computes does not: the
//   owner reads the ORIGINAL logit (no other thread writes that column in this phase) and stores one correctly rounded fp32
//   quotient or product, so the row is bit-equal to torch's l / r and l * r on the CPU (-inf stays -inf, NaN stays NaN, a zero keeps
//   its sign).  A barrier, then the bans: idempotent -inf stores, so any order gives the same row and -inf wins over a penalty.
//   Ids outside [0, V) are skipped, so nothing is touched at columns >= V of a row (ldl > V) or in another row.
//
// pm_dec_finish     BEHIND the token tail, whichever it is: it reads the position the tail has advanced to (t1) and does nothing
//   while t1 < P (a prompt-forced token never finishes a row).  A row whose finished[b] != 0 gets tokens[b, t1] = pad, tok_cur[b]
//   = pad and logprobs[b, t1] = 0; otherwise a row whose tokens[b, t1] == eos records finished[b] = t1 (its eos and the eos's
//   log-prob stay).  One thread per row, plain vector stores, no atomics.  A finished row keeps stepping on whatever its tail
//   picked - rows never read each other - and nobody reads what it computes.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int DC_THREADS = 256;
constexpr int DC_MAX_NGRAM = 8;
constexpr int DC_MAX_V = 1 << 18;  // the seen-set is V bits of LDS: 32 KB at the cap (Whisper's 51866 ids: 6.5 KB)
constexpr int DC_WORDS = DC_MAX_V / 32;

__global__ __launch_bounds__(DC_THREADS) void dec_controls_kernel(float* __restrict__ logits, int64_t ldl, int V,
                                                                  const int64_t* __restrict__ tokens, int Ttot,
                                                                  const int* __restrict__ pos_ptr, int P,
                                                                  const int* __restrict__ key_start, float r, int ngram, int min_new,
                                                                  int eos) {
  __shared__ unsigned seen[DC_WORDS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int t = *pos_ptr;
  if (t + 1 < P || t < 0 || t >= Ttot) return;  // the prompt is still being forced (or a position outside the token matrix)
  float* lg = logits + (int64_t)b * ldl;
  int s = key_start ? key_start[b] : 0;
  s = s < 0 ? 0 : (s > t ? t : s);
  const int64_t* h = tokens + (int64_t)b * Ttot + s;
  const int m = t - s + 1;

  if (r != 1.f) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += DC_THREADS) seen[w] = 0u;
    __syncthreads();
    for (int i = tid; i < m; i += DC_THREADS) {
      const int64_t v = h[i];
      if (v < 0 || v >= V) continue;
      const unsigned bit = 1u << ((int)v & 31);
      if (atomicOr(&seen[(int)v >> 5], bit) & bit) continue;  // another occurrence of v got there first: it owns the column
      const float l = lg[v];
      lg[v] = l > 0.f ? l / r : l * r;
    }
  }
  __syncthreads();  // every penalty is stored before a ban may hit the same column

  if (ngram >= 1 && m >= ngram - 1) {
    const int np = ngram - 1;  // the open n-gram: the last n - 1 ids of the history
    const int64_t* tail = h + (m - np);
    for (int i = tid; i + ngram <= m; i += DC_THREADS) {
      bool eq = true;
      for (int j = 0; j < np; ++j) eq = eq && h[i + j] == tail[j];
      const int64_t v = h[i + np];
      if (eq && v >= 0 && v < V) lg[v] = -INFINITY;
    }
  }
  if (tid == 0 && eos >= 0 && t + 1 - P < min_new) lg[eos] = -INFINITY;
}

__global__ __launch_bounds__(64) void dec_finish_kernel(int64_t* __restrict__ tokens, int Ttot, int64_t* __restrict__ tok_cur,
                                                        float* __restrict__ logprobs, int* __restrict__ finished,
                                                        const int* __restrict__ pos_ptr, int P, int64_t eos, int64_t pad, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int t1 = *pos_ptr;  // the tail in front of this launch has advanced the position
  if (b >= B || t1 < P || t1 >= Ttot) return;
  const int64_t at = (int64_t)b * Ttot + t1;
  if (finished[b] != 0) {
    tokens[at] = pad;
    tok_cur[b] = pad;
    if (logprobs) logprobs[at] = 0.f;
  } else if (tokens[at] == eos) {
    finished[b] = t1;
  }
}

}  // namespace

extern "C" int pm_dec_controls(float* logits, int64_t ldl, int64_t V, const int64_t* tokens, int64_t Ttot, const int32_t* pos_ptr,
                               int64_t P, const int32_t* key_start, float repetition_penalty, int64_t no_repeat_ngram,
                               int64_t min_new_tokens, int64_t eos, int64_t B, void* stream) {
  if (!logits || !tokens || !pos_ptr) return PM_EINVAL;
  if (V <= 0 || V > DC_MAX_V || ldl < V || P <= 0 || Ttot < P || Ttot > INT32_MAX || B <= 0 || B > 65535) return PM_EINVAL;
  if (!(repetition_penalty > 0.f) || !(repetition_penalty <= FLT_MAX)) return PM_EINVAL;  // NaN fails both comparisons
  if (no_repeat_ngram < 0 || no_repeat_ngram > DC_MAX_NGRAM) return PM_EINVAL;
  if (min_new_tokens < 0 || min_new_tokens > INT32_MAX || eos < -1 || eos >= V || (min_new_tokens > 0 && eos < 0)) return PM_EINVAL;
  if ((uintptr_t)logits & 3) return PM_EALIGN;
  hipLaunchKernelGGL(dec_controls_kernel, dim3((unsigned)B), dim3(DC_THREADS), 0, (hipStream_t)stream, logits, ldl, (int)V, tokens,
                     (int)Ttot, (const int*)pos_ptr, (int)P, (const int*)key_start, repetition_penalty, (int)no_repeat_ngram,
                     (int)min_new_tokens, (int)eos);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_dec_finish(int64_t* tokens, int64_t Ttot, int64_t* tok_cur, float* logprobs, int32_t* finished,
                             const int32_t* pos_ptr, int64_t P, int64_t eos, int64_t pad, int64_t B, void* stream) {
  if (!tokens || !tok_cur || !finished || !pos_ptr) return PM_EINVAL;
  if (P <= 0 || Ttot < P || Ttot > INT32_MAX || B <= 0 || B > (1 << 20) || eos < 0 || pad < 0) return PM_EINVAL;
  if ((uintptr_t)logprobs & 3) return PM_EALIGN;
  hipLaunchKernelGGL(dec_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tokens, (int)Ttot, tok_cur,
                     logprobs, (int*)finished, (const int*)pos_ptr, (int)P, eos, pad, (int)B);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
