// decode_t5.hip - the stages of one KV-cached T5 decode step that csrc/decode.hip cannot serve (its step assumes a centred
// LayerNorm with a bias, a positional table, bias-carrying projections, n_heads * 64 == d_model and a plain MLP):
//
//   pm_t5_dec_self_fused      RMS norm -> head h's [q|k|v] rows -> cache append at t = *pos -> one query over t + 1 keys with
//                             score + lut[h, t - j] -> att, one workgroup per (sequence, head)
//   pm_t5_dec_rms_qkv         the same projection for all heads, weights read once per 8 sequences (the B * H > 256 form) ...
//   pm_t5_dec_self_attention  ... and its attention launch
//   pm_t5_dec_cross_fused     RMS norm -> head h's q rows -> one query over the first src_len[b] keys of the packed cross K/V
//   pm_t5_dec_geglu           RMS norm -> interleaved [w_f; v_f] rows -> gelu_tanh(a) * b
//   pm_t5_dec_next_token      arg-max over the classifier's tile winners, prompt forcing, eos / pad bookkeeping, the next
//                             step's embedding row (no positional term), ticketed advance of *pos
//   pm_t5_dec_embed           x[b] = E[token[b]] before a run's first step
//
// Activations fp32, weights and caches bf16, every sum in fp32 (as decode.hip).  The projections are dot products on the
// vector ALU - a wave owns four weight rows, a lane 8 (d <= 512) or 16 columns of them - because a decode step is bound by
// the weight stream, not by arithmetic.  Every reduction has a fixed order that depends on nothing but the row's own
// geometry (d, t, src_len): a sequence's result is the same in any batch, for any padding, eager or replayed.
// Masked keys and padded rows are never loaded (they are skipped, not multiplied by zero).
#include "common.h"

namespace {

constexpr int T5_THREADS = 256;
constexpr int T5_MAX_D = 1024;      // the normalised row sits in LDS as 128 chunks of 8
constexpr int T5_MAX_KEYS = 2048;   // scores of one query sit in LDS
constexpr int T5_ROWS = 8;          // sequences per workgroup of the row-group projections

// Four partial sums per lane -> the wave total of a<g> in every lane of 16-lane group g = lane >> 4 (7 shuffles for 4 sums).
__device__ __forceinline__ float reduce4(float a0, float a1, float a2, float a3, int lane) {
  const bool hi32 = (lane & 32) != 0;
  float k0 = hi32 ? a2 : a0, k1 = hi32 ? a3 : a1;
  const float s0 = hi32 ? a0 : a2, s1 = hi32 ? a1 : a3;
  k0 += __shfl_xor(s0, 32, 64);
  k1 += __shfl_xor(s1, 32, 64);
  const bool hi16 = (lane & 16) != 0;
  float k = hi16 ? k1 : k0;
  const float s = hi16 ? k0 : k1;
  k += __shfl_xor(s, 16, 64);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
  return k;
}

__device__ __forceinline__ float dot8(bf16x8 w, f32x4 lo, f32x4 hi, float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = fmaf((float)w[i], lo[i], acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = fmaf((float)w[4 + i], hi[i], acc);
  return acc;
}

__device__ __forceinline__ float block_reduce4w(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// x * rsqrt(mean(x^2) + eps) * gamma of ONE row by the whole workgroup; chunk c (8 columns) goes to xlo[c] | xhi[c].
__device__ __forceinline__ void rms_row_block(const float* __restrict__ x, const float* __restrict__ gamma, float eps, int d,
                                              f32x4* xlo, f32x4* xhi, float* red) {
  const int tid = threadIdx.x, nchunk = d >> 3;
  f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
  if (tid < nchunk) {
    lo = *(const f32x4*)(x + tid * 8);
    hi = *(const f32x4*)(x + tid * 8 + 4);
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) ss = fmaf(lo[i], lo[i], fmaf(hi[i], hi[i], ss));
  const float r = rsqrtf(block_reduce4w(ss, red, false) / (float)d + eps);
  if (tid < nchunk) {
    const f32x4 g0 = *(const f32x4*)(gamma + tid * 8), g1 = *(const f32x4*)(gamma + tid * 8 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { lo[i] = lo[i] * r * g0[i]; hi[i] = hi[i] * r * g1[i]; }
    xlo[tid] = lo;
    xhi[tid] = hi;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------
// RMS norm + a bias-free projection for a group of T5_ROWS sequences and 16 weight rows (4 per wave, held in registers
// across the sequences).  QKV: rows [q|k|v] of (3 * inner, d): q -> out f32, k / v -> bf16 caches at t.  GEGLU: rows
// interleaved [w_0; v_0; w_1; v_1; ...] so that a gate and its value meet in one wave: out[f] = gelu_tanh(w_f x) * (v_f x).
enum { T5_QKV = 0, T5_GEGLU = 1 };

template <int MODE>
__global__ __launch_bounds__(T5_THREADS) void t5_rms_proj_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 float eps, int d, const bf16* __restrict__ W, int N,
                                                                 float* __restrict__ out, int ldo, bf16* __restrict__ kc,
                                                                 bf16* __restrict__ vc, int inner, int H, int Tmax,
                                                                 const int* __restrict__ pos_ptr, int B) {
  __shared__ f32x4 xs[T5_ROWS][2][T5_MAX_D / 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = d >> 3, r0 = blockIdx.y * T5_ROWS, n0 = blockIdx.x * 16 + wave * 4;
  // the weight rows first: they are the long loads, the norm below runs under them
  bf16x8 w[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      const bf16x8 z = __builtin_bit_cast(bf16x8, f32x4{0.f, 0.f, 0.f, 0.f});
      w[j][i] = (c < nchunk && n0 + j < N) ? *(const bf16x8*)(W + (int64_t)(n0 + j) * d + c * 8) : z;
    }
  for (int r = wave; r < T5_ROWS; r += 4) {  // a wave per sequence: no cross-wave traffic in the norm
    const int row = r0 + r;
    if (row >= B) break;
    f32x4 lo[2], hi[2];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      lo[i] = hi[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nchunk) {
        lo[i] = *(const f32x4*)(x + (int64_t)row * d + c * 8);
        hi[i] = *(const f32x4*)(x + (int64_t)row * d + c * 8 + 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(lo[i][e], lo[i][e], fmaf(hi[i][e], hi[i][e], ss));
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)d + eps);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[i][e] = lo[i][e] * rs * g0[e]; hi[i][e] = hi[i][e] * rs * g1[e]; }
        xs[r][0][c] = lo[i];
        xs[r][1][c] = hi[i];
      }
    }
  }
  __syncthreads();
  const int t = MODE == T5_QKV ? *pos_ptr : 0;
  if (MODE == T5_QKV && (t < 0 || t >= Tmax)) return;  // a position outside the caches is never written
  for (int r = 0; r < T5_ROWS; ++r) {
    const int row = r0 + r;
    if (row >= B) break;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        const f32x4 lo = xs[r][0][c], hi = xs[r][1][c];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = dot8(w[j][i], lo, hi, a[j]);
      }
    }
    const float k = reduce4(a[0], a[1], a[2], a[3], lane);
    const int g = lane >> 4, n = n0 + g;
    if constexpr (MODE == T5_GEGLU) {
      const float other = __shfl_xor(k, 16, 64);  // the value row of this gate row (g even)
      if ((lane & 31) == 0 && n + 1 < N) out[(int64_t)row * ldo + (n >> 1)] = apply_act<PM_ACT_GELU_TANH, true>(k) * other;
    } else {
      if ((lane & 15) == 0 && n < N) {
        const int which = n / inner, col = n - which * inner;
        if (which == 0) {
          out[(int64_t)row * ldo + col] = k;
        } else {
          bf16* cache = which == 1 ? kc : vc;
          cache[(((int64_t)row * H + (col >> 6)) * Tmax + t) * 64 + (col & 63)] = (bf16)k;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// One query of head h of sequence b over n keys.  SELF: n = t + 1 keys of the (B, H, Tmax, 64) caches, score + lut[h, t - j];
// cross: n = src_len[b] keys of the packed (B, S, [k | v]) projection of the memory, n == 0 -> zeros.  FUSED: the query (and
// for SELF the new key / value, appended here) come from the RMS-normed x[b] and head h's weight rows; otherwise q is read.
// Keys: a thread per key (128 B rows); values: 8 threads per key, 32 keys in flight, partial sums added in key-group order.
template <bool SELF, bool FUSED>
__global__ __launch_bounds__(T5_THREADS) void t5_attn_kernel(const float* __restrict__ xin, int d, const float* __restrict__ gamma,
                                                             float eps, const bf16* __restrict__ W, int inner,
                                                             bf16* __restrict__ Kc, bf16* __restrict__ Vc, int64_t stride_b,
                                                             int64_t stride_h, int64_t stride_t, int n_max,
                                                             const int* __restrict__ pos_ptr, const int* __restrict__ src_len,
                                                             const float* __restrict__ lut, float* __restrict__ att, int H) {
  __shared__ f32x4 xlo[T5_MAX_D / 8], xhi[T5_MAX_D / 8];
  __shared__ float proj[192];
  __shared__ __attribute__((aligned(16))) float qs[64];  // read back as f32x4
  __shared__ float kcur[64], vcur[64];
  __shared__ float sc[T5_MAX_KEYS];
  __shared__ float part[32][64];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int t = SELF ? *pos_ptr : 0;
  int n = SELF ? t + 1 : src_len[b];
  if (SELF && (t < 0 || t >= n_max)) return;
  n = n < n_max ? n : n_max;
  float* o = att + (int64_t)b * inner + h * 64;
  if (n <= 0) {  // a row with nothing to attend to yields zeros
    if (tid < 64) o[tid] = 0.f;
    return;
  }
  bf16* Kb = Kc + b * stride_b + h * stride_h;
  bf16* Vb = Vc + b * stride_b + h * stride_h;
  if constexpr (FUSED) {
    rms_row_block(xin + (int64_t)b * d, gamma, eps, d, xlo, xhi, red);
    const int nchunk = d >> 3;
    constexpr int NF = SELF ? 192 : 64;
    for (int f0 = wave * 4; f0 < NF; f0 += 16) {
      bf16x8 w[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = f0 + j;
        const bf16* wr = W + (int64_t)((f >> 6) * inner + h * 64 + (f & 63)) * d;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int c = lane + 64 * i;
          const bf16x8 z = __builtin_bit_cast(bf16x8, f32x4{0.f, 0.f, 0.f, 0.f});
          w[j][i] = c < nchunk ? *(const bf16x8*)(wr + c * 8) : z;
        }
      }
      float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
          const f32x4 lo = xlo[c], hi = xhi[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = dot8(w[j][i], lo, hi, a[j]);
        }
      }
      const float k = reduce4(a[0], a[1], a[2], a[3], lane);
      if ((lane & 15) == 0) proj[f0 + (lane >> 4)] = k;
    }
    __syncthreads();
    if (tid < 64) {
      qs[tid] = proj[tid];
      if constexpr (SELF) {  // rounded once, where they are cached; this step reads its own pair from LDS
        const bf16 kb = (bf16)proj[64 + tid], vb = (bf16)proj[128 + tid];
        Kb[t * stride_t + tid] = kb;
        Vb[t * stride_t + tid] = vb;
        kcur[tid] = (float)kb;
        vcur[tid] = (float)vb;
      }
    }
  } else {
    if (tid < 64) qs[tid] = xin[(int64_t)b * inner + h * 64 + tid];
  }
  __syncthreads();
  constexpr bool OWN = SELF && FUSED;  // key / value t live in kcur / vcur
  float q[64];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const f32x4 v = *(const f32x4*)(qs + i * 4);
    q[4 * i] = v[0]; q[4 * i + 1] = v[1]; q[4 * i + 2] = v[2]; q[4 * i + 3] = v[3];
  }
  float m = -INFINITY;
  for (int j = tid; j < n; j += T5_THREADS) {
    float s = 0.f;
    if (OWN && j == t) {
#pragma unroll
      for (int i = 0; i < 64; ++i) s = fmaf(q[i], kcur[i], s);
    } else {
      const bf16* kp = Kb + j * stride_t;
      bf16x8 kk[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) kk[c] = *(const bf16x8*)(kp + c * 8);
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(q[c * 8 + e], (float)kk[c][e], s);
    }
    s *= 0.125f;  // 1 / sqrt(64), as the attention kernels of the full-sequence path
    if constexpr (SELF) s += lut[(int64_t)h * n_max + (t - j)];
    sc[j] = s;
    m = fmaxf(m, s);
  }
  m = block_reduce4w(m, red, true);
  float l = 0.f;
  for (int j = tid; j < n; j += T5_THREADS) {
    const float p = expf(sc[j] - m);
    sc[j] = p;
    l += p;
  }
  l = block_reduce4w(l, red, false);  // (its barriers also publish sc)
  const int g = tid >> 3, oc = tid & 7;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = g; j < n; j += 32) {
    const float p = sc[j];
    if (OWN && j == t) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, vcur[oc * 8 + e], acc[e]);
    } else {
      const bf16x8 v = *(const bf16x8*)(Vb + j * stride_t + oc * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, (float)v[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[g][oc * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
#pragma unroll
    for (int gg = 0; gg < 32; ++gg) s += part[gg][tid];
    o[tid] = s / l;
  }
}

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T5_THREADS) void t5_embed_kernel(const int64_t* __restrict__ tok, int64_t ldtok,
                                                              const bf16* __restrict__ E, float* __restrict__ x, int d, int V) {
  const int b = blockIdx.x;
  int64_t id = tok[b * ldtok];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  for (int c = threadIdx.x; c < d / 8; c += T5_THREADS) {
    const bf16x8 e = *(const bf16x8*)(E + id * d + c * 8);
    f32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o0[i] = (float)e[i]; o1[i] = (float)e[4 + i]; }
    *(f32x4*)(x + (int64_t)b * d + c * 8) = o0;
    *(f32x4*)(x + (int64_t)b * d + c * 8 + 4) = o1;
  }
}

// Sequence b's workgroup: the winner over the classifier's tile winners (lowest index on ties), unless position t + 1 is
// still inside the forced prompt or the row has finished (then pad_id); a generated eos_id finishes the row and fixes its
// length; the next step's x[b] = E[token]; optionally the step's full logits row is filed at step t; the last workgroup to
// arrive (agent-scope ticket, vector atomics) stores t + 1 to *pos_rw and returns the ticket to zero.
__global__ __launch_bounds__(T5_THREADS) void t5_next_token_kernel(
    const float* __restrict__ ws_val, const int* __restrict__ ws_idx, int nt, int* pos_rw, const int64_t* __restrict__ prompt, int P,
    int64_t* __restrict__ tokens, int Ttot, int pad_id, int eos_id, int* __restrict__ finished, int64_t* __restrict__ out_len,
    const bf16* __restrict__ E, float* __restrict__ x, int d, int V, int* ticket, const float* __restrict__ logits_step,
    float* __restrict__ logits_all) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int64_t snext;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = *pos_rw, t1 = t + 1;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < nt; i += T5_THREADS) {
    const float v = ws_val[(int64_t)b * nt + i];
    const int ix = ws_idx[(int64_t)b * nt + i];
    if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    if (bi == 0x7fffffff) bi = 0;  // a row without a maximum (every tile at -inf, or NaN): index 0, as torch.argmax on -inf
    int64_t next;
    if (t1 < P) {
      next = prompt[(int64_t)b * P + t1];
    } else if (finished[b]) {
      next = pad_id;
    } else {
      next = bi;
      if (eos_id >= 0 && bi == eos_id) {
        finished[b] = 1;
        out_len[b] = t1 + 1;
      }
    }
    if (t1 < Ttot) tokens[(int64_t)b * Ttot + t1] = next;
    snext = next;
  }
  __syncthreads();
  int64_t id = snext;
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  for (int c = tid; c < d / 8; c += T5_THREADS) {
    const bf16x8 e = *(const bf16x8*)(E + id * d + c * 8);
    f32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o0[i] = (float)e[i]; o1[i] = (float)e[4 + i]; }
    *(f32x4*)(x + (int64_t)b * d + c * 8) = o0;
    *(f32x4*)(x + (int64_t)b * d + c * 8 + 4) = o1;
  }
  if (logits_all && t >= 0 && t < Ttot - 1) {
    float* dst = logits_all + ((int64_t)b * (Ttot - 1) + t) * V;
    for (int v = tid; v < V; v += T5_THREADS) dst[v] = logits_step[(int64_t)b * V + v];
  }
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int n = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == (int)gridDim.x - 1) {
      __hip_atomic_store(pos_rw, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)e) & 15) != 0;
}

}  // namespace

// =================================================================================================================
extern "C" int pm_t5_dec_embed(const int64_t* tok, int64_t ldtok, const void* emb, float* x, int64_t B, int64_t d, int64_t V,
                               void* stream) {
  if (!tok || !emb || !x || B <= 0 || d <= 0 || V <= 0 || ldtok <= 0) return PM_EINVAL;
  if (d % 8) return PM_EUNSUPPORTED;
  if (misaligned16(emb, x)) return PM_EALIGN;
  hipLaunchKernelGGL(t5_embed_kernel, dim3((unsigned)B), dim3(T5_THREADS), 0, (hipStream_t)stream, tok, ldtok, (const bf16*)emb, x,
                     (int)d, (int)V);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

static int t5_check_norm_proj(const void* x, const float* gamma, const void* w, int64_t B, int64_t d) {
  if (!x || !gamma || !w || B <= 0 || d <= 0) return PM_EINVAL;
  if (B > 64 || d % 8 || d > T5_MAX_D) return PM_EUNSUPPORTED;
  if (misaligned16(x, gamma, w)) return PM_EALIGN;
  return PM_OK;
}

extern "C" int pm_t5_dec_self_fused(const float* x, int64_t d, const float* gamma, float eps, const void* w_qkv, void* kcache,
                                    void* vcache, int64_t Tmax, const int32_t* pos_ptr, const float* lut, float* att, int64_t B,
                                    int64_t H, void* stream) {
  if (const int rc = t5_check_norm_proj(x, gamma, w_qkv, B, d)) return rc;
  if (!kcache || !vcache || !pos_ptr || !lut || !att || H <= 0 || Tmax <= 0) return PM_EINVAL;
  if (Tmax > T5_MAX_KEYS) return PM_EUNSUPPORTED;
  if (misaligned16(kcache, vcache, att)) return PM_EALIGN;
  hipLaunchKernelGGL((t5_attn_kernel<true, true>), dim3((unsigned)(B * H)), dim3(T5_THREADS), 0, (hipStream_t)stream, x, (int)d,
                     gamma, eps, (const bf16*)w_qkv, (int)(H * 64), (bf16*)kcache, (bf16*)vcache, H * Tmax * 64, Tmax * 64,
                     (int64_t)64, (int)Tmax, (const int*)pos_ptr, (const int*)nullptr, lut, att, (int)H);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_t5_dec_rms_qkv(const float* x, int64_t d, const float* gamma, float eps, const void* w_qkv, float* q,
                                 void* kcache, void* vcache, int64_t Tmax, const int32_t* pos_ptr, int64_t B, int64_t H,
                                 void* stream) {
  if (const int rc = t5_check_norm_proj(x, gamma, w_qkv, B, d)) return rc;
  if (!q || !kcache || !vcache || !pos_ptr || H <= 0 || Tmax <= 0) return PM_EINVAL;
  const int64_t inner = H * 64, N = 3 * inner;
  const dim3 grid((unsigned)(N / 16), (unsigned)((B + T5_ROWS - 1) / T5_ROWS));
  hipLaunchKernelGGL((t5_rms_proj_kernel<T5_QKV>), grid, dim3(T5_THREADS), 0, (hipStream_t)stream, x, gamma, eps, (int)d,
                     (const bf16*)w_qkv, (int)N, q, (int)inner, (bf16*)kcache, (bf16*)vcache, (int)inner, (int)H, (int)Tmax,
                     (const int*)pos_ptr, (int)B);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_t5_dec_self_attention(const float* q, const void* kcache, const void* vcache, int64_t Tmax,
                                        const int32_t* pos_ptr, const float* lut, float* att, int64_t B, int64_t H, void* stream) {
  if (!q || !kcache || !vcache || !pos_ptr || !lut || !att || B <= 0 || H <= 0 || Tmax <= 0) return PM_EINVAL;
  if (Tmax > T5_MAX_KEYS) return PM_EUNSUPPORTED;
  if (misaligned16(q, kcache, vcache, att)) return PM_EALIGN;
  hipLaunchKernelGGL((t5_attn_kernel<true, false>), dim3((unsigned)(B * H)), dim3(T5_THREADS), 0, (hipStream_t)stream, q, 0,
                     (const float*)nullptr, 0.f, (const bf16*)nullptr, (int)(H * 64), (bf16*)kcache, (bf16*)vcache, H * Tmax * 64,
                     Tmax * 64, (int64_t)64, (int)Tmax, (const int*)pos_ptr, (const int*)nullptr, lut, att, (int)H);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_t5_dec_cross_fused(const float* x, int64_t d, const float* gamma, float eps, const void* w_q, const void* cross_kv,
                                     int64_t S, const int32_t* src_len, float* att, int64_t B, int64_t H, void* stream) {
  if (const int rc = t5_check_norm_proj(x, gamma, w_q, B, d)) return rc;
  if (!cross_kv || !src_len || !att || H <= 0 || S <= 0) return PM_EINVAL;
  if (S > T5_MAX_KEYS) return PM_EUNSUPPORTED;
  if (misaligned16(cross_kv, att)) return PM_EALIGN;
  const int64_t inner = H * 64;
  hipLaunchKernelGGL((t5_attn_kernel<false, true>), dim3((unsigned)(B * H)), dim3(T5_THREADS), 0, (hipStream_t)stream, x, (int)d,
                     gamma, eps, (const bf16*)w_q, (int)inner, (bf16*)cross_kv, (bf16*)cross_kv + inner, S * 2 * inner, (int64_t)64,
                     2 * inner, (int)S, (const int*)nullptr, (const int*)src_len, (const float*)nullptr, att, (int)H);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_t5_dec_geglu(const float* x, int64_t d, const float* gamma, float eps, const void* w_wv, float* h, int64_t ldh,
                               int64_t B, int64_t F, void* stream) {
  if (const int rc = t5_check_norm_proj(x, gamma, w_wv, B, d)) return rc;
  if (!h || F <= 0 || ldh < F) return PM_EINVAL;
  if (F % 8) return PM_EUNSUPPORTED;  // 16 interleaved rows per workgroup
  const dim3 grid((unsigned)(2 * F / 16), (unsigned)((B + T5_ROWS - 1) / T5_ROWS));
  hipLaunchKernelGGL((t5_rms_proj_kernel<T5_GEGLU>), grid, dim3(T5_THREADS), 0, (hipStream_t)stream, x, gamma, eps, (int)d,
                     (const bf16*)w_wv, (int)(2 * F), h, (int)ldh, (bf16*)nullptr, (bf16*)nullptr, 0, 0, 0, (const int*)nullptr,
                     (int)B);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_t5_dec_next_token(const float* ws_val, const int32_t* ws_idx, int64_t n_tiles, int32_t* pos_ptr,
                                    const int64_t* prompt, int64_t P, int64_t* tokens, int64_t Ttot, int64_t pad_id,
                                    int64_t eos_id, int32_t* finished, int64_t* out_lengths, const void* emb, float* x, int64_t d,
                                    int64_t V, int32_t* ticket, const float* logits_step, float* logits_all, int64_t B,
                                    void* stream) {
  if (!ws_val || !ws_idx || !pos_ptr || !prompt || !tokens || !finished || !out_lengths || !emb || !x || !ticket) return PM_EINVAL;
  if (n_tiles <= 0 || P < 1 || Ttot < P || B <= 0 || d <= 0 || V <= 0 || pad_id < 0 || pad_id >= V || eos_id >= V) return PM_EINVAL;
  if ((logits_step == nullptr) != (logits_all == nullptr)) return PM_EINVAL;
  if (d % 8) return PM_EUNSUPPORTED;
  if (misaligned16(emb, x)) return PM_EALIGN;
  hipLaunchKernelGGL(t5_next_token_kernel, dim3((unsigned)B), dim3(T5_THREADS), 0, (hipStream_t)stream, ws_val, (const int*)ws_idx,
                     (int)n_tiles, (int*)pos_ptr, prompt, (int)P, tokens, (int)Ttot, (int)pad_id, (int)(eos_id < 0 ? -1 : eos_id),
                     (int*)finished, out_lengths, (const bf16*)emb, x, (int)d, (int)V, (int*)ticket, logits_step, logits_all);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
