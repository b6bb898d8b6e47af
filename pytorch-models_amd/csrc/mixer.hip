// mixer.hip - MLP-Mixer (reference: pytorch_models/image/mlp_mixer.py) kernels that the shared blocks do not serve.
//
//  * pm_mixer_token_mix_bf16  y = x + token_mixing(norm1(x)^T)^T on the (N, T, C) bf16 stream, one kernel (mlp_mixer.py:30).
//  * pm_row_stats             (M, C) rows -> (M, 2) [mean, rstd], the format pm_ln_stats_finalize writes.
//  * pm_ln_mean               head: mean over tokens of LayerNorm(x) (mlp_mixer.py:58-59), from the rows' statistics.
//  * pm_transpose_add_f32     y (N, Cc, R) = x (N, R, Cc)^T [+ resid]: the two transposes of the composed fp32 token mixing.
//
// Token mixing contracts over the TOKEN index, which is strided in the row-major stream.  A workgroup (8 waves) owns one
// image and a slab of CS = 32 * NB channels (NB = 4, or 2 where LDS is short):
//   phase 0  the slab is read once (16-byte row-major loads), normalised with the rows' (mean, rstd) and norm1's gamma / beta,
//            rounded to bf16 and written TRANSPOSED into LDS, xs[channel][token]; tokens T .. Tp-1 (Tp = T rounded up to 16,
//            the MFMA K step) are zeros, and W1 arrives with zero columns there, so the padding adds exact zeros.
//   phase 1  H = GELU(W1 Xn + b1): wave w takes the 32-row strips w, w+8, .. of W1; A = W1 fragments from global memory (each
//            is used for NB MFMAs), B = xs (channel on the lane, 8 tokens per lane contiguous).  The 32 x 32 accumulator has
//            the channel on the lane and 4 consecutive hidden rows per register group: bias + GELU + bf16 and an 8-byte write
//            to hs[channel][hidden].
//   phase 2  Y = W2 H: wave w takes the 32-token strips w, w+8, .. of W2 (rows past T are zero rows and never stored), B = hs.
//            Each 32 x 32 tile crosses a per-wave LDS scratch (aliasing xs, which is dead) to become row-major: + b2[token]
//            + x, one rounding to bf16, 32-byte stores, and the (sum, sum of squares) of the ROUNDED values per row and
//            64-channel block go to row_out in the layout pm_ln_stats_finalize reads.
// The weights arrive FRAGMENT-MAJOR (pm_mi355x.h; packed once per model): the 64 lanes' A fragments of one strip and K step
// are 1 KiB contiguous.  Read from row-major weights a wave's load touched 32 rows x 32 B, a quarter of every 128-byte line
// (measured at B/16, batch 256: 162 -> 150 us; the L2's weight traffic is the kernel's bound).
// In place (y == x) is safe: a workgroup reads its whole slab in phase 0, re-reads an element for the residual only in the thread
// that then writes it, and no other workgroup touches the slab.
// Weight reuse: a pass over W1 and W2 serves one image x CS channels; with NB = 4 that is 2x the one-image x 64-channel unit.
#include <atomic>

#include "common.h"

namespace {

constexpr int MX_WAVES = 8;  // two per SIMD: one wave's epilogue and load latency hide behind the other's MFMAs
constexpr int MX_THREADS = 64 * MX_WAVES;
constexpr int MX_SCR_LD = 33;                                   // f32 scratch row (32 + 1: column writes hit 32 banks)
constexpr int MX_SCR_BYTES = MX_WAVES * 32 * MX_SCR_LD * 4;     // one 32 x 32 tile per wave
constexpr int MX_LDS_MAX = 160 * 1024;

__host__ __device__ inline int mx_tp(int T) { return (T + 15) / 16 * 16; }
inline int mx_region_a(int nb, int T) {
  const int xs = 32 * nb * (mx_tp(T) + 8) * 2;
  return ((xs > MX_SCR_BYTES ? xs : MX_SCR_BYTES) + 15) / 16 * 16;
}
inline int mx_lds_bytes(int nb, int T, int Dt) { return mx_region_a(nb, T) + 32 * nb * (Dt + 8) * 2; }
inline int mx_pick_nb(int64_t T, int64_t Dt, int64_t C) {
  if (T < 1 || T > 4096 || Dt < 32 || Dt > 4096 || Dt % 32 || C < 64 || C % 64) return 0;
  if (C % 128 == 0 && mx_lds_bytes(4, (int)T, (int)Dt) <= MX_LDS_MAX) return 4;
  return mx_lds_bytes(2, (int)T, (int)Dt) <= MX_LDS_MAX ? 2 : 0;
}

// The A operand (weight rows) streams from global memory / L2 through a ring of MX_RING fragments per lane: step k of a
// 32-row strip uses ring[k % MX_RING] and then refills it with step k + MX_RING, so MX_RING x NB MFMAs cover a load's latency
// (one step ahead, a wave - the only one on its SIMD - waited a full L2 round trip per K step).  Refills that would run past
// the strip fetch the NEXT strip's first fragments instead, so the ring never drains between strips, nor between phase 1
// and phase 2.  The B fragments of step k + 1 are read from LDS before the MFMAs of step k.  Indices are clamped, never out
// of bounds.
constexpr int MX_RING = 8;
constexpr int MX_FRAG = 64 * 8;  // elements between a lane's fragments of consecutive K steps in the fragment-major weights

__device__ __forceinline__ void ring_prime(bf16x8 (&ring)[MX_RING], const bf16* ap, int nk) {
#pragma unroll
  for (int j = 0; j < MX_RING; ++j) ring[j] = *(const bf16x8*)(ap + MX_FRAG * min(j, nk - 1));
}

// acc[nb] += A strip (32 rows x 16 nk, ap already at the lane's fragment of step 0) x B tile nb, B in LDS at
// bl + nb * 32 * ldb (the lane's row and k half folded into bl).  On entry ring[j] holds step j of this strip (j < nk), on
// exit step j of the next one.
template <int NB>
__device__ __forceinline__ void mma_strip(bf16x8 (&ring)[MX_RING], const bf16* ap, int nk, const bf16* ap_next, int nk_next,
                                          const bf16* bl, int ldb, f32x16 (&acc)[NB]) {
  const int full = nk / MX_RING * MX_RING;
  bf16x8 b[NB], bn[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) b[nb] = *(const bf16x8*)(bl + nb * 32 * ldb);
  for (int k = 0; k < full; k += MX_RING) {
#pragma unroll
    for (int j = 0; j < MX_RING; ++j) {
      const int kk = k + j;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bn[nb] = *(const bf16x8*)(bl + nb * 32 * ldb + min(kk + 1, nk - 1) * 16);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[j], b[nb], acc[nb], 0, 0, 0);
      const bf16* src = kk + MX_RING < nk ? ap + MX_FRAG * (kk + MX_RING) : ap_next + MX_FRAG * min(j, nk_next - 1);
      ring[j] = *(const bf16x8*)src;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) b[nb] = bn[nb];
    }
  }
  if (full < nk) {  // the last, partial round; every slot ends on the next strip's step j
#pragma unroll
    for (int j = 0; j < MX_RING; ++j) {
      const int kk = full + j;
      if (kk < nk) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bn[nb] = *(const bf16x8*)(bl + nb * 32 * ldb + min(kk + 1, nk - 1) * 16);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[j], b[nb], acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[nb] = bn[nb];
      }
      ring[j] = *(const bf16x8*)(ap_next + MX_FRAG * min(j, nk_next - 1));
    }
  }
}

// the value of lane ^ 1 (quad_perm [1, 0, 3, 2]); every lane must be active
__device__ __forceinline__ float lane_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

// LDS written by some lanes of a wave and read by others of the SAME wave: the wave's DS instructions execute in order, so
// only the compiler has to be kept from moving them across this point
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NB>
__global__ __launch_bounds__(MX_THREADS) void mixer_token_mix_kernel(
    const bf16* x, const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
    const bf16* __restrict__ w1, const float* __restrict__ b1, const bf16* __restrict__ w2, const float* __restrict__ b2,
    bf16* y, float* __restrict__ row_out, int T, int Dt, int C, int region_a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CS = 32 * NB;
  const int Tp = mx_tp(T), XS = Tp + 8, HS = Dt + 8;
  bf16* xs = (bf16*)smem;               // [CS][XS]
  bf16* hs = (bf16*)(smem + region_a);  // [CS][HS]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int n = blockIdx.y, c0 = blockIdx.x * CS;
  const int64_t row0 = (int64_t)n * T;
  const bf16* xb = x + row0 * C + c0;
  const int nk1 = Tp / 16, nk2 = Dt / 16, nd = Dt / 32, nt = (T + 31) / 32;

  // the ring starts on the wave's first W1 strip while phase 0 runs (nd >= 1; a wave without a strip loads strip 0, unused)
  bf16x8 ring[MX_RING];
  // (the weights are fragment-major: strip s, step k, lane l at ((s * nk + k) * 64 + l) * 8 - a wave's load is 1 KiB contiguous)
  auto w1_strip = [&](int db) { return w1 + ((int64_t)(db < nd ? db : 0) * nk1 * 64 + lane) * 8; };
  auto w2_strip = [&](int tt) { return w2 + ((int64_t)(tt < nt ? tt : 0) * nk2 * 64 + lane) * 8; };
  ring_prime(ring, w1_strip(wv), nk1);

  // ---- phase 0: normalise the slab into xs[channel][token].  A wave takes units of 32 token pairs x 2 chunks of 8 channels:
  // a lane loads its chunk of two consecutive rows and writes 8 packed token pairs (ds_write_b32).  The LDS bank of a write
  // depends on the token pair alone (a chunk's rows are a multiple of 128 B apart), so 32 pairs x 2 chunks is 2-way, where
  // 16 chunks x 4 tokens per wave was 16-way.
  {
    constexpr int CH = CS / 8;
    const int np2 = (T + 1) / 2, nu = (CH / 2) * ((np2 + 31) / 32);
#pragma unroll 4
    for (int u = wv; u < nu; u += MX_WAVES) {
      const int cc = 2 * (u % (CH / 2)) + (lane & 1), tp = (u / (CH / 2)) * 32 + (lane >> 1);
      const int t0 = min(2 * tp, T - 1), t1 = min(2 * tp + 1, T - 1);
      const bf16x8 v0 = *(const bf16x8*)(xb + (int64_t)t0 * C + cc * 8), v1 = *(const bf16x8*)(xb + (int64_t)t1 * C + cc * 8);
      const f32x2 s0 = *(const f32x2*)(stats + (row0 + t0) * 2), s1 = *(const f32x2*)(stats + (row0 + t1) * 2);
      const f32x4 g0 = *(const f32x4*)(gamma + c0 + cc * 8), g1 = *(const f32x4*)(gamma + c0 + cc * 8 + 4);
      const f32x4 e0 = *(const f32x4*)(beta + c0 + cc * 8), e1 = *(const f32x4*)(beta + c0 + cc * 8 + 4);
      if (2 * tp < T) {
        const bool two = 2 * tp + 1 < T;  // an odd T: the pair's second token is padding, zero
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float g = i < 4 ? g0[i & 3] : g1[i & 3], e = i < 4 ? e0[i & 3] : e1[i & 3];
          bf16x2 p;
          p[0] = (bf16)fmaf(((float)v0[i] - s0[0]) * s0[1], g, e);
          p[1] = two ? (bf16)fmaf(((float)v1[i] - s1[0]) * s1[1], g, e) : (bf16)0.0f;
          *(bf16x2*)(xs + (cc * 8 + i) * XS + 2 * tp) = p;
        }
      }
    }
    const int tz = (T + 1) / 2 * 2, np = Tp - tz;  // the rest of the K padding
    for (int idx = tid; idx < CS * np; idx += MX_THREADS) xs[(idx / np) * XS + tz + idx % np] = (bf16)0.0f;
  }
  __syncthreads();

  // ---- phase 1: hs[channel][hidden] = bf16(GELU(W1 Xn + b1))
  for (int db = wv; db < nd; db += MX_WAVES) {
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
    f32x4 bb[4];  // the bias of the lane's 16 hidden rows, in flight during the strip
#pragma unroll
    for (int g = 0; g < 4; ++g) bb[g] = *(const f32x4*)(b1 + db * 32 + 8 * g + 4 * h);
    const bool last = db + MX_WAVES >= nd;  // then the ring runs on into the wave's first W2 strip
    mma_strip<NB>(ring, w1_strip(db), nk1, last ? w2_strip(wv) : w1_strip(db + MX_WAVES), last ? nk2 : nk1, xs + r * XS + 8 * h, XS, acc);
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // registers 4g .. 4g+3 = hidden rows db*32 + 8g + 4h + (0..3)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        f32x4 v = {acc[nb][4 * g] + bb[g][0], acc[nb][4 * g + 1] + bb[g][1], acc[nb][4 * g + 2] + bb[g][2], acc[nb][4 * g + 3] + bb[g][3]};
        v = apply_act4<PM_ACT_GELU>(v);
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)v[i];
        *(bf16x4*)(hs + (nb * 32 + r) * HS + db * 32 + 8 * g + 4 * h) = o;
      }
    }
  }
  if (wv >= nd) ring_prime(ring, w2_strip(wv), nk2);  // a wave that had no W1 strip
  __syncthreads();  // hs complete; xs is dead from here on (the per-wave scratch aliases it)

  // ---- phase 2: y = x + W2 H + b2
  float* scr = (float*)smem + wv * 32 * MX_SCR_LD;
  const int nblk = C / 64;
  const int orow = lane >> 1, half = lane & 1;  // epilogue: two lanes per token row, 16 channels each
  for (int tt = wv; tt < nt; tt += MX_WAVES) {
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
    const int t = tt * 32 + orow;
    const bool live = t < T;
    // the residual and the bias of the lane's output row are loaded before the strip: their latency hides behind its MFMAs.
    // (In place: these elements are written by this thread alone, after it has read them.)
    const int64_t off0 = (row0 + (live ? t : 0)) * C + c0 + half * 16;
    bf16x8 xr[NB][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      xr[nb][0] = *(const bf16x8*)(x + off0 + nb * 32);
      xr[nb][1] = *(const bf16x8*)(x + off0 + nb * 32 + 8);
    }
    const float bias2 = b2[live ? t : 0];
    mma_strip<NB>(ring, w2_strip(tt), nk2, w2_strip(tt + MX_WAVES), nk2, hs + r * HS + 8 * h, HS, acc);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int64_t off = off0 + nb * 32;
      const bf16x8 x0 = xr[nb][0], x1 = xr[nb][1];
#pragma unroll
      for (int i = 0; i < 16; ++i) scr[((i & 3) + 8 * (i >> 2) + 4 * h) * MX_SCR_LD + r] = acc[nb][i];
      wave_lds_sync();
      if (live) {
        const float* sp = scr + orow * MX_SCR_LD + half * 16;
        bf16x8 o0, o1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          o0[i] = (bf16)(sp[i] + bias2 + (float)x0[i]);
          o1[i] = (bf16)(sp[8 + i] + bias2 + (float)x1[i]);
        }
        // the statistics are those of the ROUNDED values: v_dot2_f32_bf16 on the stored pairs, sum = pair . (1, 1), sum of squares =
        // pair . pair, fp32 accumulation.  (Deliberately no chain of f32 adds here: see DESIGN.md section 13, "row sums".)
        const bf16x2 ones = {(bf16)1.0f, (bf16)1.0f};
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          const bf16x2 p0 = {o0[i], o0[i + 1]}, p1 = {o1[i], o1[i + 1]};
          s1 = __builtin_amdgcn_fdot2_f32_bf16(p0, ones, s1, false);
          s2 = __builtin_amdgcn_fdot2_f32_bf16(p0, p0, s2, false);
          s1 = __builtin_amdgcn_fdot2_f32_bf16(p1, ones, s1, false);
          s2 = __builtin_amdgcn_fdot2_f32_bf16(p1, p1, s2, false);
        }
        *(bf16x8*)(y + off) = o0;
        *(bf16x8*)(y + off + 8) = o1;
      }
      wave_lds_sync();
      if (nb & 1) {  // a 64-channel block is complete: combine the row's two lanes
        s1 += lane_xor1(s1);  // the row's other lane (quad_perm DPP, as the GEMM epilogues' sum8_dpp: VALU only, no LDS)
        s2 += lane_xor1(s2);
        if (live && half == 0 && row_out) {
          f32x2 p = {s1, s2};
          *(f32x2*)(row_out + ((row0 + t) * nblk + (c0 >> 6) + (nb >> 1)) * 2) = p;
        }
        s1 = s2 = 0.f;
      }
    }
  }
}

// one wave per row: mean, then the centred second moment (two passes over a row that stays in cache)
template <typename TX>
__global__ __launch_bounds__(256) void row_stats_kernel(const TX* __restrict__ x, int64_t ldx, float* __restrict__ stats, int64_t M, int C,
                                                        float eps) {
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  const TX* xr = x + m * ldx;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += (float)xr[c];
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = (float)xr[c] - mean;
    q = fmaf(d, d, q);
  }
  const float var = wave_sum(q) / (float)C;
  if (lane == 0) {
    stats[2 * m] = mean;
    stats[2 * m + 1] = rsqrtf(var + eps);
  }
}

// thread per channel, tokens in order (deterministic): y[n][c] = gamma[c] * mean_t((x[n][t][c] - mean_t) * rstd_t) + beta[c]
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void ln_mean_kernel(const TX* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, TY* __restrict__ y, int T, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (c >= C) return;
  const TX* xp = x + (int64_t)n * T * C + c;
  const float* st = stats + (int64_t)n * T * 2;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += ((float)xp[(int64_t)t * C] - st[2 * t]) * st[2 * t + 1];
  y[(int64_t)n * C + c] = (TY)fmaf(acc / (float)T, gamma[c], beta[c]);
}

// x (N, R, Cc) -> y (N, Cc, R) [+ resid (N, Cc, R)], y / resid rows with stride ldy, through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void transpose_add_f32_kernel(const float* __restrict__ x, const float* __restrict__ resid, float* __restrict__ y,
                                                                int R, int Cc, int64_t ldy) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* xn = x + (int64_t)n * R * Cc;
  for (int j = ty; j < 32; j += 8)
    if (r0 + j < R && c0 + tx < Cc) tile[j][tx] = xn[(int64_t)(r0 + j) * Cc + c0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, rr = r0 + tx;
    if (c < Cc && rr < R) {
      const int64_t o = ((int64_t)n * Cc + c) * ldy + rr;
      y[o] = tile[tx][j] + (resid ? resid[o] : 0.f);
    }
  }
}

template <int NB>
int launch_token_mix(size_t lds, dim3 grid, hipStream_t st, const bf16* x, const float* stats, const float* gamma, const float* beta,
                     const bf16* w1, const float* b1, const bf16* w2, const float* b2, bf16* y, float* row_out, int T, int Dt,
                     int C, int region_a) {
  auto kern = mixer_token_mix_kernel<NB>;
  // per instantiation: raise the dynamic-LDS limit at the first call (outside any stream capture: captures follow a warm-up).
  // Two host threads may both find the flag clear and both set the same attribute, which is harmless.
  static std::atomic<bool> lds_raised{false};
  if (!lds_raised.load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS_MAX) != hipSuccess) return PM_ELAUNCH;
    lds_raised.store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(kern, grid, dim3(MX_THREADS), lds, st, x, stats, gamma, beta, w1, b1, w2, b2, y, row_out, T, Dt, C, region_a);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int pm_mixer_token_mix_supported(int64_t T, int64_t Dt, int64_t C) { return mx_pick_nb(T, Dt, C) ? 1 : 0; }

/* Host-only: what pm_mixer_token_mix_bf16 launches for these shapes, from the functions it launches by; report = 8 int32: NB,
 * the dynamic LDS bytes, region_a, nk1, nk2, nd, nt, and 1 where region_a is the per-wave scratch (the slab is smaller), 0 where
 * it is the slab.  Nothing is dereferenced but the report, nothing is launched; a refusal writes nothing. */
extern "C" int pm_mixer_token_mix_plan(int64_t T, int64_t Dt, int64_t C, int32_t* report) {
  if (!report) return PM_EINVAL;
  const int nb = mx_pick_nb(T, Dt, C);
  if (!nb) return PM_EUNSUPPORTED;
  const int ra = mx_region_a(nb, (int)T);
  const int32_t r[8] = {nb, mx_lds_bytes(nb, (int)T, (int)Dt), ra, mx_tp((int)T) / 16, (int32_t)(Dt / 16), (int32_t)(Dt / 32),
                        (int32_t)((T + 31) / 32), 32 * nb * (mx_tp((int)T) + 8) * 2 > MX_SCR_BYTES ? 0 : 1};
  for (int i = 0; i < 8; ++i) report[i] = r[i];
  return PM_OK;
}

extern "C" int pm_mixer_token_mix_bf16(const void* x, const float* stats, const float* gamma, const float* beta, const void* w1,
                                       const float* b1, const void* w2, const float* b2, void* y, float* row_out, int64_t N,
                                       int64_t T, int64_t Dt, int64_t C, void* stream) {
  if (!x || !stats || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !y || N < 0) return PM_EINVAL;
  const int nb = mx_pick_nb(T, Dt, C);
  if (!nb) return PM_EUNSUPPORTED;
  if (!al16(x) || !al16(y) || !al16(w1) || !al16(w2) || !al16(gamma) || !al16(beta) || !al16(b1) || ((uintptr_t)stats & 7) ||
      ((uintptr_t)row_out & 7))
    return PM_EALIGN;
  if (N == 0) return PM_OK;
  if (N > 65535) return PM_EUNSUPPORTED;
  const dim3 grid((unsigned)(C / (32 * nb)), (unsigned)N);
  const size_t lds = (size_t)mx_lds_bytes(nb, (int)T, (int)Dt);
  const int ra = mx_region_a(nb, (int)T);
  if (nb == 4)
    return launch_token_mix<4>(lds, grid, (hipStream_t)stream, (const bf16*)x, stats, gamma, beta, (const bf16*)w1, b1,
                               (const bf16*)w2, b2, (bf16*)y, row_out, (int)T, (int)Dt, (int)C, ra);
  return launch_token_mix<2>(lds, grid, (hipStream_t)stream, (const bf16*)x, stats, gamma, beta, (const bf16*)w1, b1,
                             (const bf16*)w2, b2, (bf16*)y, row_out, (int)T, (int)Dt, (int)C, ra);
}

extern "C" int pm_row_stats(const void* x, int64_t ldx, int x_dtype, float* stats, int64_t M, int64_t C, float eps, void* stream) {
  if (!x || !stats || M < 0 || C <= 0 || ldx < C) return PM_EINVAL;
  if (C > (1 << 20)) return PM_EUNSUPPORTED;
  if (M == 0) return PM_OK;
  const dim3 grid((unsigned)((M + 3) / 4));
  if (x_dtype == PM_BF16)
    hipLaunchKernelGGL(row_stats_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, stats, M, (int)C, eps);
  else if (x_dtype == PM_F32)
    hipLaunchKernelGGL(row_stats_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, stats, M, (int)C, eps);
  else
    return PM_EINVAL;
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_ln_mean(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y, int y_dtype,
                          int64_t N, int64_t T, int64_t C, void* stream) {
  if (!x || !stats || !gamma || !beta || !y || N < 0 || T <= 0 || C <= 0) return PM_EINVAL;
  if (N > 65535 || T > (1 << 20) || C > (1 << 20)) return PM_EUNSUPPORTED;
  if (N == 0) return PM_OK;
  const dim3 grid((unsigned)((C + 255) / 256), (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
#define PM_LM(TX, TY) \
  hipLaunchKernelGGL((ln_mean_kernel<TX, TY>), grid, dim3(256), 0, st, (const TX*)x, stats, gamma, beta, (TY*)y, (int)T, (int)C)
  if (x_dtype == PM_BF16 && y_dtype == PM_BF16) PM_LM(bf16, bf16);
  else if (x_dtype == PM_BF16 && y_dtype == PM_F32) PM_LM(bf16, float);
  else if (x_dtype == PM_F32 && y_dtype == PM_F32) PM_LM(float, float);
  else if (x_dtype == PM_F32 && y_dtype == PM_BF16) PM_LM(float, bf16);
  else return PM_EINVAL;
#undef PM_LM
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_transpose_add_f32(const float* x, const float* resid, float* y, int64_t ldy, int64_t N, int64_t R, int64_t Cc,
                                    void* stream) {
  if (!x || !y || N < 0 || R <= 0 || Cc <= 0 || ldy < R) return PM_EINVAL;
  if (N > 65535 || R > (1 << 20) || Cc > (1 << 20)) return PM_EUNSUPPORTED;
  if (N == 0) return PM_OK;
  const dim3 grid((unsigned)((Cc + 31) / 32), (unsigned)((R + 31) / 32), (unsigned)N);
  hipLaunchKernelGGL(transpose_add_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, resid, y, (int)R, (int)Cc, ldy);
  PM_CHECK_LAUNCH();
  return PM_OK;
}
