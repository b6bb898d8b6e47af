// prefill.hip - pm_prefill_attention_bf16: causal attention of a CHUNK of prompt positions over the decode step's K/V caches,
// with the chunk's own keys and values appended to them (the prompt pass of audio2text/generate.py; head dim 64, bf16 MFMA).
//
// The chunk is C consecutive positions p0 .. p0 + C - 1 of every sequence.  Row b * C + i of qkv is [q | k | v] (3 * H * 64 wide)
// of position p0 + i; the caches are addressed base + b * stride_b + h * stride_h + key * stride_k as in pm_dec_attention.
//   kc / vc[b, h, p0 + i, :] = the row's k_h / v_h, bit for bit (they are bf16 already: the step's append rounds at the same point);
//   out[b * C + i, h * 64 ..] = softmax_{j <= p0 + i}(q . K_j / 8) V_j - the mask is aligned to ABSOLUTE positions, not top-left.
//
// Cache hazard rule: NO workgroup reads from the caches a row that a workgroup of the same launch writes.  Keys j < p0 (older
// chunks, the caches as they were before the launch) are read from the caches; keys j >= p0 are read from the qkv rows, never from
// the caches.  The append itself is a plain copy: the workgroup of query tile t copies the k / v of ITS 64 rows.  So the launch
// needs no ordering between workgroups, no atomics and no fences, and no cache byte outside [p0, p0 + C) is written.
//
// Workgroup = 4 waves = 64 queries of one (sequence, head); wave w owns queries 16 w .. 16 w + 15 and walks the keys 0 .. p0 + (its
// tile's last query) in tiles of 64.  The tiling is attention_hd32.hip's with two k steps per score block and four output blocks:
//   S^T = K Q^T : MFMA 16x16x32, the 64 head dims in two steps.  A = 16 key rows, B = the wave's 16 query rows, 16-byte fragments
//                 read straight from global.  The accumulator of key block kb has the QUERY on the lane (l & 15) and keys
//                 16 kb + 4 (l >> 4) + i.
//   softmax     : online, fp32, log2 domain; key > p0 + query is -inf.  Key 0 is visible to every query and lies in the first tile,
//                 so the running maximum is finite from the first tile on and a later, fully masked tile contributes p = 0.  The
//                 row sum accumulates the unrounded fp32 p, the matrix product takes p rounded to bf16 (tests/attn_cases.py).
//   O^T += V^T P^T : the S^T accumulators of key blocks (2c, 2c + 1), converted to bf16, are the B operand of k-chunk c.  V^T comes
//                 from LDS: the workgroup writes the V tile transposed (dim-major rows of 64 keys, padded to 68), rows of keys
//                 past the workgroup's last key as zeros (0 x NaN is NaN); a fragment is two 8-byte LDS reads.
// The next tile's K fragments and V chunks are requested before the current tile's arithmetic; the V tile in LDS is
// double-buffered, one barrier per tile.  A wave skips the arithmetic of a tile that lies wholly behind its mask (wave-uniform).
// Query tiles are issued last-first: the last tile of a chunk walks the most keys.
#include "common.h"

namespace {

constexpr int PF_WAVES = 4;
constexpr int PF_QB = 16 * PF_WAVES;  // queries per workgroup
constexpr int PF_KT = 64;             // keys per tile
constexpr int PF_VLD = 68;            // bf16 per dim row of the transposed V tile (64 keys + 4: 8-byte aligned, skews banks)

// RAGGED (pm_prefill_attention_ragged_bf16): sequence b's keys below key_start[b] are padding.  The query at position p keeps
// the keys lo(p) <= j <= p, lo(p) = min(key_start[b], p): a padded query (p < key_start[b]) sees itself only, so "key p is visible
// to query p" takes the place of "key 0 is visible to every query".  lo() does not decrease with p, so a wave's lowest lo is its
// first query's and the workgroup's its first row's: the walk starts at the tile that holds the workgroup's lowest lo, and a wave
// skips the tiles wholly below its own (wave-uniform, like the tiles behind the causal mask).  A query whose lo lies in a later
// tile than its wave's first meets fully masked tiles BEFORE its first visible key: its running maximum is still -inf there, and
// the exponentials are then taken against 0 instead (p = 0, alpha = 0, nothing accumulated).  The append is the plain kernel's.
template <bool RAGGED>
__global__ __launch_bounds__(64 * PF_WAVES) void prefill_attention_kernel(
    const bf16* __restrict__ QKV, int64_t ld, bf16* KC, bf16* VC, int64_t sb, int64_t sh, int64_t sk, bf16* __restrict__ O,
    int64_t ldo, int H, int C, int p0, float scale_log2, const int* __restrict__ key_start) {
  __shared__ __attribute__((aligned(16))) bf16 vt[2][64 * PF_VLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int i0 = ((int)gridDim.x - 1 - (int)blockIdx.x) * PF_QB;  // first chunk row of this workgroup
  const int q0 = i0 + wave * 16;
  const int inner = H * 64;
  const bf16* Qb = QKV + (int64_t)b * C * ld + h * 64;  // q of chunk row i: Qb + i * ld; k: + inner; v: + 2 * inner
  const bf16* Kq = Qb + inner;
  const bf16* Vq = Qb + 2 * inner;
  bf16* Kc = KC + (int64_t)b * sb + (int64_t)h * sh;
  bf16* Vc = VC + (int64_t)b * sb + (int64_t)h * sh;

  // append: the k / v of this workgroup's rows go to the caches (16-byte copies; 64 rows x 8 chunks x {k, v} = 4 per thread)
  {
    const int row = i0 + (tid >> 2);
    if (row < C) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int ch = (tid & 3) + 4 * e;
        *(bf16x8*)(Kc + (int64_t)(p0 + row) * sk + ch * 8) = *(const bf16x8*)(Kq + (int64_t)row * ld + ch * 8);
        *(bf16x8*)(Vc + (int64_t)(p0 + row) * sk + ch * 8) = *(const bf16x8*)(Vq + (int64_t)row * ld + ch * 8);
      }
    }
  }

  // the wave's query fragments: chunk row q0 + i16 (clamped: rows >= C are computed like the last row and never stored)
  const int qi = q0 + i16;
  const int qic = qi < C ? qi : C - 1;
  bf16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const bf16x8*)(Qb + (int64_t)qic * ld + 32 * ks + g * 8);
  const int qpos = p0 + qic;  // the last key this lane's query sees
  const int wave_last = p0 + (q0 + 15 < C ? q0 + 15 : C - 1);  // the last key any query of the wave sees (q0 >= C: the last row's)
  int qlo = 0, wave_lo = 0, t0 = 0;  // the first key this lane's query sees, the lowest of the wave's, the workgroup's first tile
  if constexpr (RAGGED) {
    int ks = key_start[b];
    ks = ks < 0 ? 0 : ks;
    qlo = ks < qpos ? ks : qpos;
    const int wfirst = p0 + (q0 < C ? q0 : C - 1);
    wave_lo = ks < wfirst ? ks : wfirst;
    t0 = (ks < p0 + i0 ? ks : p0 + i0) / PF_KT;
  }

  const int nkeys = p0 + (i0 + PF_QB < C ? i0 + PF_QB : C);  // keys 0 .. nkeys - 1 are visible to some query of the workgroup
  const int ntiles = (nkeys + PF_KT - 1) / PF_KT;
  // keys < p0 live in the caches, keys >= p0 in the chunk's own rows
  auto k_row = [&](int key) -> const bf16* { return key < p0 ? Kc + (int64_t)key * sk : Kq + (int64_t)(key - p0) * ld; };
  auto v_row = [&](int key) -> const bf16* { return key < p0 ? Vc + (int64_t)key * sk : Vq + (int64_t)(key - p0) * ld; };
  // V chunks of this thread: key tid >> 2 of the tile, dims 8 (tid & 3) .. + 7 and 32 + 8 (tid & 3) .. + 7
  const int vkey = tid >> 2, vch = tid & 3;
  bf16x8 kf[4][2], vreg[2];
  auto load_tile = [&](int t) {
    const int k0 = t * PF_KT;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      int key = k0 + 16 * kb + i16;
      key = key < nkeys ? key : nkeys - 1;  // clamped rows score -inf below
      const bf16* kr = k_row(key);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kb][ks] = *(const bf16x8*)(kr + 32 * ks + g * 8);
    }
    const int key = k0 + vkey;
    if (key < nkeys) {
      const bf16* vr = v_row(key);
#pragma unroll
      for (int e = 0; e < 2; ++e) vreg[e] = *(const bf16x8*)(vr + 32 * e + vch * 8);
    } else {
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int j = 0; j < 8; ++j) vreg[e][j] = (bf16)0.f;
    }
  };
  auto store_v = [&](int buf) {
    bf16* d = vt[buf] + vkey;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < 8; ++j) d[(32 * e + vch * 8 + j) * PF_VLD] = vreg[e][j];
  };

  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  load_tile(t0);
  store_v(t0 & 1);
  for (int t = t0; t < ntiles; ++t) {
    const int buf = t & 1;
    bf16x8 kc[4][2];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kc[kb][ks] = kf[kb][ks];
    __syncthreads();  // tile t's V is in vt[buf]; everyone is done reading vt[buf ^ 1] (tile t - 1)
    if (t + 1 < ntiles) load_tile(t + 1);

    const int k0 = t * PF_KT;
    if (k0 <= wave_last && (!RAGGED || k0 + PF_KT > wave_lo)) {  // wave-uniform: a tile wholly behind the wave's mask adds nothing
      f32x4 s[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[kb][0], qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[kb][1], qf[1], s[kb], 0, 0, 0);
      }
      float m = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = s[kb][i] * scale_log2;
          if (k0 + 16 * kb + 4 * g + i > qpos) v = -INFINITY;  // causal on absolute positions (covers keys >= nkeys too)
          if constexpr (RAGGED)
            if (k0 + 16 * kb + 4 * g + i < qlo) v = -INFINITY;  // the sequence's padding
          s[kb][i] = v;
          m = fmaxf(m, v);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      const float m_new = fmaxf(m_run, m);  // plain: finite, key 0 is in tile 0 and visible to every query
      // ragged: -inf until the tile of the query's first visible key - exponentials against 0 there (all of them exp2(-inf) = 0)
      const float m_ref = (RAGGED && m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = exp2f(m_run - m_ref);  // first tile: exp2(-inf) = 0
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = exp2f(s[kb][i] - m_ref);
          s[kb][i] = p;
          sum += p;
        }
      }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
      bf16x8 pf[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pf[c][j] = (bf16)s[2 * c][j];
          pf[c][4 + j] = (bf16)s[2 * c + 1][j];
        }
      }
      const bf16* vb = vt[buf];
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[db][i] *= alpha;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const bf16* row = vb + (16 * db + i16) * PF_VLD + 32 * c + 4 * g;
          const bf16x4 lo = *(const bf16x4*)row, hi = *(const bf16x4*)(row + 16);
          const bf16x8 va = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pf[c], o[db], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntiles) store_v(buf ^ 1);  // vt[buf ^ 1] was last read in iteration t - 1, before this iteration's barrier
  }
  if (qi < C) {
    const float inv = 1.0f / l_run;
    bf16* orow = O + ((int64_t)b * C + qi) * ldo + h * 64 + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db)
      *(bf16x4*)(orow + 16 * db) = bf16x4{(bf16)(o[db][0] * inv), (bf16)(o[db][1] * inv), (bf16)(o[db][2] * inv), (bf16)(o[db][3] * inv)};
  }
}

bool pf_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

template <bool RAGGED>
static int prefill_attention_impl(const void* qkv, int64_t ld_qkv, void* kc, void* vc, int64_t stride_b, int64_t stride_h,
                                  int64_t stride_k, void* out, int64_t ld_out, int64_t B, int64_t H, int64_t C, int64_t p0,
                                  int64_t lk_max, const int32_t* key_start, void* stream) {
  // every refusal is PM_EINVAL and comes before any HIP call
  if (!qkv || !kc || !vc || !out || B < 0 || H < 1 || C < 1 || p0 < 0) return PM_EINVAL;
  if (lk_max > 4096 || p0 + C > lk_max || H > 4096 || B * H > 65535) return PM_EINVAL;
  if (ld_qkv < 3 * H * 64 || ld_out < H * 64 || stride_k < 64 || stride_h < 0 || stride_b < 0) return PM_EINVAL;
  if (ld_qkv % 8 || stride_b % 8 || stride_h % 8 || stride_k % 8 || ld_out % 4) return PM_EINVAL;  // 16-byte fragment loads and
  if (!pf_aligned(qkv, 16) || !pf_aligned(kc, 16) || !pf_aligned(vc, 16) || !pf_aligned(out, 8)) return PM_EINVAL;  // copies, 8-byte stores
  if (B == 0) return PM_OK;
  const float scale_log2 = 0.125f * 1.4426950408889634f;  // 1 / sqrt(64) * log2(e)
  const dim3 grid((unsigned)((C + PF_QB - 1) / PF_QB), (unsigned)(B * H));
  hipLaunchKernelGGL(prefill_attention_kernel<RAGGED>, grid, dim3(64 * PF_WAVES), 0, (hipStream_t)stream, (const bf16*)qkv, ld_qkv,
                     (bf16*)kc, (bf16*)vc, stride_b, stride_h, stride_k, (bf16*)out, ld_out, (int)H, (int)C, (int)p0, scale_log2,
                     (const int*)key_start);
  PM_CHECK_LAUNCH();
  return PM_OK;
}

extern "C" int pm_prefill_attention_bf16(const void* qkv, int64_t ld_qkv, void* kc, void* vc, int64_t stride_b, int64_t stride_h,
                                         int64_t stride_k, void* out, int64_t ld_out, int64_t B, int64_t H, int64_t C, int64_t p0,
                                         int64_t lk_max, void* stream) {
  return prefill_attention_impl<false>(qkv, ld_qkv, kc, vc, stride_b, stride_h, stride_k, out, ld_out, B, H, C, p0, lk_max, nullptr,
                                       stream);
}

/* pm_prefill_attention_bf16 for sequences right-aligned in the caches: sequence b's keys below key_start[b] (int32, B of them, on
 * the device) are padding - see prefill_attention_kernel<true>.  key_start all zero is pm_prefill_attention_bf16 bit for bit. */
extern "C" int pm_prefill_attention_ragged_bf16(const void* qkv, int64_t ld_qkv, void* kc, void* vc, int64_t stride_b,
                                                int64_t stride_h, int64_t stride_k, void* out, int64_t ld_out, int64_t B,
                                                int64_t H, int64_t C, int64_t p0, int64_t lk_max, const int32_t* key_start,
                                                void* stream) {
  if (!key_start) return PM_EINVAL;
  return prefill_attention_impl<true>(qkv, ld_qkv, kc, vc, stride_b, stride_h, stride_k, out, ld_out, B, H, C, p0, lk_max, key_start,
                                      stream);
}
