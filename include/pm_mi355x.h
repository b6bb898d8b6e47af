/* pm_mi355x.h - C ABI of libpm_mi355x.so: the MI355X (gfx950) kernels underneath the
 * pytorch_models hot path (shared transformer forward, ViT patch-embed, Whisper front end,
 * encoder and KV-cached decoder).
 *
 * The reference (gau-nernst/pytorch-models) has no FFI: its boundary is its Python class API
 * (SURVEY.md section 8(b)).  Each entry point below replaces the stock-PyTorch primitive named in
 * its comment (reference file:line) and is what the reference-side binding in INTEGRATION.md
 * (a ctypes stub) would bind.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked host;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); no call synchronises,
 *    allocates or frees device memory; workspaces are caller-owned;
 *  - leading dimensions (ld*) are in ELEMENTS of the tensor's dtype;
 *  - return value: 0 = OK, otherwise a PM_E* code (pm_strerror gives text).  Arguments are
 *    validated on the host before any launch; a rejected call launches nothing;
 *  - dtypes: PM_BF16 / PM_F32 below;
 *  - data pointers must be non-null even when an extent is 0 (the null check comes first and returns PM_EINVAL); the wrappers of
 *    pytorch_models/_hip/ops.py never call the library with an empty operand: they return the empty result themselves.
 */
#ifndef PM_MI355X_H
#define PM_MI355X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PM_ABI_VERSION 1

enum { PM_OK = 0, PM_EINVAL = 1, PM_EUNSUPPORTED = 2, PM_ELAUNCH = 3, PM_EALIGN = 4 };
enum { PM_BF16 = 0, PM_F32 = 1 };
/* activation table of MLP - pytorch_models/transformer.py:60-65 */
enum { PM_ACT_NONE = 0, PM_ACT_GELU = 1, PM_ACT_GELU_TANH = 2, PM_ACT_RELU = 3, PM_ACT_SILU = 4 };

int pm_abi_version(void);
const char* pm_strerror(int code);

/* nn.Linear (+ fused activation / residual): y[M,N] = act(x[M,K] w[N,K]^T + bias[N]) + resid[M,N]
 * Replaces the four nn.Linear of MHA (transformer.py:28-31,47-49,53), MLP's linear1 -> act ->
 * linear2 (transformer.py:59-66) and the residual adds of Encoder/DecoderLayer (transformer.py:98-100,
 * 124-125).  x, w: bf16, K-contiguous; bias: f32 or NULL; resid: resid_dtype or NULL; y: y_dtype.
 * Requires K % 64 == 0 and 16-byte aligned x / w rows (ld % 8 == 0).  N, ldy, ldr multiples of 4 take the
 * vector epilogue; ragged N (a 51865-row vocabulary: the tied-embedding logits of whisper.py:52) stores element-wise.
 * Aliasing (all pm_linear_bf16* entry points): resid may alias y as the very same matrix (resid == y, ldr == ldy, resid_dtype ==
 * y_dtype, no resid_period): every kernel loads a residual element in the workgroup that stores that element, before the store.
 * y must not alias x, w, bias, ln_stats, ln_s or ws, and must not overlap resid in any other way. */
int pm_linear_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                   const void* resid, int64_t ldr, int resid_dtype, void* y, int64_t ldy, int y_dtype,
                   int64_t M, int64_t N, int64_t K, int act, void* stream);

/* pm_linear_bf16 with two extra addressing features (everything else identical):
 *  - x rows in two levels: row m lives at x + (m / x_rows_per_batch) * x_batch_stride + (m % x_rows_per_batch) * ldx
 *    (x_rows_per_batch == 0: plain m * ldx).  With ldx = 2*d and K = 3*d over a zero-padded time-major buffer this
 *    IS Conv1d(d, d, 3, stride 2, padding 1) (whisper.py:19): each output row reads 3 consecutive input rows;
 *  - resid rows repeat every resid_period rows (0: no repeat), e.g. "+ pos_embs[:L]" broadcast over the batch
 *    (whisper.py:31).  Order: y = act(x w^T + bias) + resid.  A periodic resid must not alias y: many tiles read each of its rows. */
int pm_linear_bf16_ex(const void* x, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride, const void* w,
                      int64_t ldw, const float* bias, const void* resid, int64_t ldr, int resid_dtype,
                      int64_t resid_period, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act,
                      void* stream);

/* nn.Linear in fp32, for modules whose parameters are fp32 (the reference's default dtype: tests/image/test_vit.py:45 asks
 * 2e-5, tests/audio2text/test_whisper.py:45 5e-5) and for the exact Whisper pipeline: y = act(x w^T + bias) + resid, all
 * operands f32, on the f32-input MFMA (exact fp32 products and accumulation; csrc/linear_f32.hip).  Addressing as
 * pm_linear_bf16_ex (two-level x rows: Conv1d / Conv2d windows as GEMM rows; periodic resid rows: a position table).
 * ldx, ldw multiples of 4, x and w 16-byte aligned; every activation of the table above.  y must not alias x, w, bias or resid. */
int pm_linear_f32(const float* x, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride, const float* w, int64_t ldw,
                  const float* bias, const float* resid, int64_t ldr, int64_t resid_period, float* y, int64_t ldy, int64_t M,
                  int64_t N, int64_t K, int act, void* stream);

/* pm_linear_bf16_ln with a caller-owned workspace: pm_linear_ws_bytes() bytes, 16-byte aligned, its first 4096 bytes zero
 * before the first call and left alone afterwards.  With it the dispatcher may deal a GEMM's K steps out as ONE stream over
 * the persistent workgroups ("stream-K", csrc/linear_bf16_sk.hip) where whole 256 x 256 tiles would leave the last round
 * badly filled (M = 50432: N = 768 is 2.31 rounds, N = 3072 9.23); tiles shared by two workgroups are combined in fp32
 * through the workspace, deterministically.  One workspace serves one stream at a time.  ws == NULL: pm_linear_bf16_ln.
 * With a workspace resid must not alias y (a tile cut along K is finished by a workgroup other than the one that started it). */
int pm_linear_bf16_ws(const void* x, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride, const void* w, int64_t ldw,
                      const float* bias, const void* resid, int64_t ldr, int resid_dtype, int64_t resid_period, void* y,
                      int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, const float* ln_stats,
                      const float* ln_s, float* ln_row_out, void* ws, int64_t ws_bytes, void* stream);
int64_t pm_linear_ws_bytes(void);

/* Host-only query: the kernel a pm_linear_bf16_ws call with these arguments would launch.  1 = 128 x 128, 2 = persistent
 * 256 x 128, 3 = 256 x 256, 4 / 5 = the stream-K / hybrid experiments, 6 / 7 = (64 MI) x 256 tiles of 256 / 320 rows; 0 when
 * M == 0 with non-null pointers (nothing is launched; an empty tensor's null pointer is PM_EINVAL like any other, so ops.linear_plan
 * answers 0 for an empty batch itself and does not ask); minus the error code the call would return.  The launch takes its decision from the same
 * function.  Pointers are looked at for null and alignment only: nothing is dereferenced or launched, no GPU is needed.
 * PM_GEMM_KERNEL (read once per process) forces a kernel where it applies and silently falls through where it does not -
 * this query is how a test learns which one ran. */
int pm_linear_bf16_plan(const void* x, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride, const void* w,
                        int64_t ldw, const float* bias, const void* resid, int64_t ldr, int resid_dtype, int64_t resid_period,
                        const void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act,
                        const float* ln_stats, const float* ln_s, const float* ln_row_out, const void* ws, int64_t ws_bytes);

/* LayerNorm folded into the GEMMs around it (pre-norm blocks, transformer.py:124-125: x + f(LN(x))).
 * pm_linear_bf16_ln = pm_linear_bf16_ex plus
 *  - ln_stats (M, 2) f32 [mean, rstd per input row] and ln_s (N) f32: y = act(rstd*(x w'^T - mean*ln_s) + bias) + resid,
 *    where the caller passes w' = bf16(gamma (.) w), ln_s[n] = sum_k w'[n][k], bias[n] = b[n] + sum_k beta[k] w[n][k];
 *  - ln_row_out (M, N/64, 2) f32: per row and 64-feature block, (sum, sum of squares) of the bf16-rounded outputs -
 *    the partial statistics of the NEXT LayerNorm, reduced by pm_ln_stats_finalize into (mean, rstd).
 * Served by the persistent kernels only: check pm_linear_ln_supported(M, N, K, act, produce) first (1 = yes). */
int pm_linear_bf16_ln(const void* x, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride, const void* w,
                      int64_t ldw, const float* bias, const void* resid, int64_t ldr, int resid_dtype,
                      int64_t resid_period, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act,
                      const float* ln_stats, const float* ln_s, float* ln_row_out, void* stream);
int pm_ln_stats_finalize(const float* row_partials, float* stats, int64_t M, int64_t N, float eps, void* stream);
int pm_linear_ln_supported(int64_t M, int64_t N, int64_t K, int act, int produce);

/* nn.LayerNorm over the last dim (transformer.py:87,90,93; vit.py:69; whisper.py:27,45):
 * y[r,:] = (x[r,:] - mean) * rsqrt(var + eps) * gamma + beta, fp32 statistics, biased variance.
 * x: x_dtype (M, d) with row stride ldx; gamma/beta: f32 (d); y: y_dtype.  d % 8 == 0.  y must not alias x, gamma or beta
 * (pm_layernorm_ex, pm_rmsnorm: nor resid). */
int pm_layernorm(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps,
                 void* y, int64_t ldy, int y_dtype, int64_t M, int64_t d, void* stream);

/* pm_layernorm with the two things the audio encoders put right behind a norm fused in:
 * y = act(LayerNorm(x)) + resid.  gamma and beta both NULL = no affine (LayerNorm1d(elementwise_affine=False),
 * audio/data2vec_audio.py:27); act: PM_ACT_NONE | PM_ACT_GELU (erff; audio/wav2vec2.py:38 norm -> GELU);
 * resid: NULL or resid_dtype (M, d) with row stride ldr. */
int pm_layernorm_ex(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps, int act,
                    const void* resid, int64_t ldr, int resid_dtype, void* y, int64_t ldy, int y_dtype, int64_t M,
                    int64_t d, void* stream);

/* T5's LayerNorm (text/t5.py:15-25): y = x * rsqrt(mean(x^2) + eps) * gamma - no centring, no bias; fp32 statistics. */
int pm_rmsnorm(const void* x, int64_t ldx, int x_dtype, const float* gamma, float eps, void* y, int64_t ldy, int y_dtype,
               int64_t M, int64_t d, void* stream);

/* The gate of GEGLU (text/t5.py:29-38) over a packed projection h = x [w; v]^T, bf16 (M, 2F) with row stride ldh:
 * out[m, f] = gelu_tanh(h[m, f]) * h[m, F + f], bf16 (M, F).  F % 8 == 0. */
int pm_geglu(const void* h, int64_t ldh, void* out, int64_t ldo, int64_t M, int64_t F, void* stream);

/* ---- Wav2Vec2 / Data2VecAudio / SEW (audio/wav2vec2.py, audio/data2vec_audio.py, audio/sew.py).
 * All feature-encoder activations are (clip, time, channel) bf16, so Conv1d(C, C', k, stride s) over them is
 * pm_linear_bf16_ex with row stride s*C and K = k*C (weight K order (tap, channel)).
 *
 * Layer 0 (audio/wav2vec2.py:32-38 with in_dim 1): out[b, t, c] = GELU(norm(bias[c] + sum_j w[c, j] x[b, t*stride + j])),
 * T0 = (L - k) / stride + 1.  x: f32 (B, L); w: f32 (C0, k) = the Conv1d weight as stored; bias: f32 (C0) or NULL;
 * out: bf16 (B, T0, C0).  norm: PM_W2V_NORM_NONE | PM_W2V_NORM_LAYER (LayerNorm1d over channels, gamma / beta f32 (C0)) |
 * PM_W2V_NORM_INSTANCE (InstanceNorm1d(affine) over time per clip and channel: the statistics come from the waveform's
 * 10 x 10 lag products, accumulated in fp64, see csrc/wav2vec2.hip; the caller supplies scratch partials, 8-byte aligned, of
 * pm_w2v_stem0_scratch_floats(B, T0) floats (the kernels keep doubles in it) and stats f32 (B, C0, 2); fixed reduction
 * order).  k == 10, C0 % 8 == 0, C0 <= 512. */
enum { PM_W2V_NORM_NONE = 0, PM_W2V_NORM_LAYER = 1, PM_W2V_NORM_INSTANCE = 2 };
int64_t pm_w2v_stem0_scratch_floats(int64_t B, int64_t T0);
int pm_w2v_stem0(const float* x, const float* w, const float* bias, int norm, const float* gamma, const float* beta, float eps,
                 float* partials, float* stats, void* out, int64_t B, int64_t L, int64_t C0, int64_t k, int64_t stride,
                 void* stream);

/* Regrouping for the grouped positional conv (audio/wav2vec2.py:70-74: ConstantPad1d + Conv1d(d, d, k, groups=G)):
 * out[b, g, pad_left + t, c] = bf16(x[b, t, g*cg + c]), zero in the pad rows and for c in [cg, cgp).  x: x_dtype
 * (B, T, >= G*cg) with row stride ldx; out: bf16 (B, G, pad_left + T + pad_right, cgp), cgp % 8 == 0.  Group g's conv
 * window at step t is then the k*cgp contiguous values at out[b, g, t*stride], i.e. one pm_linear_bf16_ex per group. */
int pm_group_windows(const void* x, int64_t ldx, int x_dtype, void* out, int64_t B, int64_t T, int64_t G, int64_t cg,
                     int64_t cgp, int64_t pad_left, int64_t pad_right, void* stream);

/* Grouped Conv1d over time with few channels per group, fused bias / activation / residual (the positional conv of
 * audio/wav2vec2.py:70-74, audio/data2vec_audio.py:25, audio/sew.py:24), on the buffer pm_group_windows builds:
 *   y[b*To + t, g*cg + n] = act(bias[g*cg + n] + sum_{tap < k, c < cg} xg[b, g, t*stride + tap, c] * w[g, n, tap*cgp + c])
 *                           + resid[b*To + t, g*cg + n],          To = (Tp - k) / stride + 1.
 * xg: bf16 (B, G, Tp, cgp); w: bf16 (G, cg, Kp), K order (tap, channel), zero-padded from k*cgp to Kp (% 64 == 0,
 * < 64 of padding); bias: f32 (G*cg) or NULL; resid: bf16 rows of stride ldr, or NULL; y: bf16 rows of stride ldy;
 * act: PM_ACT_NONE | PM_ACT_GELU.  The distinct input rows of a tile stay resident in LDS (see csrc/grouped_conv.hip).
 * pm_grouped_conv_supported(cg, cgp) == 1 for cg % 4 == 0 and cgp in {8, 16, 32, 48, 64} with cgp - cg < 8. */
int pm_grouped_conv_supported(int64_t cg, int64_t cgp);
int pm_grouped_conv_bf16(const void* xg, const void* w, const float* bias, const void* resid, int64_t ldr, void* y,
                         int64_t ldy, int64_t B, int64_t G, int64_t Tp, int64_t cg, int64_t cgp, int64_t k, int64_t stride,
                         int64_t Kp, int act, void* stream);

/* F.avg_pool1d(x, 2) over time on (B, T, d) bf16 -> (B, T / 2, d) bf16 (audio/sew.py:33; a trailing odd row is dropped). */
int pm_avgpool_time2(const void* x, void* out, int64_t B, int64_t T, int64_t d, void* stream);

/* F.scaled_dot_product_attention (transformer.py:52) for head_dim 64, bf16 operands:
 * o[b,i,h,:] = softmax_j(q[b,i,h,:] . k[b,j,h,:] / 8 [j <= i if causal]) v[b,j,h,:].
 * q/k/v/o are addressed as base + b*stride_b + token*stride_t + h*64 (elements), so the packed
 * (tokens, 3*h*64) output of a fused QKV projection is consumed in place and the result is written
 * already merged as (tokens, h*64) - the unflatten/transpose/flatten of transformer.py:47-53 never
 * materialise.  causal is top-left aligned like torch's is_causal. */
int pm_attention_bf16(const void* q, int64_t q_stride_b, int64_t q_stride_t,
                      const void* k, int64_t k_stride_b, int64_t k_stride_t,
                      const void* v, int64_t v_stride_b, int64_t v_stride_t,
                      void* o, int64_t o_stride_b, int64_t o_stride_t,
                      int64_t B, int64_t H, int64_t Lq, int64_t Lk, int causal, void* stream);

/* pm_attention_bf16 with the additive attn_mask of transformer.py:52 (`attn_bias`: T5 / MaxViT style relative position
 * bias): scores + bias[b, h, i, j] before the softmax.  bias: f32, addressed bias + b*stride_b + h*stride_h + i*stride_q + j
 * (stride 0 = broadcast over batch / heads); -inf entries mask keys.  A query row with no visible key (every bias entry -inf,
 * or left padding under causal) yields ZEROS, as F.scaled_dot_product_attention does on the CPU - never NaN, and never an
 * average over hidden keys.  The same holds for pm_attention_generic_* and pm_window_attention_bf16. */
int pm_attention_bias_bf16(const void* q, int64_t q_stride_b, int64_t q_stride_t,
                           const void* k, int64_t k_stride_b, int64_t k_stride_t,
                           const void* v, int64_t v_stride_b, int64_t v_stride_t,
                           void* o, int64_t o_stride_b, int64_t o_stride_t,
                           int64_t B, int64_t H, int64_t Lq, int64_t Lk, int causal, const float* bias,
                           int64_t bias_stride_b, int64_t bias_stride_h, int64_t bias_stride_q, void* stream);

/* Small 2-D convolution on NHWC bf16 (reference: conv_norm_act / MBConv / MobileViTBlock, pytorch_models/image/mobile_vit.py:10-69:
 * nn.Conv2d(bias=False) + eval-mode nn.BatchNorm2d [+ nn.SiLU], the norm folded into w and bias by the caller).
 * x: bf16 (N, H, W, Cin); w: bf16 (Cout, kh, kw, Cin / groups); bias: f32 (Cout) or NULL; resid: bf16 like y or NULL (added
 * after the activation); y: bf16 (N, Ho, Wo, Cout), Ho = (H + 2 pad - kh) / stride + 1.  groups divides Cin and Cout (1 = dense,
 * Cin = depthwise).  act: PM_ACT_NONE | PM_ACT_SILU | PM_ACT_RELU.  Direct convolution, fp32 accumulation; off the benchmark path. */
int pm_conv2d_nhwc_bf16(const void* x, int64_t N, int64_t H, int64_t W, int64_t Cin, const void* w, const float* bias,
                        const void* resid, void* y, int64_t Cout, int64_t kh, int64_t kw, int64_t stride, int64_t pad,
                        int64_t groups, int act, void* stream);

/* y[n, c] = mean over r of x[n, r, c]: nn.AdaptiveAvgPool2d(1) + Flatten on NHWC rows (mobile_vit.py:100).  bf16 in / out. */
int pm_mean_rows_bf16(const void* x, void* y, int64_t N, int64_t HW, int64_t C, void* stream);

/* Attention for head dims other than 64 (% 4 == 0 up to 128, % 2 == 0 up to 64; e.g. ViT-H's 80, MobileViT's 16 .. 60): same addressing with h*head_dim head
 * offsets, optional additive bias (NULL = none), Lk <= 2048.  fp32 VALU, correctness-first, off the benchmark path. */
int pm_attention_generic_bf16(const void* q, int64_t q_stride_b, int64_t q_stride_t,
                              const void* k, int64_t k_stride_b, int64_t k_stride_t,
                              const void* v, int64_t v_stride_b, int64_t v_stride_t,
                              void* o, int64_t o_stride_b, int64_t o_stride_t,
                              int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t head_dim, int causal,
                              const float* bias, int64_t bias_stride_b, int64_t bias_stride_h, int64_t bias_stride_q,
                              void* stream);

/* pm_attention_generic_bf16 on fp32 operands (strides in elements, multiples of 4; o 16-byte aligned): the attention of
 * fp32 modules and of the exact Whisper pipeline - fp32 in, fp32 arithmetic, fp32 out. */
int pm_attention_generic_f32(const float* q, int64_t q_stride_b, int64_t q_stride_t, const float* k, int64_t k_stride_b,
                             int64_t k_stride_t, const float* v, int64_t v_stride_b, int64_t v_stride_t, float* o,
                             int64_t o_stride_b, int64_t o_stride_t, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                             int64_t head_dim, int causal, const float* bias, int64_t bias_stride_b, int64_t bias_stride_h,
                             int64_t bias_stride_q, void* stream);

/* ViT token assembly (vit.py:78-81): Conv2d(3, d, P, stride P) on fp32 NCHW images, flatten,
 * transpose, + pe, prepend cls - im2col-free.  imgs: f32 (N,3,Himg,Wimg); w: bf16 (d, 3*P*P)
 * (the Conv2d weight viewed 2-D); bias: f32 (d); pe: f32 (L, d); cls: f32 (d) or NULL;
 * out: bf16 (N, L + (cls != NULL), d) contiguous.  The cls row is broadcast over the batch
 * (SURVEY.md F1).  Requires P % 2 == 0... see pm_strerror for the exact supported set. */
int pm_vit_tokens(const float* imgs, const void* w, const float* bias, const float* pe, const float* cls,
                  void* out, int64_t N, int64_t Himg, int64_t Wimg, int64_t P, int64_t d, void* stream);

/* pm_vit_tokens for any patch size P <= 64 (14: DINOv2; 32; 8): w is bf16 (d, ldw) with the 3*P*P real columns
 * followed by zeros up to ldw >= ceil(3*P*P / 64) * 64.  Scalar gather; not on the benchmark path. */
int pm_vit_tokens_generic(const float* imgs, const void* w, int64_t ldw, const float* bias, const float* pe,
                          const float* cls, void* out, int64_t N, int64_t Himg, int64_t Wimg, int64_t P, int64_t d,
                          void* stream);

/* torch.stft(n_fft, hop, hann window, center=True, reflect, onesided).abs().square() (spectrogram.py:16),
 * optionally followed by the mel filterbank (spectrogram.py:45) and Whisper's log10 (whisper.py:144-145).
 * x: f32, clip b at x + b * x_stride, T samples.  tw_cos / tw_sin: f32 twiddle tables with the window folded in,
 * laid out [ceil(nbins / 32)][n_fft / 2][64]: entry (blk, s, lane) = w[k] * cos|sin(2 pi k bin / n_fft) with
 * k = 2 s + (lane >> 5), bin = 32 blk + (lane & 31) (0 for bin >= nbins).  n_frames <= 1 + T / hop frames are
 * produced (Whisper drops the last one).  mode 0: out (B, n_fft/2+1, n_frames) power; mode 1: out
 * (B, n_mels, n_frames) mel power, the filterbank given in CSR form (mel_ptr[n_mels+1], mel_col, mel_val);
 * mode 2: log10 of mode 1 and peak[b] = order-preserving int encoding of the per-clip maximum (for
 * pm_logmel_finalize).  n_fft, hop even; T > n_fft / 2. */
int pm_stft_mel(const float* x, int64_t x_stride, int64_t B, int64_t T, const float* tw_cos, const float* tw_sin,
                int64_t n_fft, int64_t hop, int64_t n_frames, int mode, const int32_t* mel_ptr, const int32_t* mel_col,
                const float* mel_val, int64_t n_mels, float* out, int32_t* peak, void* stream);

/* pm_stft_mel for a SYMMETRIC window (w[k] == w[n_fft - k], k = 1 .. n_fft - 1: every Hann / Hamming ...): the frame is folded
 * about n_fft / 2 - cosine terms on x[k] + x[n_fft - k], sine terms on x[k] - x[n_fft - k] - which halves the contraction.
 * Tables laid out [ceil(nbins / 32)][S][64] with S = (n_fft / 2 + 2) / 2 and k = 2 s + (lane >> 5): cosine entries for
 * k = 0 .. n_fft / 2 (the k = n_fft / 2 entry HALVED, it meets its own mirror), sine entries for k = 1 .. n_fft / 2 - 1, zero
 * elsewhere.  Everything else as pm_stft_mel. */
int pm_stft_mel_folded(const float* x, int64_t x_stride, int64_t B, int64_t T, const float* tw_cos, const float* tw_sin,
                       int64_t n_fft, int64_t hop, int64_t n_frames, int mode, const int32_t* mel_ptr, const int32_t* mel_col,
                       const float* mel_val, int64_t n_mels, float* out, int32_t* peak, void* stream);

/* whisper.py:146-147 in place: out = (max(out, per-clip max - 8) + 4) / 4; per_clip = n_mels * n_frames (% 4 == 0). */
int pm_logmel_finalize(float* out, const int32_t* peak, int64_t B, int64_t per_clip, void* stream);

/* First stem conv of WhisperEncoder (whisper.py:17-18): Conv1d(C, d, 3, 1, 1) + GELU on channel-major f32
 * x (B, C, T), written time-major bf16 as out (B, T + 2, d) with zero rows 0 and T + 1 (the padding the second,
 * stride-2 conv needs: see pm_linear_bf16_ex).  w: bf16 (d, 3 * Cpad), K order (tap, channel), channels
 * zero-padded to Cpad (% 64 == 0); bias f32 (d). */
int pm_whisper_stem1(const float* x, const void* w, const float* bias, void* out, int64_t B, int64_t C, int64_t Cpad,
                     int64_t T, int64_t d, void* stream);

/* nn.Embedding + positional add (whisper.py:48-49): out[b, l, :] = emb[tokens[b, l], :] + pos[pos0 + l, :].
 * tokens: int64 (B, L); emb: bf16 (V, d); pos: f32 (>= pos0 + L, d) or NULL (no absolute positions: text/t5.py:145);
 * out: bf16 | f32 (B, L, d). */
int pm_embed_tokens(const int64_t* tokens, const void* emb, const float* pos, void* out, int out_dtype, int64_t B,
                    int64_t L, int64_t pos0, int64_t d, int64_t V, void* stream);
/* the same from an fp32 table into fp32 rows (modules whose parameters are fp32) */
int pm_embed_tokens_f32(const int64_t* tokens, const float* emb, const float* pos, float* out, int64_t B, int64_t L,
                        int64_t pos0, int64_t d, int64_t V, void* stream);

/* ---- KV-cached greedy decode step (no reference counterpart: README.md:86 lists Whisper decoding as TODO; the
 * semantics follow pytorch_models/text/generator.py:23-35 over transformer.py:96-100 and whisper.py:47-53).
 * All activations f32, weights / caches bf16.  `pos_ptr` points at ONE device int: the position t of the token being
 * consumed; every kernel of a step reads it, pm_dec_advance increments it, so one captured graph replays all steps. */

/* x[b, :] = emb[tok_cur[b], :] + pos[t, :]  (whisper.py:48-49 for one position). */
int pm_dec_embed(const int64_t* tok_cur, const void* emb, const float* pos, const int32_t* pos_ptr, float* x, int64_t B,
                 int64_t d, int64_t V, void* stream);

/* y = act([LayerNorm_{gamma,beta,eps}](x) w^T + bias) [+ resid] for M <= 64 rows of f32 x; w bf16 (N, K).
 * gamma == NULL: no LayerNorm.  mode 0: out f32 (M, N) (+ resid f32, may alias out);
 * mode 1 (N = 3*inner, [q|k|v] blocks): q -> out f32 (M, inner); k, v -> bf16 caches (M, H, Tmax, 64) at position t;
 * mode 2: no store - per row, the tile's (max logit, lowest index) go to ws_val / ws_idx (M, ceil(N / tile)),
 *         tile = pm_dec_argmax_tile(K) features.  With LayerNorm: K <= 1280.
 * act: PM_ACT_NONE | PM_ACT_GELU (erff) | PM_ACT_GELU_TANH (tanhf).  K % 32 == 0. */
int pm_dec_linear(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, const void* w,
                  int64_t ldw, const float* bias, const float* resid, int64_t ldr, float* out, int64_t ldo, int64_t M,
                  int64_t N, int64_t K, int act, int mode, void* kcache, void* vcache, int64_t inner, int64_t H,
                  int64_t Tmax, const int32_t* pos_ptr, float* ws_val, int32_t* ws_idx, void* stream);

/* Features per argmax tile of pm_dec_linear mode 2 for a given K (64, or 32 when K > 512). */
int pm_dec_argmax_tile(int64_t K);

/* Host-only query: the kernel instantiation and grid that pm_dec_linear (k_split = 0; mode 0, 1, 2), pm_dec_linear_ksplit (mode 0,
 * k_split >= 2) or pm_dec_linear_kparts (mode 3, k_split >= 2) launches for these shapes, has_ln = gamma != NULL.  The launchers
 * take their decision from the same function, PM_DEC_ROWSPLIT / PM_DEC_LOGITS_PERSIST / PM_DEC_LOGITS_WAVES included (the CU count
 * is the current device's, 256 without one).  report: 10 int32 = kernel (0 dec_linear_kernel, 1 the persistent dec_logits_kernel),
 * MT (16-row tiles per workgroup), FT (16-feature tiles per workgroup and inner step), NSTEP (K steps of 32 a wave holds in
 * registers), LN, waves per workgroup, gridDim.x, gridDim.y (K parts), gridDim.z (row tiles on their own workgroups), the number of
 * feature / arg-max tiles.  Returns the launcher's shape refusal (PM_EINVAL / PM_EUNSUPPORTED) where it has one.  Nothing is
 * dereferenced or launched. */
int pm_dec_linear_plan(int64_t M, int64_t N, int64_t K, int has_ln, int mode, int64_t k_split, int32_t* report);

/* One query per (sequence, head), head_dim 64: out = softmax(q K^T / 8) V (transformer.py:52 with L_q = 1 and NO
 * causal flag - SURVEY.md F3).  q / out f32 (B, H*64); K/V bf16 addressed base + b*stride_b + h*stride_h + key*stride_k;
 * number of keys = (lk_ptr ? *lk_ptr : 0) + lk_add  (self: pos + 1; cross: the constant 1500), <= lk_max <= 4096. */
int pm_dec_attention(const float* q, const void* kc, const void* vc, int64_t stride_b, int64_t stride_h, int64_t stride_k,
                     const int32_t* lk_ptr, int64_t lk_add, int64_t lk_max, float* out, int64_t B, int64_t H, void* stream);

/* The prompt pass of the KV-cached decoders: causal attention of a chunk of C consecutive positions p0 .. p0 + C - 1 over the
 * step's caches, with the chunk's keys and values appended (csrc/prefill.hip; head_dim 64).  qkv: bf16, row b*C + i =
 * [q | k | v] of position p0 + i (3*H*64 wide, leading dimension ld_qkv); kc / vc: the bf16 caches, addressed as in
 * pm_dec_attention; out: bf16 (B*C, H*64), heads merged.  For every b, h, i < C:
 *   kc / vc[b,h,p0+i,:] = the row's k_h / v_h, bit for bit;
 *   out[b,i,h,:] = softmax_{j <= p0+i}(q . K_j / 8) V_j, K_j / V_j = the caches as they were for j < p0, the chunk's rows after.
 * The mask is aligned to absolute positions (pm_attention_bf16's is top-left aligned).  No cache byte outside [p0, p0 + C) is
 * written, and no workgroup reads a cache row that the launch writes.  p0 is a host integer: this runs outside the captured
 * step.  PM_EINVAL before any HIP call for: a null pointer, C < 1, p0 < 0, p0 + C > lk_max, lk_max > 4096, ld_qkv < 3*H*64,
 * ld_out < H*64, stride_k < 64, B*H > 65535, ld_qkv / strides not multiples of 8, ld_out not of 4, qkv / kc / vc not
 * 16-byte aligned, out not 8-byte aligned. */
int pm_prefill_attention_bf16(const void* qkv, int64_t ld_qkv, void* kc, void* vc, int64_t stride_b, int64_t stride_h,
                              int64_t stride_k, void* out, int64_t ld_out, int64_t B, int64_t H, int64_t C, int64_t p0,
                              int64_t lk_max, void* stream);

/* pm_dec_linear, plain mode without LayerNorm, with K split over k_split (2..8) workgroups per 16-feature tile: each
 * part reads 1 / k_split of x (at M = 32, K = 2048 every workgroup of the unsplit kernel pulls all 256 KB of x through
 * one CU's L2 path) and of its weight rows; the last part to finish - an agent-scope ticket, no spinning - adds the
 * parts in part order (deterministic) and applies bias / activation / residual.  split_ws: ceil(N / 16) * k_split *
 * mt * 256 floats with mt = ceil(M / 16) rounded up to 1, 2 or 4, 16-byte aligned; split_cnt: ceil(N / 16) * 4 int32 (one ticket per feature tile and
 * row tile), zero before the first launch, zero again after every launch (graph replay).  K / 32 >= k_split. */
int pm_dec_linear_ksplit(const float* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, const float* resid,
                         int64_t ldr, float* out, int64_t ldo, int64_t M, int64_t N, int64_t K, int act, int64_t k_split,
                         float* split_ws, int32_t* split_cnt, void* stream);

/* Fused attention block of the decode step, one launch: LayerNorm(x[b]) -> per-head projection -> attention.
 * self_attn != 0: w = packed [q|k|v] bf16 (3*H*64, d), bias f32 (3*H*64) or NULL; k_h, v_h are rounded to bf16,
 *   appended to the caches kc / vc at position t = *pos_ptr and attended together with the t older keys;
 * self_attn == 0: w = q projection bf16 (H*64, d); kc / vc = the projected cross K / V, lk_const keys.
 * K/V addressing and q/out layout as pm_dec_attention.  d % 64 == 0, d <= 1280.  Replaces pm_dec_linear (mode 0/1)
 * + pm_dec_attention for the same result (same fp32 arithmetic, k/v rounding point unchanged). */
int pm_dec_attention_fused(const float* x, int64_t d, const float* gamma, const float* beta, float eps, const void* w,
                           const float* bias, void* kc, void* vc, int64_t stride_b, int64_t stride_h, int64_t stride_k,
                           const int32_t* pos_ptr, int64_t lk_const, int64_t lk_max, float* out, int64_t B, int64_t H,
                           int self_attn, void* stream);

/* pm_dec_attention_fused with FLOAT K / V caches (kc, vc point to f32, strides in elements): nothing is rounded when a key
 * or value is cached - the reference-accuracy decode of Whisper.generate(exact=True), captured in the same step graph as the
 * bf16-cache path (text/generator.py:23-35 semantics, fp32 throughout).  Same arguments otherwise. */
int pm_dec_attention_fused_kv32(const float* x, int64_t d, const float* gamma, const float* beta, float eps, const void* w,
                                const float* bias, void* kc, void* vc, int64_t stride_b, int64_t stride_h, int64_t stride_k,
                                const int32_t* pos_ptr, int64_t lk_const, int64_t lk_max, float* out, int64_t B, int64_t H,
                                int self_attn, void* stream);

/* pm_dec_attention_fused (kv_f32 = 0) / _kv32 (kv_f32 = 1) as a link of the step's chain of DEFERRED SUMS: two launches per
 * layer and the K-split's ticket leave the chain (transformer.py:50-53 and the residual adds of transformer.py:96-100, same sums).
 *   IN  - the block's input row is  x[b] + x_bias + sum_{p < n_parts} x_parts[p * part_stride + b * part_row_stride + :]  (added in
 *         part order; every (b, h) workgroup forms it itself), and workgroup (b, 0) writes it to x_out (must not alias x) as the
 *         residual stream for what follows.  n_parts = 0: plain x, x_out untouched.  Producers: pm_dec_linear_kparts (fc2 of the
 *         previous layer: part_stride = its part_stride, part_row_stride = ld_parts) and this function's own OUT side
 *         (part_stride = d, part_row_stride = H * d, x_bias = the output projection's bias).
 *   OUT - w_out != NULL (bf16 (d, H*64) row-major): instead of att the block writes the output projection's per-head partial sums
 *         head_parts[(b * H + h) * d + n] = sum_j att[b, h*64 + j] * w_out[n, h*64 + j]  (fp32 FMA chain); `out` is not written.
 *         w_out == NULL: att to `out` as pm_dec_attention_fused.
 * Other arguments as pm_dec_attention_fused. */
int pm_dec_attention_chain(const float* x, int64_t d, const float* gamma, const float* beta, float eps, const void* w,
                           const float* bias, void* kc, void* vc, int64_t stride_b, int64_t stride_h, int64_t stride_k,
                           const int32_t* pos_ptr, int64_t lk_const, int64_t lk_max, int64_t B, int64_t H, int self_attn,
                           int kv_f32, const float* x_parts, int64_t n_parts, int64_t part_stride, int64_t part_row_stride,
                           const float* x_bias, float* x_out, const void* w_out, float* head_parts, float* out, void* stream);

/* pm_dec_linear_ksplit's products WITHOUT the combining pass: part p (K steps [p, p + 1) * K / k_split) of x w^T goes to
 * parts + p * part_stride, row stride ld_parts, as it stands - no bias, no residual, no ticket; the consumer
 * (pm_dec_attention_chain) adds the parts in order.  part_stride >= M * ld_parts, both % 4 == 0, parts 16-byte aligned. */
int pm_dec_linear_kparts(const float* x, int64_t ldx, const void* w, int64_t ldw, float* parts, int64_t ld_parts,
                         int64_t part_stride, int64_t M, int64_t N, int64_t K, int64_t k_split, void* stream);

/* Finish the argmax over the n_tiles tile winners of pm_dec_linear mode 2 (lowest index on ties, like torch.argmax),
 * teacher-force the prompt (next = prompt[b, t+1] while t + 1 < P), write tok_cur[b] and tokens_out[b, t+1]. */
int pm_dec_argmax_reduce(const float* ws_val, const int32_t* ws_idx, int64_t n_tiles, const int32_t* pos_ptr,
                         const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot,
                         float* margin_out, int64_t B, void* stream);

/* ++*pos_ptr, as its own launch (every workgroup of the step has read t by then). */
int pm_dec_advance(int32_t* pos_ptr, void* stream);

/* Whisper's decoding-time logit filters on the device, between the vocabulary projection (pm_dec_linear mode 0 into logits) and
 * the token choice (pm_dec_sample_topk; k = 1 = arg-max).  The reference has no Whisper decoding (README.md:86-87: TODO); the rules
 * are those of OpenAI's whisper decoding.py (SuppressTokens, SuppressBlank, ApplyTimestampRules) as published - that package is
 * not available here, so the oracle for this entry point (oracle/ref_whisper_rules.py) is "parity unpinned".
 * logits: f32 (B, V), modified in place (-inf); tokens: int64 (B, Ttot) = prompt + generated; n = *pos_ptr + 1 is the index being
 * chosen (nothing happens while n < P); eot < timestamp_begin < V; no_timestamps < 0 = none; max_initial_timestamp < 0 = no cap
 * (else the first timestamp is at most timestamp_begin + max_initial_timestamp); suppress / blank: int32 id lists (blank applies
 * to the first generated token only).  Rules: listed ids; a transcript starts with a timestamp; timestamps come in pairs and
 * never decrease; if the timestamps' total probability exceeds the best text token's, text is masked. */
int pm_dec_whisper_rules(float* logits, int64_t ldl, int64_t V, const int64_t* tokens, int64_t Ttot, const int32_t* pos_ptr,
                         int64_t P, int64_t eot, int64_t no_timestamps, int64_t timestamp_begin, int64_t max_initial_timestamp,
                         const int32_t* suppress, int64_t n_suppress, const int32_t* blank, int64_t n_blank, int64_t B,
                         void* stream);

/* Top-k sampling in place of the arg-max (text/generator.py:30-32: topk, softmax over the k logits, one multinomial draw):
 * logits (B, V) f32, row stride ldl, of the last position (pm_dec_linear mode 0 with the final LayerNorm); per sequence the
 * k (1..64) largest (ties: lowest index first), softmax over them, one draw from a counter-based generator keyed by
 * (seed, position, sequence) - the same seed gives the same ids; then the tail of pm_dec_next_token (prompt forcing,
 * x[b] = emb[token] + pos[t + 1], ticketed advance of *pos_ptr).  k = 1 is the arg-max. */
int pm_dec_sample_topk(const float* logits, int64_t ldl, int64_t V, int64_t k, uint64_t seed, int32_t* pos_ptr,
                       const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot, const void* emb,
                       const float* pos, float* x, int64_t d, int32_t* ticket, int64_t B, void* stream);

/* pm_dec_argmax_reduce + the NEXT step's pm_dec_embed + pm_dec_advance in one launch (two launches fewer per decode
 * step): sequence b's workgroup picks its token as pm_dec_argmax_reduce does, writes x[b] = emb[token] + pos[t + 1], and
 * the last workgroup to finish - an agent-scope ticket in *ticket (int32, zero before the first launch, zero again after
 * every launch) - stores t + 1 to *pos_ptr.  Before a run's first step: *pos_ptr = 0, tok_cur set, pm_dec_embed once. */
int pm_dec_next_token(const float* ws_val, const int32_t* ws_idx, int64_t n_tiles, int32_t* pos_ptr, const int64_t* prompt,
                      int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot, float* margin_out, const void* emb,
                      const float* pos, float* x, int64_t d, int64_t V, int32_t* ticket, int64_t B, void* stream);

/* Beam search on top of the decode step (csrc/decode_beam.hip; DESIGN.md "Beam search"): rows r = b * W + w (clip b, beam w),
 * 1 <= W <= 8, the step runs at B * W rows in full-logit mode and ends with these three launches instead of a token choice.
 * The reference follows one hypothesis per sequence (text/generator.py:23-35) and decodes nothing for Whisper (README.md:86).
 *
 * pm_dec_beam_topw: per row the log-sum-exp of logits[r, :V] (f32, row stride ldl; -inf entries allowed) and its W largest
 * logits (ties: lowest index first) as candidates cand_score[r, k] = scores[r] + (logit - lse), cand_tok[r, k] (int32).  A row
 * with finished[r] != 0 (and eos >= 0) offers (scores[r], eos) alone, its other entries carry token -1; a row at -inf offers
 * tokens 0 .. W - 1 at -inf.  Nothing happens while *pos_ptr + 1 < P (the prompt is being forced).  eos < 0: no row finishes. */
int pm_dec_beam_topw(const float* logits, int64_t ldl, int64_t V, int64_t W, const float* scores, const int32_t* finished,
                     int64_t eos, const int32_t* pos_ptr, int64_t P, float* cand_score, int32_t* cand_tok, int64_t rows,
                     void* stream);

/* pm_dec_beam_select: per clip the W best of its W x W candidates, best first (score descending, then lower parent beam, then
 * lower token id) -> parents[b, j] (int32), scores[b, j], finished[b, j] = the parent's flag or token == eos; the token
 * histories tokens[b, j, 0..t] = tokens[b, parent_j, 0..t] (int64 (B * W, Ttot), in place) and tokens[b, j, t + 1] = the new
 * token; then the tail of pm_dec_next_token: tok_cur, x[r] = emb[token] + pos[t + 1], ticketed advance of *pos_ptr.  While
 * t + 1 < P: identity parents, the token is prompt[r, t + 1] (prompt: int64 (B * W, P)), scores and flags stay. */
int pm_dec_beam_select(const float* cand_score, const int32_t* cand_tok, int64_t W, float* scores, int32_t* finished,
                       int32_t* parents, int64_t eos, int64_t* tokens, int64_t Ttot, int32_t* pos_ptr, const int64_t* prompt,
                       int64_t P, int64_t* tok_cur, const void* emb, const float* pos, float* x, int64_t d, int64_t V,
                       int32_t* ticket, int64_t B, void* stream);

/* pm_dec_beam_reorder: for each of the n_caches device pointers in table (uint64 each: the K and V self-attention caches of every
 * layer, (B * W, H, Tmax, 64) bf16, or f32 with kv_f32), cache[b, j, h, 0..t, :] = cache[b, parents[b, j], h, 0..t, :], in place
 * and bit for bit, t = *pos_ptr - 1 (it runs after pm_dec_beam_select moved the position); positions above t are not written;
 * clips with identity parents are left alone. */
int pm_dec_beam_reorder(const void* table, int64_t n_caches, const int32_t* parents, const int32_t* pos_ptr, int64_t B, int64_t W,
                        int64_t H, int64_t Tmax, int kv_f32, void* stream);

/* Ragged prompt batches: sequences of different prompt lengths decode in one batch by being RIGHT-ALIGNED in
 * the caches.  With Pm the longest prompt, sequence b's tokens sit at cache positions key_start[b] = Pm - len_b .. Pm - 1 and all
 * sequences generate at Pm, Pm + 1, ... together, so the step keeps its single *pos_ptr.  Cache position t of sequence b is its
 * logical position t - key_start[b] (the positional row), and its attention never sees keys below key_start[b].  key_start: int32,
 * one per sequence, in DEVICE memory (a captured step serves any lengths).  Each entry point is its plain namesake plus key_start
 * (PM_EINVAL when it is null); key_start all zero gives the plain result bit for bit.
 *
 * pm_dec_attention_ragged: sequence b attends keys lo .. Lk - 1, lo = min(key_start[b], Lk - 1) - pm_dec_attention on the caches
 * advanced by lo keys, bit for bit; a start at or past Lk (a row still inside its padding) leaves the newest key. */
int pm_dec_attention_ragged(const float* q, const void* kc, const void* vc, int64_t stride_b, int64_t stride_h, int64_t stride_k,
                            const int32_t* lk_ptr, int64_t lk_add, int64_t lk_max, const int32_t* key_start, float* out, int64_t B,
                            int64_t H, void* stream);
/* pm_prefill_attention_ragged_bf16: the query at position p = p0 + i of sequence b keeps keys lo(p) <= j <= p with
 * lo(p) = min(key_start[b], p); a padded query (p < key_start[b]) sees itself only (its output is its own v row).  The append is
 * pm_prefill_attention_bf16's: all C rows of the chunk are bit-copied, no byte outside [p0, p0 + C) is written. */
int pm_prefill_attention_ragged_bf16(const void* qkv, int64_t ld_qkv, void* kc, void* vc, int64_t stride_b, int64_t stride_h,
                                     int64_t stride_k, void* out, int64_t ld_out, int64_t B, int64_t H, int64_t C, int64_t p0,
                                     int64_t lk_max, const int32_t* key_start, void* stream);
/* out[b, l, :] = emb[tokens[b, l], :] + pos[max(0, pos0 + l - key_start[b]), :] (pos is required) */
int pm_embed_tokens_ragged(const int64_t* tokens, const void* emb, const float* pos, const int32_t* key_start, void* out,
                           int out_dtype, int64_t B, int64_t L, int64_t pos0, int64_t d, int64_t V, void* stream);
/* x[b, :] = emb[tok_cur[b], :] + pos[max(0, t - key_start[b]), :] */
int pm_dec_embed_ragged(const int64_t* tok_cur, const void* emb, const float* pos, const int32_t* pos_ptr,
                        const int32_t* key_start, float* x, int64_t B, int64_t d, int64_t V, void* stream);
/* pm_dec_next_token / pm_dec_sample_topk whose next row is x[b] = emb[token] + pos[max(0, t + 1 - key_start[b])]; prompt is the
 * right-aligned (B, P) matrix; token choice, prompt forcing, margins, the draw (keyed by the CACHE position) and the ticketed
 * advance are the plain kernels'. */
int pm_dec_next_token_ragged(const float* ws_val, const int32_t* ws_idx, int64_t n_tiles, int32_t* pos_ptr, const int64_t* prompt,
                             int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot, float* margin_out, const void* emb,
                             const float* pos, const int32_t* key_start, float* x, int64_t d, int64_t V, int32_t* ticket,
                             int64_t B, void* stream);
int pm_dec_sample_topk_ragged(const float* logits, int64_t ldl, int64_t V, int64_t k, uint64_t seed, int32_t* pos_ptr,
                              const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot,
                              const void* emb, const float* pos, const int32_t* key_start, float* x, int64_t d, int32_t* ticket,
                              int64_t B, void* stream);

/* The sampling tail (csrc/sample.hip): pm_dec_sample_topk's place in a step, with a temperature, the whole vocabulary as an
 * option, a nucleus cut and the emitted token's log-probability.  logits (B, V) f32, row stride ldl, after the rules (finite
 * or -inf); m = the row maximum.
 *   logprobs (B, Ttot) f32 or NULL: [b, t + 1] = l[token] - (m + log sum exp(l - m)), at temperature 1 whatever is drawn;
 *             written for every stepped position (at a prompt-forced position: the forced token's)
 *   temperature == 0: the lowest index with l == m; topk and top_p are ignored
 *   temperature  > 0: weights exp((l - m) / temperature); survivors = the topk (1..64, at most V) first tokens in the order
 *             (logit descending, index ascending), topk == 0 = every token; top_p < 1: tau = the largest logit value among the
 *             survivors with mass(survivors with l >= tau) >= top_p * mass(survivors), the nucleus = every survivor with
 *             l >= tau (ties at the boundary are all kept); the pick = the first nucleus element whose running mass exceeds
 *             u * mass(nucleus), running in the sorted order (topk >= 1) or by ascending index (topk == 0), u = the draw of
 *             pm_dec_sample_topk keyed by (seed, cache position, row).  topk = k, temperature 1, top_p 1 picks what
 *             pm_dec_sample_topk picks.  An entry of weight 0 is never drawn.
 * Every reduction has one fixed order (no floating-point atomics): token and log-prob are bit-identical run to run.  Then the
 * tail of pm_dec_next_token.  PM_EINVAL before any launch: a null pointer other than logprobs, V <= 0, ldl < V, topk outside
 * 0..64, temperature negative / NaN / infinite, top_p outside (0, 1], d % 8 != 0.  The _ragged form takes the positional row
 * pos[max(0, t + 1 - key_start[b])]. */
int pm_dec_sample(const float* logits, int64_t ldl, int64_t V, int64_t topk, float temperature, float top_p, uint64_t seed,
                  int32_t* pos_ptr, const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot,
                  float* logprobs, const void* emb, const float* pos, float* x, int64_t d, int32_t* ticket, int64_t B,
                  void* stream);
int pm_dec_sample_ragged(const float* logits, int64_t ldl, int64_t V, int64_t topk, float temperature, float top_p, uint64_t seed,
                         int32_t* pos_ptr, const int64_t* prompt, int64_t P, int64_t* tok_cur, int64_t* tokens_out, int64_t Ttot,
                         float* logprobs, const void* emb, const float* pos, const int32_t* key_start, float* x, int64_t d,
                         int32_t* ticket, int64_t B, void* stream);

/* Repetition controls and eos bookkeeping of a decode step (csrc/controls.hip).
 * pm_dec_controls: between the vocabulary projection and pm_dec_whisper_rules / the token tail.  logits (B, V) f32, row stride
 *   ldl, edited in place; tokens int64 (B, Ttot); t = *pos_ptr, nothing happens while t + 1 < P.  The history of row b is
 *   tokens[b, s .. t], s = key_start[b] (int32 (B,), clamped to 0..t) or 0 when key_start is NULL; ids outside [0, V) are skipped.
 *     repetition_penalty r (finite, > 0; 1 = off): every DISTINCT id v of the history, once: l[v] = l[v] > 0 ? l[v] / r : l[v] * r,
 *       one correctly rounded fp32 operation on the original value (-inf stays -inf, NaN stays NaN, a zero keeps its sign)
 *     no_repeat_ngram n (0..8; 0 = off): with m ids of history and m >= n - 1, for every 0 <= i <= m - n whose ids i .. i + n - 2
 *       equal the last n - 1 ids: l[h[i + n - 1]] = -inf (n = 1: every id of the history)
 *     min_new_tokens (needs eos >= 0): while t + 1 - P < min_new_tokens, l[eos] = -inf.  eos = -1: none.
 *   The result does not depend on thread scheduling.  PM_EINVAL before any launch: a null logits / tokens / pos_ptr, V <= 0 or
 *   V > 262144 (the set of seen ids is V bits of LDS), ldl < V, r not finite or <= 0, n outside 0..8, min_new_tokens < 0 or
 *   without eos, eos outside -1..V - 1.
 * pm_dec_finish: behind the token tail (pm_dec_next_token, pm_dec_sample_topk, pm_dec_sample, ragged or not); t1 = *pos_ptr is the
 *   position that tail wrote and advanced to; nothing happens while t1 < P.  finished int32 (B,), 0 = still running: a row with
 *   finished[b] != 0 gets tokens[b, t1] = pad, tok_cur[b] = pad and (logprobs f32 (B, Ttot) or NULL) logprobs[b, t1] = 0;
 *   otherwise a row whose tokens[b, t1] == eos records finished[b] = t1.  PM_EINVAL: a null tokens / tok_cur / finished /
 *   pos_ptr, eos < 0, pad < 0. */
int pm_dec_controls(float* logits, int64_t ldl, int64_t V, const int64_t* tokens, int64_t Ttot, const int32_t* pos_ptr, int64_t P,
                    const int32_t* key_start, float repetition_penalty, int64_t no_repeat_ngram, int64_t min_new_tokens,
                    int64_t eos, int64_t B, void* stream);
int pm_dec_finish(int64_t* tokens, int64_t Ttot, int64_t* tok_cur, float* logprobs, int32_t* finished, const int32_t* pos_ptr,
                  int64_t P, int64_t eos, int64_t pad, int64_t B, void* stream);

/* ConvNeXt (reference: pytorch_models/image/convnext.py), csrc/convnext.hip.  NHWC rows, fp32 arithmetic; x_dtype / y_dtype
 * PM_BF16 or PM_F32; gamma / beta / bias f32.  The pointwise MLP and the downsample's Conv2d(C, 2C, 2, 2) run on the GEMMs above.
 *
 * pm_dwconv7_ln: y = LayerNorm_C(Conv2d(C, C, 7, padding 3, groups C)(x) + bias) (convnext.py:22-25).  x: (N, H, W, C)
 * contiguous; w: f32 (7, 7, C) (the weight (C, 1, 7, 7) permuted); y: (N*H*W, ldy) rows whose columns C .. ldy-1 are written as
 * zeros (ldy = C rounded up to 64 feeds pm_linear_bf16, K % 64 == 0).  C % 4 == 0, C <= 4096, ldy % 4 == 0, 16-byte aligned
 * f32 / 8-byte aligned bf16 operands. */
int pm_dwconv7_ln(const void* x, int x_dtype, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                  void* y, int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C, void* stream);

/* pm_ln_space_to_depth: LayerNorm_C of every pixel of x (N, H, W, C) (pixel row stride ldx), then output row (n, i, j) of y
 * (N*H/2*W/2, ldy) = the normalised pixels (2i, 2j), (2i, 2j+1), (2i+1, 2j), (2i+1, 2j+1) side by side, columns 4C .. ldy-1
 * zero: the downsample's LayerNorm + Conv2d(C, 2C, 2, 2) (convnext.py:47-52) becomes one GEMM with the weight permuted to
 * (Cout, kh, kw, Cin).  H, W even; any C. */
int pm_ln_space_to_depth(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps, void* y,
                         int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C, void* stream);

/* pm_convnext_stem: Conv2d(3, d, 4, stride 4) + bias, then LayerNorm_d (convnext.py:41).  imgs: f32 NCHW (N, 3, Himg, Wimg);
 * wt: f32 (48, d), the weight (d, 3, 4, 4) flattened to (d, 48) and transposed; y: (N*(Himg/4)*(Wimg/4), ldy) NHWC rows, columns
 * d .. ldy-1 zero.  fp32 fma in (ci, kh, kw) order on the VALU.  d <= 384. */
int pm_convnext_stem(const float* imgs, const float* wt, const float* bias, const float* gamma, const float* beta, float eps,
                     void* y, int64_t ldy, int y_dtype, int64_t N, int64_t Himg, int64_t Wimg, int64_t d, void* stream);

/* pm_mean_ln: y[n, :] = LayerNorm_C(mean over r < HW of x[n*HW + r, :]) (convnext.py:67-68: pool + norm); x rows with stride
 * ldx, y (N, C) contiguous.  C <= 16000. */
int pm_mean_ln(const void* x, int64_t ldx, int x_dtype, const float* gamma, const float* beta, float eps, void* y, int y_dtype,
               int64_t N, int64_t HW, int64_t C, void* stream);

/* MaxViT (reference: pytorch_models/image/maxvit.py), csrc/maxvit.hip.  NHWC rows, fp32 arithmetic; x_dtype / y_dtype PM_BF16 or
 * PM_F32.  The 1 x 1 convolutions (BatchNorms folded), q/k/v / out projections and the MLPs run on the GEMMs above.
 *
 * pm_window_attention_bf16: softmax(q k^T / sqrt(32) + bias[h]) v per (window, head), head dim 32, over the windows of an NHWC
 * image (N, Himg, Wimg) whose pixel rows hold the heads side by side: q / k / v of head h at pixel row r are the 32 bf16 at
 * base + r*ld + h*32 (the packed QKV projection read in place), the output goes to o + r*ldo + h*32 (pixel order, heads merged).
 * mode 0 = block (maxvit.py:70-81, block/unblock): window (n, wy, wx), token (i, j) is pixel (wy*ws + i, wx*ws + j); mode 1 =
 * grid (maxvit.py:84-91, grid/ungrid): pixel (i*Himg/ws + wy, j*Wimg/ws + wx).  Token t = i*ws + j indexes bias, f32 (H, L, L)
 * with L = ws*ws <= 64 (RelativeMHA's gathered relative bias, maxvit.py:105-112, shared by every window), or null.  bf16 MFMA,
 * fp32 softmax.  Himg, Wimg multiples of ws; ld % 8 == 0, 16-byte aligned q / k / v. */
int pm_window_attention_bf16(const void* q, const void* k, const void* v, int64_t ld, void* o, int64_t ldo, const float* bias,
                             int64_t N, int64_t Himg, int64_t Wimg, int64_t n_heads, int64_t ws, int mode, void* stream);

/* pm_dwconv3_bn_act: y = gelu_tanh(Conv2d(C, C, 3, stride, groups C)(x) * scale + shift) [* gate[n, c]] (MBConv's depthwise
 * conv_norm_act, maxvit.py:27-31 / 52, with its BatchNorm folded to scale / shift, and the squeeze-excitation product of
 * maxvit.py:44).  stride 1: padding 1; stride 2: the reference's F.pad(x, (0, 1, 0, 1)) + padding 0 (maxvit.py:19-21), output
 * ((H - 2) / 2 + 1, (W - 2) / 2 + 1).  x (N, H, W, C) contiguous; w f32 (3, 3, C); gate f32 (N, C) or null; psum, if not null,
 * receives f32 (N, Ho, C): the sums over each output row of the UNGATED output (the squeeze-excitation's pool, in a fixed order);
 * y may be null when psum is not.  C % 4 == 0. */
int pm_dwconv3_bn_act(const void* x, int x_dtype, const float* w, const float* scale, const float* shift, const float* gate,
                      float* psum, void* y, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C, int stride, void* stream);

/* pm_se_gate: gate[n, :] = sigmoid(w2 @ silu(w1 @ m + b1) + b2) with m = (sum over t < ntiles of psum[n, t, :]) / hw
 * (SqueezeExcitation, maxvit.py:34-41).  psum f32 (N, ntiles, C); w1 f32 (R, C); w2 f32 (C, R); gate f32 (N, C).  fp32.
 * C <= 16384, R <= 4096 and (C + R) * 4 <= 64 KiB (the pooled vector and the hidden one share one workgroup's LDS); anything
 * beyond is PM_EUNSUPPORTED. */
int pm_se_gate(const float* psum, int64_t ntiles, int64_t hw, const float* w1, const float* b1, const float* w2, const float* b2,
               float* gate, int64_t N, int64_t C, int64_t R, void* stream);

/* pm_maxvit_stem: gelu_tanh(Conv2d(3, d, 3, 2, bias=False)(F.pad(imgs, (0, 1, 0, 1))) * bn_scale + bn_shift) (maxvit.py:150-152).
 * imgs f32 NCHW (N, 3, Himg, Wimg); wt f32 (27, d), the weight (d, 3, 3, 3) times the BatchNorm scale, flattened to (d, 27) and
 * transposed; shift f32 (d); y (N*Ho*Wo, ldy) NHWC rows, columns d .. ldy-1 zero.  fp32 fma on the VALU.  d <= 256. */
int pm_maxvit_stem(const float* imgs, const float* wt, const float* shift, void* y, int64_t ldy, int y_dtype, int64_t N,
                   int64_t Himg, int64_t Wimg, int64_t d, void* stream);

/* pm_im2col3x3_nhwc: y[(n, h, w), (kh*3 + kw)*C + c] = x[n, h + kh - 1, w + kw - 1, c] (zero outside), columns 9C .. ldy-1 zero:
 * the stem's second Conv2d(s, s, 3) (maxvit.py:154) as one GEMM with the weight permuted to (Cout, kh, kw, Cin).  x (N, H, W, C)
 * contiguous; C % 4 == 0, ldy % 4 == 0. */
int pm_im2col3x3_nhwc(const void* x, int x_dtype, void* y, int64_t ldy, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                      void* stream);

/* pm_avgpool2x2_nhwc: y (N, H/2, W/2, C) = AvgPool2d(2)(x) (the MBConv shortcut, maxvit.py:59-60); x (N, H, W, C) contiguous;
 * H, W even, C % 4 == 0. */
int pm_avgpool2x2_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C, void* stream);

/* ---- DETR (reference: pytorch_models/image/detr.py): ResNet bottleneck backbone and head-dim-32 attention.
 * pm_conv_bf16: y = relu?(conv(x, w) + bias [+ resid]) as an implicit GEMM on the bf16 MFMA (csrc/resnet.hip) - the ReLU comes
 * AFTER the residual add (Bottleneck.forward, detr.py:33; pm_linear_bf16's act(..) + resid cannot express that).  x: bf16 NHWC
 * (N, H, W, Cin) contiguous; w: bf16 (Cout, ksize, ksize, Cin) contiguous (an eval BatchNorm folded in by the caller); bias: f32
 * (Cout) or NULL; resid: bf16 like y or NULL; y: bf16 (N, Ho, Wo, Cout), Ho = (H + 2 pad - ksize) / stride + 1.  ksize 3 (pad 1)
 * or 1 (pad 0); stride 1 or 2; Cin % 64 == 0; any Cout.  The input tile is gathered from the NHWC rows into LDS (zeros outside
 * the image): no im2col buffer.  fp32 accumulation, one rounding to bf16.  relu: 0 | 1.  All pointers 16-byte aligned. */
int pm_conv_bf16(const void* x, int64_t N, int64_t H, int64_t W, int64_t Cin, const void* w, const float* bias, const void* resid,
                 void* y, int64_t Cout, int64_t ksize, int64_t stride, int relu, void* stream);

/* pm_resnet_stem: MaxPool2d(3, 2, 1)(relu(Conv2d(3, 64, 7, 2, 3, bias=False)(imgs) * bn_scale + bn_shift)) (detr.py:40-45).
 * imgs f32 NCHW (N, 3, Himg, Wimg); wt f32 (147, 64): the weight (64, 3, 7, 7) times the BatchNorm scale, flattened to (64, 147)
 * and transposed; shift f32 (64); conv_map: caller-owned scratch, bf16 (N, Hc, Wc, 64) with Hc = (Himg - 1) / 2 + 1 (the
 * convolution's output, written and then pooled: two kernels); y: bf16 NHWC (N, Hp, Wp, 64), Hp = (Hc - 1) / 2 + 1.  fp32 fma
 * on the VALU (K = 147 does not suit the matrix pipe). */
int pm_resnet_stem(const float* imgs, const float* wt, const float* shift, void* conv_map, void* y, int64_t N, int64_t Himg,
                   int64_t Wimg, void* stream);

/* pm_attention_hd32_bf16: softmax(q k^T / sqrt(32)) v for head dim 32 on the bf16 MFMA, flash style (online fp32 softmax over
 * key tiles of 64, the key tail masked in the kernel; csrc/attention_hd32.hip).  Addressing as pm_attention_bf16 with h*32 head
 * offsets; any Lq >= 1, Lk >= 1; no bias, no causal mask (DETR has neither: detr.py:64-87).  Strides multiples of 8 elements
 * (o: 4), q / k / v 16-byte aligned (o: 8). */
int pm_attention_hd32_bf16(const void* q, int64_t q_stride_b, int64_t q_stride_t, const void* k, int64_t k_stride_b,
                           int64_t k_stride_t, const void* v, int64_t v_stride_b, int64_t v_stride_t, void* o,
                           int64_t o_stride_b, int64_t o_stride_t, int64_t B, int64_t H, int64_t Lq, int64_t Lk, void* stream);

/* ---- MLP-Mixer (reference: pytorch_models/image/mlp_mixer.py; csrc/mixer.hip).
 * pm_mixer_token_mix_bf16: y = x + (W2 GELU(W1 LN(x)^T + b1) + b2)^T per image (mlp_mixer.py:30), one kernel on the bf16 MFMA.
 * x, y: bf16 (N, T, C) contiguous; y may alias x (y == x: a workgroup stages its own image x channel slab behind a barrier and a
 * thread loads the residual elements it stores before it stores them); y must not alias any other operand.  stats: f32 (N*T, 2) [mean, rstd] of the rows of x (pm_ln_stats_finalize or
 * pm_row_stats); gamma, beta: f32 (C), norm1; b1: f32 (Dt); b2: f32 (T).
 * w1, w2: the weights W1 (Dt, T) and W2 (T, Dt) FRAGMENT-MAJOR, bf16: a matrix W (R, K) is zero-padded to R32 = R rounded up to
 * 32 rows and K16 = K rounded up to 16 columns and stored as [R32/32 strips][K16/16 steps][64 lanes][8], lane l of strip s and
 * step k holding W[32 s + (l & 31)][16 k + 8 (l >> 5) + 0..7] - the A operand of mfma_f32_32x32x16_bf16, so a wave's load is
 * 1 KiB contiguous.  The zero padding is part of the contract (it is the K padding of the first product).
 * LN(x) and the hidden activations are rounded to bf16, both products accumulate in fp32, the output is rounded once.
 * row_out: NULL or f32 (N*T, C/64, 2): per row and 64-channel block (sum, sum of squares) of the bf16-rounded y, the layout
 * pm_ln_stats_finalize reads.  Every image is computed alone (bit-identical at any batch size and position).
 * C % 64 == 0, Dt % 32 == 0, and one image x 64 channels of LN(x) and of the hidden activations must fit the 160 KiB LDS:
 * pm_mixer_token_mix_supported(T, Dt, C) (1 = served); N <= 65535.  All pointers 16-byte aligned (stats, row_out: 8). */
int pm_mixer_token_mix_bf16(const void* x, const float* stats, const float* gamma, const float* beta, const void* w1,
                            const float* b1, const void* w2, const float* b2, void* y, float* row_out, int64_t N, int64_t T,
                            int64_t Dt, int64_t C, void* stream);
int pm_mixer_token_mix_supported(int64_t T, int64_t Dt, int64_t C);
/* pm_mixer_token_mix_plan: host only - what pm_mixer_token_mix_bf16 launches for (T, Dt, C), decided by the launcher's own
 * functions.  report = 8 int32: NB (channels per workgroup / 32: 4 or 2), the dynamic LDS bytes, region_a (the byte offset of
 * the hidden activations), nk1 = Tp / 16, nk2 = Dt / 16, nd = Dt / 32, nt = ceil(T / 32), and 1 where region_a is the per-wave
 * scratch's size, 0 where it is the slab's.  PM_EUNSUPPORTED where pm_mixer_token_mix_supported is 0; a refusal writes nothing. */
int pm_mixer_token_mix_plan(int64_t T, int64_t Dt, int64_t C, int32_t* report);

/* pm_row_stats: stats[m] = (mean, rsqrt(biased variance + eps)) of row m of x (M, C), x_dtype rows with stride ldx: the format
 * pm_ln_stats_finalize writes, for rows that no GEMM epilogue has summed.  fp32, centred second pass. */
int pm_row_stats(const void* x, int64_t ldx, int x_dtype, float* stats, int64_t M, int64_t C, float eps, void* stream);

/* pm_ln_mean: y[n, :] = mean over t < T of LayerNorm_C(x[n, t, :]) (mlp_mixer.py:58-59: norm, then the mean over tokens - not
 * pm_mean_ln's mean-then-norm).  x (N, T, C) contiguous; stats (N*T, 2) as pm_row_stats writes them; y (N, C) contiguous. */
int pm_ln_mean(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y, int y_dtype,
               int64_t N, int64_t T, int64_t C, void* stream);

/* pm_transpose_add_f32: y (N, Cc, R) = x (N, R, Cc) transposed per n [+ resid (N, Cc, R) when not NULL]; f32; x contiguous, the
 * rows of y and resid ldy >= R apart (columns R .. ldy-1 are not written: a K padding that pm_linear_f32 never reads).
 * The two transposes of the composed fp32 token mixing. */
int pm_transpose_add_f32(const float* x, const float* resid, float* y, int64_t ldy, int64_t N, int64_t R, int64_t Cc, void* stream);

/* ---- EnCodec (reference: pytorch_models/audio/encodec.py; csrc/encodec.hip).  Everything fp32 on the exact-product f32 MFMA;
 * activations TIME-MAJOR (B, T, C).
 * pm_conv1d_f32: a 1-D convolution as an implicit GEMM.  x: clip b at x + b * x_batch_stride, (Tin, Cin) contiguous.
 * w: (up * Cout, k * Cin) row-major, column tap * Cin + ci.  Row m < Mr = (Tin + left + right - k) / stride + 1 of the product
 * reads the frames m * stride - left .. + k - 1: beyond the clip they are MIRRORED (F.pad "reflect"; left, right < Tin; right
 * includes the extra padding that rounds the length up to the stride) or, zero_pad != 0, zero.  elu != 0: ELU on the operand as
 * it is loaded.  Column n of the product is channel n % Cout of output frame m * up + n / Cout - trim; frames outside
 * [0, Tout) are dropped.  y, resid: (B, Tout, Cout) contiguous; bias (Cout) and resid (up == 1, trim == 0 only) may be NULL.
 * Conv1d: up = 1, trim = 0, Tout = Mr.  ConvTranspose1d(kernel 2 s, stride s) + Unpad1d: k = 2, stride = 1, left = right = 1,
 * zero_pad = 1, up = s, w[r * Cout + co][j * Cin + ci] = weight[ci][co][r + (1 - j) * s], trim = the left trim.
 * Cin % 4 == 0 takes 16-byte loads (x, w 16-byte aligned, x_batch_stride % 4 == 0), Cout % 4 == 0 16-byte stores.
 * pm_conv1d_f32_supported: 1 when the geometry is served. */
int pm_conv1d_f32(const float* x, int64_t x_batch_stride, const float* w, const float* bias, const float* resid, float* y,
                  int64_t B, int64_t Tin, int64_t Cin, int64_t Cout, int64_t k, int64_t stride, int64_t left, int64_t right,
                  int zero_pad, int elu, int64_t up, int64_t trim, int64_t Tout, void* stream);
int pm_conv1d_f32_supported(int64_t Tin, int64_t Cin, int64_t Cout, int64_t k, int64_t stride, int64_t left, int64_t right,
                            int zero_pad, int64_t up);

/* pm_lstm_f32: n_layers stacked LSTM layers (nn.LSTM: gates i, f, g, o; zero initial state) over x (B, T, H) time-major, input
 * size == hidden size H (H % 64 == 0).  w_ih, w_hh, bias: HOST arrays of n_layers device pointers: (4H, H), (4H, H) and
 * bias_ih + bias_hh (4H).  y (B, T, H) = the last layer's h (+ x when flags & 1).  ONE LAUNCH PER STEP, no grid-wide wait of any
 * kind.  Two layers run as a wavefront: one pm_linear_f32 for layer 0's input projections of all frames, then T + 1 launches in
 * which layer 0 at frame s runs beside layer 1 at frame s - 1 (layer 1 multiplies [h0, h1_prev] with [W_ih; W_hh] itself).
 * flags & 2, or another number of layers: plain passes, per layer one pm_linear_f32 and T launches.  Every launch goes to `stream`,
 * so the call can be captured in a graph.  work: pm_lstm_workspace_floats(B, T, H) floats, 16-byte aligned.  Rows of the batch are
 * independent: row i is bit-identical at any batch size. */
int pm_lstm_f32(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* bias, int64_t n_layers,
                float* work, float* y, int flags, int64_t B, int64_t T, int64_t H, void* stream);
int64_t pm_lstm_workspace_floats(int64_t B, int64_t T, int64_t H);

/* pm_rvq_encode_f32: residual vector quantization of z (M, dim) with the first n_q of codebooks (n_q, codebook_size, dim);
 * norms (n_q, codebook_size) = the squared norms of the entries.  Per stage: argmin of |e|^2 - 2 r.e (lowest index on exact
 * ties), r -= e.  codes: int64 (n_q, M).  dim == 128 and codebook_size == 1024 only.
 * pm_rvq_decode_f32: out (B * T, dim) = sum over q < n_q, in stage order, of codebooks[q][codes[b * stride_b + q * stride_q +
 * t * stride_t]] (indices outside the codebook are clamped into it). */
int pm_rvq_encode_f32(const float* z, const float* codebooks, const float* norms, int64_t* codes, int64_t M, int64_t n_q,
                      int64_t dim, int64_t codebook_size, void* stream);
int pm_rvq_decode_f32(const int64_t* codes, int64_t stride_b, int64_t stride_q, int64_t stride_t, const float* codebooks,
                      float* out, int64_t B, int64_t T, int64_t n_q, int64_t dim, int64_t codebook_size, void* stream);

/* pm_groupnorm1_f32: GroupNorm(1, C) of B clips in place: x (B, n) with n = T * C time-major (channel = index % C), biased
 * variance over the whole clip, per-channel affine, + resid (B, n) when not NULL.  Per thread the fp32 mean of 64 floats and their
 * centred sums, combined in fp64 (Chan): no (mean / sigma)^2 error.  work: pm_groupnorm1_workspace_doubles(B, n) doubles.  B <= 65535. */
int pm_groupnorm1_f32(float* x, const float* gamma, const float* beta, const float* resid, double* work, int64_t B, int64_t n,
                      int64_t C, float eps, void* stream);
int64_t pm_groupnorm1_workspace_doubles(int64_t B, int64_t n);

/* pm_encodec_scale_f32: scale[b] = sqrt(mean_t(mean_c(x[b, c, t])^2)) + 1e-8 of x (B, C, T) (encodec.py:198).
 * pm_scale_clips_f32: y[b, i] = x[b, i] / scale[b] (divide != 0) or x[b, i] * scale[b], i < n; y may alias x.  B <= 65535. */
int pm_encodec_scale_f32(const float* x, float* scale, int64_t B, int64_t C, int64_t T, void* stream);
int pm_scale_clips_f32(const float* x, const float* scale, float* y, int64_t B, int64_t n, int divide, void* stream);

/* ---- KV-cached T5 decode step (text/t5.py: T5Model.generate), csrc/decode_t5.hip.  The stages whose form differs from the
 * pm_dec_* step: RMS norm without centring or bias (gamma f32 (d), eps), bias-free projections (bf16 weights, K-contiguous rows
 * of d), inner = H * 64 independent of d, a relative-position bias on the self-attention scores, a gated MLP, eos bookkeeping.
 * x: f32 (B, d) contiguous, B <= 64, d % 8 == 0, d <= 1024; all pointers 16-byte aligned.  Every result of sequence b depends
 * on sequence b alone, in one fixed summation order.
 *
 * pm_t5_dec_self_fused: one workgroup per (b, h): [q|k|v] = rmsnorm(x[b]) w_qkv[{q,k,v} rows of head h]^T (w_qkv (3 * inner, d)),
 *   k / v rounded to bf16 into kcache / vcache (B, H, Tmax, 64) at t = *pos_ptr, then softmax_j(q k_j / 8 + lut[h, t - j]) v_j over
 *   j <= t -> att f32 (B, inner).  lut: f32 (H, Tmax), the one-sided relative-position bias by distance.  Tmax <= 2048.
 * pm_t5_dec_rms_qkv + pm_t5_dec_self_attention: the same result as two launches (the projection reads w_qkv once per 8 sequences;
 *   q: f32 (B, inner) scratch) - for B * H beyond the number of compute units.
 * pm_t5_dec_cross_fused: q = rmsnorm(x[b]) w_q[rows of head h]^T over the first src_len[b] (int32 (B), clamped to S) keys of
 *   cross_kv bf16 (B, S, [k | v]) (2 * inner per key); src_len[b] == 0 -> zeros.  S <= 2048.
 * pm_t5_dec_geglu: h[b, f] = gelu_tanh(rmsnorm(x[b]) . w_wv[2 f]) * (rmsnorm(x[b]) . w_wv[2 f + 1]): w_wv (2 F, d) holds the
 *   gate row and the value row of feature f next to each other; h f32, row stride ldh.  F % 8 == 0.
 * pm_t5_dec_next_token: per sequence the winner of the (n_tiles) tile winners pm_dec_linear mode 2 left (lowest index on ties);
 *   position t + 1 (t = *pos_ptr) gets prompt[b, t + 1] while t + 1 < P, pad_id once finished[b], else the winner, and a winner
 *   equal to eos_id >= 0 sets finished[b] (int32) and out_lengths[b] = t + 2 (int64); tokens (B, Ttot) int64; x[b] = emb[token]
 *   (no positional term); logits_all != NULL: logits_step (B, V) f32 is copied to logits_all[b, t, :] of (B, Ttot - 1, V); the last
 *   workgroup (agent-scope ticket, *ticket zero before and after) stores t + 1 to *pos_ptr.
 * pm_t5_dec_embed: x[b] = emb[tok[b * ldtok]] (before a run's first step). */
int pm_t5_dec_embed(const int64_t* tok, int64_t ldtok, const void* emb, float* x, int64_t B, int64_t d, int64_t V, void* stream);
int pm_t5_dec_self_fused(const float* x, int64_t d, const float* gamma, float eps, const void* w_qkv, void* kcache, void* vcache,
                         int64_t Tmax, const int32_t* pos_ptr, const float* lut, float* att, int64_t B, int64_t H, void* stream);
int pm_t5_dec_rms_qkv(const float* x, int64_t d, const float* gamma, float eps, const void* w_qkv, float* q, void* kcache,
                      void* vcache, int64_t Tmax, const int32_t* pos_ptr, int64_t B, int64_t H, void* stream);
int pm_t5_dec_self_attention(const float* q, const void* kcache, const void* vcache, int64_t Tmax, const int32_t* pos_ptr,
                             const float* lut, float* att, int64_t B, int64_t H, void* stream);
int pm_t5_dec_cross_fused(const float* x, int64_t d, const float* gamma, float eps, const void* w_q, const void* cross_kv,
                          int64_t S, const int32_t* src_len, float* att, int64_t B, int64_t H, void* stream);
int pm_t5_dec_geglu(const float* x, int64_t d, const float* gamma, float eps, const void* w_wv, float* h, int64_t ldh, int64_t B,
                    int64_t F, void* stream);
int pm_t5_dec_next_token(const float* ws_val, const int32_t* ws_idx, int64_t n_tiles, int32_t* pos_ptr, const int64_t* prompt,
                         int64_t P, int64_t* tokens, int64_t Ttot, int64_t pad_id, int64_t eos_id, int32_t* finished,
                         int64_t* out_lengths, const void* emb, float* x, int64_t d, int64_t V, int32_t* ticket,
                         const float* logits_step, float* logits_all, int64_t B, void* stream);

/* ---- Class-token tail (csrc/cls_tail.hip): the last encoder layer of a class-token ViT for ONE query per image and head,
 * without projecting K or V.  With W'k, W'v the k / v weights with the layer's sa_norm gamma folded in and (mean_j, rstd_j)
 * the sa_norm statistics of the stored rows x_j: u_h = W'k,h^T q_h, p_hj = softmax_j(scale rstd_j (u_h . x_j - mean_j sum(u_h))),
 * ctx_h = sum_j p_hj rstd_j (x_j - mean_j), o_h = W'v,h ctx_h + (W_v beta + b_v)_h.
 * pm_cls_attend: x bf16, N images of L rows of d (row stride x_row_stride, image stride x_batch_stride, elements; both % 8);
 *   stats f32 (N*L, 2) [mean, rstd] of the rows (pm_ln_stats_finalize / pm_row_stats), or NULL: the kernel computes them with
 *   eps in the pass it makes anyway; u bf16 (N, H, d) contiguous; ctx bf16 (N, H, d) contiguous.  One workgroup per image: the
 *   result of an image does not depend on N or on its position.  d % 64 == 0, H <= 16 (else PM_EINVAL); d <= 1024 (else
 *   PM_EUNSUPPORTED; pm_cls_attend_supported(L, d, H) = 1 where served).  x, u 16-byte aligned; ctx, stats 8.
 * pm_cls_head_gemm: y[m, g, :] = x[m, g, :] w[g]^T (+ bias[g]) for g < G in one launch: x bf16, row m of group g = K elements at
 *   x + m ldx + g x_group_stride; w bf16 (G, N, K) contiguous; bias f32 (G, N) or NULL; y bf16 at y + m ldy + g y_group_stride.
 *   N % 64 == 0, K % 32 == 0.  fp32 accumulation in a fixed order per element: a row's result does not depend on M or on the
 *   row's position. */
int pm_cls_attend(const void* x, int64_t x_row_stride, int64_t x_batch_stride, const float* stats, const void* u, void* ctx,
                  int64_t N, int64_t L, int64_t d, int64_t H, float scale, float eps, void* stream);
int pm_cls_attend_supported(int64_t L, int64_t d, int64_t H);
int pm_cls_head_gemm(const void* x, int64_t ldx, int64_t x_group_stride, const void* w, const float* bias, void* y, int64_t ldy,
                     int64_t y_group_stride, int64_t M, int64_t N, int64_t K, int64_t G, void* stream);

/* ---- Sequence scoring (csrc/lm_score.hip): the vocabulary projection with the logits consumed in registers.  With
 * x[m, v] = sum_k h[m, k] w[v, k] (fp32 accumulation): lse[m] = log sum_{v < V} exp(x[m, v]), logprob[m] = x[m, targets[m]] - lse[m],
 * argmax[m] = the LOWEST index among the maxima of x[m, :V].  The (M, V) matrix is never stored.
 *   h bf16 (M, K), row stride ldh; w bf16 (V, K), row stride ldw (elements, both % 8, bases 16-byte aligned: else PM_EALIGN);
 *   targets int64 (M) in [-1, V): -1 (and any id outside [0, V): a bad id cannot fault; callers validate the range) means "ignore":
 *   logprob[m] = 0, lse and argmax are still written.  logprob f32 (M); lse f32 (M) or NULL; argmax int32 (M) or NULL;
 *   ws: pm_lm_score_ws_bytes(M, V) bytes (20 per row and 2048-column vocabulary chunk), 4-byte aligned, no initial state.
 *   K % 8 == 0 (else PM_EUNSUPPORTED); any M, V, K >= 1 otherwise.  No atomics; chunking and merge order depend on V alone, so a
 *   row's outputs are bit-identical wherever the row sits in the batch and whatever M is. */
int pm_lm_score_bf16(const void* h, int64_t ldh, const void* w, int64_t ldw, const int64_t* targets, float* logprob, float* lse,
                     int32_t* argmax, void* ws, int64_t M, int64_t V, int64_t K, void* stream);
int64_t pm_lm_score_ws_bytes(int64_t M, int64_t V);

/* ---- Whisper token timestamps (csrc/align.hip): cross-attention alignment matrix + dynamic time warping.  For B clips with
 * len_b <= L token rows and F_b <= S frames, and the n_sel selected heads of ONE decoder layer (head dim 64):
 *   lse[b, a, t] = log sum_{f < F_b} exp(q_t . k_f / 8);   p = exp(q_t . k_f / 8 - lse);   n = (p - mean_t p) / std_t p over t < len_b
 *   (biased std; a column whose rows are all equal - std exactly 0 - gives 0);   m[b, t, f] (+)= inv_heads * sum_a median7_f(n[a, t, :]) with reflect
 *   padding at 0 and F_b - 1.  The (n_sel, L, F) probabilities are never stored.
 *   q bf16: row t of clip b = n_heads * 64 elements at q + b q_batch_stride + t ldq, head h at column 64 h; k likewise with S rows
 *   (a view into a packed k|v projection has ldk = 2 * n_heads * 64).  Strides in elements, all % 8, bases 16-byte aligned (else
 *   PM_EALIGN); ldq, ldk >= n_heads * 64 (else PM_EINVAL).  heads int32 (n_sel) device array of head indices (clamped into
 *   [0, n_heads): a bad index cannot fault; callers validate); lengths, frames int32 (B) device arrays, 1 <= len_b <= L,
 *   4 <= F_b <= S (clamped into [1, L] and [1, S] likewise).  B, n_sel <= 65535.
 * pm_align_lse_bf16: lse f32 (B, n_sel, L) contiguous; rows t >= len_b are not written.  Any L.
 * pm_align_matrix_bf16: one call per aligned layer, in a fixed order.  m f32: row t of clip b at m + b m_batch_stride + t ldm,
 *   ldm >= S.  first != 0: m is overwritten, and entries with t >= len_b or f >= F_b are set to 0 (m needs no initial state);
 *   first == 0: the call adds to the entries with t < len_b and f < F_b.  inv_heads = 1 / (heads of ALL calls).  L <= 448 (else
 *   PM_EUNSUPPORTED).
 * pm_align_dtw_f32: x = -m[b, skip_first : len_b - skip_last, 0 : F_b] (N rows, M columns), cost[0][0] = 0, the other border
 *   cells +inf, cost[i][j] = x[i-1][j-1] + min(cost[i-1][j-1], cost[i-1][j], cost[i][j-1]) in fp32 with STRICT comparisons: the
 *   diagonal if it is below both others, else the cell above if it is below both others, else the cell to the left; back from
 *   (N, M) to (0, 0) in at most N + M moves whatever m holds.  start int32 (B, L) contiguous: the first frame of each row of the
 *   window on that path, -1 for every other row (all rows when N <= 0).  ws: pm_align_ws_bytes(B, L, S) bytes (2 bits per cell in
 *   8-byte words per row and 32 anti-diagonals), 8-byte aligned, no initial state.  L <= 448 (else PM_EUNSUPPORTED).
 * No atomics: a clip's outputs are bit-identical wherever it sits in the batch and whatever B is. */
int pm_align_lse_bf16(const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk, int64_t k_batch_stride,
                      const int32_t* heads, const int32_t* lengths, const int32_t* frames, float* lse, int64_t B, int64_t L,
                      int64_t S, int64_t n_sel, int64_t n_heads, void* stream);
int pm_align_matrix_bf16(const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk, int64_t k_batch_stride,
                         const int32_t* heads, const int32_t* lengths, const int32_t* frames, const float* lse, float* m,
                         int64_t ldm, int64_t m_batch_stride, int64_t B, int64_t L, int64_t S, int64_t n_sel, int64_t n_heads,
                         float inv_heads, int first, void* stream);
int pm_align_dtw_f32(const float* m, int64_t ldm, int64_t m_batch_stride, const int32_t* lengths, const int32_t* frames,
                     int32_t* start, void* ws, int64_t B, int64_t L, int64_t S, int64_t skip_first, int64_t skip_last, void* stream);
int64_t pm_align_ws_bytes(int64_t B, int64_t L, int64_t S);

/* ---- Variable-length (packed) encoder batches (csrc/varlen.hip, csrc/attention_bf16.hip; DESIGN.md "packed sequences").
 * B right-padded sequences run as one (T_total, d) matrix, T_total = sum(len_b).  cu_seqlens: int32 (B + 1) in DEVICE memory,
 * cu[0] = 0, non-decreasing; sequence b owns rows cu[b] .. cu[b + 1].  The caller guarantees that the packed operand holds
 * cu[B] rows; the padded side is protected by clamping len_b to [0, L].  Strides are in elements. */

/* Self-attention of every sequence with itself, head_dim 64, bf16: for rows i, j of sequence b,
 * o[cu[b] + i, h, :] = softmax_j(q[cu[b] + i, h, :] . k[cu[b] + j, h, :] / 8 [j <= i if causal]) v[cu[b] + j, h, :].
 * q / k / v / o: packed rows addressed base + row*stride_t + h*64 (column slices of one packed QKV projection are consumed in
 * place).  The tiled kernel of pm_attention_bf16 with per-sequence extents: the grid is B * H * ceil(max_len / 128) workgroups
 * (max_len >= every len_b; it sizes the grid and nothing else), a workgroup whose query block lies past its sequence returns
 * at once, and key tiles come from the sequence's own length.  A sequence of length 0 writes nothing; rows outside
 * 0 .. cu[B] are neither read nor written.  Per sequence the arithmetic is that of pm_attention_bf16's tiled kernel on that
 * sequence alone, whatever its position in the batch.  No bias, no cross-attention. */
int pm_attention_varlen_bf16(const void* q, int64_t q_stride_t, const void* k, int64_t k_stride_t, const void* v,
                             int64_t v_stride_t, void* o, int64_t o_stride_t, const int32_t* cu_seqlens, int64_t B,
                             int64_t H, int64_t max_len, int causal, void* stream);

/* pm_attention_varlen_bf16 plus an additive bias that depends on key - query alone (T5's relative-position bias), read from a
 * per-head distance table instead of a (B, H, L, L) one:
 *   bias(h, i, j) = rel_lut[h * lut_stride_h + clamp(j - i, -radius, radius) + radius]      fp32, natural-log units
 * with i, j positions inside the sequence.  rel_lut: device memory, 4-byte aligned, H rows of >= 2 * radius + 1 floats
 * (lut_stride_h >= 2 * radius + 1, in elements); 0 <= radius <= PM_RELBIAS_MAX_RADIUS (the head's table is staged in LDS
 * beside the K/V tiles).  Entries may be -inf (a masked distance); a row whose visible keys all carry -inf returns zeros, as
 * pm_attention_bias_bf16 does.  Both causal values.  Per sequence the arithmetic - and the bits - are those of
 * pm_attention_bias_bf16 on that sequence alone with the (1, H, len, len) table gathered from rel_lut. */
#define PM_RELBIAS_MAX_RADIUS 512
int pm_attention_varlen_relbias_bf16(const void* q, int64_t q_stride_t, const void* k, int64_t k_stride_t, const void* v,
                                     int64_t v_stride_t, void* o, int64_t o_stride_t, const int32_t* cu_seqlens, int64_t B,
                                     int64_t H, int64_t max_len, int causal, const float* rel_lut, int64_t lut_stride_h,
                                     int64_t radius, void* stream);

/* pm_embed_tokens into packed rows: out[cu[b] + t, :] = emb[tokens[b, t], :] + pos[t, :] for t < len_b.  tokens: int64 (B, L)
 * contiguous, right-padded (ids at t >= len_b are not read); emb: (V, d) of emb_dtype (PM_BF16 | PM_F32; an f32 table needs
 * out_dtype PM_F32); pos: f32 (>= L, d) or NULL; out: (cu[B], d) contiguous.  Ids are clamped to [0, V) like pm_embed_tokens. */
int pm_embed_tokens_varlen(const int64_t* tokens, const void* emb, int emb_dtype, const float* pos,
                           const int32_t* cu_seqlens, void* out, int out_dtype, int64_t B, int64_t L, int64_t d,
                           int64_t V, void* stream);

/* Plain row copies between the padded (B, L, d) layout (x_stride_b / x_stride_t, unit last stride) and the packed (cu[B], d)
 * layout, 16-byte accesses: d * elem_bytes and every stride in bytes must be multiples of 16, elem_bytes is 2 or 4.
 *   pm_rows_pack:      out[cu[b] + t] = x[b, t]                       for t < len_b (padded rows are not read)
 *   pm_rows_unpack:    out[b, t] = t < len_b ? x[cu[b] + t] : 0       for every t < L
 *   pm_rows_zero_tail: x[b, t] = 0                                    for len_b <= t < L, in place */
int pm_rows_pack(const void* x, int64_t x_stride_b, int64_t x_stride_t, const int32_t* cu_seqlens, void* out,
                 int64_t out_stride_t, int64_t B, int64_t L, int64_t d, int64_t elem_bytes, void* stream);
int pm_rows_unpack(const void* x, int64_t x_stride_t, const int32_t* cu_seqlens, void* out, int64_t out_stride_b,
                   int64_t out_stride_t, int64_t B, int64_t L, int64_t d, int64_t elem_bytes, void* stream);
int pm_rows_zero_tail(void* x, int64_t x_stride_b, int64_t x_stride_t, const int32_t* cu_seqlens, int64_t B, int64_t L,
                      int64_t d, int64_t elem_bytes, void* stream);

/* out[b, :] = mean of the rows cu[b] .. cu[b + 1] of x (packed, x_dtype PM_BF16 | PM_F32, row stride x_stride_t) -> f32 (B, d)
 * contiguous.  fp32 accumulation over the rows in order, one divide: the result is bit-determined (no atomics).  A sequence of
 * length 0 gives zeros.  d % 8 == 0 (bf16) / % 4 (f32); B <= 65535. */
int pm_segment_mean(const void* x, int64_t x_stride_t, int x_dtype, const int32_t* cu_seqlens, float* out, int64_t B,
                    int64_t d, void* stream);

/* ---- CTC heads of the wav2vec2 family (csrc/ctc.hip; DESIGN.md "CTC heads").  Frames are PACKED: clip b owns the rows
 * cu_frames[b] .. cu_frames[b + 1] (int32 (B + 1), device memory, cu[0] = 0, non-decreasing, cu[B] <= total_frames).  No atomics:
 * a clip's outputs are bit-identical wherever it sits in the batch and whatever B is.  Ids and lengths are clamped on the
 * device, so a bad one cannot fault; callers validate on the host.  Strides are in elements. */

/* Vocabulary projection + bias + log-softmax + arg-max in one pass over the hidden rows:
 *   x[m, v] = sum_k h[m, k] w[v, k] + bias[v]   (bf16 operands, fp32 accumulation on the MFMA, bias f32 (V) or NULL)
 *   logp[m, v] = x[m, v] - lse[m]               f32 (M, ldl >= V); columns V .. ldl are not written
 *   best[m] = the LOWEST index among the maxima of x[m, :V], best_logp[m] (or NULL) = logp[m, best[m]].
 * 2 <= V <= 256, K % 8 == 0, ldh / ldw % 8 == 0, h / w 16-byte aligned, any M >= 0.  A workgroup owns 64 rows and all V
 * columns: no second kernel, no workspace. */
int pm_ctc_head_bf16(const void* h, int64_t ldh, const void* w, int64_t ldw, const float* bias, float* logp, int64_t ldl,
                     int32_t* best, float* best_logp, int64_t M, int64_t V, int64_t K, void* stream);

/* Best-path decoding: per clip the arg-max sequence best[cu[b] ..] with repeats merged and `blank` removed.
 *   ids / start: int32 (B, Tmax): the emitted ids and the first frame of each, then -1;  n: int32 (B) their count.
 *   path_logp: f32 (B) = sum of best_logp over the clip's frames (thread i of 256 adds frames i, i + 256, .. in ascending order,
 *   a wave folds its partials with the xor butterfly 32 .. 1, the four wave sums are added in wave order); best_logp NULL <=>
 *   path_logp NULL.  A clip of 0 frames gives n = 0; a clip longer than Tmax is cut at Tmax. */
int pm_ctc_greedy(const int32_t* best, const int32_t* cu_frames, const float* best_logp, int32_t* ids, int32_t* n, int32_t* start,
                  float* path_logp, int64_t total_frames, int64_t B, int64_t Tmax, int64_t blank, void* stream);

/* loglik[b] = log p(targets[b, :U_b] | clip b): the CTC alpha recursion in log space over the S_b = 2 U_b + 1 extended labels
 * (state s takes s, s - 1, and s - 2 when its label is not the blank and differs from the label at s - 2; the result merges the
 * last two states).  logp: f32 (total_frames, ldl >= V) - pm_ctc_head_bf16's output or any f32 matrix; -inf entries are legal
 * and give no NaN (an all -inf merge is -inf).  targets: int32 (B, ldt >= Umax) right-padded, entries at u >= U_b are never
 * read; target_lengths: int32 (B).  An infeasible pair gives exactly -inf; U_b = 0 gives the all-blank path; a clip of 0
 * frames gives -inf.  Umax <= 511, 0 <= blank < V. */
int pm_ctc_forward_f32(const float* logp, int64_t ldl, const int32_t* cu_frames, const int32_t* targets, int64_t ldt,
                       const int32_t* target_lengths, float* loglik, int64_t total_frames, int64_t B, int64_t Umax, int64_t V,
                       int64_t blank, void* stream);

/* The same recursion with max in place of the merge (one kernel template) and the backtrace on the device.  Tie rule: stay if it
 * is not below the others, else s - 1 if it is not below s - 2, else s - 2; at the end the final blank state unless the last
 * label state is strictly above it.  Every score is one fp32 max followed by one fp32 add: the path is bit-determined by logp.
 *   start / stop: int32 (B, Umax): first frame and one past the last frame of each target token, -1 at u >= U_b;
 *   score: f32 (B).  An infeasible pair gives -1 everywhere and -inf.
 *   ws: pm_ctc_ws_bytes(B, Tmax, Umax) bytes, 16-byte aligned, no initial state (two bits per frame and state). Tmax >= every
 *   clip's frame count (longer clips are cut). */
int64_t pm_ctc_ws_bytes(int64_t B, int64_t Tmax, int64_t Umax);
int pm_ctc_viterbi_f32(const float* logp, int64_t ldl, const int32_t* cu_frames, const int32_t* targets, int64_t ldt,
                       const int32_t* target_lengths, int32_t* start, int32_t* stop, float* score, void* ws, int64_t total_frames,
                       int64_t B, int64_t Tmax, int64_t Umax, int64_t V, int64_t blank, void* stream);

#ifdef __cplusplus
}
#endif
#endif
