"""The CPU-device forms of the shared blocks, ViT and Whisper: plain torch on CPU tensors (BASELINE.json configs[0]: "ViT-Ti/16
... on the repo's CPU path (plumbing, no GPU)"; the reference's modules run on whatever device holds them).

Selected ONLY by ``device.type == "cpu"`` of BOTH the input and the parameters (`on_cpu`); a HIP tensor never comes here, and a
HIP call whose library is missing still raises (pytorch_models._hip.lib) - this is not a fallback of the HIP path.  Nothing
is imported from ``oracle/`` (that is test infrastructure).  The arithmetic follows the reference's module code line for line
in meaning (file:line cited per function) and is pinned to the reference's own vectors at the reference's own tolerances by
tests/test_cpu_device.py (tests/golden/vit.npz, blocks.npz, mha.npz, whisper.npz, audio.npz)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def on_cpu(x: Tensor, *params) -> bool:
    """True when the input AND every given parameter live on the CPU; mixed placements are an error, as everywhere."""
    ps = [p for p in params if p is not None]
    if x.device.type == "cpu":
        for p in ps:
            if p.device.type != "cpu":
                raise RuntimeError(f"pytorch_models: input on {x.device} but parameters on {p.device}; move both to one device")
        return True
    return False


_ACT = {
    "gelu": F.gelu,
    "approximate_gelu": lambda x: F.gelu(x, approximate="tanh"),
    "relu": F.relu,
    "silu": F.silu,
    "none": lambda x: x,
}


def linear(x: Tensor, w: Tensor, b: Tensor | None) -> Tensor:
    return F.linear(x.to(w.dtype), w, b)


def mha(m, q: Tensor, k, v, attn_bias, causal: bool, residual: Tensor | None) -> Tensor:
    """reference transformer.py:36-53: q/k/v projections, heads split by unflatten + transpose, SDPA, merge, out_proj."""
    k = q if k is None else k
    v = k if v is None else v
    dt = m.q_proj.weight.dtype
    qh = F.linear(q.to(dt), m.q_proj.weight, m.q_proj.bias).unflatten(-1, (m.n_heads, m.head_dim)).transpose(-2, -3)
    kh = F.linear(k.to(dt), m.k_proj.weight, m.k_proj.bias).unflatten(-1, (m.n_heads, m.head_dim)).transpose(-2, -3)
    vh = F.linear(v.to(dt), m.v_proj.weight, m.v_proj.bias).unflatten(-1, (m.n_heads, m.head_dim)).transpose(-2, -3)
    if attn_bias is not None and attn_bias.dtype != torch.bool:
        attn_bias = attn_bias.to(dt)
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_bias, 0.0, causal)
    y = F.linear(o.transpose(-2, -3).flatten(-2), m.out_proj.weight, m.out_proj.bias)
    return y if residual is None else residual.to(dt) + y


def mha_packed(m, x: Tensor, seq, causal: bool, residual: Tensor | None) -> Tensor:
    """MHA.attend_packed on the CPU: `mha` on each sequence's rows cu[b] .. cu[b + 1] of the packed (T_total, d) input."""
    dt = m.q_proj.weight.dtype
    out, r0 = [], 0
    for n in seq.lengths:
        if n:
            out.append(mha(m, x[r0 : r0 + n][None], None, None, None, causal, None)[0])
        r0 += n
    y = torch.cat(out, 0) if out else x.new_zeros((0, m.out_proj.out_features), dtype=dt)
    return y if residual is None else residual.to(dt) + y


def mlp(m, x: Tensor, residual: Tensor | None) -> Tensor:
    """reference transformer.py:56-67."""
    dt = m.linear1.weight.dtype
    h = _ACT[m.act_name](F.linear(x.to(dt), m.linear1.weight, m.linear1.bias))
    y = F.linear(h, m.linear2.weight, m.linear2.bias)
    return y if residual is None else residual.to(dt) + y


def vit_tokens(vit, imgs: Tensor) -> Tensor:
    """reference image/vit.py:78-81: patch_embed -> flatten -> + pe -> cls token prepended (batch-broadcast: SURVEY F1)."""
    dt = vit.patch_embed.weight.dtype
    out = F.conv2d(imgs.to(dt), vit.patch_embed.weight, vit.patch_embed.bias, stride=vit.patch_embed.stride).flatten(2).transpose(1, 2)
    if out.shape[1] != vit.pe.shape[1]:
        raise ValueError(f"ViT: pe holds {vit.pe.shape[1]} positions, the image has {out.shape[1]} patches; call resize_pe first")
    out = out + vit.pe
    if vit.cls_token is not None:
        out = torch.cat([vit.cls_token.expand(out.shape[0], 1, -1), out], 1)
    return out


def whisper_stem(enc, x: Tensor) -> Tensor:
    """reference audio2text/whisper.py:29-33: conv stem, transpose to (B, T, d), + pos_embs."""
    dt = enc.stem[0].weight.dtype
    y = enc.stem(x.to(dt)).transpose(1, 2)
    return y + enc.pos_embs[: y.shape[1]].to(dt)


def embed_tokens(tok: Tensor, E: Tensor, pos: Tensor | None) -> Tensor:
    """reference whisper.py:48 / text models: token embedding (+ learned positions)."""
    y = F.embedding(tok, E)
    return y if pos is None else y + pos[: tok.shape[-1]].to(E.dtype)


def spectrogram(x: Tensor, window: Tensor, n_fft: int, hop: int) -> Tensor:
    """reference audio/spectrogram.py:15-16: centred STFT (reflect padding) -> power spectrogram."""
    return torch.stft(x, n_fft, hop, window=window, return_complex=True).abs().square()


def mel_spectrogram(x: Tensor, window: Tensor, filters: Tensor, n_fft: int, hop: int) -> Tensor:
    """reference audio/spectrogram.py:44-45."""
    return filters @ spectrogram(x, window, n_fft, hop)


def whisper_log_mel(x: Tensor, window: Tensor, filters: Tensor) -> Tensor:
    """reference audio2text/whisper.py:143-148: last frame dropped, log10, floored at the PER-SAMPLE max - 8, (x + 4) / 4
    (the -inf of an all-zero clip propagates exactly as the reference's does)."""
    y = mel_spectrogram(x, window, filters, 400, 160)[..., :-1]
    y = y.clamp(0).log10()
    y = y.maximum(y.flatten(-2).max(-1, keepdim=True)[0].unsqueeze(-1) - 8)
    return (y + 4) / 4


# ---- variable-length batches (lengths=): the packed layout of the HIP path in plain torch
def rows_pack(x: Tensor, lengths) -> Tensor:
    """padded (B, L, ...) -> packed (sum(lengths), ...): the first lengths[b] rows of every sample, in order."""
    return torch.cat([x[b, :n] for b, n in enumerate(lengths)], 0)


def rows_unpack(x: Tensor, lengths, L: int) -> Tensor:
    """packed (sum(lengths), d) -> padded (B, L, d), zeros past each length."""
    out = x.new_zeros((len(lengths), L, x.shape[-1]))
    r0 = 0
    for b, n in enumerate(lengths):
        out[b, :n] = x[r0 : r0 + n]
        r0 += n
    return out


def segment_mean(x: Tensor, lengths) -> Tensor:
    """packed (sum(lengths), d) -> fp32 (B, d): the mean of each sequence's rows (zeros for a length of 0)."""
    out = torch.zeros((len(lengths), x.shape[-1]), dtype=torch.float32)
    r0 = 0
    for b, n in enumerate(lengths):
        if n:
            out[b] = x[r0 : r0 + n].float().mean(0)
        r0 += n
    return out


def w2v_features(m, x: Tensor) -> Tensor:
    """reference audio/wav2vec2.py:19-39, 66-68 for the layer-norm stem: conv -> LayerNorm over channels -> GELU per stem layer,
    then the LayerNorm [+ Linear] projection; waveform (B, n) -> (B, T, d).  Serves Wav2Vec2.forward(x, lengths=) on the CPU."""
    dt = m.proj[0].weight.dtype
    h = x.to(dt)[:, None, :]
    for blk in m.feature_encoder:
        conv, norm = blk[0], blk[2]
        h = F.conv1d(h, conv.weight, conv.bias, conv.stride)
        h = F.layer_norm(h.transpose(1, 2), norm.normalized_shape, norm.weight, norm.bias, norm.eps).transpose(1, 2)
        h = F.gelu(h)
    h = h.transpose(1, 2)
    for layer in m.proj:
        h = layer(h)
    return h


def w2v_positional(m, h: Tensor) -> Tensor:
    """reference audio/wav2vec2.py:80: x + GELU(grouped conv(pad(x))) on time-major (B, T, d)."""
    conv = m.pe_conv[1]
    pad = m.pe_conv[0].padding
    y = F.conv1d(F.pad(h.transpose(1, 2), (pad[0], pad[1])), conv.weight, conv.bias, conv.stride, groups=conv.groups)
    return h + F.gelu(y).transpose(1, 2)


# ---- CTC heads (audio/ctc.py): the four ops of csrc/ctc.hip on packed frames, plain torch / numpy
def ctc_head(h: Tensor, w: Tensor, b: Tensor | None):
    """(M, K) rows -> (logp f32 (M, V), best int32 (M), best_logp f32 (M)): log_softmax of the fp32 logits, the lowest arg-max."""
    x = F.linear(h.float(), w.float(), None if b is None else b.float())  # fp32 logits also for a bf16 module, as the kernel keeps them
    logp = torch.log_softmax(x, -1)
    V = x.shape[-1]
    idx = torch.arange(V).expand_as(x)
    best = torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values
    return logp, best.to(torch.int32), logp.gather(1, best[:, None])[:, 0]


def ctc_greedy(best: Tensor, frames, L: int, best_logp: Tensor | None, blank: int):
    """packed arg-max ids -> (ids (B, L), n (B), start (B, L), path_logp (B) | None): repeats merged, blanks removed, then -1."""
    B = len(frames)
    ids = torch.full((B, L), -1, dtype=torch.int32)
    start = torch.full((B, L), -1, dtype=torch.int32)
    n = torch.zeros(B, dtype=torch.int32)
    path = torch.zeros(B, dtype=torch.float32) if best_logp is not None else None
    r0 = 0
    for b, T in enumerate(frames):
        a = best[r0 : r0 + T]
        keep = a != blank
        keep[1:] &= a[1:] != a[:-1]
        f = torch.nonzero(keep)[:, 0]
        n[b] = f.numel()
        ids[b, : f.numel()] = a[f]
        start[b, : f.numel()] = f.to(torch.int32)
        if path is not None:
            path[b] = best_logp[r0 : r0 + T].sum()
        r0 += T
    return ids, n, start, path


def _ctc_ext(target, blank: int):
    ext = [blank]
    for t in target:
        ext += [int(t), blank]
    return ext


def ctc_forward(logp: Tensor, frames, targets: Tensor, target_lengths, blank: int) -> Tensor:
    """log p(target_b | clip_b) by the alpha recursion in log space (float64 inside, f32 out); -inf for an infeasible pair."""
    import numpy as np

    lp = logp.double().numpy()
    out = np.full(len(frames), -np.inf)
    r0 = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for b, T in enumerate(frames):
            ext = np.array(_ctc_ext(targets[b, : int(target_lengths[b])].tolist(), blank))
            S = len(ext)
            skip = np.zeros(S, dtype=bool)
            skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
            a = np.full(S, -np.inf)
            a[:2] = lp[r0, ext[:2]]
            for t in range(1, T):
                p1 = np.concatenate(([-np.inf], a[:-1]))
                p2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], a[:-2]))[:S], -np.inf)
                m = np.maximum(a, np.maximum(p1, p2))
                mm = np.where(np.isfinite(m), m, 0.0)
                a = np.where(np.isfinite(m), mm + np.log(np.exp(a - mm) + np.exp(p1 - mm) + np.exp(p2 - mm)), -np.inf) + lp[r0 + t, ext]
            out[b] = np.logaddexp(a[-1], a[-2]) if S > 1 else a[-1]
            r0 += T
    return torch.from_numpy(out).float()


def ctc_viterbi(logp: Tensor, frames, targets: Tensor, target_lengths, blank: int):
    """The best CTC path in fp32 (one max, one add per state and frame).  Ties: stay if not below the others, else s - 1 if not
    below s - 2, else s - 2; at the end the final blank unless the last label state is strictly above it.
    -> (start (B, Umax), stop (B, Umax), score (B)); -1 / -inf for an infeasible pair."""
    import numpy as np

    lp = logp.float().numpy()
    B, Umax = len(frames), targets.shape[1]
    start = np.full((B, Umax), -1, dtype=np.int32)
    stop = np.full((B, Umax), -1, dtype=np.int32)
    score = np.full(B, -np.inf, dtype=np.float32)
    ninf = np.float32(-np.inf)
    r0 = 0
    for b, T in enumerate(frames):
        ext = np.array(_ctc_ext(targets[b, : int(target_lengths[b])].tolist(), blank))
        S = len(ext)
        skip = np.zeros(S, dtype=bool)
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        v = np.full(S, ninf, dtype=np.float32)
        v[:2] = lp[r0, ext[:2]]
        bp = np.zeros((T, S), dtype=np.int8)
        for t in range(1, T):
            p1 = np.concatenate(([ninf], v[:-1]))
            p2 = np.where(skip, np.concatenate(([ninf, ninf], v[:-2]))[:S], ninf)
            stay = (v >= p1) & (v >= p2)
            one = ~stay & (p1 >= p2)
            bp[t] = np.where(stay, 0, np.where(one, 1, 2))
            v = (np.where(stay, v, np.where(one, p1, p2)) + lp[r0 + t, ext]).astype(np.float32)
        s = S - 1
        if S > 1 and v[S - 2] > v[S - 1]:
            s = S - 2
        if v[s] > ninf:
            score[b] = v[s]
            for t in range(T - 1, -1, -1):
                if s & 1:
                    u = s >> 1
                    if stop[b, u] < 0:
                        stop[b, u] = t + 1
                    start[b, u] = t
                s -= int(bp[t, s]) if t else 0
        r0 += T
    return torch.from_numpy(start), torch.from_numpy(stop), torch.from_numpy(score)
