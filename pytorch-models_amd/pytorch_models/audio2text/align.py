"""Whisper token timestamps: cross-attention alignment + dynamic time warping (WhisperDecoder.align / Whisper.align).

The published method (Whisper's word-timestamp path), restated in DESIGN.md section 21 - OpenAI's package is not a dependency
and parity is against that restatement (tests/align_cases.py), not against their code:

  1. teacher-forced decoder pass; for every alignment head (l, h): q = head h of layers[l].ca.q_proj(ca_norm(x)) and
     k = head h of layers[l].ca.k_proj(memory), 64 wide;
  2. p[a, t, f] = softmax over f < F_b of q_t . k_f / 8, t < len_b;
  3. per head and frame column: (p - mean_t) / std_t (biased; a column whose std is exactly 0 normalises to 0 - the published
     code yields NaN there), median filter of width 7 along f with reflect padding, mean over the heads -> m (B, L, S);
  4. DTW on -m[skip_first : len_b - skip_last, : F_b] in fp32 with strict comparisons; start[b, t] = the first frame of token t.

bf16 parameters on a HIP device run csrc/align.hip (ops.align_lse / align_matrix / align_dtw): the (B, heads, L, S)
probabilities are never stored.  A CPU module with CPU inputs takes the plain-torch form below, in the module's dtype.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _cpu
from .._hip import ops
from ..transformer import MHA, _f32, _fused_attend, _fused_mlp, _wb, _xb


def default_heads(n_layers: int, n_heads: int) -> list:
    """Every head of the upper half of the decoder layers: the published fallback of a checkpoint without an alignment-head table."""
    return [(l, h) for l in range(n_layers // 2, n_layers) for h in range(n_heads)]


def _counts(v, n: int, lo: int, hi: int, default: int, name: str) -> list:
    if v is None:
        return [default] * n
    if isinstance(v, Tensor):
        v = v.tolist()
    vals = [int(v)] * n if isinstance(v, int) else [int(x) for x in v]
    if len(vals) != n or any(not lo <= x <= hi for x in vals):
        raise ValueError(f"{name} must hold {n} values in [{lo}, {hi}], got {vals}")
    return vals


def check_args(who: str, tokens: Tensor, memory: Tensor, n_layers: int, n_heads: int, heads, lengths, frames, skip_first, skip_last):
    """Shape and range errors of align(), raised before any launch -> (heads as a list of (layer, head), lengths, frames)."""
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise ValueError(f"{who}: tokens must be int64 (B, L), got {tokens.dtype} {tuple(tokens.shape)}")
    B, L = tokens.shape
    if memory.dim() != 3 or memory.shape[0] != B:
        raise ValueError(f"{who}: memory must be (B = {B}, S, d), got {tuple(memory.shape)}")
    S = memory.shape[1]
    if B < 1 or L < 1 or S < 4:
        raise ValueError(f"{who}: an empty batch is refused: needs at least one clip, one token and 4 frames (tokens {tuple(tokens.shape)}, memory {tuple(memory.shape)})")
    hs = default_heads(n_layers, n_heads) if heads is None else [tuple(int(v) for v in p) for p in heads]
    if not hs or any(len(p) != 2 or not (0 <= p[0] < n_layers and 0 <= p[1] < n_heads) for p in hs) or len(set(hs)) != len(hs):
        raise ValueError(f"{who}: heads must be distinct (layer, head) pairs with layer < {n_layers} and head < {n_heads}, got {hs}")
    for name, v in (("skip_first", skip_first), ("skip_last", skip_last)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{who}: {name} must be an int >= 0, got {v!r}")
    return hs, _counts(lengths, B, 1, L, L, f"{who}: lengths"), _counts(frames, B, 4, S, S, f"{who}: frames")


def align_gate(who: str, w: Tensor, head_dim: int, *inputs: Tensor) -> None:
    """Device and dtype rule of the kernel path: operands on one HIP device (the device error first), bf16 parameters, head dim 64."""
    ops.check_devices(w, *inputs)
    if w.dtype != torch.bfloat16:
        raise NotImplementedError(f"{who}: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda()); the alignment kernels "
                                  "read bf16 q / k projections, fp32 parameters are not aligned")
    if head_dim != 64:
        raise NotImplementedError(f"{who}: head dim 64 only (got {head_dim}): the alignment kernels are built for Whisper's heads")


def _by_layer(hs: list) -> dict:
    out: dict = {}
    for l, h in hs:
        out.setdefault(l, []).append(h)
    return out


def _walk(dec, h: Tensor, memory: Tensor, layers_wanted, fold) -> None:
    """The decoder's layers in order, as DecoderLayer.forward runs them; at a wanted layer, fold(l, q, layer.ca, memory) sees the
    cross-attention query projection (B, L, inner) that layer's attention consumes.  Stops behind the last wanted layer."""
    last = max(layers_wanted)
    for l, layer in enumerate(dec.layers):
        if l not in layers_wanted:
            h = layer(h, memory)
            continue
        if not layer.pre_norm or layer.ca is None or type(layer.ca).forward is not MHA.forward:
            raise NotImplementedError("align: plain pre-norm decoder layers with cross-attention only")
        x = _fused_attend(layer.sa, layer.sa_norm(h), None, True, h)
        xn = layer.ca_norm(x)
        fold(l, layer.ca.q_proj(xn), layer.ca, memory)
        if l == last:
            return
        x = _fused_attend(layer.ca, xn, memory, False, x)
        h = _fused_mlp(layer.mlp, layer.mlp_norm(x), x)


def median7_reflect(n: Tensor) -> Tensor:
    """Median of 7 along the last dim with reflect padding (index -i reads i, F - 1 + i reads F - 1 - i); F >= 4."""
    pad = torch.nn.functional.pad(n.unsqueeze(0), (3, 3), mode="reflect").squeeze(0)
    return pad.unfold(-1, 7, 1).sort(-1).values[..., 3]


def head_matrix_torch(q: Tensor, k: Tensor) -> Tensor:
    """One head, one clip, plain torch fp32: q (len, 64), k (F, 64) -> median-filtered normalised probabilities (len, F)."""
    p = torch.softmax(q.float() @ k.float().T * 0.125, -1)
    std, mean = torch.std_mean(p, 0, keepdim=True, unbiased=False)
    live = (std > 0) & (p.amax(0, keepdim=True) != p.amin(0, keepdim=True))  # equal rows: std is exactly 0 whatever the mean rounds to
    n = torch.where(live, (p - mean) / torch.where(live, std, torch.ones_like(std)), torch.zeros_like(p))
    return median7_reflect(n)


def dtw_start_torch(m: Tensor, skip_first: int, skip_last: int) -> Tensor:
    """m f32 (len, F) of one clip -> start int32 (len): the published fp32 DTW on -m[skip_first : len - skip_last], swept by
    anti-diagonals (the cells of one diagonal do not depend on each other), then the backtrace; -1 outside the window."""
    ln, M = m.shape
    start = torch.full((ln,), -1, dtype=torch.int32)
    N = ln - skip_first - skip_last
    if N <= 0:
        return start
    x = -m[skip_first : skip_first + N].float()
    inf = float("inf")
    cost = torch.full((N + 1, M + 1), inf, dtype=torch.float32)
    cost[0, 0] = 0.0
    trace = torch.full((N + 1, M + 1), 2, dtype=torch.int8)
    trace[:, 0] = 1
    trace[0, :] = 2
    for d in range(2, N + M + 1):
        i = torch.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        c = torch.where(t0, c0, torch.where(t1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = torch.where(t0, 0, torch.where(t1, 1, 2)).to(torch.int8)
    tr = trace.tolist()
    i, j = N, M
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            start[skip_first + i - 1] = j - 1
        t = tr[i][j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return start


def _align_cpu(dec, tokens, memory, hs, lens, frs, skip_first, skip_last, return_matrix):
    E = dec.token_embs.weight
    B, L = tokens.shape
    S = memory.shape[1]
    m = torch.zeros((B, L, S), dtype=torch.float32)
    by = _by_layer(hs)

    def fold(l, q, ca, mem):
        k = ca.k_proj(mem)
        for b in range(B):
            for h in by[l]:
                sl = slice(64 * h, 64 * h + 64)
                m[b, : lens[b], : frs[b]] += head_matrix_torch(q[b, : lens[b], sl], k[b, : frs[b], sl])

    _walk(dec, _cpu.embed_tokens(tokens, E, dec.pos_embs), memory.to(E.dtype), by, fold)
    m /= len(hs)
    start = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        start[b, : lens[b]] = dtw_start_torch(m[b, : lens[b], : frs[b]], skip_first, skip_last)
    return (start, m) if return_matrix else start


@torch.no_grad()
def align(dec, tokens: Tensor, memory: Tensor, *, lengths=None, frames=None, heads=None, skip_first: int = 0, skip_last: int = 0,
          return_matrix: bool = False):
    """WhisperDecoder.align (documented there)."""
    who = "WhisperDecoder.align"
    ops.no_capture(who, "uploads its counts and head tables and back-traces the path on the host")
    sa = dec.layers[0].sa
    hs, lens, frs = check_args(who, tokens, memory, len(dec.layers), sa.n_heads, heads, lengths, frames, skip_first, skip_last)
    w = dec.token_embs.weight
    if sa.head_dim != 64:
        raise NotImplementedError(f"{who}: head dim 64 only (got {sa.head_dim})")
    if _cpu.on_cpu(tokens, w) and not memory.is_cuda:
        return _align_cpu(dec, tokens, memory, hs, lens, frs, skip_first, skip_last, return_matrix)
    align_gate(who, w, sa.head_dim, tokens, memory)
    B, L = tokens.shape
    S = memory.shape[1]
    dev = tokens.device
    by = _by_layer(hs)
    # every upload before the first launch; nothing below waits for the device
    lens_d = ops.align_counts(lens, B, 1, L, f"{who}: lengths", dev)
    frs_d = ops.align_counts(frs, B, 4, S, f"{who}: frames", dev)
    heads_d = {l: torch.tensor(v, dtype=torch.int32).to(dev) for l, v in by.items()}
    m = torch.empty((B, L, S), dtype=torch.float32, device=dev)
    inner = sa.n_heads * 64
    first = [True]

    def fold(l, q, ca, mem):
        wkv, bkv = ca._pack("kv")  # the packed projection attend() itself uses; k is a view with row stride 2 * inner
        k = ops.linear(mem.reshape(-1, mem.shape[-1]), wkv, bkv).view(B, S, 2 * inner)[..., :inner]
        lse = ops.align_lse(q, k, heads_d[l], lens_d, frs_d)
        ops.align_matrix(q, k, heads_d[l], lens_d, frs_d, lse, m, 1.0 / len(hs), first[0])
        first[0] = False

    h0 = ops.embed_tokens(tokens, _wb(dec.token_embs, "E", w), _f32(dec, "pos", dec.pos_embs))  # as WhisperDecoder.hidden_rows
    _walk(dec, h0, _xb(memory), by, fold)
    start = ops.align_dtw(m, lens_d, frs_d, skip_first, skip_last)
    return (start, m) if return_matrix else start
