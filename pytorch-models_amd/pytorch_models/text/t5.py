"""T5 v1.1 / Flan-T5 / mT5 on MI355X: drop-in for /root/reference pytorch_models/text/t5.py (LayerNorm, GEGLU,
RelativePositionBias, T5Block, T5Encoder, T5Decoder, T5Model; same parameter names, so a t5x checkpoint converted the
reference's way loads unchanged).

    LayerNorm (no centring, no bias)  -> pm_rmsnorm
    self- / cross-attention           -> transformer.MHA (packed projections, pm_attention_bias_bf16 with the relative-
                                         position bias; the decoder's causal mask is the kernel's own, not a -1e10 table),
                                         residual add in the out_proj epilogue
    GEGLU + output projection         -> ONE pm_linear_bf16 over the packed [w; v] weight, pm_geglu, pm_linear_bf16 (+residual)
    token embedding, classifier       -> pm_embed_tokens (no positional term), pm_linear_bf16 (fp32 logits)

The bucket table of RelativePositionBias is index arithmetic on the host (as in the reference, t5.py:49-70), cached per
length; the (heads, L, L) bias is gathered from the parameter on the device.  Inference only; no CPU path.

Right-padded source batches (encode(x, lengths), forward / score(..., src_lengths=), generate(..., packed=True)) run the encoder
on the valid rows only (forward_packed): the bias then comes from RelativePositionBias.lut, an (heads, 2 * max_distance + 1) table
by distance that pm_attention_varlen_relbias_bf16 reads inside the kernel, and no (heads, L, L) tensor exists on that path."""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from .._hip import ops
from ..transformer import MHA, Linear, _f32, _wb, derived, require_bf16_params


class LayerNorm(nn.Module):
    """x * rsqrt(mean(x^2) + eps) * weight (t5.py:15-25); statistics in fp32."""

    def __init__(self, dim: int, eps: float = 1e-5) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.dim = dim
        self.eps = eps

    def forward(self, x: Tensor, out_dtype: torch.dtype | None = None) -> Tensor:
        if not x.is_cuda:
            raise RuntimeError("T5 LayerNorm: HIP devices only (no CPU path)")
        y = ops.rmsnorm(x.reshape(-1, x.shape[-1]), _f32(self, "g", self.weight), self.eps, out_dtype)
        return y.view(*x.shape)


class GEGLU(nn.Module):
    """gelu_tanh(w x) * (v x) (t5.py:29-38): one GEMM over the stacked weight, then the gate kernel."""

    def __init__(self, dim: int, mlp_dim: int) -> None:
        super().__init__()
        self.w = Linear(dim, mlp_dim, False)
        self.v = Linear(dim, mlp_dim, False)
        self.act = nn.GELU(approximate="tanh")

    def _packed(self) -> Tensor:
        return derived(self, "wv", (self.w.weight, self.v.weight),
                       lambda: torch.cat([self.w.weight.detach(), self.v.weight.detach()], 0).to(torch.bfloat16).contiguous())

    def forward(self, x: Tensor) -> Tensor:
        if not x.is_cuda:
            raise RuntimeError("GEGLU: HIP devices only (no CPU path)")
        xb = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        h = ops.linear(xb.reshape(-1, x.shape[-1]), self._packed(), None)
        return ops.geglu(h).view(*x.shape[:-1], h.shape[-1] // 2)


class RelativePositionBias(nn.Module):
    def __init__(self, n_heads: int, n_buckets: int = 32, max_distance: int = 128) -> None:
        super().__init__()
        self.n_buckets = n_buckets
        self.max_distance = max_distance
        self.bias = nn.Parameter(torch.zeros(n_heads, n_buckets))

    def buckets(self, length: int, bidirection: bool) -> Tensor:
        """(L, L) int64 bucket ids, key position minus query position binned: exact below n/2, logarithmic up to
        max_distance, clipped beyond; separate halves for the two directions when bidirectional (t5.py:49-70)."""
        idx = torch.arange(length)
        rel = idx[None, :] - idx[:, None]
        if bidirection:
            n = self.n_buckets // 2
            offset = (rel > 0).long() * n
            rel = rel.abs()
        else:
            n = self.n_buckets
            offset = torch.zeros_like(rel)
            rel = (-rel).clamp(min=0)
        exact = n // 2
        scale = (n - exact) / math.log(self.max_distance / exact)
        far = exact + (torch.log(rel / exact + torch.finfo(torch.float32).eps) * scale).long()
        far = far.clamp(max=n - 1)
        return torch.where(rel < exact, rel, far) + offset

    def forward(self, length: int, bidirection: bool) -> Tensor:
        cache = self.__dict__.setdefault("_pm_buckets", {})
        key = (length, bidirection, self.bias.device)
        if key not in cache:
            cache[key] = self.buckets(length, bidirection).to(self.bias.device)
        return self.bias[:, cache[key]]  # (heads, L, L)

    def lut(self, bidirection: bool) -> Tensor:
        """The same bias by distance: fp32 (heads, 2 R + 1), R = max_distance, lut[:, d + R] = the bias of key - query = d
        clamped to [-R, R] - the bucket depends on the distance alone and no longer changes once |d| >= max_distance, so this
        table holds all of forward(L, bidirection) for every L.  One-sided: d > 0 holds the bucket-0 value, as the dense table
        does above its diagonal.  Gathered from the parameter with buckets() itself; a derived value per direction, rebuilt
        when the parameter changes (in place, storage, dtype or device).  Works on CPU tensors."""
        R = self.max_distance

        def build():
            b = self.buckets(R + 1, bidirection)  # b[q, k]
            row = torch.cat([b[R, :R], b[0]])  # d = -R .. -1 seen from query R, d = 0 .. R seen from query 0
            return self.bias.detach().float()[:, row.to(self.bias.device)].contiguous()

        return derived(self, f"lut{int(bool(bidirection))}", (self.bias,), build)


class T5Block(nn.Module):
    def __init__(self, dim: int, n_heads: int, mlp_dim: int, dropout: float = 0.0, cross_attn: bool = False) -> None:
        super().__init__()
        self.sa_norm = LayerNorm(dim)
        self.sa = MHA(dim, n_heads=n_heads, head_dim=64, bias=False, dropout=dropout)
        self.ca_norm = LayerNorm(dim) if cross_attn else None
        self.ca = MHA(dim, n_heads=n_heads, head_dim=64, bias=False, dropout=dropout) if cross_attn else None
        self.mlp_norm = LayerNorm(dim)
        self.mlp = nn.Sequential(GEGLU(dim, mlp_dim), nn.Dropout(dropout), Linear(mlp_dim, dim, False), nn.Dropout(dropout))

    def forward(self, x: Tensor, memory: Tensor | None = None, attn_bias: Tensor | None = None, causal: bool = False,
                memory_bias: Tensor | None = None) -> Tensor:
        """``memory_bias``: additive f32 bias of the cross-attention, broadcastable to (B, H, L, S) (a key mask of padded sources)."""
        x = self.sa.attend(self.sa_norm(x), attn_bias=attn_bias, causal=causal, residual=x)
        if self.ca is not None:
            x = self.ca.attend(self.ca_norm(x), memory, attn_bias=memory_bias, residual=x)
        g = self.mlp[0](self.mlp_norm(x))
        wo = self.mlp[2]
        y = ops.linear(g.reshape(-1, g.shape[-1]), _wb(wo, "w", wo.weight), None, resid=x.reshape(-1, x.shape[-1]), out_dtype=x.dtype)
        return y.view(*x.shape)

    def forward_packed(self, x: Tensor, seq: "ops.SeqLens", rel_lut: Tensor, radius: int) -> Tensor:
        """The encoder block on packed rows (T_total, d) of a ragged batch (ops.seq_lens): every stage but the attention is
        row-wise, the attention is MHA.attend_packed with the relative-position bias read by distance from ``rel_lut``."""
        if self.ca is not None:
            raise NotImplementedError("T5Block.forward_packed: encoder blocks only (no cross-attention on packed rows)")
        x = self.sa.attend_packed(self.sa_norm(x), seq, residual=x, rel_lut=rel_lut, radius=radius)
        g = self.mlp[0](self.mlp_norm(x))
        wo = self.mlp[2]
        return ops.linear(g, _wb(wo, "w", wo.weight), None, resid=x, out_dtype=x.dtype)


class T5Encoder(nn.Module):
    def __init__(self, dim: int, n_heads: int, n_layers: int, mlp_dim: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.in_drop = nn.Dropout(dropout)
        self.attn_bias = RelativePositionBias(n_heads)
        self.layers = nn.Sequential(*[T5Block(dim, n_heads, mlp_dim, dropout, False) for _ in range(n_layers)])
        self.norm = LayerNorm(dim)
        self.out_drop = nn.Dropout(dropout)

    def forward(self, x: Tensor) -> Tensor:
        require_bf16_params(self, "T5Encoder")
        bias = self.attn_bias(x.shape[-2], bidirection=True)
        for layer in self.layers:
            x = layer(x, attn_bias=bias)
        return self.norm(x)

    def forward_packed(self, x: Tensor, seq: "ops.SeqLens") -> Tensor:
        """forward on the packed rows (T_total, d) of a ragged batch: no padded row, no (H, L, L) bias table - every layer reads
        the (H, 2 * max_distance + 1) distance table inside pm_attention_varlen_relbias_bf16."""
        require_bf16_params(self, "T5Encoder.forward_packed")
        rp = self.attn_bias
        if rp.max_distance > ops.RELBIAS_MAX_RADIUS:
            raise NotImplementedError(f"T5Encoder.forward_packed: max_distance {rp.max_distance} exceeds the {ops.RELBIAS_MAX_RADIUS} the "
                                      "packed attention kernel stages per head (PM_RELBIAS_MAX_RADIUS); run without lengths")
        lut = rp.lut(True)
        for layer in self.layers:
            x = layer.forward_packed(x, seq, lut, rp.max_distance)
        return self.norm(x)


class T5Decoder(nn.Module):
    def __init__(self, dim: int, n_heads: int, n_layers: int, mlp_dim: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.in_drop = nn.Dropout(dropout)
        self.attn_bias = RelativePositionBias(n_heads)
        self.layers = nn.Sequential(*[T5Block(dim, n_heads, mlp_dim, dropout, True) for _ in range(n_layers)])
        self.norm = LayerNorm(dim)
        self.out_drop = nn.Dropout(dropout)

    def forward(self, x: Tensor, memory: Tensor, memory_bias: Tensor | None = None) -> Tensor:
        """``memory_bias``: f32 (B, 1, 1, S) additive key mask of the cross-attention (-inf at padded source positions).  The
        bias kernel takes one row per query (it refuses a query stride below S), so the mask is expanded here to a contiguous
        (B, 1, L, S) copy - B * L * S * 4 bytes per call, shared by the layers."""
        require_bf16_params(self, "T5Decoder")
        bias = self.attn_bias(x.shape[-2], bidirection=False)  # + the causal mask, applied inside the attention kernel
        if memory_bias is not None:  # the bias kernel wants one row per query: expanded once here, not once per layer
            memory_bias = memory_bias.float().expand(memory.shape[0], 1, x.shape[-2], memory.shape[-2]).contiguous()
        for layer in self.layers:
            x = layer(x, memory, attn_bias=bias, causal=True, memory_bias=memory_bias)
        return self.norm(x)


_SIZES = dict(small=(512, 6, 8, 1024), base=(768, 12, 12, 2048), large=(1024, 16, 24, 2816), xl=(2048, 32, 24, 5120),
              xxl=(4096, 64, 24, 10240))


class T5Model(nn.Module):
    def __init__(self, vocab_size: int, dim: int, n_heads: int, n_layers: int, mlp_dim: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.token_embs = nn.Embedding(vocab_size, dim)
        self.encoder = T5Encoder(dim, n_heads, n_layers, mlp_dim, dropout)
        self.decoder = T5Decoder(dim, n_heads, n_layers, mlp_dim, dropout)
        self.classifier = Linear(dim, vocab_size, False)

    def _embed(self, x: Tensor) -> Tensor:
        E = _wb(self.token_embs, "E", self.token_embs.weight)
        return ops.embed_tokens(x.reshape(-1, x.shape[-1]), E, None).view(*x.shape, E.shape[1])

    def encode(self, x: Tensor, lengths=None) -> Tensor:
        """Source ids (..., S) -> memory (..., S, d).  ``lengths`` (B,), a list or an integer tensor with 0 <= len_b <= S, marks a
        right-padded (B, S) batch: the encoder then runs on the sum(len_b) valid rows only (ops.embed_tokens_varlen,
        T5Encoder.forward_packed, ops.rows_unpack) - row b on [:len_b] is what encode returns for x[b:b+1, :len_b], rows past
        len_b are exactly zero and the ids there are never read."""
        if lengths is None:
            return self.encoder(self._embed(x))
        require_bf16_params(self, "T5Model.encode")
        if not isinstance(x, Tensor) or x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError("T5Model.encode: with lengths, x must be int64 (B, S), right-padded")
        return self._encode_packed(x, ops.seq_lens(lengths, x.shape[1], x.device))

    def _encode_packed(self, x: Tensor, seq: "ops.SeqLens") -> Tensor:
        E = _wb(self.token_embs, "E", self.token_embs.weight)
        if seq.B != x.shape[0]:
            raise ValueError(f"T5Model.encode: {seq.B} lengths for {x.shape[0]} rows")
        if seq.total == 0:
            ops.check_devices(E, x)
            return torch.zeros(*x.shape, E.shape[1], dtype=torch.bfloat16, device=E.device)
        h = ops.embed_tokens_varlen(x, E, None, seq)
        return ops.rows_unpack(self.encoder.forward_packed(h, seq), seq)

    def _encode_src(self, x: Tensor, src_lengths, who: str):
        """(memory, cross-attention key mask) of a right-padded source batch: the packed encoder and an f32 (B, 1, 1, S) table
        with -inf at s >= src_lengths[b].  A row without a source token has no key to attend to and is refused."""
        require_bf16_params(self, who)
        if not isinstance(x, Tensor) or x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError(f"{who}: with src_lengths, x must be int64 (B, S), right-padded")
        seq = ops.seq_lens(src_lengths, x.shape[1], x.device, lo=1)  # ValueError on a length of 0; the one upload of cu_seqlens
        memory = self._encode_packed(x, seq)
        S = x.shape[1]
        dead = torch.arange(S, device=x.device)[None, :] >= (seq.cu[1:] - seq.cu[:-1])[:, None]
        mask = torch.zeros(dead.shape, dtype=torch.float32, device=x.device).masked_fill_(dead, float("-inf"))
        return memory, mask[:, None, None, :]

    def decode(self, x: Tensor, memory: Tensor, memory_bias: Tensor | None = None) -> Tensor:
        h, W = self.hidden_rows(x, memory, memory_bias)
        return ops.linear(h.reshape(-1, h.shape[-1]), W, None, out_dtype=torch.float32).view(*x.shape, W.shape[0])

    def hidden_rows(self, x: Tensor, memory: Tensor, memory_bias: Tensor | None = None):
        """(hidden rows (..., L, d) bf16, classifier weights (V, d) bf16): what decode's last GEMM and score's kernel both read."""
        h = self.decoder(self._embed(x), memory) if memory_bias is None else self.decoder(self._embed(x), memory, memory_bias)
        return h, _wb(self.classifier, "w", self.classifier.weight)

    @torch.no_grad()
    def score(self, x: Tensor, targets: Tensor, lengths=None, *, src_lengths=None, return_argmax: bool = False):
        """Teacher-forced scoring in O(B L) memory: source ids x (B, S) and decoder input ids targets (B, L) int64 - exactly what
        forward takes - -> (B, L - 1) fp32 with out[b, t] = log p(targets[b, t + 1] | targets[b, : t + 1], x[b]).  ``lengths``
        (B,), 1 <= len_b <= L, marks right-padded decoder ids: positions with t + 1 >= len_b are ignored and return 0, so
        out.sum(-1) is the sequence log-likelihood.  ``src_lengths`` (B,), 1 <= len_b <= S, marks right-padded source ids: the
        packed encoder runs and the cross-attention masks the keys past len_b, so row b is score on x[b:b+1, :len_b].
        ``return_argmax``: also the (B, L - 1) int64 greedy predictions.  bf16
        parameters on a HIP device; projection, log-softmax and gather are one kernel (ops.lm_score), the (B, L, vocab) logits
        are never stored."""
        from .gpt2 import score_gate, score_rows, score_targets

        require_bf16_params(self, "T5Model.score")  # forward's own refusals (CPU model, fp32 parameters), in forward's order
        score_gate("T5Model.score", self.classifier.weight, x, targets)
        score_targets(targets, lengths, "T5Model.score")  # shape and lengths errors before any launch
        if src_lengths is None:
            h, W = self.hidden_rows(targets, self.encode(x))
        else:
            h, W = self.hidden_rows(targets, *self._encode_src(x, src_lengths, "T5Model.score"))
        return score_rows(h, W, targets, lengths, return_argmax, "T5Model.score")

    def forward(self, x: Tensor, targets: Tensor, src_lengths=None) -> Tensor:
        """token ids (..., S), (..., L) int64 -> logits (..., L, vocab) fp32 (t5.py:144-151).  ``src_lengths`` (B,),
        1 <= len_b <= S: x is a right-padded (B, S) batch (see score)."""
        if src_lengths is None:
            return self.decode(targets, self.encode(x))
        return self.decode(targets, *self._encode_src(x, src_lengths, "T5Model.forward"))

    @torch.no_grad()
    def generate_ids(self, input_ids: Tensor, max_tokens: int = 100, pad_id: int = 0, eos_id: int = 1) -> Tensor:
        """The loop of the reference's T5Generator.generate (t5.py:213-227) on token ids, one sequence: start from the pad
        id, append the arg-max of the last position until eos or max_tokens; the encoder runs once."""
        memory = self.encode(input_ids.view(1, -1))
        out = [pad_id]
        while len(out) < max_tokens:
            logits = self.decode(torch.tensor([out], device=input_ids.device), memory)
            out.append(int(logits[0, -1].argmax()))
            if out[-1] == eos_id:
                break
        return torch.tensor(out, device=input_ids.device)

    @torch.no_grad()
    def generate(self, input_ids: Tensor, *, lengths=None, max_new_tokens: int = 100, pad_id: int = 0, eos_id: int = 1,
                 decoder_prompt: Tensor | None = None, graph: bool = True, return_logits: bool = False, packed: bool = False):
        """Batched greedy generation with a KV cache (text/t5_generate.py over csrc/decode_t5.hip): the loop of generate_ids per
        row of a right-padded batch.  input_ids int64 (B, S); lengths (B,) tensor or list, None = every row is full;
        decoder_prompt int64 (B, P), teacher-forced, default one column of pad_id.  Returns ids (B, P + max_new_tokens) int64 and
        out_lengths (B,) int64 - a row that has produced eos_id emits pad_id from then on and its length counts up to and
        including the eos (eos_id < 0 never stops) - and with return_logits the fp32 last-position logits of every step,
        (B, P + max_new_tokens - 1, vocab).  graph=True captures one step into a HIP graph and replays it; graph=False issues
        the same launches eagerly.  packed=True with lengths runs the encoder on the valid source rows only (encode(x, lengths):
        no (B, H, S, S) bias table); the default keeps the dense-table encoder.  bf16 parameters, at most 64 sequences, d_model <= 1024 (small / base / large)."""
        from .t5_generate import generate

        return generate(self, input_ids, lengths=lengths, max_new_tokens=max_new_tokens, pad_id=pad_id, eos_id=eos_id,
                        decoder_prompt=decoder_prompt, graph=graph, return_logits=return_logits, packed=packed)

    @staticmethod
    def from_t5x(model_tag: str, *, pretrained: bool = False, **kwargs) -> "T5Model":
        variant, size = model_tag.split("-")
        dim, n_heads, n_layers, mlp_dim = _SIZES[size]
        vocab_size = 250112 if variant.startswith("mt5") else 32128
        m = T5Model(vocab_size, dim, n_heads, n_layers, mlp_dim, **kwargs)
        if pretrained:
            raise NotImplementedError(
                "T5Model.from_t5x(pretrained=True) streams a t5x checkpoint over HTTP in the reference; this build has no "
                "network: construct with pretrained=False and call load_t5x_checkpoint(dict of the flattened t5x tensors).")
        return m

    @torch.no_grad()
    def load_t5x_checkpoint(self, ckpt: dict) -> None:
        """Flattened t5x ``target`` tensors (name -> array, e.g. what the reference caches under checkpoints/) into this
        model: kernels are stored (in, out) and transposed here; the query / key kernels are scaled by 64^(1/4) each
        because T5 attention has no 1/sqrt(head_dim) while the attention kernel applies one (t5.py:169-176)."""
        sd = {}
        for k, v in ckpt.items():
            v = torch.as_tensor(v)
            if k.endswith("kernel"):
                v = v.T
            if k.endswith(("query.kernel", "key.kernel")):
                v = v * 64**0.25
            sd[_rename_key(k)] = v
        self.load_state_dict(sd)


_RENAMES = (
    ("token_embedder.embedding", "token_embs.weight"), ("decoder.logits_dense.kernel", "classifier.weight"),
    (".encoder_norm.scale", ".norm.weight"), (".decoder_norm.scale", ".norm.weight"),
    (".relpos_bias.rel_embedding", ".attn_bias.bias"), (".layers_", ".layers."),
    (".pre_attention_layer_norm.scale", ".sa_norm.weight"), (".pre_self_attention_layer_norm.scale", ".sa_norm.weight"),
    (".pre_cross_attention_layer_norm.scale", ".ca_norm.weight"), (".pre_mlp_layer_norm.scale", ".mlp_norm.weight"),
    (".attention.", ".sa."), (".self_attention.", ".sa."), (".encoder_decoder_attention.", ".ca."),
    (".query.kernel", ".q_proj.weight"), (".key.kernel", ".k_proj.weight"), (".value.kernel", ".v_proj.weight"),
    (".out.kernel", ".out_proj.weight"), (".wi_0.kernel", ".0.w.weight"), (".wi_1.kernel", ".0.v.weight"),
    (".wo.kernel", ".2.weight"),
)


def _rename_key(key: str) -> str:
    """t5x parameter path -> this module tree (the table of t5.py:230-252, applied in the same order)."""
    for old, new in _RENAMES:
        key = key.replace(old, new)
    return key
