"""Whisper on MI355X, drop-in for /root/reference pytorch_models/audio2text/whisper.py
(WhisperEncoder, WhisperDecoder, Whisper, WhisperPreprocessor, Whisper.from_openai; same parameter
names: stem.0 / stem.2, pos_embs, layers, norm, token_embs).

New capability (absent in the reference, README.md:86): ``Whisper.generate`` - batched greedy decoding
with a KV cache, see generate.py.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..audio.spectrogram import MelSpectrogram
from ..transformer import Decoder, Encoder, LayerNorm, _f32, _wb, clear_derived, derived

_SIZES = {  # tag -> (n_layers, d_model); "base" is 8 layers exactly as the reference builds it
    "tiny": (4, 384), "tiny.en": (4, 384), "base": (8, 512), "base.en": (8, 512),
    "small": (12, 768), "small.en": (12, 768), "medium": (24, 1024), "medium.en": (24, 1024),
    "large-v1": (32, 1280), "large-v2": (32, 1280), "large-v3": (32, 1280),
}


class WhisperEncoder(nn.Module):
    max_seq_len = 3000

    def __init__(self, n_layers: int, d_model: int, n_mels: int = 80, dropout: float = 0.0) -> None:
        super().__init__()
        self.stem = nn.Sequential(
            nn.Conv1d(n_mels, d_model, 3, 1, 1),
            nn.GELU(),
            nn.Conv1d(d_model, d_model, 3, 2, 1),
            nn.GELU(),
        )
        self.register_buffer("pos_embs", torch.zeros(self.max_seq_len // 2, d_model))
        self.pos_embs: Tensor
        self.layers = Encoder(n_layers, d_model, dropout=dropout)
        self.norm = LayerNorm(d_model)

    def _stem_weights(self):
        c1, c2 = self.stem[0], self.stem[2]

        def build():
            d, n_mels, _ = c1.weight.shape
            cpad = (n_mels + 63) // 64 * 64
            w1 = torch.zeros(d, 3, cpad, dtype=torch.bfloat16, device=c1.weight.device)  # (out, tap, channel) K-major
            w1[:, :, :n_mels] = c1.weight.detach().permute(0, 2, 1).to(torch.bfloat16)
            w2 = c2.weight.detach().permute(0, 2, 1).contiguous().view(d, 3 * d).to(torch.bfloat16)
            return w1.view(d, 3 * cpad), c1.bias.detach().float().contiguous(), w2, c2.bias.detach().float().contiguous()

        return derived(self, "stem", (c1.weight, c1.bias, c2.weight, c2.bias), build)

    def forward(self, x: Tensor) -> Tensor:
        """(B, n_mels, T) -> (B, T // 2, d): conv stem (both convs as MFMA GEMMs with fused GELU, the second
        also adding pos_embs in its epilogue), Encoder, LayerNorm."""
        if _cpu.on_cpu(x, self.stem[0].weight):  # CPU tensors and parameters: plain torch (pytorch_models/_cpu.py)
            return self.norm(self.layers(_cpu.whisper_stem(self, x)))
        if self.stem[0].weight.dtype == torch.float32:
            return self._forward_f32(x)
        w1, b1, w2, b2 = self._stem_weights()
        B, _, T = x.shape
        d = w2.shape[0]
        y1 = ops.whisper_stem1(x.float().contiguous(), w1, b1)  # (B, T + 2, d) bf16, rows 0 and T + 1 zero
        L = (T - 1) // 2 + 1
        pos = _f32(self, "pos", self.pos_embs)[:L]
        # Conv1d(d, d, 3, stride 2, pad 1): output row t' reads buffer rows 2t', 2t'+1, 2t'+2 = 3*d contiguous values
        y2 = ops.linear_strided(y1, M=B * L, K=3 * d, row_stride=2 * d, rows_per_batch=L, batch_stride=(T + 2) * d,
                                w=w2, bias=b2, act="gelu", resid=pos, resid_period=L)
        return self.norm(self.layers(y2.view(B, L, d)), self.stem[0].weight.dtype)  # fp32 model -> fp32 memory


def _encoder_forward_f32(self: WhisperEncoder, x: Tensor) -> Tensor:
    """fp32 parameters: both convolutions as fp32 GEMMs over windows (a window view + one contiguous copy each is layout,
    the arithmetic is pm_linear_f32 with GELU and, for the second, + pos_embs in its epilogue), fp32 Encoder, fp32 LayerNorm."""
    c1, c2 = self.stem[0], self.stem[2]
    B, C, T = x.shape
    d = c1.weight.shape[0]
    xp = torch.nn.functional.pad(x.float(), (1, 1))
    cols = xp.unfold(2, 3, 1).permute(0, 2, 1, 3).reshape(B * T, C * 3)  # (B T, C * 3): K order (channel, tap) = weight.view(d, -1)
    y1 = ops.linear_f32(cols, c1.weight.view(d, C * 3), c1.bias, act="gelu").view(B, T, d)
    L = (T - 1) // 2 + 1
    yp = torch.nn.functional.pad(y1, (0, 0, 1, 1))
    cols = yp.unfold(1, 3, 2).reshape(B * L, d * 3)  # window dim last: (B, L, d, 3) -> K order (channel, tap)
    pos = self.pos_embs.float()[:L].contiguous()
    y2 = ops.linear_f32(cols, c2.weight.view(d, d * 3), c2.bias, act="gelu", resid=pos, resid_period=L)
    return self.norm(self.layers(y2.view(B, L, d)))


WhisperEncoder._forward_f32 = _encoder_forward_f32


class WhisperDecoder(nn.Module):
    max_seq_len = 448

    def __init__(self, vocab_size: int, n_layers: int, d_model: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.token_embs = nn.Embedding(vocab_size, d_model)
        self.pos_embs = nn.Parameter(torch.zeros(self.max_seq_len, d_model))
        self.layers = Decoder(n_layers, d_model, cross_attn=True, dropout=dropout)
        self.norm = LayerNorm(d_model)

    def forward(self, x: Tensor, memory: Tensor) -> Tensor:
        """tokens (B, L) int64, memory (B, S, d) -> logits (B, L, V) (tied embeddings), teacher-forced."""
        if _cpu.on_cpu(x, self.token_embs.weight):
            E = self.token_embs.weight
            h = self.norm(self.layers(_cpu.embed_tokens(x, E, self.pos_embs), memory.to(E.dtype)))
            return h @ E.T
        if self.token_embs.weight.dtype == torch.float32:  # fp32 parameters: fp32 throughout
            E = self.token_embs.weight
            h = self.norm(self.layers(ops.embed_tokens(x, E, self.pos_embs), memory.float()))
            return ops.linear_f32(h.view(-1, h.shape[-1]), E).view(*x.shape, E.shape[0])
        h, E = self.hidden_rows(x, memory)
        return ops.linear(h.view(-1, h.shape[-1]), E, None, out_dtype=torch.float32).view(*x.shape, E.shape[0])

    def hidden_rows(self, x: Tensor, memory: Tensor):
        """bf16 parameters: (hidden rows (B, L, d) bf16, head weights (V, d) bf16) - what forward's last GEMM and score's
        kernel both read."""
        E = _wb(self.token_embs, "E", self.token_embs.weight)
        h = ops.embed_tokens(x, E, _f32(self, "pos", self.pos_embs))  # (B, L, d) bf16
        return self.norm(self.layers(h, memory)), E

    @torch.no_grad()
    def score(self, tokens: Tensor, memory: Tensor, lengths=None, *, return_argmax: bool = False):
        """Teacher-forced scoring in O(B L) memory: tokens (B, L) int64 - the decoder's input ids, exactly what forward takes -
        and memory (B, S, d) -> (B, L - 1) fp32 with out[b, t] = log p(tokens[b, t + 1] | tokens[b, : t + 1], memory[b]).
        ``lengths`` (B,), 1 <= len_b <= L, marks a right-padded batch: positions with t + 1 >= len_b are ignored and return 0, so
        out.sum(-1) is the sequence log-likelihood and out.sum(-1) / (lengths - 1) Whisper's avg_logprob.  ``return_argmax``:
        also the (B, L - 1) int64 greedy predictions.  bf16 parameters on a HIP device: projection, log-softmax and gather are
        one kernel (ops.lm_score), the (B, L, V) logits are never stored.  A module and inputs that both live on the CPU take
        the plain-torch form: fp32 log_softmax of forward's logits and a gather."""
        from ..text.gpt2 import score_gate, score_rows, score_targets

        if _cpu.on_cpu(tokens, self.token_embs.weight):
            tgt = score_targets(tokens, lengths, "WhisperDecoder.score")
            logits = self.forward(tokens, memory)[:, :-1].float()
            lp = torch.log_softmax(logits, -1).gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            lp = torch.where(tgt >= 0, lp, torch.zeros_like(lp))
            return (lp, logits.argmax(-1)) if return_argmax else lp
        score_gate("WhisperDecoder.score", self.token_embs.weight, tokens, memory)
        score_targets(tokens, lengths, "WhisperDecoder.score")  # shape and lengths errors before any launch
        h, E = self.hidden_rows(tokens, memory)
        return score_rows(h, E, tokens, lengths, return_argmax, "WhisperDecoder.score")

    @torch.no_grad()
    def align(self, tokens: Tensor, memory: Tensor, *, lengths=None, frames=None, heads=None, skip_first: int = 0,
              skip_last: int = 0, return_matrix: bool = False):
        """Token timestamps by cross-attention alignment and dynamic time warping: tokens (B, L) int64 - the decoder's input ids,
        as forward takes them - and memory (B, S, d) -> start (B, L) int32, the encoder position (Whisper.SECONDS_PER_FRAME each)
        at which token t begins; a token ends where the next aligned one begins.  ``lengths`` / ``frames``: host ints or sequences
        of B ints, 1 <= len_b <= L tokens and 4 <= F_b <= S encoder positions that count (defaults L and S).  ``heads``:
        [(layer, head), ...], default every head of the upper half of the layers.  ``skip_first`` / ``skip_last``: rows dropped from
        the warped window (the published use is skip_first = len(sot_sequence), skip_last = 1 with the eot row kept in tokens);
        rows outside the window or at or beyond len_b return -1.  ``return_matrix``: also m (B, L, S) fp32, the normalised,
        median-filtered, head-averaged attention the path runs through (exactly 0 where t >= len_b or f >= F_b).  A frame column
        whose probabilities do not vary over the tokens (std exactly 0) normalises to 0, where the published code yields NaN.
        bf16 parameters on a HIP device (audio2text/align.py, csrc/align.hip): no probabilities are stored and nothing waits for
        the device; fp32 parameters raise NotImplementedError; a CPU module with CPU inputs takes the plain-torch form."""
        from .align import align

        return align(self, tokens, memory, lengths=lengths, frames=frames, heads=heads, skip_first=skip_first, skip_last=skip_last,
                     return_matrix=return_matrix)

    @torch.no_grad()
    def generate(self, memory: Tensor, prompt: Tensor, max_new_tokens: int, *, graph: bool = True, rules=None,
                 path: str = "auto", beams: int = 1, eos_token_id: int | None = None, return_beams: bool = False,
                 prefill: bool = False, lengths=None, pad_token_id: int = 0, topk: int = 1, seed: int = 0, temperature: float = 1.0,
                 top_p: float = 1.0, return_logprobs: bool = False, return_lengths: bool = False, min_new_tokens: int = 0,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """Batched greedy decoding with a KV cache: (B, P) int64 prompt -> (B, P + max_new_tokens) ids.  ``rules``: a
        generate.WhisperRules (token suppression, timestamp pairing / monotonicity) applied to the logits on the device;
        ``path``: "persistent" / "launches" / "auto" (generate.GreedyDecoder).  ``beams`` > 1: beam search of that width
        (generate.beam_decode; 1..8, B * beams <= 64) - the best hypothesis, or with ``return_beams`` (tokens (B, beams, P + n),
        scores (B, beams)), best first; ``eos_token_id`` ends a hypothesis (default: rules.eot under rules).  ``prefill``: the
        prompt fills the caches in one batched pass instead of one step per token (generate.greedy_decode; bf16 model and memory).
        ``lengths`` (B,), 1 <= len_b <= P: a ragged batch - ``prompt`` is right-padded, row b of the result is prompt[b, :len_b], its
        new ids, then P - len_b times ``pad_token_id``: what generate() returns for that clip and prompt alone (generate.greedy_decode;
        bf16 model and memory, beams = 1, not path="persistent").
        ``topk`` (1..64; 0 = the whole vocabulary), ``seed``, ``temperature`` (0 = arg-max), ``top_p``, ``return_logprobs`` (-> (ids,
        logprobs (B, max_new_tokens) f32), each new token's log-probability at temperature 1 after the controls and the rules; with
        ``eos_token_id`` logprobs.sum(-1) / n_new is Whisper's avg_logprob): generate.greedy_decode's sampling; bf16 model and memory,
        beams = 1, not path="persistent".
        ``eos_token_id`` (beams = 1; None = never finish, also under ``rules``): a row finishes at its first GENERATED eos, later positions hold ``pad_token_id`` and log-prob 0.0,
        the run ends once every row has finished; ``return_lengths`` appends n_new (B,) int64 (eos included) as the last element of the
        result; ``min_new_tokens`` / ``repetition_penalty`` / ``no_repeat_ngram_size`` (0..8): the logit controls of
        generate.greedy_decode (one pm_dec_controls launch per step); bf16 parameters, beams = 1, not path="persistent"."""
        from .._hip.controls import check_controls
        from .generate import beam_decode, check_ragged, check_sampling_tail, greedy_decode, greedy_exact

        ops.refuse_empty_batch("WhisperDecoder.generate", memory, prompt)
        fp32 = self.token_embs.weight.dtype == torch.float32
        check_controls("WhisperDecoder.generate", eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size,
                       return_lengths, vocab=self.token_embs.weight.shape[0], beams=1 if beams == 1 and not return_beams else max(beams, 2),
                       path=path, kv32=memory is not None and memory.dtype == torch.float32, fp32=fp32)
        check_sampling_tail("WhisperDecoder.generate", topk, temperature, top_p, return_logprobs,
                            beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path,
                            kv32=memory is not None and memory.dtype == torch.float32, fp32=fp32)
        if topk != 1 and (beams != 1 or return_beams):
            raise ValueError("beam decode: topk sampling and arg-max margins are greedy decode's")
        if topk != 1 and fp32:
            raise NotImplementedError("WhisperDecoder.generate: topk sampling needs bf16 parameters (model.to(torch.bfloat16)); fp32 "
                                      "parameters decode through greedy_exact, arg-max only: topk=1")
        check_ragged("WhisperDecoder.generate", lengths, beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path,
                     kv32=memory is not None and memory.dtype == torch.float32, fp32=self.token_embs.weight.dtype == torch.float32)
        if prefill and self.token_embs.weight.dtype == torch.float32:
            raise NotImplementedError("WhisperDecoder.generate: prefill=True needs bf16 parameters (model.to(torch.bfloat16)); fp32 "
                                      "parameters decode through greedy_exact, token by token: prefill=False")
        if beams != 1 or return_beams:
            if self.token_embs.weight.dtype == torch.float32:
                raise NotImplementedError("beam decode: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda()); "
                                          "Whisper.generate(exact=True) is the fp32-cache form")
            return beam_decode(self, memory, prompt, max_new_tokens, beams=beams, eos_token_id=eos_token_id, graph=graph,
                               rules=rules, path=path, kv32=memory.dtype == torch.float32, return_beams=return_beams, prefill=prefill)
        if self.token_embs.weight.dtype == torch.float32:  # fp32 parameters: the fp32 end-to-end loop (no bf16 storage points)
            if rules is not None:
                raise NotImplementedError("WhisperDecoder.generate: the decoding rules run on the bf16 model's step kernels")
            return greedy_exact(self, memory, prompt, max_new_tokens)
        return greedy_decode(self, memory, prompt, max_new_tokens, graph=graph, rules=rules, path=path, prefill=prefill,
                             lengths=lengths, pad_token_id=pad_token_id, topk=topk, seed=seed, temperature=temperature, top_p=top_p,
                             return_logprobs=return_logprobs, eos_token_id=eos_token_id, return_lengths=return_lengths, min_new_tokens=min_new_tokens,
                             repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)


class Whisper(nn.Module):
    def __init__(self, vocab_size: int, n_layers: int, d_model: int, n_mels: int = 80, dropout: float = 0.0, *,
                 n_decoder_layers: int | None = None) -> None:
        """``n_decoder_layers`` (superset of the reference signature): a shallower decoder than encoder, the geometry of
        the distilled checkpoints the reference lists as TODO (README.md:87; e.g. distil-large-v2 = 32 encoder / 2 decoder
        layers).  Parameter names are unchanged, so such a checkpoint loads through load_openai_state_dict."""
        super().__init__()
        self.encoder = WhisperEncoder(n_layers, d_model, n_mels, dropout=dropout)
        self.decoder = WhisperDecoder(vocab_size, n_layers if n_decoder_layers is None else n_decoder_layers, d_model, dropout=dropout)

    def forward(self, x: Tensor, targets: Tensor) -> Tensor:
        return self.decoder(targets, self.encoder(x))

    @torch.no_grad()
    def score(self, x: Tensor, tokens: Tensor, lengths=None, *, return_argmax: bool = False):
        """log-mel (B, n_mels, T) + decoder input ids (B, L) -> (B, L - 1) fp32 log-probabilities of tokens[b, t + 1] given
        tokens[b, : t + 1] and the clip (WhisperDecoder.score's convention: ``lengths`` for a right-padded batch, ignored positions
        return 0, ``return_argmax`` adds the greedy predictions)."""
        return self.decoder.score(tokens, self.encoder(x), lengths, return_argmax=return_argmax)

    SECONDS_PER_FRAME = 0.02  # one encoder position: two 10 ms mel frames

    @torch.no_grad()
    def align(self, x: Tensor, tokens: Tensor, **kwargs):
        """log-mel (B, n_mels, T) + decoder input ids (B, L) -> start (B, L) int32 encoder positions (x SECONDS_PER_FRAME seconds):
        WhisperDecoder.align on this clip's encoder output, with its keywords."""
        return self.decoder.align(tokens, self.encoder(x), **kwargs)

    @torch.no_grad()
    def generate(self, x: Tensor, prompt: Tensor, max_new_tokens: int, *, graph: bool = True, rules=None, path: str = "auto",
                 exact: bool = False, beams: int = 1, eos_token_id: int | None = None, return_beams: bool = False,
                 prefill: bool = False, lengths=None, pad_token_id: int = 0, topk: int = 1, seed: int = 0, temperature: float = 1.0,
                 top_p: float = 1.0, return_logprobs: bool = False, return_lengths: bool = False, min_new_tokens: int = 0,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """log-mel (B, n_mels, T) + prompt ids (B, P) -> greedy ids (B, P + max_new_tokens); ``beams`` > 1: beam search
        (WhisperDecoder.generate), with ``exact=True`` on the fp32-cache step (B * beams * n_heads <= 256).
        ``exact=True`` (bf16 model): the whole pipeline - encoder, cross K/V, decoder, caches - in fp32 on an fp32 copy of
        this model's (bf16-valued) weights: the ids are those of the reference's fp32 forward on the same weights, bit for
        bit (tests/test_hip_exact.py); costs ~10x the bf16 encoder and an eager fp32 step loop.  A model whose
        parameters are fp32 always decodes this way.  ``prefill``: WhisperDecoder.generate's; not with ``exact``.
        ``lengths`` / ``pad_token_id``: WhisperDecoder.generate's ragged prompt batch; not with ``exact``, beams or fp32 parameters.
        ``topk`` / ``seed`` / ``temperature`` / ``top_p`` / ``return_logprobs``: WhisperDecoder.generate's sampling; not with ``exact``,
        beams or fp32 parameters.
        ``eos_token_id`` (beams = 1) / ``return_lengths`` / ``min_new_tokens`` / ``repetition_penalty`` / ``no_repeat_ngram_size``:
        WhisperDecoder.generate's eos stopping and logit controls; not with ``exact``, beams or fp32 parameters."""
        from .._hip.controls import check_controls
        from .generate import check_ragged, check_sampling_tail

        ops.refuse_empty_batch("Whisper.generate", x, prompt)
        check_controls("Whisper.generate", eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size,
                       return_lengths, vocab=self.decoder.token_embs.weight.shape[0],
                       beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path, kv32=exact,
                       fp32=self.decoder.token_embs.weight.dtype == torch.float32)
        check_sampling_tail("Whisper.generate", topk, temperature, top_p, return_logprobs,
                            beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path, kv32=exact,
                            fp32=self.decoder.token_embs.weight.dtype == torch.float32)
        if topk != 1 and exact:
            raise NotImplementedError("Whisper.generate: exact=True promises the reference's arg-max ids; topk sampling runs on the "
                                      "bf16-cache step: exact=False")
        check_ragged("Whisper.generate", lengths, beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path, kv32=exact,
                     fp32=self.decoder.token_embs.weight.dtype == torch.float32)
        if prefill and exact:
            raise NotImplementedError("Whisper.generate: prefill=True fills bf16 caches; exact=True promises bit equality with the "
                                      "reference and keeps the token-by-token prompt: prefill=False")
        if beams != 1 or return_beams:
            w = self.decoder.token_embs.weight
            if w.dtype == torch.float32 or not w.is_cuda:
                raise NotImplementedError("beam decode: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda())")
            memory = self.exact_copy().encoder(x) if exact else self.encoder(x)
            return self.decoder.generate(memory, prompt, max_new_tokens, graph=graph, rules=rules, path=path, beams=beams,
                                         eos_token_id=eos_token_id, return_beams=return_beams, prefill=prefill, topk=topk)
        if exact and self.decoder.token_embs.weight.dtype != torch.float32:
            # fp32 encoder on the fp32 twin of the (bf16-valued) weights; the decode step is the throughput path's own launch
            # list with fp32 K / V caches - its projections are fp32-exact as they stand (bf16 weights x activations in three
            # bf16 terms) - replayed as one HIP graph per token.  Geometries that list does not cover (more than 256
            # (sequence, head) pairs) fall back to the eager fp32 loop of the twin.
            from .generate import greedy_decode

            twin = self.exact_copy()
            H = self.decoder.layers[0].sa.n_heads
            if rules is None and prompt.shape[0] * H <= 256 and prompt.shape[0] <= 64:
                return greedy_decode(self.decoder, twin.encoder(x), prompt, max_new_tokens, graph=graph, kv32=True)
            return twin.generate(x, prompt, max_new_tokens)
        return self.decoder.generate(self.encoder(x), prompt, max_new_tokens, graph=graph, rules=rules, path=path, prefill=prefill,
                                     lengths=lengths, pad_token_id=pad_token_id, topk=topk, seed=seed, temperature=temperature,
                                     top_p=top_p, return_logprobs=return_logprobs, eos_token_id=eos_token_id, return_lengths=return_lengths, min_new_tokens=min_new_tokens,
                                     repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)

    def exact_copy(self) -> "Whisper":
        """fp32 twin of this model (same values: bf16 -> fp32 is exact), rebuilt when a parameter changes."""
        import copy

        params = list(self.parameters()) + list(self.buffers())
        def build():
            twin = copy.deepcopy(self).float()
            clear_derived(twin)  # the twin derives its own packed / re-typed weights
            return twin

        return derived(self, "exact32", params, build)

    def load_openai_state_dict(self, state_dict) -> None:
        """OpenAI ``model_state_dict`` (e.g. ``torch.load(path, weights_only=True)["model_state_dict"]``)."""
        from ..converters import load_openai_whisper

        left = load_openai_whisper(self, state_dict)
        if left:
            print(left)

    @staticmethod
    def from_openai(model_tag: str, *, pretrained: bool = False, **kwargs) -> "Whisper":
        n_layers, d_model = _SIZES[model_tag]
        if model_tag == "large-v3":
            n_mels, vocab_size = 128, 51866
        else:
            n_mels, vocab_size = 80, (51864 if model_tag.endswith(".en") else 51865)
        m = Whisper(vocab_size, n_layers, d_model, n_mels, **kwargs)
        if pretrained:
            raise NotImplementedError(
                "Whisper.from_openai(pretrained=True) needs a network download, which this build does not do; "
                "construct with pretrained=False and load a local checkpoint into the (reference-named) parameters.")
        return m


class WhisperPreprocessor(MelSpectrogram):
    def __init__(self, variant: str = "tiny") -> None:
        n_mels = 128 if variant == "large-v3" else 80
        super().__init__(400, 160, n_mels, 16_000)

    def forward(self, x: Tensor) -> Tensor:
        """(..., T) waveform -> (..., n_mels, T // 160) log-mel: last frame dropped, log10, floored at the
        PER-SAMPLE max - 8, (x + 4) / 4 - all inside the two logmel kernels."""
        if _cpu.on_cpu(x, self.window, self.filters):
            return _cpu.whisper_log_mel(x, self.window, self.filters)
        if x.numel() == 0:  # as the CPU path, whose reflect padding has no empty batch
            raise ValueError(f"WhisperPreprocessor: an empty batch of waveforms is refused (got {tuple(x.shape)})")
        return ops.stft_mel(x, self._tables(), 400, 160, x.shape[-1] // 160, 2, self._csr(), self.filters.shape[0])
