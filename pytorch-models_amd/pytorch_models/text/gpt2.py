"""GPT-2 on MI355X: drop-in for /root/reference pytorch_models/text/gpt2.py (GPT2, from_hf, load_hf_state_dict; parameter
names token_embs, pos_embs, layers, norm).

forward = pm_embed_tokens (token + position rows in one kernel) -> Decoder of pre-norm, causal, tanh-GELU layers
(transformer.py) -> LayerNorm -> logits against the tied embedding matrix (pm_linear_bf16, fp32 out, ragged N = 50257).
Greedy generation with a KV cache: GPT2.generate / text.DecoderGenerator (generate.py's decode-step kernels).
Teacher-forced scoring: GPT2.score = the same hidden rows -> pm_lm_score_bf16 (projection, log-softmax and gather in one kernel; the
logits are never stored).  score_rows / score_targets / score_gate below are the scoring tail every model's ``score`` shares."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .._hip import ops
from ..transformer import Decoder, LayerNorm, _f32, _wb

_SIZES = {"gpt2": (12, 768), "gpt2-medium": (24, 1024), "gpt2-large": (36, 1280), "gpt2-xl": (48, 1600)}


def _lm_forward(m, tokens: Tensor, final_norm) -> Tensor:
    lead = tokens.shape
    tok2 = tokens.reshape(-1, lead[-1])  # the reference also accepts an unbatched (L,) sequence (generator.py:25)
    if m.token_embs.weight.dtype == torch.float32:  # fp32 parameters: fp32 rows, fp32 blocks, fp32 logits
        E = m.token_embs.weight
        h = m.layers(ops.embed_tokens(tok2, E, m.pos_embs))
        if final_norm is not None:
            h = final_norm(h)
        return ops.linear_f32(h.view(-1, h.shape[-1]), E).view(*lead, E.shape[0])
    h, E = _lm_hidden(m, tok2, final_norm)
    logits = ops.linear(h.view(-1, h.shape[-1]), E, None, out_dtype=torch.float32)
    return logits.view(*lead, E.shape[0])


def _lm_hidden(m, tok2: Tensor, final_norm):
    """bf16 parameters: the hidden rows (B, L, d) the vocabulary projection reads, and its (V, d) weights.  forward and score
    both start here."""
    E = m.token_embs.weight
    h = ops.embed_tokens(tok2, E, _f32(m, "pos", m.pos_embs))
    h = m.layers(h)
    if final_norm is not None:
        h = final_norm(h)
    return h, E


def score_gate(who: str, w: Tensor, *inputs: Tensor) -> None:
    """Device and dtype rule of every ``score``: operands on one HIP device (the device error first, as forward raises it), bf16
    parameters."""
    ops.check_devices(w, *inputs)
    if w.dtype != torch.bfloat16:
        raise NotImplementedError(f"{who}: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda()); fp32 parameters "
                                  "score through forward() and torch.log_softmax")


def score_targets(tokens: Tensor, lengths, who: str) -> Tensor:
    """The (B, L - 1) int64 targets of teacher-forced scoring: tokens[b, t + 1], or -1 ("ignore") where t + 1 >= len_b."""
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise ValueError(f"{who}: tokens must be int64 (B, L), got {tokens.dtype} {tuple(tokens.shape)}")
    B, L = tokens.shape
    tgt = tokens[:, 1:]
    if lengths is None:
        return tgt.contiguous()
    ops.no_capture(who, "reads lengths on the host")
    lens = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
    if lens.numel() != B or (B and (int(lens.min()) < 1 or int(lens.max()) > L)):
        raise ValueError(f"{who}: lengths must hold {B} values in [1, {L}], got {lens.tolist()}")
    keep = torch.arange(1, L, device=tokens.device)[None, :] < lens.to(tokens.device)[:, None]
    return torch.where(keep, tgt, torch.full_like(tgt, -1))


def score_rows(h: Tensor, W: Tensor, tokens: Tensor, lengths, return_argmax: bool, who: str):
    """THE scoring tail of every model: hidden rows h (B, L, d) bf16 (what forward multiplies by W), head weights W (V, d) bf16,
    decoder input ids tokens (B, L) -> out (B, L - 1) f32, out[b, t] = log p(tokens[b, t + 1] | tokens[b, : t + 1]); positions
    with t + 1 >= lengths[b] are ignored and return exactly 0, so out.sum(-1) is the sequence log-likelihood.  With
    return_argmax also the (B, L - 1) int64 greedy predictions (the lowest arg-max index of each position's logits).  One
    ops.lm_score launch over the B (L - 1) rows: nothing of size rows x V is allocated."""
    tgt = score_targets(tokens, lengths, who)
    B, L = tokens.shape
    if L == 1:
        out = torch.zeros((B, 0), dtype=torch.float32, device=h.device)
        return (out, torch.zeros((B, 0), dtype=torch.int64, device=h.device)) if return_argmax else out
    rows = h[:, :-1].reshape(B * (L - 1), h.shape[-1])  # the last position predicts nothing that is scored
    res = ops.lm_score(rows, W, tgt.reshape(-1), want_argmax=return_argmax)
    if return_argmax:
        return res[0].view(B, L - 1), res[1].to(torch.int64).view(B, L - 1)
    return res.view(B, L - 1)


def _lm_score(m, tokens: Tensor, final_norm, lengths, return_argmax: bool, who: str):
    score_gate(who, m.token_embs.weight, tokens)
    score_targets(tokens, lengths, who)  # shape and lengths errors before any launch
    h, E = _lm_hidden(m, tokens, final_norm)
    return score_rows(h, E, tokens, lengths, return_argmax, who)


class GPT2(nn.Module):
    vocab_size = 50257
    max_seq_len: int = 1024

    def __init__(self, n_layers: int, d_model: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.token_embs = nn.Embedding(self.vocab_size, d_model)
        self.pos_embs = nn.Parameter(torch.zeros(self.max_seq_len, d_model))
        self.layers = Decoder(n_layers, d_model, dropout=dropout, act="approximate_gelu")
        self.norm = LayerNorm(d_model)

    def forward(self, x: Tensor) -> Tensor:
        """token ids (..., L) int64 -> logits (..., L, 50257) fp32 (gpt2.py:21-27)."""
        return _lm_forward(self, x, self.norm)

    def hidden_rows(self, tokens: Tensor):
        """(hidden rows (B, L, d) bf16, head weights (V, d) bf16): what forward's last GEMM and score's kernel both read."""
        return _lm_hidden(self, tokens, self.norm)

    @torch.no_grad()
    def score(self, tokens: Tensor, lengths=None, *, return_argmax: bool = False):
        """Teacher-forced scoring in O(B L) memory: tokens (B, L) int64 - exactly what forward takes - -> (B, L - 1) fp32 with
        out[b, t] = log p(tokens[b, t + 1] | tokens[b, : t + 1]).  ``lengths`` (B,), 1 <= len_b <= L, marks a right-padded batch:
        positions with t + 1 >= len_b are ignored and return 0, so out.sum(-1) is the sequence log-likelihood (and
        -out.sum() / (lengths - 1).sum() the log-perplexity).  ``return_argmax``: also the (B, L - 1) int64 greedy predictions.
        The vocabulary projection, the log-softmax and the gather are one kernel (ops.lm_score): the (B, L, 50257) logits are
        never stored.  bf16 parameters on a HIP device."""
        return _lm_score(self, tokens, self.norm, lengths, return_argmax, "GPT2.score")

    @torch.no_grad()
    def generate(self, prompt: Tensor, max_new_tokens: int, *, graph: bool = True, topk: int = 1, seed: int = 0,
                 path: str = "auto", beams: int = 1, eos_token_id: int | None = None, return_beams: bool = False,
                 prefill: bool = False, lengths=None, pad_token_id: int = 0, temperature: float = 1.0, top_p: float = 1.0,
                 return_logprobs: bool = False, return_lengths: bool = False, min_new_tokens: int = 0,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """Batched decoding with a KV cache: (B, P) int64 prompt -> (B, P + max_new_tokens) ids; greedy (topk = 1) or
        top-k sampling on the device (softmax over the k largest logits; the same seed gives the same ids); ``beams`` > 1:
        beam search (audio2text.generate.beam_decode), with ``return_beams`` (tokens (B, beams, P + n), scores (B, beams)).
        ``prefill``: the prompt fills the caches in one batched pass instead of one step per token (generate.greedy_decode).
        ``lengths`` (B,), 1 <= len_b <= P: a ragged batch - ``prompt`` is right-padded, row b of the result is prompt[b, :len_b], its
        new ids, then P - len_b times ``pad_token_id``: what generate() returns for that row alone (greedy; top-k draws are keyed
        by the cache position, so they differ from the row's own run).  bf16 parameters, beams = 1, not path="persistent".
        ``temperature`` (0 = arg-max), ``top_p``, ``topk`` = 0 (the whole vocabulary), ``return_logprobs`` (-> (ids, logprobs (B,
        max_new_tokens) f32)): the sampling tail of generate.greedy_decode; bf16 parameters, beams = 1, not path="persistent".
        ``eos_token_id`` (beams = 1): a row finishes at its first GENERATED eos, later positions hold ``pad_token_id`` and log-prob 0.0,
        the run ends once every row has finished; ``return_lengths`` appends n_new (B,) int64 (eos included) as the last element of the
        result; ``min_new_tokens`` / ``repetition_penalty`` / ``no_repeat_ngram_size`` (0..8): the logit controls of
        generate.greedy_decode (one pm_dec_controls launch per step); bf16 parameters, beams = 1, not path="persistent"."""
        from .._hip.controls import check_controls
        from ..audio2text.generate import beam_decode, check_ragged, check_sampling_tail, greedy_decode, greedy_exact

        ops.refuse_empty_batch("GPT2.generate", prompt)
        check_controls("GPT2.generate", eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size, return_lengths,
                       vocab=self.token_embs.weight.shape[0], beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path,
                       fp32=self.token_embs.weight.dtype == torch.float32)

        check_sampling_tail("GPT2.generate", topk, temperature, top_p, return_logprobs, beams=1 if beams == 1 and not return_beams else max(beams, 2),
                            path=path, fp32=self.token_embs.weight.dtype == torch.float32)
        check_ragged("GPT2.generate", lengths, beams=1 if beams == 1 and not return_beams else max(beams, 2), path=path,
                     fp32=self.token_embs.weight.dtype == torch.float32)
        if prefill and self.token_embs.weight.dtype == torch.float32:
            raise NotImplementedError("GPT2.generate: prefill=True needs bf16 parameters (model.to(torch.bfloat16)); fp32 parameters "
                                      "decode through greedy_exact, token by token: prefill=False")
        if beams != 1 or return_beams:
            if self.token_embs.weight.dtype == torch.float32:
                raise NotImplementedError("beam decode: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda())")
            if topk != 1:
                raise ValueError("beam decode: topk sampling and arg-max margins are greedy decode's")
            return beam_decode(self, None, prompt, max_new_tokens, beams=beams, eos_token_id=eos_token_id, graph=graph, path=path,
                               return_beams=return_beams, prefill=prefill)
        if self.token_embs.weight.dtype == torch.float32 and topk == 1:  # fp32 parameters: fp32 end to end
            return greedy_exact(self, None, prompt, max_new_tokens)
        return greedy_decode(self, None, prompt, max_new_tokens, graph=graph, topk=topk, seed=seed, path=path, prefill=prefill,
                             lengths=lengths, pad_token_id=pad_token_id, temperature=temperature, top_p=top_p,
                             return_logprobs=return_logprobs, eos_token_id=eos_token_id, return_lengths=return_lengths, min_new_tokens=min_new_tokens,
                             repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)

    @staticmethod
    def from_hf(model_tag: str, *, pretrained=False, **kwargs) -> "GPT2":
        n_layers, d_model = _SIZES[model_tag]
        m = GPT2(n_layers, d_model, **kwargs)
        if pretrained:
            raise NotImplementedError(
                "GPT2.from_hf(pretrained=True) needs a network download, which this build does not do; construct with "
                "pretrained=False and call load_hf_state_dict(torch.load(path, weights_only=True)).")
        return m

    def load_hf_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        """Hugging Face GPT2LMHeadModel state_dict (converters.load_hf_gpt2)."""
        from ..converters import load_hf_gpt2

        load_hf_gpt2(self, state_dict)
