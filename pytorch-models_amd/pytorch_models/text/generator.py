"""Text generation for decoder-only models: drop-in for /root/reference pytorch_models/text/generator.py
(DecoderGenerator(model, tokenizer).generate(prompt, max_tokens, topk)).

A pre-norm model (GPT-2) runs the KV-cached decode-step kernels of audio2text/generate.py, greedy or with top-k
sampling on the device (pm_dec_sample_topk) - the reference re-runs the whole sequence for every new token
(generator.py:24-25, O(T^2)); post-norm models (GPT) re-run the HIP forward per token like the reference does.  The tokenizer is any object with
``encode(str) -> list[int]``, ``decode(list[int]) -> str`` and ``eos_token_id`` (no tokenizer ships with this build)."""
from __future__ import annotations

import torch
from torch import nn


class DecoderGenerator:
    def __init__(self, model: nn.Module, tokenizer) -> None:
        self.model = model
        self.tokenizer = tokenizer

    @torch.inference_mode()
    def generate_ids(self, tokens: list[int], max_tokens: int = 100, topk: int = 1, eos_token_id: int | None = None,
                     generator: torch.Generator | None = None, seed: int = 0, prefill: bool = False, *, temperature: float = 1.0,
                     top_p: float = 1.0, min_new_tokens: int = 0, repetition_penalty: float = 1.0,
                     no_repeat_ngram_size: int = 0) -> list[int]:
        """Token-level form of generate(): prompt ids -> prompt + new ids, stopping after eos_token_id (kept, as the
        reference keeps it) or max_tokens new tokens.  ``prefill``: passed to the model's KV-cached generate() (the prompt in
        one batched pass); a model that decodes another way refuses it.  ``temperature`` (0 = arg-max) / ``top_p`` / ``topk`` = 0
        (the whole vocabulary): the sampling tail of the KV-cached generate() (pm_dec_sample), refused likewise elsewhere.
        ``min_new_tokens`` / ``repetition_penalty`` / ``no_repeat_ngram_size``: the logit controls of the KV-cached generate()
        (pm_dec_controls), refused likewise elsewhere; an ``eos_token_id`` inside the vocabulary goes to it too, so the run ends at the
        eos instead of being cut after max_tokens steps - the ids are the same."""
        sampling = self._sampling(topk, temperature, top_p)
        controls = self._controls(eos_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size)
        p0 = next(self.model.parameters())
        device = p0.device
        tokens = list(tokens)
        n = len(tokens)
        # KV-cached decoding: the graph-replayed step kernels for bf16 pre-norm stacks (GPT-2), the fp32 cached loop
        # (generate.greedy_exact) for everything else the layer algebra covers - fp32 parameters, post-norm stacks (GPT) -
        # instead of the reference's O(T^2) full-prefix loop, which remains for top-k sampling on those models
        kv_ok = p0.dtype == torch.bfloat16 and all(l.pre_norm for l in self.model.layers)
        # a model without a position table (anything that is not one of this package's decoders) has no length limit here
        room = self.model.pos_embs.shape[0] - n if hasattr(self.model, "pos_embs") else max_tokens
        if topk <= 64 and hasattr(self.model, "generate") and kv_ok:
            out = self.model.generate(torch.tensor([tokens], device=device), min(max_tokens, room), topk=topk, seed=seed,
                                      **({"prefill": True} if prefill else {}), **sampling, **controls)[0].tolist()
            new = out[n:]
            if eos_token_id is not None and eos_token_id in new:
                new = new[: new.index(eos_token_id) + 1]
            return tokens + new
        if prefill:
            raise NotImplementedError("DecoderGenerator: prefill=True runs on the KV-cached step kernels (a bf16 pre-norm model "
                                      "with generate(): GPT-2); this model decodes token by token: prefill=False")
        if sampling:
            raise NotImplementedError("DecoderGenerator: temperature / top_p / topk=0 run on the KV-cached step kernels (a bf16 pre-norm "
                                      "model with generate(): GPT-2); this model takes topk >= 1 at temperature 1, top_p 1")
        if controls and set(controls) != {"eos_token_id"}:
            raise NotImplementedError("DecoderGenerator: min_new_tokens / repetition_penalty / no_repeat_ngram_size run on the KV-cached "
                                      "step kernels (a bf16 pre-norm model with generate(): GPT-2); leave them at their defaults")
        if topk == 1 and hasattr(self.model, "token_embs") and hasattr(self.model, "pos_embs"):
            from ..audio2text.generate import greedy_exact
            from ..transformer import clear_derived, derived

            m32 = self.model
            if p0.dtype != torch.float32:  # fp32 twin of a bf16 post-norm model (same values), rebuilt when a parameter changes
                import copy

                def build():
                    twin = copy.deepcopy(self.model).float()
                    clear_derived(twin)
                    return twin

                m32 = derived(self.model, "exact32", list(self.model.parameters()) + list(self.model.buffers()), build)
            out = greedy_exact(m32, None, torch.tensor([tokens], device=device), min(max_tokens, room))[0].tolist()
            new = out[n:]
            if eos_token_id is not None and eos_token_id in new:
                new = new[: new.index(eos_token_id) + 1]
            return tokens + new
        while len(tokens) - n < max_tokens:
            logits = self.model(torch.tensor(tokens, device=device))[-1]
            if topk == 1:
                token = int(logits.argmax(-1))
            else:  # top-k sampling (generator.py:30-32)
                vals, idx = logits.topk(topk)
                token = int(idx[torch.multinomial(vals.softmax(-1), 1, generator=generator)])
            tokens.append(token)
            if eos_token_id is not None and token == eos_token_id:
                break
        return tokens

    @staticmethod
    def _sampling(topk: int, temperature: float, top_p: float) -> dict:
        """the keywords of the sampling tail for the model's generate(): empty at the defaults, which call it as always"""
        from .._hip.sampling import check_sampling, wants_sampling_tail

        if not wants_sampling_tail(topk, temperature, top_p, False):
            return {}
        check_sampling("DecoderGenerator", topk, temperature, top_p)
        return dict(temperature=temperature, top_p=top_p)

    def _controls(self, eos_token_id, min_new_tokens: int, repetition_penalty: float, no_repeat_ngram_size: int) -> dict:
        """the keywords of eos stopping and the logit controls for the model's generate(): the controls only away from their defaults,
        the eos only when it is an id of the model's vocabulary (any other never matches, and the host cut below finds nothing)"""
        from .._hip.controls import check_controls, wants_logit_controls

        kw = {}
        emb = getattr(self.model, "token_embs", None)
        if isinstance(eos_token_id, int) and not isinstance(eos_token_id, bool) and emb is not None and 0 <= eos_token_id < emb.weight.shape[0]:
            kw["eos_token_id"] = eos_token_id
        if wants_logit_controls(min_new_tokens, repetition_penalty, no_repeat_ngram_size):
            check_controls("DecoderGenerator", eos_token_id, 0, min_new_tokens, repetition_penalty, no_repeat_ngram_size)
            kw.update(min_new_tokens=min_new_tokens, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
        return kw

    @torch.inference_mode()
    def generate_ids_batch(self, prompts: list[list[int]], max_tokens: int = 100, topk: int = 1, eos_token_id: int | None = None,
                           seed: int = 0, prefill: bool = False, *, temperature: float = 1.0, top_p: float = 1.0, min_new_tokens: int = 0, repetition_penalty: float = 1.0,
                           no_repeat_ngram_size: int = 0) -> list[list[int]]:
        """generate_ids() for a batch of prompts of different lengths: one ragged call of the model's KV-cached generate() per shard
        of at most 64 prompts (right-padded, ``lengths=``), the padding stripped, each row cut after its first eos_token_id (kept).
        Greedy rows are what generate_ids() returns for them; top-k draws are keyed by (seed, cache position, row) and differ from
        the row's own run.  A shard decodes min(max_tokens, room of its LONGEST prompt) new tokens per row.  A model without the
        KV-cached step (post-norm GPT, fp32 parameters) goes through generate_ids() row by row.  ``temperature`` / ``top_p`` /
        ``min_new_tokens`` / ``repetition_penalty`` / ``no_repeat_ngram_size``: generate_ids()'s."""
        sampling = self._sampling(topk, temperature, top_p)
        controls = self._controls(eos_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size)
        prompts = [list(p) for p in prompts]
        if any(len(p) == 0 for p in prompts):
            raise ValueError("DecoderGenerator: every prompt needs at least one token")
        p0 = next(self.model.parameters())
        kv_ok = p0.dtype == torch.bfloat16 and all(l.pre_norm for l in self.model.layers)
        if not (topk <= 64 and hasattr(self.model, "generate") and kv_ok):
            return [self.generate_ids(p, max_tokens, topk, eos_token_id, seed=seed, prefill=prefill, temperature=temperature, top_p=top_p,
                                      min_new_tokens=min_new_tokens, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
                    for p in prompts]
        out = []
        for s in range(0, len(prompts), 64):
            shard = prompts[s : s + 64]
            lens = [len(p) for p in shard]
            width = max(lens)
            n_new = min(max_tokens, self.model.pos_embs.shape[0] - width) if hasattr(self.model, "pos_embs") else max_tokens
            padded = torch.zeros(len(shard), width, dtype=torch.int64)
            for row, p in zip(padded, shard):
                row[: len(p)] = torch.tensor(p)
            toks = self.model.generate(padded.to(p0.device), n_new, topk=topk, seed=seed, lengths=lens, pad_token_id=0,
                                       **({"prefill": True} if prefill else {}), **sampling, **controls).tolist()
            for p, row in zip(shard, toks):
                new = row[len(p) : len(p) + n_new]
                if eos_token_id is not None and eos_token_id in new:
                    new = new[: new.index(eos_token_id) + 1]
                out.append(p + new)
        return out

    def generate_batch(self, prompts: list[str], max_tokens: int = 100, topk: int = 1, prefill: bool = False, *, temperature: float = 1.0,
                       top_p: float = 1.0, min_new_tokens: int = 0, repetition_penalty: float = 1.0,
                       no_repeat_ngram_size: int = 0) -> list[str]:
        """generate() for a batch of prompts: one ragged batched decode (generate_ids_batch)"""
        ids = self.generate_ids_batch([self.tokenizer.encode(p) for p in prompts], max_tokens, topk,
                                      getattr(self.tokenizer, "eos_token_id", None), prefill=prefill, temperature=temperature, top_p=top_p,
                                      min_new_tokens=min_new_tokens, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
        return [self.tokenizer.decode(i) for i in ids]

    def generate(self, prompt: str, max_tokens: int = 100, topk: int = 1, prefill: bool = False, *, temperature: float = 1.0,
                 top_p: float = 1.0, min_new_tokens: int = 0, repetition_penalty: float = 1.0,
                 no_repeat_ngram_size: int = 0) -> str:
        ids = self.generate_ids(self.tokenizer.encode(prompt), max_tokens, topk, getattr(self.tokenizer, "eos_token_id", None),
                                prefill=prefill, temperature=temperature, top_p=top_p, min_new_tokens=min_new_tokens, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
        return self.tokenizer.decode(ids)
