"""Batched greedy decoding with a KV cache for WhisperDecoder on MI355X.

New capability (the reference decodes nothing for Whisper: README.md:86).  Semantics = the reference's
generic greedy loop (text/generator.py:23-35): at each step take argmax of the last position's logits and
append it; here for a whole batch, with the self-attention K/V cached and the cross-attention K/V projected
once.  The stop rule is build-defined (no tokenizer in the reference): a fixed number of new tokens, or - with ``eos_token_id`` -
until every row has emitted its eos (pm_dec_finish keeps the rows' finished flags on the device).

One step is ~8 launches per layer (csrc/decode.hip); the position and current tokens live on the device, so the
step is captured ONCE into a HIP graph and replayed - no tracing compiler, no host round trips in the loop.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch
from torch import Tensor

from .._hip import DecLayer, decode_plan as plan, lib, ops
from .._hip.controls import check_controls
from .._hip.sampling import check_sampling, wants_sampling_tail
from ..transformer import _f32


# path="auto" = the launch-per-stage list.  Measured (tools/decode_paths_bench.py, MI355X, batch 32, us per step): Whisper-base 461
# launches / 623 persistent, small 1044 / 1665, large-v2 4476 / 7160 - inside one launch a stage boundary costs MORE than a
# kernel boundary (poll + barrier + sc1 round trips ~4-5 us against ~1.5 us + first loads), exactly what
# cdna_hip_programming.md 5.6 reports for latency-bound phases.  The persistent path stays selectable and tested.
PERSISTENT_BY_DEFAULT = False

# With eos_token_id, GreedyDecoder.run reads the rows' finished flags back every POLL_EVERY steps (one synchronisation each) and
# stops once every row has finished: T5Model.generate's figure (text/t5_generate.py)
POLL_EVERY = 32


def _ln(norm) -> tuple:
    """(gamma f32, beta f32, eps) of a LayerNorm module"""
    return _f32(norm, "g", norm.weight), _f32(norm, "b", norm.bias), norm.eps


@dataclass
class WhisperRules:
    """Whisper's decoding-time logit filters (pm_dec_whisper_rules): ids of the tokenizer in use.  ``blank`` = ids forbidden as
    the first generated token (the blank token and end-of-text); ``max_initial_timestamp`` counts timestamp steps (0.02 s each)
    from ``timestamp_begin``, < 0 = no cap."""
    eot: int
    timestamp_begin: int
    no_timestamps: int = -1
    max_initial_timestamp: int = -1
    suppress: tuple = ()
    blank: tuple = ()


def check_ragged(what: str, lengths, *, beams: int = 1, path: str = "auto", kv32: bool = False, fp32: bool = False) -> None:
    """the refusals of a ragged prompt batch (``lengths`` given), before anything touches a device: each names the form that runs"""
    if lengths is None:
        return
    if beams != 1:
        raise NotImplementedError(f"{what}: lengths= (ragged prompts) follows one hypothesis per row; beam search takes a rectangular "
                                  "prompt: beams=1, or one call per distinct prompt length without lengths=")
    if path == "persistent":
        raise NotImplementedError(f"{what}: lengths= does not run on path='persistent' (its self-attention stage has no per-row first "
                                  "key); use path='launches'")
    if kv32:
        raise NotImplementedError(f"{what}: lengths= runs the unfused self-attention block on bf16 caches; the fp32-cache step "
                                  "(kv32=True / exact=True) is the fused block's: one call per distinct prompt length without lengths=")
    if fp32:
        raise NotImplementedError(f"{what}: lengths= needs bf16 parameters (model.to(torch.bfloat16)); fp32 parameters decode through "
                                  "greedy_exact: one call per distinct prompt length without lengths=")


def check_sampling_tail(what: str, topk: int, temperature: float, top_p: float, return_logprobs: bool, *, margins: bool = False,
                        beams: int = 1, path: str = "auto", kv32: bool = False, fp32: bool = False) -> bool:
    """whether the sampling tail (pm_dec_sample) is asked for - temperature != 1, top_p != 1, topk == 0 or return_logprobs - and then its
    argument checks (ValueError) and refusals, before anything touches a device: each names the form that does run"""
    if not wants_sampling_tail(topk, temperature, top_p, return_logprobs):
        return False
    check_sampling(what, topk, temperature, top_p)
    if beams != 1:
        raise ValueError(f"{what}: temperature / top_p / topk=0 / return_logprobs draw one hypothesis per row; beam search returns "
                         "its own scores (return_beams=True): beams=1, or these arguments at their defaults")
    if margins:
        raise ValueError(f"{what}: margins are an arg-max diagnostic of the default tail (topk == 1); with temperature / top_p / "
                         "topk=0 ask for return_logprobs=True instead")
    if path == "persistent":
        raise NotImplementedError(f"{what}: temperature / top_p / topk=0 / return_logprobs read the full logits of the launch-per-stage "
                                  "step; use path='launches' (or 'auto')")
    if kv32:
        raise NotImplementedError(f"{what}: the fp32-cache step (kv32=True / exact=True) promises the reference's arg-max ids; temperature / "
                                  "top_p / topk=0 / return_logprobs run on the bf16-cache step: exact=False")
    if fp32:
        raise NotImplementedError(f"{what}: temperature / top_p / topk=0 / return_logprobs need bf16 parameters (model.to(torch.bfloat16)); "
                                  "fp32 parameters decode through greedy_exact, arg-max only: leave these arguments at their defaults")
    return True


def _ragged_lengths(prompt: Tensor, lengths, longest: int | None = None) -> Tensor:
    """``lengths`` of a right-padded (B, P) prompt as int64 (B,) on the host; ValueError unless 1 <= len_b <= P (<= longest)"""
    if prompt.dim() != 2 or prompt.dtype != torch.int64 or prompt.shape[1] < 1:
        raise ValueError("greedy decode: prompt must be int64 (B, P >= 1)")
    B, P = prompt.shape
    lens = lengths.detach().cpu() if isinstance(lengths, Tensor) else torch.as_tensor(list(lengths))
    if lens.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or lens.shape != (B,):
        raise ValueError(f"greedy decode: lengths must be a sequence or integer tensor of shape ({B},), one prompt length per row")
    lens = lens.to(torch.int64)
    if B and (int(lens.min()) < 1 or int(lens.max()) > P):
        raise ValueError(f"greedy decode: every length must be in 1..{P} (the prompt's width)")
    if longest is not None and B and int(lens.max()) > longest:
        raise ValueError(f"greedy decode: this decoder was built for prompts of up to {longest} tokens")
    return lens


def _right_align(prompt: Tensor, lens: Tensor, width: int, pad: int) -> Tensor:
    """(B, width) with row b's len_b tokens at columns width - len_b .. width - 1 and ``pad`` in front (host indexing, no kernel)"""
    idx = torch.arange(width)[None, :] - (width - lens)[:, None]
    dev = prompt.device
    return torch.where((idx >= 0).to(dev), prompt.gather(1, idx.clamp(min=0).to(dev)), torch.full((), pad, dtype=torch.int64, device=dev))


class GreedyDecoder(plan.CapturedStep):
    """State + launch list of the decode step for one (decoder, batch, memory length) geometry."""
    _own_eos = False  # BeamDecoder: ``eos`` is beam search's own argument, at any width

    def __init__(self, dec, memory: Tensor, prompt: Tensor, n_new: int, margins: bool = False, fused: bool = True,
                 topk: int = 1, seed: int = 0, rules: "WhisperRules | None" = None, path: str = "auto", kv32: bool = False,
                 beams: int = 1, eos: int | None = None, prefill: bool = False, prefill_chunk: int | None = None, lengths=None,
                 pad_token_id: int = 0, *, temperature: float = 1.0, top_p: float = 1.0, return_logprobs: bool = False,
                 min_new_tokens: int = 0, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0) -> None:
        """``kv32``: the reference-accuracy form of the same step - fp32 memory in, cross and self K/V kept in fp32 (nothing is
        rounded when it is cached; pm_dec_attention_fused_kv32), everything else as in the throughput path, whose projections
        are fp32-exact already (bf16 weights x activations split into three bf16 terms) - graph-replayed like it.
        ``beams`` > 1 (through BeamDecoder): the same step at B * beams rows (row b * beams + w) in full-logit mode, ending in
        the beam kernels instead of a token choice; ``beams`` = 1 builds exactly the launch list it always did.
        ``prefill``: prompt positions 0 .. P - 2 go through the layers as one batched pass per ``prefill_chunk`` positions
        (default 512, PM_PREFILL_CHUNK) that fills the self-attention caches (prefill()); the step then starts at position
        P - 1 and runs n_new times instead of P + n_new - 1.  The step itself, and everything after the caches, is unchanged.
        ``lengths`` (B,) with 1 <= len_b <= P: a RAGGED batch - ``prompt`` is right-padded, row b's prompt is prompt[b, :len_b]
        (DESIGN.md section 19).  Internally the rows are right-aligned to Pm = max(lengths): row b's tokens sit at cache positions
        key_start[b] = Pm - len_b .. Pm - 1, ``P`` / ``Ttot`` / ``tokens`` / ``margins`` are in that layout (Pm + n_new wide), and
        output() shifts back.  The step keeps its one device position; the self block runs unfused (pm_dec_linear mode 1 +
        pm_dec_attention_ragged), the embedding rows take pos[max(0, t - key_start[b])].  Any ``lengths`` - all equal to P too -
        takes this path; ``lengths=None`` builds exactly the launch list it always did.
        ``temperature`` / ``top_p`` / ``topk`` = 0 / ``return_logprobs``: the sampling tail (pm_dec_sample) in
        place of the token choice - taken only when temperature != 1, top_p != 1, topk == 0 or return_logprobs; with the defaults
        the launch list is the one it always was.  ``logprobs`` (B, Ttot) f32 then holds every stepped position's log-probability
        (at temperature 1, after the controls and the rules); output_logprobs() returns the new positions in the caller's row layout.
        ``eos`` (beams = 1; under BeamDecoder it is beam search's own): row b FINISHES when a generated token equals it (a prompt-forced
        token never does) - pm_dec_finish behind the token tail, whichever it is, keeps ``finished`` (B,) int32 (0 = running, else the
        state column of the row's eos) and from then on writes ``pad_token_id`` and log-prob 0.0; run() polls
        ``finished`` every POLL_EVERY steps and stops early (``steps_run``); output_lengths() counts the generated tokens.  No launch
        in front of it changes: the ids up to each row's eos are those of the run without ``eos``.
        ``min_new_tokens`` (needs ``eos``) / ``repetition_penalty`` / ``no_repeat_ngram_size``: one pm_dec_controls launch on the full
        logits, between the vocabulary projection and the rules (whose -inf wins); any of them takes the full-logits route as
        ``rules`` does (topk == 1 without sampling = pm_dec_sample_topk at k = 1, the arg-max).  A row's history is its real tokens,
        prompt included, the padding of a ragged batch excluded.  With the defaults the launch list is the one it always was."""
        E0 = dec.token_embs.weight
        self._stops, self._controls = check_controls(
            "greedy decode", None if self._own_eos else eos, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size, vocab=E0.shape[0], margins=margins,
            beams=int(beams), path=path, kv32=kv32, fp32=E0.dtype == torch.float32)
        self._eos = int(eos) if self._stops else None
        self._ctl = dict(repetition_penalty=float(repetition_penalty), no_repeat_ngram=int(no_repeat_ngram_size),
                         min_new_tokens=int(min_new_tokens), eos=self._eos)
        self.steps_run = 0
        self._sampling = check_sampling_tail("greedy decode", topk, temperature, top_p, return_logprobs, margins=margins, beams=int(beams),
                                             path=path, kv32=kv32, fp32=dec.token_embs.weight.dtype == torch.float32)
        if path not in ("auto", "launches", "persistent"):
            raise ValueError("greedy decode: path must be 'auto', 'launches' or 'persistent'")
        self.W = int(beams)
        prompt, path = self._check_ragged(dec, prompt, lengths, pad_token_id, n_new, path, kv32)
        path = self._check_prefill(dec, prefill, prefill_chunk, path, kv32)
        path = self._check_request(path, topk, margins)
        prompt = self._check_geometry(dec, memory, prompt, n_new, kv32)
        self._choose_path(dec, path, fused)
        self._choose_attention(memory, fused, kv32)
        # plain projections with a long K (fc2: K = 4 d) are split over workgroups along K: see pm_dec_linear_ksplit
        super().__init__(self.B, self._E.device, k_split=int(os.environ.get("PM_DEC_KSPLIT", "4")),
                         ksplit_min_k=int(os.environ.get("PM_DEC_KSPLIT_MINK", "1024")))
        self.watch(dec)  # rebind() / run() refuse to go on once a parameter or buffer of the decoder changed
        self._allocate(dec, memory, prompt, margins)
        for layer in dec.layers:
            if not layer.pre_norm:
                raise NotImplementedError("greedy decode: pre-norm layers only (the post-norm GPT decodes through forward())")
            if (layer.ca is None) != (memory is None):
                raise ValueError("greedy decode: cross-attention layers need a memory, decoder-only layers must not get one")
            self._self_block(layer)
            if layer.ca is not None:
                self._cross_block(layer, memory.reshape(self.clips * self.S, self.d))
            self._mlp_block(layer, last=layer is dec.layers[-1])
        self.err = torch.zeros(1, dtype=torch.int32, device=self._E.device)
        if self.path == "persistent":
            self._persistent_table(dec)
        if not (1 <= topk <= 64 or (self._sampling and topk == 0)):
            raise ValueError("greedy decode: topk must be in 1..64")
        self.topk, self.temperature, self.top_p = topk, float(temperature), float(top_p)
        self._token_tail(dec, topk, seed, rules, margins, eos)
        if self._stops:  # behind the tail, whichever it was: no launch in front of it changes
            self.add(lib().pm_dec_finish, *plan.finish_args(self.tokens, self.tok_cur, self.logprobs, self.finished, self.pos, self.P,
                                                            self._eos, self._pad))
        self._prefill_setup(dec)

    # ---- what is asked for
    def _check_prefill(self, dec, prefill: bool, chunk: int | None, path: str, kv32: bool) -> str:
        """the refusals of the prompt pass, before anything touches a device: each names the form that does run"""
        self._prefill = bool(prefill)
        self._prefill_chunk = int(os.environ.get("PM_PREFILL_CHUNK", "512")) if chunk is None else int(chunk)
        if not prefill:
            return path
        if self._prefill_chunk < 1:
            raise ValueError("greedy decode: prefill_chunk must be >= 1")
        if path == "persistent":
            raise NotImplementedError("greedy decode: prefill=True does not run on path='persistent' (its arrival counters are epochs "
                                      "of the position, counted from 0); use path='launches', or prefill=False")
        if kv32:
            raise NotImplementedError("greedy decode: prefill=True fills bf16 caches; the fp32-cache step (kv32=True / exact=True) "
                                      "promises bit equality with the reference and keeps the token-by-token prompt: prefill=False")
        if dec.token_embs.weight.dtype == torch.float32:
            raise NotImplementedError("greedy decode: prefill=True needs bf16 parameters (model.to(torch.bfloat16)); fp32 parameters "
                                      "decode through greedy_exact, token by token: prefill=False")
        return "launches"  # 'auto' never picks the persistent kernel under prefill

    def _check_ragged(self, dec, prompt: Tensor, lengths, pad: int, n_new: int, path: str, kv32: bool) -> tuple:
        """the refusals and the argument checks of a ragged batch; returns (the right-aligned (B, max(lengths)) prompt, path).
        Sets _ragged, _P_in (the caller's prompt width), _pad and _starts (host int64 (B,): each row's first cache position)."""
        self._ragged, self._pad, self._starts = lengths is not None, int(pad), None
        self._P_in = prompt.shape[1] if prompt.dim() == 2 else 0
        if lengths is None:
            return prompt, path
        E = dec.token_embs.weight
        check_ragged("greedy decode", lengths, beams=self.W, path=path, kv32=kv32, fp32=E.dtype == torch.float32)
        lens = _ragged_lengths(prompt, lengths)
        longest = int(lens.max())
        if longest + n_new > dec.pos_embs.shape[0]:
            raise ValueError(f"greedy decode: {longest + n_new} positions (max(lengths) + new tokens) > max_seq_len {dec.pos_embs.shape[0]}")
        if not 0 <= self._pad < E.shape[0]:
            raise ValueError("greedy decode: pad_token_id outside the vocabulary")
        if int(prompt.min()) < 0 or int(prompt.max()) >= E.shape[0]:  # the padding too: its ids go through the embedding
            raise ValueError("greedy decode: prompt ids out of range")
        self._starts = longest - lens
        return _right_align(prompt, lens, longest, self._pad), "launches"  # 'auto' never picks the persistent kernel for a ragged batch

    def _check_request(self, path: str, topk: int, margins: bool) -> str:
        if self.W != 1:
            raise ValueError("greedy decode: beams > 1 is BeamDecoder's")
        return path

    def _rows(self, dec, prompt: Tensor, kv32: bool) -> Tensor:
        """the prompt of every ROW of the step (BeamDecoder: sequences x beams)"""
        return prompt

    def _check_geometry(self, dec, memory, prompt: Tensor, n_new: int, kv32: bool) -> Tensor:
        """validates; sets clips, B (rows), S, d, V, P, H, inner, Ttot, n_steps; returns the rows' prompt"""
        E = dec.token_embs.weight
        if E.dtype != torch.bfloat16 or not E.is_cuda:
            raise NotImplementedError("greedy decode: bf16 weights on a HIP device only (model.to(torch.bfloat16).cuda())")
        if memory is None:  # decoder-only language model (GPT-2): no cross-attention, nothing to attend to but itself
            B, S, d = prompt.shape[0], 0, E.shape[1]
        else:
            if memory.dtype != (torch.float32 if kv32 else torch.bfloat16) or memory.dim() != 3:
                raise ValueError("greedy decode: memory must be the encoder's (B, S, d) output, bf16 (fp32 with kv32=True)")
            B, S, d = memory.shape
        P = prompt.shape[1]
        if prompt.shape[0] != B or prompt.dtype != torch.int64 or P < 1:
            raise ValueError("greedy decode: prompt must be int64 (B, P >= 1)")
        V = E.shape[0]
        self._E, self.clips, self.S, self.d, self.V, self.P = E, B, S, d, V, P
        prompt = self._rows(dec, prompt, kv32)  # every buffer and launch below is per ROW
        B = prompt.shape[0]
        if int(prompt.min()) < 0 or int(prompt.max()) >= V:
            raise ValueError("greedy decode: prompt ids out of range")
        self.Ttot = P + n_new
        if self.Ttot > dec.pos_embs.shape[0]:
            raise ValueError(f"greedy decode: {self.Ttot} positions > max_seq_len {dec.pos_embs.shape[0]}")
        if B > 64:
            raise NotImplementedError("greedy decode: at most 64 sequences per call (shard larger batches)")
        ops.check_devices(E, memory, prompt if prompt.is_cuda else None)
        H = dec.layers[0].sa.n_heads
        for i, layer in enumerate(dec.layers):  # the launch list below is built per layer from ONE geometry
            for name, att in (("sa", layer.sa), ("ca", layer.ca)):
                if att is not None and (att.head_dim != 64 or att.n_heads != H or att.n_heads * 64 != d):
                    raise NotImplementedError(f"greedy decode: layer {i} {name}: head_dim 64 with n_heads * 64 == d_model in every "
                                              f"layer only (got {att.n_heads} x {att.head_dim}, d_model {d})")
        self.B, self.H, self.inner, self.n_steps = B, H, H * 64, self.Ttot - 1
        return prompt

    def _choose_path(self, dec, path: str, fused: bool) -> None:
        """One persistent launch for all layers of a step (csrc/decode_persist.hip) where its geometry rules hold; the
        launch-per-stage list otherwise (and on request: tests compare the two)"""
        d, L = self.d, lib()
        self._hid_max = hid_max = max(layer.mlp.linear1.out_features for layer in dec.layers)
        nstep = 4 if d <= 512 else 8 if d <= 1024 else 10
        self._ksp_p = ksp_p = -(-(hid_max // 32) // (4 * nstep))
        acts = {layer.mlp.act_name for layer in dec.layers}
        hids = {layer.mlp.linear1.out_features for layer in dec.layers}
        persist_ok = (all(layer.pre_norm for layer in dec.layers) and len(acts) == 1 and len(hids) == 1 and d % 64 == 0 and d <= 1280
                      and hid_max % 32 == 0 and ksp_p <= 8 and self.S <= 2048 and self.Ttot <= 2048 and fused
                      and len({layer.ca is None for layer in dec.layers}) == 1 and hasattr(L, "pm_dec_layers")
                      and L.pm_dec_layers_grid() > 0)
        if path == "persistent" and not persist_ok:
            raise NotImplementedError("greedy decode: the persistent layer kernel needs pre-norm layers of one MLP width and activation, "
                                      "d_model % 64 == 0 <= 1280, memory and total length <= 2048")
        env_path = os.environ.get("PM_DEC_PATH")
        if path == "auto" and env_path in ("launches", "persistent"):
            path = env_path if (env_path == "launches" or persist_ok) else "launches"
        self.path = "persistent" if (path == "persistent" or (path == "auto" and persist_ok and PERSISTENT_BY_DEFAULT)) else "launches"

    def _choose_attention(self, memory, fused: bool, kv32: bool) -> None:
        """the form of the self and cross blocks: sets _attn_fused, kv32, _fuse_self, _fuse_cross, _chain"""
        B, H, L = self.B, self.H, lib()
        # the attention block with the whole K stream in flight from the start (decode_persist.hip): opt-in, for A/B runs
        v2 = os.environ.get("PM_DEC_ATTN_V2", "0") != "0" and max(self.S, self.Ttot) <= 2048 and hasattr(L, "pm_dec_attention_fused_v2")  # measured slower (527 vs 461 us per step): off
        self._attn_fused = L.pm_dec_attention_fused_v2 if v2 else L.pm_dec_attention_fused
        self.kv32 = bool(kv32)
        if kv32:
            if self.path == "persistent" or not fused or B * H > 256 or os.environ.get("PM_DEC_FUSE_SELF") == "0" or os.environ.get("PM_DEC_FUSE_CROSS") == "0":
                raise NotImplementedError("greedy decode: fp32 K/V caches run on the fused attention blocks (B * n_heads <= 256)")
            self._attn_fused = L.pm_dec_attention_fused_kv32
        # the fused self block is one 512-thread workgroup per (sequence, head) that pulls the head's q/k/v weights
        # (3 * 64 * d * 2 B) through its CU: it wins while every workgroup has a CU to itself (B * H <= 256 on MI355X:
        # Whisper-base b = 32), beyond that the row-split projection + attention pair is faster (GPT-2 small b = 32,
        # B * H = 384: 705 -> 641 us per step)
        env_fs = os.environ.get("PM_DEC_FUSE_SELF")
        self._fuse_self = fused and (B * H <= 256 if env_fs is None else env_fs != "0")
        self._fuse_cross = fused and os.environ.get("PM_DEC_FUSE_CROSS", "1") != "0"
        # the chain of deferred sums (pm_dec_attention_chain): the self block leaves its output projection as per-head partial
        # sums that the cross block adds while it loads its row, fc2 leaves its K parts to the next layer's self block - one
        # launch and one ticket pass per layer less.  Needs both blocks fused (their workgroups own whole rows).
        self._chain = (self._fuse_self and self._fuse_cross and memory is not None and self.path != "persistent" and not v2
                       and os.environ.get("PM_DEC_CHAIN", "1") != "0")
        if self._ragged:  # the fused self block and the chain have no per-row first key: the unfused pair; the cross block stays
            self._fuse_self = self._chain = False

    def _allocate(self, dec, memory, prompt: Tensor, margins: bool) -> None:
        """the state of a run and the scratch rows of a step"""
        B, d, V, E, L = self.B, self.d, self.V, self._E, lib()
        dev = E.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.empty(B, d, **f32)
        self.q = torch.empty(B, self.inner, **f32)
        self.att = torch.empty(B, self.inner, **f32)
        self.h = torch.empty(B, self._hid_max, **f32)  # widest MLP of the stack (mlp_ratio is free: transformer.py:77)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.prompt = prompt.contiguous().to(dev)
        self.tok_cur = self.prompt[:, 0].clone()
        self.tokens = torch.zeros(B, self.Ttot, dtype=torch.int64, device=dev)
        self.tokens[:, : self.P] = self.prompt
        self.margins = torch.zeros(B, self.Ttot, **f32) if margins else None
        self.logprobs = torch.zeros(B, self.Ttot, **f32) if self._sampling else None  # an attribute: the plan points into it
        self.finished = torch.zeros(B, dtype=torch.int32, device=dev) if self._stops else None  # likewise; BeamDecoder has its own
        # d_model > 512: the final LayerNorm runs once as its own launch and the vocabulary projection without the
        # in-kernel LayerNorm, whose register budget would halve the feature tile (GPT-2 small: 101 -> ~55 us per step)
        self.split_final_norm = (d // 32 + 3) // 4 > 4
        tile = 64 if self.split_final_norm else L.pm_dec_argmax_tile(d)
        self._n_tiles = (V + tile - 1) // tile  # pm_dec_linear mode 2 leaves one (max, index) per tile and sequence
        self.ws_val = torch.empty(B, self._n_tiles, **f32)
        self.ws_idx = torch.empty(B, self._n_tiles, dtype=torch.int32, device=dev)
        self._pos_tab = _f32(dec, "pos", dec.pos_embs)
        self.keep(E, self._pos_tab, memory)
        self._lin = dict(geom=(self.inner, self.H, self.Ttot), pos=self.pos, argmax_ws=(self.ws_val, self.ws_idx))
        # x for position 0 comes from reset(); every later x row is written by the previous step's pm_dec_next_token
        self._embed0 = (L.pm_dec_embed, (self.tok_cur.data_ptr(), E.data_ptr(), self._pos_tab.data_ptr(), self.pos.data_ptr(),
                                         self.x.data_ptr(), B, d, V, None))
        self.key_start = None
        if self._ragged:  # in device memory: the captured step serves any lengths, rebind() rewrites it in place
            self.key_start = self._starts.to(device=dev, dtype=torch.int32)
            self._embed0 = (L.pm_dec_embed_ragged, plan.ragged_embed_args(self.tok_cur, E, self._pos_tab, self.pos, self.key_start, self.x))
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.fc2_parts = None
        self.head_parts = torch.empty(B * self.H * d, **f32) if self._chain else None
        self.x2 = torch.empty(B, d, **f32) if self._chain else None
        # the chain's hand-off: the residual stream's buffer, the other one, the sums the next chain block must add
        self._cur, self._oth, self._pending = self.x, self.x2, None
        self.self_k, self.self_v, self.cross_kv, self._cross_w, self._table = [], [], [], [], []

    # ---- the blocks of a layer
    def _self_block(self, layer) -> None:
        B, H, d, Tmax, L, sa, cur = self.B, self.H, self.d, self.Ttot, lib(), layer.sa, self._cur
        kc = torch.empty(B, H, Tmax, 64, dtype=torch.float32 if self.kv32 else torch.bfloat16, device=cur.device)
        vc = torch.empty_like(kc)
        self.self_k.append(kc)
        self.self_v.append(vc)
        wqkv, bqkv = sa._pack("qkv")
        ln = _ln(layer.sa_norm)
        wo, bo = sa.out_proj.weight, _f32(sa.out_proj, "b", sa.out_proj.bias)
        self.keep(wqkv, bqkv, ln[0], ln[1], wo, bo)
        kv = plan.cache_kv(kc, vc)
        if self.path == "persistent":
            self._table.append(DecLayer())
            self._record(sa_g=ln[0], sa_b=ln[1], w_qkv=wqkv, b_qkv=bqkv, kc=kc, vc=vc, w_so=wo, b_so=bo, sa_eps=float(ln[2]))
        elif self._chain:
            parts = self._pending
            self.add(L.pm_dec_attention_chain, *plan.chain_args(
                cur, ln, wqkv, bqkv, kv, B, H, self_attn=True, pos=self.pos, n_keys=Tmax, kv_f32=self.kv32, parts=parts,
                x_out=self._oth if parts is not None else None, w_out=wo, head_parts=self.head_parts))
            if parts is not None:
                self._cur, self._oth = self._oth, self._cur
            self._pending = plan.Parts(H, self.head_parts, d, H * d, bo)
        elif self._fuse_self:  # LN + q/k/v projection + cache append + attention in one launch per layer
            self.add(self._attn_fused, *plan.fused_args(cur, ln, wqkv, bqkv, kv, self.att, B, H, self_attn=True, pos=self.pos,
                                                        n_keys=Tmax))
        else:
            self.linear(cur, wqkv, self.q, ln=ln, bias=bqkv, mode=1, cache=(kc, vc))
            if self._ragged:
                self.add(L.pm_dec_attention_ragged, *plan.ragged_attention_args(self.q, kv, self.att, B, H, pos=self.pos, lk_add=1,
                                                                                lk_max=Tmax, key_start=self.key_start))
            else:
                self.add(L.pm_dec_attention, *plan.attention_args(self.q, kv, self.att, B, H, pos=self.pos, lk_add=1, lk_max=Tmax))
        if self.path != "persistent" and not self._chain:
            self.linear(self.att, wo, cur, bias=bo, resid=cur)

    def _cross_block(self, layer, mem2: Tensor) -> None:
        """cross attention: K/V of the memory projected ONCE (the reference re-projects them on every call,
        transformer.py:44-49), kept packed (B, S, [k | v]) in bf16"""
        B, H, S, L, ca, cur = self.B, self.H, self.S, lib(), layer.ca, self._cur
        wkv, bkv = ca._pack("kv")
        kvt = self._project_memory(mem2, wkv, bkv)
        self.cross_kv.append(kvt)
        self._cross_w.append((wkv, bkv))
        ln = _ln(layer.ca_norm)
        wq, bq = ca.q_proj.weight, _f32(ca.q_proj, "b", ca.q_proj.bias)
        wo, bo = ca.out_proj.weight, _f32(ca.out_proj, "b", ca.out_proj.bias)
        self.keep(ln[0], ln[1], wq, bq)
        kv = plan.packed_kv(kvt, S, self.inner)
        if self.path == "persistent":
            return self._record(ca_g=ln[0], ca_b=ln[1], ca_eps=float(ln[2]), w_q=wq, b_q=bq, cross_kv=kvt, w_co=wo, b_co=bo)
        if self._chain:  # x = the stream + the self block's projection (heads in order) + its bias, formed while loading
            self.add(L.pm_dec_attention_chain, *plan.chain_args(cur, ln, wq, bq, kv, B, H, self_attn=False, n_keys=S, kv_f32=self.kv32,
                                                                parts=self._pending, x_out=self._oth, out=self.att))
            self._cur, self._oth = self._oth, self._cur
            self._pending = None
        elif self._fuse_cross:
            self.add(self._attn_fused, *plan.fused_args(cur, ln, wq, bq, kv, self.att, B, H, self_attn=False, n_keys=S))
        else:
            self.linear(cur, wq, self.q, ln=ln, bias=bq)
            self.add(L.pm_dec_attention, *plan.attention_args(self.q, kv, self.att, B, H, pos=None, lk_add=S, lk_max=S))
        self.linear(self.att, wo, self._cur, bias=bo, resid=self._cur)

    def _mlp_block(self, layer, last: bool) -> None:
        B, d, mlp, cur = self.B, self.d, layer.mlp, self._cur
        ln = _ln(layer.mlp_norm)
        if mlp.act_name not in ("gelu", "approximate_gelu"):
            raise NotImplementedError("greedy decode: GELU / tanh-GELU MLPs only")
        hid = mlp.linear1.out_features
        if hid % 32 or mlp.linear2.in_features != hid or self.h[:, :hid].shape[1] != hid:
            raise NotImplementedError(f"greedy decode: MLP hidden width {hid} must be a multiple of 32 and fit the scratch row")
        w1, b1 = mlp.linear1.weight, _f32(mlp.linear1, "b", mlp.linear1.bias)
        w2, b2 = mlp.linear2.weight, _f32(mlp.linear2, "b", mlp.linear2.bias)
        if self.path == "persistent":
            return self._record(mlp_g=ln[0], mlp_b=ln[1], mlp_eps=float(ln[2]), w1=w1, b1=b1, w2=w2, b2=b2)
        self.linear(cur, w1, self.h[:, :hid], ln=ln, bias=b1, act=ops.ACT[mlp.act_name])
        ksp = self.ksplit(hid)
        if self._chain and not last and ksp:
            # fc2's K parts stay parts: the next layer's self block adds them (with the bias and this stream) while it loads
            if self.fc2_parts is None:
                self.fc2_parts = torch.empty(8, B, d, dtype=torch.float32, device=cur.device)
            self.keep(w2, b2)
            self.add(lib().pm_dec_linear_kparts, *plan.kparts_args(self.h, w2, self.fc2_parts, B, ksp))
            self._pending = plan.Parts(ksp, self.fc2_parts, B * d, d, b2)
        else:
            self.linear(self.h[:, :hid], w2, cur, bias=b2, resid=cur)

    def _record(self, **fields) -> None:
        """fields of the current layer's record of the persistent table: tensors go in as pointers and are kept alive"""
        for name, v in fields.items():
            if isinstance(v, Tensor):
                self.keep(v)
                v = v.data_ptr()
            setattr(self._table[-1], name, v)

    def _persistent_table(self, dec) -> None:
        """the layers' records on the device and the one launch that walks them"""
        import ctypes

        B, d, table, dev = self.B, self.d, self._table, self._E.device
        arr = (DecLayer * len(table))(*table)
        self.table = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))), dtype=torch.uint8).to(dev)
        mt = (B + 15) // 16
        self.ps_cnt = torch.zeros(len(table) * 24, dtype=torch.int32, device=dev)
        ws = torch.empty((d // 16) * mt * self._ksp_p * 256, dtype=torch.float32, device=dev)
        tick = torch.zeros((d // 16) * mt, dtype=torch.int32, device=dev)
        self.keep(ws)
        self._ks_cnts.append(tick)
        self.add(lib().pm_dec_layers, self.table.data_ptr(), len(table), B, d, self.H, self.S, self.Ttot, self._hid_max,
                 ops.ACT[dec.layers[0].mlp.act_name], self._ksp_p, self.pos.data_ptr(), self.x.data_ptr(), self.att.data_ptr(),
                 self.h.data_ptr(), self.h.stride(0), self.ps_cnt.data_ptr(), ws.data_ptr(), tick.data_ptr(), self.err.data_ptr(), None)

    # ---- from the last layer's row to the next token
    def _final_norm(self, dec) -> tuple:
        """(x, ln) for the vocabulary projection: the stream and the final LayerNorm, or (d_model > 512) the stream normed by a
        launch of its own and no LayerNorm.  (The chain leaves the stream in x or x2; the next step's row always goes to x.)"""
        g, b, eps = _ln(dec.norm)
        if not self.split_final_norm:
            return self._cur, (g, b, eps)
        self.xn = torch.empty_like(self.x)
        self.keep(g, b)
        self.add(lib().pm_layernorm, self._cur.data_ptr(), self.d, 1, g.data_ptr(), b.data_ptr(), float(eps), self.xn.data_ptr(), self.d, 1,
                 self.B, self.d, None)
        return self.xn, (None, None, eps)

    def _full_logits(self, xl: Tensor, ln: tuple, rules: "WhisperRules | None") -> None:
        """logits of the last position for every row, then the controls and the logit filters (k = 1 after them = arg-max)"""
        B, V, P, L = self.B, self.V, self.P, lib()
        self.logits = torch.empty(B, V, dtype=torch.float32, device=xl.device)
        self.linear(xl, self._E, self.logits, ln=ln, mode=0)
        if self._controls:  # in front of the rules: their -inf wins
            self.add(L.pm_dec_controls, *plan.controls_args(self.logits, self.tokens, self.pos, P, self.key_start, **self._ctl))
        if rules is not None:
            i32 = dict(dtype=torch.int32, device=xl.device)
            sup, blk = torch.tensor(list(rules.suppress), **i32), torch.tensor(list(rules.blank), **i32)
            if not (0 <= rules.eot < rules.timestamp_begin < V) or any(not 0 <= int(i) < V for i in (*rules.suppress, *rules.blank)):
                raise ValueError("WhisperRules: need 0 <= eot < timestamp_begin < vocab and listed ids inside the vocabulary")
            self.keep(sup, blk)
            self.add(L.pm_dec_whisper_rules, self.logits.data_ptr(), self.logits.stride(0), V, self.tokens.data_ptr(), self.Ttot,
                     self.pos.data_ptr(), P, rules.eot, rules.no_timestamps, rules.timestamp_begin, rules.max_initial_timestamp,
                     sup.data_ptr() if sup.numel() else None, sup.numel(), blk.data_ptr() if blk.numel() else None, blk.numel(),
                     B, None)

    def _token_tail(self, dec, topk: int, seed: int, rules, margins: bool, eos) -> None:
        B, d, V, P, E, L = self.B, self.d, self.V, self.P, self._E, lib()
        xl, ln = self._final_norm(dec)
        if self._sampling:  # full logits, the rules, then temperature / top-k / top-p / log-prob and the tail in one launch
            self._full_logits(xl, ln, rules)
            state = (self.logits, topk, self.temperature, self.top_p, seed, self.pos, self.prompt, self.tok_cur, self.tokens, self.logprobs,
                     E, self._pos_tab)
            if self._ragged:
                return self.add(L.pm_dec_sample_ragged, *plan.ragged_sample_args(*state, self.key_start, self.x, self.ticket))
            return self.add(L.pm_dec_sample, *plan.sample_args(*state, self.x, self.ticket))
        if topk == 1 and rules is None and not self._controls:
            self.linear(xl, E, None, ln=ln, mode=2)
            # token choice + the next step's embedding row + position advance: one launch
            if self._ragged:
                return self.add(L.pm_dec_next_token_ragged, *plan.ragged_next_token_args(
                    self.ws_val, self.ws_idx, self.pos, self.prompt, self.tok_cur, self.tokens, self.margins, E, self._pos_tab,
                    self.key_start, self.x, self.ticket))
            self.add(L.pm_dec_next_token, self.ws_val.data_ptr(), self.ws_idx.data_ptr(), self._n_tiles, self.pos.data_ptr(),
                     self.prompt.data_ptr(), P, self.tok_cur.data_ptr(), self.tokens.data_ptr(), self.Ttot, plan.ptr(self.margins),
                     E.data_ptr(), self._pos_tab.data_ptr(), self.x.data_ptr(), d, V, self.ticket.data_ptr(), B, None)
        else:  # top-k sampling on the device (text/generator.py:30-32): full logits of the last position, then the draw
            if margins:
                raise ValueError("greedy decode: margins are an arg-max diagnostic (topk == 1)")
            self._full_logits(xl, ln, rules)
            if self._ragged:
                return self.add(L.pm_dec_sample_topk_ragged, *plan.ragged_sample_topk_args(
                    self.logits, topk, seed, self.pos, self.prompt, self.tok_cur, self.tokens, E, self._pos_tab, self.key_start, self.x,
                    self.ticket))
            self.add(L.pm_dec_sample_topk, self.logits.data_ptr(), self.logits.stride(0), V, topk, int(seed) & (2**64 - 1),
                     self.pos.data_ptr(), self.prompt.data_ptr(), P, self.tok_cur.data_ptr(), self.tokens.data_ptr(), self.Ttot,
                     E.data_ptr(), self._pos_tab.data_ptr(), self.x.data_ptr(), d, self.ticket.data_ptr(), B, None)

    def _project_memory(self, mem2: Tensor, wkv: Tensor, bkv, out: Tensor | None = None) -> Tensor:
        """packed cross K/V of the memory rows: bf16 GEMM, or (kv32) the exact fp32 product of the fp32 memory with the
        bf16-valued weights."""
        if not self.kv32:
            return ops.linear(mem2, wkv, bkv, out=out)
        from ..transformer import derived

        w32 = derived(self, ("kv32w", wkv.data_ptr()), (wkv,), lambda: wkv.float())
        return ops.linear_f32(mem2, w32, bkv, out=out)

    # ---- the prompt pass
    def _prefill_setup(self, dec) -> None:
        """the chunks of positions 0 .. P - 2, the layers' operands and the scratch of the widest chunk - all allocated here, so
        that rebind() and repeated run() allocate nothing"""
        n_pre = self.P - 1
        self._pre_chunks = []
        if not self._prefill or n_pre == 0:  # a one-token prompt has nothing to prefill: the run is the plain one
            return
        if self.Ttot > 4096:
            raise NotImplementedError("greedy decode: prefill=True covers caches of up to 4096 positions")
        B, d, inner, dev = self.B, self.d, self.inner, self._E.device
        C = min(self._prefill_chunk, n_pre)
        self._pre_chunks = [(p0, min(C, n_pre - p0)) for p0 in range(0, n_pre, C)]
        self.n_steps = self.Ttot - self.P  # the step starts at position P - 1
        bf, f32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev)
        n = B * C
        self._pre_tok = torch.empty(n, dtype=torch.int64, device=dev)
        self._pre_x = [torch.empty(n * d, **f32), torch.empty(n * d, **f32)]  # the f32 residual stream, in and out of a block
        self._pre_xn = torch.empty(n * d, **bf)
        self._pre_qkv = torch.empty(n * 3 * inner, **bf)
        self._pre_att = torch.empty(n * inner, **bf)
        self._pre_h = torch.empty(n * self._hid_max, **bf)
        self._pre_layers = []
        for layer in dec.layers:
            sa, ca, mlp = layer.sa, layer.ca, layer.mlp
            rec = dict(sa_ln=_ln(layer.sa_norm), wqkv=sa._pack("qkv"), so=(sa.out_proj.weight, _f32(sa.out_proj, "b", sa.out_proj.bias)))
            if ca is not None:
                rec.update(ca_ln=_ln(layer.ca_norm), wq=(ca.q_proj.weight, _f32(ca.q_proj, "b", ca.q_proj.bias)),
                           co=(ca.out_proj.weight, _f32(ca.out_proj, "b", ca.out_proj.bias)))
            rec.update(mlp_ln=_ln(layer.mlp_norm), w1=(mlp.linear1.weight, _f32(mlp.linear1, "b", mlp.linear1.bias)),
                       w2=(mlp.linear2.weight, _f32(mlp.linear2, "b", mlp.linear2.bias)), act=mlp.act_name)
            self._pre_layers.append(rec)

    def _prefill_chunk_pass(self, p0: int, c: int, log: list | None) -> None:
        """positions p0 .. p0 + c - 1 of every row through the layers: bf16 where forward() rounds (LayerNorm output, q/k/v,
        attention output, MLP hidden), the residual stream in f32 like the step's.  The last layer stops after its attention
        kernel: the caches are full then, and the step recomputes position P - 1 from its own embedding row."""
        B, d, H, inner, S = self.B, self.d, self.H, self.inner, self.S
        n = B * c
        view = lambda buf, cols: buf[: n * cols].view(n, cols)  # noqa: E731
        tok = self._pre_tok[:n].view(B, c)
        tok.copy_(self.prompt[:, p0 : p0 + c])
        x, y = view(self._pre_x[0], d), view(self._pre_x[1], d)
        xn, qkv, att, q = view(self._pre_xn, d), view(self._pre_qkv, 3 * inner), view(self._pre_att, inner), view(self._pre_qkv, inner)
        if self._ragged:
            ops.embed_tokens_ragged(tok, self._E, self._pos_tab, self.key_start, pos0=p0, out_dtype=torch.float32, out=x.view(B, c, d))
        else:
            ops.embed_tokens(tok, self._E, self._pos_tab, pos0=p0, out_dtype=torch.float32, out=x.view(B, c, d))
        for l, rec in enumerate(self._pre_layers):
            if log is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                log.append((l, e0, e1))
            ops.layernorm(x, *rec["sa_ln"], out=xn)
            ops.linear(xn, *rec["wqkv"], out=qkv)
            if self._ragged:
                ops.prefill_attention_ragged(qkv, self.self_k[l], self.self_v[l], H, p0, self.key_start, out=att)
            else:
                ops.prefill_attention(qkv, self.self_k[l], self.self_v[l], H, p0, out=att)
            if l + 1 < len(self._pre_layers):
                ops.linear(att, *rec["so"], resid=x, out=y)
                x, y = y, x
                if "wq" in rec:
                    kv = self.cross_kv[l].view(B, S, 2 * inner)
                    ops.layernorm(x, *rec["ca_ln"], out=xn)
                    ops.linear(xn, *rec["wq"], out=q)
                    ops.attention(q.view(B, c, inner), kv[..., :inner], kv[..., inner:], H, out=att.view(B, c, inner))
                    ops.linear(att, *rec["co"], resid=x, out=y)
                    x, y = y, x
                hid = rec["w1"][0].shape[0]
                h = view(self._pre_h, hid)
                ops.layernorm(x, *rec["mlp_ln"], out=xn)
                ops.linear(xn, *rec["w1"], act=rec["act"], out=h)
                ops.linear(h, *rec["w2"], resid=x, out=y)
                x, y = y, x
            if log is not None:
                e1.record()

    def prefill(self, log: list | None = None) -> None:
        """After reset(): fill every layer's self-attention caches for positions 0 .. P - 2, chunk by chunk (eagerly, outside
        the captured step: a chunk's first position is a host integer), then put the step at position P - 1 with the last
        prompt token.  ``log`` collects (layer, start event, end event) per layer and chunk."""
        for p0, c in self._pre_chunks:
            self._prefill_chunk_pass(p0, c, log)
        self.pos.fill_(self.P - 1)
        self.tok_cur.copy_(self.prompt[:, self.P - 1])
        self.start()  # x[b] = emb[prompt[b, P - 1]] + pos[P - 1]

    def rebind(self, memory: Tensor, prompt: Tensor, lengths=None) -> None:
        """New clips, same geometry: re-project the cross K/V INTO the existing buffers and swap the prompt, so the
        captured graph (which holds raw pointers) stays valid.  A decoder built with ``lengths`` takes new ones here (each at
        most the longest it was built for): key_start is rewritten in place, the same graph serves them.  RuntimeError once the
        decoder's parameters changed (CapturedStep.check_model): the plan points into the old derived weights - build a new one."""
        self.check_model()
        assert (self.clips, self._P_in) == tuple(prompt.shape)
        if self._ragged != (lengths is not None):
            raise ValueError("greedy decode: rebind() takes lengths= exactly when the decoder was built with lengths=")
        if self._ragged:
            lens = _ragged_lengths(prompt, lengths, longest=self.P)
            if int(prompt.min()) < 0 or int(prompt.max()) >= self.V:
                raise ValueError("greedy decode: prompt ids out of range")
            self._starts = self.P - lens
            self.key_start.copy_(self._starts.to(torch.int32))
            prompt = _right_align(prompt, lens, self.P, self._pad)
        if memory is not None:
            B, S, d = memory.shape
            assert B == self.clips and memory.dtype == (torch.float32 if self.kv32 else torch.bfloat16)
            mem2 = memory.reshape(B * S, d)
            for kv, (wkv, bkv) in zip(self.cross_kv, self._cross_w):
                assert kv.shape[0] == self.B * S
                self._project_memory(mem2, wkv, bkv, out=kv)
        self.prompt.copy_(prompt if self.W == 1 else prompt.repeat_interleave(self.W, 0))
        self.tokens[:, : self.P] = self.prompt
        if self._stops:
            self.finished.zero_()

    def reset(self) -> None:
        self.pos.zero_()
        self.ticket.zero_()
        self.err.zero_()
        if self._stops:
            self.finished.zero_()  # no row has finished
        if self.path == "persistent":
            self.ps_cnt.zero_()  # arrival counters count up by epochs of the position: zero with it
        self.tok_cur.copy_(self.prompt[:, 0])
        self.start()  # x[b] = emb[prompt[b, 0]] + pos[0]

    def run(self, graph: bool = True) -> Tensor:
        one_step = self.begin(graph)
        if self._pre_chunks:
            self.prefill()
        if not self._stops:
            for _ in range(self.n_steps):
                one_step()
            self.steps_run = self.n_steps
            return self.tokens
        done = 0
        while done < self.n_steps:
            for _ in range(min(POLL_EVERY, self.n_steps - done)):
                one_step()
            done = min(done + POLL_EVERY, self.n_steps)
            if done < self.n_steps and int(self.finished.min()) > 0:  # one read-back: every row has emitted its eos
                break
        self.steps_run = done
        if done < self.n_steps:  # the positions never stepped: what pm_dec_finish would have written there
            c0 = (self.P - 1 if self._pre_chunks else 0) + done + 1
            self.tokens[:, c0:] = self._pad
            for buf in (self.logprobs, self.margins):
                if buf is not None:
                    buf[:, c0:] = 0.0
        return self.tokens

    def output_lengths(self) -> Tensor:
        """(B,) int64: the number of generated tokens of every row of the last run, its eos included; n_new for a row that never
        finished (and for every row of a decoder built without ``eos``).  The caller's row order, ragged or not."""
        n = self.Ttot - self.P
        if not self._stops:
            return torch.full((self.B,), n, dtype=torch.int64, device=self.tokens.device)
        f = self.finished.to(torch.int64)
        return torch.where(f > 0, f - self.P + 1, torch.full_like(f, n))

    def _live_margins(self) -> "Tensor | None":
        """margins with zeros behind a finished row's eos: the default tail goes on writing the margins of what it picks there"""
        if self.margins is None or not self._stops:
            return self.margins
        f = self.finished.to(torch.int64)[:, None]
        cols = torch.arange(self.Ttot, device=self.margins.device)[None, :]
        return torch.where((f > 0) & (cols > f), torch.zeros((), device=self.margins.device), self.margins)

    def output(self) -> tuple:
        """(tokens, margins or None) of the last run in the caller's layout.  Rectangular prompts: the state itself.  Ragged: (B,
        P + n_new), row b = its prompt, its new ids, then P - len_b times pad_token_id (margins: zeros) - host indexing of the
        right-aligned state."""
        margins = self._live_margins()
        if not self._ragged:
            return self.tokens, margins
        dev = self.tokens.device
        idx = torch.arange(self._P_in + self.Ttot - self.P)[None, :] + self._starts[:, None]
        live, idx = (idx < self.Ttot).to(dev), idx.clamp(max=self.Ttot - 1).to(dev)
        toks = torch.where(live, self.tokens.gather(1, idx), torch.full((), self._pad, dtype=torch.int64, device=dev))
        marg = None if margins is None else torch.where(live, margins.gather(1, idx), torch.zeros((), device=dev))
        return toks, marg

    def output_logprobs(self) -> Tensor:
        """(B, n_new) f32: the log-probability of every new token of the last run (at temperature 1, of the logits after the controls
        and the rules; exactly 0.0 behind a finished row's eos, so sum(-1) is the sequence log-probability), in the caller's
        row order - for a ragged run row b's new ids sit at state columns P .. Ttot - 1 whatever its length, as output() knows"""
        if self.logprobs is None:
            raise ValueError("greedy decode: this decoder was built without return_logprobs / the sampling tail")
        return self.logprobs[:, self.P:].clone()

    def check(self) -> None:
        """Raise if a hand-off inside the persistent step kernel gave up (one read-back: call it where the tokens are consumed)."""
        if self.path == "persistent" and int(self.err.item()) != 0:
            raise RuntimeError("greedy decode: a hand-off of the persistent decode-step kernel timed out (not every workgroup of "
                               "the launch was resident, or the device is shared); tokens of this run are invalid - re-run with "
                               "path='launches'")


class BeamDecoder(GreedyDecoder):
    """Fixed-shape beam search of width ``beams`` over B clips: GreedyDecoder's step at B * beams rows (row b * beams + w) in
    full-logit mode, then pm_dec_whisper_rules (optional), pm_dec_beam_topw, pm_dec_beam_select, pm_dec_beam_reorder - captured
    and replayed like the greedy step; parents, scores and the K/V re-gather never leave the device (DESIGN.md "Beam search").
    State: ``scores`` (B, W) f32, ``finished`` / ``parents`` (B, W) int32 (of the last step), ``tokens`` (B * W, P + n) int64,
    ``logits`` (B * W, V) f32 of the last step (after the rules), ``self_k`` / ``self_v`` per layer (B * W, H, P + n, 64).
    ``prefill``: GreedyDecoder's prompt pass at all B * W rows - the W rows of a clip hold the same prompt, so their caches come
    out identical up to position P - 2, which is what the beam kernels assume at the first generated position."""
    _own_eos = True

    def __init__(self, dec, memory: Tensor | None, prompt: Tensor, n_new: int, beams: int, *, eos: int | None = None,
                 rules: "WhisperRules | None" = None, path: str = "auto", kv32: bool = False, fused: bool = True,
                 prefill: bool = False, prefill_chunk: int | None = None) -> None:
        super().__init__(dec, memory, prompt, n_new, False, fused, 1, 0, rules, path, kv32, beams=beams, eos=eos, prefill=prefill,
                         prefill_chunk=prefill_chunk)

    def _check_request(self, path: str, topk: int, margins: bool) -> str:
        if not 1 <= self.W <= 8:
            raise ValueError("beam decode: beams must be in 1..8")
        if path == "persistent":
            raise NotImplementedError("beam decode: the persistent layer kernel follows one hypothesis per sequence (path='launches')")
        if topk != 1 or margins:
            raise ValueError("beam decode: topk sampling and arg-max margins are greedy decode's")
        return "launches"

    def _rows(self, dec, prompt: Tensor, kv32: bool) -> Tensor:
        """row b * W + w = beam w of clip b"""
        if self.clips * self.W > 64:
            raise NotImplementedError("beam decode: at most 64 rows (sequences x beams) per call (shard larger batches)")
        if self.W > self.V:
            raise ValueError("beam decode: more beams than vocabulary entries")
        if kv32 and self.clips * self.W * dec.layers[0].sa.n_heads > 256:
            raise NotImplementedError("beam decode: fp32 K/V caches run on the fused attention blocks (B * beams * n_heads <= 256)")
        return prompt.repeat_interleave(self.W, 0)

    def _token_tail(self, dec, topk: int, seed: int, rules, margins: bool, eos) -> None:
        """full logits (+ rules), then the W best continuations per clip, their bookkeeping and the caches' re-gather"""
        self._full_logits(*self._final_norm(dec), rules)
        B, W, V, E, L = self.clips, self.W, self.V, self._E, lib()
        dev = E.device
        if eos is None and rules is not None:
            eos = rules.eot
        if eos is not None and not 0 <= int(eos) < V:
            raise ValueError("beam decode: eos_token_id outside the vocabulary")
        self.eos = -1 if eos is None else int(eos)
        self.scores = torch.empty(B, W, dtype=torch.float32, device=dev)
        self.finished = torch.zeros(B, W, dtype=torch.int32, device=dev)
        self.parents = torch.zeros(B, W, dtype=torch.int32, device=dev)
        self._cand_score = torch.empty(B * W, W, dtype=torch.float32, device=dev)
        self._cand_tok = torch.zeros(B * W, W, dtype=torch.int32, device=dev)
        # the layers' (K, V) cache pointers, read by the one reorder launch
        self._cache_table = torch.tensor([c.data_ptr() for kv in zip(self.self_k, self.self_v) for c in kv], dtype=torch.int64,
                                         device=dev)
        self.add(L.pm_dec_beam_topw, self.logits.data_ptr(), self.logits.stride(0), V, W, self.scores.data_ptr(),
                 self.finished.data_ptr(), self.eos, self.pos.data_ptr(), self.P, self._cand_score.data_ptr(),
                 self._cand_tok.data_ptr(), B * W, None)
        self.add(L.pm_dec_beam_select, self._cand_score.data_ptr(), self._cand_tok.data_ptr(), W, self.scores.data_ptr(),
                 self.finished.data_ptr(), self.parents.data_ptr(), self.eos, self.tokens.data_ptr(), self.Ttot, self.pos.data_ptr(),
                 self.prompt.data_ptr(), self.P, self.tok_cur.data_ptr(), E.data_ptr(), self._pos_tab.data_ptr(), self.x.data_ptr(),
                 self.d, V, self.ticket.data_ptr(), B, None)
        self.add(L.pm_dec_beam_reorder, self._cache_table.data_ptr(), self._cache_table.numel(), self.parents.data_ptr(),
                 self.pos.data_ptr(), B, W, self.H, self.Ttot, int(self.kv32), None)

    def _project_memory(self, mem2: Tensor, wkv: Tensor, bkv, out: Tensor | None = None) -> Tensor:
        """cross K/V projected ONCE per clip, then copied to the clip's W rows (the attention blocks read one K/V image per row;
        sharing one between a clip's beams needs attention kernels of its own: DESIGN.md)."""
        kv = super()._project_memory(mem2, wkv, bkv)
        S = mem2.shape[0] // self.clips
        rows = kv.view(self.clips, 1, S, kv.shape[1]).expand(-1, self.W, -1, -1)
        if out is None:
            return rows.reshape(self.clips * self.W * S, kv.shape[1])
        out.view(self.clips, self.W, S, kv.shape[1]).copy_(rows)
        return out

    def reset(self) -> None:
        super().reset()
        self.scores.fill_(float("-inf"))  # only beam 0 is live at the first generated position: W distinct continuations
        self.scores[:, 0] = 0.0
        self.finished.zero_()
        self.parents.copy_(torch.arange(self.W, dtype=torch.int32, device=self.parents.device).expand_as(self.parents))

    def beams(self) -> tuple[Tensor, Tensor]:
        """(tokens (B, W, P + n) int64, scores (B, W) f32), best beam first"""
        return self.tokens.view(self.clips, self.W, self.Ttot), self.scores


@torch.no_grad()
def beam_decode(dec, memory: Tensor | None, prompt: Tensor, n_new: int, *, beams: int, eos_token_id: int | None = None,
                graph: bool = True, rules: "WhisperRules | None" = None, path: str = "auto", kv32: bool = False,
                return_beams: bool = False, prefill: bool = False, prefill_chunk: int | None = None):
    """Beam search of width ``beams`` (1..8, B * beams <= 64): the best hypothesis per sequence, (B, P + n_new) int64, or with
    ``return_beams`` (tokens (B, beams, P + n_new), scores (B, beams) f32 = sum of the tokens' log-probabilities), best first.
    No length penalty, no early exit: always n_new steps; a hypothesis that emitted ``eos_token_id`` (default: rules.eot when
    rules are given, else none) is extended with it at no cost.  ``prefill`` / ``prefill_chunk``: as in greedy_decode, at the
    B * beams rows."""
    st = BeamDecoder(dec, memory, prompt, n_new, beams, eos=eos_token_id, rules=rules, path=path, kv32=kv32, prefill=prefill,
                     prefill_chunk=prefill_chunk)
    st.run(graph)
    toks, scores = st.beams()
    return (toks.clone(), scores.clone()) if return_beams else toks[:, 0].clone()


@torch.no_grad()
def greedy_decode(dec, memory: Tensor, prompt: Tensor, n_new: int, *, graph: bool = True, margins: bool = False,
                  fused: bool = True, topk: int = 1, seed: int = 0, rules: "WhisperRules | None" = None, path: str = "auto",
                  kv32: bool = False, prefill: bool = False, prefill_chunk: int | None = None, lengths=None, pad_token_id: int = 0,
                  temperature: float = 1.0, top_p: float = 1.0, return_logprobs: bool = False, eos_token_id: int | None = None,
                  return_lengths: bool = False, min_new_tokens: int = 0, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
    """tokens (B, P + n_new) int64 [and per-position diagnostic margins].  fused=False uses the unfused
    projection + attention launches (same arithmetic, 2 more launches per layer); topk > 1 samples each token from the
    softmax over the k largest logits on the device (same seed -> same ids); path: "persistent" (all layers of a step in
    one launch), "launches" (a launch per stage) or "auto".  ``prefill``: the prompt's positions 0 .. P - 2 fill the caches in
    one batched pass per ``prefill_chunk`` positions (default 512) instead of one decode step each, and the step runs n_new
    times; bf16 parameters and caches, not path="persistent" (NotImplementedError otherwise).  The prompt pass rounds where
    forward() does, so its ids follow forward()'s contract (rel-L2 2e-2 on the logits), not the step's fp32-exact projections.
    ``lengths`` (a sequence or integer tensor (B,), 1 <= len_b <= P): a ragged batch - ``prompt`` is right-padded, row b of the result
    is prompt[b, :len_b], its n_new new ids, then P - len_b times ``pad_token_id``; margins are aligned the same way.  Row b is what
    this function returns for prompt[b:b+1, :len_b] alone.  Works with prefill, rules and top-k sampling (the draw is keyed by
    (seed, cache position, row), so a row's draws differ from those of the same row decoded alone); not with beams, path="persistent",
    kv32 or fp32 parameters (NotImplementedError), ValueError for lengths outside 1..P or max(lengths) + n_new > max_seq_len.
    ``temperature`` (finite, >= 0; 0 = arg-max), ``top_p`` in (0, 1], ``topk`` = 0 (the whole vocabulary) and ``return_logprobs`` take
    the sampling tail (pm_dec_sample): weights exp((l - max) / temperature) over the topk first tokens (or all),
    cut to the smallest set of highest logits whose mass reaches top_p (ties at the boundary kept), one draw keyed by (seed, cache
    position, row).  With ``return_logprobs`` the result is (tokens, logprobs (B, n_new) f32): each new token's log-probability at
    temperature 1 after the rules, what score() returns for it.  Works with prefill, lengths and rules; not with margins, beams
    (ValueError), path="persistent", kv32 or fp32 parameters (NotImplementedError).  With the defaults nothing changes.
    ``eos_token_id`` (None = never finish, also under ``rules``): row b finishes when a GENERATED token equals it (a prompt-forced one
    never does).  Its eos and the eos's log-prob stay; every later position holds ``pad_token_id`` (default 0) and log-prob exactly
    0.0, so logprobs.sum(-1) is the sequence log-probability and logprobs.sum(-1) / n_new Whisper's avg_logprob, eos included.  The
    run ends once every row has finished (polled every POLL_EVERY steps); the ids up to each row's eos are those of the run without
    it.  ``return_lengths`` appends n_new (B,) int64 as the LAST element of the result: the generated tokens of the row, its eos
    included, n_new for a row that never finished.
    ``min_new_tokens`` (needs eos_token_id): the logit of eos_token_id is -inf while fewer tokens have been generated.
    ``repetition_penalty`` r (finite, > 0): every distinct id v of the row's history, once: l[v] / r if l[v] > 0 else l[v] * r.
    ``no_repeat_ngram_size`` n (0..8): no n-gram occurs twice in a row - every id that would complete an n-gram the history (prompt
    included) already holds gets -inf; n = 1 bans every id of the history.  History = the row's real tokens (the padding of a
    ragged batch excluded); order in the step: vocabulary projection, these controls, the rules (whose -inf wins), the token tail;
    a reported log-prob is of the logits after controls and rules.  Any of the three takes the full-logits route as ``rules`` does.
    All of this works with prefill, lengths, rules, top-k and the sampling tail; ``eos_token_id`` alone also with margins (zeros behind
    the eos).  Refused before anything touches a device: a logit control with margins, beams (ValueError), path="persistent", kv32
    or fp32 parameters (NotImplementedError), eos / pad outside the vocabulary (ValueError)."""
    check_controls("greedy decode", eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size, return_lengths,
                   vocab=dec.token_embs.weight.shape[0], margins=margins, path=path, kv32=kv32,
                   fp32=dec.token_embs.weight.dtype == torch.float32)
    st = GreedyDecoder(dec, memory, prompt, n_new, margins, fused, topk, seed, rules, path, kv32, eos=eos_token_id, prefill=prefill,
                       prefill_chunk=prefill_chunk, lengths=lengths, pad_token_id=pad_token_id, temperature=temperature, top_p=top_p,
                       return_logprobs=return_logprobs, min_new_tokens=min_new_tokens, repetition_penalty=repetition_penalty,
                       no_repeat_ngram_size=no_repeat_ngram_size)
    st.run(graph)
    st.check()
    toks, marg = st.output()
    res = (toks, st.output_logprobs()) if return_logprobs else (toks, marg) if margins else (toks,)
    if return_lengths:
        res += (st.output_lengths(),)
    return res if len(res) > 1 else res[0]


@torch.no_grad()
def greedy_exact(dec, memory: Tensor | None, prompt: Tensor, n_new: int, *, margins: bool = False):
    """KV-cached greedy decoding in fp32 END TO END for a decoder whose parameters are fp32: fp32 weights, fp32 activations,
    fp32 self and cross K/V (nothing rounded to bf16 anywhere), one token per step through pm_linear_f32 /
    pm_attention_generic_f32 / pm_layernorm.  This is the path whose ids are compared bit for bit with the reference's fp32
    full-prefix loop (text/generator.py:23-35 semantics; tests/golden/whisper.npz greedy_*_224): same algebra as the
    reference, cached instead of recomputed (the single-token step attends WITHOUT a causal flag: SURVEY.md F3).
    ~14 eager launches per layer and step - a reference-accuracy mode, not the throughput path (that is GreedyDecoder on a
    bf16 model).  It is also the KV-cached decode of what GreedyDecoder's step kernels do not cover: post-norm stacks (GPT)
    and heads other than 64 wide / n_heads * head_dim != d_model (any head_dim % 8 == 0 up to 128).  Returns tokens (B, P + n_new) [and the top-1 minus top-2 logit of every generated position]."""
    from ..transformer import MHA

    E = dec.token_embs.weight
    if E.dtype != torch.float32 or not E.is_cuda:
        raise NotImplementedError("greedy_exact: fp32 parameters on a HIP device (bf16 models: GreedyDecoder, or Whisper.generate(exact=True))")
    B, P = prompt.shape
    V, d = E.shape
    Ttot = P + n_new
    if Ttot > dec.pos_embs.shape[0]:
        raise ValueError(f"greedy decode: {Ttot} positions > max_seq_len {dec.pos_embs.shape[0]}")
    dev = E.device
    prompt = prompt.to(dev)
    tokens = torch.zeros(B, Ttot, dtype=torch.int64, device=dev)
    tokens[:, :P] = prompt
    marg = torch.zeros(B, Ttot, dtype=torch.float32, device=dev) if margins else None
    pos = dec.pos_embs.float()
    layers = list(dec.layers)
    for layer in layers:
        if type(layer.sa) is not MHA or layer.sa.head_dim % 8 or layer.sa.head_dim > 128:
            raise NotImplementedError("greedy_exact: plain MHA layers with head_dim % 8 == 0 (<= 128)")
    cross, caches = [], []
    for layer in layers:
        inner = layer.sa.n_heads * layer.sa.head_dim
        caches.append((torch.empty(B, Ttot, inner, dtype=torch.float32, device=dev), torch.empty(B, Ttot, inner, dtype=torch.float32, device=dev)))
        if layer.ca is not None:
            if memory is None:
                raise ValueError("greedy_exact: cross-attention layers need a memory")
            w, b = layer.ca._pack32("kv")
            mem = memory.float()
            ci = layer.ca.n_heads * layer.ca.head_dim
            kv = ops.linear_f32(mem.reshape(-1, mem.shape[-1]), w, b).view(B, mem.shape[1], 2 * ci)
            cross.append((kv[..., :ci], kv[..., ci:]))
        else:
            cross.append(None)
    for t in range(Ttot - 1):
        x = ops.embed_tokens(tokens[:, t : t + 1], E, pos, pos0=t).view(B, d)  # f32 rows
        for layer, (kc, vc), xkv in zip(layers, caches, cross):
            # pre-norm: x + f(norm(x)); post-norm (GPT, text/gpt.py:23): norm(x + f(x)) - transformer.py:96-105
            pre = layer.pre_norm
            sa = layer.sa
            inner = sa.n_heads * sa.head_dim
            w, b = sa._pack32("qkv")
            qkv = ops.linear_f32(layer.sa_norm(x) if pre else x, w, b)
            kc[:, t] = qkv[:, inner : 2 * inner]
            vc[:, t] = qkv[:, 2 * inner :]
            a = ops.attention_f32(qkv[:, :inner].unsqueeze(1), kc[:, : t + 1], vc[:, : t + 1], sa.n_heads)
            x = ops.linear_f32(a.view(B, inner), sa.out_proj.weight, sa.out_proj.bias, resid=x)
            if not pre:
                x = layer.sa_norm(x)
            if xkv is not None:
                ca = layer.ca
                q = ops.linear_f32(layer.ca_norm(x) if pre else x, ca.q_proj.weight, ca.q_proj.bias)
                a = ops.attention_f32(q.unsqueeze(1), xkv[0], xkv[1], ca.n_heads)
                x = ops.linear_f32(a.view(B, -1), ca.out_proj.weight, ca.out_proj.bias, resid=x)
                if not pre:
                    x = layer.ca_norm(x)
            mlp = layer.mlp
            h = ops.linear_f32(layer.mlp_norm(x) if pre else x, mlp.linear1.weight, mlp.linear1.bias, act=mlp.act_name)
            x = ops.linear_f32(h, mlp.linear2.weight, mlp.linear2.bias, resid=x)
            if not pre:
                x = layer.mlp_norm(x)
        logits = ops.linear_f32(dec.norm(x) if getattr(dec, "norm", None) is not None else x, E)  # (B, V) f32
        if t + 1 < P:
            tokens[:, t + 1] = prompt[:, t + 1]
        else:
            if margins:
                top2 = logits.topk(2, -1)
                marg[:, t + 1] = top2.values[:, 0] - top2.values[:, 1]
                tokens[:, t + 1] = top2.indices[:, 0]
            else:
                tokens[:, t + 1] = logits.argmax(-1)
    return (tokens, marg) if margins else tokens
