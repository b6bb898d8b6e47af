"""Eos stopping and the repetition controls of a decode step on explicit state (csrc/controls.hip): what the
generators put into their launch lists as pm_dec_controls / pm_dec_finish, as standalone calls - and the one statement of which
(eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size) are allowed, shared with GreedyDecoder and
the models' generate().
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import decode_plan as plan, lib
from .ops import _apart, _cuda, _key_start, _need, _stream, capturing

MAX_NGRAM = 8       # pm_dec_controls compares at most 7 ids per candidate position
MAX_VOCAB = 1 << 18  # its set of seen ids is V bits of LDS


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def wants_logit_controls(min_new_tokens: int, repetition_penalty: float, no_repeat_ngram_size: int) -> bool:
    """a logit control is asked for: the step takes the full-logits route and gets one pm_dec_controls launch"""
    return min_new_tokens != 0 or repetition_penalty != 1.0 or no_repeat_ngram_size != 0


def check_controls(what: str, eos_token_id, pad_token_id, min_new_tokens, repetition_penalty, no_repeat_ngram_size,
                   return_lengths: bool = False, *, vocab: int | None = None, margins: bool = False, beams: int = 1, path: str = "auto",
                   kv32: bool = False, fp32: bool = False) -> tuple[bool, bool]:
    """(eos stopping is on, a logit control is on) - and, when either or ``return_lengths`` is asked for, the argument checks
    (ValueError) and the refusals, before anything touches a device: each names the form that does run.  With every argument at its
    default nothing is checked and a decoder builds the launch list it always built.  Under ``beams`` > 1 ``eos_token_id`` is beam
    search's own argument and does not count."""
    controls = wants_logit_controls(min_new_tokens, repetition_penalty, no_repeat_ngram_size)
    stops = eos_token_id is not None and beams == 1
    if not (controls or stops or return_lengths):
        return False, False
    if not _is_int(min_new_tokens) or min_new_tokens < 0:
        raise ValueError(f"{what}: min_new_tokens must be an integer >= 0, got {min_new_tokens!r}")
    if not _is_int(no_repeat_ngram_size) or not 0 <= no_repeat_ngram_size <= MAX_NGRAM:
        raise ValueError(f"{what}: no_repeat_ngram_size must be an integer in 0..{MAX_NGRAM} (0 = off), got {no_repeat_ngram_size!r}")
    try:
        r = float(repetition_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: repetition_penalty must be a number, got {repetition_penalty!r}") from None
    r32 = float(torch.tensor(r, dtype=torch.float32))
    if math.isnan(r) or math.isinf(r32) or not r32 > 0.0:
        raise ValueError(f"{what}: repetition_penalty must be a finite fp32 number > 0 (1 = off), got {repetition_penalty!r}")
    if beams != 1:
        raise ValueError(f"{what}: min_new_tokens / repetition_penalty / no_repeat_ngram_size / return_lengths follow one hypothesis "
                         "per row; beam search has eos_token_id of its own and returns its scores (return_beams=True): beams=1, or "
                         "these arguments at their defaults")
    if eos_token_id is not None and not _is_int(eos_token_id):
        raise ValueError(f"{what}: eos_token_id must be an integer or None, got {eos_token_id!r}")
    if min_new_tokens > 0 and eos_token_id is None:
        raise ValueError(f"{what}: min_new_tokens holds back eos_token_id, which is None: pass eos_token_id=, or min_new_tokens=0")
    if controls and margins:
        raise ValueError(f"{what}: margins are an arg-max diagnostic of the default tail's own logits; min_new_tokens / repetition_penalty "
                         "/ no_repeat_ngram_size edit the logits: margins=False, or eos_token_id alone (which keeps the default tail)")
    if path == "persistent":
        raise NotImplementedError(f"{what}: eos_token_id / min_new_tokens / repetition_penalty / no_repeat_ngram_size / return_lengths run "
                                  "in the launch-per-stage step; use path='launches' (or 'auto')")
    if kv32:
        raise NotImplementedError(f"{what}: the fp32-cache step (kv32=True / exact=True) promises the reference's arg-max ids for a fixed "
                                  "number of tokens; eos_token_id / min_new_tokens / repetition_penalty / no_repeat_ngram_size / "
                                  "return_lengths run on the bf16-cache step: exact=False")
    if fp32:
        raise NotImplementedError(f"{what}: eos_token_id / min_new_tokens / repetition_penalty / no_repeat_ngram_size / return_lengths need "
                                  "bf16 parameters (model.to(torch.bfloat16)); fp32 parameters decode through greedy_exact, a fixed "
                                  "number of arg-max tokens: leave these arguments at their defaults")
    if stops and not _is_int(pad_token_id):
        raise ValueError(f"{what}: pad_token_id must be an integer, got {pad_token_id!r}")
    if vocab is not None:
        if stops and not 0 <= eos_token_id < vocab:
            raise ValueError(f"{what}: eos_token_id {eos_token_id} outside the vocabulary [0, {vocab})")
        if stops and not 0 <= pad_token_id < vocab:
            raise ValueError(f"{what}: pad_token_id {pad_token_id} outside the vocabulary [0, {vocab})")
        if controls and vocab > MAX_VOCAB:
            raise NotImplementedError(f"{what}: min_new_tokens / repetition_penalty / no_repeat_ngram_size cover vocabularies of up to "
                                      f"{MAX_VOCAB} ids (the kernel's set of seen ids lives in LDS), got {vocab}")
    return stops, controls


def _pos_inside(what: str, pos: Tensor, Ttot: int) -> None:
    _need(pos.dtype == torch.int32 and pos.numel() == 1, f"{what}: pos is one device int32")
    # (a validation that reads *pos back: not under capture, where the position is whatever the replay finds there)
    _need(capturing() or 0 <= int(pos) < Ttot, f"{what}: the position must lie inside tokens")


def dec_controls(logits: Tensor, tokens: Tensor, pos: Tensor, P: int, *, key_start: Tensor | None = None, repetition_penalty: float = 1.0,
                 no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, eos_token_id: int | None = None) -> Tensor:
    """pm_dec_controls as a standalone op (the generator puts it into its launch list in front of pm_dec_whisper_rules): edits logits
    (B, V) f32 (unit column stride, rows that do not overlap) IN PLACE for the token at index pos + 1 of tokens (B, Ttot) int64 and
    returns them.  Row b's history is tokens[b, key_start[b] .. pos] (key_start int32 (B,), else from 0); nothing happens while
    pos + 1 < P."""
    check_controls("dec_controls", eos_token_id, 0, min_new_tokens, repetition_penalty, no_repeat_ngram_size)
    _cuda(logits, tokens, pos, key_start)
    _need(logits.dim() == 2 and logits.dtype == torch.float32 and (logits.shape[1] == 1 or logits.stride(1) == 1) and _apart(logits)
          and (logits.shape[0] == 1 or logits.stride(0) >= logits.shape[1]), "dec_controls: logits f32 (B, V) rows that do not overlap")
    B, V = logits.shape
    _need(1 <= V <= MAX_VOCAB, f"dec_controls: 1 <= V <= {MAX_VOCAB}")
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.shape[0] == B and 1 <= P <= tokens.shape[1],
          "dec_controls: contiguous int64 tokens (B, Ttot >= P >= 1)")
    _need(eos_token_id is None or 0 <= eos_token_id < V, "dec_controls: eos_token_id outside the vocabulary")
    _pos_inside("dec_controls", pos, tokens.shape[1])
    if key_start is not None:
        _key_start(key_start, B, "dec_controls")
    plan.call(lib().pm_dec_controls, plan.controls_args(logits, tokens, pos, P, key_start, repetition_penalty=repetition_penalty,
                                                        no_repeat_ngram=no_repeat_ngram_size, min_new_tokens=min_new_tokens,
                                                        eos=eos_token_id), _stream())
    return logits


def dec_finish(tokens: Tensor, tok_cur: Tensor, finished: Tensor, pos: Tensor, P: int, *, eos_token_id: int, pad_token_id: int = 0,
               logprobs: Tensor | None = None) -> Tensor:
    """pm_dec_finish as a standalone op (the generator puts it behind its token tail): pos is the position the tail advanced TO.
    Updates tokens (B, Ttot) int64, tok_cur (B,) int64, logprobs (f32, contiguous, shaped like tokens; optional) and finished (B,)
    int32 (0 = still running, else the position of the row's eos) IN PLACE; returns finished.  Nothing happens while pos < P."""
    _need(_is_int(eos_token_id) and eos_token_id >= 0 and _is_int(pad_token_id) and pad_token_id >= 0,
          "dec_finish: eos_token_id and pad_token_id must be integers >= 0")
    _cuda(tokens, tok_cur, finished, pos, logprobs)
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64 and tokens.is_contiguous() and 1 <= P <= tokens.shape[1],
          "dec_finish: contiguous int64 tokens (B, Ttot >= P >= 1)")
    B = tokens.shape[0]
    _need(tok_cur.dtype == torch.int64 and tok_cur.shape == (B,) and tok_cur.is_contiguous(), "dec_finish: contiguous int64 tok_cur (B,)")
    _need(finished.dtype == torch.int32 and finished.shape == (B,) and finished.is_contiguous(), "dec_finish: contiguous int32 finished (B,)")
    _need(logprobs is None or (logprobs.dtype == torch.float32 and logprobs.shape == tokens.shape and logprobs.is_contiguous()),
          "dec_finish: logprobs f32, contiguous, shaped like tokens")
    _pos_inside("dec_finish", pos, tokens.shape[1])
    plan.call(lib().pm_dec_finish, plan.finish_args(tokens, tok_cur, logprobs, finished, pos, P, eos_token_id, pad_token_id), _stream())
    return finished
