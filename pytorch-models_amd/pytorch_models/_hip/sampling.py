"""The sampling tail of a decode step on explicit state (csrc/sample.hip): what the generators put into their launch lists as
pm_dec_sample / pm_dec_sample_ragged, as a standalone call - and the one statement of which (topk, temperature, top_p) are
allowed, shared with GreedyDecoder.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import decode_plan as plan, lib
from .ops import _all_unaliased, _cuda, _key_start, _need, _stream, _tail_pos, _tail_state


def check_sampling(what: str, topk: int, temperature: float, top_p: float) -> None:
    """ValueError unless topk is an integer in 0..64 (0 = the whole vocabulary), temperature a finite number >= 0 (0 = arg-max)
    and top_p in (0, 1]; nothing touches a device"""
    if isinstance(topk, bool) or not isinstance(topk, int) or not 0 <= topk <= 64:
        raise ValueError(f"{what}: topk must be an integer in 0..64 (0 = the whole vocabulary), got {topk!r}")
    try:
        t, p = float(temperature), float(top_p)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: temperature and top_p must be numbers, got {temperature!r} and {top_p!r}") from None
    if math.isnan(t) or math.isinf(t) or t < 0.0:
        raise ValueError(f"{what}: temperature must be finite and >= 0 (0 = arg-max), got {temperature!r}")
    if not 0.0 < p <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"{what}: top_p must lie in (0, 1], got {top_p!r}")
    if t > torch.finfo(torch.float32).max or (t > 0.0 and float(torch.tensor(t, dtype=torch.float32)) == 0.0):
        raise ValueError(f"{what}: temperature {temperature!r} is not a positive fp32 number (0 = arg-max)")
    if float(torch.tensor(p, dtype=torch.float32)) == 0.0:
        raise ValueError(f"{what}: top_p {top_p!r} rounds to 0 in fp32")


def wants_sampling_tail(topk: int, temperature: float, top_p: float, return_logprobs: bool) -> bool:
    """the new tail is taken only when one of these holds; otherwise a decoder builds the launch list it always built"""
    return temperature != 1.0 or top_p != 1.0 or topk == 0 or bool(return_logprobs)


def dec_sample(logits: Tensor, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor, emb: Tensor, pos_tab: Tensor, ticket: Tensor,
               *, topk: int = 0, temperature: float = 1.0, top_p: float = 1.0, seed: int = 0, logprobs: Tensor | None = None,
               key_start: Tensor | None = None) -> Tensor:
    """pm_dec_sample (key_start None) or pm_dec_sample_ragged on explicit state, as ops.dec_sample_topk: logits (B, V) f32 with unit
    column stride (any row stride), after the rules.  Picks the token after position *pos, updates tok_cur, tokens, logprobs
    (f32, contiguous, shaped like tokens; column pos + 1 receives the log-probability), pos and ticket IN PLACE and returns the
    next step's rows x (B, d) f32."""
    check_sampling("dec_sample", topk, temperature, top_p)
    _cuda(logits, pos, prompt, tok_cur, tokens, emb, pos_tab, ticket, logprobs, key_start)
    _tail_state("dec_sample", pos, prompt, tok_cur, tokens, emb, pos_tab, ticket)
    B = prompt.shape[0]
    V, d = emb.shape
    _need(logits.dtype == torch.float32 and logits.shape == (B, V) and (V == 1 or logits.stride(1) == 1)
          and (B == 1 or logits.stride(0) >= V), "dec_sample: logits f32 (B, V) with unit column stride and rows that do not overlap")
    _need(d % 8 == 0, "dec_sample: d_model must be a multiple of 8")
    _need(logprobs is None or (logprobs.dtype == torch.float32 and logprobs.shape == tokens.shape and logprobs.is_contiguous()),
          "dec_sample: logprobs f32, contiguous, shaped like tokens")
    _all_unaliased("dec_sample", ("pos", "tok_cur", "tokens", "ticket", "logprobs"), (pos, tok_cur, tokens, ticket, logprobs),
                   ("logits", "prompt", "emb", "pos_tab", "key_start"), (logits, prompt, emb, pos_tab, key_start))
    _tail_pos("dec_sample", pos, pos_tab)
    x = torch.empty(B, d, dtype=torch.float32, device=emb.device)
    if key_start is None:
        plan.call(lib().pm_dec_sample, plan.sample_args(logits, topk, temperature, top_p, seed, pos, prompt, tok_cur, tokens, logprobs, emb,
                                                        pos_tab, x, ticket), _stream())
    else:
        _key_start(key_start, B, "dec_sample")
        plan.call(lib().pm_dec_sample_ragged, plan.ragged_sample_args(logits, topk, temperature, top_p, seed, pos, prompt, tok_cur, tokens,
                                                                      logprobs, emb, pos_tab, key_start, x, ticket), _stream())
    return x
