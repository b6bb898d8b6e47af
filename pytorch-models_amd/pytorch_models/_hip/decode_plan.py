"""The launch plan of a decode step: the one place that knows (1) the positional C signatures of the long step kernels
(csrc/decode.hip), (2) the K-split workspace layout and (3) the capture / replay protocol of a step.

A decode step is nothing but its launch list: ``launches`` holds (fn, args) pairs of raw pointers and integers whose last
argument (the stream) is replaced at call time, so the loop has no per-step Python work beyond ctypes and the list can be
captured ONCE into a HIP graph and replayed.  The raw pointers are the price: every tensor a launch points into must stay
alive as long as the plan - as an attribute of the decoder or in ``_keep`` (tools/decode_plan.py resolves every pointer of a
plan into such a tensor; tests/test_hip_decode_plan.py asserts it for every decoder form).

GreedyDecoder / BeamDecoder (audio2text/generate.py) and T5DecodeState (text/t5_generate.py) build their lists here; the
standalone wrappers in ops.py use the same argument builders.
"""
from __future__ import annotations

from collections import namedtuple

import torch
from torch import Tensor

from . import check, lib


def ptr(t: Tensor | None):
    return None if t is None else t.data_ptr()


def _ld(t: Tensor | None) -> int:
    return 0 if t is None else t.stride(0)


# ---- argument builders: tensors and named options in, the positional tuple of the C entry point out (stream slot = None) ----
def _unit_rows(what: str, *ts: Tensor | None) -> None:
    """The builders pass a row stride and a pointer per matrix: the columns must be one element apart.  Checked where a plan is
    BUILT (attribute reads); a built plan holds integers and is not looked at again."""
    for t in ts:
        if t is not None and t.dim() >= 1 and t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError(f"{what}: operand rows must have unit column stride, got strides {tuple(t.stride())}")


def linear_args(x: Tensor, w: Tensor, out: Tensor | None, rows: int, *, ln=None, bias=None, resid=None, act: int = 0, mode: int = 0,
                cache=(None, None), geom=(0, 0, 0), pos=None, argmax_ws=(None, None)) -> tuple:
    """pm_dec_linear: act(LN?(x) w^T + bias) + resid.  mode 0 stores to ``out``; mode 1 ([q|k|v]) stores q to ``out`` and k, v into
    ``cache`` = (kc, vc) at *pos, addressed by ``geom`` = (inner, heads, t_max); mode 2 stores nothing but the per-tile
    (max, index) pairs to ``argmax_ws`` = (ws_val, ws_idx).  ``ln`` = (gamma, beta, eps) or None."""
    N, K = w.shape
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    _unit_rows("linear_args", x, w, resid, out, g, b, bias)
    return (x.data_ptr(), x.stride(0), ptr(g), ptr(b), float(eps), w.data_ptr(), w.stride(0), ptr(bias), ptr(resid), _ld(resid),
            ptr(out), _ld(out), rows, N, K, act, mode, ptr(cache[0]), ptr(cache[1]), *geom, ptr(pos), ptr(argmax_ws[0]),
            ptr(argmax_ws[1]), None)


def ksplit_workspace(rows: int, N: int, k_split: int, device) -> tuple[Tensor, Tensor]:
    """(ws, tickets) of pm_dec_linear_ksplit - THE statement of the layout the kernel indexes by: one 16 x 16 float tile per (feature tile,
    K part, row tile), with the row tile count that of the kernel instantiation (1, 2 or 4), and one zeroed ticket per (feature tile,
    row tile)."""
    nt, mt = (N + 15) // 16, (rows + 15) // 16
    mt = 1 if mt <= 1 else 2 if mt == 2 else 4
    return (torch.empty(nt * k_split * mt * 256, dtype=torch.float32, device=device),
            torch.zeros(nt * 4, dtype=torch.int32, device=device))


def ksplit_args(x: Tensor, w: Tensor, out: Tensor, rows: int, k_split: int, ws: Tensor, tickets: Tensor, *, bias=None, resid=None,
                act: int = 0) -> tuple:
    """pm_dec_linear_ksplit: linear_args' mode 0 without LayerNorm, K split over ``k_split`` workgroups per feature tile"""
    N, K = w.shape
    _unit_rows("ksplit_args", x, w, resid, out, bias)
    return (x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), ptr(bias), ptr(resid), _ld(resid), out.data_ptr(), out.stride(0),
            rows, N, K, act, k_split, ws.data_ptr(), tickets.data_ptr(), None)


def kparts_args(x: Tensor, w: Tensor, parts: Tensor, rows: int, k_split: int) -> tuple:
    """pm_dec_linear_kparts: the K parts of x w^T left as parts in ``parts`` (>= k_split, rows, N) for the next chain block to add"""
    N, K = w.shape
    _unit_rows("kparts_args", x, w, parts)
    return (x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), parts.data_ptr(), parts.stride(1), parts.stride(0), rows, N, K,
            k_split, None)


# where an attention block finds its keys and values: base + b * stride_b + h * stride_h + key * stride_k (strides in elements)
KV = namedtuple("KV", "k v stride_b stride_h stride_k")


def cache_kv(kc: Tensor, vc: Tensor) -> KV:
    """self-attention caches (rows, heads, t_max, 64)"""
    _unit_rows("cache_kv", kc, vc)
    if kc.shape != vc.shape or any(a != b for n, a, b in zip(kc.shape, kc.stride(), vc.stride()) if n > 1):
        raise ValueError(f"cache_kv: k and v caches must share one layout, got strides {tuple(kc.stride())} and {tuple(vc.stride())}")
    return KV(kc.data_ptr(), vc.data_ptr(), kc.stride(0), kc.stride(1), kc.stride(2))


def packed_kv(kv: Tensor, S: int, inner: int) -> KV:
    """the projected memory, packed (rows, S, [k | v]): the V half starts ``inner`` elements into a row"""
    return KV(kv.data_ptr(), kv.data_ptr() + inner * kv.element_size(), S * 2 * inner, 64, 2 * inner)


def _block_args(x: Tensor, ln, w: Tensor, bias, kv: KV, self_attn: bool, pos: Tensor | None, n_keys: int) -> tuple:
    """the 15 leading arguments the fused and the chain block share: a self block attends *pos older keys and its own (at most
    n_keys), a cross block n_keys"""
    g, b, eps = ln
    return (x.data_ptr(), x.shape[1], g.data_ptr(), b.data_ptr(), float(eps), w.data_ptr(), ptr(bias), *kv,
            *((pos.data_ptr(), 0, n_keys) if self_attn else (None, n_keys, n_keys)))


def attention_args(q: Tensor, kv: KV, out: Tensor, rows: int, heads: int, *, pos: Tensor | None, lk_add: int, lk_max: int) -> tuple:
    """pm_dec_attention over (*pos if pos else 0) + lk_add keys"""
    return (q.data_ptr(), *kv, ptr(pos), lk_add, lk_max, out.data_ptr(), rows, heads, None)


def prefill_attention_args(qkv: Tensor, kv: KV, out: Tensor, rows: int, heads: int, chunk: int, p0: int, lk_max: int) -> tuple:
    """pm_prefill_attention_bf16: ``chunk`` positions from p0 of each of ``rows`` sequences, [q | k | v] rows in, caches appended"""
    return (qkv.data_ptr(), qkv.stride(0), kv.k, kv.v, kv.stride_b, kv.stride_h, kv.stride_k, out.data_ptr(), out.stride(0), rows,
            heads, chunk, p0, lk_max, None)


# ---- ragged prompt batches: the sequences are right-aligned in the caches and ``key_start`` (int32 (rows,), on the device) holds
# each one's first cache position; every builder is its plain namesake plus that pointer (include/pm_mi355x.h) ----
def ragged_attention_args(q: Tensor, kv: KV, out: Tensor, rows: int, heads: int, *, pos: Tensor | None, lk_add: int, lk_max: int,
                          key_start: Tensor) -> tuple:
    """pm_dec_attention_ragged: row b attends keys min(key_start[b], Lk - 1) .. Lk - 1 of its (*pos if pos else 0) + lk_add keys"""
    return (q.data_ptr(), *kv, ptr(pos), lk_add, lk_max, key_start.data_ptr(), out.data_ptr(), rows, heads, None)


def ragged_prefill_attention_args(qkv: Tensor, kv: KV, out: Tensor, rows: int, heads: int, chunk: int, p0: int, lk_max: int,
                                  key_start: Tensor) -> tuple:
    """pm_prefill_attention_ragged_bf16: prefill_attention_args with the keys below key_start[b] masked"""
    return (*prefill_attention_args(qkv, kv, out, rows, heads, chunk, p0, lk_max)[:-1], key_start.data_ptr(), None)


def ragged_embed_args(tok_cur: Tensor, emb: Tensor, pos_tab: Tensor, pos: Tensor, key_start: Tensor, x: Tensor) -> tuple:
    """pm_dec_embed_ragged: x[b] = emb[tok_cur[b]] + pos_tab[max(0, *pos - key_start[b])]"""
    V, d = emb.shape
    return (tok_cur.data_ptr(), emb.data_ptr(), pos_tab.data_ptr(), pos.data_ptr(), key_start.data_ptr(), x.data_ptr(), x.shape[0], d, V,
            None)


def ragged_next_token_args(ws_val: Tensor, ws_idx: Tensor, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor,
                           margins: Tensor | None, emb: Tensor, pos_tab: Tensor, key_start: Tensor, x: Tensor, ticket: Tensor) -> tuple:
    """pm_dec_next_token_ragged: ``prompt`` is the right-aligned (rows, P) matrix"""
    V, d = emb.shape
    return (ws_val.data_ptr(), ws_idx.data_ptr(), ws_val.shape[1], pos.data_ptr(), prompt.data_ptr(), prompt.shape[1], tok_cur.data_ptr(),
            tokens.data_ptr(), tokens.shape[1], ptr(margins), emb.data_ptr(), pos_tab.data_ptr(), key_start.data_ptr(), x.data_ptr(), d,
            V, ticket.data_ptr(), x.shape[0], None)


def ragged_sample_topk_args(logits: Tensor, k: int, seed: int, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor,
                            emb: Tensor, pos_tab: Tensor, key_start: Tensor, x: Tensor, ticket: Tensor) -> tuple:
    """pm_dec_sample_topk_ragged: the draw stays keyed by (seed, cache position, row)"""
    V, d = emb.shape
    return (logits.data_ptr(), logits.stride(0), V, k, int(seed) & (2**64 - 1), pos.data_ptr(), prompt.data_ptr(), prompt.shape[1],
            tok_cur.data_ptr(), tokens.data_ptr(), tokens.shape[1], emb.data_ptr(), pos_tab.data_ptr(), key_start.data_ptr(),
            x.data_ptr(), d, ticket.data_ptr(), x.shape[0], None)


def sample_args(logits: Tensor, topk: int, temperature: float, top_p: float, seed: int, pos: Tensor, prompt: Tensor, tok_cur: Tensor,
                tokens: Tensor, logprobs: Tensor | None, emb: Tensor, pos_tab: Tensor, x: Tensor, ticket: Tensor) -> tuple:
    """pm_dec_sample: the sampling tail (csrc/sample.hip); ``logprobs`` f32 like ``tokens``, or None"""
    V, d = emb.shape
    _unit_rows("sample_args", logits, prompt, tokens, logprobs, emb, pos_tab, x)
    return (logits.data_ptr(), logits.stride(0), V, topk, float(temperature), float(top_p), int(seed) & (2**64 - 1), pos.data_ptr(),
            prompt.data_ptr(), prompt.shape[1], tok_cur.data_ptr(), tokens.data_ptr(), tokens.shape[1], ptr(logprobs), emb.data_ptr(),
            pos_tab.data_ptr(), x.data_ptr(), d, ticket.data_ptr(), x.shape[0], None)


def ragged_sample_args(logits: Tensor, topk: int, temperature: float, top_p: float, seed: int, pos: Tensor, prompt: Tensor,
                       tok_cur: Tensor, tokens: Tensor, logprobs: Tensor | None, emb: Tensor, pos_tab: Tensor, key_start: Tensor,
                       x: Tensor, ticket: Tensor) -> tuple:
    """pm_dec_sample_ragged: sample_args plus key_start; the draw stays keyed by (seed, cache position, row)"""
    a = sample_args(logits, topk, temperature, top_p, seed, pos, prompt, tok_cur, tokens, logprobs, emb, pos_tab, x, ticket)
    return (*a[:16], key_start.data_ptr(), *a[16:])


def controls_args(logits: Tensor, tokens: Tensor, pos: Tensor, P: int, key_start: Tensor | None, *, repetition_penalty: float = 1.0,
                  no_repeat_ngram: int = 0, min_new_tokens: int = 0, eos: int | None = None) -> tuple:
    """pm_dec_controls (csrc/controls.hip): the repetition penalty, the n-gram ban and the minimum length on the fp32 logits of the
    row at *pos, in place; ``key_start`` (a ragged batch) keeps the padding out of the history, ``eos`` None = none"""
    _unit_rows("controls_args", logits, tokens)
    return (logits.data_ptr(), logits.stride(0), logits.shape[1], tokens.data_ptr(), tokens.shape[1], pos.data_ptr(), int(P),
            ptr(key_start), float(repetition_penalty), int(no_repeat_ngram), int(min_new_tokens), -1 if eos is None else int(eos),
            logits.shape[0], None)


def finish_args(tokens: Tensor, tok_cur: Tensor, logprobs: Tensor | None, finished: Tensor, pos: Tensor, P: int, eos: int,
                pad: int) -> tuple:
    """pm_dec_finish (csrc/controls.hip), behind the token tail: ``finished`` int32 (rows,), 0 = still running; ``logprobs`` f32 like
    ``tokens``, or None"""
    _unit_rows("finish_args", tokens, logprobs)
    return (tokens.data_ptr(), tokens.shape[1], tok_cur.data_ptr(), ptr(logprobs), finished.data_ptr(), pos.data_ptr(), int(P),
            int(eos), int(pad), tokens.shape[0], None)


def fused_args(x: Tensor, ln, w: Tensor, bias, kv: KV, out: Tensor, rows: int, heads: int, *, self_attn: bool, pos=None,
               n_keys: int) -> tuple:
    """pm_dec_attention_fused / _fused_kv32 / _fused_v2: LayerNorm + projection (+ cache append) + attention, self or cross"""
    return (*_block_args(x, ln, w, bias, kv, self_attn, pos, n_keys), out.data_ptr(), rows, heads, int(self_attn), None)


# deferred sums a chain block adds to its input row: ``n`` parts in the tensor ``buf``, part p of row b at p * stride + b * row_stride,
# and the bias (a tensor or None) that goes with them
Parts = namedtuple("Parts", "n buf stride row_stride bias")


def chain_args(x: Tensor, ln, w: Tensor, bias, kv: KV, rows: int, heads: int, *, self_attn: bool, pos=None, n_keys: int, kv_f32: bool,
               parts: Parts | None = None, x_out=None, w_out=None, head_parts=None, out=None) -> tuple:
    """pm_dec_attention_chain: fused_args' block as a link of the chain of deferred sums - IN: ``parts`` are added to x and the
    sum goes to ``x_out``; OUT: with ``w_out`` the per-head partial sums of the output projection go to ``head_parts``, else the
    attention output to ``out``"""
    p = (parts.buf.data_ptr(), parts.n, parts.stride, parts.row_stride, ptr(parts.bias)) if parts is not None else (None, 0, 0, 0, None)
    return (*_block_args(x, ln, w, bias, kv, self_attn, pos, n_keys), rows, heads, int(self_attn), int(kv_f32), *p, ptr(x_out),
            ptr(w_out), ptr(head_parts), ptr(out), None)


def call(fn, args: tuple, stream=None, what: str | None = None) -> None:
    """one launch of a plan entry outside a step, on ``stream`` (default: the current one)"""
    check(fn(*args[:-1], torch.cuda.current_stream().cuda_stream if stream is None else stream), what or fn.__name__)


class CapturedStep:
    """A decode step as a launch list: built once by a subclass, run eagerly or captured once and replayed.

    ``launches``: the (fn, args) pairs of one step; ``_keep``: every tensor they point into that is not an attribute of the
    subclass; ``_ks_cnts``: the K-split tickets (zeroed by start()); ``_graph``: the captured step.  The subclass sets
    ``_embed0`` (the launch that writes position 0's row) and ``_lin`` (linear_args' per-decoder keywords) and owns reset()
    (which ends in start()) and the run loop (which starts with begin())."""

    def __init__(self, rows: int, device, k_split: int, ksplit_min_k: int) -> None:
        from . import ops  # (ops imports this module)

        ops.no_capture(type(self).__name__, "builds caches, uploads its tables and captures a graph of its own")
        self.launches, self._keep, self._ks_cnts, self._graph = [], [], [], None
        self._n_rows, self._device, self._k_split, self._ksplit_min_k = rows, device, k_split, ksplit_min_k
        self._model, self._model_sig = None, None

    def watch(self, model) -> None:
        """Record the signature of every parameter and buffer of ``model`` (transformer.state_signature): the plan points into
        them and into values derived from them, and cannot be rebuilt in place."""
        from ..transformer import state_signature

        self._model, self._model_sig = model, state_signature(model)

    def check_model(self) -> None:
        """RuntimeError when a parameter or buffer of the watched model changed since the plan was built: its launches would read
        the new values of the tensors they use directly and the old values of everything derived - a mixture of two checkpoints."""
        if self._model is None:
            return
        from ..transformer import state_signature

        if state_signature(self._model) != self._model_sig:
            raise RuntimeError(f"{type(self).__name__}: the model's parameters changed since this decoder was built (in-place update, "
                               "load_state_dict or .to()); its launch plan holds raw pointers into the old derived weights and "
                               "cannot be rebuilt in place - build a new decoder")

    def add(self, fn, *args) -> None:
        self.launches.append((fn, args))

    def keep(self, *tensors) -> None:
        self._keep += [t for t in tensors if t is not None]

    def ksplit(self, K: int) -> int:
        """plain projections with a long K (fc2: K = 4 d) are split over workgroups along K (pm_dec_linear_ksplit): into how many
        parts, 0 = not split"""
        return max(2, min(self._k_split, 8, K // 32)) if K >= self._ksplit_min_k and self._k_split > 1 else 0

    def linear(self, x: Tensor, w: Tensor, out: Tensor | None, *, ln=None, bias=None, resid=None, act: int = 0, mode: int = 0,
               cache=(None, None)) -> None:
        """add a projection: pm_dec_linear, or pm_dec_linear_ksplit when it is plain and its K is long"""
        N, K = w.shape
        g, b = ln[:2] if ln is not None else (None, None)
        self.keep(w, bias, g, b)
        ksp = self.ksplit(K)
        if mode == 0 and g is None and N <= 4096 and ksp:
            ws, tickets = ksplit_workspace(self._n_rows, N, ksp, self._device)
            self.keep(ws)
            self._ks_cnts.append(tickets)
            self.add(lib().pm_dec_linear_ksplit, *ksplit_args(x, w, out, self._n_rows, ksp, ws, tickets, bias=bias, resid=resid, act=act))
        else:
            self.add(lib().pm_dec_linear, *linear_args(x, w, out, self._n_rows, ln=ln, bias=bias, resid=resid, act=act, mode=mode,
                                                       cache=cache, **self._lin))

    def step(self, log: dict | None = None) -> None:
        st = torch.cuda.current_stream().cuda_stream
        for fn, args in self.launches:
            if log is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = fn(*args[:-1], st)
            if log is not None:
                e1.record()
                log.setdefault(fn.__name__, []).append((e0, e1, args))
            if rc:
                check(rc, fn.__name__)

    def start(self) -> None:
        """the end of a reset(): tickets to zero, position 0's row into x"""
        for cnt in self._ks_cnts:  # the K-split tickets return to zero by themselves; this covers an aborted run
            cnt.zero_()
        call(*self._embed0)

    def begin(self, graph: bool):
        """the head of a run: warm up once eagerly, synchronise and capture once (``graph``), reset; returns the call that runs a step"""
        self.check_model()
        if graph and self._graph is None:
            self.reset()
            self.step()  # eager warm-up: loads every kernel before the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.step()
            self._graph = g
        self.reset()
        return self._graph.replay if graph else self.step
