"""Batched greedy generation with a KV cache for T5Model on MI355X (T5Model.generate).

Semantics = the reference's T5Generator.generate loop (text/t5.py:213-227, restated by oracle/ref_t5.greedy) per row: start
from the pad id, take the arg-max of the last position (lowest index on ties), append it, stop at eos.  Here for a padded
batch: the encoder runs once with a per-row key mask, the cross-attention K/V are projected once, the self-attention K/V are
cached, and one step is a list of launches (csrc/decode_t5.hip for the stages whose form is T5's own, csrc/decode.hip's
geometry-agnostic pm_dec_linear / pm_dec_linear_ksplit for the bias-free output projections and the classifier) whose
position and tokens live on the device: the step is captured ONCE into a HIP graph and replayed.

The relative-position bias of the one-sided (decoder) case depends only on the distance t - j >= 0, so the step reads a
(heads, Tmax) fp32 table by distance (``distance_lut``); no (heads, L, L) tensor exists on the step path.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .._hip import PM_F32, decode_plan as plan, lib, ops
from ..transformer import _f32, _wb, derived, require_bf16_params

MAX_BATCH, MAX_D, MAX_KEYS = 64, 1024, 2048
POLL_EVERY = 32  # steps between two reads of the all-rows-finished flag (the only host work in the loop besides the replay)


def distance_lut(rp, t_max: int) -> Tensor:
    """lut[h, dist] = the bias a query at position t gives the key at t - dist, fp32 (heads, t_max): the last row of the one-sided
    bucket table read backwards (the bucket depends on the distance alone), gathered from the parameter."""
    row = rp.buckets(t_max, False)[t_max - 1].flip(0)  # bucket of distance 0, 1, ..., t_max - 1
    return rp.bias.detach().float()[:, row.to(rp.bias.device)].contiguous()


def _interleaved_wv(geglu) -> Tensor:
    """(2F, d) bf16 with the gate row and the value row of feature f next to each other (rows 2f, 2f + 1): the two halves of a
    GEGLU feature meet in one wave of pm_t5_dec_geglu."""
    w, v = geglu.w.weight, geglu.v.weight
    return derived(geglu, "wv_interleaved", (w, v),
                   lambda: torch.stack([w.detach(), v.detach()], 1).reshape(2 * w.shape[0], w.shape[1]).to(torch.bfloat16).contiguous())


def encode_dense(model, input_ids: Tensor, lengths: Tensor):
    """The padded-rectangle encoder of a lengths batch: (memory (B, S, d) bf16, bytes of its bias table).  The additive bias of
    every encoder layer is per row - the relative bias plus -inf on the key columns >= lengths[b] - built once per call, fp32
    (B, H, S, S); rows of padded queries hold finite garbage that nothing reads (the cross attention stops at lengths[b])."""
    enc = model.encoder
    x = model._embed(input_ids)
    S = input_ids.shape[1]
    rel = enc.attn_bias(S, bidirection=True).float()  # (H, S, S)
    dead = torch.arange(S, device=x.device)[None, :] >= lengths[:, None]  # (B, S)
    bias = rel[None] + torch.zeros(dead.shape, dtype=torch.float32, device=x.device).masked_fill_(dead, float("-inf"))[:, None, None, :]
    for layer in enc.layers:
        x = layer(x, attn_bias=bias)
    return enc.norm(x), bias.numel() * 4


class T5DecodeState(plan.CapturedStep):
    """State + launch list of the decode step for one (model, batch, source length, prompt length, new tokens) geometry."""

    def __init__(self, model, B: int, S: int, P: int, n_new: int, pad_id: int = 0, eos_id: int = 1, return_logits: bool = False) -> None:
        require_bf16_params(model, "T5Model.generate")
        dec = model.decoder
        E = _wb(model.token_embs, "E", model.token_embs.weight)
        Wc = _wb(model.classifier, "w", model.classifier.weight)
        V, d = E.shape
        dev = E.device
        if B > MAX_BATCH:
            raise NotImplementedError("T5 generate: at most 64 sequences per call (shard larger batches)")
        if B < 1 or S < 1 or P < 1 or n_new < 1:
            raise ValueError("T5 generate: need at least one sequence, one source token, one prompt token and one new token")
        if not 0 <= pad_id < V or eos_id >= V:
            raise ValueError(f"T5 generate: pad_id / eos_id outside the vocabulary of {V}")
        if d % 32 or d > MAX_D:
            raise NotImplementedError(f"T5 generate: d_model % 32 == 0 and <= {MAX_D} (t5 small / base / large); got {d}")
        Ttot = P + n_new
        if Ttot > MAX_KEYS or S > MAX_KEYS:
            raise NotImplementedError(f"T5 generate: at most {MAX_KEYS} source tokens and {MAX_KEYS} decoder positions "
                                      f"(got {S} and {Ttot})")
        H = dec.layers[0].sa.n_heads
        inner = H * 64
        for i, layer in enumerate(dec.layers):
            for name, att in (("sa", layer.sa), ("ca", layer.ca)):
                if att is None or att.head_dim != 64 or att.n_heads != H or att.q_proj.bias is not None:
                    raise NotImplementedError(f"T5 generate: layer {i} {name}: bias-free heads of 64 and one head count in every layer")
            F = layer.mlp[2].in_features
            if F % 32:
                raise NotImplementedError(f"T5 generate: layer {i}: MLP width {F} must be a multiple of 32")
        self.model, self.B, self.S, self.P, self.Ttot, self.n_steps = model, B, S, P, Ttot, Ttot - 1
        self.pad_id, self.eos_id, self.V, self.d, self.H = int(pad_id), int(eos_id) if eos_id >= 0 else -1, V, d, H
        L = lib()
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        Tmax = Ttot
        f_max = max(layer.mlp[2].in_features for layer in dec.layers)
        self.x = torch.empty(B, d, **f32)
        self.xn = torch.empty(B, d, **f32)
        self.q = torch.empty(B, inner, **f32)
        self.att = torch.empty(B, inner, **f32)
        self.h = torch.empty(B, f_max, **f32)
        self.pos = torch.zeros(1, **i32)
        self.ticket = torch.zeros(1, **i32)
        self.finished = torch.zeros(B, **i32)
        self.src_len = torch.full((B,), S, **i32)
        self.out_len = torch.full((B,), Ttot, dtype=torch.int64, device=dev)
        self.prompt = torch.full((B, P), self.pad_id, dtype=torch.int64, device=dev)
        self.tokens = torch.full((B, Ttot), self.pad_id, dtype=torch.int64, device=dev)
        self.lut = distance_lut(dec.attn_bias, Tmax)  # (H, Tmax) fp32, built once
        n_tiles = (V + 63) // 64  # pm_dec_linear mode 2 without its own norm: one (max, index) per 64 features and sequence
        self.ws_val = torch.empty(B, n_tiles, **f32)
        self.ws_idx = torch.empty(B, n_tiles, **i32)
        self.logits_step = torch.empty(B, V, **f32) if return_logits else None
        self.logits = torch.zeros(B, Ttot - 1, V, **f32) if return_logits else None
        # bias-free x w^T (+ resid) through pm_dec_linear (mode 2: arg-max tiles), split along a long K as GreedyDecoder does
        super().__init__(B, dev, k_split=4, ksplit_min_k=1024)
        self.keep(E, Wc)
        self._lin = dict(geom=(inner, H, Tmax), pos=self.pos, argmax_ws=(self.ws_val, self.ws_idx))
        # one workgroup per (sequence, head) pulls the head's q/k/v rows through its CU: that wins while every workgroup has a CU
        # to itself (B * H <= 256); beyond, the projection that reads the weights once per 8 sequences + an attention launch
        self.fuse_self = B * H <= 256
        self.self_k, self.self_v, self.cross_kv, self._cross_w = [], [], [], []
        x = self.x
        for layer in dec.layers:
            sa, ca, geglu, wo = layer.sa, layer.ca, layer.mlp[0], layer.mlp[2]
            kc = torch.empty(B, H, Tmax, 64, dtype=torch.bfloat16, device=dev)
            vc = torch.empty_like(kc)
            self.self_k.append(kc)
            self.self_v.append(vc)
            wqkv, _ = sa._pack("qkv")
            g = _f32(layer.sa_norm, "g", layer.sa_norm.weight)
            self.keep(wqkv, g)
            if self.fuse_self:
                self.add(L.pm_t5_dec_self_fused, x.data_ptr(), d, g.data_ptr(), float(layer.sa_norm.eps), wqkv.data_ptr(), kc.data_ptr(),
                         vc.data_ptr(), Tmax, self.pos.data_ptr(), self.lut.data_ptr(), self.att.data_ptr(), B, H, None)
            else:
                self.add(L.pm_t5_dec_rms_qkv, x.data_ptr(), d, g.data_ptr(), float(layer.sa_norm.eps), wqkv.data_ptr(), self.q.data_ptr(),
                         kc.data_ptr(), vc.data_ptr(), Tmax, self.pos.data_ptr(), B, H, None)
                self.add(L.pm_t5_dec_self_attention, self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), Tmax, self.pos.data_ptr(),
                         self.lut.data_ptr(), self.att.data_ptr(), B, H, None)
            self.linear(self.att, _wb(sa.out_proj, "w", sa.out_proj.weight), x, resid=x)
            # cross attention: K/V of the memory projected ONCE per call into packed bf16 (B, S, [k | v]) (bind())
            wkv, _ = ca._pack("kv")
            kv = torch.empty(B * S, 2 * inner, dtype=torch.bfloat16, device=dev)
            self.cross_kv.append(kv)
            self._cross_w.append(wkv)
            g = _f32(layer.ca_norm, "g", layer.ca_norm.weight)
            wq = _wb(ca.q_proj, "w", ca.q_proj.weight)
            self.keep(g, wq)
            self.add(L.pm_t5_dec_cross_fused, x.data_ptr(), d, g.data_ptr(), float(layer.ca_norm.eps), wq.data_ptr(), kv.data_ptr(), S,
                     self.src_len.data_ptr(), self.att.data_ptr(), B, H, None)
            self.linear(self.att, _wb(ca.out_proj, "w", ca.out_proj.weight), x, resid=x)
            F = wo.in_features
            g = _f32(layer.mlp_norm, "g", layer.mlp_norm.weight)
            wv = _interleaved_wv(geglu)
            self.keep(g, wv)
            self.add(L.pm_t5_dec_geglu, x.data_ptr(), d, g.data_ptr(), float(layer.mlp_norm.eps), wv.data_ptr(), self.h.data_ptr(),
                     self.h.stride(0), B, F, None)
            self.linear(self.h[:, :F], _wb(wo, "w", wo.weight), x, resid=x)
        g = _f32(dec.norm, "g", dec.norm.weight)
        self.keep(g)
        self.add(L.pm_rmsnorm, x.data_ptr(), d, PM_F32, g.data_ptr(), float(dec.norm.eps), self.xn.data_ptr(), d, PM_F32, B, d, None)
        self.linear(self.xn, Wc, None, mode=2)
        if return_logits:  # the full last-position logits as well (diagnostics / tests): the same products, stored
            self.add(L.pm_dec_linear, *plan.linear_args(self.xn, Wc, self.logits_step, B, **self._lin))
        self.add(L.pm_t5_dec_next_token, self.ws_val.data_ptr(), self.ws_idx.data_ptr(), n_tiles, self.pos.data_ptr(),
                 self.prompt.data_ptr(), P, self.tokens.data_ptr(), Ttot, self.pad_id, self.eos_id, self.finished.data_ptr(),
                 self.out_len.data_ptr(), E.data_ptr(), x.data_ptr(), d, V, self.ticket.data_ptr(), plan.ptr(self.logits_step),
                 plan.ptr(self.logits), B, None)
        self._embed0 = (L.pm_t5_dec_embed, (self.prompt.data_ptr(), P, E.data_ptr(), x.data_ptr(), B, d, V, None))
        self.encoder_bias_bytes = 0

    # ---- per call: encoder (with source padding), cross K/V, prompt
    def encode(self, input_ids: Tensor, lengths: Tensor | None, packed: bool = False) -> Tensor:
        """memory (B, S, d) bf16.  Padded sources: encode_dense, the padded rectangle under an fp32 (B, H, S, S) bias table.
        ``packed`` (with lengths): the packed encoder of T5Model.encode(x, lengths) instead - no padded row is computed, the
        bias comes from the (H, 2 * max_distance + 1) distance table inside the attention kernel, and rows past lengths[b] of
        the memory are zero."""
        m = self.model
        self.encoder_bias_bytes = 0
        if lengths is None:
            return m.encoder(m._embed(input_ids))
        if packed:
            return m.encode(input_ids, lengths)
        memory, self.encoder_bias_bytes = encode_dense(m, input_ids, lengths)
        return memory

    def bind(self, input_ids: Tensor, lengths: Tensor | None, prompt: Tensor | None, packed: bool = False) -> None:
        """New sources (and prompt), same geometry: everything is written INTO the existing buffers, so the captured graph (which
        holds raw pointers) stays valid."""
        B, S = self.B, self.S
        assert tuple(input_ids.shape) == (B, S)
        memory = self.encode(input_ids, lengths, packed)
        mem2 = memory.reshape(B * S, self.d)
        for kv, wkv in zip(self.cross_kv, self._cross_w):
            ops.linear(mem2, wkv, None, out=kv)
        if lengths is None:
            self.src_len.fill_(S)
        else:
            self.src_len.copy_(lengths)
        if prompt is None:
            self.prompt.fill_(self.pad_id)
        else:
            self.prompt.copy_(prompt)

    def reset(self) -> None:
        self.pos.zero_()
        self.ticket.zero_()
        self.finished.zero_()
        self.out_len.fill_(self.Ttot)
        self.tokens.fill_(self.pad_id)
        self.tokens[:, : self.P] = self.prompt
        if self.logits is not None:
            self.logits.zero_()
        self.start()  # x[b] = emb[prompt[b, 0]]

    def run(self, graph: bool = True) -> None:
        one_step = self.begin(graph)
        # rows that have all produced eos emit nothing but pad (already in ``tokens``): look every POLL_EVERY steps
        poll = self.eos_id >= 0 and self.logits is None
        for i in range(self.n_steps):
            one_step()
            if poll and i % POLL_EVERY == POLL_EVERY - 1 and i + 1 < self.n_steps and bool(self.finished.all()):
                break


def _signature(model) -> tuple:
    """every parameter and buffer, with the fields derived() keys on: a dtype or device change separates two states too"""
    from ..transformer import state_signature

    return state_signature(model)


@torch.no_grad()
def generate(model, input_ids: Tensor, *, lengths=None, max_new_tokens: int = 100, pad_id: int = 0, eos_id: int = 1,
             decoder_prompt: Tensor | None = None, graph: bool = True, return_logits: bool = False, packed: bool = False):
    ops.no_capture("T5Model.generate", "reads ids and lengths on the host and captures a graph of its own")
    require_bf16_params(model, "T5Model.generate")
    if not isinstance(input_ids, Tensor) or input_ids.dtype != torch.int64 or input_ids.dim() != 2:
        raise ValueError("T5Model.generate: input_ids must be int64 (B, S), right-padded")
    if not input_ids.is_cuda or (decoder_prompt is not None and not decoder_prompt.is_cuda):
        raise RuntimeError("T5Model.generate: HIP devices only - this build has no CPU path (move the inputs to the GPU)")
    B, S = input_ids.shape
    if B > MAX_BATCH:
        raise NotImplementedError("T5 generate: at most 64 sequences per call (shard larger batches)")
    dev = input_ids.device
    ops.check_devices(model.token_embs.weight, input_ids, decoder_prompt)
    V = model.token_embs.weight.shape[0]
    if B < 1 or S < 1 or int(input_ids.min()) < 0 or int(input_ids.max()) >= V:
        raise ValueError("T5Model.generate: input_ids empty or outside the vocabulary")
    len_t = None
    if lengths is not None:
        len_host = torch.as_tensor(lengths).detach().to("cpu", torch.int64).reshape(-1)
        if len_host.numel() != B or int(len_host.min()) < 0 or int(len_host.max()) > S:
            raise ValueError(f"T5Model.generate: lengths must be (B,) = ({B},) values in 0..{S}")
        len_t = len_host.to(dev, torch.int32)
    P = 1
    if decoder_prompt is not None:
        if decoder_prompt.dtype != torch.int64 or decoder_prompt.dim() != 2 or decoder_prompt.shape[0] != B or decoder_prompt.shape[1] < 1:
            raise ValueError("T5Model.generate: decoder_prompt must be int64 (B, P >= 1)")
        if int(decoder_prompt.min()) < 0 or int(decoder_prompt.max()) >= V:
            raise ValueError("T5Model.generate: decoder_prompt ids outside the vocabulary")
        P = decoder_prompt.shape[1]
    key = (B, S, P, int(max_new_tokens), int(pad_id), int(eos_id), bool(return_logits), _signature(model))
    cached = model.__dict__.get("_pm_t5_decode")  # one state (buffers + captured graph) is kept: repeated calls of one geometry
    if cached is None or cached[0] != key:
        cached = (key, T5DecodeState(model, B, S, P, int(max_new_tokens), int(pad_id), int(eos_id), bool(return_logits)))
        model.__dict__["_pm_t5_decode"] = cached
    st = cached[1]
    st.bind(input_ids, len_t, decoder_prompt, bool(packed))
    st.run(graph)
    out = (st.tokens.clone(), st.out_len.clone())
    return out + (st.logits.clone(),) if return_logits else out
