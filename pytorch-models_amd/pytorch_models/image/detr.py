"""DETR (https://arxiv.org/abs/2005.12872) on the MI355X kernels: drop-in for the reference's pytorch_models/image/detr.py (same
module-level names, constructor arguments, `nn.Sequential` indices, parameter and buffer names, `from_facebook` table and
`load_facebook_state_dict` key map), so a reference state_dict loads unchanged.

Execution on HIP tensors (eval forward, bf16 parameters; no autograd), images (N, 3, H, W) of any size:

* activations are bf16 NHWC rows from the stem to the encoder; every eval BatchNorm folds into its convolution's weight and a
  bias (derived tensors, rebuilt when a parameter changes);
* stem: `pm_resnet_stem` (Conv 7 x 7 / 2 + BN + ReLU on the fp32 VALU, then the 3 x 3 / 2 max pool);
* Bottleneck: 1 x 1 + ReLU = `pm_linear_bf16` with the ReLU epilogue; 3 x 3 (stride 1 / 2) + ReLU = `pm_conv_bf16`, the
  implicit-GEMM MFMA convolution; the shortcut's 1 x 1 (stride 1 / 2) = `pm_conv_bf16`; the last 1 x 1 = `pm_conv_bf16` with
  the shortcut as its residual and the ReLU AFTER the add;
* `input_proj` is one GEMM over the pixel rows;
* the position embeddings never meet the activations: q_proj(x + pos) = q_proj(x) + W_q pos, so every layer runs ONE packed
  projection GEMM whose periodic residual is the cached f32 table [W_q pos + b_q | W_k pos + b_k | b_v] (period H*W; for the
  decoder's self-attention the table of `query_embed`, period n_queries; for the cross-attention a Q table on the queries and a
  [K | V] table on the memory).  The sinusoid is built once per (h, w) on the host;
* attention (head dim 32) is `pm_attention_hd32_bf16`, reading the packed projections in place; out_proj and linear2 add the
  residual in their epilogues; the post-norm LayerNorms are `pm_layernorm`;
* `logits` and `boxes` come out in f32 (the box head's final sigmoid over (N, n_queries, 4) is a torch elementwise op).

fp32 parameters on a HIP device are refused (`require_bf16_params`), and so is training mode.  On the CPU (module AND input
there) the modules run the reference's arithmetic in plain torch.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import MHA, DecoderLayer, EncoderLayer, LayerNorm, _f32, _sig, _wb, derived, require_bf16_params
from .vit import _no_download


def _bn_fold(bn: nn.BatchNorm2d) -> tuple[Tensor, Tensor]:
    """Eval BatchNorm as f32 (scale, shift)."""

    def build():
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        return s.contiguous(), (bn.bias.detach().float() - bn.running_mean.detach().float() * s).contiguous()

    return derived(bn, "bn_fold", (bn.weight, bn.bias, bn.running_mean, bn.running_var), build)


def _conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> tuple[Tensor, Tensor]:
    """conv (bias=False) + eval BatchNorm -> (bf16 weight (Cout, kh, kw, Cin) with the scale folded in, f32 bias (Cout))."""
    sc, sh = _bn_fold(bn)
    return derived(conv, "conv_bn", (conv.weight, sc, sh),
                   lambda: ((conv.weight.detach().float() * sc[:, None, None, None]).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous(), sh))


class Bottleneck(nn.Module):
    def __init__(self, in_dim: int, out_dim: int, stride: int = 1) -> None:
        super().__init__()
        mid = out_dim // 4
        self.residual = nn.Sequential(
            nn.Conv2d(in_dim, mid, 1, bias=False),
            nn.BatchNorm2d(mid),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, 3, stride, 1, bias=False),
            nn.BatchNorm2d(mid),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid, out_dim, 1, bias=False),
            nn.BatchNorm2d(out_dim),
        )
        if stride > 1 or out_dim != in_dim:
            self.shortcut = nn.Sequential(nn.Conv2d(in_dim, out_dim, 1, stride, bias=False), nn.BatchNorm2d(out_dim))
        else:
            self.shortcut = nn.Identity()
        self.act = nn.ReLU(inplace=True)

    def forward(self, x: Tensor) -> Tensor:
        """(N, C, H, W) in and out, as the reference's block."""
        p = self.residual[0].weight
        if _cpu.on_cpu(x, p):
            return self.act(self.shortcut(x) + self.residual(x))
        ops.check_devices(x, p)
        require_bf16_params(self, "Bottleneck")
        if x.dim() != 4:
            raise ValueError(f"Bottleneck: expected (N, C, H, W), got {tuple(x.shape)}")
        y = self.run(x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous())
        return y.permute(0, 3, 1, 2).to(x.dtype)

    def run(self, h: Tensor) -> Tensor:
        """h: bf16 NHWC (N, H, W, Cin) -> bf16 NHWC (N, Ho, Wo, Cout)."""
        if self.training:
            raise NotImplementedError("Bottleneck: BatchNorm in training mode is not covered by the HIP kernels; call model.eval()")
        r = self.residual
        N, H, W, Cin = h.shape
        w1, b1 = _conv_bn(r[0], r[1])
        w2, b2 = _conv_bn(r[3], r[4])
        w3, b3 = _conv_bn(r[6], r[7])
        stride = r[3].stride[0]
        u = ops.linear(h.view(N * H * W, Cin), w1.view(w1.shape[0], Cin), b1, act="relu").view(N, H, W, w1.shape[0])
        t = ops.conv_bf16(u, w2, b2, stride, relu=True)
        sc = h
        if not isinstance(self.shortcut, nn.Identity):
            ws, bs = _conv_bn(self.shortcut[0], self.shortcut[1])
            sc = ops.conv_bf16(h, ws, bs, self.shortcut[0].stride[0])
        return ops.conv_bf16(t, w3, b3, 1, relu=True, resid=sc)


class ResNet(nn.Module):
    def __init__(self, n_layers: list[int]) -> None:
        super().__init__()
        in_dim = 64
        self.stem = nn.Sequential(
            nn.Conv2d(3, in_dim, 7, 2, 3, bias=False),
            nn.BatchNorm2d(64),
            nn.ReLU(inplace=True),
            nn.MaxPool2d(3, 2, 1),
        )
        self.stages = nn.Sequential()
        for i, n_layer in enumerate(n_layers):
            out_dim = 256 << i
            blocks = [Bottleneck(in_dim, out_dim, stride=1 if i == 0 else 2)]
            blocks += [Bottleneck(out_dim, out_dim) for _ in range(n_layer - 1)]
            self.stages.append(nn.Sequential(*blocks))
            in_dim = out_dim
        self.out_dim = in_dim

    def _stem_ops(self) -> tuple[Tensor, Tensor]:
        """Derived: the stem weight as f32 (147, 64) with the BatchNorm scale folded, and the shift."""
        conv, bn = self.stem[0], self.stem[1]
        sc, sh = _bn_fold(bn)
        return derived(self.stem, "stem", (conv.weight, sc, sh),
                       lambda: ((conv.weight.detach().float() * sc[:, None, None, None]).reshape(64, 147).t().contiguous(), sh))

    def forward_stages(self, imgs: Tensor) -> list[Tensor]:
        """HIP path: [stem output, stage outputs...] as bf16 NHWC (N, h, w, C) tensors."""
        p = self.stem[0].weight
        ops.check_devices(imgs, p)
        require_bf16_params(self, "ResNet")
        if self.training:
            raise NotImplementedError("ResNet: BatchNorm in training mode is not covered by the HIP kernels; call model.eval()")
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"ResNet: expected (N, 3, H, W), got {tuple(imgs.shape)}")
        wt, sh = self._stem_ops()
        h = ops.resnet_stem(imgs.float().contiguous(), wt, sh)
        outs = [h]
        for stage in self.stages:
            for blk in stage:
                h = blk.run(h)
            outs.append(h)
        return outs

    def forward(self, x: Tensor) -> Tensor:
        if _cpu.on_cpu(x, self.stem[0].weight):
            return self.stages(self.stem(x))
        return self.forward_stages(x)[-1].permute(0, 3, 1, 2)  # bf16, (N, C, h, w) as a view of the NHWC rows


# ------------------------------------------------------------------------------------------------ transformer layers
def _embed_table(mha: MHA, names: str, emb: Tensor, n_emb: int) -> Tensor:
    """f32 (rows, len(names) * inner): the packed projection of the position rows ``emb`` plus the biases; the first ``n_emb``
    projections see the embedding (W emb + b), the others only their bias - the reference adds it to q and k, never to v.
    One table per embedding tensor is KEPT: the position rows differ with the feature map's (h, w), and a captured forward
    holds the pointer of the table it was captured with, so a call at another image size must add a table, never replace one
    (class 5).  The derived() entry is the dict of the tables of one state of the projections."""
    mods = [getattr(mha, f"{n}_proj") for n in names]

    def build():
        e = emb.detach().float()
        cols = []
        for i, m in enumerate(mods):
            b = m.bias.detach().float() if m.bias is not None else e.new_zeros(m.out_features)
            cols.append(e @ m.weight.detach().float().t() + b if i < n_emb else b.expand(e.shape[0], -1))
        return torch.cat(cols, 1).contiguous()

    tables = derived(mha, f"embed_{names}_{n_emb}", [m.weight for m in mods] + [m.bias for m in mods], dict)
    sig = _sig((emb,))
    hit = tables.get(id(emb))
    if hit is None or hit[0] is not emb or hit[1] != sig:  # (the kept tensor cannot lend its id to another)
        with torch.no_grad():
            hit = tables[id(emb)] = (emb, sig, build())
        if not ops.capturing():
            torch.cuda.current_stream().synchronize()  # as derived(): built on this stream, used from any
    return hit[2]


def _attn_out(mha: MHA, o: Tensor, resid: Tensor) -> Tensor:
    op = mha.out_proj
    return ops.linear(o.view(-1, o.shape[-1]), _wb(op, "w", op.weight), _f32(op, "b", op.bias), resid=resid)


def _norm(n: LayerNorm, x: Tensor) -> Tensor:
    return ops.layernorm(x, _f32(n, "g", n.weight), _f32(n, "b", n.bias), n.eps, torch.bfloat16)


def _mlp_norm(layer: DecoderLayer, x: Tensor) -> Tensor:
    l1, l2 = layer.mlp.linear1, layer.mlp.linear2
    u = ops.linear(x, _wb(l1, "w", l1.weight), _f32(l1, "b", l1.bias), act=layer.mlp.act_name)
    return _norm(layer.mlp_norm, ops.linear(u, _wb(l2, "w", l2.weight), _f32(l2, "b", l2.bias), resid=x))


def _check_layer(layer: DecoderLayer, who: str) -> None:
    require_bf16_params(layer, who)
    if layer.training:
        raise NotImplementedError(f"{who}: inference only on the HIP kernels; call model.eval()")
    if layer.sa.head_dim != 32:
        raise NotImplementedError(f"{who}: head dim {layer.sa.head_dim} is not covered (pm_attention_hd32_bf16 serves 32)")


class DETRDecoderLayer(DecoderLayer):
    def __init__(self, d_model: int) -> None:
        super().__init__(d_model, n_heads=8, cross_attn=True, act="relu", mlp_ratio=8, pre_norm=False)

    def forward(self, x: Tensor, memory: Tensor, query_embed: Tensor, pos_embed: Tensor) -> Tensor:
        if _cpu.on_cpu(x, self.sa.q_proj.weight):
            qk = x + query_embed
            x = self.sa_norm(x + self.sa(qk, qk, x))
            x = self.ca_norm(x + self.ca(x + query_embed, memory + pos_embed, memory))
            return self.mlp_norm(x + self.mlp(x))
        ops.check_devices(x, memory, query_embed, pos_embed, self.sa.q_proj.weight)
        if memory.dim() != 3 or query_embed.dim() != 2 or pos_embed.dim() != 2 or pos_embed.shape[0] != memory.shape[1]:
            raise ValueError("DETRDecoderLayer: memory (N, HW, d), query_embed (Q, d), pos_embed (HW, d) expected")
        N, d = memory.shape[0], memory.shape[2]
        xb = x.to(torch.bfloat16).expand(N, query_embed.shape[0], d).contiguous().view(-1, d)
        y = self.run(xb, memory.to(torch.bfloat16).contiguous().view(-1, d), N, query_embed, pos_embed)
        return y.view(N, -1, d).to(x.dtype)

    def run(self, x: Tensor, mem: Tensor, N: int, query_embed: Tensor, pos_embed: Tensor) -> Tensor:
        """x: bf16 rows (N*Q, d), mem: bf16 rows (N*HW, d) -> bf16 rows (N*Q, d)."""
        _check_layer(self, "DETRDecoderLayer")
        sa, ca = self.sa, self.ca
        H, d = sa.n_heads, sa.n_heads * 32
        Q, HW = query_embed.shape[0], pos_embed.shape[0]
        w, _ = sa._pack("qkv")
        qkv = ops.linear(x, w, None, resid=_embed_table(sa, "qkv", query_embed, 2), resid_period=Q).view(N, Q, 3 * d)
        o = ops.attention_hd32(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H)
        x = _norm(self.sa_norm, _attn_out(sa, o, x))
        q = ops.linear(x, _wb(ca.q_proj, "w", ca.q_proj.weight), None, resid=_embed_table(ca, "q", query_embed, 1),
                       resid_period=Q).view(N, Q, d)
        wkv, _ = ca._pack("kv")
        kv = ops.linear(mem, wkv, None, resid=_embed_table(ca, "kv", pos_embed, 1), resid_period=HW).view(N, HW, 2 * d)
        o = ops.attention_hd32(q, kv[..., :d], kv[..., d:], H)
        x = _norm(self.ca_norm, _attn_out(ca, o, x))
        return _mlp_norm(self, x)


class DETREncoderLayer(EncoderLayer):
    def __init__(self, d_model: int) -> None:
        super().__init__(d_model, n_heads=8, act="relu", mlp_ratio=8, pre_norm=False)

    def forward(self, x: Tensor, pos_embed: Tensor) -> Tensor:
        if _cpu.on_cpu(x, self.sa.q_proj.weight):
            qk = x + pos_embed
            x = self.sa_norm(x + self.sa(qk, qk, x))
            return self.mlp_norm(x + self.mlp(x))
        ops.check_devices(x, pos_embed, self.sa.q_proj.weight)
        if x.dim() < 2 or pos_embed.dim() != 2 or pos_embed.shape[0] != x.shape[-2]:
            raise ValueError(f"DETREncoderLayer: x (..., HW, d) and pos_embed (HW, d) expected, got {tuple(x.shape)}, {tuple(pos_embed.shape)}")
        d = x.shape[-1]
        xb = x.to(torch.bfloat16).contiguous().view(-1, d)
        return self.run(xb, xb.shape[0] // x.shape[-2], pos_embed).view(x.shape).to(x.dtype)

    def run(self, x: Tensor, N: int, pos_embed: Tensor) -> Tensor:
        """x: bf16 rows (N*HW, d) -> bf16 rows (N*HW, d)."""
        _check_layer(self, "DETREncoderLayer")
        sa = self.sa
        H, d, HW = sa.n_heads, sa.n_heads * 32, pos_embed.shape[0]
        w, _ = sa._pack("qkv")
        qkv = ops.linear(x, w, None, resid=_embed_table(sa, "qkv", pos_embed, 2), resid_period=HW).view(N, HW, 3 * d)
        o = ops.attention_hd32(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H)
        x = _norm(self.sa_norm, _attn_out(sa, o, x))
        return _mlp_norm(self, x)


def _axis_embed(freqs: Tensor, n: int) -> Tensor:
    """(n, 2 * len(freqs)): sin / cos interleaved of position * 2 pi / (n + 1e-6), positions 1 .. n."""
    ts = torch.arange(1, n + 1, device=freqs.device, dtype=freqs.dtype) / (n + 1e-6) * 2 * torch.pi
    ang = ts.view(-1, 1) * freqs
    return torch.stack([ang.sin(), ang.cos()], dim=2).flatten(1)


def _sinusoid_2d(freqs: Tensor, h: int, w: int) -> Tensor:
    ye = _axis_embed(freqs, h).view(h, 1, -1).expand(h, w, -1)
    xe = _axis_embed(freqs, w).view(1, w, -1).expand(h, w, -1)
    return torch.cat([ye, xe], dim=2)


class SinusoidalPositionEmbedding2d(nn.Module):
    """(h, w) -> (h, w, d_model): the first half of the channels encodes the row, the second the column."""

    def __init__(self, d_model: int) -> None:
        super().__init__()
        half = d_model // 2
        self.register_buffer("freqs", 10_000 ** (-2 * torch.arange(half // 2) / half), persistent=False)

    def _make_embed(self, x: int) -> Tensor:
        return _axis_embed(self.freqs, x)

    def forward(self, h: int, w: int) -> Tensor:
        return _sinusoid_2d(self.freqs, h, w)

    def table(self, h: int, w: int) -> Tensor:
        """HIP path: the (h*w, d_model) f32 table, built once per (h, w) on the host (f32 frequencies, recomputed there: the
        buffer is bf16 after model.to(bfloat16)) and kept on the buffer's device."""
        cache = self.__dict__.setdefault("_pm_tables", {})
        key = (h, w, str(self.freqs.device))
        if key not in cache:
            half = self.freqs.numel() * 2
            freqs = 10_000 ** (-2 * torch.arange(half // 2) / half)
            cache[key] = _sinusoid_2d(freqs, h, w).flatten(0, 1).contiguous().to(self.freqs.device)
        return cache[key]


class DETR(nn.Module):
    def __init__(self, backbone_layers: list[int], d_model: int = 256, n_classes: int = 91, n_queries: int = 100) -> None:
        super().__init__()
        self.backbone = ResNet(backbone_layers)
        self.input_proj = nn.Conv2d(self.backbone.out_dim, d_model, 1)
        self.pos_embed = SinusoidalPositionEmbedding2d(d_model)
        self.query_embed = nn.Parameter(torch.zeros(n_queries, d_model))
        self.encoder = nn.ModuleList([DETREncoderLayer(d_model) for _ in range(6)])
        self.decoder = nn.ModuleList([DETRDecoderLayer(d_model) for _ in range(6)])
        self.norm = LayerNorm(d_model)
        self.classifier = nn.Linear(d_model, n_classes + 1)
        self.box_head = nn.Sequential(
            nn.Linear(d_model, d_model),
            nn.ReLU(inplace=True),
            nn.Linear(d_model, d_model),
            nn.ReLU(inplace=True),
            nn.Linear(d_model, 4),
        )

    def forward_stages(self, imgs: Tensor) -> dict[str, Tensor]:
        """HIP path: every checkpoint of the forward - "stem", "stage0" .. "stage3" (bf16 NHWC), "input_proj" (bf16 (N, HW, d)),
        "memory" (bf16 (N, HW, d)), "logits" (f32 (N, Q, classes + 1)), "boxes" (f32 (N, Q, 4))."""
        ops.check_devices(imgs, self.query_embed)
        require_bf16_params(self, "DETR")
        if self.training:
            raise NotImplementedError("DETR: inference only on the HIP kernels; call model.eval()")
        feats = self.backbone.forward_stages(imgs)
        out = {"stem": feats[0]}
        out.update({f"stage{i}": f for i, f in enumerate(feats[1:])})
        f = feats[-1]
        N, h, w, C = f.shape
        ip = self.input_proj
        wp = derived(ip, "w2d", (ip.weight,), lambda: ip.weight.detach().reshape(ip.out_channels, C).to(torch.bfloat16).contiguous())
        x = ops.linear(f.view(N * h * w, C), wp, _f32(ip, "b", ip.bias))
        d = x.shape[1]
        out["input_proj"] = x.view(N, h * w, d)
        pos = self.pos_embed.table(h, w)
        for layer in self.encoder:
            x = layer.run(x, N, pos)
        out["memory"] = x.view(N, h * w, d)
        qe = self.query_embed
        Q = qe.shape[0]
        query = torch.zeros((N * Q, d), dtype=torch.bfloat16, device=x.device)
        for layer in self.decoder:
            query = layer.run(query, x, N, qe, pos)
        query = _norm(self.norm, query)
        cl = self.classifier
        out["logits"] = ops.linear(query, _wb(cl, "w", cl.weight), _f32(cl, "b", cl.bias), out_dtype=torch.float32).view(N, Q, cl.weight.shape[0])
        b0, b1, b2 = self.box_head[0], self.box_head[2], self.box_head[4]
        u = ops.linear(query, _wb(b0, "w", b0.weight), _f32(b0, "b", b0.bias), act="relu")
        u = ops.linear(u, _wb(b1, "w", b1.weight), _f32(b1, "b", b1.bias), act="relu")
        out["boxes"] = ops.linear(u, _wb(b2, "w", b2.weight), _f32(b2, "b", b2.bias), out_dtype=torch.float32).sigmoid().view(N, Q, 4)
        return out

    def forward(self, x: Tensor) -> tuple[Tensor, Tensor]:
        if not _cpu.on_cpu(x, self.query_embed):
            out = self.forward_stages(x)
            return out["logits"], out["boxes"]
        x = self.input_proj(self.backbone(x))
        pos = self.pos_embed(x.shape[-2], x.shape[-1]).flatten(0, 1)
        x = x.flatten(-2).transpose(-1, -2)  # (N, C, h, w) -> (N, hw, C)
        for layer in self.encoder:
            x = layer(x, pos)
        query = torch.zeros_like(self.query_embed)
        for layer in self.decoder:
            query = layer(query, x, self.query_embed, pos)
        query = self.norm(query)
        return self.classifier(query), self.box_head(query).sigmoid()

    @staticmethod
    def from_facebook(model_tag: str, *, pretrained: bool = False) -> "DETR":
        """"resnet50" (detr-r50-e632da11.pth) or "resnet101" (detr-r101-2c7b67e5.pth) of facebookresearch/detr."""
        backbone_layers = dict(resnet50=[3, 4, 6, 3], resnet101=[3, 4, 23, 3])[model_tag]
        if pretrained:
            _no_download("DETR.from_facebook")
        return DETR(backbone_layers)

    @torch.no_grad()
    def load_facebook_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        """facebookresearch/detr checkpoint (its "model" dict) -> this module, the reference's key map."""
        sd = dict(state_dict)

        def take(m: nn.Module, prefix: str) -> None:
            m.weight.copy_(sd.pop(f"{prefix}.weight"))
            if getattr(m, "bias", None) is not None:
                m.bias.copy_(sd.pop(f"{prefix}.bias"))
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(sd.pop(f"{prefix}.running_mean"))
                m.running_var.copy_(sd.pop(f"{prefix}.running_var"))

        def take_mha(m: MHA, prefix: str) -> None:
            ws = sd.pop(f"{prefix}.in_proj_weight").chunk(3, dim=0)
            bs = sd.pop(f"{prefix}.in_proj_bias").chunk(3, dim=0)
            for name, w, b in zip("qkv", ws, bs):
                proj = getattr(m, f"{name}_proj")
                proj.weight.copy_(w)
                proj.bias.copy_(b)
            take(m.out_proj, f"{prefix}.out_proj")

        body = "backbone.0.body"
        take(self.backbone.stem[0], f"{body}.conv1")
        take(self.backbone.stem[1], f"{body}.bn1")
        for si, stage in enumerate(self.backbone.stages):
            for bi, blk in enumerate(stage):
                pre = f"{body}.layer{si + 1}.{bi}"
                for k, idx in enumerate((0, 3, 6)):
                    take(blk.residual[idx], f"{pre}.conv{k + 1}")
                    take(blk.residual[idx + 1], f"{pre}.bn{k + 1}")
                if bi == 0:
                    take(blk.shortcut[0], f"{pre}.downsample.0")
                    take(blk.shortcut[1], f"{pre}.downsample.1")
        take(self.input_proj, "input_proj")
        self.query_embed.copy_(sd.pop("query_embed.weight"))
        for kind in ("encoder", "decoder"):
            for li, layer in enumerate(getattr(self, kind)):
                pre = f"transformer.{kind}.layers.{li}"
                take_mha(layer.sa, f"{pre}.self_attn")
                take(layer.sa_norm, f"{pre}.norm1")
                if kind == "decoder":
                    take_mha(layer.ca, f"{pre}.multihead_attn")
                    take(layer.ca_norm, f"{pre}.norm2")
                take(layer.mlp.linear1, f"{pre}.linear1")
                take(layer.mlp.linear2, f"{pre}.linear2")
                take(layer.mlp_norm, f"{pre}.norm2" if kind == "encoder" else f"{pre}.norm3")  # norm2 means two things
        take(self.norm, "transformer.decoder.norm")
        take(self.classifier, "class_embed")
        for i, idx in enumerate((0, 2, 4)):
            take(self.box_head[idx], f"bbox_embed.layers.{i}")


def _load_coco_classes() -> list[str]:
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "coco_classes.json")) as f:
        return json.load(f)


class DETRPipeline(nn.Module):
    """Host-side pre / post-processing around a DETR: pad to a common size, ImageNet normalisation, softmax, threshold, boxes in
    pixels as (x1, y1, x2, y2)."""

    COCO_CLASSES = _load_coco_classes()  # the 91 COCO category slots ("N/A" where the id is unused): image/coco_classes.json

    def __init__(self, model: DETR, threshold: float = 0.7) -> None:
        super().__init__()
        self.model = model.eval()
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1))
        self.th = threshold

    @staticmethod
    def cxcywh_to_xyxy(boxes: Tensor) -> Tensor:
        cx, cy, w, h = boxes.unbind(-1)
        return torch.stack([cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5], dim=-1)

    @torch.no_grad()
    def forward(self, images: list[Tensor], th: float | None = None):
        ops.no_capture("DETRPipeline", "builds Python lists from the detections on the host")
        height = max(img.shape[-2] for img in images)
        width = max(img.shape[-1] for img in images)
        batch = torch.stack([F.pad(img, (0, width - img.shape[-1], 0, height - img.shape[-2])) for img in images], dim=0)
        logits, boxes = self.model((batch - self.mean) / self.std)
        logits, boxes = logits.float(), boxes.float()
        probs = logits.softmax(-1)[..., :-1]  # the last class is "no object"
        keep = probs.amax(-1) >= (th or self.th)
        boxes = self.cxcywh_to_xyxy(boxes * boxes.new_tensor([width, height, width, height]))
        results = []
        for i in range(batch.shape[0]):
            p, cls = probs[i, keep[i]].max(-1)
            results.append([[self.COCO_CLASSES[c] for c in cls.cpu()], boxes[i, keep[i]], p])
        return results
