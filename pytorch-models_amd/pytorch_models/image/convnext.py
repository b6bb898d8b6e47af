"""ConvNeXt (https://arxiv.org/abs/2201.03545) on the MI355X kernels: drop-in for the reference's pytorch_models/image/convnext.py
(same classes, constructor arguments, `nn.Sequential` indices, parameter names, `from_facebook` table and
`load_facebook_state_dict` key map), so a reference state_dict loads unchanged.

Execution on HIP tensors (eval forward; no autograd), precision following the parameters (bf16: the bf16 tile GEMMs; fp32: the
f32-input MFMA GEMM), images (N, 3, H, W) with H, W multiples of 32:

* the stem, Conv2d(3, d, 4, 4) + LayerNorm, is `pm_convnext_stem` (fp32 on the VALU, NCHW images in, NHWC rows out);
* the residual stream is f32 NHWC rows (N*H*W, C) for both precisions (36 residual adds in `base`);
* a block is `pm_dwconv7_ln` (depthwise 7 x 7 + bias + LayerNorm, rows padded with zeros to a multiple of 64) -> fc1 + GELU ->
  fc2 with `gamma` folded into its weight and bias and the residual added in the GEMM's epilogue; atto's 4C = 160 hidden
  features are padded to 192 with zero weight rows and bias (GELU(0) = 0 columns, a valid K for fc2);
* a downsample, LayerNorm + Conv2d(C, 2C, 2, 2), is `pm_ln_space_to_depth` + one GEMM with K = 4C (weight permuted to
  (Cout, kh, kw, Cin), zero-padded along K);
* the head, pool + norm, is `pm_mean_ln`.

On the CPU (module AND input there) the modules run the reference's arithmetic: plain `nn.Sequential.forward`.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import _f32, derived
from .vit import _no_download


class Permute(nn.Module):
    def __init__(self, *dims):
        super().__init__()
        self.dims = dims

    def forward(self, x: Tensor) -> Tensor:
        return x.permute(self.dims)


def _pad64(n: int) -> int:
    return -(-n // 64) * 64


def _gemm(x: Tensor, w: Tensor, b: Tensor, act: str = "none", resid: Tensor | None = None, out_dtype=torch.float32,
          K: int | None = None) -> Tensor:
    """x (M, Kp) rows of the block's GEMM dtype -> act(x[:, :K] @ w.T + b) (+ resid).  bf16: w (N, Kp) with zero columns past K;
    f32: w (N, K) and the first K columns of x (window form of pm_linear_f32)."""
    if w.dtype == torch.bfloat16:
        return ops.linear(x, w, b, act=act, resid=resid, out_dtype=out_dtype)
    return ops.linear_f32(x, w, b, act=act, resid=resid, M=x.shape[0], K=w.shape[1], row_stride=x.stride(0))


class ConvNeXtBlock(nn.Sequential):
    expansion = 4

    def __init__(self, d_model: int, norm_eps: float = 1e-6, v2: bool = False) -> None:
        hidden_dim = d_model * self.expansion
        super().__init__(
            Permute(0, 3, 1, 2),
            nn.Conv2d(d_model, d_model, 7, padding=3, groups=d_model),
            Permute(0, 2, 3, 1),
            nn.LayerNorm(d_model, norm_eps),
            nn.Linear(d_model, hidden_dim),
            nn.GELU(),
            nn.Linear(hidden_dim, d_model),
        )
        self.gamma = nn.Parameter(torch.full((d_model,), 1e-6))

    def _packed(self):
        """Derived operands: dwconv weight f32 (7, 7, C); fc1 (Np, Cp) / bias (Np) and fc2 with gamma folded in (C, Np) / bias (C)
        in the GEMM dtype (bf16: zero-padded to Np = 4C and Cp = C rounded up to 64; f32: unpadded)."""
        dw, fc1, fc2 = self[1], self[4], self[6]
        params = (dw.weight, dw.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, self.gamma)

        def build():
            C, Hd = fc1.in_features, fc1.out_features
            wdw = dw.weight.detach().float().reshape(C, 7, 7).permute(1, 2, 0).contiguous()
            g = self.gamma.detach().float()
            w1, b1 = fc1.weight.detach().float(), fc1.bias.detach().float()
            w2, b2 = fc2.weight.detach().float() * g[:, None], fc2.bias.detach().float() * g
            if fc1.weight.dtype == torch.bfloat16:
                Cp, Np = _pad64(C), _pad64(Hd)
                w1p = w1.new_zeros((Np, Cp))
                w1p[:Hd, :C] = w1
                b1p = b1.new_zeros(Np)
                b1p[:Hd] = b1
                w2p = w2.new_zeros((C, Np))
                w2p[:, :Hd] = w2
                return wdw, w1p.to(torch.bfloat16), b1p, w2p.to(torch.bfloat16).contiguous(), b2.contiguous()
            return wdw, w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()

        return derived(self, "convnext_block", params, build)

    def run(self, h: Tensor, N: int, H: int, W: int) -> Tensor:
        """h: f32 residual rows (N*H*W, C) -> h + block(h), f32 rows."""
        C = h.shape[1]
        dw, ln = self[1], self[3]
        wdw, w1, b1, w2, b2 = self._packed()
        gdt = w1.dtype
        t = ops.dwconv7_ln(h.view(N, H, W, C), wdw, _f32(dw, "b", dw.bias), _f32(ln, "g", ln.weight), _f32(ln, "b", ln.bias),
                           ln.eps, gdt)
        u = _gemm(t, w1, b1, act="gelu", out_dtype=gdt)
        return _gemm(u, w2, b2, resid=h, out_dtype=torch.float32)

    def forward(self, x: Tensor) -> Tensor:
        """(N, H, W, C) NHWC in and out, as the reference's block."""
        p = self.gamma
        if _cpu.on_cpu(x, p):
            return x + super().forward(x) * self.gamma
        ops.check_devices(x, p)
        if x.dim() != 4:
            raise ValueError(f"ConvNeXtBlock: expected (N, H, W, C), got {tuple(x.shape)}")
        N, H, W, C = x.shape
        y = self.run(x.float().contiguous().view(N * H * W, C), N, H, W)
        return y.view(N, H, W, C).to(torch.promote_types(x.dtype, p.dtype))


class ConvNeXt(nn.Sequential):
    def __init__(self, d_model: int, depths: tuple[int, ...], norm_eps: float = 1e-6, v2: bool = False) -> None:
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, d_model, 4, 4), Permute(0, 2, 3, 1), nn.LayerNorm(d_model, norm_eps))

        self.stages = nn.Sequential()

        for stage_idx, depth in enumerate(depths):
            stage = nn.Sequential()
            if stage_idx > 0:
                # equivalent to PatchMerging in SwinTransformer
                downsample = nn.Sequential(
                    nn.LayerNorm(d_model, norm_eps),
                    Permute(0, 3, 1, 2),
                    nn.Conv2d(d_model, d_model * 2, 2, 2),
                    Permute(0, 2, 3, 1),
                )
                d_model *= 2
            else:
                downsample = nn.Identity()
            stage.append(downsample)

            for block_idx in range(depth):
                block = ConvNeXtBlock(d_model, norm_eps, v2)
                stage.append(block)

            self.stages.append(stage)

        self.pool = nn.Sequential(Permute(0, 3, 1, 2), nn.AdaptiveAvgPool2d(1), nn.Flatten(1))
        self.norm = nn.LayerNorm(d_model, norm_eps)

    def _stem_w(self) -> Tensor:
        conv = self.stem[0]
        return derived(conv, "stem_t", (conv.weight,), lambda: conv.weight.detach().float().reshape(conv.out_channels, 48).t().contiguous())

    @staticmethod
    def _down_w(ds: nn.Sequential) -> Tensor:
        """Conv2d(C, 2C, 2, 2) weight as the GEMM operand (2C, kh, kw, C) -> (2C, 4C) (bf16: K zero-padded to a multiple of 64)."""
        conv = ds[2]

        def build():
            w = conv.weight.detach().float().permute(0, 2, 3, 1).reshape(conv.out_channels, -1)
            if conv.weight.dtype == torch.bfloat16:
                wp = w.new_zeros((w.shape[0], _pad64(w.shape[1])))
                wp[:, : w.shape[1]] = w
                return wp.to(torch.bfloat16)
            return w.contiguous()

        return derived(conv, "s2d", (conv.weight,), build)

    def forward_stages(self, imgs: Tensor) -> list[Tensor]:
        """HIP path: [stem output, stage outputs...] as f32 NHWC (N, h, w, C) tensors, then the features (N, C_last)."""
        p = self.stem[0].weight
        ops.check_devices(imgs, p)
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"ConvNeXt: expected (N, 3, H, W), got {tuple(imgs.shape)}")
        N, _, Hi, Wi = imgs.shape
        if Hi % 32 or Wi % 32 or Hi == 0 or Wi == 0:
            raise ValueError(f"ConvNeXt: image sides must be multiples of 32, got {tuple(imgs.shape[2:])}")
        ln = self.stem[2]
        h = ops.convnext_stem(imgs.float().contiguous(), self._stem_w(), _f32(self.stem[0], "b", self.stem[0].bias),
                              _f32(ln, "g", ln.weight), _f32(ln, "b", ln.bias), ln.eps)
        H, W, C = h.shape[1], h.shape[2], h.shape[3]
        outs = [h]
        h = h.view(-1, C)
        for stage_idx, stage in enumerate(self.stages):
            if stage_idx > 0:
                ds = stage[0]
                w = self._down_w(ds)
                t = ops.ln_space_to_depth(h.view(N, H, W, C), _f32(ds[0], "g", ds[0].weight), _f32(ds[0], "b", ds[0].bias),
                                          ds[0].eps, w.dtype)
                h = _gemm(t, w, _f32(ds[2], "b", ds[2].bias))
                H, W, C = H // 2, W // 2, w.shape[0]
            for block in list(stage)[1:]:
                h = block.run(h, N, H, W)
            outs.append(h.view(N, H, W, C))
        feats = ops.mean_ln(h.view(N, H * W, C), _f32(self.norm, "g", self.norm.weight), _f32(self.norm, "b", self.norm.bias),
                            self.norm.eps, p.dtype)
        return outs + [feats]

    def forward(self, imgs: Tensor) -> Tensor:
        if _cpu.on_cpu(imgs, self.stem[0].weight):
            return super().forward(imgs)
        return self.forward_stages(imgs)[-1]

    @staticmethod
    def from_facebook(variant: str, *, pretrained: bool = False) -> "ConvNeXt":
        d_model, depths = dict(
            atto=(40, (2, 2, 6, 2)),
            femto=(48, (2, 2, 6, 2)),
            pico=(64, (2, 2, 6, 2)),
            nano=(80, (2, 2, 8, 2)),
            tiny=(96, (3, 3, 9, 3)),
            small=(96, (3, 3, 27, 3)),
            base=(128, (3, 3, 27, 3)),
            large=(192, (3, 3, 27, 3)),
            xlarge=(256, (3, 3, 27, 3)),
            huge=(352, (3, 3, 27, 3)),
        )[variant]
        if pretrained:
            _no_download("ConvNeXt.from_facebook")
        return ConvNeXt(d_model, depths)

    @torch.no_grad()
    def load_facebook_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        """facebookresearch/ConvNeXt checkpoint ("model" entry) -> this module, the reference's key map; keys it does not
        name (the classifier `head.*`) are ignored, as there."""
        state_dict = dict(state_dict)

        def copy_(m: nn.Conv2d | nn.Linear | nn.LayerNorm, prefix: str):
            m.weight.copy_(state_dict.pop(f"{prefix}.weight"))
            m.bias.copy_(state_dict.pop(f"{prefix}.bias"))

        copy_(self.stem[0], "downsample_layers.0.0")
        copy_(self.stem[2], "downsample_layers.0.1")

        for stage_idx, stage in enumerate(self.stages):
            if stage_idx > 0:
                copy_(stage[0][0], f"downsample_layers.{stage_idx}.0")
                copy_(stage[0][2], f"downsample_layers.{stage_idx}.1")

            for block_idx in range(1, len(stage)):
                block: ConvNeXtBlock = stage[block_idx]
                prefix = f"stages.{stage_idx}.{block_idx - 1}"

                copy_(block[1], f"{prefix}.dwconv")
                copy_(block[3], f"{prefix}.norm")
                copy_(block[4], f"{prefix}.pwconv1")
                copy_(block[6], f"{prefix}.pwconv2")
                block.gamma.copy_(state_dict.pop(f"{prefix}.gamma"))

        copy_(self.norm, "norm")
