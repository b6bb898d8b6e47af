"""MaxViT (https://arxiv.org/abs/2204.01697) on the MI355X kernels: drop-in for the reference's pytorch_models/image/maxvit.py (same
module-level names, constructor arguments, `nn.Sequential` indices, parameter names, non-persistent `bias_index` buffers,
`from_google` table and `load_google_state_dict` key map), so a reference state_dict loads unchanged.

Execution on HIP tensors (eval forward; no autograd), precision following the parameters (bf16: the bf16 tile GEMMs; fp32: the
f32-input MFMA GEMM), images (N, 3, H, W) with H, W multiples of 224 (every stage's side must be a multiple of the 7 x 7 window):

* activations are NHWC rows (N*H*W, C) from the stem to the head and the residual stream is f32 rows for both precisions; the
  block's NCHW <-> NHWC permutes and block() / grid() / unblock() / ungrid() never run: LayerNorm, the projections and the MLP
  are per row, so only the attention kernel (`pm_window_attention_bf16`) knows which pixels form a window;
* the stem is `pm_maxvit_stem` (Conv2d(3, s, 3, 2) + BN + GELU-tanh, fp32 VALU) -> `pm_im2col3x3_nhwc` -> one GEMM (K = 9s);
* MBConv: the pre-norm BatchNorm and the expand BatchNorm fold into the expand GEMM (GELU-tanh epilogue); the depthwise 3 x 3
  + BN + GELU-tanh is `pm_dwconv3_bn_act` run twice: once for the squeeze-excitation's per-row channel sums only, then - after
  `pm_se_gate` - again with the gate applied, writing the hidden tensor once; the shrink GEMM adds the shortcut (identity, or
  `pm_avgpool2x2_nhwc` [+ a 1 x 1 GEMM]) in its epilogue;
* EncoderLayer: LayerNorm -> packed QKV GEMM -> window attention (block or grid mode, the (H, 49, 49) relative bias a derived
  tensor) -> out_proj + residual -> LayerNorm -> linear1 + GELU-tanh -> linear2 + residual;
* the head, pool + norm, is `pm_mean_ln`.
fp32 models take the same plan on `pm_linear_f32`, except the attention: rows are gathered into window order, run through
`pm_attention_generic_f32` with the bias, and scattered back (not the timed path).  bf16 models round the f32 residual stream
to bf16 once per MBConv for the expand GEMM's operand.

On the CPU (module AND input there) the modules run the reference's arithmetic.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import MHA, MLP, LayerNorm, _f32, _wb, derived
from .vit import _no_download


def _pad64(n: int) -> int:
    return -(-n // 64) * 64


def _gemm(x: Tensor, w: Tensor, b: Tensor | None, act: str = "none", resid: Tensor | None = None,
          out_dtype=torch.float32) -> Tensor:
    """act(x @ w.T + b) (+ resid) on the GEMM of w's dtype (bf16: the tile GEMMs, f32 out or bf16; f32: pm_linear_f32)."""
    if w.dtype == torch.bfloat16:
        return ops.linear(x, w, b, act=act, resid=resid, out_dtype=out_dtype)
    return ops.linear_f32(x, w, b, act=act, resid=resid)


def _bn_fold(bn: nn.BatchNorm2d) -> tuple[Tensor, Tensor]:
    """Eval BatchNorm as f32 (scale, shift)."""
    if bn.training:
        raise NotImplementedError("MaxViT: BatchNorm in training mode is not covered by the HIP kernels; call model.eval()")

    def build():
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        return s.contiguous(), (bn.bias.detach().float() - bn.running_mean.detach().float() * s).contiguous()

    return derived(bn, "bn_fold", (bn.weight, bn.bias, bn.running_mean, bn.running_var), build)


def _gemm_w(w: Tensor, like: Tensor) -> Tensor:
    """f32 (N, K) GEMM operand in the dtype of the parameter ``like``."""
    return w.to(torch.bfloat16).contiguous() if like.dtype == torch.bfloat16 else w.contiguous()


class Conv2d(nn.Conv2d):
    """nn.Conv2d with "same" padding at stride 1 and, at stride 2, no padding after a zero row / column on the bottom / right."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, groups: int = 1,
                 bias: bool = True) -> None:
        pad = (kernel_size - 1) // 2 if stride == 1 else 0
        super().__init__(in_channels, out_channels, kernel_size, stride, pad, groups=groups, bias=bias)

    def forward(self, x: Tensor) -> Tensor:
        if self.stride == (2, 2):
            x = F.pad(x, (0, 1, 0, 1))
        return super().forward(x)


def conv_norm_act(in_dim: int, out_dim: int, kernel_size: int, stride: int = 1, groups: int = 1) -> nn.Sequential:
    conv = Conv2d(in_dim, out_dim, kernel_size, stride, groups=groups, bias=False)
    return nn.Sequential(conv, nn.BatchNorm2d(out_dim, eps=1e-3, momentum=0.01), nn.GELU(approximate="tanh"))


class SqueezeExcitation(nn.Sequential):
    def __init__(self, dim: int) -> None:
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(dim, dim // 16, 1), nn.SiLU(), nn.Conv2d(dim // 16, dim, 1), nn.Sigmoid())

    def forward(self, x: Tensor) -> Tensor:
        return x * super().forward(x)


class MBConv(nn.Module):
    """Pre-norm MBConv (no stochastic depth): shortcut(x) + residual(x)."""

    def __init__(self, in_dim: int, out_dim: int, stride: int = 1) -> None:
        super().__init__()
        hidden = 4 * out_dim
        self.residual = nn.Sequential(
            nn.BatchNorm2d(in_dim, eps=1e-3, momentum=0.01),
            conv_norm_act(in_dim, hidden, 1),
            conv_norm_act(hidden, hidden, 3, stride, hidden),
            SqueezeExcitation(hidden),
            nn.Conv2d(hidden, out_dim, 1),
        )
        self.shortcut = nn.Sequential()
        if stride > 1:
            self.shortcut.append(nn.AvgPool2d(stride))
        if out_dim != in_dim:
            self.shortcut.append(nn.Conv2d(in_dim, out_dim, 1))
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        return self.shortcut(x) + self.residual(x)

    # ---- HIP path
    def _packed(self):
        """Derived operands: expand weight / bias with both BatchNorms folded, depthwise (3, 3, C) f32 weight and BN scale / shift,
        SE weights f32, shrink and shortcut GEMM weights / biases."""
        pre, (econv, ebn, _), (dconv, dbn, _), se, shrink = self.residual
        a, b = _bn_fold(pre)
        s1, t1 = _bn_fold(ebn)
        s2, t2 = _bn_fold(dbn)
        sc_conv = self.shortcut[-1] if len(self.shortcut) and isinstance(self.shortcut[-1], nn.Conv2d) else None
        params = (econv.weight, a, b, s1, t1, s2, t2, dconv.weight, se[1].weight, se[1].bias, se[3].weight, se[3].bias, shrink.weight,
                  shrink.bias) + ((sc_conv.weight, sc_conv.bias) if sc_conv is not None else ())

        def build():
            we = econv.weight.detach().float().flatten(1)
            w_exp = s1[:, None] * we * a[None, :]
            b_exp = (s1 * (we @ b) + t1).contiguous()
            hid = dconv.out_channels
            wdw = dconv.weight.detach().float().reshape(hid, 9).t().reshape(3, 3, hid).contiguous()
            se1 = (se[1].weight.detach().float().flatten(1).contiguous(), se[1].bias.detach().float().contiguous())
            se2 = (se[3].weight.detach().float().flatten(1).contiguous(), se[3].bias.detach().float().contiguous())
            w_sh = _gemm_w(shrink.weight.detach().float().flatten(1), econv.weight)
            sc = None
            if sc_conv is not None:
                sc = (_gemm_w(sc_conv.weight.detach().float().flatten(1), econv.weight), sc_conv.bias.detach().float().contiguous())
            return (_gemm_w(w_exp, econv.weight), b_exp, wdw, s2, t2, se1, se2, w_sh, shrink.bias.detach().float().contiguous(), sc)

        return derived(self, "mbconv", params, build)

    def run(self, h: Tensor, N: int, H: int, W: int) -> tuple[Tensor, int, int]:
        """h: f32 rows (N*H*W, Cin) -> (f32 rows (N*Ho*Wo, Cout), Ho, Wo)."""
        if self.stride not in (1, 2):
            raise NotImplementedError(f"MBConv: stride {self.stride} is not covered by the HIP kernels (1 or 2)")
        w_exp, b_exp, wdw, s2, t2, (w1, b1), (w2, b2), w_sh, b_sh, sc = self._packed()
        gdt = w_exp.dtype
        Cin = h.shape[1]
        xg = h.to(gdt) if gdt != h.dtype else h
        u = _gemm(xg, w_exp, b_exp, act="approximate_gelu", out_dtype=gdt)
        hid = u.shape[1]
        u4 = u.view(N, H, W, hid)
        ps = ops.dwconv3_bn_act(u4, wdw, s2, t2, self.stride, want_psum=True, write_y=False)
        Ho, Wo = ps.shape[1], (W if self.stride == 1 else (W - 2) // 2 + 1)
        gate = ops.se_gate(ps, Ho * Wo, w1, b1, w2, b2)
        t = ops.dwconv3_bn_act(u4, wdw, s2, t2, self.stride, gate=gate, out_dtype=gdt)
        if self.stride == 2:
            p = ops.avgpool2x2(h.view(N, H, W, Cin), out_dtype=gdt if sc is not None else torch.float32).view(N * Ho * Wo, Cin)
        else:
            p = xg if sc is not None else h
        resid = _gemm(p, sc[0], sc[1]) if sc is not None else p
        return _gemm(t.view(N * Ho * Wo, hid), w_sh, b_sh, resid=resid), Ho, Wo


def block(x: Tensor, size: int) -> Tensor:
    """(N, H, W, C) -> ((N, nH*nW, size*size, C) non-overlapping size x size windows, nH, nW)."""
    N, H, W, C = x.shape
    nH, nW = H // size, W // size
    return x.view(N, nH, size, nW, size, C).transpose(2, 3).reshape(N, nH * nW, size * size, C), nH, nW


def unblock(x: Tensor, nH: int, nW: int, size: int) -> Tensor:
    N, C = x.shape[0], x.shape[-1]
    return x.view(N, nH, nW, size, size, C).transpose(2, 3).reshape(N, nH * size, nW * size, C)


def grid(x: Tensor, size: int) -> Tensor:
    """(N, H, W, C) -> ((N, nH*nW, size*size, C) dilated windows: window (i, j) = pixels (r*nH + i, c*nW + j), nH, nW)."""
    N, H, W, C = x.shape
    nH, nW = H // size, W // size
    return x.view(N, size, nH, size, nW, C).permute(0, 2, 4, 1, 3, 5).reshape(N, nH * nW, size * size, C), nH, nW


def ungrid(x: Tensor, nH: int, nW: int, size: int) -> Tensor:
    N, C = x.shape[0], x.shape[-1]
    return x.view(N, nH, nW, size, size, C).permute(0, 3, 1, 4, 2, 5).reshape(N, size * nH, size * nW, C)


def _window_bias(attn_bias: Tensor, index: Tensor) -> Tensor:
    """(H, 2s-1, 2s-1) relative table -> (H, s*s, s*s): query (r, c), key (r', c') -> table[h, index[r, r'], index[c, c']]."""
    s = index.shape[0]
    b = attn_bias[:, index[:, None, :, None], index[None, :, None, :]]  # (H, r, c, r', c')
    return b.reshape(attn_bias.shape[0], s * s, s * s)


_WINDOW_ROWS: dict = {}


def _window_rows(N: int, H: int, W: int, ws: int, mode: str, device) -> Tensor:
    """Pixel row of every (window, token) in window order (the fp32 path's gather / scatter index)."""
    key = (str(device), N, H, W, ws, mode)
    if key not in _WINDOW_ROWS:
        rows = torch.arange(N * H * W, device=device).view(N, H, W, 1)
        _WINDOW_ROWS[key] = (block if mode == "block" else grid)(rows, ws)[0].reshape(-1).contiguous()
    return _WINDOW_ROWS[key]


class RelativeMHA(MHA):
    def __init__(self, input_size: int, d_model: int, dropout: float = 0.0) -> None:
        super().__init__(d_model, head_dim=32, dropout=dropout)
        span = 2 * input_size - 1  # offsets -(input_size - 1) .. input_size - 1
        self.attn_bias = nn.Parameter(torch.zeros(self.n_heads, span, span))
        offs = torch.arange(input_size)
        self.register_buffer("bias_index", offs[None, :] - offs[:, None] + input_size - 1, persistent=False)
        self.bias_index: Tensor
        self.window_size = input_size

    def window_bias(self) -> Tensor:
        """HIP path: the (H, L, L) f32 bias, rebuilt when attn_bias changes."""
        return derived(self, "win_bias", (self.attn_bias,),
                       lambda: _window_bias(self.attn_bias.detach().float(), self.bias_index).contiguous())

    def forward(self, x: Tensor) -> Tensor:
        p = self.q_proj.weight
        if _cpu.on_cpu(x, p):
            return super().forward(x, attn_bias=_window_bias(self.attn_bias, self.bias_index))
        ops.check_devices(x, p, self.attn_bias)
        ws = self.window_size
        if x.dim() < 2 or x.shape[-2] != ws * ws:
            raise ValueError(f"RelativeMHA: expected (..., {ws * ws}, C), got {tuple(x.shape)}")
        C = x.shape[-1]
        a = x.reshape(-1, C).to(p.dtype).contiguous()
        y = self.attend_rows(a, a.shape[0] // (ws * ws), ws, ws, "block")
        return y.view(*x.shape[:-1], y.shape[-1])

    def attend_rows(self, a: Tensor, N: int, H: int, W: int, mode: str, resid: Tensor | None = None) -> Tensor:
        """a: normalised pixel rows (N*H*W, C) in the parameters' dtype -> out_proj(window attention) (+ resid, f32 rows)."""
        if self.training and self.dropout > 0.0:
            raise NotImplementedError("RelativeMHA: inference only (attention dropout is not implemented)")
        ws, d = self.window_size, self.n_heads * 32
        op = self.out_proj
        if a.dtype == torch.bfloat16:
            w, b = self._pack("qkv")
            qkv = ops.linear(a, w, b)
            o = ops.window_attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], N, H, W, self.n_heads, ws, mode, self.window_bias())
            return ops.linear(o, _wb(op, "w", op.weight), _f32(op, "b", op.bias), resid=resid,
                              out_dtype=torch.float32 if resid is not None else torch.bfloat16)
        w, b = self._pack32("qkv")
        qkv = ops.linear_f32(a, w, b)
        idx = _window_rows(N, H, W, ws, mode, a.device)
        L = ws * ws
        qw = qkv.index_select(0, idx).view(-1, L, 3 * d)
        ow = ops.attention_f32(qw[..., :d], qw[..., d:2 * d], qw[..., 2 * d:], self.n_heads, False, self.window_bias()[None])
        o = torch.empty((a.shape[0], d), dtype=torch.float32, device=a.device)
        o.index_copy_(0, idx, ow.view(-1, d))
        return ops.linear_f32(o, op.weight, op.bias, resid=resid)


class EncoderLayer(nn.Module):
    def __init__(self, d_model: int, window_size: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.sa_norm = LayerNorm(d_model, 1e-5)
        self.sa = RelativeMHA(window_size, d_model, dropout)
        self.mlp_norm = LayerNorm(d_model, 1e-5)
        self.mlp = MLP(d_model, d_model * 4, dropout, act="approximate_gelu")

    def forward(self, x: Tensor) -> Tensor:
        p = self.sa.q_proj.weight
        if _cpu.on_cpu(x, p):
            x = x + self.sa(self.sa_norm(x))
            return x + self.mlp(self.mlp_norm(x))
        ops.check_devices(x, p)
        ws = self.sa.window_size
        if x.dim() < 2 or x.shape[-2] != ws * ws:
            raise ValueError(f"EncoderLayer: expected (..., {ws * ws}, C), got {tuple(x.shape)}")
        C = x.shape[-1]
        h = x.reshape(-1, C).float().contiguous()
        y = self.run(h, h.shape[0] // (ws * ws), ws, ws, "block")
        return y.view(x.shape).to(torch.promote_types(x.dtype, p.dtype))

    def run(self, h: Tensor, N: int, H: int, W: int, mode: str) -> Tensor:
        """h: f32 residual rows (N*H*W, C) in pixel order -> the layer's output rows, f32; attention over ``mode`` windows."""
        if self.training and self.mlp.dropout.p > 0.0:
            raise NotImplementedError("EncoderLayer: inference only (dropout is not implemented)")
        gdt = self.sa.q_proj.weight.dtype
        n1, n2, l1, l2 = self.sa_norm, self.mlp_norm, self.mlp.linear1, self.mlp.linear2
        a = ops.layernorm(h, _f32(n1, "g", n1.weight), _f32(n1, "b", n1.bias), n1.eps, gdt)
        h = self.sa.attend_rows(a, N, H, W, mode, resid=h)
        a = ops.layernorm(h, _f32(n2, "g", n2.weight), _f32(n2, "b", n2.bias), n2.eps, gdt)
        if gdt == torch.bfloat16:
            u = ops.linear(a, _wb(l1, "w", l1.weight), _f32(l1, "b", l1.bias), act="approximate_gelu")
            return ops.linear(u, _wb(l2, "w", l2.weight), _f32(l2, "b", l2.bias), resid=h, out_dtype=torch.float32)
        u = ops.linear_f32(a, l1.weight, l1.bias, act="approximate_gelu")
        return ops.linear_f32(u, l2.weight, l2.bias, resid=h)


class MaxViTBlock(nn.Module):
    def __init__(self, in_dim: int, out_dim: int, stride: int = 1, window_size: int = 7, dropout: float = 0.0) -> None:
        super().__init__()
        self.mbconv = MBConv(in_dim, out_dim, stride)
        self.block_layer = EncoderLayer(out_dim, window_size, dropout)
        self.grid_layer = EncoderLayer(out_dim, window_size, dropout)
        self.window_size = window_size

    def forward(self, x: Tensor) -> Tensor:
        """(N, C, H, W) in and out, as the reference's block."""
        p = self.block_layer.sa.q_proj.weight
        if _cpu.on_cpu(x, p):
            ws = self.window_size
            x = self.mbconv(x).permute(0, 2, 3, 1)
            x, nH, nW = block(x, ws)
            x = unblock(self.block_layer(x), nH, nW, ws)
            x, nH, nW = grid(x, ws)
            x = ungrid(self.grid_layer(x), nH, nW, ws)
            return x.permute(0, 3, 1, 2)
        ops.check_devices(x, p)
        if x.dim() != 4:
            raise ValueError(f"MaxViTBlock: expected (N, C, H, W), got {tuple(x.shape)}")
        N, C, H, W = x.shape
        h, Ho, Wo = self.run(x.permute(0, 2, 3, 1).float().contiguous().view(-1, C), N, H, W)
        return h.view(N, Ho, Wo, -1).permute(0, 3, 1, 2).to(torch.promote_types(x.dtype, p.dtype))

    def run(self, h: Tensor, N: int, H: int, W: int) -> tuple[Tensor, int, int]:
        """h: f32 NHWC rows (N*H*W, Cin) -> (f32 rows (N*Ho*Wo, Cout), Ho, Wo)."""
        if self.mbconv.stride == 2 and (H % 2 or W % 2):
            raise ValueError(f"MaxViTBlock: a stride-2 block needs even sides, got {H} x {W}")
        h, H, W = self.mbconv.run(h, N, H, W)
        ws = self.window_size
        if H % ws or W % ws:
            raise ValueError(f"MaxViTBlock: sides {H} x {W} are not multiples of the window {ws}")
        h = self.block_layer.run(h, N, H, W, "block")
        return self.grid_layer.run(h, N, H, W, "grid"), H, W


class MaxViT(nn.Module):
    def __init__(self, stem_dim: int, n_blocks: list[int], dims: list[int], dropout: float = 0.0):
        super().__init__()
        self.stem = nn.Sequential(
            Conv2d(3, stem_dim, 3, 2),
            nn.BatchNorm2d(stem_dim, eps=1e-3, momentum=0.01),
            nn.GELU(approximate="tanh"),
            Conv2d(stem_dim, stem_dim, 3),
        )
        self.stages = nn.Sequential()
        in_dim = stem_dim
        for n_block, dim in zip(n_blocks, dims):
            stage = nn.Sequential()
            for i in range(n_block):
                stage.append(MaxViTBlock(in_dim, dim, stride=2 if i == 0 else 1, dropout=dropout))
                in_dim = dim
            self.stages.append(stage)
        self.norm = nn.LayerNorm(in_dim, 1e-5)

    def _stem_ops(self):
        """Derived: stem conv 1 as f32 (27, s) with the BatchNorm scale folded + the shift (its bias folded in); conv 2 as the GEMM operand
        (s, kh, kw, s) -> (s, 9s) (bf16: K zero-padded to a multiple of 64) + f32 bias."""
        c1, bn, _, c2 = self.stem
        sc, sh = _bn_fold(bn)

        def build():
            s = c1.out_channels
            wt = (c1.weight.detach().float() * sc[:, None, None, None]).reshape(s, 27).t().contiguous()
            shift = sh if c1.bias is None else (sh + sc * c1.bias.detach().float()).contiguous()
            w2 = c2.weight.detach().float().permute(0, 2, 3, 1).reshape(s, 9 * s)
            if c2.weight.dtype == torch.bfloat16:
                wp = w2.new_zeros((s, _pad64(9 * s)))
                wp[:, : 9 * s] = w2
                w2 = wp.to(torch.bfloat16)
            return wt, shift, w2.contiguous(), c2.bias.detach().float().contiguous()

        return derived(self.stem, "stem", (c1.weight, c1.bias, sc, sh, c2.weight, c2.bias), build)

    def forward_stages(self, imgs: Tensor) -> list[Tensor]:
        """HIP path: [stem output, stage outputs...] as f32 NHWC (N, h, w, C) tensors, then the features (N, C_last)."""
        p = self.stem[0].weight
        ops.check_devices(imgs, p)
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"MaxViT: expected (N, 3, H, W), got {tuple(imgs.shape)}")
        N, _, Hi, Wi = imgs.shape
        if Hi % 224 or Wi % 224 or Hi == 0 or Wi == 0:
            raise ValueError(f"MaxViT: image sides must be multiples of 224, got {tuple(imgs.shape[2:])}")
        wt, sh, w2, b2 = self._stem_ops()
        gdt = w2.dtype
        s0 = ops.maxvit_stem(imgs.float().contiguous(), wt, sh, gdt)
        N, H, W, C = s0.shape
        h = _gemm(ops.im2col3x3(s0, ldy=w2.shape[1]), w2, b2)
        outs = [h.view(N, H, W, C)]
        for stage in self.stages:
            for blk in stage:
                h, H, W = blk.run(h, N, H, W)
            outs.append(h.view(N, H, W, h.shape[1]))
        C = h.shape[1]
        feats = ops.mean_ln(h.view(N, H * W, C), _f32(self.norm, "g", self.norm.weight), _f32(self.norm, "b", self.norm.bias),
                            self.norm.eps, p.dtype)
        return outs + [feats]

    def forward(self, x: Tensor) -> Tensor:
        if _cpu.on_cpu(x, self.stem[0].weight):
            x = self.stem(x)
            for stage in self.stages:
                x = stage(x)
            return self.norm(F.adaptive_avg_pool2d(x, 1).flatten(1))
        return self.forward_stages(x)[-1]

    @staticmethod
    def from_google(variant: str, *, pretrained: bool = False, **kwargs) -> "MaxViT":
        # (stem_dim, blocks per stage, dims per stage): table 1 of the paper
        stem_dim, n_blocks, dims = dict(
            tiny=(64, [2, 2, 5, 2], [64, 128, 256, 512]),
            small=(64, [2, 2, 5, 2], [96, 192, 384, 768]),
            base=(64, [2, 6, 14, 2], [96, 192, 384, 768]),
            large=(128, [2, 6, 14, 2], [128, 256, 512, 1024]),
            xlarge=(192, [2, 6, 14, 2], [192, 384, 768, 1536]),
        )[variant]
        if pretrained:
            _no_download("MaxViT.from_google")
        return MaxViT(stem_dim, n_blocks, dims, **kwargs)

    @torch.no_grad()
    def load_google_state_dict(self, reader) -> None:
        """google-research/maxvit TF checkpoint -> this module, the reference's key map (the ExponentialMovingAverage copies).
        ``reader``: any object with get_variable_to_shape_map() and get_tensor(name) (e.g. tf.train.load_checkpoint's)."""
        ema = "/ExponentialMovingAverage"
        pending = {k for k in reader.get_variable_to_shape_map() if k.endswith("ExponentialMovingAverage")}

        def param(name: str) -> Tensor:
            key = f"maxvit/{name}{ema}"
            pending.remove(key)
            return torch.from_numpy(reader.get_tensor(key))

        def conv(m: nn.Conv2d, prefix: str, depthwise: bool = False) -> None:
            if depthwise:  # (kh, kw, C, 1) -> (C, 1, kh, kw)
                m.weight.copy_(param(f"{prefix}/depthwise_kernel").permute(2, 3, 0, 1))
            else:  # (kh, kw, in, out) -> (out, in, kh, kw)
                m.weight.copy_(param(f"{prefix}/kernel").permute(3, 2, 0, 1))
            if m.bias is not None:
                m.bias.copy_(param(f"{prefix}/bias"))

        def dense(m: nn.Linear, prefix: str, merge: int | None = None) -> None:
            w = param(f"{prefix}/weight")
            if merge is not None:  # q / k / v (d, H, 32): merge dims 1, 2; o (H, 32, d): merge dims 0, 1
                w = w.flatten(merge, merge + 1)
            m.weight.copy_(w.T)
            m.bias.copy_(param(f"{prefix}/bias").flatten())

        def norm(m: nn.LayerNorm | nn.BatchNorm2d, prefix: str) -> None:
            m.weight.copy_(param(f"{prefix}/gamma"))
            m.bias.copy_(param(f"{prefix}/beta"))
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(param(f"{prefix}/moving_mean"))
                m.running_var.copy_(param(f"{prefix}/moving_variance"))

        conv(self.stem[0], "stem/conv_0")
        norm(self.stem[1], "stem/norm_0")
        conv(self.stem[3], "stem/conv_1")
        for si, stage in enumerate(self.stages):
            for bi, blk in enumerate(stage):
                pre = f"block_{si:02d}_{bi:02d}"
                r = blk.mbconv.residual
                norm(r[0], f"{pre}/mbconv/pre_norm")
                conv(r[1][0], f"{pre}/mbconv/expand_conv")
                norm(r[1][1], f"{pre}/mbconv/expand_norm")
                conv(r[2][0], f"{pre}/mbconv/depthwise_conv", depthwise=True)
                norm(r[2][1], f"{pre}/mbconv/depthwise_norm")
                conv(r[3][1], f"{pre}/mbconv/se/reduce_conv2d")
                conv(r[3][3], f"{pre}/mbconv/se/expand_conv2d")
                conv(r[4], f"{pre}/mbconv/shrink_conv")
                if len(blk.mbconv.shortcut) == 2:
                    conv(blk.mbconv.shortcut[1], f"{pre}/mbconv/shortcut_conv")
                for layer, sfx in ((blk.block_layer, ""), (blk.grid_layer, "_1")):
                    norm(layer.sa_norm, f"{pre}/attn_layer_norm{sfx}")
                    layer.sa.attn_bias.copy_(param(f"{pre}/attention{sfx}/relative_bias"))
                    for n in "qkv":
                        dense(getattr(layer.sa, f"{n}_proj"), f"{pre}/attention{sfx}/{n}", 1)
                    dense(layer.sa.out_proj, f"{pre}/attention{sfx}/o", 0)
                    norm(layer.mlp_norm, f"{pre}/ffn_layer_norm{sfx}")
                    dense(layer.mlp.linear1, f"{pre}/ffn{sfx}/expand_dense")
                    dense(layer.mlp.linear2, f"{pre}/ffn{sfx}/shrink_dense")
        norm(self.norm, "final_layer_norm")
