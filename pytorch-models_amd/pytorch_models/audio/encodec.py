"""EnCodec (https://arxiv.org/abs/2210.13438, https://github.com/facebookresearch/encodec) on the MI355X kernels: drop-in for the
reference's pytorch_models/audio/encodec.py (same classes, constructor arguments and defaults, child names and state-dict keys -
`pad` / `conv` / `norm` / `unpad`, `layers` / `shortcut`, `encoder` / `decoder` / `quantizer`, the weight-norm keys
`conv.parametrizations.weight.original0/1` - and the upstream key renaming), so a reference state_dict loads unchanged.

Execution on HIP tensors is fp32 ONLY (eval forward; no autograd): the encoder ends in an argmin over 1024 distances, and with
bf16 operands a tenth of the codes differ from the reference's - another codec.  fp32 parameters (the reference's default and
what `from_facebook` returns) run on the exact-product f32 MFMA (csrc/encodec.hip); bf16 / fp16 parameters on HIP raise.
Activations are time-major (B, T, C) inside, the public layout stays (B, C, T):

* Conv1d           -> `pm_conv1d_f32`: implicit GEMM; the reflect padding (and the extra padding up to the stride) as mirrored
                      indices, the ELU in front of the convolution applied to the operand as it is loaded, bias and - in a
                      weight-norm block - `shortcut(x) +` in the epilogue;
* ConvTranspose1d  -> the same kernel's zero-padded / "up" mode on a repacked (stride * Cout, 2 * Cin) matrix (kernel == 2 * stride
                      only, which is every layer of the decoder), `Unpad1d` as the trim of the output rows;
* LSTM             -> `pm_lstm_f32`: a GEMM for layer 0's input projections of all frames, then one launch per step with both
                      layers in it (layer 1 one frame behind layer 0);
* RVQ              -> `pm_rvq_encode_f32` (every stage in one kernel) / `pm_rvq_decode_f32`;
* GroupNorm(1, C) of `time_group_norm` -> `pm_groupnorm1_f32` in place (a block's shortcut added by the same kernel); the 48 kHz
  input scale -> `pm_encodec_scale_f32` / `pm_scale_clips_f32`; layout changes -> `pm_transpose_add_f32`.
Derived operands (the effective weight g * v / |v| repacked tap-major, the transposed convolutions' matrices, the LSTM's summed
biases, the stacked codebooks and their squared norms) are built once per module and rebuilt when a parameter changes.
There is no fallback: what the kernels do not serve raises.

On the CPU (module AND input there) every class runs the reference's arithmetic in plain torch, any dtype, training included.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import derived


def _placement(x: Tensor, p: Tensor) -> bool:
    """True: input and parameters on the CPU (the plain-torch form); False: both on the current HIP device.  Any other placement
    is a ValueError carrying the shared guards' message."""
    try:
        if _cpu.on_cpu(x, p):
            return True
        ops.check_devices(x, p)
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return False


def _gate(m: nn.Module, x: Tensor, p: Tensor, who: str, channels: int | None) -> None:
    """What the HIP path refuses: anything but fp32 parameters and input, training mode, a wrong rank or channel count."""
    if p.dtype != torch.float32 or x.dtype != torch.float32:
        raise NotImplementedError(
            f"{who}: fp32 parameters and input only on a HIP device (got {p.dtype} parameters, {x.dtype} input): the quantizer's "
            "argmin does not survive bf16 / fp16 operands (a tenth of the codes change), so there is no reduced-precision path")
    if m.training:
        raise NotImplementedError(f"{who}: inference only on a HIP device (call .eval()); training runs on the CPU form")
    if x.dim() != 3 or (channels is not None and x.shape[1] != channels):
        raise ValueError(f"{who}: expected (B, {channels if channels is not None else 'C'}, T), got {tuple(x.shape)}")
    if x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")


def _to_tm(x: Tensor) -> Tensor:
    """(B, C, T) -> time-major (B, T, C)."""
    x = x.contiguous()
    return x.view(x.shape[0], x.shape[2], 1) if x.shape[1] == 1 else ops.transpose_add_f32(x)


def _from_tm(x: Tensor) -> Tensor:
    """time-major (B, T, C) -> (B, C, T)."""
    return x.view(x.shape[0], 1, x.shape[1]) if x.shape[2] == 1 else ops.transpose_add_f32(x)


def _weight_params(conv: nn.Module) -> tuple:
    """The tensors the effective weight of a (possibly weight-normed) convolution is derived from."""
    if nn.utils.parametrize.is_parametrized(conv, "weight"):
        return tuple(conv.parametrizations.weight.parameters())
    return (conv.weight,)


def _f32c(module: nn.Module, key: str, t: Tensor | None) -> Tensor | None:
    return None if t is None else derived(module, key, (t,), lambda: t.detach().float().contiguous())


def _norm_hip(norm: nn.Module, y: Tensor, resid: Tensor | None) -> Tensor:
    return ops.groupnorm1_(y, _f32c(norm, "g", norm.weight), _f32c(norm, "b", norm.bias), norm.eps, resid)


class Pad1d(nn.Module):
    def __init__(self, kernel_size: int, stride: int, causal: bool) -> None:
        super().__init__()
        padding_total = kernel_size - stride
        self.right = 0 if causal else padding_total // 2
        self.left = padding_total - self.right
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        if x.device.type != "cpu":
            raise NotImplementedError("Pad1d: on a HIP device the padding is part of the convolution kernel (call the Conv1d that owns it)")
        extra = math.ceil(x.shape[2] / self.stride) * self.stride - x.shape[2]  # the length rounded up to the stride
        return F.pad(x, (self.left, self.right + extra), mode="reflect")


class Unpad1d(nn.Module):
    def __init__(self, kernel_size: int, stride: int, causal: bool = False) -> None:
        super().__init__()
        padding_total = kernel_size - stride
        self.right = padding_total if causal else padding_total // 2
        self.left = padding_total - self.right

    def forward(self, x: Tensor) -> Tensor:
        if x.device.type != "cpu":
            raise NotImplementedError("Unpad1d: on a HIP device the trim is part of the transposed-convolution kernel (call the ConvTranspose1d that owns it)")
        return x[..., self.left : -self.right]


class Conv1d(nn.Sequential):
    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        kernel_size: int,
        stride: int = 1,
        norm_type: str = "weight_norm",
        causal: bool = False,
    ) -> None:
        super().__init__()
        self.pad = Pad1d(kernel_size, stride, causal)
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride)
        self.norm = nn.GroupNorm(1, out_channels) if norm_type == "time_group_norm" else nn.Identity()
        if norm_type == "weight_norm":
            nn.utils.parametrizations.weight_norm(self.conv)

    def run_tm(self, x: Tensor, elu: bool = False, resid: Tensor | None = None) -> Tensor:
        """HIP: time-major (B, T, Cin) -> (B, ceil(T / stride), Cout) = norm(conv(pad(ELU(x) if elu else x))) [+ resid]."""
        conv = self.conv
        k, s = conv.kernel_size[0], conv.stride[0]
        if x.shape[2] != conv.in_channels:
            raise ValueError(f"Conv1d: built for {conv.in_channels} channels, got {x.shape[2]}")
        # tap-major rows: column tap * Cin + ci, the order of a time-major window
        w = derived(self, "w2d", _weight_params(conv), lambda: conv.weight.detach().float().permute(0, 2, 1).reshape(conv.out_channels, -1).contiguous())
        extra = -x.shape[1] % s
        gn = isinstance(self.norm, nn.GroupNorm)
        y = ops.conv1d_f32(x, w, _f32c(self, "b", conv.bias), k=k, stride=s, left=self.pad.left, right=self.pad.right + extra, elu=elu,
                           resid=None if gn else resid)
        return _norm_hip(self.norm, y, resid) if gn else y

    def forward(self, x: Tensor) -> Tensor:
        p = _weight_params(self.conv)[0]
        if _placement(x, p):
            return super().forward(x)
        _gate(self, x, p, "Conv1d", self.conv.in_channels)
        return _from_tm(self.run_tm(_to_tm(x)))


class ConvTranspose1d(nn.Sequential):
    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        kernel_size: int,
        stride: int = 1,
        norm_type: str = "weight_norm",
        causal: bool = False,
    ) -> None:
        super().__init__()
        self.conv = nn.ConvTranspose1d(in_channels, out_channels, kernel_size, stride)
        self.norm = nn.GroupNorm(1, out_channels) if norm_type == "time_group_norm" else nn.Identity()
        self.unpad = Unpad1d(kernel_size, stride, causal)
        if norm_type == "weight_norm":
            nn.utils.parametrizations.weight_norm(self.conv)

    def run_tm(self, x: Tensor, elu: bool = False) -> Tensor:
        """HIP: time-major (B, T, Cin) -> (B, T * stride, Cout).  With kernel 2 s, output sample j s + r is
        W[:, :, r]^T x[j] + W[:, :, r + s]^T x[j - 1]: a window product over rows [x[j-1], x[j]] whose (T + 1, s * Cout) result is
        the time-major output before the trim."""
        conv = self.conv
        k, s = conv.kernel_size[0], conv.stride[0]
        if k != 2 * s:
            raise ValueError(f"ConvTranspose1d: the HIP kernel serves kernel_size == 2 * stride (got {k}, {s})")
        if x.shape[2] != conv.in_channels:
            raise ValueError(f"ConvTranspose1d: built for {conv.in_channels} channels, got {x.shape[2]}")
        cin, cout = conv.in_channels, conv.out_channels

        def pack():  # [r * Cout + co][j * Cin + ci] = weight[ci][co][r + (1 - j) * s]
            return conv.weight.detach().float().view(cin, cout, 2, s).flip(2).permute(3, 1, 2, 0).reshape(s * cout, 2 * cin).contiguous()

        w = derived(self, "w2d", _weight_params(conv), pack)
        bias = _f32c(self, "b", conv.bias)
        left, right = self.unpad.left, self.unpad.right
        if not isinstance(self.norm, nn.GroupNorm):
            return ops.conv1d_f32(x, w, bias, k=2, left=1, right=1, zero_pad=True, elu=elu, up=s, trim=left, t_out=(x.shape[1] + 1) * s - left - right)
        # GroupNorm sees the untrimmed output (the reference normalises before Unpad1d): trim afterwards, as a view
        y = _norm_hip(self.norm, ops.conv1d_f32(x, w, bias, k=2, left=1, right=1, zero_pad=True, elu=elu, up=s), None)
        return y[:, left : y.shape[1] - right]

    def forward(self, x: Tensor) -> Tensor:
        p = _weight_params(self.conv)[0]
        if _placement(x, p):
            return super().forward(x)
        _gate(self, x, p, "ConvTranspose1d", self.conv.in_channels)
        return _from_tm(self.run_tm(_to_tm(x)).contiguous())


class LSTM(nn.LSTM):
    def __init__(self, dim: int, n_layers: int) -> None:
        super().__init__(dim, dim, n_layers)

    def run_tm(self, x: Tensor) -> Tensor:
        """HIP: time-major (B, T, dim) -> x + lstm(x)."""
        if x.shape[2] != self.input_size:
            raise ValueError(f"LSTM: built for {self.input_size} channels, got {x.shape[2]}")
        w_ih, w_hh, bias = [], [], []
        for l in range(self.num_layers):
            wi, wh = getattr(self, f"weight_ih_l{l}"), getattr(self, f"weight_hh_l{l}")
            bi, bh = getattr(self, f"bias_ih_l{l}"), getattr(self, f"bias_hh_l{l}")
            w_ih.append(_f32c(self, f"wi{l}", wi))
            w_hh.append(_f32c(self, f"wh{l}", wh))
            bias.append(derived(self, f"b{l}", (bi, bh), lambda: (bi.detach().float() + bh.detach().float()).contiguous()))
        return ops.lstm_f32(x if x.is_contiguous() else x.contiguous(), w_ih, w_hh, bias, residual=True)

    def forward(self, x: Tensor) -> Tensor:
        p = self.weight_ih_l0
        if _placement(x, p):  # nn.LSTM is sequence-first; the skip connection goes around both layers
            return x + super().forward(x.permute(2, 0, 1))[0].permute(1, 2, 0)
        _gate(self, x, p, "LSTM", self.input_size)
        return _from_tm(self.run_tm(_to_tm(x)))


class EnCodecBlock(nn.Module):
    def __init__(self, dim: int, kernel_size: int, norm_type: str, causal: bool) -> None:
        super().__init__()
        self.layers = nn.Sequential(
            nn.ELU(),
            Conv1d(dim, dim // 2, kernel_size, 1, norm_type, causal),
            nn.ELU(),
            Conv1d(dim // 2, dim, 1, 1, norm_type, causal),
        )
        self.shortcut = Conv1d(dim, dim, 1, 1, norm_type, causal)

    def run_tm(self, x: Tensor) -> Tensor:
        """HIP: three launches (five with GroupNorm): the shortcut, then the two convolutions with their ELUs on load and the sum
        in the last epilogue."""
        sc = self.shortcut.run_tm(x)
        h = self.layers[1].run_tm(x, elu=True)
        return self.layers[3].run_tm(h, elu=True, resid=sc)

    def forward(self, x: Tensor) -> Tensor:
        p = _weight_params(self.shortcut.conv)[0]
        if _placement(x, p):
            return self.shortcut(x) + self.layers(x)
        _gate(self, x, p, "EnCodecBlock", self.shortcut.conv.in_channels)
        return _from_tm(self.run_tm(_to_tm(x)))


def _run_stack_tm(stack: nn.Sequential, x: Tensor, keep: dict | None = None) -> Tensor:
    """The HIP walk over an encoder / decoder: an nn.ELU is carried into the convolution behind it.  ``keep`` receives every
    child's output (key = its index), time-major."""
    elu = False
    for name, m in stack.named_children():
        if isinstance(m, nn.ELU):
            if m.alpha != 1.0:
                raise NotImplementedError("EnCodec: the HIP kernels apply ELU with alpha == 1")
            elu = True
            continue
        if isinstance(m, (Conv1d, ConvTranspose1d)):
            x = m.run_tm(x, elu=elu)
        elif elu:
            raise NotImplementedError(f"EnCodec: an ELU in front of {type(m).__name__} is not served (only in front of a convolution)")
        elif isinstance(m, (EnCodecBlock, LSTM)):
            x = m.run_tm(x)
        else:
            raise NotImplementedError(f"EnCodec: no HIP kernel for a {type(m).__name__} in the stack")
        elu = False
        if keep is not None:
            keep[name] = x
    if elu:
        raise NotImplementedError("EnCodec: a trailing ELU is not served")
    return x


def _stack_channels(stack: nn.Sequential) -> int:
    return next(iter(stack.children())).conv.in_channels


class EnCodecEncoder(nn.Sequential):
    def __init__(
        self,
        audio_channels: int,
        base_dim: int = 32,
        dim: int = 128,
        strides: tuple[int, ...] = (2, 4, 5, 8),
        norm_type: str = "weight_norm",
        causal: bool = False,
    ) -> None:
        super().__init__()
        self.append(Conv1d(audio_channels, base_dim, 7, norm_type=norm_type, causal=causal))
        for stride in strides:  # a residual block, then the strided convolution that doubles the width
            self.append(EnCodecBlock(base_dim, 3, norm_type, causal))
            self.append(nn.ELU())
            self.append(Conv1d(base_dim, base_dim * 2, stride * 2, stride, norm_type, causal))
            base_dim *= 2
        self.append(LSTM(base_dim, 2))
        self.append(nn.ELU())
        self.append(Conv1d(base_dim, dim, 7, 1, norm_type, causal))

    def run_tm(self, x: Tensor, keep: dict | None = None) -> Tensor:
        return _run_stack_tm(self, x, keep)

    def forward(self, x: Tensor) -> Tensor:
        """(B, audio_channels, T) -> the latent (B, dim, ceil(T / prod(strides)))."""
        p = _weight_params(self[0].conv)[0]
        if _placement(x, p):
            return super().forward(x)
        _gate(self, x, p, "EnCodecEncoder", _stack_channels(self))
        return _from_tm(self.run_tm(_to_tm(x)))

    def load_facebook_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        self.load_state_dict({_rename_key(k): v for k, v in state_dict.items()})


class EnCodecDecoder(nn.Sequential):
    def __init__(
        self,
        audio_channels: int,
        base_dim: int = 32,
        dim: int = 128,
        strides: tuple[int, ...] = (8, 5, 4, 2),
        norm_type: str = "weight_norm",
        causal: bool = False,
    ) -> None:
        super().__init__()
        base_dim *= 2 ** len(strides)
        self.append(Conv1d(dim, base_dim, 7, 1, norm_type, causal))
        self.append(LSTM(base_dim, 2))
        for stride in strides:  # the transposed convolution that halves the width, then a residual block
            self.append(nn.ELU())
            self.append(ConvTranspose1d(base_dim, base_dim // 2, stride * 2, stride, norm_type, causal))
            self.append(EnCodecBlock(base_dim // 2, 3, norm_type, causal))
            base_dim //= 2
        self.append(nn.ELU())
        self.append(Conv1d(base_dim, audio_channels, 7, 1, norm_type, causal))

    def run_tm(self, x: Tensor, keep: dict | None = None) -> Tensor:
        return _run_stack_tm(self, x, keep)

    def forward(self, x: Tensor) -> Tensor:
        """The latent (B, dim, T) -> (B, audio_channels, T * prod(strides))."""
        p = _weight_params(self[0].conv)[0]
        if _placement(x, p):
            return super().forward(x)
        _gate(self, x, p, "EnCodecDecoder", _stack_channels(self))
        return _from_tm(self.run_tm(_to_tm(x)))

    def load_facebook_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        self.load_state_dict({_rename_key(k): v for k, v in state_dict.items()})


def _check_rows(x: Tensor, p: Tensor, who: str) -> None:
    if p.dtype != torch.float32 or x.dtype != torch.float32:
        raise NotImplementedError(f"{who}: fp32 codebooks and rows only on a HIP device (got {p.dtype}, {x.dtype})")
    if x.dim() < 1 or x.shape[-1] != p.shape[-1]:
        raise ValueError(f"{who}: rows of {p.shape[-1]} values expected, got {tuple(x.shape)}")


def _check_codes(x: Tensor, who: str) -> None:
    if x.dtype != torch.int64:
        raise ValueError(f"{who}: int64 indices expected, got {x.dtype}")


# inference only: the codebooks are buffers
class VQ(nn.Module):
    def __init__(self, dim: int, codebook_size: int) -> None:
        super().__init__()
        self.register_buffer("embed", torch.zeros(codebook_size, dim))
        self.embed: Tensor

    def _books(self) -> tuple[Tensor, Tensor]:
        e = self.embed
        return (derived(self, "book", (e,), lambda: e.detach()[None].contiguous()),
                derived(self, "norm", (e,), lambda: e.detach().square().sum(-1)[None].contiguous()))

    def quantize(self, x: Tensor) -> Tensor:
        """(..., dim) -> the index of the nearest entry (squared distance; the lowest index on ties)."""
        if _placement(x, self.embed):
            distances = x.square().sum(-1, keepdim=True) - 2 * x @ self.embed.T + self.embed.square().sum(-1)
            return distances.argmin(-1)
        _check_rows(x, self.embed, "VQ.quantize")
        books, norms = self._books()
        return ops.rvq_encode(x.reshape(-1, x.shape[-1]).contiguous(), books, norms, 1)[0].view(x.shape[:-1])

    def dequantize(self, x: Tensor) -> Tensor:
        if _placement(x, self.embed):
            return F.embedding(x, self.embed)
        _check_codes(x, "VQ.dequantize")
        return ops.rvq_decode(x.reshape(1, 1, -1), self._books()[0]).view(*x.shape, self.embed.shape[1])


class RVQ(nn.ModuleList):
    def __init__(self, dim: int, codebook_size: int, n_quantizers: int) -> None:
        super().__init__([VQ(dim, codebook_size) for _ in range(n_quantizers)])

    def _books(self) -> tuple[Tensor, Tensor]:
        es = tuple(vq.embed for vq in self)
        return (derived(self, "books", es, lambda: torch.stack([e.detach() for e in es]).contiguous()),
                derived(self, "norms", es, lambda: torch.stack([e.detach().square().sum(-1) for e in es]).contiguous()))

    def quantize(self, x: Tensor, n_quantizers: int | None = None) -> Tensor:
        """(B, T, dim) -> indices (n_quantizers, B, T): each stage quantizes what the stages before it left."""
        n_quantizers = n_quantizers or len(self)
        if not 1 <= n_quantizers <= len(self):
            raise ValueError(f"RVQ: n_quantizers must be in 1..{len(self)}, got {n_quantizers}")
        if _placement(x, self[0].embed):
            all_indices = []
            for vq in list(self)[:n_quantizers]:
                indices = vq.quantize(x)
                x = x - vq.dequantize(indices)
                all_indices.append(indices)
            return torch.stack(all_indices, 0)
        _check_rows(x, self[0].embed, "RVQ.quantize")
        books, norms = self._books()
        return ops.rvq_encode(x.reshape(-1, x.shape[-1]).contiguous(), books, norms, n_quantizers).view(n_quantizers, *x.shape[:-1])

    def dequantize(self, x: Tensor) -> Tensor:
        """indices (n_q, B, T) -> the sum of the chosen entries (B, T, dim)."""
        if _placement(x, self[0].embed):
            out = self[0].dequantize(x[0])
            for i in range(1, x.shape[0]):
                out = out + self[i].dequantize(x[i])
            return out
        _check_codes(x, "RVQ.dequantize")
        if x.dim() != 3 or not 1 <= x.shape[0] <= len(self):
            raise ValueError(f"RVQ.dequantize: expected (n_q <= {len(self)}, B, T) indices, got {tuple(x.shape)}")
        return ops.rvq_decode(x.permute(1, 0, 2), self._books()[0])


class EnCodec(nn.Module):
    def __init__(self, audio_channels: int, norm_type: str, causal: bool, n_quantizers: int, normalize: bool) -> None:
        super().__init__()
        self.encoder = EnCodecEncoder(audio_channels, norm_type=norm_type, causal=causal)
        self.decoder = EnCodecDecoder(audio_channels, norm_type=norm_type, causal=causal)
        self.quantizer = RVQ(128, 1024, n_quantizers)
        self.normalize = normalize

    def encode_checkpoints(self, x: Tensor, n_quantizers: int | None = None, keep_layers: bool = True) -> dict[str, Tensor]:
        """HIP path of ``encode`` with the intermediates kept: every encoder child's output under its index (time-major), "latent"
        (B, T, 128) time-major, "codes" (B, n_q, T) and "scale" (None without ``normalize``).  ``keep_layers=False`` (what
        ``encode`` passes) keeps no layer output alive: at 32 clips x 10 s the first layers are about 1 GB each."""
        p = _weight_params(self.encoder[0].conv)[0]
        if _placement(x, p):
            raise ValueError("EnCodec.encode_checkpoints is the HIP path; a CPU module runs encode()")
        _gate(self, x, p, "EnCodec.encode", _stack_channels(self.encoder))
        n_q = n_quantizers or len(self.quantizer)
        if not 1 <= n_q <= len(self.quantizer):
            raise ValueError(f"EnCodec.encode: n_quantizers must be in 1..{len(self.quantizer)}, got {n_quantizers}")
        x = x.contiguous()
        ck: dict = {}
        scale = ops.encodec_scale(x) if self.normalize else None
        h = _to_tm(x)
        if scale is not None:
            h = ops.scale_clips(h, scale, divide=True)
        z = self.encoder.run_tm(h, ck if keep_layers else None)
        del h
        ck["latent"] = z
        ck["codes"] = self.quantizer.quantize(z, n_q).transpose(0, 1)
        ck["scale"] = scale
        return ck

    def encode(self, x: Tensor, n_quantizers: int | None = None) -> tuple[Tensor, Tensor | None]:
        """(B, audio_channels, T) -> (codes (B, n_quantizers, T / 320), scale (B, 1, 1) or None)."""
        if _placement(x, _weight_params(self.encoder[0].conv)[0]):
            if self.normalize:  # the 48 kHz variant: clips are brought to unit RMS of their mono mix
                scale = x.mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8
                x = x / scale
            else:
                scale = None
            z = self.encoder(x)
            return self.quantizer.quantize(z.transpose(1, 2), n_quantizers).transpose(0, 1), scale
        ck = self.encode_checkpoints(x, n_quantizers, keep_layers=False)
        return ck["codes"], ck["scale"]

    def decode_checkpoints(self, x: Tensor, scale: Tensor | None = None, keep_layers: bool = True) -> dict[str, Tensor]:
        """HIP path of ``decode`` with the intermediates kept: "quantized" (B, T, 128) and every decoder child's output under its
        index, time-major; "out" (B, audio_channels, T * 320).  ``keep_layers=False`` (what ``decode`` passes) keeps only "out"."""
        p = _weight_params(self.decoder[0].conv)[0]
        if _placement(x, p):
            raise ValueError("EnCodec.decode_checkpoints is the HIP path; a CPU module runs decode()")
        if p.dtype != torch.float32:
            raise NotImplementedError(f"EnCodec.decode: fp32 parameters only on a HIP device (got {p.dtype})")
        if self.training:
            raise NotImplementedError("EnCodec.decode: inference only on a HIP device (call .eval())")
        _check_codes(x, "EnCodec.decode")
        if x.dim() != 3 or not 1 <= x.shape[1] <= len(self.quantizer) or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"EnCodec.decode: expected (B, n_q <= {len(self.quantizer)}, T) indices, neither B nor T empty, got {tuple(x.shape)}")
        if scale is not None:
            try:
                ops.check_devices(x, scale)
            except RuntimeError as e:
                raise ValueError(str(e)) from None
            if scale.dtype != torch.float32 or scale.numel() != x.shape[0]:
                raise ValueError("EnCodec.decode: scale must be fp32 with one value per clip")
        ck: dict = {}
        q = self.quantizer.dequantize(x.transpose(0, 1))
        if keep_layers:
            ck["quantized"] = q
        y = _from_tm(self.decoder.run_tm(q, ck if keep_layers else None).contiguous())
        del q
        ck["out"] = y if scale is None else ops.scale_clips(y, scale.contiguous(), divide=False)
        return ck

    def decode(self, x: Tensor, scale: Tensor | None = None) -> Tensor:
        """codes (B, n_q, T) [, scale] -> (B, audio_channels, T * 320)."""
        if _placement(x, _weight_params(self.decoder[0].conv)[0]):
            y = self.decoder(self.quantizer.dequantize(x.transpose(0, 1)).transpose(1, 2))
            return y if scale is None else y * scale
        return self.decode_checkpoints(x, scale, keep_layers=False)["out"]

    @staticmethod
    def from_facebook(variant: str, pretrained: bool = False) -> "EnCodec":
        """"24khz" (mono, causal, weight norm, 32 codebooks) or "48khz" (stereo, GroupNorm over time, 16 codebooks, normalised)."""
        audio_channels, norm_type, causal, n_quantizers, normalize = {
            "24khz": (1, "weight_norm", True, 32, False),
            "48khz": (2, "time_group_norm", False, 16, True),
        }[variant]
        m = EnCodec(audio_channels, norm_type, causal, n_quantizers, normalize)
        if pretrained:
            ckpt = {"24khz": "encodec_24khz-d7cc33bc.th", "48khz": "encodec_48khz-7e698e3e.th"}[variant]
            state_dict = torch.hub.load_state_dict_from_url("https://dl.fbaipublicfiles.com/encodec/v0/" + ckpt)
            m.load_facebook_state_dict(state_dict)
        return m

    def load_facebook_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        # strict=False: upstream's codebooks carry training statistics (cluster sizes, running sums) that inference does not need
        self.load_state_dict({_rename_key(k): v for k, v in state_dict.items()}, strict=False)


_UPSTREAM_TO_LOCAL = (
    ("model.", ""),
    ("conv.conv.", "conv."),
    ("conv.norm.", "norm."),
    ("convtr.convtr.", "conv."),
    ("convtr.norm.", "norm."),
    ("block.", "layers."),
    ("lstm.", ""),
    ("vq.layers.", ""),
    ("_codebook.", ""),
)


def _rename_key(key: str) -> str:
    """facebookresearch/encodec state-dict key -> this module tree's key (applied in order)."""
    for old, new in _UPSTREAM_TO_LOCAL:
        key = key.replace(old, new)
    return key
