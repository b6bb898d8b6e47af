"""MLP-Mixer (https://arxiv.org/abs/2105.01601) on the MI355X kernels: drop-in for the reference's pytorch_models/image/mlp_mixer.py
(same classes, constructor arguments and defaults, child names `patch_embed`, `layers`, `norm`; `norm1`, `token_mixing`, `norm2`,
`channel_mixing`; the `from_google` tag grammar and the `load_jax_weights` key map), so a reference state_dict loads unchanged.

Execution on HIP tensors (eval forward; no autograd), precision following the parameters:

bf16 parameters - the residual stream is bf16 (N, T, C) rows, as ViT's:
* patch embedding is `pm_vit_tokens` / `pm_vit_tokens_generic` with a zero position table and no class token;
* token mixing, `x + token_mixing(norm1(x)^T)^T`, is ONE kernel, `pm_mixer_token_mix_bf16` (csrc/mixer.hip): it needs the (mean, rstd)
  of every row of x, because a workgroup owns only a slab of channels;
* the FOLDED route (`route() == "fold"`, shapes the persistent GEMMs serve: `pm_linear_ln_supported`): the token-mixing kernel
  emits the partial row statistics of its output, `norm2` is folded into channel mixing's fc1, and fc2's epilogue emits the
  statistics the next layer's token mixing (or the head) reads.  A layer is token-mix, finalize, fc1, fc2, finalize;
* the PLAIN route (small batches, widths the fold does not serve): `pm_row_stats` -> token-mix -> `pm_layernorm` -> fc1 -> fc2;
* the head, `norm` then the mean over tokens, is `pm_ln_mean` on the rows' statistics.
Both routes are the HIP path; there is no fallback: a geometry outside the served set raises a ValueError naming the limit.

fp32 parameters - composed from the fp32 kernels (off the benchmark path): `pm_layernorm`, `pm_transpose_add_f32`, `pm_linear_f32`
twice, `pm_transpose_add_f32` with the residual; channel mixing is `MLP.run`'s fp32 branch.

On the CPU (module AND input there) the modules run the reference's arithmetic in plain torch.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import MLP, LayerNorm, _f32, _fold_ln, derived
from .vit import _no_download, load_flax_conv2d, load_flax_linear, load_flax_ln

_SIZES = dict(S=(8, 512), B=(12, 768), L=(24, 1024), H=(32, 1280))  # Table 1 of the paper: (layers, d_model)


# (loader, submodule of a MixerBlock, key under "MixerBlock_{i}/") of a vision_transformer Mixer checkpoint
_FLAX_BLOCK_KEYS = (
    (load_flax_ln, "norm1", "LayerNorm_0"),
    (load_flax_ln, "norm2", "LayerNorm_1"),
    (load_flax_linear, "token_mixing.linear1", "token_mixing/Dense_0"),
    (load_flax_linear, "token_mixing.linear2", "token_mixing/Dense_1"),
    (load_flax_linear, "channel_mixing.linear1", "channel_mixing/Dense_0"),
    (load_flax_linear, "channel_mixing.linear2", "channel_mixing/Dense_1"),
)


def _placement(x: Tensor, p: Tensor) -> bool:
    """True: input and parameters on the CPU (the plain-torch form); False: both on the current HIP device.  Any other placement
    is a ValueError carrying the shared guards' message (_cpu.on_cpu, ops.check_devices)."""
    try:
        if _cpu.on_cpu(x, p):
            return True
        ops.check_devices(x, p)
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return False


def _refuse_training(m: MLP, who: str) -> None:
    if m.training and m.dropout.p > 0.0:
        raise NotImplementedError(f"{who}: inference only (dropout is not implemented)")


class MixerBlock(nn.Module):
    def __init__(
        self,
        n_tokens: int,
        d_model: int,
        mlp_ratio: tuple[float, float] = (0.5, 4.0),
        dropout: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__()
        # both hidden widths are fractions of d_model (the token-mixing one too: it does not depend on n_tokens)
        token_hidden, channel_hidden = int(d_model * mlp_ratio[0]), int(d_model * mlp_ratio[1])
        self.norm1 = LayerNorm(d_model, norm_eps)
        self.token_mixing = MLP(n_tokens, token_hidden, dropout)
        self.norm2 = LayerNorm(d_model, norm_eps)
        self.channel_mixing = MLP(d_model, channel_hidden, dropout)

    # ---- geometry the bf16 kernels serve
    def check_served(self) -> None:
        tm = self.token_mixing
        T, Dt, C = tm.linear1.in_features, tm.linear1.out_features, self.norm1.normalized_shape[0]
        if C % 64 or Dt % 32 or self.channel_mixing.linear1.out_features % 64:
            raise ValueError(f"MixerBlock: the HIP kernels need d_model % 64 == 0, a token-mixing width % 32 == 0 and a channel-mixing "
                             f"width % 64 == 0 (got d_model={C}, {Dt}, {self.channel_mixing.linear1.out_features})")
        if not ops.mixer_token_mix_supported(T, Dt, C):
            raise ValueError(f"MixerBlock: {T} tokens with a token-mixing width of {Dt} are not served: 64 channels of the normalised "
                             "tokens and of the hidden activations, 128 * (T rounded up to 16 + width + 16) bytes, must fit the 160 KiB LDS")

    def _token_operands(self):
        """Derived operands of pm_mixer_token_mix_bf16: W1 and W2 fragment-major (zero-padded to the MFMA tile) and the f32 vectors."""
        l1, l2 = self.token_mixing.linear1, self.token_mixing.linear2
        w1f = derived(self, "mixer_w1f", (l1.weight,), lambda: ops.mixer_pack_weight(l1.weight))
        w2f = derived(self, "mixer_w2f", (l2.weight,), lambda: ops.mixer_pack_weight(l2.weight))
        return (_f32(self.norm1, "g", self.norm1.weight), _f32(self.norm1, "b", self.norm1.bias), w1f, _f32(l1, "b", l1.bias),
                w2f, _f32(l2, "b", l2.bias))

    def fold_ok(self, M: int) -> bool:
        """True when norm2 can be folded into channel mixing and fc2 can emit the next rows' statistics (M = images x tokens)."""
        cm = self.channel_mixing
        C, hid = cm.linear1.in_features, cm.linear1.out_features
        return (type(cm).forward is MLP.forward and cm.act_name == "gelu" and cm.linear1.weight.dtype == torch.bfloat16
                and ops.linear_ln_supported(M, C, hid, "none", True) and ops.linear_ln_supported(M, hid, C, "gelu", False))

    def run_bf16(self, x: Tensor, stats: Tensor | None, fold: bool, next_eps: float | None, keep: dict | None = None):
        """x bf16 (N, T, C) -> (block(x), statistics of its rows under ``next_eps`` or None).  ``stats``: (mean, rstd) of the rows
        of x under norm1 (None: pm_row_stats computes them).  ``keep``: a dict that receives the stream after token mixing."""
        N, T, C = x.shape
        if T != self.token_mixing.linear1.in_features:
            raise ValueError(f"MixerBlock: built for {self.token_mixing.linear1.in_features} tokens, got {T}")
        _refuse_training(self.token_mixing, "MixerBlock")
        _refuse_training(self.channel_mixing, "MixerBlock")
        g1, be1, w1f, b1, w2f, b2 = self._token_operands()
        if stats is None:
            stats = ops.row_stats(x.view(N * T, C), self.norm1.eps)
        cm, n2 = self.channel_mixing, self.norm2
        if not fold:
            y = ops.mixer_token_mix(x, stats, g1, be1, w1f, b1, w2f, b2).view(N * T, C)
            if keep is not None:
                keep["mix0"] = y.view(N, T, C)
            t = ops.layernorm(y, _f32(n2, "g", n2.weight), _f32(n2, "b", n2.bias), n2.eps)
            return cm.run(t, residual=y).view(N, T, C), None
        y, rows = ops.mixer_token_mix(x, stats, g1, be1, w1f, b1, w2f, b2, want_row_stats=True)
        y = y.view(N * T, C)
        if keep is not None:
            keep["mix0"] = y.view(N, T, C)
        st = ops.ln_stats_finalize(rows, C, n2.eps)
        l1, l2 = cm.linear1, cm.linear2
        wl, s, c = derived(cm, "l1_ln", (l1.weight, l1.bias, n2.weight, n2.bias), lambda: _fold_ln(l1.weight, l1.bias, n2))
        h = ops.linear(y, wl, c, act=cm.act_name, ln_stats=st, ln_s=s)
        if next_eps is None:
            return ops.linear(h, l2.weight, _f32(l2, "b", l2.bias), resid=y).view(N, T, C), None
        z, rows = ops.linear(h, l2.weight, _f32(l2, "b", l2.bias), resid=y, want_row_stats=True)
        return z.view(N, T, C), ops.ln_stats_finalize(rows, C, next_eps)

    def run_f32(self, x: Tensor, keep: dict | None = None) -> Tensor:
        """x f32 (N, T, C) -> block(x) in fp32 arithmetic, composed from the fp32 kernels."""
        N, T, C = x.shape
        tm, n1, n2 = self.token_mixing, self.norm1, self.norm2
        if T != tm.linear1.in_features:
            raise ValueError(f"MixerBlock: built for {tm.linear1.in_features} tokens, got {T}")
        _refuse_training(tm, "MixerBlock")
        T4 = -(-T // 4) * 4  # pm_linear_f32 wants 16-byte rows: the transposed tokens and W1 get a row stride of T4 (K stays T)

        def pad_w1():
            w = torch.zeros((tm.linear1.out_features, T4), dtype=torch.float32, device=x.device)
            w[:, :T] = tm.linear1.weight.detach()
            return w

        w1 = derived(self, "mixer_w1_f32", (tm.linear1.weight,), pad_w1)[:, :T]
        xn = ops.layernorm(x.view(N * T, C), _f32(n1, "g", n1.weight), _f32(n1, "b", n1.bias), n1.eps).view(N, T, C)
        xt = ops.transpose_add_f32(xn, ldy=T4)  # (N, C, T) with row stride T4
        h = ops.linear_f32(xt, w1, tm.linear1.bias, act=tm.act_name, M=N * C, K=T, row_stride=T4)
        u = ops.linear_f32(h, tm.linear2.weight, tm.linear2.bias)  # (N*C, T)
        y = ops.transpose_add_f32(u.view(N, C, T), resid=x).reshape(N * T, C)
        if keep is not None:
            keep["mix0"] = y.view(N, T, C)
        t = ops.layernorm(y, _f32(n2, "g", n2.weight), _f32(n2, "b", n2.bias), n2.eps)
        return self.channel_mixing.run(t, residual=y).view(N, T, C)

    def forward(self, x: Tensor) -> Tensor:
        """(N, n_tokens, d_model) in and out."""
        p = self.norm1.weight
        if _placement(x, p):  # CPU: the MLP over the token axis of the normalised rows, then the MLP over the channels
            mixed = self.token_mixing(self.norm1(x).mT).mT
            x = x + mixed
            return x + self.channel_mixing(self.norm2(x))
        if x.dim() != 3:
            raise ValueError(f"MixerBlock: expected (N, n_tokens, d_model), got {tuple(x.shape)}")
        if p.dtype == torch.float32:
            return self.run_f32(x.float().contiguous())
        self.check_served()
        return self.run_bf16(x.to(torch.bfloat16).contiguous(), None, False, None)[0].to(x.dtype)


class MLPMixer(nn.Module):
    fold: bool | None = None  # None: the predicate decides (route()); False: always the plain route

    def __init__(
        self,
        n_layers: int,
        d_model: int,
        patch_size: int,
        img_size: int = 224,
        mlp_ratio: tuple[float, float] = (0.5, 4.0),
        dropout: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        if img_size % patch_size:
            raise AssertionError(f"MLPMixer: img_size {img_size} is not a multiple of patch_size {patch_size}")
        super().__init__()
        grid = img_size // patch_size
        self.patch_embed = nn.Conv2d(3, d_model, kernel_size=patch_size, stride=patch_size)
        blocks = [MixerBlock(grid * grid, d_model, mlp_ratio, dropout, norm_eps) for _ in range(n_layers)]
        self.layers = nn.Sequential(*blocks)
        self.norm = LayerNorm(d_model, norm_eps)

    # ---- HIP path
    def route(self, n_images: int) -> str:
        """"fold" or "plain": how a bf16 batch of ``n_images`` runs (see the module docstring)."""
        if self.fold is False or os.environ.get("PM_LN_FOLD", "1") == "0" or self.patch_embed.weight.dtype != torch.bfloat16:
            return "plain"
        layers = list(self.layers)
        M = n_images * layers[0].token_mixing.linear1.in_features if layers else 0
        return "fold" if layers and all(type(l).forward is MixerBlock.forward and l.fold_ok(M) for l in layers) else "plain"

    def tokens(self, imgs: Tensor) -> Tensor:
        """(N, 3, H, W) -> (N, T, C) rows in the parameters' dtype: Conv2d(3, d, P, P), flattened and transposed."""
        pw = self.patch_embed.weight
        d, _, P, _ = pw.shape
        N, _, H, W = imgs.shape
        if H % P or W % P:
            raise ValueError(f"MLPMixer: image sides must be multiples of the patch size {P}, got {tuple(imgs.shape[2:])}")
        T = (H // P) * (W // P)
        if pw.dtype == torch.float32:  # the patch projection as an fp32 GEMM over patch windows, as ViT's fp32 form
            cols = imgs.float().unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(N * T, 3 * P * P)
            return ops.linear_f32(cols, pw.view(d, -1), self.patch_embed.bias).view(N, T, d)
        if P == 16:
            w2d = pw.view(d, -1)
        else:  # other patch sizes: K = 3*P*P zero-padded to a multiple of 64 (derived copy)
            def pad():
                k = 3 * P * P
                w = torch.zeros(d, (k + 63) // 64 * 64, dtype=pw.dtype, device=pw.device)
                w[:, :k] = pw.detach().reshape(d, -1)
                return w

            w2d = derived(self, "w2d_pad", (pw,), pad)
        # Mixer has no position table: a cached zero one
        pe0 = derived(self, f"pe0_{T}", (pw,), lambda: torch.zeros((T, d), dtype=torch.float32, device=pw.device))
        return ops.vit_tokens(imgs.float().contiguous(), w2d, _f32(self, "pb", self.patch_embed.bias), pe0, None, P)

    def forward_checkpoints(self, imgs: Tensor) -> dict[str, Tensor]:
        """HIP path with the intermediate streams kept: "tokens", "mix0" (after layer 0's token mixing), "layer0", "last", "out"."""
        p = self.patch_embed.weight
        if _placement(imgs, p):
            raise ValueError("MLPMixer.forward_checkpoints is the HIP path; a CPU module runs forward()")
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"MLPMixer: expected (N, 3, H, W), got {tuple(imgs.shape)}")
        layers = list(self.layers)
        n_tok = (imgs.shape[2] // p.shape[2]) * (imgs.shape[3] // p.shape[3])
        if layers and n_tok != layers[0].token_mixing.linear1.in_features:
            raise ValueError(f"MLPMixer: built for {layers[0].token_mixing.linear1.in_features} tokens, the image has {n_tok} patches")
        if p.dtype not in (torch.bfloat16, torch.float32):
            raise NotImplementedError(f"MLPMixer: bf16 or fp32 parameters only (got {p.dtype})")
        if p.dtype == torch.bfloat16:
            for l in layers:
                l.check_served()
        x = self.tokens(imgs)
        N, T, C = x.shape
        ck = {"tokens": x}
        g, b = _f32(self.norm, "g", self.norm.weight), _f32(self.norm, "b", self.norm.bias)
        if p.dtype == torch.float32:
            for i, l in enumerate(layers):
                x = l(x) if type(l).forward is not MixerBlock.forward else l.run_f32(x, ck if i == 0 else None)
                if i == 0:
                    ck["layer0"] = x
            stats = ops.row_stats(x.reshape(N * T, C), self.norm.eps)
        else:
            fold = self.route(N) == "fold"
            stats = None
            for i, l in enumerate(layers):
                if type(l).forward is not MixerBlock.forward:  # a subclass with its own forward: call it
                    x, stats = l(x), None
                else:
                    nxt = (layers[i + 1].norm1.eps if i + 1 < len(layers) else self.norm.eps) if fold else None
                    x, stats = l.run_bf16(x, stats, fold, nxt, ck if i == 0 else None)
                if i == 0:
                    ck["layer0"] = x
            if stats is None:
                stats = ops.row_stats(x.reshape(N * T, C), self.norm.eps)
        ck["last"] = x
        ck["out"] = ops.ln_mean(x.contiguous(), stats, g, b, p.dtype)
        return ck

    def forward(self, x: Tensor) -> Tensor:
        if _placement(x, self.patch_embed.weight):
            pe = self.patch_embed  # CPU: patch rows, the blocks, the final norm, then the mean over the tokens
            rows = F.conv2d(x.to(pe.weight.dtype), pe.weight, pe.bias, stride=pe.stride).flatten(2).mT
            return self.norm(self.layers(rows)).mean(1)
        return self.forward_checkpoints(x)["out"]

    @staticmethod
    def from_google(model_tag: str, *, pretrained: bool = False, **kwargs) -> "MLPMixer":
        """"B/16", "L/16_imagenet21k", ... (default weights: gsam)."""
        tag, _, weights = model_tag.partition("_")
        if tag.count("/") != 1 or weights.count("_"):
            raise ValueError(f"MLPMixer.from_google: expected '<size>/<patch>[_<weights>]', got {model_tag!r}")
        size, patch = tag.split("/")
        weights = weights or "gsam"
        n_layers, d_model = _SIZES[size]
        m = MLPMixer(n_layers, d_model, int(patch), **kwargs)
        if pretrained:
            _no_download(f"MLPMixer.from_google ({weights} weights)")
        return m

    @torch.no_grad()
    def load_jax_weights(self, path) -> None:
        """google-research/vision_transformer Mixer ``.npz``: a local path or a mapping of its arrays (nothing is downloaded)."""
        from ..converters import _as_tensors

        w = _as_tensors(path)
        load_flax_conv2d(self.patch_embed, w, "stem")
        load_flax_ln(self.norm, w, "pre_head_layer_norm")
        for i, layer in enumerate(self.layers):
            for loader, module, key in _FLAX_BLOCK_KEYS:
                loader(layer.get_submodule(module), w, f"MixerBlock_{i}/{key}")
