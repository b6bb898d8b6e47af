"""Synthetic EnCodec weights, inputs and checkpoints shared by tests/golden/make_golden_encodec.py (which imports the reference)
and the tests (which import this package): both sides run the same plain-torch statements on the same synthetic tensors.

`fill(m, seed, gain)` is `synthweights.fill_module` plus two corrections it does not know:
* every weight-norm gain `original0` becomes `gain * |v|` per output channel, i.e. an effective weight of `gain * v` (left at
  N(0, 0.1) the signal dies within a few layers and the output is bias only);
* for a whole EnCodec, codebook i is rescaled to a standard deviation of 0.5 * 0.85**i times that of the latent of `calib_clip`, and
  codebook 0 gets the latent's per-channel mean added, so that the residual norm falls from stage to stage and more than a
  handful of entries are used.
`clip` makes noise with an amplitude envelope and a level per clip.  `facebook_state_dict` is a synthetic checkpoint under the
upstream (facebookresearch/encodec) key names - `model.N.conv.conv.*`, `convtr.convtr`, `block.`, `lstm.`, the old-style
`weight_g` / `weight_v` of torch.nn.utils.weight_norm, `vq.layers.N._codebook.embed` - with the training statistics of the
codebooks that the loader drops.  `cpu_checkpoints` walks a CPU model through every layer."""
import math

import torch
from torch import nn

from synthweights import fill_module, synth_input, synth_tensor

VARIANTS = ("24khz", "48khz")
CHANNELS = {"24khz": 1, "48khz": 2}
GAIN = {"24khz": 0.8, "48khz": 1.0}
SEED = 151
HOP = 320  # samples per latent frame: 2 * 4 * 5 * 8
# (tag, samples): the reference tests' shape, a length that is no multiple of 320 (the extra padding), 75 LSTM steps
LENGTHS = {"24khz": (("a", 3200), ("b", 3000), ("c", 24000)), "48khz": (("a", 3200), ("b", 3000), ("c", 12800))}
LAYER_CLIP = 2240  # the clip of encodec_layers.npz: 7 frames (the shortest the last convolution's reflect padding of 6 admits), batch 1


def clip(tag: str, batch: int, channels: int, samples: int, seed: int = SEED) -> torch.Tensor:
    """Noise of standard deviation 0.3 under a slow amplitude envelope, each clip of the batch at its own level."""
    x = synth_input("encodec:" + tag, (batch, channels, samples), seed, scale=0.3)
    t = torch.arange(samples, dtype=torch.float32)
    b = torch.arange(batch, dtype=torch.float32)[:, None, None]
    env = 0.6 + 0.4 * torch.sin(2 * math.pi * t / 2400.0 + 1.3 * b)
    return x * env / (1.0 + 0.5 * b)


def calib_clip(channels: int, seed: int = SEED) -> torch.Tensor:
    return clip("calib", 4, channels, 9600, seed)


@torch.no_grad()
def fill(m: nn.Module, seed: int = SEED, gain: float = 0.8) -> None:
    fill_module(m, seed)
    for mod in m.modules():
        if isinstance(mod, (nn.Conv1d, nn.ConvTranspose1d)) and nn.utils.parametrize.is_parametrized(mod, "weight"):
            p = mod.parametrizations.weight
            v = p.original1
            p.original0.copy_(gain * v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))
    if hasattr(m, "quantizer") and hasattr(m, "encoder"):
        was_training = m.training
        m.eval()
        x = calib_clip(next(iter(m.encoder.children())).conv.in_channels, seed)
        if m.normalize:
            x = x / (x.mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8)
        z = m.encoder(x).transpose(1, 2).reshape(-1, 128)
        std, mean = z.std(), z.mean(0)
        for i, vq in enumerate(m.quantizer):
            vq.embed.copy_(vq.embed / vq.embed.std() * (0.5 * 0.85**i) * std)
        m.quantizer[0].embed.add_(mean)
        m.train(was_training)


def _leaf(parts) -> str:
    s = ".".join(parts)
    return s.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")


def _conv_key(conv_mod: nn.Module, parts) -> str:
    """`conv.<leaf>` / `norm.<leaf>` of a Conv1d / ConvTranspose1d wrapper -> upstream's doubled names."""
    name = "convtr" if isinstance(conv_mod.conv, nn.ConvTranspose1d) else "conv"
    inner = name if parts[0] == "conv" else "norm"
    return f"{name}.{inner}.{_leaf(parts[1:])}"


def _stack_key(stack: nn.Module, parts) -> str:
    child = stack[int(parts[0])]
    head = f"model.{parts[0]}."
    kind = type(child).__name__
    if kind in ("Conv1d", "ConvTranspose1d"):
        return head + _conv_key(child, parts[1:])
    if kind == "LSTM":
        return head + "lstm." + ".".join(parts[1:])
    if kind == "EnCodecBlock":
        if parts[1] == "layers":
            return head + f"block.{parts[2]}." + _conv_key(child.layers[int(parts[2])], parts[3:])
        return head + "shortcut." + _conv_key(child.shortcut, parts[2:])
    raise KeyError(parts)


def upstream_key(m: nn.Module, key: str) -> str:
    parts = key.split(".")
    if hasattr(m, "quantizer"):
        if parts[0] == "quantizer":
            return f"quantizer.vq.layers.{parts[1]}._codebook.{parts[2]}"
        return parts[0] + "." + _stack_key(getattr(m, parts[0]), parts[1:])
    return _stack_key(m, parts)


def facebook_state_dict(m: nn.Module, seed: int = SEED + 1) -> dict:
    """A checkpoint for ``m`` (EnCodec, EnCodecEncoder or EnCodecDecoder of either package) under upstream's key names."""
    sd = {}
    for k, v in m.state_dict().items():
        up = upstream_key(m, k)
        sd[up] = synth_tensor("ckpt:" + up, v.shape, seed)
    if hasattr(m, "quantizer"):  # what upstream's EuclideanCodebook keeps for training; the loader drops them
        for i, vq in enumerate(m.quantizer):
            base = f"quantizer.vq.layers.{i}._codebook."
            sd[base + "inited"] = torch.ones(1)
            sd[base + "cluster_size"] = synth_tensor("ckpt:" + base + "cluster_size", (vq.embed.shape[0],), seed)
            sd[base + "embed_avg"] = synth_tensor("ckpt:" + base + "embed_avg", vq.embed.shape, seed)
    return sd


def _walk(stack: nn.Module, x: torch.Tensor, prefix: str, out: dict) -> torch.Tensor:
    """Every child of an encoder / decoder in plain torch, outputs kept as (B, C, T) under prefix + index (ELUs are not kept: the
    HIP path folds them into the next convolution)."""
    for name, child in stack.named_children():
        x = child(x)
        if not isinstance(child, nn.ELU):
            out[prefix + name] = x
    return x


@torch.no_grad()
def cpu_checkpoints(m: nn.Module, x: torch.Tensor, n_quantizers=None) -> dict:
    """enc.<i> / dec.<i> for every layer, latent (B, 128, T), codes, codes_q (the first n_quantizers), scale (or None), quantized
    (B, 128, T) and wave = decode(codes, scale) of a CPU EnCodec, in plain torch on its parameters."""
    out = {}
    if m.normalize:
        scale = x.mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8
        h = x / scale
    else:
        scale, h = None, x
    z = _walk(m.encoder, h, "enc.", out)
    out["latent"] = z
    codes = m.quantizer.quantize(z.transpose(1, 2)).transpose(0, 1)
    out["codes"] = codes
    if n_quantizers is not None:
        out["codes_q"] = m.quantizer.quantize(z.transpose(1, 2), n_quantizers).transpose(0, 1)
    out["scale"] = scale
    q = m.quantizer.dequantize(codes.transpose(0, 1)).transpose(1, 2)
    out["quantized"] = q
    y = _walk(m.decoder, q, "dec.", out)
    out["wave"] = y if scale is None else y * scale
    return out
