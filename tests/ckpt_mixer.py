"""Synthetic google-research/vision_transformer MLP-Mixer checkpoint (the arrays of Mixer-*.npz; reference loader:
pytorch_models/image/mlp_mixer.py, load_jax_weights), built from geometry with values from synthweights.synth_tensor keyed by the
upstream key, so the golden generator (reference loader) and the tests (this package's loader) read identical inputs.  Flax
layouts: Conv kernel (P, P, 3, d), Dense kernel (in, out), LayerNorm scale / bias.  It carries the classifier `head/*` that the
loader leaves unread.  `cpu_checkpoints` walks a CPU model through the five checkpoints the fixtures hold."""
import torch.nn.functional as F

from synthweights import synth_tensor

SIZES = dict(S=(8, 512), B=(12, 768), L=(24, 1024), H=(32, 1280))
VARIANTS = ("S/16", "S/32", "B/16", "B/32", "L/16", "H/14")


def flax_mixer(n_layers, d_model, patch, n_tokens, mlp_ratio=(0.5, 4.0), n_classes=11, seed=0):
    ck = {}

    def put(k, shape):
        ck[k] = synth_tensor("ckpt:" + k, shape, seed).numpy()

    def dense(prefix, n_in, n_out):
        put(f"{prefix}/kernel", (n_in, n_out))
        put(f"{prefix}/bias", (n_out,))

    def ln(prefix):
        put(f"{prefix}/scale", (d_model,))
        put(f"{prefix}/bias", (d_model,))

    dt, dc = int(d_model * mlp_ratio[0]), int(d_model * mlp_ratio[1])
    put("stem/kernel", (patch, patch, 3, d_model))
    put("stem/bias", (d_model,))
    for i in range(n_layers):
        p = f"MixerBlock_{i}"
        ln(f"{p}/LayerNorm_0")
        dense(f"{p}/token_mixing/Dense_0", n_tokens, dt)
        dense(f"{p}/token_mixing/Dense_1", dt, n_tokens)
        ln(f"{p}/LayerNorm_1")
        dense(f"{p}/channel_mixing/Dense_0", d_model, dc)
        dense(f"{p}/channel_mixing/Dense_1", dc, d_model)
    ln("pre_head_layer_norm")
    dense("head", d_model, n_classes)
    return ck


def cpu_checkpoints(m, x):
    """tokens, mix0 (after layer 0's token mixing), layer0, last, out of a CPU MLPMixer, in plain torch on its parameters."""
    out = {}
    h = F.conv2d(x, m.patch_embed.weight, m.patch_embed.bias, stride=m.patch_embed.stride).flatten(2).transpose(1, 2)
    out["tokens"] = h
    for i, l in enumerate(m.layers):
        if i == 0:
            out["mix0"] = h + l.token_mixing(l.norm1(h).transpose(-1, -2)).transpose(-1, -2)
        h = l(h)
        if i == 0:
            out["layer0"] = h
    out["last"] = h
    out["out"] = m(x)
    return out
