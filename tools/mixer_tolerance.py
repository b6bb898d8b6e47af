"""End-to-end bf16 tolerance of MLP-Mixer's HIP form, derived on the CPU (no GPU, no kernel): this package's CPU form run with
every tensor the HIP form STORES rounded to bf16 - the patch-embed rows, LayerNorm outputs (the normalised slab in LDS, norm2's
rows), both hidden activations, the residual stream after each half of a layer, the features - against the unrounded CPU form on
the same bf16-rounded weights, rel-L2 per checkpoint.  Accumulation stays fp32, as on the MFMA.  tests/test_hip_mixer.py allows
2 x these figures (other summation order, polynomial GELU, statistics of the rounded stream); DESIGN.md section 13 quotes them.

    python tools/mixer_tolerance.py            # the four models of tests/test_hip_mixer.py
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-models_amd"))
from pytorch_models.image import MLPMixer  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)
SEED = 141
CASES = (("S/16", 64, 2), ("S/32", 224, 1), ("S/16", 224, 2), ("B/16", 224, 2))


def r(t):
    return t.to(torch.bfloat16).float()


def ident(t):
    return t


def walk(m, x, q):
    """The model's five checkpoints with ``q`` applied wherever the HIP form stores a tensor (q = ident: the plain CPU form)."""
    out = {}
    h = q(F.conv2d(x, m.patch_embed.weight, m.patch_embed.bias, stride=m.patch_embed.stride).flatten(2).transpose(1, 2))
    out["tokens"] = h
    for i, l in enumerate(m.layers):
        tm, cm = l.token_mixing, l.channel_mixing
        n = q(l.norm1(h)).transpose(-1, -2)
        u = q(F.gelu(F.linear(n, tm.linear1.weight, tm.linear1.bias)))
        h = q(h + F.linear(u, tm.linear2.weight, tm.linear2.bias).transpose(-1, -2))
        if i == 0:
            out["mix0"] = h
        u = q(F.gelu(F.linear(q(l.norm2(h)), cm.linear1.weight, cm.linear1.bias)))
        h = q(h + F.linear(u, cm.linear2.weight, cm.linear2.bias))
        if i == 0:
            out["layer0"] = h
    out["last"] = h
    out["out"] = q(m.norm(h).mean(1))
    return out


def build(tag, img, batch):
    m = MLPMixer.from_google(tag, img_size=img).eval()
    fill_module(m, SEED)
    bf16_round_(m)
    return m, synth_input(f"mixer_x{img}", (batch, 3, img, img), SEED)


if __name__ == "__main__":
    for tag, img, batch in CASES:
        m, x = build(tag, img, batch)
        want, got = walk(m, x, ident), walk(m, x, r)
        torch.testing.assert_close(want["out"], m(x), rtol=1e-6, atol=1e-6)
        for k in want:
            print(f"{tag:5s} @{img:<4d} {k:7s} rel-L2 {float((got[k] - want[k]).norm() / want[k].norm()):.5f}")
