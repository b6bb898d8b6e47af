"""Generate the MLP-Mixer fixtures by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_mixer.py

* mixer.npz              S/16 at img_size 64 (T = 16; synthweights.fill_module, seed 141) on 2 x 3 x 64 x 64 images: the patch-embed
                         rows ("tokens"), the stream after layer 0's token mixing ("mix0"), after layer 0 ("layer0"), after the last
                         layer ("last") and the features ("out"); and the features alone of S/16 and B/16 at 224 (T = 196), batch 2;
* mixer_t49.npz          the same five checkpoints of S/32 at 224 (T = 49, no multiple of an MFMA K step), batch 1;
* mixer_geometry.json    state_dict key -> shape of S/16, S/32, B/16, B/32, L/16, H/14;
* mixer_converter.json   digests of what the reference's load_jax_weights makes of tests/ckpt_mixer.py's synthetic checkpoint (the
                         reference takes a path only, so the arrays go through a temporary .npz).
Conventions (save / digest, weights keyed by parameter name) as make_golden.py; only data is written."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))  # ckpt_mixer

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.image import MLPMixer  # noqa: E402

import ckpt_mixer as CK  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_convnext import state_digest  # noqa: E402
from synthweights import fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)
SEED = 141


def checkpoints(tag, img, batch, prefix=""):
    m = MLPMixer.from_google(tag, img_size=img).eval()
    fill_module(m, SEED)
    x = synth_input(f"mixer_x{img}", (batch, 3, img, img), SEED)
    out = {}
    h = m.patch_embed(x).flatten(2).transpose(1, 2)
    out["tokens"] = h
    for i, l in enumerate(m.layers):
        if i == 0:
            out["mix0"] = h + l.token_mixing(l.norm1(h).transpose(-1, -2)).transpose(-1, -2)
        h = l(h)
        if i == 0:
            out["layer0"] = h
    out["last"] = h
    out["out"] = m.norm(h).mean(1)
    torch.testing.assert_close(out["out"], m(x), rtol=0, atol=0)
    return {prefix + k: v.contiguous() for k, v in out.items()}


def g_outputs():
    out = checkpoints("S/16", 64, 2)
    out["s16_224_out"] = checkpoints("S/16", 224, 2)["out"]
    out["b16_224_out"] = checkpoints("B/16", 224, 2)["out"]
    save("mixer", dict(seed=SEED, input="mixer_x{img}", model="S/16 @ 64, batch 2; *_224_out: features at 224, batch 2"), **out)
    save("mixer_t49", dict(seed=SEED, input="mixer_x224", model="S/32 @ 224, batch 1"), **checkpoints("S/32", 224, 1))


def g_geometry_and_converter():
    geo, conv = {}, {}
    for tag in CK.VARIANTS:
        m = MLPMixer.from_google(tag)
        geo[tag] = {k: list(v.shape) for k, v in m.state_dict().items()}
    for tag in ("S/16", "S/32"):
        size, patch = tag.split("/")
        n_layers, d = CK.SIZES[size]
        m = MLPMixer.from_google(tag)
        ck = CK.flax_mixer(n_layers, d, int(patch), (224 // int(patch)) ** 2, seed=142)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "mixer.npz")
            np.savez(path, **ck)
            m.load_jax_weights(path)
        conv[tag] = state_digest(m.state_dict())
    for name, obj in (("mixer_geometry", geo), ("mixer_converter", conv)):
        with open(os.path.join(HERE, name + ".json"), "w") as f:  # one line per variant
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(obj[k], sort_keys=True)}" for k in sorted(obj)) + "\n}\n")


if __name__ == "__main__":
    g_outputs()
    g_geometry_and_converter()
