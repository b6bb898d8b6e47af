"""Generate the ConvNeXt fixtures by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_convnext.py

* convnext.npz             atto and tiny (synthweights.fill_module, seed 71) on 2 x 3 x 64 x 64 images: the stem output, each
                           stage's output (NHWC) and the features;
* convnext_geometry.json   state_dict key -> shape of all ten `from_facebook` variants;
* convnext_converter.json  digests of what the reference's load_facebook_state_dict makes of tests/ckpt_convnext.py's
                           synthetic checkpoint (with stray `head.*` keys, which the loader ignores).
Conventions (save / digest, weights keyed by parameter name) as make_golden.py; only data is written."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))  # ckpt_convnext

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.image import ConvNeXt  # noqa: E402

import ckpt_convnext as CK  # noqa: E402
from make_golden import save  # noqa: E402
from synthweights import fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)


def state_digest(sd) -> dict:
    out = {}
    for k, v in sd.items():
        f = v.detach().double().flatten()
        w = 1.0 + (torch.arange(f.numel(), dtype=torch.float64) % 251) / 251.0
        out[k] = [f.sum().item(), f.abs().sum().item(), (f * w).sum().item()]
    return out


def g_outputs():
    out = {}
    x = synth_input("cnx_x", (2, 3, 64, 64), 71)
    for variant in ("atto", "tiny"):
        m = ConvNeXt.from_facebook(variant).eval()
        fill_module(m, 71)
        h = m.stem(x)
        out[f"{variant}_stem"] = h
        for i, stage in enumerate(m.stages):
            h = stage(h)
            out[f"{variant}_stage{i}"] = h
        out[f"{variant}_out"] = m.norm(m.pool(h))
        torch.testing.assert_close(out[f"{variant}_out"], m(x), rtol=0, atol=0)
    save("convnext", dict(img=64, seed=71, input="cnx_x"), **out)


def g_geometry_and_converter():
    geo, conv = {}, {}
    for variant, (d, depths) in CK.VARIANTS.items():
        m = ConvNeXt.from_facebook(variant)
        geo[variant] = {k: list(v.shape) for k, v in m.state_dict().items()}
        if variant in ("atto", "tiny"):
            m.load_facebook_state_dict(CK.facebook_convnext(d, depths, seed=72))
            conv[variant] = state_digest(m.state_dict())
    for name, obj in (("convnext_geometry", geo), ("convnext_converter", conv)):
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(obj, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    g_outputs()
    g_geometry_and_converter()
