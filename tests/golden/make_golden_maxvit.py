"""Generate the MaxViT fixtures by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_maxvit.py

* maxvit.npz             `small` = MaxViT(32, [1, 1, 2, 1], [32, 64, 96, 128]) and `tiny` (synthweights.fill_module, seed 91) on
                         2 x 3 x 224 x 224 images: the stem output and each stage's output (NHWC, pixels subsampled on a stride-7
                         / stride-4 lattice to keep the file small) and the features;
* maxvit_geometry.json   per `from_google` variant (all five): the number of state_dict keys, of parameters, and the sha256 of
                         the sorted "key shape" lines (geometry_digest below; tests/test_maxvit_cpu.py recomputes it);
* maxvit_converter.json  per-key digests of what the reference's load_google_state_dict makes of tests/ckpt_maxvit.py's
                         synthetic reader for the small config (its five blocks cover every key kind: pool-only and
                         pool + conv shortcuts, identity shortcuts, both attention layers), one key per line.
Conventions (save / digest) as make_golden_convnext.py; only data is written."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))  # ckpt_maxvit

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.image import MaxViT  # noqa: E402

import ckpt_maxvit as CK  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_convnext import state_digest  # noqa: E402
from synthweights import fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)

SMALL = (32, [1, 1, 2, 1], [32, 64, 96, 128])
SUB = {0: 7, 1: 7, 2: 4, 3: 2, 4: 1}  # stem / stage i output -> pixel lattice stride


def sub(h, i):
    s = SUB[i]
    return h.permute(0, 2, 3, 1)[:, ::s, ::s].contiguous()


def g_outputs():
    out = {}
    x = synth_input("mvit_x", (2, 3, 224, 224), 91)
    for name, cfg in (("small", SMALL), ("tiny", CK.VARIANTS["tiny"])):
        m = MaxViT(*cfg).eval()
        fill_module(m, 91)
        h = m.stem(x)
        out[f"{name}_stem"] = sub(h, 0)
        for i, stage in enumerate(m.stages):
            h = stage(h)
            out[f"{name}_stage{i}"] = sub(h, i + 1)
        out[f"{name}_out"] = m(x)
    save("maxvit", dict(img=224, seed=91, input="mvit_x", sub=SUB), **out)


def geometry_digest(sd) -> dict:
    lines = sorted(f"{k} {list(v.shape)}" for k, v in sd.items())
    return dict(keys=len(lines), params=sum(v.numel() for v in sd.values()),
                sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest())


def dump_lines(obj: dict, path: str) -> None:
    """JSON object with one entry per line (reviewable, small diffs)."""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(obj[k])}" for k in sorted(obj)) + "\n}\n")


def g_geometry_and_converter():
    geo = {variant: geometry_digest(MaxViT.from_google(variant).state_dict()) for variant in CK.VARIANTS}
    m = MaxViT(*SMALL)
    m.load_google_state_dict(CK.google_maxvit(*SMALL, seed=92))
    dump_lines(geo, os.path.join(HERE, "maxvit_geometry.json"))
    dump_lines(state_digest(m.state_dict()), os.path.join(HERE, "maxvit_converter.json"))


if __name__ == "__main__":
    g_outputs()
    g_geometry_and_converter()
