"""Generate the DETR fixtures by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_detr.py

* detr_geometry.json    per `from_facebook` variant (resnet50, resnet101): the number of state_dict keys, of parameters, and the
                        sha256 of the sorted "key shape" lines;
* detr_converter.json   per-key digests of what the reference's load_facebook_state_dict makes of tests/ckpt_detr.py's synthetic
                        checkpoint for DETR([1, 1, 1, 1]) (in_proj chunking, downsample, both meanings of norm2, query_embed.weight);
* coco_classes.json     DETRPipeline.COCO_CLASSES as data;
* detr.npz              whole model, synthweights.fill_module (seed 131; the analytic `freqs` buffer is kept, like the STFT window):
                        `small` = DETR([1, 1, 1, 1]) on 2 x 3 x 224 x 225 images (7 x 8 tokens; odd width: the stride-2 edges) and
                        `r50` = from_facebook("resnet50") on 2 x 3 x 224 x 224: stem output, each stage output (NHWC, pixels on a
                        lattice), input_proj output and encoder memory ((N, HW, d), every 2nd token), logits (every 2nd query), boxes;
* detr_layers.npz       one DETREncoderLayer(256) and one DETRDecoderLayer(256) on N(0, 1) inputs with the real sinusoid, because
                        the whole-model outputs are nearly blind to the decoder's embedding handling: `enc` (2, 56, 256) with the
                        7 x 8 table; `dec` queries (2, 100, 256), memory (2, 56, 256), query_embed N(0, 1); and HW = 950 (25 x 38)
                        forms `enc950` / `dec950` of which a row lattice is kept.  Before anything is written, seven MUTANTS of
                        the embedding handling are run on the reference and, on the 56-token shape, each must be at least 10 x the
                        distance that rounding weights and inputs to bf16 causes; all measured distances go into the metadata.
Conventions (save / digest) as make_golden_maxvit.py; only data is written."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))  # ckpt_detr

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.image import detr as R  # noqa: E402

import ckpt_detr as CK  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_convnext import state_digest  # noqa: E402
from make_golden_maxvit import dump_lines, geometry_digest  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)

SEED = 131
SKIP = ("window", "filters", "freqs")  # analytic buffers keep their values
SUB = dict(small={0: 8, 1: 14, 2: 7, 3: 7, 4: 7}, r50={0: 8, 1: 14, 2: 7, 3: 7, 4: 6})  # stem / stage i output -> pixel lattice stride (last column of the odd-width maps included)
TOK = 2  # token lattice of input_proj / memory, query lattice of the logits
ROWS950 = 19  # row lattice of the 950-token outputs


def rel(a, b):
    return float((a - b).norm() / b.norm())


def g_outputs():
    out = {}
    for name, m, shape in (("small", R.DETR([1, 1, 1, 1]), (2, 3, 224, 225)), ("r50", R.DETR.from_facebook("resnet50"), (2, 3, 224, 224))):
        m.eval()
        fill_module(m, SEED, skip=SKIP)
        x = synth_input(f"detr_{name}_x", shape, SEED)
        sub = SUB[name]
        h = m.backbone.stem(x)
        out[f"{name}_stem"] = h.permute(0, 2, 3, 1)[:, ::sub[0], ::sub[0]].contiguous()
        for i, stage in enumerate(m.backbone.stages):
            h = stage(h)
            out[f"{name}_stage{i}"] = h.permute(0, 2, 3, 1)[:, ::sub[i + 1], ::sub[i + 1]].contiguous()
        h = m.input_proj(h)
        pos = m.pos_embed(h.shape[-2], h.shape[-1]).flatten(0, 1)
        t = h.flatten(-2).transpose(-1, -2)
        out[f"{name}_input_proj"] = t[:, ::TOK].contiguous()
        for layer in m.encoder:
            t = layer(t, pos)
        out[f"{name}_memory"] = t[:, ::TOK].contiguous()
        logits, boxes = m(x)
        out[f"{name}_logits"], out[f"{name}_boxes"] = logits[:, ::TOK].contiguous(), boxes
    save("detr", dict(seed=SEED, sub=SUB, tok=TOK, inputs="detr_{small,r50}_x", skip=SKIP), **out)


# ---------------------------------------------------------------------------------------------------------------- layer fixtures
def enc_forward(layer, x, pos, mutant=None):
    q = k = x if mutant == "no_pos" else x + pos
    v = x + pos if mutant == "pos_on_v" else x
    x = layer.sa_norm(x + layer.sa(q, k, v))
    return layer.mlp_norm(x + layer.mlp(x))


def dec_forward(layer, x, mem, qe, pos, mutant=None):
    q = k = x if mutant == "no_qe_sa" else x + qe
    v = x + qe if mutant == "qe_on_sa_v" else x
    x = layer.sa_norm(x + layer.sa(q, k, v))
    cq = x if mutant == "no_qe_ca" else x + qe
    ck = mem if mutant == "no_pos_ca" else mem + pos
    cv = mem + pos if mutant == "pos_on_ca_v" else mem
    x = layer.ca_norm(x + layer.ca(cq, ck, cv))
    return layer.mlp_norm(x + layer.mlp(x))


ENC_MUTANTS = ("no_pos", "pos_on_v")
DEC_MUTANTS = ("no_qe_sa", "no_qe_ca", "no_pos_ca", "qe_on_sa_v", "pos_on_ca_v")


def rounded(layer, *ts):
    import copy

    l2 = copy.deepcopy(layer)
    bf16_round_(l2)
    return l2, [t.to(torch.bfloat16).float() for t in ts]


def g_layers():
    out, dist = {}, {}
    pe = R.SinusoidalPositionEmbedding2d(256)
    enc = R.DETREncoderLayer(256).eval()
    dec = R.DETRDecoderLayer(256).eval()
    fill_module(enc, SEED)
    fill_module(dec, SEED + 1)
    qe = synth_input("detr_layer_qe", (100, 256), SEED)
    xq = synth_input("detr_layer_queries", (2, 100, 256), SEED)
    for tag, (h, w) in (("", (7, 8)), ("950", (25, 38))):
        pos = pe(h, w).flatten(0, 1).contiguous()
        x = synth_input(f"detr_layer_x{tag}", (2, h * w, 256), SEED)
        want = enc(x, pos)
        assert torch.equal(want, enc_forward(enc, x, pos)), "the local spelling of the layer IS the reference's forward"
        l2, (x2, p2) = rounded(enc, x, pos)
        base = rel(enc_forward(l2, x2, p2), want)
        dist[f"enc{tag}:bf16"] = base
        for mu in ENC_MUTANTS:
            dist[f"enc{tag}:{mu}"] = d = rel(enc_forward(enc, x, pos, mu), want)
            assert tag or d >= 10 * base, f"enc mutant {mu}: {d:.4f} is not 10 x the bf16 rounding distance {base:.4f}"
        mem = synth_input(f"detr_layer_mem{tag}", (2, h * w, 256), SEED)
        wantd = dec(xq, mem, qe, pos)
        assert torch.equal(wantd, dec_forward(dec, xq, mem, qe, pos))
        l2, (q2, m2, e2, p2) = rounded(dec, xq, mem, qe, pos)
        base = rel(dec_forward(l2, q2, m2, e2, p2), wantd)
        dist[f"dec{tag}:bf16"] = base
        for mu in DEC_MUTANTS:
            dist[f"dec{tag}:{mu}"] = d = rel(dec_forward(dec, xq, mem, qe, pos, mu), wantd)
            # the 10 x requirement is on the 56-token shape; over 950 random memory tokens the position term on the cross keys
            # carries less (measured about 7 x): that shape is there for the key tiles, its distances are recorded only
            assert tag or d >= 10 * base, f"dec mutant {mu}: {d:.4f} is not 10 x the bf16 rounding distance {base:.4f}"
        if tag == "":
            out["enc"], out["dec"] = want, wantd
        else:
            out["enc950"], out["dec950"] = want[:, ::ROWS950].contiguous(), wantd
    for k in sorted(dist):
        print(f"{k:24s} {dist[k]:.4f}")
    save("detr_layers", dict(seed=SEED, rows950=ROWS950, distances=dist,
                             inputs="detr_layer_{x,x950,mem,mem950,qe,queries}; enc weights seed, dec weights seed + 1"), **out)


def g_geometry_and_converter():
    geo = {variant: geometry_digest(R.DETR.from_facebook(variant).state_dict()) for variant in CK.VARIANTS}
    m = R.DETR([1, 1, 1, 1])
    m.load_facebook_state_dict(CK.facebook_detr([1, 1, 1, 1], seed=SEED + 2))
    dump_lines(geo, os.path.join(HERE, "detr_geometry.json"))
    dump_lines(state_digest(m.state_dict()), os.path.join(HERE, "detr_converter.json"))
    with open(os.path.join(HERE, "coco_classes.json"), "w") as f:
        json.dump(list(R.DETRPipeline.COCO_CLASSES), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    g_geometry_and_converter()
    g_layers()
    g_outputs()
