"""Generate the EnCodec fixtures by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_encodec.py

* encodec_24khz.npz, encodec_48khz.npz   EnCodec.from_facebook(variant) with tests/ckpt_encodec.py's weights (fill, seed 151) on
      batch-2 clips (ckpt_encodec.clip) of 3200 samples (the reference tests' shape), 3000 samples (no multiple of 320: the extra
      padding) and 24000 / 12800 samples (75 / 40 LSTM steps): per length <tag>_latent (2, 128, T), <tag>_codes (all quantizers) and
      <tag>_codes4 (n_quantizers=4) as int16, <tag>_scale (48khz) and <tag>_wave = decode(codes, scale).
      meta["gap"]: per length the reference's own fp32-against-fp64 gap as a fraction of each tensor's max-abs (latent, wave, the
      worst encoder layer, the worst decoder layer; the fp64 decoder is fed the fp32 codes), meta["codes_fp64_differ"] the number
      of codes the fp64 model chooses differently, meta["distinct"] the entries used per codebook on the long clip.
* encodec_layers_24khz.npz, encodec_layers_48khz.npz    the output of EVERY layer of encoder and decoder, enc.<i> / dec.<i>,
      (1, C, T), for one 2240-sample clip (7 frames: the shortest the reference serves - its last convolution reflects 6 frames),
      batch 1.  Layers longer than 48 steps keep their first and last 24 steps (every padded edge; the interior is pinned by
      latent and wave), so that the files stay small; meta["gap"] as above per layer.
* encodec_geometry.json   state_dict key -> shape, both variants.
* encodec_converter.json  digests of what the reference's load_facebook_state_dict makes of ckpt_encodec.facebook_state_dict, for
      EnCodec (both variants), EnCodecEncoder and EnCodecDecoder (weight norm / causal and GroupNorm / centred).
Conventions (save / digest) as make_golden.py; only data is written."""
import copy
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))  # ckpt_encodec

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.audio.encodec import EnCodec, EnCodecDecoder, EnCodecEncoder  # noqa: E402

import ckpt_encodec as CK  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_convnext import state_digest  # noqa: E402

torch.set_grad_enabled(False)
EDGE = 24


def model(variant):
    m = EnCodec.from_facebook(variant).eval()
    CK.fill(m, CK.SEED, CK.GAIN[variant])
    return m


def rel_gap(a32, a64):
    return float((a32.double() - a64).abs().max() / a64.abs().max())


def gaps(m, m64, x, ck):
    """fp32 against fp64 of the reference itself; the fp64 decoder gets the fp32 codes so that a flipped code is counted apart."""
    ck64 = {}
    h = x.double()
    if m.normalize:
        h = h / (h.mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8)
    z = CK._walk(m64.encoder, h, "enc.", ck64)
    ck64["latent"] = z
    codes64 = m64.quantizer.quantize(z.transpose(1, 2)).transpose(0, 1)
    q = m64.quantizer.dequantize(ck["codes"].transpose(0, 1)).transpose(1, 2)
    y = CK._walk(m64.decoder, q, "dec.", ck64)
    ck64["wave"] = y if ck["scale"] is None else y * ck["scale"].double()
    per = {k: rel_gap(ck[k], v) for k, v in ck64.items()}
    return per, int((codes64 != ck["codes"]).sum())


def g_outputs():
    for variant in CK.VARIANTS:
        m = model(variant)
        m64 = copy.deepcopy(m).double()
        out, meta = {}, dict(seed=CK.SEED, gain=CK.GAIN[variant], input="ckpt_encodec.clip('<variant>_<tag>', 2, C, samples)", gap={},
                             codes_fp64_differ={}, distinct={})
        for tag, samples in CK.LENGTHS[variant]:
            x = CK.clip(f"{variant}_{tag}", 2, CK.CHANNELS[variant], samples)
            ck = CK.cpu_checkpoints(m, x, 4)
            codes, scale = m.encode(x)
            assert torch.equal(codes, ck["codes"]) and torch.equal(m.encode(x, 4)[0], ck["codes_q"])
            torch.testing.assert_close(m.decode(codes, scale), ck["wave"], rtol=0, atol=0)
            assert int(ck["codes"].max()) < 1024
            out[f"{tag}_latent"] = ck["latent"]
            out[f"{tag}_codes"] = ck["codes"].to(torch.int16)
            out[f"{tag}_codes4"] = ck["codes_q"].to(torch.int16)
            if scale is not None:
                out[f"{tag}_scale"] = scale
            out[f"{tag}_wave"] = ck["wave"]
            per, differ = gaps(m, m64, x, ck)
            meta["gap"][tag] = dict(latent=per["latent"], wave=per["wave"],
                                    enc_max=max(v for k, v in per.items() if k.startswith("enc.")),
                                    dec_max=max(v for k, v in per.items() if k.startswith("dec.")))
            meta["codes_fp64_differ"][tag] = differ
            meta["distinct"][tag] = [int(ck["codes"][:, i].unique().numel()) for i in range(ck["codes"].shape[1])]
            rng = {k: float(v.abs().max()) for k, v in ck.items() if k.startswith(("enc.", "dec."))}
            print(variant, tag, samples, "frames", ck["latent"].shape[2], "gap", meta["gap"][tag], "fp64 codes differ", differ,
                  "distinct", meta["distinct"][tag][:4], "layer max-abs %.3g .. %.3g" % (min(rng.values()), max(rng.values())))
        save(f"encodec_{variant}", meta, **out)


def g_layers():
    for variant in CK.VARIANTS:
        out, meta = {}, dict(seed=CK.SEED, samples=CK.LAYER_CLIP, edge=EDGE, gap={})
        m = model(variant)
        m64 = copy.deepcopy(m).double()
        x = CK.clip(f"{variant}_layers", 1, CK.CHANNELS[variant], CK.LAYER_CLIP)
        ck = CK.cpu_checkpoints(m, x)
        per, _ = gaps(m, m64, x, ck)
        for k, v in ck.items():
            if k.startswith(("enc.", "dec.")):
                out[k] = v if v.shape[2] <= 2 * EDGE else torch.cat([v[..., :EDGE], v[..., -EDGE:]], 2)
                meta["gap"][k] = per[k]
        out["codes"] = ck["codes"].to(torch.int16)
        print(variant, "layers: worst gap", max(meta["gap"].values()))
        save(f"encodec_layers_{variant}", meta, **out)


def g_geometry_and_converter():
    geo, conv = {}, {}
    for variant in CK.VARIANTS:
        m = EnCodec.from_facebook(variant)
        geo[variant] = {k: list(v.shape) for k, v in m.state_dict().items()}
        m.load_facebook_state_dict(CK.facebook_state_dict(m))
        conv[variant] = state_digest(m.state_dict())
    for cls, name in ((EnCodecEncoder, "encoder"), (EnCodecDecoder, "decoder")):
        for norm_type, causal in (("weight_norm", True), ("time_group_norm", False)):
            m = cls(1, norm_type=norm_type, causal=causal)
            m.load_facebook_state_dict(CK.facebook_state_dict(m))
            conv[f"{name}/{norm_type}"] = state_digest(m.state_dict())
    for name, obj in (("encodec_geometry", geo), ("encodec_converter", conv)):
        with open(os.path.join(HERE, name + ".json"), "w") as f:  # one line per variant
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(obj[k], sort_keys=True)}" for k in sorted(obj)) + "\n}\n")


if __name__ == "__main__":
    g_outputs()
    g_layers()
    g_geometry_and_converter()
