"""MLP-Mixer on the CPU: this package's classes against the reference's state_dict layout (tests/golden/mixer_geometry.json), its
Flax loader (digests in mixer_converter.json) and its outputs (mixer.npz, mixer_t49.npz; make_golden_mixer.py), the `vit.load_flax_*`
helpers the reference's Mixer imports, the tag grammar and the no-network rule.  No kernel runs here."""
import json
import os

import numpy as np
import pytest
import torch

import ckpt_mixer as CK
from synthweights import fill_module, synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 141
TOL = dict(rtol=2e-5, atol=2e-5)  # the reference's own tolerance (its tests/image/test_mlp_mixer.py)


def _digest(sd):
    return {k: [float(x) for x in (v.double().sum(), v.double().abs().sum(),
                                   (v.double().flatten() * (1.0 + (torch.arange(v.numel(), dtype=torch.float64) % 251) / 251.0)).sum())]
            for k, v in sd.items()}


def _ckpt(tag):
    size, patch = tag.split("/")
    n_layers, d = CK.SIZES[size]
    return CK.flax_mixer(n_layers, d, int(patch), (224 // int(patch)) ** 2, seed=142)


def test_exported_from_image_and_vit_names():
    from pytorch_models.image import MLPMixer
    from pytorch_models.image.mlp_mixer import MixerBlock
    from pytorch_models.image.vit import MLP, load_flax_conv2d, load_flax_linear, load_flax_ln  # noqa: F401  (the reference's import line)

    m = MLPMixer(2, 64, 16, img_size=32)
    assert [n for n, _ in m.named_children()] == ["patch_embed", "layers", "norm"]
    blk = m.layers[0]
    assert isinstance(blk, MixerBlock) and [n for n, _ in blk.named_children()] == ["norm1", "token_mixing", "norm2", "channel_mixing"]
    assert isinstance(blk.token_mixing, MLP) and blk.token_mixing.linear1.weight.shape == (32, 4)  # int(64 * 0.5) x (32 / 16)^2
    assert blk.channel_mixing.linear2.weight.shape == (64, 256) and blk.norm1.eps == 1e-6 and m.norm.eps == 1e-6


@pytest.mark.parametrize("tag", list(CK.VARIANTS))
def test_geometry_matches_the_reference(tag):
    from pytorch_models.image import MLPMixer

    want = json.load(open(os.path.join(GOLDEN, "mixer_geometry.json")))[tag]
    got = {k: list(v.shape) for k, v in MLPMixer.from_google(tag).state_dict().items()}
    assert got == want


@pytest.mark.parametrize("tag,img,batch,fixture", [("S/16", 64, 2, "mixer"), ("S/32", 224, 1, "mixer_t49")])
def test_cpu_forward_matches_the_reference_checkpoints(golden, tag, img, batch, fixture):
    from pytorch_models.image import MLPMixer

    g = golden(fixture)
    m = MLPMixer.from_google(tag, img_size=img).eval()
    with torch.no_grad():
        fill_module(m, SEED)
        got = CK.cpu_checkpoints(m, synth_input(f"mixer_x{img}", (batch, 3, img, img), SEED))
    for k in ("tokens", "mix0", "layer0", "last", "out"):
        torch.testing.assert_close(got[k], g[k], **TOL, msg=lambda s, k=k: f"{k}: {s}")


@pytest.mark.parametrize("tag,key", [("S/16", "s16_224_out"), ("B/16", "b16_224_out")])
def test_cpu_features_at_224_match_the_reference(golden, tag, key):
    from pytorch_models.image import MLPMixer

    m = MLPMixer.from_google(tag).eval()
    with torch.no_grad():
        fill_module(m, SEED)
        y = m(synth_input("mixer_x224", (2, 3, 224, 224), SEED))
    torch.testing.assert_close(y, golden("mixer")[key], **TOL)


@pytest.mark.parametrize("tag", ["S/16", "S/32"])
@pytest.mark.parametrize("how", ["path", "mapping"])
def test_jax_loader_matches_the_reference(tmp_path, tag, how):
    from pytorch_models.image import MLPMixer

    want = json.load(open(os.path.join(GOLDEN, "mixer_converter.json")))[tag]
    ck = _ckpt(tag)
    assert any(k.startswith("head/") for k in ck)
    m = MLPMixer.from_google(tag)
    if how == "path":
        path = tmp_path / "mixer.npz"
        np.savez(path, **ck)
        m.load_jax_weights(str(path))
    else:
        m.load_jax_weights(ck)
    got = _digest(m.state_dict())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


def test_vit_load_flax_helpers_behave_as_the_references():
    """The three helpers alone, driven as the reference's load_jax_weights drives them, reproduce the converter fixture; each pops
    the keys it reads and nothing else."""
    from pytorch_models.image import MLPMixer
    from pytorch_models.image.vit import load_flax_conv2d, load_flax_linear, load_flax_ln

    want = json.load(open(os.path.join(GOLDEN, "mixer_converter.json")))["S/16"]
    w = {k: torch.from_numpy(v) for k, v in _ckpt("S/16").items()}
    n0 = len(w)
    m = MLPMixer.from_google("S/16")
    with torch.no_grad():
        load_flax_conv2d(m.patch_embed, w, "stem")
        assert len(w) == n0 - 2 and "stem/kernel" not in w
        load_flax_ln(m.norm, w, "pre_head_layer_norm")
        assert len(w) == n0 - 4
        for i, layer in enumerate(m.layers):
            load_flax_ln(layer.norm1, w, f"MixerBlock_{i}/LayerNorm_0")
            load_flax_linear(layer.token_mixing.linear1, w, f"MixerBlock_{i}/token_mixing/Dense_0")
            load_flax_linear(layer.token_mixing.linear2, w, f"MixerBlock_{i}/token_mixing/Dense_1")
            load_flax_ln(layer.norm2, w, f"MixerBlock_{i}/LayerNorm_1")
            load_flax_linear(layer.channel_mixing.linear1, w, f"MixerBlock_{i}/channel_mixing/Dense_0")
            load_flax_linear(layer.channel_mixing.linear2, w, f"MixerBlock_{i}/channel_mixing/Dense_1")
    assert sorted(w) == ["head/bias", "head/kernel"]
    got = _digest(m.state_dict())
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k
    lin = torch.nn.Linear(3, 2, bias=False)
    with torch.no_grad():
        load_flax_linear(lin, {"d/kernel": torch.arange(6.0).view(3, 2)}, "d")  # (in, out) -> (out, in); no bias key is asked for
    assert torch.equal(lin.weight, torch.arange(6.0).view(3, 2).T)


def test_tag_grammar_and_pretrained_refusal(monkeypatch):
    from pytorch_models.image import MLPMixer

    m = MLPMixer.from_google("B/32_imagenet21k", img_size=64)
    assert len(m.layers) == 12 and m.patch_embed.weight.shape == (768, 3, 32, 32)
    assert m.layers[0].token_mixing.linear1.weight.shape == (384, 4)
    assert len(MLPMixer.from_google("H/14").layers) == 32 and MLPMixer.from_google("L/16").norm.weight.shape == (1024,)
    with pytest.raises(KeyError):
        MLPMixer.from_google("Ti/16")

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    for tag in ("S/16", "S/16_sam"):
        with pytest.raises(NotImplementedError, match="download"):
            MLPMixer.from_google(tag, pretrained=True)


def test_mixer_block_standalone():
    from pytorch_models.image.mlp_mixer import MixerBlock

    blk = MixerBlock(6, 16, mlp_ratio=(0.5, 2.0)).eval()
    assert blk.token_mixing.linear1.weight.shape == (8, 6) and blk.channel_mixing.linear1.weight.shape == (32, 16)
    with torch.no_grad():
        fill_module(blk, 143)
        x = synth_input("mixer_blk", (3, 6, 16), 143)
        y = blk(x)
        F = torch.nn.functional
        n1 = F.layer_norm(x, (16,), blk.norm1.weight, blk.norm1.bias, 1e-6).transpose(1, 2)
        tm = blk.token_mixing
        u = x + F.linear(F.gelu(F.linear(n1, tm.linear1.weight, tm.linear1.bias)), tm.linear2.weight, tm.linear2.bias).transpose(1, 2)
        cm = blk.channel_mixing
        n2 = F.layer_norm(u, (16,), blk.norm2.weight, blk.norm2.bias, 1e-6)
        want = u + F.linear(F.gelu(F.linear(n2, cm.linear1.weight, cm.linear1.bias)), cm.linear2.weight, cm.linear2.bias)
    assert y.shape == x.shape
    torch.testing.assert_close(y, want, rtol=1e-6, atol=1e-6)
