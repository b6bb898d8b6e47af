"""ConvNeXt on the CPU: this package's classes against the reference's state_dict layout (tests/golden/convnext_geometry.json), its
facebook loader (digests in convnext_converter.json) and its outputs (convnext.npz, make_golden_convnext.py), plus the CPU
form's torch.compile and the no-network rule.  No kernel runs here."""
import json
import os

import pytest
import torch

import ckpt_convnext as CK
from synthweights import fill_module, synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_exported_from_image():
    from pytorch_models.image import ConvNeXt
    from pytorch_models.image.convnext import ConvNeXtBlock, Permute

    assert issubclass(ConvNeXt, torch.nn.Sequential) and issubclass(ConvNeXtBlock, torch.nn.Sequential)
    assert ConvNeXtBlock.expansion == 4 and Permute(0, 2, 3, 1)(torch.zeros(1, 2, 3, 4)).shape == (1, 3, 4, 2)


@pytest.mark.parametrize("variant", list(CK.VARIANTS))
def test_geometry_matches_the_reference(variant):
    from pytorch_models.image import ConvNeXt

    want = json.load(open(os.path.join(GOLDEN, "convnext_geometry.json")))[variant]
    got = {k: list(v.shape) for k, v in ConvNeXt.from_facebook(variant).state_dict().items()}
    assert got == want


@pytest.mark.parametrize("variant", ["atto", "tiny"])
def test_facebook_loader_matches_the_reference(variant):
    from pytorch_models.image import ConvNeXt

    want = json.load(open(os.path.join(GOLDEN, "convnext_converter.json")))[variant]
    d, depths = CK.VARIANTS[variant]
    m = ConvNeXt.from_facebook(variant)
    ck = CK.facebook_convnext(d, depths, seed=72)
    assert any(k.startswith("head.") for k in ck)
    m.load_facebook_state_dict(ck)
    got = {k: [float(x) for x in (v.double().sum(), v.double().abs().sum(),
                                  (v.double().flatten() * (1.0 + (torch.arange(v.numel(), dtype=torch.float64) % 251) / 251.0)).sum())]
           for k, v in m.state_dict().items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


@pytest.mark.parametrize("variant", ["atto", "tiny"])
def test_cpu_forward_matches_the_reference_outputs(golden, variant):
    from pytorch_models.image import ConvNeXt

    g = golden("convnext")
    m = ConvNeXt.from_facebook(variant).eval()
    with torch.no_grad():
        fill_module(m, 71)
        x = synth_input("cnx_x", (2, 3, 64, 64), 71)
        h = m.stem(x)
        torch.testing.assert_close(h, g[f"{variant}_stem"], rtol=2e-5, atol=2e-5)
        for i, stage in enumerate(m.stages):
            h = stage(h)
            torch.testing.assert_close(h, g[f"{variant}_stage{i}"], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(m(x), g[f"{variant}_out"], rtol=2e-5, atol=2e-5)


def test_pretrained_raises_without_the_network(monkeypatch):
    from pytorch_models.image import ConvNeXt

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    with pytest.raises(NotImplementedError, match="download"):
        ConvNeXt.from_facebook("tiny", pretrained=True)


def test_cpu_form_compiles_fullgraph():
    from pytorch_models.image import ConvNeXt

    m = ConvNeXt.from_facebook("atto").eval()
    with torch.no_grad():
        fill_module(m, 73)
        x = synth_input("cnx_compile", (1, 3, 32, 32), 73)
        want = m(x)
        got = torch.compile(m, fullgraph=True)(x)
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)


def test_cpu_block_is_nhwc_in_and_out():
    from pytorch_models.image.convnext import ConvNeXtBlock

    blk = ConvNeXtBlock(8).eval()
    with torch.no_grad():
        fill_module(blk, 74)
        x = synth_input("cnx_blk", (2, 5, 6, 8), 74)
        y = blk(x)
        want = x + blk[6](blk[5](blk[4](blk[3](blk[1](x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))))) * blk.gamma
    assert y.shape == x.shape
    torch.testing.assert_close(y, want, rtol=0, atol=0)
