"""MaxViT on the CPU: this package's classes against the reference's state_dict layout (tests/golden/maxvit_geometry.json), its
google loader (digests in maxvit_converter.json) and its outputs (maxvit.npz, make_golden_maxvit.py), plus the CPU form's
torch.compile and the no-network rule.  No kernel runs here."""
import json
import os

import pytest
import torch

import ckpt_maxvit as CK
from synthweights import fill_module, synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = (32, [1, 1, 2, 1], [32, 64, 96, 128])
CONFIGS = dict(small=SMALL, tiny=CK.VARIANTS["tiny"])


def _digest(v):
    f = v.double().flatten()
    w = 1.0 + (torch.arange(f.numel(), dtype=torch.float64) % 251) / 251.0
    return [float(f.sum()), float(f.abs().sum()), float((f * w).sum())]


def test_exported_from_image():
    from pytorch_models.image import MaxViT
    from pytorch_models.image import maxvit as M
    from pytorch_models.transformer import MHA

    for name in ("Conv2d", "conv_norm_act", "SqueezeExcitation", "MBConv", "block", "unblock", "grid", "ungrid", "RelativeMHA",
                 "EncoderLayer", "MaxViTBlock", "MaxViT"):
        assert hasattr(M, name), name
    assert M.MaxViT is MaxViT and issubclass(M.RelativeMHA, MHA)
    sa = M.RelativeMHA(7, 96)
    assert sa.head_dim == 32 and sa.n_heads == 3 and sa.attn_bias.shape == (3, 13, 13)
    assert "bias_index" not in sa.state_dict() and sa.bias_index.shape == (7, 7)


def test_block_grid_round_trip():
    from pytorch_models.image.maxvit import block, grid, unblock, ungrid

    x = torch.arange(2 * 14 * 21 * 3, dtype=torch.float32).view(2, 14, 21, 3)
    b, nH, nW = block(x, 7)
    assert b.shape == (2, 6, 49, 3) and (nH, nW) == (2, 3)
    assert torch.equal(b[1, 4, 7 * 2 + 5], x[1, 7 + 2, 7 * 1 + 5])
    assert torch.equal(unblock(b, nH, nW, 7), x)
    g, nH, nW = grid(x, 7)
    assert torch.equal(g[1, 4, 7 * 2 + 5], x[1, 2 * 2 + 1, 5 * 3 + 1])
    assert torch.equal(ungrid(g, nH, nW, 7), x)


@pytest.mark.parametrize("variant", list(CK.VARIANTS))
def test_geometry_matches_the_reference(variant):
    import hashlib

    from pytorch_models.image import MaxViT

    want = json.load(open(os.path.join(GOLDEN, "maxvit_geometry.json")))[variant]
    sd = MaxViT.from_google(variant).state_dict()
    lines = sorted(f"{k} {list(v.shape)}" for k, v in sd.items())
    got = dict(keys=len(lines), params=sum(v.numel() for v in sd.values()),
               sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest())
    assert got == want


def test_google_loader_matches_the_reference():
    from pytorch_models.image import MaxViT

    want = json.load(open(os.path.join(GOLDEN, "maxvit_converter.json")))
    m = MaxViT(*SMALL)
    m.load_google_state_dict(CK.google_maxvit(*SMALL, seed=92))
    got = {k: _digest(v) for k, v in m.state_dict().items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


def test_google_loader_rejects_a_missing_variable():
    from pytorch_models.image import MaxViT

    r = CK.google_maxvit(*SMALL, seed=92)
    del r.tensors["maxvit/block_00_00/attention_1/relative_bias/ExponentialMovingAverage"]
    with pytest.raises(KeyError):
        MaxViT(*SMALL).load_google_state_dict(r)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_cpu_forward_matches_the_reference_outputs(golden, name):
    from pytorch_models.image import MaxViT

    g = golden("maxvit")
    sub = {int(k): v for k, v in g["meta"]["sub"].items()}
    m = MaxViT(*CONFIGS[name]).eval()
    with torch.no_grad():
        fill_module(m, 91)
        x = synth_input("mvit_x", (2, 3, 224, 224), 91)
        h = m.stem(x)
        nhwc = lambda t, i: t.permute(0, 2, 3, 1)[:, :: sub[i], :: sub[i]]  # noqa: E731
        torch.testing.assert_close(nhwc(h, 0), g[f"{name}_stem"], rtol=2e-5, atol=2e-5)
        for i, stage in enumerate(m.stages):
            h = stage(h)
            torch.testing.assert_close(nhwc(h, i + 1), g[f"{name}_stage{i}"], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(m(x), g[f"{name}_out"], rtol=2e-5, atol=2e-5)


def test_pretrained_raises_without_the_network(monkeypatch):
    import builtins

    from pytorch_models.image import MaxViT

    real_import = builtins.__import__

    def guarded(name, *a, **k):
        if name.split(".")[0] == "tensorflow":
            raise AssertionError("tensorflow was imported")
        return real_import(name, *a, **k)

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(builtins, "__import__", guarded)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    with pytest.raises(NotImplementedError, match="download"):
        MaxViT.from_google("tiny", pretrained=True)


def test_cpu_form_compiles_fullgraph():
    from pytorch_models.image import MaxViT

    m = MaxViT(16, [1, 1], [32, 64]).eval()
    with torch.no_grad():
        fill_module(m, 93)
        x = synth_input("mvit_compile", (1, 3, 56, 56), 93)
        want = m(x)
        got = torch.compile(m, fullgraph=True)(x)
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)
