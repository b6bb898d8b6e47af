"""DETR on the CPU: this package's classes against the reference's state_dict layout (tests/golden/detr_geometry.json), its
facebook loader (digests in detr_converter.json), its outputs (detr.npz) and its layers on inputs that SEE the position and query
embeddings (detr_layers.npz; make_golden_detr.py proves on the reference that every way of mishandling an embedding moves those
outputs by at least 10 x the bf16 rounding distance), plus the pipeline, torch.compile, the no-network rule - and the layer
subclassing that DETR is the first model here to use: a subclassed MHA inside a stock EncoderLayer, and EncoderLayer /
DecoderLayer subclasses that override forward and call self.sa(q, k, v) with three tensors.  No kernel runs here."""
import hashlib
import json
import os

import pytest
import torch
from torch import Tensor

import ckpt_detr as CK
from synthweights import fill_module, synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 131
SKIP = ("window", "filters", "freqs")
RTOL, ATOL = 2e-5, 3e-5  # the reference's own tolerances (tests/image/test_detr.py)
torch.set_grad_enabled(False)


def _digest(v):
    f = v.double().flatten()
    w = 1.0 + (torch.arange(f.numel(), dtype=torch.float64) % 251) / 251.0
    return [float(f.sum()), float(f.abs().sum()), float((f * w).sum())]


def _model(name):
    from pytorch_models.image import DETR

    m = (DETR([1, 1, 1, 1]) if name == "small" else DETR.from_facebook("resnet50")).eval()
    fill_module(m, SEED, skip=SKIP)
    shape = (2, 3, 224, 225) if name == "small" else (2, 3, 224, 224)
    return m, synth_input(f"detr_{name}_x", shape, SEED)


def test_exported_from_image():
    from pytorch_models.image import DETR, DETRPipeline
    from pytorch_models.image import detr as D
    from pytorch_models.transformer import DecoderLayer, EncoderLayer

    for name in ("Bottleneck", "ResNet", "DETRDecoderLayer", "DETREncoderLayer", "SinusoidalPositionEmbedding2d", "DETR", "DETRPipeline"):
        assert hasattr(D, name), name
    assert D.DETR is DETR and D.DETRPipeline is DETRPipeline
    assert issubclass(D.DETREncoderLayer, EncoderLayer) and issubclass(D.DETRDecoderLayer, DecoderLayer)
    layer = D.DETRDecoderLayer(256)
    assert layer.sa.head_dim == 32 and layer.sa.n_heads == 8 and layer.mlp.linear1.out_features == 2048 and not layer.pre_norm
    assert "pos_embed.freqs" not in DETR([1, 1, 1, 1]).state_dict()


@pytest.mark.parametrize("variant", list(CK.VARIANTS))
def test_geometry_matches_the_reference(variant):
    from pytorch_models.image import DETR

    want = json.load(open(os.path.join(GOLDEN, "detr_geometry.json")))[variant]
    sd = DETR.from_facebook(variant).state_dict()
    lines = sorted(f"{k} {list(v.shape)}" for k, v in sd.items())
    got = dict(keys=len(lines), params=sum(v.numel() for v in sd.values()),
               sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest())
    assert got == want
    if variant == "resnet50":
        assert got["keys"] == 583


def test_facebook_loader_matches_the_reference():
    from pytorch_models.image import DETR

    want = json.load(open(os.path.join(GOLDEN, "detr_converter.json")))
    m = DETR([1, 1, 1, 1])
    m.load_facebook_state_dict(CK.facebook_detr([1, 1, 1, 1], seed=SEED + 2))
    got = {k: _digest(v) for k, v in m.state_dict().items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


def test_facebook_loader_rejects_a_missing_key():
    from pytorch_models.image import DETR

    sd = CK.facebook_detr([1, 1, 1, 1], seed=SEED + 2)
    del sd["transformer.decoder.layers.3.multihead_attn.in_proj_bias"]
    with pytest.raises(KeyError):
        DETR([1, 1, 1, 1]).load_facebook_state_dict(sd)


def test_a_reference_layout_state_dict_loads_strictly():
    """The keys and shapes of the reference's resnet50 state_dict (digest-checked above) load with strict=True and change the
    model; round trip through a fresh instance."""
    from pytorch_models.image import DETR

    src = DETR.from_facebook("resnet50")
    fill_module(src, 7, skip=SKIP)
    dst = DETR.from_facebook("resnet50")
    res = dst.load_state_dict(src.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.decoder[5].ca.k_proj.weight, src.decoder[5].ca.k_proj.weight)
    assert torch.equal(dst.backbone.stages[3][0].shortcut[1].running_var, src.backbone.stages[3][0].shortcut[1].running_var)


@pytest.mark.parametrize("name", ["small", "r50"])
def test_cpu_forward_matches_the_reference_outputs(golden, name):
    g = golden("detr")
    sub = {int(k): v for k, v in g["meta"]["sub"][name].items()}
    tok = g["meta"]["tok"]
    m, x = _model(name)
    nhwc = lambda t, i: t.permute(0, 2, 3, 1)[:, :: sub[i], :: sub[i]]  # noqa: E731
    h = m.backbone.stem(x)
    torch.testing.assert_close(nhwc(h, 0), g[f"{name}_stem"], rtol=RTOL, atol=ATOL)
    for i, stage in enumerate(m.backbone.stages):
        h = stage(h)
        torch.testing.assert_close(nhwc(h, i + 1), g[f"{name}_stage{i}"], rtol=RTOL, atol=ATOL)
    h = m.input_proj(h)
    pos = m.pos_embed(h.shape[-2], h.shape[-1]).flatten(0, 1)
    t = h.flatten(-2).transpose(-1, -2)
    torch.testing.assert_close(t[:, ::tok], g[f"{name}_input_proj"], rtol=RTOL, atol=ATOL)
    for layer in m.encoder:
        t = layer(t, pos)
    torch.testing.assert_close(t[:, ::tok], g[f"{name}_memory"], rtol=RTOL, atol=ATOL)
    logits, boxes = m(x)
    assert logits.shape == (2, 100, 92) and boxes.shape == (2, 100, 4)
    torch.testing.assert_close(logits[:, ::tok], g[f"{name}_logits"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(boxes, g[f"{name}_boxes"], rtol=RTOL, atol=ATOL)


def layer_inputs(tag: str):
    """The inputs of make_golden_detr.g_layers for tag "" (7 x 8) or "950" (25 x 38)."""
    from pytorch_models.image.detr import SinusoidalPositionEmbedding2d

    h, w = (7, 8) if tag == "" else (25, 38)
    pos = SinusoidalPositionEmbedding2d(256)(h, w).flatten(0, 1).contiguous()
    return dict(pos=pos, x=synth_input(f"detr_layer_x{tag}", (2, h * w, 256), SEED),
                mem=synth_input(f"detr_layer_mem{tag}", (2, h * w, 256), SEED),
                qe=synth_input("detr_layer_qe", (100, 256), SEED), queries=synth_input("detr_layer_queries", (2, 100, 256), SEED))


def layer_modules():
    from pytorch_models.image.detr import DETRDecoderLayer, DETREncoderLayer

    enc, dec = DETREncoderLayer(256).eval(), DETRDecoderLayer(256).eval()
    fill_module(enc, SEED)
    fill_module(dec, SEED + 1)
    return enc, dec


@pytest.mark.parametrize("tag", ["", "950"])
def test_cpu_layers_match_the_reference(golden, tag):
    g = golden("detr_layers")
    rows = g["meta"]["rows950"]
    d = g["meta"]["distances"]
    for kind in ("enc", "dec"):  # what the fixture is worth: every mutant of the embedding handling is far from it
        muts = [v for k, v in d.items() if k.startswith(f"{kind}:") and not k.endswith(":bf16")]
        assert muts and min(muts) >= 10 * d[f"{kind}:bf16"]
    i = layer_inputs(tag)
    enc, dec = layer_modules()
    got = enc(i["x"], i["pos"])
    torch.testing.assert_close(got if tag == "" else got[:, ::rows], g[f"enc{tag}"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dec(i["queries"], i["mem"], i["qe"], i["pos"]), g[f"dec{tag}"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("size", [224, 225])
def test_any_image_size_runs(size):
    from pytorch_models.image import DETR

    m = DETR([1, 1, 1, 1]).eval()
    fill_module(m, 3, skip=SKIP)
    logits, boxes = m(synth_input("detr_size", (1, 3, size, size), 3))
    assert logits.shape == (1, 100, 92) and boxes.shape == (1, 100, 4)
    assert torch.isfinite(logits).all() and (boxes >= 0).all() and (boxes <= 1).all()


def test_cpu_form_compiles_fullgraph():
    from pytorch_models.image import DETR

    m = DETR([1, 1, 1, 1], d_model=64, n_classes=5, n_queries=7).eval()
    fill_module(m, 5, skip=SKIP)
    x = synth_input("detr_compile", (1, 3, 64, 64), 5)
    want = m(x)
    got = torch.compile(m, fullgraph=True)(x)
    torch.testing.assert_close(got[0], want[0], rtol=2e-5, atol=3e-5)
    torch.testing.assert_close(got[1], want[1], rtol=2e-5, atol=3e-5)


def test_pretrained_raises_without_the_network(monkeypatch):
    from pytorch_models.image import DETR

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    for tag in ("resnet50", "resnet101"):
        with pytest.raises(NotImplementedError, match="download"):
            DETR.from_facebook(tag, pretrained=True)
    with pytest.raises(KeyError):
        DETR.from_facebook("resnet18")


def test_coco_classes_are_the_committed_data():
    from pytorch_models.image import DETRPipeline

    want = json.load(open(os.path.join(GOLDEN, "coco_classes.json")))
    assert len(want) == 91 and DETRPipeline.COCO_CLASSES == want


def test_pipeline_on_fixed_logits_and_boxes():
    """Host-side post-processing on a model stub: padding to the largest image, thresholding on the best real class (the last
    class is "no object"), boxes scaled to pixels and converted from (cx, cy, w, h) to corners."""
    from pytorch_models.image import DETRPipeline
    from pytorch_models.image.detr import DETR

    class Stub(DETR):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.seen = None

        def forward(self, x):
            self.seen = x
            logits = torch.full((2, 3, 92), -10.0)
            logits[0, 0, 17] = 10.0   # confident
            logits[0, 1, 91] = 10.0   # confident "no object"
            logits[0, 2, 1] = -9.0    # diffuse
            logits[1, 2, 2] = 10.0
            boxes = torch.tensor([[0.5, 0.5, 0.2, 0.4]]).expand(2, 3, 4).clone()
            boxes[1, 2] = torch.tensor([0.25, 0.75, 0.5, 0.5])
            return logits, boxes

    stub = Stub()
    pipe = DETRPipeline(stub)
    imgs = [torch.ones(3, 40, 100), torch.ones(3, 50, 80)]
    out = pipe(imgs)
    assert stub.seen.shape == (2, 3, 50, 100)
    torch.testing.assert_close(stub.seen[0, :, 0, 0], (1 - pipe.mean.flatten()) / pipe.std.flatten())
    torch.testing.assert_close(stub.seen[0, :, 45, 0], (0 - pipe.mean.flatten()) / pipe.std.flatten())  # the padding, normalised
    (c0, b0, p0), (c1, b1, p1) = out
    assert c0 == [DETRPipeline.COCO_CLASSES[17]] and c1 == [DETRPipeline.COCO_CLASSES[2]]
    assert p0.shape == (1,) and float(p0[0]) > 0.99
    torch.testing.assert_close(b0, torch.tensor([[40.0, 15.0, 60.0, 35.0]]))
    torch.testing.assert_close(b1, torch.tensor([[0.0, 25.0, 50.0, 50.0]]))
    assert len(pipe(imgs, th=1.1)[0][0]) == 0
    torch.testing.assert_close(DETRPipeline.cxcywh_to_xyxy(torch.tensor([1.0, 2.0, 2.0, 2.0])), torch.tensor([0.0, 1.0, 2.0, 3.0]))


# ---------------------------------------------------------------------------------------------------------------- subclassing
def test_subclassed_mha_with_the_reference_signature_inside_a_stock_encoder_layer():
    """RelativeMHA-style: forward(self, x) only (reference image/maxvit.py:108).  The stock EncoderLayer calls self.sa(x) - no
    `causal` keyword where the layer is not causal."""
    from pytorch_models.transformer import MHA, EncoderLayer

    class OneArgMHA(MHA):
        def forward(self, x: Tensor) -> Tensor:
            return super().forward(x, attn_bias=torch.zeros(x.shape[-2], x.shape[-2]))

    for pre in (True, False):
        layer = EncoderLayer(64, n_heads=2, pre_norm=pre).eval()
        plain = layer.sa
        sub = OneArgMHA(64, n_heads=2).eval()
        sub.load_state_dict(plain.state_dict())
        fill_module(layer, 9)
        x = synth_input("sub_x", (2, 5, 64), 9)
        want = layer(x)
        sub.load_state_dict(plain.state_dict())
        layer.sa = sub
        torch.testing.assert_close(layer(x), want, rtol=2e-5, atol=3e-5)


def test_subclassed_mha_in_a_decoder_layer_still_gets_causal_and_memory():
    from pytorch_models.transformer import MHA, DecoderLayer

    calls = []

    class Spy(MHA):
        def forward(self, q, k=None, v=None, attn_bias=None, causal=False):
            calls.append((k is not None, causal))
            return super().forward(q, k, v, attn_bias, causal)

    layer = DecoderLayer(64, n_heads=2, cross_attn=True).eval()
    fill_module(layer, 9)
    x, mem = synth_input("sub_x", (2, 5, 64), 9), synth_input("sub_mem", (2, 3, 64), 9)
    want = layer(x, mem)
    for name in ("sa", "ca"):
        spy = Spy(64, n_heads=2).eval()
        spy.load_state_dict(getattr(layer, name).state_dict())
        setattr(layer, name, spy)
    torch.testing.assert_close(layer(x, mem), want, rtol=2e-5, atol=3e-5)
    assert calls == [(False, True), (True, False)]


def test_detr_style_layer_subclasses_call_sa_with_three_tensors():
    from pytorch_models.transformer import DecoderLayer, EncoderLayer

    class Enc(EncoderLayer):
        def forward(self, x, pos):
            q = k = x + pos
            x = self.sa_norm(x + self.sa(q, k, x))
            return self.mlp_norm(x + self.mlp(x))

    class Dec(DecoderLayer):
        def forward(self, x, memory, qe, pos):
            q = k = x + qe
            x = self.sa_norm(x + self.sa(q, k, x))
            x = self.ca_norm(x + self.ca(x + qe, memory + pos, memory))
            return self.mlp_norm(x + self.mlp(x))

    enc = Enc(64, n_heads=2, act="relu", pre_norm=False).eval()
    dec = Dec(64, n_heads=2, cross_attn=True, act="relu", pre_norm=False).eval()
    fill_module(enc, 9)
    fill_module(dec, 10)
    x, pos = synth_input("sub_x", (2, 6, 64), 9), synth_input("sub_pos", (6, 64), 9)
    y = enc(x, pos)
    # against the formula written out with torch's own attention
    import torch.nn.functional as F

    def mha(m, q, k, v):
        split = lambda t: t.unflatten(-1, (m.n_heads, m.head_dim)).transpose(-2, -3)  # noqa: E731
        o = F.scaled_dot_product_attention(split(F.linear(q, m.q_proj.weight, m.q_proj.bias)), split(F.linear(k, m.k_proj.weight, m.k_proj.bias)),
                                           split(F.linear(v, m.v_proj.weight, m.v_proj.bias)))
        return F.linear(o.transpose(-2, -3).flatten(-2), m.out_proj.weight, m.out_proj.bias)

    ln = lambda n, t: F.layer_norm(t, (64,), n.weight, n.bias, n.eps)  # noqa: E731
    mlp = lambda m, t: F.linear(F.relu(F.linear(t, m.linear1.weight, m.linear1.bias)), m.linear2.weight, m.linear2.bias)  # noqa: E731
    w = ln(enc.sa_norm, x + mha(enc.sa, x + pos, x + pos, x))
    torch.testing.assert_close(y, ln(enc.mlp_norm, w + mlp(enc.mlp, w)), rtol=2e-5, atol=3e-5)
    qe, q0 = synth_input("sub_qe", (4, 64), 9), torch.zeros(4, 64)
    out = dec(q0, y, qe, pos)  # unbatched queries against a batched memory, as DETR's first decoder layer sees them
    a = ln(dec.sa_norm, q0 + mha(dec.sa, q0 + qe, q0 + qe, q0))
    b = ln(dec.ca_norm, a + mha(dec.ca, a + qe, y + pos, y))
    torch.testing.assert_close(out, ln(dec.mlp_norm, b + mlp(dec.mlp, b)), rtol=2e-5, atol=3e-5)
    assert out.shape == (2, 4, 64)
