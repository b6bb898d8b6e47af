"""EnCodec on the CPU: this package's classes against the reference's state_dict layout (tests/golden/encodec_geometry.json), its
upstream-checkpoint loader (digests in encodec_converter.json) and its outputs (encodec_24khz.npz, encodec_48khz.npz and the per-layer
encodec_layers_*.npz; make_golden_encodec.py), standalone encoder / decoder, and the refusals that need no GPU.  No kernel runs."""
import json
import os

import pytest
import torch

import ckpt_encodec as CK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _digest(sd):
    return {k: [float(x) for x in (v.double().sum(), v.double().abs().sum(),
                                   (v.double().flatten() * (1.0 + (torch.arange(v.numel(), dtype=torch.float64) % 251) / 251.0)).sum())]
            for k, v in sd.items()}


def _model(variant):
    from pytorch_models.audio import EnCodec

    m = EnCodec.from_facebook(variant).eval()
    CK.fill(m, CK.SEED, CK.GAIN[variant])
    return m


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = _model(variant)
        return cache[variant]

    return get


def test_import_paths_and_exports():
    import pytorch_models.audio as A
    from pytorch_models.audio import EnCodec, EnCodecDecoder, EnCodecEncoder
    from pytorch_models.audio.encodec import RVQ, VQ, Conv1d, ConvTranspose1d, EnCodecBlock, LSTM, Pad1d, Unpad1d  # noqa: F401

    assert {"EnCodec", "EnCodecEncoder", "EnCodecDecoder"} <= set(A.__all__)
    assert "not built" not in A.__doc__
    m = EnCodec.from_facebook("24khz")
    assert [n for n, _ in m.named_children()] == ["encoder", "decoder", "quantizer"] and m.normalize is False
    assert isinstance(m.encoder, EnCodecEncoder) and isinstance(m.decoder, EnCodecDecoder) and len(m.quantizer) == 32
    assert [n for n, _ in m.encoder[0].named_children()] == ["pad", "conv", "norm"]
    assert [n for n, _ in m.decoder[3].named_children()] == ["conv", "norm", "unpad"]
    assert [n for n, _ in m.encoder[1].named_children()] == ["layers", "shortcut"]
    m48 = EnCodec.from_facebook("48khz")
    assert m48.normalize is True and len(m48.quantizer) == 16 and isinstance(m48.encoder[0].norm, torch.nn.GroupNorm)
    with pytest.raises(KeyError):
        EnCodec.from_facebook("16khz")


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_geometry_and_key_names_match_the_reference(variant):
    from pytorch_models.audio import EnCodec

    want = json.load(open(os.path.join(GOLDEN, "encodec_geometry.json")))[variant]
    got = {k: list(v.shape) for k, v in EnCodec.from_facebook(variant).state_dict().items()}
    assert got == want
    if variant == "24khz":
        assert "encoder.0.conv.parametrizations.weight.original0" in got and "decoder.3.conv.parametrizations.weight.original1" in got


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_facebook_loader_matches_the_reference(variant):
    from pytorch_models.audio import EnCodec

    want = json.load(open(os.path.join(GOLDEN, "encodec_converter.json")))[variant]
    m = EnCodec.from_facebook(variant)
    ck = CK.facebook_state_dict(m)
    assert any(k.endswith("_codebook.cluster_size") for k in ck) and any(".conv.conv." in k for k in ck) and any(".convtr.convtr." in k for k in ck)
    m.load_facebook_state_dict(ck)
    got = _digest(m.state_dict())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


@pytest.mark.parametrize("norm_type,causal", [("weight_norm", True), ("time_group_norm", False)])
@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_standalone_loader_is_strict_and_matches_the_reference(which, norm_type, causal):
    from pytorch_models.audio import EnCodecDecoder, EnCodecEncoder

    cls = dict(encoder=EnCodecEncoder, decoder=EnCodecDecoder)[which]
    want = json.load(open(os.path.join(GOLDEN, "encodec_converter.json")))[f"{which}/{norm_type}"]
    m = cls(1, norm_type=norm_type, causal=causal)
    ck = CK.facebook_state_dict(m)
    m.load_facebook_state_dict(ck)
    got = _digest(m.state_dict())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k
    ck["model.0.conv.conv.extra"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_facebook_state_dict(ck)  # strict, unlike EnCodec's


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_cpu_forward_matches_the_reference(golden, models, variant):
    g = golden(f"encodec_{variant}")
    m = models(variant)
    for tag, samples in CK.LENGTHS[variant]:
        x = CK.clip(f"{variant}_{tag}", 2, CK.CHANNELS[variant], samples)
        with torch.no_grad():
            latent = m.encoder(x / g[f"{tag}_scale"] if m.normalize else x)
            codes, scale = m.encode(x)
            codes4, _ = m.encode(x, 4)
            wave = m.decode(g[f"{tag}_codes"].long(), scale)
        torch.testing.assert_close(latent, g[f"{tag}_latent"], msg=lambda s: f"{tag} latent: {s}")
        assert codes.dtype == torch.int64 and codes.shape == (2, len(m.quantizer), -(-samples // CK.HOP))
        assert torch.equal(codes, g[f"{tag}_codes"].long()), tag
        assert torch.equal(codes4, g[f"{tag}_codes4"].long()) and codes4.shape[1] == 4, tag
        if m.normalize:
            torch.testing.assert_close(scale, g[f"{tag}_scale"])
        else:
            assert scale is None
        torch.testing.assert_close(wave, g[f"{tag}_wave"], msg=lambda s: f"{tag} wave: {s}")
        assert wave.shape == (2, CK.CHANNELS[variant], codes.shape[2] * CK.HOP)


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_cpu_layers_match_the_reference(golden, models, variant):
    g = golden(f"encodec_layers_{variant}")
    edge = g["meta"]["edge"]
    m = models(variant)
    ck = CK.cpu_checkpoints(m, CK.clip(f"{variant}_layers", 1, CK.CHANNELS[variant], CK.LAYER_CLIP))
    keys = [k for k in g if k.startswith(("enc.", "dec."))]
    assert sorted(keys) == sorted(k for k in ck if k.startswith(("enc.", "dec."))) and len(keys) == 22
    for k in keys:
        got = ck[k] if ck[k].shape[2] <= 2 * edge else torch.cat([ck[k][..., :edge], ck[k][..., -edge:]], 2)
        torch.testing.assert_close(got, g[k], msg=lambda s, k=k: f"{k}: {s}")
    assert torch.equal(ck["codes"], g["codes"].long())


@pytest.mark.parametrize("norm_type,causal", [("weight_norm", True), ("weight_norm", False), ("time_group_norm", True), ("time_group_norm", False)])
def test_standalone_encoder_decoder_one_channel(norm_type, causal):
    """The reference tests' shapes; the arithmetic is re-derived here from torch.nn.functional for the first encoder layer and
    the first decoder up-sampling."""
    import torch.nn.functional as F

    from pytorch_models.audio import EnCodecDecoder, EnCodecEncoder

    enc = EnCodecEncoder(1, norm_type=norm_type, causal=causal).eval()
    dec = EnCodecDecoder(1, norm_type=norm_type, causal=causal).eval()
    CK.fill(enc, 152)
    CK.fill(dec, 153)
    x = CK.clip("standalone", 2, 1, 3200)
    with torch.no_grad():
        z = enc(x)
        y = dec(z)
        assert z.shape == (2, 128, 10) and y.shape == (2, 1, 3200)
        c0 = enc[0]
        left, right = (6, 0) if causal else (3, 3)
        want = F.conv1d(F.pad(x, (left, right), mode="reflect"), c0.conv.weight, c0.conv.bias)
        if norm_type == "time_group_norm":
            want = F.group_norm(want, 1, c0.norm.weight, c0.norm.bias)
        torch.testing.assert_close(c0(x), want, rtol=1e-6, atol=1e-6)
        h = dec[1](dec[0](z))
        up = dec[3]
        want = F.conv_transpose1d(F.elu(h), up.conv.weight, up.conv.bias, stride=8)
        if norm_type == "time_group_norm":
            want = F.group_norm(want, 1, up.norm.weight, up.norm.bias)
        want = want[..., : -8] if causal else want[..., 4:-4]
        torch.testing.assert_close(up(dec[2](h)), want, rtol=1e-6, atol=1e-6)
    assert torch.isfinite(y).all() and float(y.std()) > 0


def test_cpu_form_trains_and_serves_other_dtypes():
    from pytorch_models.audio import EnCodecEncoder

    enc = EnCodecEncoder(1).train()
    with torch.enable_grad():  # (another test module may have switched autograd off for the process)
        enc(torch.randn(1, 1, 3200)).sum().backward()
    assert enc[0].conv.parametrizations.weight.original0.grad is not None
    enc = enc.double().eval()
    with torch.no_grad():
        assert enc(torch.randn(1, 1, 3200, dtype=torch.float64)).dtype == torch.float64


def test_quantizer_ties_take_the_lowest_index_and_n_quantizers_is_checked():
    from pytorch_models.audio.encodec import RVQ

    q = RVQ(128, 1024, 3)
    with torch.no_grad():
        for i, vq in enumerate(q):
            vq.embed.copy_(torch.randn(1024, 128) * 0.5**i)
        q[0].embed[700] = q[0].embed[5]
    x = q[0].embed[[5, 9]].clone()[None]
    codes = q.quantize(x)
    assert codes.shape == (3, 1, 2) and codes[0, 0].tolist() == [5, 9]
    assert q.quantize(x, 2).shape == (2, 1, 2) and torch.equal(q.quantize(x, 2), codes[:2])
    torch.testing.assert_close(q.dequantize(codes[:1]), x)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="n_quantizers"):
            q.quantize(x, bad)


def test_refusals_without_a_gpu(monkeypatch):
    from pytorch_models.audio import EnCodec
    from pytorch_models.audio.encodec import Pad1d

    m = EnCodec.from_facebook("24khz").eval()
    x = torch.zeros(1, 1, 3200)
    with pytest.raises(ValueError, match="HIP path"):
        m.encode_checkpoints(x)
    with pytest.raises(ValueError, match="HIP path"):
        m.decode_checkpoints(torch.zeros(1, 32, 10, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="convolution kernel"):
        Pad1d(7, 1, True)(torch.zeros(1, 1, 16, device="meta"))
    with pytest.raises(ValueError, match="parameters on"):  # mixed placement: a CPU input for parameters elsewhere
        EnCodec.from_facebook("24khz").to("meta").encode(x)

    def no_fetch(*a, **k):
        raise ConnectionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    with pytest.raises(ConnectionError):  # pretrained=True keeps the reference's behaviour: it asks torch.hub for the checkpoint
        EnCodec.from_facebook("24khz", pretrained=True)
