"""EnCodec on the MI355X: the kernels of csrc/encodec.hip against torch written here, the models against the reference's own
outputs (tests/golden/encodec_*.npz; make_golden_encodec.py) and, layer by layer on the long clips, against the CPU form.

Tolerance for fp32 activations: the project's fp32 figure is 2e-5 on outputs of order one; the synthetic 24khz stack reaches
hundreds, so every checkpoint is held to rtol = 2e-5, atol = 2e-5 * max|gold| (`close`).  The reference's own fp32-against-fp64 gap
(the fixtures' metadata) is at most 1.7e-6 of max-abs at any checkpoint, under a quarter of the absolute part.  The LSTM kernel
test uses rtol = atol = 2e-5 outright (its outputs lie in (-1, 1)).

Codes are integers and have no tolerance; a flip at stage i changes every later stage of that frame.  `decided` recomputes in fp64,
from the FIXTURE's latent, each decision's margin d(second) - d(best) and calls it decided when the margin exceeds
2 e |c_best - c_second| + 8 * 2^-24 (|r|^2 + 2 |r.c_best| + |c_best|^2): what a latent error of L2 norm e in that frame can move
the difference, plus the rounding of the fp32 distance itself.  In every frame the first stage at which the kernel's code differs
from the fixture's must be an undecided one, later stages of that frame are exempt, and differing (frame, stage) pairs are at most
1 % of all pairs.  Level 1 feeds the kernel the fixture's latent (e = 0); level 2 is encode(x) end to end with e = twice the L2
distance between the GPU encoder's latent and the fixture's in that frame (the latent is bounded by its own checkpoint).

The per-layer fixtures (encodec_layers_*.npz) hold layers of at most 48 steps in full (the late ones, 128 - 512 channels) and the
first and last 24 steps of the longer, early ones: the INTERIOR of the early layers is not pinned to the reference directly but
rests on the CPU form (`test_every_layer_of_the_long_clip_against_the_cpu_form`, itself pinned by tests/test_encodec_cpu.py) and
on the latent and the waveform, which are compared with the reference in full."""
import pytest
import torch
import torch.nn.functional as F

import ckpt_encodec as CK
from synthweights import fill_module, synth_input

pytestmark = pytest.mark.gpu

DEV = "cuda"


def close(got, gold, what=""):
    """rtol = 2e-5, atol = 2e-5 * max|gold|; prints the used fraction of the allowance before it asserts."""
    got, gold = got.detach().float().cpu(), gold.detach().float().cpu()
    assert got.shape == gold.shape, (what, got.shape, gold.shape)
    atol = 2e-5 * float(gold.abs().max())
    used = float(((got - gold).abs() / (atol + 2e-5 * gold.abs())).max()) if gold.numel() else 0.0
    print(f"{what}: max-abs {float(gold.abs().max()):.3g}, {used:.3f} of the allowance")
    torch.testing.assert_close(got, gold, rtol=2e-5, atol=atol, msg=lambda s: f"{what}: {s}")


def tm(x):
    """(B, C, T) -> time-major (B, T, C) on the device."""
    return x.transpose(1, 2).contiguous().to(DEV)


def _model(variant):
    from pytorch_models.audio import EnCodec

    m = EnCodec.from_facebook(variant).eval()
    CK.fill(m, CK.SEED, CK.GAIN[variant])
    return m


@pytest.fixture(scope="module")
def models():
    import copy

    cache = {}

    def get(variant):
        if variant not in cache:
            cpu = _model(variant)
            cache[variant] = (cpu, copy.deepcopy(cpu).to(DEV))
        return cache[variant]

    return get


# ------------------------------------------------------------------------------------------------ convolution kernel
# (Cin, Cout, k, stride) of every convolution of encoder and decoder, both variants
CONVS = [(1, 32, 7, 1), (2, 32, 7, 1), (32, 16, 3, 1), (16, 32, 1, 1), (32, 32, 1, 1), (32, 64, 4, 2), (64, 32, 3, 1), (64, 128, 8, 4),
         (128, 64, 3, 1), (128, 256, 10, 5), (256, 128, 3, 1), (256, 256, 1, 1), (256, 512, 16, 8), (512, 128, 7, 1), (128, 512, 7, 1),
         (32, 1, 7, 1), (32, 2, 7, 1)]


def _conv_case(cin, cout, k, stride, causal, T, B, elu, resid):
    from pytorch_models._hip import ops

    tag = f"conv{cin}_{cout}_{k}_{stride}_{T}"
    x = synth_input(tag + "x", (B, cin, T), 161)
    w = synth_input(tag + "w", (cout, cin, k), 161) * (cin * k) ** -0.5
    b = synth_input(tag + "b", (cout,), 161) * 0.1
    total = k - stride
    right = 0 if causal else total // 2
    left = total - right
    extra = -T % stride
    xin = F.elu(x.double()) if elu else x.double()
    want = F.conv1d(F.pad(xin, (left, right + extra), mode="reflect"), w.double(), b.double(), stride=stride)
    res = synth_input(tag + "r", tuple(want.shape), 161) if resid else None
    if resid:
        want = want + res.double()
    got = ops.conv1d_f32(tm(x), w.permute(0, 2, 1).reshape(cout, -1).contiguous().to(DEV), b.to(DEV), k=k, stride=stride, left=left,
                         right=right + extra, elu=elu, resid=tm(res) if resid else None)
    assert got.shape == (B, -(-T // stride), cout)
    return got.transpose(1, 2), want


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("cin,cout,k,stride", CONVS)
def test_conv_kernel_against_torch(cin, cout, k, stride, causal):
    """Each stage's shape: a length shorter than a tile that needs extra padding (plain), and one of several tiles with the ELU on
    load and the residual in the epilogue."""
    close(*_conv_case(cin, cout, k, stride, causal, 37, 2, False, False), f"conv {cin}->{cout} k{k} s{stride} T=37")
    close(*_conv_case(cin, cout, k, stride, causal, 333, 3, True, True), f"conv {cin}->{cout} k{k} s{stride} T=333 elu+resid")


@pytest.mark.parametrize("elu,resid", [(True, False), (False, True)])
def test_conv_kernel_elu_and_residual_alone(elu, resid):
    close(*_conv_case(32, 64, 4, 2, True, 131, 2, elu, resid), f"conv elu={elu} resid={resid}")
    close(*_conv_case(64, 32, 3, 1, False, 128, 1, elu, resid), f"conv (one full tile) elu={elu} resid={resid}")


def test_conv_kernel_shortest_clips_and_refusals():
    from pytorch_models._hip import lib, ops

    close(*_conv_case(512, 128, 7, 1, True, 7, 1, True, False), "conv T=7, 6 mirrored frames")
    close(*_conv_case(32, 64, 4, 2, False, 2, 2, False, False), "conv T=2")
    x = torch.zeros(1, 6, 512, device=DEV)
    w = torch.zeros(128, 7 * 512, device=DEV)
    with pytest.raises(ValueError, match="not served"):  # F.pad(mode="reflect") refuses a padding as long as the clip too
        ops.conv1d_f32(x, w, None, k=7, left=6, right=0)
    with pytest.raises(ValueError):
        ops.conv1d_f32(x, w[:, :-1].contiguous(), None, k=7, left=3, right=3)
    L = lib()
    assert L.pm_conv1d_f32(x.data_ptr(), 6 * 512, w.data_ptr(), None, None, x.data_ptr(), 1, 6, 512, 128, 7, 1, 6, 0, 0, 0, 1, 0, 6, None) == 2
    assert L.pm_conv1d_f32(None, 0, None, None, None, None, 1, 6, 512, 128, 7, 1, 3, 3, 0, 0, 1, 0, 6, None) == 1


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("cin,cout,stride", [(512, 256, 8), (256, 128, 5), (128, 64, 4), (64, 32, 2)])
def test_transposed_conv_against_torch(cin, cout, stride, causal):
    from pytorch_models.audio.encodec import ConvTranspose1d

    for T, B in ((7, 2), (75, 3)):
        m = ConvTranspose1d(cin, cout, 2 * stride, stride, "time_group_norm", causal).eval()  # GroupNorm form: plain weight
        m.norm = torch.nn.Identity()
        fill_module(m, 162)
        x = synth_input(f"convt{cin}_{T}", (B, cin, T), 162)
        want = F.conv_transpose1d(F.elu(x.double()), m.conv.weight.double(), m.conv.bias.double(), stride=stride)
        total = stride
        right = total if causal else total // 2
        want = want[..., total - right: -right]
        got = m.to(DEV).run_tm(tm(x), elu=True)
        assert got.shape == (B, T * stride, cout)
        close(got.transpose(1, 2), want, f"convT {cin}->{cout} s{stride} T={T}")


# ------------------------------------------------------------------------------------------------ LSTM
@pytest.fixture(scope="module")
def lstm_pair():
    ref = torch.nn.LSTM(512, 512, 2).eval()
    fill_module(ref, 163)
    ws = [[getattr(ref, f"{n}_l{l}").detach().to(DEV) for l in range(2)] for n in ("weight_ih", "weight_hh")]
    bias = [(getattr(ref, f"bias_ih_l{l}") + getattr(ref, f"bias_hh_l{l}")).detach().to(DEV) for l in range(2)]
    return ref, ws[0], ws[1], bias


@pytest.mark.parametrize("T", [1, 2, 10, 75, 300])
@pytest.mark.parametrize("B", [1, 2, 5, 33])
def test_lstm_kernel_against_nn_lstm(lstm_pair, T, B):
    from pytorch_models._hip import ops

    ref, w_ih, w_hh, bias = lstm_pair
    x = synth_input(f"lstm{T}_{B}", (B, T, 512), 163)
    with torch.no_grad():
        want = ref(x.transpose(0, 1))[0].transpose(0, 1)
    got = ops.lstm_f32(x.to(DEV), w_ih, w_hh, bias).cpu()
    print(f"lstm T={T} B={B}: max |err| {float((got - want).abs().max()):.3g}")
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)
    plain = ops.lstm_f32(x.to(DEV), w_ih, w_hh, bias, plain=True).cpu()  # per layer a GEMM and T launches, not the wavefront
    torch.testing.assert_close(plain, want, rtol=2e-5, atol=2e-5)
    if T == 10:
        res = ops.lstm_f32(x.to(DEV), w_ih, w_hh, bias, residual=True).cpu()
        torch.testing.assert_close(res, x + want, rtol=2e-5, atol=2e-5)
        one = ops.lstm_f32(x.to(DEV), w_ih[:1], w_hh[:1], bias[:1]).cpu()  # a single layer (plain passes by construction)
        with torch.no_grad():
            l0 = torch.nn.LSTM(512, 512, 1).eval()
            l0.load_state_dict({k: v for k, v in ref.state_dict().items() if k.endswith("_l0")})
            torch.testing.assert_close(one, l0(x.transpose(0, 1))[0].transpose(0, 1), rtol=2e-5, atol=2e-5)


def test_lstm_and_conv_rows_of_a_batch_are_independent(lstm_pair):
    from pytorch_models._hip import ops

    _, w_ih, w_hh, bias = lstm_pair
    x = synth_input("lstm_indep", (19, 12, 512), 164).to(DEV)
    full = ops.lstm_f32(x, w_ih, w_hh, bias, residual=True)
    for i in (0, 7, 18):
        assert torch.equal(ops.lstm_f32(x[i:i + 1].contiguous(), w_ih, w_hh, bias, residual=True)[0], full[i]), i
    xc = synth_input("conv_indep", (5, 300, 64), 164).to(DEV)
    w = (synth_input("conv_indep_w", (128, 8 * 64), 164) / 22.0).to(DEV)
    b = synth_input("conv_indep_b", (128,), 164).to(DEV)
    full = ops.conv1d_f32(xc, w, b, k=8, stride=4, left=4, right=0, elu=True)
    for i in (0, 2, 4):
        assert torch.equal(ops.conv1d_f32(xc[i:i + 1].contiguous(), w, b, k=8, stride=4, left=4, right=0, elu=True)[0], full[i]), i


def test_lstm_refusals():
    from pytorch_models._hip import lib, ops

    w = [torch.zeros(4 * 96, 96, device=DEV)]
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.lstm_f32(torch.zeros(1, 2, 96, device=DEV), w, w, [torch.zeros(4 * 96, device=DEV)])
    assert lib().pm_lstm_f32(None, None, None, None, 2, None, None, 0, 1, 1, 512, None) == 1


# ------------------------------------------------------------------------------------------------ GroupNorm, scale
@pytest.mark.parametrize("B,T,C,offset", [(2, 37, 32, 0.0), (3, 1120, 64, 3.0), (1, 312500, 32, 1.0)])
def test_groupnorm_kernel(B, T, C, offset):
    """The last case is a clip of 10^7 values with a mean of its own standard deviation: fp32 sums of that length lose the figure."""
    from pytorch_models._hip import ops

    x = synth_input(f"gn{T}", (B, C, T), 165) + offset
    g = synth_input("gn_g", (C,), 165) * 0.5 + 1
    b = synth_input("gn_b", (C,), 165)
    r = synth_input(f"gn_r{T}", (B, C, T), 165)
    want = F.group_norm(x.double(), 1, g.double(), b.double(), 1e-5)
    close(ops.groupnorm1_(tm(x), g.to(DEV), b.to(DEV), 1e-5).transpose(1, 2), want, f"groupnorm T={T}")
    close(ops.groupnorm1_(tm(x), g.to(DEV), b.to(DEV), 1e-5, tm(r)).transpose(1, 2), want + r.double(), f"groupnorm + resid T={T}")


def test_scale_kernels():
    from pytorch_models._hip import ops

    x = CK.clip("scale", 3, 2, 12345)
    want = x.double().mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8
    s = ops.encodec_scale(x.to(DEV))
    assert s.shape == (3, 1, 1)
    close(s, want, "scale")
    close(ops.scale_clips(x.to(DEV), s, divide=True), x.double() / want, "x / scale")
    close(ops.scale_clips(x.to(DEV), s, divide=False), x.double() * want, "x * scale")


# ------------------------------------------------------------------------------------------------ the quantizer
def decided(latent, books, codes, e):
    """latent (M, 128), books (Q, 1024, 128), codes (Q, M) of the fixture, e (M,): bool (Q, M), see the module docstring."""
    r = latent.double().clone()
    E = books.double()
    e = e.double()
    out = []
    for q in range(codes.shape[0]):
        d = r.square().sum(-1, keepdim=True) - 2 * r @ E[q].T + E[q].square().sum(-1)
        best = codes[q][:, None]
        dbest = d.gather(1, best)[:, 0]
        d2 = d.scatter(1, best, float("inf"))
        dsec, second = d2.min(1)
        cb, cs = E[q][codes[q]], E[q][second]
        thr = 2 * e * (cb - cs).norm(dim=1) + 8 * 2.0 ** -24 * (r.square().sum(-1) + 2 * (r * cb).sum(-1).abs() + cb.square().sum(-1))
        out.append(dsec - dbest > thr)
        r = r - cb
    return torch.stack(out)


def check_codes(got, fix, dec, what):
    """got, fix (Q, M) codes; dec (Q, M) decided flags."""
    differ = got != fix
    Q, M = fix.shape
    first = torch.where(differ.any(0), differ.int().argmax(0), torch.full((M,), -1))
    frames = (first >= 0).nonzero()[:, 0]
    bad = [(int(f), int(first[f])) for f in frames if bool(dec[first[f], f])]
    frac = float(differ.sum()) / differ.numel()
    print(f"{what}: {int((~dec).sum())} of {dec.numel()} decisions undecided, {len(frames)} frames differ, {100 * frac:.3f} % of pairs differ")
    assert not bad, f"{what}: (frame, stage) differs from the fixture at a decided decision: {bad[:8]}"
    assert frac <= 0.01, f"{what}: {100 * frac:.2f} % of (frame, stage) pairs differ"


def _books(m):
    return torch.stack([vq.embed for vq in m.quantizer])


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_rvq_kernel_on_the_fixture_latent(golden, models, variant):
    cpu, hip = models(variant)
    g = golden(f"encodec_{variant}")
    Q = len(cpu.quantizer)
    for tag, _ in CK.LENGTHS[variant]:
        z = g[f"{tag}_latent"].transpose(1, 2).contiguous()  # (B, T, 128)
        rows = z.reshape(-1, 128)
        fix = g[f"{tag}_codes"].long().transpose(0, 1).reshape(Q, -1)
        dec = decided(rows, _books(cpu), fix, torch.zeros(rows.shape[0]))
        got = hip.quantizer.quantize(z.to(DEV))
        assert got.dtype == torch.int64 and got.shape == (Q, *z.shape[:2])
        check_codes(got.cpu().reshape(Q, -1), fix, dec, f"{variant} {tag} RVQ kernel")
        got4 = hip.quantizer.quantize(z.to(DEV), 4)
        assert torch.equal(got4, got[:4])
        # decode: the sum of the chosen rows in stage order is the same fp32 additions as the reference's
        q = hip.quantizer.dequantize(got)
        assert torch.equal(q.cpu(), cpu.quantizer.dequantize(got.cpu()))
        assert torch.equal(hip.quantizer[1].dequantize(got[1]).cpu(), cpu.quantizer[1].dequantize(got[1].cpu()))
        one = hip.quantizer[0].quantize(z.to(DEV))
        assert torch.equal(one, got[0])


def test_rvq_ties_take_the_lowest_index():
    from pytorch_models.audio.encodec import RVQ

    q = RVQ(128, 1024, 2)
    with torch.no_grad():
        for vq in q:
            vq.embed.copy_(synth_input("tie_book", (1024, 128), 166))
        q[0].embed[900] = q[0].embed[17]
        q[0].embed[300] = q[0].embed[17]
        q[0].embed[1023] = q[0].embed[1022]
    x = q[0].embed[[17, 1022, 300, 4]].clone()[None]
    want = q.quantize(x)
    got = q.to(DEV).quantize(x.to(DEV)).cpu()
    assert got[0, 0].tolist() == [17, 1022, 17, 4] and torch.equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_latent_codes_and_waveform_against_the_reference(golden, models, variant):
    cpu, hip = models(variant)
    g = golden(f"encodec_{variant}")
    Q = len(cpu.quantizer)
    for tag, samples in CK.LENGTHS[variant]:
        x = CK.clip(f"{variant}_{tag}", 2, CK.CHANNELS[variant], samples)
        ck = hip.encode_checkpoints(x.to(DEV))
        latent = ck["latent"].transpose(1, 2).cpu()
        close(latent, g[f"{tag}_latent"], f"{variant} {tag} latent")
        if cpu.normalize:
            close(ck["scale"], g[f"{tag}_scale"], f"{variant} {tag} scale")
        else:
            assert ck["scale"] is None
        # codes, level 2: end to end, e = twice the latent's distance to the fixture's in that frame
        fix = g[f"{tag}_codes"].long()
        rows = g[f"{tag}_latent"].transpose(1, 2).reshape(-1, 128)
        e = 2 * (latent.transpose(1, 2).reshape(-1, 128).double() - rows.double()).norm(dim=1)
        dec = decided(rows, _books(cpu), fix.transpose(0, 1).reshape(Q, -1), e)
        codes, scale = hip.encode(x.to(DEV))
        assert codes.shape == fix.shape and codes.dtype == torch.int64
        check_codes(codes.cpu().transpose(0, 1).reshape(Q, -1), fix.transpose(0, 1).reshape(Q, -1), dec, f"{variant} {tag} encode")
        codes4, _ = hip.encode(x.to(DEV), 4)
        assert torch.equal(codes4, codes[:, :4])
        # waveform: decode of the FIXTURE's codes
        wave = hip.decode(fix.to(DEV), scale)
        close(wave, g[f"{tag}_wave"], f"{variant} {tag} wave")
        # round trip, per clip: the fixture's waveform where every code equals the fixture's, else the CPU form on the GPU's codes
        trip = hip.decode(codes, scale).cpu()
        for i in range(2):
            if torch.equal(codes[i].cpu(), fix[i]):
                close(trip[i], g[f"{tag}_wave"][i], f"{variant} {tag} round trip, clip {i}")
            else:
                with torch.no_grad():
                    want = cpu.decode(codes[i:i + 1].cpu(), None if scale is None else scale[i:i + 1].cpu())
                close(trip[i], want[0], f"{variant} {tag} round trip on the GPU's codes, clip {i}")


def _edges(t, edge):
    return t if t.shape[2] <= 2 * edge else torch.cat([t[..., :edge], t[..., -edge:]], 2)


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_every_layer_against_the_reference(golden, models, variant):
    cpu, hip = models(variant)
    g = golden(f"encodec_layers_{variant}")
    edge = g["meta"]["edge"]
    x = CK.clip(f"{variant}_layers", 1, CK.CHANNELS[variant], CK.LAYER_CLIP)
    enc = hip.encode_checkpoints(x.to(DEV))
    dec = hip.decode_checkpoints(g["codes"].long().to(DEV), enc["scale"])
    n = 0
    for side, ck in (("enc.", enc), ("dec.", dec)):
        for k in [k for k in g if k.startswith(side)]:
            close(_edges(ck[k[4:]].transpose(1, 2), edge), g[k], f"{variant} {k}")
            n += 1
    assert n == 22


@pytest.mark.parametrize("variant", CK.VARIANTS)
def test_every_layer_of_the_long_clip_against_the_cpu_form(models, variant):
    cpu, hip = models(variant)
    tag, samples = CK.LENGTHS[variant][2]
    x = CK.clip(f"{variant}_{tag}", 2, CK.CHANNELS[variant], samples)
    want = CK.cpu_checkpoints(cpu, x)
    enc = hip.encode_checkpoints(x.to(DEV))
    dec = hip.decode_checkpoints(want["codes"].to(DEV), enc["scale"])
    for k in [k for k in want if k.startswith(("enc.", "dec."))]:
        close((enc if k.startswith("enc.") else dec)[k[4:]].transpose(1, 2), want[k], f"{variant} long clip {k}")
    close(dec["quantized"].transpose(1, 2), want["quantized"], f"{variant} long clip quantized")
    close(dec["out"], want["wave"], f"{variant} long clip wave")


@pytest.mark.parametrize("norm_type,causal", [("weight_norm", True), ("weight_norm", False), ("time_group_norm", True), ("time_group_norm", False)])
def test_standalone_encoder_and_decoder(norm_type, causal):
    from pytorch_models.audio import EnCodecDecoder, EnCodecEncoder

    enc = EnCodecEncoder(1, norm_type=norm_type, causal=causal).eval()
    dec = EnCodecDecoder(1, norm_type=norm_type, causal=causal).eval()
    CK.fill(enc, 152)
    CK.fill(dec, 153)
    x = CK.clip("standalone", 2, 1, 3200)
    z = synth_input("standalone_z", (2, 128, 10), 167)
    with torch.no_grad():
        want_z, want_y = enc(x), dec(z)
        blk_in = synth_input("standalone_b", (2, 32, 50), 167)
        want_b, want_l = enc[1](blk_in), enc[13](synth_input("standalone_l", (2, 512, 9), 167))
    enc, dec = enc.to(DEV), dec.to(DEV)
    got_z, got_y = enc(x.to(DEV)), dec(z.to(DEV))
    assert got_z.shape == (2, 128, 10) and got_y.shape == (2, 1, 3200) and got_z.is_cuda
    close(got_z, want_z, f"standalone encoder {norm_type} causal={causal}")
    close(got_y, want_y, f"standalone decoder {norm_type} causal={causal}")
    close(enc[1](blk_in.to(DEV)), want_b, "standalone block")
    close(enc[13](synth_input("standalone_l", (2, 512, 9), 167).to(DEV)), want_l, "standalone LSTM")


def test_graphed_encoder_replay_equals_eager(models):
    from pytorch_models.graph import GraphedForward

    _, hip = models("24khz")
    x = CK.clip("graph", 2, 1, 6400).to(DEV)
    eager = hip.encoder(x).clone()
    g = GraphedForward(hip.encoder, x)
    assert torch.equal(g(x), eager)
    x2 = CK.clip("graph2", 2, 1, 6400).to(DEV)
    out2 = g(x2).clone()
    assert torch.equal(out2, hip.encoder(x2)) and not torch.equal(out2, eager)


def test_derived_weights_follow_the_parameters(models):
    import copy

    _, hip = models("24khz")
    m = copy.deepcopy(hip)
    x = CK.clip("derived", 1, 1, 3200).to(DEV)
    a = m.encoder(x).clone()
    with torch.no_grad():
        m.encoder[0].conv.parametrizations.weight.original0.mul_(1.5)
    b = m.encoder(x)
    with torch.no_grad():
        want = copy.deepcopy(m).cpu().encoder(x.cpu())
    assert not torch.equal(a, b)
    close(b, want, "after an in-place change of a weight-norm gain")


def test_refusals(models):
    from pytorch_models.audio import EnCodec, EnCodecEncoder

    cpu, hip = models("24khz")
    x = CK.clip("refuse", 1, 1, 3200)
    with pytest.raises(ValueError, match="parameters on"):
        hip.encode(x)
    with pytest.raises(ValueError, match="HIP devices only|no CPU path"):
        cpu.encode(x.to(DEV))
    with pytest.raises(ValueError):
        hip.decode(torch.zeros(1, 32, 10, dtype=torch.int64))
    for dt in (torch.bfloat16, torch.float16):
        m = EnCodecEncoder(1).eval().to(DEV).to(dt)
        with pytest.raises(NotImplementedError, match="fp32"):
            m(x.to(DEV).to(dt))
        with pytest.raises(NotImplementedError, match="fp32"):
            m(x.to(DEV))
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.encode(x.to(DEV).double())
    m = EnCodec.from_facebook("24khz").to(DEV)  # training mode
    with pytest.raises(NotImplementedError, match="eval"):
        m.encode(x.to(DEV))
    with pytest.raises(NotImplementedError, match="eval"):
        m.decode(torch.zeros(1, 32, 10, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="expected"):
        hip.encode(x[0].to(DEV))
    with pytest.raises(ValueError, match="expected"):
        hip.encode(torch.zeros(1, 2, 3200, device=DEV))
    with pytest.raises(ValueError, match="n_quantizers"):
        hip.encode(x.to(DEV), 33)
    with pytest.raises(ValueError):
        hip.decode(torch.zeros(1, 33, 10, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int64"):
        hip.decode(torch.zeros(1, 32, 10, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="not served"):  # 6 frames: the last convolution mirrors 6, as F.pad refuses on the CPU
        hip.encode(x[..., :1920].to(DEV))
