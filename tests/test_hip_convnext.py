"""ConvNeXt on the MI355X: the four kernels of csrc/convnext.hip against fp32 torch written here (F.conv2d(groups=C),
F.layer_norm), the models against the CPU form (bf16: on bf16-rounded weights, rel-L2 <= 1e-2 per stage) and against the reference's
own outputs (fp32: tests/golden/convnext.npz at 2e-5), and the properties of the HIP path."""
import pytest
import torch
import torch.nn.functional as F

from synthweights import bf16_round_, fill_module, synth_input

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm())


def _vec(tag, n, seed, scale=1.0, offset=0.0):
    return (synth_input(tag, (n,), seed) * scale + offset).to(DEV)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("C,hw,N,xdt,ydt", [
    (40, (7, 7), 3, torch.float32, torch.float32),
    (40, (56, 56), 1, torch.bfloat16, torch.bfloat16),
    (96, (9, 13), 2, torch.bfloat16, torch.float32),
    (96, (56, 56), 2, torch.float32, torch.bfloat16),
    (160, (9, 13), 1, torch.float32, torch.float32),
    (160, (7, 7), 2, torch.bfloat16, torch.bfloat16),
    (768, (7, 7), 2, torch.float32, torch.float32),
    (768, (9, 13), 1, torch.bfloat16, torch.bfloat16),
    (768, (56, 56), 1, torch.float32, torch.float32),
])
def test_dwconv7_ln(C, hw, N, xdt, ydt):
    from pytorch_models._hip import ops

    H, W = hw
    x = synth_input(f"dw_x{C}", (N, H, W, C), 81).to(xdt)
    w = synth_input(f"dw_w{C}", (C, 1, 7, 7), 81) * 0.2
    b = synth_input(f"dw_b{C}", (C,), 81)
    g = synth_input(f"dw_g{C}", (C,), 81) * 0.5 + 1.0
    be = synth_input(f"dw_be{C}", (C,), 81)
    want = F.layer_norm(F.conv2d(x.float().permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1), (C,), g, be, 1e-6)
    wt = w.reshape(C, 7, 7).permute(1, 2, 0).contiguous()
    y = ops.dwconv7_ln(x.to(DEV), wt.to(DEV), b.to(DEV), g.to(DEV), be.to(DEV), 1e-6, ydt)
    ldy = -(-C // 64) * 64
    assert y.shape == (N * H * W, ldy) and y.dtype == ydt
    y = y.cpu()
    assert torch.equal(y[:, C:].float(), torch.zeros(N * H * W, ldy - C)), "pad columns must be written as zeros"
    tol = 2e-5 if ydt == torch.float32 else 1e-2
    torch.testing.assert_close(y[:, :C].float().view(N, H, W, C), want, rtol=tol, atol=tol)


@pytest.mark.parametrize("C,xdt,ydt", [(37, torch.float32, torch.float32), (96, torch.float32, torch.bfloat16),
                                       (37, torch.bfloat16, torch.float32)])
def test_ln_space_to_depth(C, xdt, ydt):
    from pytorch_models._hip import ops

    N, H, W = 2, 6, 10
    x = synth_input(f"s2d_x{C}", (N, H, W, C), 82).to(xdt)
    g, be = synth_input(f"s2d_g{C}", (C,), 82) + 1.0, synth_input(f"s2d_b{C}", (C,), 82)
    n = F.layer_norm(x.float(), (C,), g, be, 1e-6)
    want = n.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C)
    y = ops.ln_space_to_depth(x.to(DEV), g.to(DEV), be.to(DEV), 1e-6, ydt).cpu()
    ldy = -(-4 * C // 64) * 64
    assert y.shape == (N * H * W // 4, ldy)
    assert torch.equal(y[:, 4 * C:].float(), torch.zeros(y.shape[0], ldy - 4 * C))
    tol = 2e-5 if ydt == torch.float32 else 1e-2
    torch.testing.assert_close(y[:, :4 * C].float(), want, rtol=tol, atol=tol)


@pytest.mark.parametrize("d,ydt", [(45, torch.float32), (96, torch.float32), (352, torch.bfloat16)])
def test_convnext_stem(d, ydt):
    from pytorch_models._hip import ops

    imgs = synth_input(f"stem_x{d}", (2, 3, 36, 20), 83)
    w = synth_input(f"stem_w{d}", (d, 3, 4, 4), 83) * 0.2
    b, g, be = (synth_input(f"stem_{t}{d}", (d,), 83) for t in "bgc")
    want = F.layer_norm(F.conv2d(imgs, w, b, stride=4).permute(0, 2, 3, 1), (d,), g, be, 1e-6)
    y = ops.convnext_stem(imgs.to(DEV), w.reshape(d, 48).t().contiguous().to(DEV), b.to(DEV), g.to(DEV), be.to(DEV), 1e-6, ydt)
    assert y.shape == (2, 9, 5, d) and y.dtype == ydt
    tol = 2e-5 if ydt == torch.float32 else 1e-2
    torch.testing.assert_close(y.cpu().float(), want, rtol=tol, atol=tol)


@pytest.mark.parametrize("C,HW,xdt,ydt", [(37, 49, torch.float32, torch.float32), (768, 4, torch.float32, torch.bfloat16),
                                          (301, 9, torch.bfloat16, torch.float32)])
def test_mean_ln(C, HW, xdt, ydt):
    from pytorch_models._hip import ops

    x = synth_input(f"mln_x{C}", (3, HW, C), 84).to(xdt)
    g, be = synth_input(f"mln_g{C}", (C,), 84), synth_input(f"mln_b{C}", (C,), 84)
    want = F.layer_norm(x.float().mean(1), (C,), g, be, 1e-6)
    y = ops.mean_ln(x.to(DEV), g.to(DEV), be.to(DEV), 1e-6, ydt)
    tol = 2e-5 if ydt == torch.float32 else 1e-2
    torch.testing.assert_close(y.cpu().float(), want, rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------ models
def _model(variant, seed):
    from pytorch_models.image import ConvNeXt

    m = ConvNeXt.from_facebook(variant).eval()
    with torch.no_grad():
        fill_module(m, seed)
    return m


def _cpu_stages(m, x):
    with torch.no_grad():
        h = m.stem(x)
        outs = [h]
        for stage in m.stages:
            h = stage(h)
            outs.append(h)
        return outs + [m.norm(m.pool(h))]


@pytest.mark.parametrize("variant,side,batch", [("atto", 64, 2), ("tiny", 64, 2), ("tiny", 224, 2)])
def test_bf16_model_against_the_cpu_form(variant, side, batch):
    m = _model(variant, 85)
    bf16_round_(m)
    x = synth_input(f"cnx_bf16_{side}", (batch, 3, side, side), 85)
    want = _cpu_stages(m, x)
    g = m.to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        got = g.forward_stages(x.to(DEV))
        feats = g(x.to(DEV))
    assert feats.dtype == torch.bfloat16 and feats.shape == want[-1].shape
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, i
        assert rel(a, b) <= 1e-2, (i, rel(a, b))
    assert rel(feats, want[-1]) <= 1e-2


@pytest.mark.parametrize("variant", ["atto", "tiny"])
def test_fp32_model_against_the_reference_outputs(golden, variant):
    g = golden("convnext")
    m = _model(variant, 71).to(DEV)
    x = synth_input("cnx_x", (2, 3, 64, 64), 71).to(DEV)
    with torch.no_grad():
        outs = m.forward_stages(x)
        feats = m(x)
    names = ["stem"] + [f"stage{i}" for i in range(4)] + ["out"]
    for o, nm in zip(outs, names):
        torch.testing.assert_close(o.cpu(), g[f"{variant}_{nm}"], rtol=2e-5, atol=2e-5)
    assert feats.dtype == torch.float32
    torch.testing.assert_close(feats.cpu(), g[f"{variant}_out"], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_single_block_on_gpu_matches_cpu(dtype):
    from pytorch_models.image.convnext import ConvNeXtBlock

    blk = ConvNeXtBlock(96).eval()
    with torch.no_grad():
        fill_module(blk, 86)
        bf16_round_(blk)
        x = synth_input("cnx_block", (2, 9, 11, 96), 86).to(dtype)
        want = blk(x.float())
        got = blk.to(dtype).to(DEV)(x.to(DEV))
    assert got.shape == x.shape and got.dtype == dtype
    if dtype == torch.float32:
        torch.testing.assert_close(got.cpu(), want, rtol=2e-5, atol=2e-5)
    else:
        assert rel(got, want) <= 1e-2


# ------------------------------------------------------------------------------------------------ properties
def test_batch_permutation_and_repeat_are_bit_exact():
    m = _model("atto", 87).to(torch.bfloat16).to(DEV)
    x = synth_input("cnx_perm", (4, 3, 64, 96), 87).to(DEV)
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    with torch.no_grad():
        a = m(x)
        b = m(x)
        c = m(x[perm])
    assert torch.equal(a, b)
    assert torch.equal(a[perm], c)


def test_parameter_copy_rebuilds_the_derived_tensors():
    m = _model("atto", 88)
    x = synth_input("cnx_copy", (2, 3, 32, 32), 88)
    g = _model("atto", 88).to(DEV)
    with torch.no_grad():
        before = g(x.to(DEV)).cpu()
        torch.testing.assert_close(before, m(x), rtol=2e-5, atol=2e-5)
        for mod in (m, g):
            mod.stages[1][1].gamma.copy_(torch.linspace(-1, 1, 80))
            mod.stages[2][0][2].weight.mul_(-0.5)
            mod.stages[0][1][1].weight.add_(0.1)
            mod.stem[0].weight.mul_(2.0)
        after = g(x.to(DEV)).cpu()
        want = m(x)
    assert not torch.equal(before, after)
    torch.testing.assert_close(after, want, rtol=2e-5, atol=2e-5)


def test_bad_sides_and_mixed_devices_raise():
    m = _model("atto", 89)
    g = _model("atto", 89).to(DEV)
    with torch.no_grad():
        for side in ((48, 64), (64, 40)):
            with pytest.raises(ValueError, match="multiples of 32"):
                g(torch.zeros(1, 3, *side, device=DEV))
        with pytest.raises(RuntimeError):
            g(torch.zeros(1, 3, 32, 32))
        with pytest.raises(RuntimeError):
            m(torch.zeros(1, 3, 32, 32, device=DEV))
        with pytest.raises(RuntimeError):
            m.stages[0][1](torch.zeros(1, 7, 7, 40, device=DEV))
