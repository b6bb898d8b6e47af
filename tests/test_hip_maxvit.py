"""MaxViT on the MI355X: the six kernels of csrc/maxvit.hip against fp32 torch written here (explicit block() / grid() +
F.scaled_dot_product_attention with the bias, F.conv2d(groups=C) with the reference's padding, ...), the models against the CPU
form (bf16: on bf16-rounded weights, rel-L2 <= 1e-2 per stage) and against the reference's own outputs (fp32:
tests/golden/maxvit.npz at 2e-5), and the properties of the HIP path."""
import pytest
import torch
import torch.nn.functional as F

from synthweights import bf16_round_, fill_module, synth_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = (32, [1, 1, 2, 1], [32, 64, 96, 128])
TINY = (64, [2, 2, 5, 2], [64, 128, 256, 512])


def rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm())


def _gelu_t(x):
    return F.gelu(x, approximate="tanh")


# ------------------------------------------------------------------------------------------------ kernels
def _windows(x, ws, mode):
    """(N, H, W, C) -> (N * nwin, ws * ws, C), the reference's block() / grid() order."""
    N, H, W, C = x.shape
    nH, nW = H // ws, W // ws
    if mode == "block":
        t = x.view(N, nH, ws, nW, ws, C).transpose(2, 3)
    else:
        t = x.view(N, ws, nH, ws, nW, C).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(N * nH * nW, ws * ws, C)


def _window_attn_ref(qkv, N, H, W, heads, ws, mode, bias):
    d = 32 * heads
    w = _windows(qkv.float().view(N, H, W, 3 * d), ws, mode)
    q, k, v = (w[..., i * d:(i + 1) * d].unflatten(-1, (heads, 32)).transpose(1, 2) for i in range(3))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias[None] if bias is not None else None)
    o = o.transpose(1, 2).flatten(2)  # (nwin, L, d) in window order
    out = torch.empty(N * H * W, d)
    rows = _windows(torch.arange(N * H * W).view(N, H, W, 1), ws, mode).reshape(-1)
    out[rows] = o.reshape(-1, d)
    return out


@pytest.mark.parametrize("N,H,W,heads,ws,mode,with_bias", [
    (2, 56, 56, 2, 7, "block", True),
    (2, 56, 56, 2, 7, "grid", True),
    (1, 28, 56, 4, 7, "block", True),
    (1, 28, 56, 4, 7, "grid", True),
    (3, 7, 7, 16, 7, "grid", True),     # a single window (stage 4 at 224)
    (2, 14, 14, 8, 7, "block", False),
    (2, 10, 15, 3, 5, "grid", True),    # ws < 7
    (1, 16, 8, 5, 8, "block", True),    # ws = 8: L = 64, no padded keys
])
def test_window_attention(N, H, W, heads, ws, mode, with_bias):
    from pytorch_models._hip import ops

    d = 32 * heads
    qkv = synth_input(f"wa_qkv{H}{W}{heads}", (N * H * W, 3 * d), 101).to(torch.bfloat16)
    L = ws * ws
    bias = synth_input(f"wa_b{heads}{ws}", (heads, L, L), 101) if with_bias else None
    want = _window_attn_ref(qkv, N, H, W, heads, ws, mode, bias)
    q = qkv.to(DEV)
    got = ops.window_attention(q[:, :d], q[:, d:2 * d], q[:, 2 * d:], N, H, W, heads, ws, mode,
                               bias.to(DEV) if bias is not None else None)
    assert got.shape == (N * H * W, d) and got.dtype == torch.bfloat16
    torch.testing.assert_close(got.float().cpu(), want, rtol=1e-2, atol=1e-2)


def test_window_attention_rejects_bad_windows():
    from pytorch_models._hip import ops

    q = torch.zeros(1 * 9 * 9, 3 * 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.window_attention(q[:, :32], q[:, 32:64], q[:, 64:], 1, 9, 9, 1, 9, "block")  # L = 81 > 64
    with pytest.raises(RuntimeError):
        ops.window_attention(q[:, :32], q[:, 32:64], q[:, 64:], 1, 9, 9, 1, 7, "grid")  # 9 % 7


def _dw_ref(x, w, scale, shift, stride, gate=None):
    xc = x.float().permute(0, 3, 1, 2)
    C = xc.shape[1]
    if stride == 2:
        y = F.conv2d(F.pad(xc, (0, 1, 0, 1)), w, None, 2, 0, groups=C)
    else:
        y = F.conv2d(xc, w, None, 1, 1, groups=C)
    y = _gelu_t(y * scale[None, :, None, None] + shift[None, :, None, None])
    ps = y.sum(3).permute(0, 2, 1)  # (N, Ho, C)
    if gate is not None:
        y = y * gate[:, :, None, None]
    return y.permute(0, 2, 3, 1), ps


@pytest.mark.parametrize("C,hw,N,stride,dt,gated", [
    (40, (7, 7), 2, 1, torch.float32, False),
    (40, (14, 15), 1, 2, torch.float32, True),
    (256, (56, 56), 2, 1, torch.bfloat16, True),
    (256, (56, 56), 1, 2, torch.bfloat16, False),
    (384, (9, 13), 2, 2, torch.float32, True),
    (384, (28, 28), 1, 1, torch.bfloat16, True),
    (2048, (7, 7), 2, 1, torch.bfloat16, True),
    (2048, (14, 14), 1, 2, torch.float32, False),
])
def test_dwconv3_bn_act(C, hw, N, stride, dt, gated):
    from pytorch_models._hip import ops

    H, W = hw
    x = synth_input(f"dw3_x{C}", (N, H, W, C), 102).to(dt)
    w = synth_input(f"dw3_w{C}", (C, 1, 3, 3), 102) * 0.3
    sc = synth_input(f"dw3_s{C}", (C,), 102) * 0.2 + 1.0
    sh = synth_input(f"dw3_t{C}", (C,), 102) * 0.1
    gate = torch.sigmoid(synth_input(f"dw3_g{C}", (N, C), 102)) if gated else None
    want, want_ps = _dw_ref(x, w, sc, sh, stride, gate)
    wt = w.reshape(C, 9).t().reshape(3, 3, C).contiguous().to(DEV)
    y, ps = ops.dwconv3_bn_act(x.to(DEV), wt, sc.to(DEV), sh.to(DEV), stride, gate=gate.to(DEV) if gated else None,
                               want_psum=True)
    assert y.shape == want.shape and y.dtype == dt
    tol = 2e-5 if dt == torch.float32 else 1e-2
    torch.testing.assert_close(y.float().cpu(), want, rtol=tol, atol=tol)
    torch.testing.assert_close(ps.cpu(), want_ps, rtol=1e-4, atol=1e-3 if dt == torch.bfloat16 else 1e-4)
    only = ops.dwconv3_bn_act(x.to(DEV), wt, sc.to(DEV), sh.to(DEV), stride, want_psum=True, write_y=False)
    assert torch.equal(only, ps)


def test_se_gate():
    from pytorch_models._hip import ops

    N, T, C, R, hw = 3, 5, 384, 24, 35
    ps = synth_input("se_ps", (N, T, C), 103) * 3
    w1 = synth_input("se_w1", (R, C), 103) * 0.05
    b1 = synth_input("se_b1", (R,), 103) * 0.1
    w2 = synth_input("se_w2", (C, R), 103) * 0.2
    b2 = synth_input("se_b2", (C,), 103) * 0.1
    m = ps.sum(1) / hw
    want = torch.sigmoid(F.silu(m @ w1.T + b1) @ w2.T + b2)
    got = ops.se_gate(ps.to(DEV), hw, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))
    torch.testing.assert_close(got.cpu(), want, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("d,H,W", [(64, 224, 224), (32, 30, 17), (192, 14, 28)])
def test_maxvit_stem(d, H, W):
    from pytorch_models._hip import ops

    img = synth_input(f"ms_img{d}", (2, 3, H, W), 104)
    w = synth_input(f"ms_w{d}", (d, 3, 3, 3), 104) * 0.3
    sh = synth_input(f"ms_t{d}", (d,), 104) * 0.1
    want = _gelu_t(F.conv2d(F.pad(img, (0, 1, 0, 1)), w, None, 2) + sh[None, :, None, None]).permute(0, 2, 3, 1)
    got = ops.maxvit_stem(img.to(DEV), w.reshape(d, 27).t().contiguous().to(DEV), sh.to(DEV))
    torch.testing.assert_close(got.cpu(), want, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("C,dt", [(32, torch.float32), (64, torch.bfloat16), (12, torch.float32)])
def test_im2col3x3(C, dt):
    from pytorch_models._hip import ops

    N, H, W = 2, 9, 6
    x = synth_input(f"i2c{C}", (N, H, W, C), 105).to(dt)
    got = ops.im2col3x3(x.to(DEV)).cpu()
    ldy = -(-9 * C // 64) * 64
    cols = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1)  # (N, C*9, HW) in (c, kh, kw) order
    want = cols.view(N, C, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * C)
    assert got.shape == (N * H * W, ldy)
    assert torch.equal(got[:, 9 * C:].float(), torch.zeros(N * H * W, ldy - 9 * C))
    torch.testing.assert_close(got[:, :9 * C].float(), want, rtol=0, atol=0)


@pytest.mark.parametrize("dt,odt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_avgpool2x2(dt, odt):
    from pytorch_models._hip import ops

    x = synth_input("ap", (2, 14, 10, 48), 106).to(dt)
    want = F.avg_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    got = ops.avgpool2x2(x.to(DEV), out_dtype=odt)
    tol = 2e-5 if odt == torch.float32 else 1e-2
    torch.testing.assert_close(got.float().cpu(), want, rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------ models
def _model(cfg, seed, dtype):
    from pytorch_models.image import MaxViT

    m = MaxViT(*cfg).eval()
    with torch.no_grad():
        fill_module(m, seed)
        if dtype == torch.bfloat16:
            bf16_round_(m)
    return m


def _cpu_stages(m, x):
    outs = []
    with torch.no_grad():
        h = m.stem(x)
        outs.append(h.permute(0, 2, 3, 1))
        for stage in m.stages:
            h = stage(h)
            outs.append(h.permute(0, 2, 3, 1))
        outs.append(m(x))
    return outs


@pytest.mark.parametrize("cfg,hw", [(SMALL, (224, 448)), (TINY, (224, 224))], ids=["small_224x448", "tiny"])
def test_bf16_model_matches_the_cpu_form(cfg, hw):
    m = _model(cfg, 111, torch.bfloat16)
    x = synth_input("mv_bf16", (2, 3, *hw), 111)
    want = _cpu_stages(m, x)
    g = m.to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        got = g.forward_stages(x.to(DEV))
        feats = g(x.to(DEV))
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, i
        assert rel(a, b) <= 1e-2, (i, rel(a, b))
    assert feats.dtype == torch.bfloat16 and rel(feats, want[-1]) <= 1e-2


@pytest.mark.parametrize("name,cfg", [("small", SMALL), ("tiny", TINY)])
def test_fp32_model_matches_the_reference_outputs(golden, name, cfg):
    g = golden("maxvit")
    sub = {int(k): v for k, v in g["meta"]["sub"].items()}
    m = _model(cfg, 91, torch.float32).to(DEV)
    x = synth_input("mvit_x", (2, 3, 224, 224), 91)
    with torch.no_grad():
        got = m.forward_stages(x.to(DEV))
    for i in range(len(got) - 1):
        key = f"{name}_stem" if i == 0 else f"{name}_stage{i - 1}"
        torch.testing.assert_close(got[i][:, :: sub[i], :: sub[i]].cpu(), g[key], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got[-1].cpu(), g[f"{name}_out"], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_single_block_and_layer_on_the_gpu(dtype):
    from pytorch_models.image.maxvit import MaxViTBlock, block

    blk = MaxViTBlock(32, 64, stride=2).eval()
    with torch.no_grad():
        fill_module(blk, 112)
        bf16_round_(blk)
    x = synth_input("mv_blk", (2, 32, 28, 42), 112).to(torch.bfloat16).float()
    with torch.no_grad():
        want = blk(x)
        wl, _, _ = block(blk.mbconv(x).permute(0, 2, 3, 1), 7)
        want_l = blk.block_layer(wl)
        want_sa = blk.block_layer.sa(blk.block_layer.sa_norm(wl))
    g = blk.to(dtype).to(DEV)
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-4
    with torch.no_grad():
        got = g(x.to(DEV).to(dtype))
        got_l = g.block_layer(wl.to(DEV).to(dtype))
        got_sa = g.block_layer.sa(g.block_layer.sa_norm(wl.to(DEV).to(dtype)))
    assert got.shape == want.shape == (2, 64, 14, 21)
    assert rel(got, want) <= tol and rel(got_l, want_l) <= tol and rel(got_sa, want_sa) <= tol


def test_batch_permutation_and_rerun_are_bit_exact():
    m = _model(SMALL, 113, torch.bfloat16).to(torch.bfloat16).to(DEV)
    x = synth_input("mv_perm", (3, 3, 224, 224), 113).to(DEV)
    perm = torch.tensor([2, 0, 1], device=DEV)
    with torch.no_grad():
        a = m(x)
        b = m(x)
        c = m(x[perm])
    assert torch.equal(a, b)
    assert torch.equal(a[perm], c)


def test_in_place_changes_rebuild_the_derived_tensors():
    from pytorch_models.image import MaxViT

    m = MaxViT(*SMALL).eval()
    with torch.no_grad():
        fill_module(m, 114)
    x = synth_input("mv_upd", (1, 3, 224, 224), 114)
    g = MaxViT(*SMALL).eval().to(DEV)
    with torch.no_grad():
        fill_module(g, 114)
        g(x.to(DEV))  # builds every derived tensor
        blk = m.stages[1][0]
        gblk = g.stages[1][0]
        for mod in (blk, gblk):
            mod.grid_layer.sa.attn_bias.mul_(3.0)
            mod.mbconv.residual[2][1].running_var.mul_(2.0)
            mod.mbconv.residual[1][0].weight.mul_(-1.0)
        m.stem[1].running_mean.add_(0.5)
        g.stem[1].running_mean.add_(0.5)
        want = m(x)
        got = g(x.to(DEV))
    torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-4)


def test_uncovered_inputs_raise():
    from pytorch_models.image import MaxViT

    g = MaxViT(*SMALL).eval().to(DEV)
    with pytest.raises(ValueError, match="224"):
        g(torch.zeros(1, 3, 224, 200, device=DEV))
    with pytest.raises(RuntimeError):
        g(torch.zeros(1, 3, 224, 224))  # CPU input, HIP model
    g.stages[0][0].mbconv.residual[0].train()
    with pytest.raises(NotImplementedError, match="training"):
        g(torch.zeros(1, 3, 224, 224, device=DEV))
