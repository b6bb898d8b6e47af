"""Adversarial fp64 parity of every attention kernel, through the C ABI: peaked logits, planted keys at every tile edge, dense and
broadcast biases on both bias-load paths, leading / interior / checkerboard masks, dead rows.  References, bound and case lists
live in tests/attn_cases.py (tests/test_attn_cases_cpu.py proves on the CPU that a correct kernel satisfies every assertion
made here).  bf16 kernels: |got - want| <= 1.5 x u (A + |want|) per element (bound_ratio <= 1.5); f32 kernels: rtol = atol = 2e-5;
decode: 1e-5.  Dead rows are zeros.  Each test prints the figure it asserts ("RATIO ..." lines, pytest -s).

Measured on an MI355X (worst err / bound per kernel and family): see DESIGN.md, "attention numerics contract"."""
import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from pytorch_models._hip import ops as o

    return o


def _run(ops, case, inp, v=None, bias="case"):
    dt = torch.float32 if case.f32 else torch.bfloat16
    q, k = inp["q"].to(dt).cuda(), inp["k"].to(dt).cuda()
    v = (inp["v"] if v is None else v).to(dt).cuda()
    bias = inp["bias"] if isinstance(bias, str) else bias
    bias = None if bias is None else AC.place_bias(bias, case, "cuda")
    if bias is not None and case.kernel == "tiled_bias" and case.family == "bias":
        want_vec = case.form not in ("off4",) and (case.Lk % 4 == 0 or case.form == "padrow")
        assert AC.bias_vector_path(bias) == want_vec, "the bias layout selects the load path this case is named for"
    fn = ops.attention_f32 if case.f32 else ops.attention
    return fn(q, k, v, case.H, case.causal, bias)


def _dead_elems(case, dead):
    return AC.merge_heads(dead[..., None].expand(-1, -1, -1, case.hd))


def _check(case, got, want, A, dead, what="parity"):
    got = got.float().cpu()
    dm = _dead_elems(case, dead)
    assert torch.isfinite(got).all(), f"{case.id}: non-finite output"
    assert (got[dm] == 0).all(), f"{case.id}: dead rows must be zeros"
    if case.f32:
        err = (got.double() - want).abs()
        print(f"RATIO {case.kernel} {case.family} {case.id} {what} {float((err / (AC.F32_TOL * (1 + want.abs()))).max()):.3f}")
        torch.testing.assert_close(got.double(), want, rtol=AC.F32_TOL, atol=AC.F32_TOL)
    else:
        ratio = AC.bound_ratio(got, want, A)
        print(f"RATIO {case.kernel} {case.family} {case.id} {what} {ratio:.3f}")
        assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_parity(ops, case):
    inp = AC.build(case)
    want, A, dead = AC.reference(case, inp)
    got = _run(ops, case, inp)
    assert got.shape == want.shape
    _check(case, got, want, A, dead)
    assert torch.equal(got, _run(ops, case, inp)), "rerun must give the same bits"


@pytest.mark.parametrize("case", AC.MASKED_CASES, ids=lambda c: c.id)
def test_masked_properties(ops, case):
    """v == 1: every live output within 2^-7 of 1 (row sum and P agree about which keys exist), dead rows zero.
    v one-hot on a masked key: that key carries NO weight - exact zeros wherever it is hidden."""
    inp = AC.build(case)
    _, _, dead = AC.reference(case, inp)
    dm = _dead_elems(case, dead)
    out = _run(ops, case, inp, v=torch.ones_like(inp["v"])).float().cpu()
    assert torch.isfinite(out).all() and (out[dm] == 0).all()
    assert (out[~dm] - 1).abs().max().item() <= 2 ** -7
    # per batch element: the key hidden from the most queries
    vis = inp["keep"].expand(case.B, 1, case.Lq, case.Lk)[:, 0]
    if case.causal:
        vis = vis & torch.ones(case.Lq, case.Lk, dtype=torch.bool).tril()
    v1 = torch.zeros_like(inp["v"])
    hidden = torch.zeros(case.B, case.Lq, dtype=torch.bool)
    for b in range(case.B):
        j = int((~vis[b]).sum(0).argmax())
        v1[b, j] = 1.0
        hidden[b] = ~vis[b, :, j]
    assert hidden.any()
    out = _run(ops, case, inp, v=v1).float().cpu()
    assert torch.isfinite(out).all()
    assert (out[hidden] == 0).all(), f"{case.id}: a masked key carries weight {out[hidden].abs().max().item():.3e}"
    if (~hidden).any():
        assert out[~hidden].abs().max() > 0  # the key is seen where it is visible


@pytest.mark.parametrize("case", AC.DIFFUSE_CASES, ids=lambda c: c.id)
def test_row_sums_are_unbiased(ops, case):
    """v == 1, rows with at least 64 effective keys: exactly 1 (attn_cases.NEFF_EXACT: six sigma of round-to-nearest P errors stay
    inside bf16's rounding interval around 1; a biased P conversion - truncation - lands on 1 - 2^-8)."""
    inp = AC.build(case)
    rows = AC.row_neff(case, inp) >= AC.NEFF_EXACT
    out = AC.split_heads(_run(ops, case, inp, v=torch.ones_like(inp["v"])).float().cpu(), case.H)
    frac = float((out[rows] == 1).float().mean())
    print(f"RATIO {case.kernel} rowsum {case.id} exact-fraction {frac:.4f}")
    assert (out[rows] == 1).all(), f"{case.id}: {1 - frac:.2%} of the diffuse rows are not exactly 1"


@pytest.mark.parametrize("case", [c for c in AC.MASKED_CASES if c.mask == "deadbatch"], ids=lambda c: c.id)
def test_live_rows_do_not_depend_on_dead_rows_elsewhere(ops, case):
    inp = AC.build(case)
    got = _run(ops, case, inp)
    alive = inp["bias"].clone()
    alive[case.B - 1] = alive[0]
    got2 = _run(ops, case, inp, bias=alive)
    assert torch.equal(got[: case.B - 1], got2[: case.B - 1])
    assert (got[case.B - 1] == 0).all() and torch.isfinite(got2).all() and got2[case.B - 1].abs().max() > 0


def test_misaligned_operands_are_refused_not_launched(ops):
    """q 2 bytes past a 16-byte boundary, bias rows shorter than Lk: PM_EALIGN / PM_EINVAL from the argument checks alone."""
    from pytorch_models import _hip

    PM_EINVAL, PM_EALIGN = 1, 4  # include/pm_mi355x.h
    L = _hip.lib()
    buf = torch.zeros(2 * 8 * 128 + 8, dtype=torch.bfloat16, device="cuda")
    q, k = buf[1:1 + 8 * 128], buf[8:8 + 8 * 128]
    o = torch.zeros(8 * 128, dtype=torch.bfloat16, device="cuda")
    rc = L.pm_attention_bf16(q.data_ptr(), 8 * 128, 128, k.data_ptr(), 8 * 128, 128, k.data_ptr(), 8 * 128, 128, o.data_ptr(), 8 * 128, 128,
                             1, 2, 8, 8, 0, None)
    assert rc == PM_EALIGN
    bias = torch.zeros(8 * 8, device="cuda")
    rc = L.pm_attention_bias_bf16(k.data_ptr(), 8 * 128, 128, k.data_ptr(), 8 * 128, 128, k.data_ptr(), 8 * 128, 128, o.data_ptr(), 8 * 128, 128,
                                  1, 2, 8, 8, 0, bias.data_ptr(), 0, 0, 7, None)  # bias rows shorter than Lk
    assert rc == PM_EINVAL


# --------------------------------------------------------------------------------------------------------------- window / grid
def _run_window(ops, c, inp, v=None):
    q, k = inp["q"].bfloat16().cuda(), inp["k"].bfloat16().cuda()
    v = (inp["v"] if v is None else v).bfloat16().cuda()
    bias = None if inp["bias"] is None else inp["bias"].cuda().contiguous()
    return ops.window_attention(q, k, v, c.N, c.Himg, c.Wimg, c.heads, c.ws, c.mode, bias)


@pytest.mark.parametrize("case", AC.WCASES, ids=lambda c: c.id)
def test_window_parity(ops, case):
    inp = AC.build_window(case)
    want, A, dead = AC.reference_window(case, inp)
    got = _run_window(ops, case, inp)
    gw = AC.window_partition(got.float().cpu(), case)
    dm = AC.merge_heads(dead[..., None].expand(-1, -1, -1, 32))
    assert torch.isfinite(gw).all() and (gw[dm] == 0).all(), "dead rows are zeros"
    ratio = AC.bound_ratio(gw, want, A)
    print(f"RATIO window {'dead' if case.dead else 'bias' if case.bias_amp else 'scale'} {case.id} parity {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"
    assert torch.equal(got, _run_window(ops, case, inp))
    # v == 1: rows sum to one over exactly the keys that exist (key >= L padding, -inf bias entries)
    out = AC.window_partition(_run_window(ops, case, inp, v=torch.ones_like(inp["v"])).float().cpu(), case)
    assert (out[dm] == 0).all() and (out[~dm] - 1).abs().max().item() <= 2 ** -7
    if case.dead:  # key 0 of head 0 is masked for every query: one-hot v there -> head 0 is exactly zero
        L = case.ws * case.ws
        vw = torch.zeros(want.shape[0], L, 32 * case.heads)
        vw[:, 0, :] = 1.0
        out = AC.window_partition(_run_window(ops, case, inp, v=AC.window_unpartition(vw, case)).float().cpu(), case)
        assert torch.isfinite(out).all() and (out[..., :32] == 0).all()
        if case.heads > 1:
            assert out[..., 32:].abs().max() > 0


# --------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("case", AC.DCASES, ids=lambda c: c.id)
def test_decode_parity(ops, case):
    inp = AC.build_decode(case)
    want, _ = AC.reference_decode(case, inp)
    q, k, v = inp["q"].cuda(), inp["k"].bfloat16().cuda(), inp["v"].bfloat16().cuda()
    got = ops.dec_attention(q, k, v, case.lk)
    err = (got.cpu().double() - want).abs()
    print(f"RATIO dec_attention {case.family} {case.id} parity {float((err / (AC.DEC_TOL * (1 + want.abs()))).max()):.3f}")
    torch.testing.assert_close(got.cpu().double(), want, rtol=AC.DEC_TOL, atol=AC.DEC_TOL)
    assert torch.equal(got, ops.dec_attention(q, k, v, case.lk))


@pytest.mark.parametrize("case", AC.DCASES, ids=lambda c: c.id)
@pytest.mark.parametrize("kv32", [0, 1])
def test_decode_fused_parity(case, kv32):
    """pm_dec_attention_fused / _fused_kv32, cross form over the first lk keys.  The block's query is LayerNorm(x) W^T + b: W = 0
    makes it the bias exactly, so that the planted key is planted for the query the kernel really uses."""
    from pytorch_models._hip import check, lib

    L = lib()
    B, H, T, d = case.B, case.H, case.T, 512
    inner = H * 64
    inp = AC.build_decode(case, per_batch_q=False)
    want, _ = AC.reference_decode(case, inp)
    kdt = torch.float32 if kv32 else torch.bfloat16
    x = AC.synth_input("adv_dx", (B, d), 5).cuda()
    g, be = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    w = torch.zeros(inner, d, dtype=torch.bfloat16, device="cuda")
    qb = inp["q"][0].contiguous().cuda()
    kc, vc = inp["k"].to(kdt).cuda(), inp["v"].to(kdt).cuda()
    fused = L.pm_dec_attention_fused_kv32 if kv32 else L.pm_dec_attention_fused

    def go():
        att = torch.full((B, inner), float("nan"), device="cuda")
        check(fused(x.data_ptr(), d, g.data_ptr(), be.data_ptr(), 1e-5, w.data_ptr(), qb.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                    H * T * 64, T * 64, 64, None, case.lk, T, att.data_ptr(), B, H, 0, None), "fused")
        return att

    got = go()
    err = (got.cpu().double() - want).abs()
    name = "dec_fused_kv32" if kv32 else "dec_fused"
    print(f"RATIO {name} {case.family} {case.id} parity {float((err / (AC.DEC_TOL * (1 + want.abs()))).max()):.3f}")
    torch.testing.assert_close(got.cpu().double(), want, rtol=AC.DEC_TOL, atol=AC.DEC_TOL)
    assert torch.equal(got, go())


# --------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("mask", AC.MASKS + ("deadbatch",))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_mha_bool_masks_match_the_cpu_form(mask, causal, dtype):
    """The same mask families as a BOOLEAN keep-mask through MHA (converted to a -inf bias on the way): finite everywhere, dead
    rows are out_proj's bias (the attention output is zero there), live rows match the CPU form per sequence (bf16: rel-L2 <= 1e-2,
    the model tolerance; fp32 parameters: 2e-5)."""
    import copy

    from pytorch_models.transformer import MHA
    from synthweights import bf16_round_, fill_module

    case = AC.Case("tiled_bias", 3, 2, 197, 200, family="mask", scale=1.0, form="BH", mask=mask, causal=causal)
    keep = AC.keep_mask(case)
    m = MHA(128, 2).eval()
    fill_module(m, 91)
    bf16_round_(m)
    q = AC.bf16r(AC.synth_input("adv_mha_q", (case.B, case.Lq, 128), 92))
    kv = AC.bf16r(AC.synth_input("adv_mha_kv", (case.B, case.Lk, 128), 93))
    want = m(q, kv, attn_bias=keep, causal=causal)
    vis = keep.expand(case.B, 1, case.Lq, case.Lk)[:, 0]
    if causal:
        vis = vis & torch.ones(case.Lq, case.Lk, dtype=torch.bool).tril()
    dead = ~vis.any(-1)
    assert torch.isfinite(want).all() and (want[dead] == m.out_proj.bias).all()
    want64 = copy.deepcopy(m).double()(q.double(), kv.double(), attn_bias=keep, causal=causal)
    g = copy.deepcopy(m).to(dtype).cuda()
    got = g(q.to(dtype).cuda(), kv.to(dtype).cuda(), attn_bias=keep.cuda(), causal=causal).float().cpu()
    assert torch.isfinite(got).all()
    if dead.any():
        torch.testing.assert_close(got[dead], want[dead], rtol=2 ** -8, atol=1e-6)  # the bias, through one bf16 store at most
    for b in range(case.B):
        live = ~dead[b]
        if not live.any():
            continue
        if dtype == torch.float32:  # against the CPU form in float64, so that the tolerance is the kernel's alone
            torch.testing.assert_close(got[b][live].double(), want64[b][live], rtol=AC.F32_TOL, atol=AC.F32_TOL)
        else:
            rel = float((got[b][live] - want[b][live]).norm() / want[b][live].norm())
            assert rel <= 1e-2, (b, rel)


@pytest.mark.parametrize("n_heads", [2, 4])  # head_dim 64: attn_fwd_hd64<causal, bias>; 32: the generic kernel
def test_left_padded_causal_encoder_stays_finite(n_heads):
    """Two pre-norm encoder layers, bool key-padding mask with LEFT padding through MHA + causal: the first pad queries of a padded
    sequence see no key.  A NaN there would be a V row of layer 2 and poison every query of the sequence (0 x NaN on the matrix
    pipe).  Finite everywhere; live rows match the CPU form at the model tolerance (rel-L2 <= 1e-2 per sequence)."""
    import copy

    from pytorch_models.transformer import Encoder
    from synthweights import bf16_round_, fill_module

    B, L, d = 3, 200, 128
    pads = (0, 65, 130)
    m = Encoder(2, d, n_heads).eval()
    fill_module(m, 77)
    bf16_round_(m)
    x = AC.bf16r(AC.synth_input("adv_enc_x", (B, L, d), 78))
    keep = torch.ones(B, 1, L, L, dtype=torch.bool)
    for b, p in enumerate(pads):
        keep[b, :, :, :p] = False

    def run(layers, x, keep):
        for layer in layers:
            x = x + layer.sa(layer.sa_norm(x), attn_bias=keep, causal=True)
            x = x + layer.mlp(layer.mlp_norm(x))
        return x

    want = run(m, x, keep)
    assert torch.isfinite(want).all()
    g = copy.deepcopy(m).to(torch.bfloat16).cuda()
    got = run(g, x.bfloat16().cuda(), keep.cuda()).float().cpu()
    assert torch.isfinite(got).all()
    for b, p in enumerate(pads):
        rel = float((got[b, p:] - want[b, p:]).norm() / want[b, p:].norm())
        print(f"RATIO encoder{n_heads} e2e seq{b} rel-L2 {rel:.3e}")
        assert rel <= 1e-2, (b, rel)
