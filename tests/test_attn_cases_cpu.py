"""Keeps the adversarial attention suite (tests/test_hip_attention_adversarial.py) honest without a GPU: its reference is
F.scaled_dot_product_attention's, its dead-row contract is what the installed torch does on the CPU, its bf16 bound is satisfiable by
a correct kernel on every case the GPU file runs (the case lists are shared through tests/attn_cases.py), and the bound rejects
errors that the older metrics accept."""
import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC

torch.set_grad_enabled(False)


def _sdpa(inp, case, dtype):
    qh, kh, vh = (AC.split_heads(inp[n], case.H).to(dtype) for n in ("q", "k", "v"))
    bias = None if inp["bias"] is None else inp["bias"].to(dtype)
    if case.causal and bias is not None:  # SDPA takes one or the other: fold the triangle into the bias
        tri = torch.ones(case.Lq, case.Lk, dtype=torch.bool).tril()
        bias = bias.expand(-1, -1, case.Lq, case.Lk).masked_fill(~tri, AC.NEG_INF)
        return AC.merge_heads(F.scaled_dot_product_attention(qh, kh, vh, bias))
    return AC.merge_heads(F.scaled_dot_product_attention(qh, kh, vh, bias, 0.0, case.causal))


def test_every_case_reaches_the_kernel_it_names():
    for c in AC.CASES:
        assert AC.expected_kernel(c) == c.kernel, c.id
    kernels = {c.kernel for c in AC.CASES}
    assert kernels == {"head", "tiled", "tiled_bias", "generic_bf16", "generic_f32", "mfma_f32"}
    for kern in ("tiled_bias", "generic_bf16", "generic_f32"):  # every masked-capable kernel meets every mask family and dead rows
        masks = {(c.mask, c.causal) for c in AC.CASES if c.kernel == kern}
        assert {m for m, _ in masks} >= set(AC.MASKS) | {"deadbatch"}, kern
        assert any(m.startswith("lead") and causal for m, causal in masks if m), kern
    assert {c.form for c in AC.CASES if c.kernel == "tiled_bias" and c.family == "bias"} == set(AC.BIAS_FORMS)
    assert {c.scale for c in AC.CASES if c.f32 and c.family == "scale"} == set(AC.F32_SCALES)


def test_bias_forms_cover_both_load_paths():
    """Layouts as place_bias() builds them (on the CPU here: the same strides and offsets): the 16-byte path with Lk % 4 == 0 and
    with a ragged last group (padded rows), the scalar path for Lk % 4 != 0, for a base 4 bytes past a 16-byte boundary."""
    seen = set()
    for c in AC.CASES:
        if c.kernel != "tiled_bias" or c.family != "bias":
            continue
        b = AC.place_bias(AC.build(c)["bias"], c, "cpu")
        assert b.shape[2:] == (c.Lq, c.Lk) and b.stride(3) == 1 and b.stride(2) >= c.Lk
        if c.form != "off4":  # the CPU allocator gives 64-byte bases like the device one; off4 asserts its own offset
            assert b.data_ptr() % 16 == 0
        seen.add((c.form, c.Lk % 4 == 0, AC.bias_vector_path(b)))
    assert ("BH", True, True) in seen and ("BH", False, False) in seen
    assert ("padrow", False, True) in seen and ("off4", True, False) in seen and ("expand", True, True) in seen


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_every_gpu_case(case):
    inp = AC.build(case)
    want, A, dead = AC.reference(case, inp)
    dead_m = AC.merge_heads(dead[..., None].expand(-1, -1, -1, case.hd))
    assert torch.isfinite(want).all() and (want[dead_m] == 0).all() and not dead.all()
    assert dead.any() == (case.mask == "deadbatch" or (case.causal and (case.mask or "").startswith("lead"))), "dead rows where planned"
    # the reference IS F.scaled_dot_product_attention in float64 on live rows
    sd64 = _sdpa(inp, case, torch.float64)
    assert (sd64[~dead_m] - want[~dead_m]).abs().max() <= 1e-12
    if case.f32:  # the f32 kernels' tolerance is satisfiable: fp32 SDPA itself meets it
        sd32 = _sdpa(inp, case, torch.float32).double()
        torch.testing.assert_close(sd32[~dead_m], want[~dead_m], rtol=AC.F32_TOL, atol=AC.F32_TOL)
    else:  # the bf16 bound is satisfiable: the kernels' arithmetic, emulated, stays inside 1.0 x of it
        qh, kh, vh = (AC.split_heads(inp[n], case.H) for n in ("q", "k", "v"))
        emu = AC.merge_heads(AC.emulate_bf16_kernel(qh, kh, vh, inp["bias"], case.causal))
        ratio = AC.bound_ratio(emu, want, A)
        assert ratio <= 1.0, f"{case.id}: emulation at {ratio:.3f} x bf16_bound"


@pytest.mark.parametrize("case", AC.WCASES, ids=lambda c: c.id)
def test_window_cases_reference_and_bound(case):
    inp = AC.build_window(case)
    want, A, dead = AC.reference_window(case, inp)
    assert dead.any() == case.dead and torch.isfinite(want).all()
    qh, kh, vh = (AC.split_heads(AC.window_partition(inp[n], case), case.heads) for n in ("q", "k", "v"))
    bias = None if inp["bias"] is None else inp["bias"][None]
    sd = AC.merge_heads(F.scaled_dot_product_attention(qh.double(), kh.double(), vh.double(), None if bias is None else bias.double()))
    dead_m = AC.merge_heads(dead[..., None].expand(-1, -1, -1, 32))
    assert (sd[~dead_m] - want[~dead_m]).abs().max() <= 1e-12
    ratio = AC.bound_ratio(AC.merge_heads(AC.emulate_bf16_kernel(qh, kh, vh, bias)), want, A)
    assert ratio <= 1.0, f"{case.id}: emulation at {ratio:.3f} x bf16_bound"


@pytest.mark.parametrize("case", AC.DCASES, ids=lambda c: c.id)
@pytest.mark.parametrize("per_batch_q", [True, False])
def test_decode_cases_reference(case, per_batch_q):
    inp = AC.build_decode(case, per_batch_q)
    want, _ = AC.reference_decode(case, inp)
    q = inp["q"].view(case.B, case.H, 1, 64)
    k, v = inp["k"][:, :, : case.lk], inp["v"][:, :, : case.lk]
    sd64 = F.scaled_dot_product_attention(q.double(), k.double(), v.double()).reshape(case.B, -1)
    assert (sd64 - want).abs().max() <= 1e-12
    sd32 = F.scaled_dot_product_attention(q, k, v).reshape(case.B, -1).double()
    torch.testing.assert_close(sd32, want, rtol=AC.DEC_TOL, atol=AC.DEC_TOL)
    if case.family == "planted":  # the planted key dominates: its weight is above one half for every (b, h)
        p = torch.softmax((q.double() @ k.double().transpose(-1, -2)) / 8.0, -1)
        assert p.max(-1).values.min() > 0.5


def test_dead_row_contract_is_the_cpu_references():
    """Dead rows are ZEROS because that is what F.scaled_dot_product_attention and this project's own CPU form return with the
    installed torch - fp32 and fp64, -inf float bias and boolean mask - not because the suite prefers zeros."""
    from pytorch_models.transformer import MHA

    case = next(c for c in AC.CASES if c.kernel == "tiled_bias" and c.mask == "lead65" and c.causal and c.Lk == 133)
    inp = AC.build(case)
    _, _, dead = AC.reference(case, inp)
    dead_m = AC.merge_heads(dead[..., None].expand(-1, -1, -1, case.hd))
    assert dead_m.any() and not dead_m.all()
    for dt in (torch.float32, torch.float64):
        got = _sdpa(inp, case, dt)
        assert torch.isfinite(got).all() and (got[dead_m] == 0).all(), dt
    qh, kh, vh = (AC.split_heads(inp[n], case.H) for n in ("q", "k", "v"))
    keep = inp["keep"] & torch.ones(case.Lq, case.Lk, dtype=torch.bool).tril()
    got = AC.merge_heads(F.scaled_dot_product_attention(qh, kh, vh, keep))
    assert torch.isfinite(got).all() and (got[dead_m] == 0).all()
    # pytorch_models._cpu.mha: the rows of a fully masked query are out_proj's bias (attention output zero), and finite
    m = MHA(128, 2).eval()
    x = AC.bf16r(torch.randn(2, 9, 128, generator=torch.Generator().manual_seed(1)))
    keep = torch.ones(2, 1, 9, 9, dtype=torch.bool)
    keep[1, :, :, :3] = False
    y = m(x, attn_bias=keep, causal=True)
    assert torch.isfinite(y).all()
    torch.testing.assert_close(y[1, :3], m.out_proj.bias.expand(3, -1), rtol=0, atol=0)
    assert not torch.equal(y[0, :3], m.out_proj.bias.expand(3, -1))


def _close_bf16_accepts(got, want, rel=1.5e-2) -> bool:
    """tests/test_hip_kernels.py::close_bf16"""
    rms = want.square().mean().sqrt().item()
    try:
        torch.testing.assert_close(got.float(), want.float(), rtol=rel, atol=rel * max(rms, 1e-6))
        return True
    except AssertionError:
        return False


def test_new_metric_rejects_what_the_old_ones_accept():
    """Peaked softmax (score deviation 30).  (a) one key that should be masked takes weight w in one row, w chosen between the two
    tolerances: close_bf16(rel=1.5e-2) accepts, 1.5 x bf16_bound rejects.  (b) >= 10^4 rows, one replaced by its neighbour: the
    global rel-L2 < 2e-2 of the block / model tests accepts, the bound rejects.  Both halves are asserted."""
    case = AC.Case("tiled", 24, 8, 448, 257, scale=30.0)
    inp = AC.build(case)
    want, A, _ = AC.reference(case, inp)
    rms = want.square().mean().sqrt().item()
    # (a) row (b, i), head 0: move weight w from the softmax onto key j:  got = (1 - w) want + w v_j
    b, i, j = 1, 77, 200
    vj = inp["v"][b, j, :64].double()
    row, arow = want[b, i, :64], A[b, i, :64]
    d = (vj - row).abs()
    # the largest w that close_bf16 still accepts everywhere, halved; it must stay above what the bound allows somewhere
    w = 0.5 * float(((1.5e-2 * row.abs() + 1.5e-2 * rms) / d.clamp_min(1e-30)).min())
    assert 1e-3 < w < 0.5
    bad = want.clone()
    bad[b, i, :64] = (1 - w) * row + w * vj
    assert _close_bf16_accepts(bad, want), "old elementwise metric accepts the mis-masked key"
    assert AC.bound_ratio(bad, want, A) > 1.5, "the bound rejects it"
    assert float((w * d / (AC.U_BF16 * (arow + row.abs()))).max()) > 1.5
    # (b) one whole query row replaced by its neighbour's
    rows = want.shape[0] * want.shape[1] * case.H
    assert rows >= 10_000
    bad = want.clone()
    bad[2, 100] = want[2, 101]
    rel_l2 = float((bad - want).norm() / want.norm())
    assert 0 < rel_l2 < 2e-2, "old global metric accepts a wrong row"
    assert AC.bound_ratio(bad, want, A) > 1.5
    # and the metric is not simply strict: the emulated kernel passes it on the same case
    qh, kh, vh = (AC.split_heads(inp[n], case.H) for n in ("q", "k", "v"))
    assert AC.bound_ratio(AC.merge_heads(AC.emulate_bf16_kernel(qh, kh, vh)), want, A) <= 1.0


@pytest.mark.parametrize("case", AC.DIFFUSE_CASES, ids=lambda c: c.id)
def test_unbiased_row_sum_property_is_satisfiable_and_has_teeth(case):
    """v == 1 on rows with n_eff >= 64: the emulated round-to-nearest kernel returns exactly 1 (so the GPU assertion can hold),
    the same arithmetic with P truncated does not (so it is not vacuous) - while the truncating form passes the 2^-7 property."""
    inp = AC.build(case)
    rows = AC.row_neff(case, inp) >= AC.NEFF_EXACT
    assert rows.float().mean() > 0.25, "the case has diffuse rows"
    qh, kh = (AC.split_heads(inp[n], case.H) for n in ("q", "k"))
    ones = torch.ones_like(AC.split_heads(inp["v"], case.H))
    good = AC.emulate_bf16_kernel(qh, kh, ones, inp["bias"], case.causal)
    assert (good[rows] == 1).all()
    bad = AC.emulate_bf16_kernel(qh, kh, ones, inp["bias"], case.causal, truncate=True)
    assert (bad[rows] - 1).abs().max() <= 2 ** -7 and (bad[rows] != 1).float().mean() > 0.9
