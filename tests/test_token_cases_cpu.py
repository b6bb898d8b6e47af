"""Keeps the adversarial token-path suite (tests/test_hip_token_adversarial.py) honest without a GPU: its float64 references are
torch's own forms (F.layer_norm + F.gelu + F.linear, F.conv2d, softmax attention over LayerNorm'd rows), a correct kernel (fp32
arithmetic with the kernels' rounding points, torch's summation order) satisfies every assertion of the GPU suite at 1.0 x the bound
and equals the exact families bit for bit, every defect in token_cases.MUTANTS is rejected DECISIVELY (a bit difference in an exact
case or more than 10 x the bound) by a case of the family aimed at it, the case lists reach every kernel path they are named for,
every family keeps its preconditions (exactness, saturation, needle dominance, the offset ratios), and the host-only
pm_mixer_token_mix_plan sends every token-mixing case where the table says."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import token_cases as TC

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = TC.build(case)
            cache[case.id] = (inp, TC.reference(case, inp))
        return cache[case.id]

    return get


def _lib():
    from pytorch_models import _hip

    return _hip.lib()


# --------------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_reach_every_named_path():
    assert set(TC.REQUIRED_PATHS) == set(TC.OPS)
    for op, need in TC.REQUIRED_PATHS.items():
        have = set().union(*(TC.paths(c) for c in TC.CASES if c.op == op))
        assert need <= have, (op, need - have)
    fams = {"token_mix": {"exact", "needle", "poison", "perm"}, "ln_mean": {"exact", "poison"}, "transpose": {"move"},
            "cls_head_gemm": {"exact", "poison"}, "cls_attend": {"exact", "needle", "offset", "const", "poison", "perm"},
            "vit_tokens": {"exact", "locate", "locpe", "poison"}, "mean_ln": {"poison"}, "s2d": {"locate", "poison"},
            "se_gate": {"poison"}, "mean_rows": {"poison"}, "rmsnorm": {"offset", "poison"}, "geglu": {"poison"}}
    for op in TC.OPS:
        assert {c.family for c in TC.CASES if c.op == op} == fams[op], op
    assert len({c.id for c in TC.CASES}) == len(TC.CASES)
    assert {c.d["ratio"] for c in TC.CASES if c.op == "cls_attend" and c.family == "offset"} == {4, 64, 4096}
    # a few workgroups each: the largest operand is the 127-image ViT batch (127 x 3 x 16 x 16 pixels) resp. 65 x 1024 rows
    assert max(t.numel() for c in TC.CASES for t in TC.build(c).values() if isinstance(t, torch.Tensor)) <= 1 << 20


def test_mutant_table_is_the_issues():
    want = {"token_mix": {"pad_token_live", "pad_hidden_live", "stats_image0", "b2_by_channel", "gelu_before_bias", "row_sums_unrounded",
                          "slab_offset", "resid_dropped"},
            "cls_attend": {"mean_dropped", "cm_unrounded", "tail_rows_live", "no_rescale", "rstd_once", "head_pad_leak"},
            "cls_head_gemm": {"group_stride", "bias_group0", "wave3_lost", "trunc_store"},
            "vit_tokens": {"gy_gx_swapped", "pe_shifted_by_cls", "cls_every_row", "pixel_trunc", "generic_tail_live", "channel_stride"},
            "rows": {"ln_of_mean_for_mean_of_ln", "s2d_quadrants", "se_div_ntiles", "rms_centred", "geglu_halves_swapped", "transpose_ldy"}}
    got = {}
    for m, (op, _) in TC.MUTANT_OF.items():
        got.setdefault(op if op in want else "rows", set()).add(m)
    assert got == want


# --------------------------------------------------------------------------------------------------------------- path authority
def test_token_mix_cases_go_where_the_table_says():
    """pm_mixer_token_mix_plan (built from the launcher's own mx_pick_nb / mx_region_a / mx_lds_bytes) against the table."""
    from pytorch_models._hip import ops

    for c in (c for c in TC.CASES if c.op == "token_mix"):
        T, Dt, C = c.d["T"], c.d["Dt"], c.d["C"]
        rep = ops.mixer_token_mix_plan(T, Dt, C)
        assert rep == TC.tm_plan(T, Dt, C), (c.id, rep)
        assert ops.mixer_token_mix_supported(T, Dt, C) and rep["lds"] <= TC.MX_LDS_MAX
        assert TC.paths(c, rep) == TC.paths(c)
    for T, Dt, C in TC.REFUSED_TOKEN_MIX:
        assert ops.mixer_token_mix_plan(T, Dt, C) == {"refused": 2} and TC.tm_plan(T, Dt, C) is None and not ops.mixer_token_mix_supported(T, Dt, C)
    plan = ops.mixer_token_mix_plan
    assert plan(16, 256, 128)["NB"] == 4 and plan(16, 32, 64)["NB"] == 2 and plan(15, 288, 192)["NB"] == 2
    assert plan(16, 640, 128)["NB"] == 2 and plan(16, 512, 128)["NB"] == 2 and plan(16, 480, 128)["NB"] == 4  # NB 2 by LDS from Dt 512 on
    assert plan(16, 992, 128)["lds"] == 161792 and "refused" in plan(16, 1024, 128)   # the last served and the first refused Dt at T 16
    assert plan(112, 32, 128)["scratch"] and not plan(128, 32, 128)["scratch"] and plan(128, 32, 128)["region_a"] == 34816
    assert [plan(T, 32, 64)["nk1"] for T in (1, 16, 49, 128, 196, 257)] == [1, 1, 4, 8, 13, 17]
    assert [plan(16, Dt, 64)["nk2"] for Dt in (32, 128, 160, 288)] == [2, 8, 10, 18] and [plan(16, Dt, 64)["nd"] for Dt in (32, 256, 288)] == [1, 8, 9]
    assert [plan(T, 32, 64)["nt"] for T in (32, 256, 257)] == [1, 8, 9]


def test_se_gate_refuses_what_its_lds_cannot_hold():
    """(C + R) * 4 bytes of dynamic LDS above 64 KiB: refused by the argument checks (host side, nothing is launched)."""
    L = _lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 1, 16384, 1, None) == 2
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 1, 16383, 2, None) == 2 and L.pm_se_gate(p, 1, 1, p, p, p, p, p, 1, 12289, 4096, None) == 2
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 0, 16383, 1, None) == 0  # N = 0 at the limit: accepted, nothing to do
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 0, 16385, 1, None) == 2


# --------------------------------------------------------------------------------------------------------------- independent forms
def test_token_mix_reference_is_torchs_mixer_block():
    case = next(c for c in TC.CASES if c.id == "token_mix-poison-T49-Dt128-C128-N3-rows")
    inp = TC.build(case)
    x = inp["x"].double()
    v, m = torch.var_mean(x, -1, unbiased=False)
    inp["stats"] = torch.stack([m, torch.rsqrt(v + TC.EPS)], -1).reshape(-1, 2)  # float64 statistics: the reference takes what it is given
    xn = F.layer_norm(x, (128,), inp["gamma"].double(), inp["beta"].double(), TC.EPS)
    want = x + F.linear(F.gelu(F.linear(xn.transpose(1, 2), inp["w1"].double(), inp["b1"].double())), inp["w2"].double(),
                        inp["b2"].double()).transpose(1, 2)
    ref = TC.tm_reference(case, inp)
    torch.testing.assert_close(ref["want"], want, rtol=1e-12, atol=1e-12)
    assert bool((ref["bound"] > 0).all()) and float(ref["bound"].max()) < 1.0


@pytest.mark.parametrize("cid", ["vit_tokens-poison-P16-H32-W48-N1-d64-cls-ldpad0", "vit_tokens-poison-P14-H28-W42-N2-d4-cls-ldpad0-generic"])
def test_vit_reference_is_torchs_conv2d(cid):
    case = next(c for c in TC.CASES if c.id == cid)
    inp = TC.build(case)
    P, dd, K = case.d["P"], case.d["d"], TC.vit_geometry(case)["K"]
    w = inp["w"].double()[:, :K].view(dd, 3, P, P)
    tok = F.conv2d(TC.bf16r(inp["imgs"]).double(), w, inp["bias"].double(), stride=P).flatten(2).transpose(1, 2) + inp["pe"].double()
    want = torch.cat([TC.bf16r(inp["cls"]).double().expand(case.d["N"], 1, dd), tok], 1)
    torch.testing.assert_close(TC.vit_reference(case, inp)["want"], want, rtol=1e-12, atol=1e-12)


def test_cls_attend_reference_is_softmax_attention_over_normalised_rows():
    case = next(c for c in TC.CASES if c.id == "cls_attend-poison-L65-d192-H16-N3")
    inp = TC.build(case)
    xh = F.layer_norm(inp["x"].double(), (192,), eps=TC.EPS)
    p = torch.softmax(TC.ATT_SCALE * torch.einsum("nhc,nlc->nhl", inp["u"].double(), xh), -1)
    torch.testing.assert_close(TC.cls_attend_reference(case, inp)["want"], torch.einsum("nhl,nlc->nhc", p, xh), rtol=1e-10, atol=1e-10)


def test_row_reduction_references_are_torchs():
    get = lambda cid: next(c for c in TC.CASES if c.id == cid)  # noqa: E731
    c = get("mean_ln-poison-C37-HW9-N3-ldpad3-xdtbf16-ydtbf16")
    inp = TC.build(c)
    want = F.layer_norm(inp["x"][..., :37].double().mean(1), (37,), inp["gamma"].double(), inp["beta"].double(), TC.EPS)
    torch.testing.assert_close(TC.reference(c, inp)["want"], want, rtol=1e-12, atol=1e-12)
    c = get("s2d-poison-H6-W10-C37-N2-ldpad3-xdtbf16-ydtbf16")
    inp = TC.build(c)
    y = F.layer_norm(inp["x"][..., :37].double(), (37,), inp["gamma"].double(), inp["beta"].double(), TC.EPS)
    want = y.view(2, 3, 2, 5, 2, 37).permute(0, 1, 3, 2, 4, 5).reshape(30, 4 * 37)  # (n, i, j, dh, dw, c)
    ref = TC.reference(c, inp)
    torch.testing.assert_close(ref["want"][:, :148], want, rtol=1e-12, atol=1e-12)
    assert bool((ref["want"][:, 148:] == 0).all()) and bool((ref["bound"][:, 148:] == 0).all())  # the pad columns: exactly zero
    c = get("se_gate-poison-ntiles3-hw49-C64-R5-N3")
    inp = TC.build(c)
    m = inp["psum"].double().sum(1) / 49
    want = torch.sigmoid(F.linear(F.silu(F.linear(m, inp["w1"].double(), inp["b1"].double())), inp["w2"].double(), inp["b2"].double()))
    torch.testing.assert_close(TC.reference(c, inp)["want"], want, rtol=1e-12, atol=1e-12)
    c = get("geglu-poison-F136-M5-ldpad8")
    inp = TC.build(c)
    h = inp["h"].double()
    torch.testing.assert_close(TC.reference(c, inp)["want"], F.gelu(h[:, :136], approximate="tanh") * h[:, 136:272], rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------- the families' conditions
@pytest.mark.parametrize("case", [c for c in TC.CASES if c.family in ("exact", "needle", "locate", "locpe", "offset", "const")], ids=lambda c: c.id)
def test_families_keep_their_preconditions(solved, case):
    inp, ref = solved(case)
    assert TC.exact_preconditions(case, inp, ref) == []
    if case.family in ("exact", "locpe") or (case.family == "locate" and case.op == "vit_tokens"):
        assert bool((ref["bound"] == 0).all())


def test_a_broken_precondition_is_noticed():
    case = next(c for c in TC.CASES if c.op == "token_mix" and c.family == "exact")
    inp = TC.build(case)
    inp["b1"] = inp["b1"] / 32  # +-2: the pre-activations leave the saturated range
    assert TC.exact_preconditions(case, inp, TC.reference(case, inp))


# --------------------------------------------------------------------------------------------------------------- stand-in and mutants
@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_a_correct_kernel_passes_at_one_times_the_bound(solved, case):
    inp, ref = solved(case)
    ok, r, msg = TC.verify(case, inp, ref, TC.StandIn(), margin=1.0)
    assert ok, f"{case.id}: {msg}"
    assert r <= 1.0


@pytest.mark.parametrize("mutant", TC.MUTANTS)
def test_each_mutant_is_rejected_decisively(solved, mutant):
    op, fam = TC.MUTANT_OF[mutant]
    aimed = [c for c in TC.CASES if c.op == op and c.family == fam]
    assert aimed
    be = TC.StandIn(mutant)
    verdicts = [(c, *TC.verify(c, *solved(c), be)[:2]) for c in aimed]
    exact = {"exact", "locate", "locpe", "move"}
    decisive = [c.id for c, ok, r in verdicts if not ok and (r > 10 or (c.family in exact and r == float("inf")))]
    assert decisive, f"{mutant}: not rejected decisively by any {fam} case of {op}: {[(c.id, ok, r) for c, ok, r in verdicts]}"


def test_embedded_buffers_are_aligned_and_guarded():
    for dt in (torch.float32, torch.bfloat16):
        t = torch.arange(30.0).view(2, 3, 5).to(dt)
        buf, v = TC.embedded(t, "cpu")
        assert torch.equal(v, t) and v.data_ptr() % 16 == 0 and int(torch.isnan(buf.float()).sum()) == buf.numel() - t.numel()
        buf, v = TC.embedded(torch.empty(2, 5, 3, dtype=dt), "cpu", sentinel=True)
        v.fill_(1.0)
        assert TC.sentinels_intact(buf, v)
        buf[-1] = 0.0
        assert not TC.sentinels_intact(buf, v)
