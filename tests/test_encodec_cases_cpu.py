"""Keeps the adversarial EnCodec suite (tests/test_hip_encodec_adversarial.py) honest without a GPU: its float64 references are
F.conv1d / F.conv_transpose1d / nn.LSTM / F.group_norm's, a correct kernel (fp32 arithmetic in another summation order) satisfies
every assertion of the GPU suite at 1.0 x the bound and equals the exact family bit for bit, every defect in
encodec_cases.MUTANTS is rejected by a case of the family aimed at it, the case lists reach every kernel path they are named for,
no case is a refusal in disguise, and the families keep their conditions (ties at every stage of the exact RVQ family, planted
pairs decided at 4 x and undecided at 0.25 x the threshold, at most 1 % undecided decisions among the Gaussian rows,
|mean| / sigma = 4096 in GroupNorm's offset family)."""
import pytest
import torch
import torch.nn.functional as F

import encodec_cases as EC

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = EC.build(case)
            cache[case.id] = (inp, EC.reference(case, inp))
        return cache[case.id]

    return get


# --------------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_reach_every_named_path():
    for op, need in EC.REQUIRED_PATHS.items():
        have = set().union(*(EC.paths(c) for c in EC.CASES if c.op == op))
        assert need <= have, (op, need - have)
    fams = {"conv": {"exact", "cancel", "poison", "batch"}, "convT": {"exact", "poison", "batch"},
            "lstm": {"onehot", "saturate", "poison", "batch"}, "rvq_encode": {"exact", "gaussian", "poison", "batch"},
            "rvq_decode": {"exact", "poison", "batch"}, "groupnorm": {"exact", "offset", "small", "poison", "batch"},
            "scale": {"exact", "poison", "batch"}}
    for op in EC.OPS:
        assert {c.family for c in EC.CASES if c.op == op} == fams[op], op
    assert {c.sub for c in EC.CASES if c.op in ("conv", "convT") and c.family == "exact"} == {"", "ramp"}
    for c in EC.CASES:
        assert EC.abi_refusal(c) is None, c.id
        assert c.family != "batch" or (c.T if c.op == "rvq_encode" else c.B) > 1, c.id
    assert len(EC.REFUSED_RC) == len(EC.REFUSED) and set(EC.REFUSED_RC) <= {1, 2}
    for c in EC.REFUSED:
        assert EC.abi_refusal(c), c.id
    # every case is milliseconds on the device: the largest operand is the 257-chunk GroupNorm clip
    assert max(c.B * c.T * max(c.C, 1) for c in EC.CASES) == 131200 * 32


def test_mutant_tables_are_complete():
    assert set(EC.MUTANT_FAMILY) == set(EC.MUTANTS) == set(EC.MUTANT_OP)
    assert {"mirror_edge", "replicate", "extra_pad_zero", "elu_after", "tap_carry", "clip_cross", "up_phase_swap", "trim_shift", "bias_lane",
            "gate_order", "stale_acc", "c_not_reset", "row_clamp", "tie_highest", "wave_tie", "no_norm", "resid_stale", "onepass",
            "var_unbiased", "chan_step", "eps_outside", "square_first"} == set(EC.MUTANTS)


# --------------------------------------------------------------------------------------------------------------- independent forms
@pytest.mark.parametrize("case", [c for c in EC.CASES if c.op == "conv" and c.family in ("poison", "cancel")], ids=lambda c: c.id)
def test_conv_reference_is_torchs_reflect_padded_conv1d(solved, case):
    inp, ref = solved(case)
    x = inp["x"].double().transpose(1, 2)
    x = F.elu(x) if case.elu else x
    w = inp["w"].double().view(case.Cout, case.k, case.C).permute(0, 2, 1)
    want = F.conv1d(F.pad(x, (case.left, case.right), mode="reflect"), w, None if inp["bias"] is None else inp["bias"].double(), case.stride)
    want = want.transpose(1, 2) + (inp["resid"].double() if case.resid else 0.0)
    torch.testing.assert_close(ref["want"], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", [c for c in EC.CASES if c.op == "convT" and c.family == "poison"], ids=lambda c: c.id)
def test_transposed_reference_is_torchs_conv_transpose1d_plus_trim(case):
    """The header's formula w[r Cout + co][j Cin + ci] = weight[ci][co][r + (1 - j) s] applied to a ConvTranspose1d weight."""
    g = torch.Generator().manual_seed(5)
    weight = torch.randn(case.C, case.Cout, 2 * case.stride, generator=g)
    inp = EC.build(case)
    inp["w"] = EC.convt_matrix(weight)
    x = inp["x"].double().transpose(1, 2)
    full = F.conv_transpose1d(F.elu(x) if case.elu else x, weight.double(), inp["bias"].double(), stride=case.stride).transpose(1, 2)
    geo = EC.conv_geometry(case)
    assert full.shape[1] == geo["Mr"] * case.stride == (case.T + 1) * case.stride
    want = full[:, case.trim:case.trim + geo["Tout"]]
    torch.testing.assert_close(EC.conv_forward(case, inp)["want"], want, rtol=1e-12, atol=1e-12)


def test_ramp_outputs_name_their_source():
    """One-hot weight rows on x[b, t, c] = (b Tin + t) Cin + c: without bias and residual the output IS the mirrored source index."""
    case = EC.Case("conv", "exact", 2, 4, C=3, Cout=2, k=7, left=3, right=3, bias=False, sub="ramp")
    inp = EC.build(case)
    y = EC.conv_forward(case, inp)["want"]
    col = (torch.arange(2) * 7 + 3) % 21
    for b in range(2):
        for m in range(4):
            for n in range(2):
                tap, ci = divmod(int(col[n]), 3)
                f = abs(m - 3 + tap)
                f = 6 - f if f >= 4 else f
                assert y[b, m, n] == (b * 4 + f) * 3 + ci


def test_lstm_step_reference_is_nn_lstm_when_fed_its_own_h():
    H, B, T = 64, 3, 5
    m = torch.nn.LSTM(H, H, 1).double()
    x = torch.randn(B, T, H, generator=torch.Generator().manual_seed(1)).double()
    want = m(x.transpose(0, 1))[0].transpose(0, 1)
    got, bound = EC.lstm_step_reference(m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0 + m.bias_hh_l0, x, want, False)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4


def test_groupnorm_and_scale_references_are_torchs():
    case = next(c for c in EC.CASES if c.id == "groupnorm-poison-b3-t342-c48-r")
    inp = EC.build(case)
    want = F.group_norm(inp["x"].double().transpose(1, 2), 1, inp["gamma"].double(), inp["beta"].double(), EC.EPS).transpose(1, 2) + inp["resid"].double()
    torch.testing.assert_close(EC.gn_forward(case, inp)["want"], want, rtol=1e-12, atol=1e-12)
    x = torch.randn(3, 2, 100)
    want = x.double().mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8
    torch.testing.assert_close(EC.scale_forward({"x": x})["want"], want, rtol=1e-14, atol=0)


def test_rvq_decode_reference_is_the_cpu_models():
    from pytorch_models.audio.encodec import RVQ

    case = next(c for c in EC.CASES if c.id == "rvq_decode-poison-b3-t9-q32")
    inp = EC.build(case)
    q = RVQ(128, 1024, 32)
    for i, vq in enumerate(q):
        vq.embed.copy_(inp["E"][i])
    assert torch.equal(EC.rvq_decode_reference(inp["codes"], inp["E"]), q.dequantize(inp["codes"].transpose(0, 1)))


# --------------------------------------------------------------------------------------------------------------- the families' conditions
@pytest.mark.parametrize("case", [c for c in EC.CASES if c.op == "rvq_encode"], ids=lambda c: c.id)
def test_rvq_families_keep_their_conditions(solved, case):
    inp, ref = solved(case)
    if case.family == "exact":
        assert bool(ref["ties"].all()), "every decision of every stage must be a tie"
        E0, nq = inp["E"][0], case.nq
        j = torch.arange(EC.RVQ_N)
        for q in range(nq):  # every entry equals its twin, and every stage holds all four kinds of pair
            tw = EC.rvq_twin(j, q)
            assert torch.equal(EC.rvq_twin(tw, q), j) and torch.equal(inp["E"][q][tw], inp["E"][q])
            assert set((j ^ tw).tolist()) == {1, 4, 16, 256}
        for i, a in EC.RVQ_EXACT_ROWS.items():  # the planted rows: the code of stage 0 is the lowest index of the tied set
            if i < case.T:
                tied = (E0 == inp["z"][i]).all(1).nonzero()[:, 0].tolist()
                assert a in tied and len(tied) > 1 and int(ref["codes"][0, i]) == tied[0], (i, a, tied)
                if i == 0:  # inside a lane, across fq, tiles and waves at once, in front of every M
                    assert tuple(tied) == EC.RVQ_TIE_SETS[0] and {1, 4, 16} <= {t ^ tied[0] for t in tied} and tied[-1] // 256 == 3
                elif i == 2:  # the last entry of wave 0 against the first of wave 1
                    assert tuple(tied) == EC.RVQ_TIE_SETS[1] and tied[:2] == [255, 256]
                else:
                    assert tied == sorted((a, EC.rvq_twin(a, 0)))
        if nq > 1 and case.T > 4:  # row 4: the residual of stage 0 IS entry 261 of stage 1 and its twin
            assert int(ref["codes"][1, 4]) == min(261, EC.rvq_twin(261, 1))
        assert float(inp["E"].abs().max()) <= 3 and bool((inp["z"] == inp["z"].round()).all())
        return
    planted = {i for i, *_ in inp["planted"]}
    for i, a, b, f in inp["planted"]:
        assert int(ref["codes"][0, i]) == a and bool(ref["decided"][0, i]) == (f > 1), (i, a, b, f)
    rows = [m for m in range(case.T) if m not in planted]
    undecided = float((~ref["decided"][:, rows]).float().mean()) if rows else 0.0
    assert undecided <= 0.01, f"{case.id}: {100 * undecided:.2f} % of the Gaussian decisions are undecided"


def test_groupnorm_offset_family_sits_at_4096(solved):
    for case in (c for c in EC.CASES if c.op == "groupnorm" and c.family == "offset" and c.T * c.C >= 32):
        _, ref = solved(case)
        rt = ref["mean"].abs() / ref["var"].sqrt()
        assert bool((rt > 3000).all() and (rt < 5500).all()), (case.id, rt)


# --------------------------------------------------------------------------------------------------------------- stand-in and mutants
@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.id)
def test_a_correct_kernel_passes_at_one_times_the_bound(solved, case):
    inp, ref = solved(case)
    ok, r, msg = EC.verify(case, inp, ref, EC.StandIn(), margin=1.0)
    assert ok, f"{case.id}: {msg}"
    assert r <= 1.0


@pytest.mark.parametrize("mutant", EC.MUTANTS)
def test_each_mutant_is_rejected_by_its_family(solved, mutant):
    be = EC.StandIn(torch.float64, mutant)
    aimed = [c for c in EC.CASES if c.op == EC.MUTANT_OP[mutant] and c.family == EC.MUTANT_FAMILY[mutant]]
    assert aimed
    rejected = [c.id for c in aimed if not EC.verify(c, *solved(c), be)[0]]
    assert rejected, f"{mutant}: accepted by every {EC.MUTANT_FAMILY[mutant]} case of {EC.MUTANT_OP[mutant]}"
    if mutant == "stale_acc":  # the hazard of DESIGN.md section 14 must show at T = 2 already
        assert any("-t2-" in i for i in rejected), rejected


def test_embedded_buffers_are_aligned_and_guarded():
    for shape, gap in (((2, 3, 5), 0), ((3, 7, 4), 8), ((1, 9), 0)):
        t = torch.arange(float(torch.Size(shape).numel())).view(shape)
        buf, v = EC.embedded(t, "cpu", gap)
        assert torch.equal(v, t) and v.data_ptr() % 16 == 0 and int(torch.isnan(buf).sum()) == buf.numel() - t.numel()
    buf, v = EC.embedded(torch.empty(2, 5, 3), "cpu", sentinel=True)
    v.fill_(1.0)
    assert EC.sentinels_intact(buf, v)
    buf[2] = 0.0
    assert not EC.sentinels_intact(buf, v)
    buf, v = EC.embedded(torch.empty(1, 2, 7, dtype=torch.int64), "cpu", sentinel=True)
    v.fill_(3)
    assert EC.sentinels_intact(buf, v)
    buf[-1] = 0
    assert not EC.sentinels_intact(buf, v)
