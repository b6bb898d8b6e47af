"""Keeps the adversarial audio front-end suite (tests/test_hip_audio_adversarial.py) honest without a GPU: its float64 references
are F.conv1d / F.layer_norm / F.instance_norm / F.avg_pool1d's and oracle/ref_audio.py's, a correct kernel (fp32 arithmetic in
another summation order, gelu_poly, a bf16 store) stays inside 1.0 x of every bound and equals the exact family bit for bit, every
defect in audio_cases.MUTANTS is rejected by a case of the family aimed at it, the case lists reach every kernel path they are
named for, no case is a refusal in disguise (the real ops wrappers run their own argument checks on every case, against a stub
library), and the families keep their conditions (the bf16-exact share, var >> eps and A / sigma in 1e3 .. 1e4 in w2v_stem0's
cancel family, at most 10 % uninformative comparisons outside the cancel families)."""
import pytest
import torch
import torch.nn.functional as F

import audio_cases as AC
from oracle import ref_audio as RA
from oracle import ref_spectrogram as RS

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = AC.build(case)
            cache[case.id] = (inp, AC.reference(case, inp))
        return cache[case.id]

    return get


# --------------------------------------------------------------------------------------------------------------- independent forms
def _torch_form(case, inp):
    """The op through torch's own float64 functions, written without audio_cases' helpers."""
    dd = lambda k: None if inp.get(k) is None else inp[k].double()  # noqa: E731
    if case.op == "w2v_stem0":
        n = AC.wave_len(case) - case.tail
        v = F.conv1d(inp["x"].double()[:, None, :n], inp["w"].double()[:, None, :], dd("bias"), case.stride)  # (B, C0, T0)
        if case.norm == "layer":
            v = F.layer_norm(v.transpose(1, 2), (case.C,), dd("gamma"), dd("beta"), AC.EPS).transpose(1, 2)
        elif case.norm == "instance":
            v = F.instance_norm(v, weight=dd("gamma"), bias=dd("beta"), eps=AC.EPS) if case.T > 1 else dd("beta")[None, :, None].expand_as(v)
        return F.gelu(v).transpose(1, 2)
    if case.op == "whisper_stem1":
        d, Cp = case.d, AC.cpad(case)
        w = inp["w"].double().view(d, 3, Cp)[:, :, :case.C].permute(0, 2, 1)  # (d, C, 3)
        y = F.gelu(F.conv1d(inp["x"].bfloat16().double(), w, dd("bias"), 1, 1)).transpose(1, 2)
        return F.pad(y, (0, 0, 1, 1))
    if case.op == "grouped_conv":
        G, cg, cgp, k = case.G, case.cg, case.cgp, case.k
        x = inp["x"].double()[..., :cg].permute(0, 1, 3, 2).reshape(case.B, G * cg, -1)  # (B, d, Tp)
        w = inp["w"].double()[:, :, :k * cgp].view(G, cg, k, cgp)[..., :cg].permute(0, 1, 3, 2).reshape(G * cg, cg, k)
        z = F.conv1d(x, w, dd("bias"), case.stride, 0, 1, G).transpose(1, 2).reshape(case.B * case.T, G * cg)
        z = F.gelu(z) if case.act == "gelu" else z
        return z if inp["resid"] is None else z + dd("resid")
    if case.op == "group_windows":
        x = inp["x"].double().view(case.B, case.T, case.G, case.cg).permute(0, 2, 1, 3)
        return F.pad(x, (0, case.cgp - case.cg, *case.pads))
    return F.avg_pool1d(inp["x"].double().transpose(1, 2), 2).transpose(1, 2)


def _oracle_form(case, inp):
    """oracle/ref_audio.py where it applies: conv1d_tl for the three convolutions, _norm_free for the two norms."""
    if case.op == "w2v_stem0":
        n = AC.wave_len(case) - case.tail
        v = RA.conv1d_tl(inp["w"].double()[:, None, :], None if inp["bias"] is None else inp["bias"].double(), inp["x"].double()[:, :n, None], case.stride)
        if case.norm != "none":
            v = RA._norm_free(v, 1 if case.norm == "instance" else 2, AC.EPS) * inp["gamma"].double() + inp["beta"].double()
        return F.gelu(v)
    if case.op == "grouped_conv":
        G, cg, cgp, k = case.G, case.cg, case.cgp, case.k
        x = inp["x"].double()[..., :cg].permute(0, 2, 1, 3).reshape(case.B, -1, G * cg)  # (B, Tp, d)
        w = inp["w"].double()[:, :, :k * cgp].view(G, cg, k, cgp)[..., :cg].permute(0, 1, 3, 2).reshape(G * cg, cg, k)
        z = RA.conv1d_tl(w, None if inp["bias"] is None else inp["bias"].double(), x, case.stride, G).reshape(case.B * case.T, G * cg)
        z = F.gelu(z) if case.act == "gelu" else z
        return z if inp["resid"] is None else z + inp["resid"].double()
    return None


# --------------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_reach_every_named_path():
    for op, need in AC.REQUIRED_PATHS.items():
        have = set().union(*(AC.paths(c) for c in AC.CASES if c.op == op))
        assert need <= have, (op, need - have)
    by = lambda op, f: {f(c) for c in AC.CASES if c.op == op}  # noqa: E731
    assert by("w2v_stem0", lambda c: c.T) >= {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025}
    assert by("w2v_stem0", lambda c: c.C) >= {8, 64, 504, 512} and by("w2v_stem0", lambda c: c.B) == {1, 3}
    assert {c.T for c in AC.CASES if c.op == "w2v_stem0" and c.norm == "instance"} >= {3, 4, 255, 256, 257, 1023, 1024, 1025}
    assert by("whisper_stem1", lambda c: (c.C, AC.cpad(c))) == {(3, 64), (64, 64), (80, 128), (128, 128)}
    assert by("whisper_stem1", lambda c: c.T) == {1, 2, 127, 128, 129, 300} and by("whisper_stem1", lambda c: c.d) == {4, 64, 128, 132, 384}
    assert by("grouped_conv", lambda c: (c.cg, c.cgp)) == {(4, 8), (8, 8), (12, 16), (16, 16), (28, 32), (32, 32), (44, 48), (48, 48), (60, 64), (64, 64)}
    assert by("grouped_conv", lambda c: c.k) == {1, 2, 3, 19, 31, 128} and by("grouped_conv", lambda c: c.stride) == {1, 2, 3}
    assert by("grouped_conv", lambda c: c.T) == {1, 15, 16, 17, 64, 65, 128, 129, 257}
    for mi in (1, 4):  # both activations, both LDS row layouts at both MI
        got = {(c.act, AC.gc_launch(c)["swz"]) for c in AC.CASES if c.op == "grouped_conv" and AC.gc_launch(c)["mi"] == mi}
        assert got == {(a, s) for a in ("none", "gelu") for s in (False, True)}, (mi, got)
    assert by("group_windows", lambda c: c.cg) >= {4, 12, 44, 8, 48} and by("avgpool_time2", lambda c: c.T) == {2, 3, 301}
    for c in AC.CASES:
        assert c.family in ("exact", "onehot", "cancel", "offset", "poison", "batch") and c.op in AC.OPS
        assert c.family != "exact" or (c.op not in AC.GELU_OPS and c.act == "none"), c.id
        assert c.family != "onehot" or c.op in AC.GELU_OPS or c.act == "gelu", c.id
        assert c.family != "offset" or (c.norm == "layer" and c.C <= 96), c.id
        assert c.family != "batch" or c.B > 1, c.id
    # every case is a few milliseconds on the device: the largest output is 3 x 1025 x 512 values
    assert max(torch.Size(AC.out_shape(c)).numel() for c in AC.CASES) == 3 * 1025 * 512


class _StubLib:
    """Answers PM_OK (and a scratch size) to every entry point: what runs is the wrappers' own Python-side argument checks."""

    def __getattr__(self, name):
        return (lambda B, T0: B * -(-T0 // 1024) * 160) if name == "pm_w2v_stem0_scratch_floats" else (lambda *a: 0)


def test_no_case_is_a_refusal_in_disguise(monkeypatch):
    from pytorch_models._hip import ops

    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "lib", lambda: _StubLib())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for case in AC.CASES:
        assert AC.abi_refusal(case) is None, case.id
        out = AC.run(ops, case, AC.to_device(case, AC.build(case), "cpu"))
        assert tuple(out["y"].shape) == AC.out_shape(case) and out["y"].dtype == torch.bfloat16, case.id
    for case in AC.REFUSED:  # and the limits are real
        assert AC.abi_refusal(case), case.id
    assert AC.abi_refusal(AC.Case("w2v_stem0", "poison", 1, 4, C=12)) and AC.abi_refusal(AC.Case("whisper_stem1", "poison", 1, 4, C=3, d=6))
    assert AC.abi_refusal(AC.Case("avgpool_time2", "exact", 1, 4, d=12))


def test_embedded_slices_are_aligned_and_guarded():
    for shape, dt, ld in (((2, 3, 5), torch.float32, 0), ((7, 12), torch.bfloat16, 20), ((9,), torch.float32, 0)):
        t = torch.arange(float(torch.Size(shape).numel())).view(shape).to(dt)
        buf, v = AC.embedded(t, "cpu", ld)
        assert torch.equal(v.reshape(-1), t.reshape(-1)) and v.data_ptr() % 16 == 0 and int(torch.isnan(buf.float()).sum()) == buf.numel() - t.numel()
    buf, v = AC.embedded(torch.empty(5, 12, dtype=torch.bfloat16), "cpu", 20, sentinel=True)
    v.fill_(1.0)
    assert AC.sentinels_intact(buf, v)
    buf[3] = 0.0
    assert not AC.sentinels_intact(buf, v)
    buf, v = AC.embedded(torch.empty(5, 12, dtype=torch.bfloat16), "cpu", 20, sentinel=True)
    buf.view(-1)[v.storage_offset() + 12] = 0.0  # a pad column of row 0
    assert not AC.sentinels_intact(buf, v)


# --------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_every_gpu_case(case, solved):
    inp, ref = solved(case)
    want, bound = ref["want"], ref["bound"]
    assert want.dtype == torch.float64 and tuple(want.shape) == AC.out_shape(case) == tuple(bound.shape)
    assert torch.isfinite(want).all() and torch.isfinite(bound).all() and (bound >= 0).all()
    # the reference is torch's own float64 form and the oracle's; 1 / sigma amplifies the last float64 bits where a norm cancels
    amp = 1.0
    if case.norm == "instance":
        amp = float((ref["A"] / ref["sigma"]).max())
    elif case.norm == "layer":
        amp = float((ref["A"].max(-1).values / torch.sqrt(ref["v"].var(-1, unbiased=False) + AC.EPS)).max())
    tol = 1e-12 * (1.0 + float(ref["A"].max())) * max(amp, 1.0)
    for other in (_torch_form(case, inp), _oracle_form(case, inp)):
        if other is not None:
            assert other.shape == want.shape and float((other - want).abs().max()) <= tol, float((other - want).abs().max())
    # a correct kernel: fp32 arithmetic in the opposite order, gelu_poly, a bf16 store
    emu = AC.emulate(case, inp)
    if case.family == "exact":
        assert torch.equal(emu["y"], AC.store(want, "bf16")), "integers: exact in any order"
        assert float(ref["A"].max()) < 2 ** 24
        if case.op == "grouped_conv":
            assert float((want.abs() <= 256).double().mean()) >= 0.9, "at least 90 % of the outputs are exact in bf16"
        if case.op == "avgpool_time2":
            assert bool((want[..., 0] == 257).all()) and bool((AC.store(want, "bf16")[..., 0] == 256).all()), "ties round to even"
    else:
        r = AC.ratio(emu["y"], want, bound)
        assert r <= 1.0, f"{case.id}: the fp32 evaluation sits at {r:.3f} x its own bound"
    assert AC.accepts(case, emu, ref)[0]
    assert AC.accepts(case, {"y": AC.store(want, "bf16")}, ref)[0], "the reference rounded once is accepted"
    # the family conditions
    if case.family == "onehot":
        v = ref["v"] if "v" in ref and case.norm == "none" else None
        if v is not None:
            assert bool((v * 2 == (v * 2).round()).all()) and float(ref["A"].max()) < 2 ** 24, "the pre-activation is exact"
    if case.op == "whisper_stem1":
        assert bool((want[:, 0] == 0).all() and (want[:, -1] == 0).all() and (bound[:, 0] == 0).all() and (bound[:, -1] == 0).all())
    if case.family == "cancel" and case.op == "w2v_stem0":
        cond = (ref["A"].mean(1, keepdim=True) / ref["sigma"]).flatten()
        assert float(ref["var"].min()) >= 1e3 * AC.EPS, "var >> eps"
        assert 1e3 <= float(cond.min()) and float(cond.max()) <= 1e4, (float(cond.min()), float(cond.max()))
    elif case.family == "cancel":
        inner = slice(1, -1) if case.op == "whisper_stem1" else slice(None)
        rel = (want.abs() / ref["A"].clamp_min(1e-300))[:, inner][ref["A"][:, inner] > 0]
        assert rel.numel() == 0 or float(rel.median()) < 0.1, "|want| << A"
    else:
        assert AC.uninformative_fraction(ref) <= 0.10, f"{case.id}: {AC.uninformative_fraction(ref):.3f} of the comparisons say little"


# --------------------------------------------------------------------------------------------------------------- the families' teeth
def test_cancel_family_separates_first_order_from_second_order_statistics(solved):
    """The instance statistics: normalising the computed fp32 conv output stays inside the bound, the variance from fp32
    autocorrelation sums (w^T (R / T - s s^T) w) is outside it by the factor its (A / sigma)^2 error predicts."""
    seen = 0
    for case in (c for c in AC.CASES if c.family == "cancel" and c.op == "w2v_stem0"):
        inp, ref = solved(case)
        first = AC.ratio(AC.emulate(case, inp)["y"], ref["want"], ref["bound"])
        bad = AC.forward(case, inp, mutant="var_second_order")
        rel = float(((bad["var"] - ref["var"]).abs() / ref["var"]).max())
        second = AC.ratio(AC.store(bad["want"], "bf16"), ref["want"], ref["bound"])
        print(f"FIGURE {case.id} first-order {first:.3f} second-order {second:.3e} worst relative variance error {rel:.3e}")
        assert first <= 1.0 and second > AC.MARGIN and rel > 1e-2
        seen += 1
    assert seen == 3


def test_offset_family_separates_one_pass_from_two_pass_variance(solved):
    for case in (c for c in AC.CASES if c.family == "offset"):
        inp, ref = solved(case)
        rel = (ref["mean"].abs() / torch.sqrt(ref["v"].var(-1, unbiased=False, keepdim=True) + AC.EPS)).flatten()
        assert 0.8 * AC.OFFSET_RATIO <= float(rel.min()) and float(rel.max()) <= 1.25 * AC.OFFSET_RATIO, case.id
        two = AC.ratio(AC.emulate(case, inp)["y"], ref["want"], ref["bound"])
        one = AC.ratio(AC.mutant_output(case, inp, "onepass")["y"], ref["want"], ref["bound"])
        print(f"FIGURE {case.id} two-pass {two:.4f} one-pass {one:.3e}")
        assert two <= 1.0 and one > 10.0, (case.id, two, one)


@pytest.mark.parametrize("mutant", AC.MUTANTS)
def test_every_mutant_is_rejected_by_the_family_aimed_at_it(mutant, solved):
    fam = AC.MUTANT_FAMILY[mutant]
    aimed = [c for c in AC.CASES if c.family == fam and AC.mutant_applies(c, mutant)]
    assert aimed, f"no {fam} case can see {mutant}"
    rejected = []
    for case in aimed:
        inp, ref = solved(case)
        ok, r = AC.accepts(case, AC.mutant_output(case, inp, mutant), ref)
        if not ok:
            rejected.append((case.id, r))
    assert rejected, f"{mutant}: accepted by all {len(aimed)} {fam} cases"
    ops_hit = {c.split("-")[0] for c, _ in rejected}
    want_ops = {"trunc": {"w2v_stem0", "whisper_stem1", "grouped_conv", "group_windows", "avgpool_time2"},
                "padrow": {"whisper_stem1", "group_windows"}}.get(mutant, {aimed[0].op})
    assert ops_hit >= want_ops, (mutant, want_ops - ops_hit)
    if mutant == "chunk_edge":  # both chunk sizes' neighbours are among the rejecting cases
        assert {c.T for c in aimed if any(c.id == i for i, _ in rejected)} >= {257, 1025}
    if mutant == "tile_edge":  # at MI = 1 and at MI = 4
        assert {AC.gc_launch(c)["mi"] for c in aimed if any(c.id == i for i, _ in rejected)} == {1, 4}


# =============================================================================================================== STFT / mel / log-mel
@pytest.fixture(scope="module")
def stft_solved():
    from pytorch_models._hip import ops

    cache = {}

    def get(case):
        if case.id not in cache:
            inp = AC.stft_build(case, ops.stft_tables)
            cache[case.id] = (inp, AC.stft_forward(case, inp))
        return cache[case.id]

    return get


def test_stft_case_list_reaches_every_named_path(monkeypatch):
    have = set().union(*(AC.stft_paths(c) for c in AC.STFT_CASES))
    assert AC.STFT_REQUIRED <= have, AC.STFT_REQUIRED - have
    assert {(c.n_fft, c.hop) for c in AC.STFT_CASES if c.mode in (1, 2)} >= {(512, 128), (400, 160)}
    assert {c.family for c in AC.STFT_CASES} == {"exact", "cancel", "poison", "batch", "loudness"}
    assert {c.win for c in AC.STFT_CASES if c.family == "exact"} == {"int", "intfold"}
    # no case is a refusal in disguise: the wrapper's own checks against a stub library; and the limits are real
    from pytorch_models._hip import ops

    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "lib", lambda: _StubLib())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for c in AC.STFT_CASES:
        assert AC.stft_refusal(c) is None and AC.stft_lds_bytes(c) <= 64 * 1024, c.id
        y = AC.stft_run(ops, c, AC.stft_build(c, ops.stft_tables), "cpu")
        assert tuple(y.shape) == (*(c.lead or (c.B,)), c.n_fft // 2 + 1 if c.mode == 0 else c.n_mels, c.frames) and y.dtype == torch.float32
    assert [bool(AC.stft_refusal(c)) for c in AC.STFT_REFUSED] == [True, True, True]
    big = AC.STFT_REFUSED[0]
    assert AC.stft_lds_bytes(big, 0) <= 64 * 1024 < AC.stft_lds_bytes(big, 1), "(1024, 256): mode 0 served, mode 1 refused"


@pytest.mark.parametrize("case", AC.STFT_CASES, ids=lambda c: c.id)
def test_stft_reference_and_bound_on_every_gpu_case(case, stft_solved):
    inp, ref = stft_solved(case)
    want, bound = ref["want"], ref["bound"]
    assert want.dtype == torch.float64 and want.shape == bound.shape and not torch.isnan(want).any() and (bound >= 0).all()
    win = AC.stft_window(case)
    if win is not None:  # the true float64 windowed DFT (center = True, reflect) + a dense filterbank product
        x = inp["x"].double()
        X = torch.stft(x, case.n_fft, case.hop, window=win.double(), center=True, pad_mode="reflect", return_complex=True)[..., :case.frames]
        fr = RS.frames(x, case.n_fft, case.hop)[:, :case.frames]
        wd = win.double()
        sym = torch.zeros_like(wd)
        if case.folded:
            sym[1:] = (wd[1:] - 0.5 * (wd[1:] + wd[1:].flip(0))).abs()
        e = (2 * AC.U32 * (fr.abs() * wd).sum(-1) + (fr.abs() * sym).sum(-1))[:, None, :]  # table rounding + the symmetrisation, per frame
        p = X.real.square() + X.imag.square()
        dp = 2 * X.abs() * 1.42 * e + 2 * e * e + 1e-13 * p
        if case.mode:
            p, dp = inp["filters"].double() @ p, inp["filters"].double() @ dp
        if case.mode == 2:
            v = torch.log10(p)
            pk = v.flatten(1).max(1).values[:, None, None]
            p = (torch.maximum(v, pk - 8) + 4) / 4
            floored = v < pk - 8
            dp = torch.where(floored, torch.zeros_like(dp), dp / (p.abs() * 0 + 10 ** v * 2.302585092994046) / 4) + 1e-6
        mine = want.reshape(p.shape)
        fin = torch.isfinite(p)
        assert torch.equal(torch.isfinite(mine), fin)
        assert bool(((mine - p).abs()[fin] <= dp[fin] + 1e-30).all()), float(((mine - p).abs()[fin] / (dp[fin] + 1e-30)).max())
    emu = AC.stft_emulate(case, inp)
    ok, r = AC.stft_accepts(case, emu, ref)
    assert ok and r <= 1.0, f"{case.id}: the fp32 evaluation sits at {r:.3f} x its own bound"
    if case.family == "exact":
        assert float(ref["A"].max()) < 2 ** 24 and bool((want == want.round()).all())
        if case.empty_row:
            assert bool((want.reshape(-1, case.n_mels, case.frames)[:, case.n_mels // 2] == 0).all())
    elif case.family == "cancel":
        assert float((want.reshape(ref["A"].shape) / ref["A"]).median()) < 1e-2, "|want| << A: most bins are far from the tone"
    else:
        fin = torch.isfinite(want)
        assert float(((bound > 0.5 * want.abs()) & (bound > 0))[fin].double().mean()) <= 0.10
    if case.family == "loudness":
        w = want.reshape(4, -1)
        assert float(ref["peak"][0]) > 0 and float(ref["peak"][1]) < 0 and bool(torch.isinf(w[3]).all() and (w[3] < 0).all()) and bool(torch.isfinite(w[:3]).all())
        assert bool((w[2] == (ref["peak"][2] - 4) / 4).any()), "the half-silent clip reaches its floor"


def test_stft_reference_matches_the_oracle(stft_solved):
    case = next(c for c in AC.STFT_CASES if c.family == "cancel" and (c.n_fft, c.hop, c.win) == (400, 160, "hann"))
    inp, ref = stft_solved(case)
    other = RS.power_spectrogram(inp["x"], 400, 160).double()
    assert float((other - ref["want"]).abs().max()) <= 1e-5 * float(ref["want"].max())


@pytest.mark.parametrize("mutant", AC.STFT_MUTANTS)
def test_every_stft_mutant_is_rejected_by_the_family_aimed_at_it(mutant, stft_solved):
    fam = AC.STFT_MUTANT_FAMILY[mutant]
    aimed = [c for c in AC.STFT_CASES if c.family == fam and AC.stft_mutant_applies(c, mutant)]
    assert aimed, f"no {fam} case can see {mutant}"
    rejected = [c.id for c in aimed if not AC.stft_accepts(c, AC.stft_mutant_output(c, stft_solved(c)[0], mutant), stft_solved(c)[1])[0]]
    assert rejected, f"{mutant}: accepted by all {len(aimed)} {fam} cases"
    if mutant in ("reflect_edge", "frame_shift", "bin_rows"):  # on both table layouts
        assert {("fold" in i) for i in rejected} == {True, False}
