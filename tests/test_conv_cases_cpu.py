"""Keeps the adversarial convolution suite (tests/test_hip_conv_adversarial.py) honest without a GPU: its float64 references are
F.conv2d / F.unfold / F.layer_norm's, a correct kernel (fp32 arithmetic in another summation order, output rounded to the kernel's
dtype) stays inside 1.0 x of every bound and equals the exact family bit for bit, every defect in conv_cases.MUTANTS is rejected by
a case of the family aimed at it, the case lists reach every kernel path they are named for, and no case is a refusal in disguise
(the real ops wrappers run their own argument checks on every case, against a stub library)."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = CC.build(case)
            cache[case.id] = (inp, CC.reference(case, inp))
        return cache[case.id]

    return get


# --------------------------------------------------------------------------------------------------------------- independent forms
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _conv2d(case, inp):
    """The op's convolution + bias through F.conv2d in float64, explicit zero pad.  (N, Ho, Wo, Cout)."""
    stride, (pt, pl, pb, pr), groups = CC.geometry(case)
    bias = inp.get("bias")
    z = F.conv2d(F.pad(_nchw(inp["x"]), (pl, pr, pt, pb)), _nchw(inp["w"]), None if bias is None else bias.double(), stride, 0, 1, groups)
    return z.permute(0, 2, 3, 1)


def _unfold(case, inp):
    """The same as a gather (F.unfold) followed by one matrix product per group."""
    stride, (pt, pl, pb, pr), groups = CC.geometry(case)
    x, w = F.pad(_nchw(inp["x"]), (pl, pr, pt, pb)), _nchw(inp["w"])  # w (Cout, cg, kh, kw)
    N, Cin = x.shape[:2]
    Cout, cg, kh, kw = w.shape
    Ho, Wo = (x.shape[2] - kh) // stride + 1, (x.shape[3] - kw) // stride + 1
    outs = []
    for g in range(groups):
        cols = F.unfold(x[:, g * cg:(g + 1) * cg], (kh, kw), stride=stride)  # (N, cg kh kw, Ho Wo)
        wg = w[g * (Cout // groups):(g + 1) * (Cout // groups)].reshape(Cout // groups, -1)
        outs.append(wg @ cols)
    z = torch.cat(outs, 1).reshape(N, Cout, Ho, Wo).permute(0, 2, 3, 1)
    return z if inp.get("bias") is None else z + inp["bias"].double()


def _torch_form(case, inp, z):
    """The rest of the op with torch's own functions in float64, from the convolution z."""
    if case.op == "conv_bf16":
        z = z if inp["resid"] is None else z + inp["resid"].double()
        return F.relu(z) if case.act == "relu" else z
    if case.op == "conv2d_nhwc":
        z = {"none": lambda t: t, "relu": F.relu, "silu": F.silu}[case.act](z)
        return z if inp["resid"] is None else z + inp["resid"].double()
    if case.op == "resnet_stem":
        return F.max_pool2d(F.relu(z).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    if case.op in CC.LN_OPS:
        y = F.layer_norm(z, (z.shape[-1],), inp["gamma"].double(), inp["beta"].double(), CC.EPS)
        if case.op == "dwconv7_ln":
            y = F.pad(y.reshape(-1, y.shape[-1]), (0, CC.default_ldy(case) - y.shape[-1]))
        return y
    if case.op == "dwconv3":
        y = F.gelu(z * inp["scale"].double() + inp["shift"].double(), approximate="tanh")
        return y if inp["gate"] is None else y * inp["gate"].double()[:, None, None, :]
    if case.op == "maxvit_stem":
        y = F.gelu(z, approximate="tanh")
        return F.pad(y, (0, CC.default_ldy(case) - y.shape[-1]))
    raise ValueError(case.op)


def _whole_op(case, inp, conv):
    if case.op == "im2col3x3":
        x = inp["x"].double()
        N, H, W, C = x.shape
        cols = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1)  # (N, C 9, HW), rows in (c, kh, kw) order
        y = cols.view(N, C, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * C)
        return F.pad(y, (0, CC.default_ldy(case) - 9 * C))
    if case.op == "avgpool2x2":
        return F.avg_pool2d(inp["x"].double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    return _torch_form(case, inp, conv(case, inp))


# --------------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_reach_every_named_path():
    for op, need in CC.REQUIRED_PATHS.items():
        have = set().union(*(CC.paths(c) for c in CC.CASES if c.op == op))
        assert need <= have, (op, need - have)
    by = lambda op, f: {f(c) for c in CC.CASES if c.op == op}  # noqa: E731
    assert by("conv_bf16", lambda c: c.Cout) >= {8, 24, 64, 65, 68, 72, 128, 130, 132, 136, 200}
    assert by("conv_bf16", lambda c: c.C) == {64, 128, 192}
    assert any(c.op == "conv_bf16" and c.N == 3 and CC.out_hw(c) == (5, 10) for c in CC.CASES)
    assert by("dwconv7_ln", lambda c: c.C) == {4, 8, 40, 96, 1028, 2048, 2052, 4096}
    assert by("dwconv7_ln", lambda c: (c.H, c.W)) == {(1, 1), (3, 3), (1, 8), (2, 9), (7, 7), (5, 17)}
    assert by("dwconv7_ln", lambda c: (c.xdt, c.ydt)) == {(a, b) for a in ("bf16", "f32") for b in ("bf16", "f32")}
    assert by("dwconv7_ln", lambda c: c.N) == {1, 3}
    assert by("maxvit_stem", lambda c: c.Cout) == {1, 32, 65, 96, 128, 200, 256}
    assert by("maxvit_stem", lambda c: (c.H, c.W)) == {(2, 2), (3, 5), (30, 17)}
    assert by("convnext_stem", lambda c: c.Cout) == {1, 45, 64, 65, 352} and by("convnext_stem", lambda c: (c.H, c.W)) == {(4, 4), (8, 36)}
    assert by("resnet_stem", lambda c: (c.H, c.W)) == {(1, 1), (2, 3), (5, 5), (8, 9), (33, 18)}
    assert {(c.C, c.H, c.W) for c in CC.CASES if c.op == "dwconv3" and c.stride == 1} >= {(4, 1, 1), (40, 1, 5), (40, 5, 1), (256, 7, 7)}
    assert {(c.H, c.W) for c in CC.CASES if c.op == "dwconv3" and c.stride == 2} == {(2, 2), (3, 2), (9, 13), (14, 15)}
    for c in CC.CASES:
        assert c.family in ("exact", "cancel", "offset", "poison", "batch")
        assert c.family != "exact" or (c.op in CC.EXACT_OPS and c.act != "silu"), c.id
        assert c.family != "offset" or (c.op in CC.LN_OPS and (c.Cout or c.C) <= 96), c.id
        assert c.family != "batch" or c.N > 1, c.id
    # the largest tensor stays at 3 x 5 x 17 x 4096 floats: every case is a few milliseconds
    assert max(c.N * c.H * c.W * c.C for c in CC.CASES) == 3 * 5 * 17 * 4096


class _StubLib:
    """Answers PM_OK to every entry point: what runs is the wrappers' own Python-side argument checks."""

    def __getattr__(self, name):
        return lambda *a: 0


def test_no_case_is_a_refusal_in_disguise(monkeypatch):
    from pytorch_models._hip import ops

    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "lib", lambda: _StubLib())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for case in CC.CASES:
        assert CC.abi_refusal(case) is None, case.id
        out = CC.run(ops, case, CC.to_device(case, CC.build(case), "cpu"))
        assert tuple(out["y"].shape) == CC.out_shape(case) and out["y"].dtype == CC.DT[case.ydt], case.id
    # and the limits are real: one step past each is refused by the same function
    assert CC.abi_refusal(CC.Case("dwconv7_ln", "cancel", 1, 3, 3, 4100, k=7)) and CC.abi_refusal(CC.Case("dwconv7_ln", "cancel", 1, 3, 3, 6, k=7))
    assert CC.abi_refusal(CC.Case("maxvit_stem", "cancel", 1, 1, 4, 3, Cout=8)) and CC.abi_refusal(CC.Case("convnext_stem", "cancel", 1, 3, 4, 3, Cout=8))
    assert CC.abi_refusal(CC.Case("dwconv3", "cancel", 1, 1, 4, 8, stride=2))


def test_poisoned_slices_are_aligned_and_surrounded():
    for shape, dt in (((2, 3, 1, 1), torch.float32), ((3, 5, 17, 4), torch.bfloat16), ((7,), torch.float32)):
        t = torch.arange(float(torch.Size(shape).numel())).view(shape).to(dt)
        p = CC.poisoned(t, "cpu")
        assert torch.equal(p, t) and p.data_ptr() % 16 == 0 and p.is_contiguous()


# --------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_every_gpu_case(case, solved):
    inp, ref = solved(case)
    want, bound = ref["want"], ref["bound"]
    assert want.dtype == torch.float64 and tuple(want.shape) == CC.out_shape(case) == tuple(bound.shape)
    assert torch.isfinite(want).all() and torch.isfinite(bound).all() and (bound >= 0).all()
    # the reference is torch's own float64 form, through F.conv2d and through the independently written gather
    scale = 1e-12 * (1.0 + float(ref["A"].abs().max()))
    for conv in (_conv2d, _unfold):
        other = _whole_op(case, inp, conv)
        tol = scale * (1e3 if case.op in CC.LN_OPS else 1.0)  # 1 / sigma amplifies the last float64 bits of the offset family
        assert float((other - want).abs().max()) <= tol, (conv.__name__, float((other - want).abs().max()))
    # a correct kernel: fp32 arithmetic in the opposite tap / channel order, output rounded to the kernel's dtype
    emu = CC.emulate(case, inp)
    if case.family == "exact":
        assert torch.equal(emu["y"], CC.store(want, case.ydt)), "integers: exact in any order"
        assert torch.equal(emu["y"].double(), want) or case.ydt == "bf16"
        assert CC.exact_fraction(case, ref) >= 0.9, "at least 90 % of the outputs are exact in bf16"
        assert float(ref["A"].max()) < 2 ** 24
    else:
        r = CC.ratio(emu["y"], want, bound)
        assert r <= 1.0, f"{case.id}: the fp32 evaluation sits at {r:.3f} x its own bound"
        if "psum" in ref:
            r = CC.ratio(emu["psum"], ref["psum"], ref["psum_bound"])
            assert r <= 1.0, f"{case.id}: psum at {r:.3f} x its bound"
    ok, _ = CC.accepts(case, emu, ref)
    assert ok
    ldy, width = CC.default_ldy(case), (9 * case.C if case.op == "im2col3x3" else case.Cout or case.C)
    if ldy is not None and ldy > width:
        assert (want[..., width:] == 0).all() and (bound[..., width:] == 0).all(), "pad columns: exact zeros"
    if case.family == "cancel" and case.op in ("conv_bf16", "conv2d_nhwc") and (case.k == 1 or min(case.H, case.W) >= 5):
        # |want| << A wherever the whole window is inside the image (border outputs see a partial, non-cancelling filter)
        assert float((want.abs() / ref["A"].clamp_min(1e-300))[ref["A"] > 0].median()) < 0.1


# --------------------------------------------------------------------------------------------------------------- the offset family
def test_offset_family_separates_one_pass_from_two_pass_variance(solved):
    seen = set()
    for case in (c for c in CC.CASES if c.family == "offset"):
        inp, ref = solved(case)
        C = case.Cout or case.C
        if C > 1:
            rel = (ref["mean"].abs() / ref["sigma"]).flatten()
            assert 0.8 * CC.OFFSET_RATIO <= float(rel.min()) and float(rel.max()) <= 1.25 * CC.OFFSET_RATIO, case.id
        two = CC.ratio(CC.emulate(case, inp)["y"], ref["want"], ref["bound"])
        one = CC.ratio(CC.mutant_output(case, inp, "onepass")["y"], ref["want"], ref["bound"])
        assert two <= 1.0
        if C in (40, 96):
            seen.add(C)
            # two-pass: a few hundredths of the bound where the f32 store does not hide it; one-pass: four orders outside
            assert (two < 0.1 or case.ydt == "bf16") and one > 1e4, (case.id, two, one)
            print(f"FIGURE {case.id} two-pass {two:.4f} one-pass {one:.3e}")
    assert seen == {40, 96}


# --------------------------------------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_every_mutant_is_rejected_by_the_family_aimed_at_it(mutant, solved):
    fam = CC.MUTANT_FAMILY[mutant]
    aimed = [c for c in CC.CASES if c.family == fam and CC.mutant_applies(c, mutant)]
    assert aimed, f"no {fam} case can see {mutant}"
    rejected = []
    for case in aimed:
        inp, ref = solved(case)
        ok, r = CC.accepts(case, CC.mutant_output(case, inp, mutant), ref)
        if not ok:
            rejected.append((case.id, r))
    assert rejected, f"{mutant}: accepted by all {len(aimed)} {fam} cases"
    ops_hit = {c.split("-")[0] for c, _ in rejected}
    want_ops = {"replicate": {"conv_bf16", "conv2d_nhwc", "resnet_stem", "im2col3x3"}, "origin": {"conv_bf16", "conv2d_nhwc", "resnet_stem"},
                "transpose": {"conv_bf16", "conv2d_nhwc", "resnet_stem"}, "trunc": {"conv_bf16", "conv2d_nhwc", "resnet_stem", "dwconv7_ln",
                "convnext_stem", "dwconv3", "maxvit_stem"}, "onepass": set(CC.LN_OPS), "padcols": {"dwconv7_ln", "maxvit_stem"},
                "biastail": {"conv_bf16", "conv2d_nhwc"}}.get(mutant, {"conv_bf16"})
    assert ops_hit >= want_ops, (mutant, want_ops - ops_hit)
    if mutant == "origin":  # both conventions: the symmetric pad (exact family) and the right / bottom pad (MaxViT kernels, by the bound)
        rb = [c for c in CC.CASES if c.family == "cancel" and c.op in ("maxvit_stem", "dwconv3") and CC.mutant_applies(c, mutant)]
        hit = {c.op for c in rb if not CC.accepts(c, CC.mutant_output(c, solved(c)[0], mutant), solved(c)[1])[0]}
        assert hit == {"maxvit_stem", "dwconv3"}


def test_correct_outputs_are_not_rejected_by_the_mutant_machinery(solved):
    """mutant_output() without a defect is the reference rounded once: accepted everywhere (the rejections above are the defects')."""
    for case in CC.CASES[::7]:
        inp, ref = solved(case)
        r = CC.forward(case, inp)
        out = {"y": CC.store(r["want"], case.ydt)}
        if "psum" in r:
            out["psum"] = r["psum"].float()
        assert CC.accepts(case, out, ref)[0], case.id
