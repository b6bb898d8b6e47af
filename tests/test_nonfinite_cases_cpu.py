"""CPU: the non-finite operand contract without a GPU (tests/nonfinite_cases.py).

  * the protocol has teeth: toy ops with each defect planted - a masked neighbour multiplied by 0 instead of skipped, a workspace
    reduced over all samples, an arg-max that keeps its 0x7fffffff start, a comparison clamp that turns NaN into 0, a poison
    nothing reads - are each reported, and the correct twin of each passes;
  * the tables are complete and consistent with the CPU builds of wrapper_cases.ROWS (shapes come from the recording stub of
    tests/test_wrapper_cases_cpu.py: the wrappers allocate their results, nothing is launched);
  * the families hold what their names say, and torch's own arg-max / sort give on them what the contract states;
  * the models with a CPU form run the model protocol end to end."""
import pytest
import torch

import coherence_cases as CC
import graph_cases as GC
import nonfinite_cases as NF
import wrapper_cases as WC
from pytorch_models._hip import ops
from test_wrapper_cases_cpu import _install

torch.set_grad_enabled(False)
CPU = torch.device("cpu")
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------------------- planted defects
def _x(seed=0, S=4):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn((S, 3, 5), generator=g)}


def _named(fn):
    return lambda kw: [("output 0", fn(kw["x"]).clone())]


UNIT = NF.U("x")


def per_sample_sum(x):  # the correct twin: a sample reads its own rows only
    return x.sum(1)


def masked_neighbour_times_zero(x):  # every sample's rows enter every sum, the neighbours' weighted by 0: 0 x NaN = NaN
    w = torch.eye(x.shape[0])
    return torch.einsum("bc,cld->bd", w, x)


def shared_workspace(x):  # per-sample partial maxima land in one workspace that is then reduced over ALL samples
    ws = x.amax((1, 2))
    return x.sum(1) - ws.max()


def own_workspace(x):
    return x.sum(1) - x.amax((1, 2))[:, None]


def compare_clamp(x):  # relu by comparison: NaN > 0 is false, the NaN becomes 0
    y = x.sum(1)
    return torch.where(y > 0, y, torch.zeros_like(y))


def ignores_first_column(x):
    return x[:, :, 1:].sum(1)


@pytest.mark.parametrize("poison", NF.POISONS)
def test_correct_twins_pass(poison):
    for fn in (per_sample_sum, own_workspace):
        assert NF.check_isolation(_named(fn), _x(), UNIT, poison) == [], fn.__name__


def test_a_neighbour_multiplied_by_zero_is_reported():
    for poison in ("nan", "+inf", "-inf"):  # 0 x inf = NaN as well; 0 x a finite value is the leak no finite suite can see
        problems = NF.check_isolation(_named(masked_neighbour_times_zero), _x(), UNIT, poison)
        assert any("another sample holds a non-finite value" in p for p in problems), (poison, problems)
    assert NF.check_isolation(_named(masked_neighbour_times_zero), _x(), UNIT, "max") == []


def test_a_workspace_reduced_over_all_samples_is_reported():
    for poison in ("nan", "+inf", "max"):
        problems = NF.check_isolation(_named(shared_workspace), _x(), UNIT, poison)
        assert any("another sample" in p for p in problems), (poison, problems)


def test_a_comparison_clamp_is_reported_unless_listed():
    kw = {"x": _x()["x"].abs()}  # positive sums: the clamp is the identity on the clean run
    problems = NF.check_isolation(_named(compare_clamp), kw, UNIT, "nan")
    assert len(problems) == 1 and "swallowed" in problems[0], problems
    assert NF.check_isolation(_named(compare_clamp), kw, UNIT, "nan", swallows=True) == []
    stale = NF.check_isolation(_named(per_sample_sum), kw, UNIT, "nan", swallows=True)  # a listed case that swallows nothing
    assert len(stale) == 1 and "stale" in stale[0], stale
    # per operand: y's clamp is listed, x (added behind it) is not - a swallow on x is reported although the row is listed
    two = {"x": kw["x"], "y": kw["x"].clone()}
    unit2 = NF.U("x", "y")
    behind = lambda k: [("output 0", compare_clamp(k["y"]) + k["x"].sum(1))]  # noqa: E731
    both = lambda k: [("output 0", compare_clamp(k["y"]) + compare_clamp(k["x"]))]  # noqa: E731
    assert NF.check_isolation(behind, two, unit2, "nan", swallows=("y",)) == []
    found = NF.check_isolation(both, two, unit2, "nan", swallows=("y",))
    assert len(found) == 1 and found[0].startswith("x[") and "swallowed" in found[0], found
    found = NF.check_isolation(behind, two, unit2, "nan", swallows=("x", "y"))
    assert len(found) == 1 and found[0].startswith("x[") and "stale" in found[0], found


def test_a_poison_nothing_reads_proves_nothing():
    with pytest.raises(NF.CaseProvesNothing, match="not read"):
        NF.check_isolation(_named(ignores_first_column), _x(), UNIT, "nan")
    kw = _x()
    kw["x"][2, 1, 1] = INF
    with pytest.raises(NF.CaseProvesNothing, match="already non-finite"):
        NF.check_isolation(_named(per_sample_sum), kw, UNIT, "nan")


def test_a_call_that_raises_is_a_problem_and_a_device_error_stops():
    def refuses(kw):
        if bool(kw["x"].isnan().any()):
            raise ValueError("non-finite operand")
        return [("output 0", kw["x"].sum(1))]

    def faults(kw):
        raise RuntimeError("HIP error: an illegal memory access was encountered")
    assert any("raised ValueError" in p for p in NF.check_isolation(refuses, _x(), UNIT, "nan"))
    with pytest.raises(WC.GpuFault):
        NF.check_isolation(faults, _x(), UNIT, "nan")


def test_an_integer_outside_its_range_and_a_changed_shared_result_are_reported():
    def run(kw):
        x = kw["x"]
        best = x.sum(1).argmax(-1)
        best = torch.where(x.isnan().any(2).any(1), torch.full_like(best, NF.NONE_IDX), best)
        return [("output 0", x.sum(1)), ("best", best), ("count", x.isnan().sum().view(1))]
    unit = NF.U("x", outs={"count": NF.SHARED}, ranges={"best": (0, 5)})
    problems = NF.check_isolation(run, _x(), unit, "nan")
    assert any("2147483647 lies outside [0, 5)" in p for p in problems) and any("no sample owns" in p for p in problems), problems


def _toy_decision(guarded: bool) -> NF.Decision:
    def run(dev, family, V, clean):
        c, rows = NF.family_rows(family, V)
        rows = c if clean else rows
        val, idx = NF.tile_winners(rows, tile=V)  # one tile: the kernels' own loop, strict > from (-inf, none)
        best = idx[:, 0].long()
        if guarded:
            best = torch.where(best == NF.NONE_IDX, torch.zeros_like(best), best)
        lse = torch.logsumexp(rows, -1)
        return {"best": (best, 0, V)}, {"lse": lse}, rows
    return NF.Decision("toy", run, sizes=(5,), pick=lambda ints, u: [int(ints["best"][0][u])], ref=lambda row: [NF.lowest_argmax(row)])


@pytest.mark.parametrize("family", ["all_nan", "all_neginf"])
def test_an_argmax_that_keeps_its_start_is_reported(family):
    problems = NF.check_decision(_toy_decision(False), CPU, family, 5)
    assert any("2147483647 lies outside [0, 5)" in p for p in problems), problems
    assert NF.check_decision(_toy_decision(True), CPU, family, 5) == []


def test_the_guarded_toy_decision_passes_every_family():
    for family in NF.FAMILIES:
        assert NF.check_decision(_toy_decision(True), CPU, family, 5) == [], family


def test_ignored_regions_are_checked_both_ways():
    seq = ops.SeqLens([2, 3], torch.tensor([0, 2, 5], dtype=torch.int32), 3)
    kw = {"x": torch.randn(2, 3, 4), "seq": seq}
    masks = {"x": NF.IGNORED["rows_pack"]["x"]}

    def skips(k):  # the correct twin: padded rows are not read
        return [("output 0", torch.cat([k["x"][b, :n] for b, n in enumerate(k["seq"].lengths)]).clone())]

    def multiplies(k):  # padded rows multiplied by 0
        keep = (torch.arange(3)[None, :] < torch.tensor(k["seq"].lengths)[:, None]).float()
        return [("output 0", (k["x"] * keep[..., None]).sum(1))]
    assert NF.check_ignored(skips, kw, masks) == []
    assert NF.check_ignored(multiplies, kw, masks), "0 x NaN must be reported"


# ---------------------------------------------------------------------------------------------------------------- completeness
def test_every_row_is_in_exactly_one_table():
    assert set(NF.UNITS) | set(NF.NO_UNITS) == set(WC.ROWS)
    assert not set(NF.UNITS) & set(NF.NO_UNITS)
    assert all(isinstance(v, str) and v for v in list(NF.NO_UNITS.values()) + list(NF.SWALLOWS.values()))


def test_every_table_id_exists():
    models = set(GC.MODELS)
    assert set(NF.SWALLOWS) <= set(NF.UNITS) | models | set(NF.ENTRY_POINTS), set(NF.SWALLOWS) - set(NF.UNITS) - models
    for named in ("Whisper.generate", "WhisperDecoder.generate:beam", "T5Model.generate", "Wav2Vec2CTC.decode", "Wav2Vec2CTC.score",
                  "Wav2Vec2CTC.align", "Whisper.align"):  # (EnCodec.encode is a row of MODELS)
        assert named in NF.ENTRY_POINTS
    assert set(NF.IGNORED) <= set(WC.ROWS)
    assert set(NF.MODELS_POISON) == models, set(NF.MODELS_POISON) ^ models
    for key, mp in NF.MODELS_POISON.items():
        assert (mp.input is None) == bool(mp.why), key
    for d in NF.DECISIONS.values():
        assert set(d.families) <= set(NF.FAMILIES) | ({"one_finite"} if d.id == "dec_beam" else set()) and d.sizes and d.families, d.id
    wanted = ("dec_argmax", "dec_next_token", "dec_sample_topk", "dec_sample:k0", "dec_sample:k3", "dec_sample:T0", "dec_beam", "t5_next_token", "ctc_head",
              "ctc_greedy", "ctc_viterbi", "lm_score", "rvq_encode", "align_dtw")
    assert set(wanted) <= set(NF.DECISIONS)
    assert sum(51865 in d.sizes for d in NF.DECISIONS.values()) >= 9  # Whisper's vocabulary once per entry point that has one


def test_no_units_rows_have_no_per_sample_float_operand():
    for rid in NF.NO_UNITS:
        kw = WC.ROWS[rid].build(CPU)
        floats = [p[0] for p, t in WC.operands(kw) if t.is_floating_point() and p[0] not in WC.ROWS[rid].inplace]
        assert set(floats) <= {"emb", "pos", "pos_tab", "codebooks"}, (rid, floats)


def test_swallows_hold_only_the_two_allowed_kinds():
    assert not set(NF.SWALLOWS_CLAMP) & set(NF.SWALLOWS_NO_FLOAT) and set(NF.SWALLOWS) == set(NF.SWALLOWS_CLAMP) | set(NF.SWALLOWS_NO_FLOAT)
    for key, why in NF.SWALLOWS_CLAMP.items():
        assert "fmaxf" in why and ".hip:" in why or "common.h:" in why, key  # the clamp and its kernel line
    for key, names in NF.SWALLOWED_OPERANDS.items():
        assert key in NF.SWALLOWS_CLAMP and set(names) <= {WC.path_name(p) for p, _, _ in NF.UNITS[key].operands}, key
    for key in NF.SWALLOWS_CLAMP:  # a clamp row with several operands says which of them the clamp stands behind
        assert key not in NF.UNITS or len(NF.UNITS[key].operands) == 1 or key in NF.SWALLOWED_OPERANDS, key
    assert NF.swallowed("linear_f32") == ("x",) and NF.swallowed("rvq_encode") is True and NF.swallowed("linear") is False


@pytest.mark.parametrize("rid", list(NF.PAD_COLUMNS))
def test_pad_column_operands_have_the_rowpad_variant_and_are_accepted(rid, monkeypatch):
    """ties PAD_COLUMNS to section 26: each listed operand has a "rowpad" variant (a view into a NaN parent) and its wrapper takes it"""
    _install(monkeypatch)
    r = WC.ROWS[rid]
    kw = r.build(CPU)
    for name in NF.PAD_COLUMNS[rid]:
        assert kw[name].is_floating_point() and name not in r.inplace
        v = [v for v in WC.variants(kw[name].clone()) if v.tag == "rowpad"]
        assert len(v) == 1 and v[0].tensor.stride(-2) == kw[name].shape[-1] + 8 and bool(v[0].parent.isnan().any())
        WC.call(ops, r, WC.replaced(r.build(CPU), (name,), v[0].tensor))  # a refusal raises
    assert NF.check_pad_columns(lambda k: [("output 0", k[NF.PAD_COLUMNS[rid][0]].sum(-1))], kw, NF.PAD_COLUMNS[rid][:1]) == []


def test_pad_columns_cover_the_ctc_rows_and_a_leak_is_reported():
    assert {"ctc_forward", "ctc_viterbi", "ctc_head"} <= set(NF.PAD_COLUMNS)
    kw = {"x": torch.randn(4, 6)}
    reads_packed = lambda k: [("output 0", k["x"].as_strided((4, 6), (6, 1)).sum(-1))]  # noqa: E731 - takes data_ptr() as packed
    assert NF.check_pad_columns(lambda k: [("output 0", k["x"].sum(-1))], kw, ("x",)) == []
    assert NF.check_pad_columns(reads_packed, kw, ("x",))  # the leading dimension ignored: the pad columns' NaN is read


@pytest.mark.parametrize("rid", list(NF.UNITS))
def test_unit_matches_the_cpu_build(rid, monkeypatch):
    _install(monkeypatch)
    r, unit = WC.ROWS[rid], NF.UNITS[rid]
    kw = r.build(CPU)
    S = NF.n_samples(unit, kw)
    assert S >= 2, "at least two samples"
    u = NF.unit_sample(S)
    assert 0 < u and (u < S - 1 or S == 2)
    lengths = NF._lengths(unit, kw)
    for which, (path, dim, _) in enumerate(unit.operands):
        t = WC.get(kw, path)
        assert t.is_floating_point(), f"{rid}: {WC.path_name(path)} is {t.dtype}"
        assert (NF.sample_ids(t.shape[dim], S, lengths) == u).any()
        got, idx = NF.poisoned(GC.clone_kw(kw), unit, which, NAN, u, S, "nan")
        assert int(WC.get(got, path).isnan().sum()) == 1 and not bool(t.isnan().any()), "one element, of a clone"
    snap = WC.snapshot(r, kw, WC.call(ops, r, kw))
    names = [n for n, _ in snap]
    assert names, rid
    assert set(unit.outs or {}) <= set(names) and set(unit.ranges) <= set(names), (rid, names)
    for name, t in snap:
        spec = (unit.outs or {}).get(name, 0)
        if spec in (NF.SHARED, NF.SKIP):
            continue
        ids = NF.sample_ids(t.shape[spec], S, lengths)  # raises where the extent does not hold the samples
        assert (ids == u).any(), (rid, name)
        if name in unit.ranges:
            assert not t.is_floating_point(), (rid, name)
    floats = [n for n, t in snap if t.is_floating_point() and (unit.outs or {}).get(n, 0) != NF.SKIP]
    no_float = rid in NF.SWALLOWS_NO_FLOAT
    assert floats or no_float, f"{rid}: no float result and no SWALLOWS entry saying so"


@pytest.mark.parametrize("rid", list(NF.IGNORED))
def test_ignored_masks_fit_the_cpu_build(rid, monkeypatch):
    _install(monkeypatch)  # (a row may size its workspace through the library)
    kw = WC.ROWS[rid].build(CPU)
    for name, mask_of in NF.IGNORED[rid].items():
        m = mask_of(kw)
        assert m.shape == kw[name].shape and m.dtype == torch.bool and bool(m.any()) and not bool(m.all()), (rid, name)
        assert kw[name].is_floating_point()


# -------------------------------------------------------------------------------------------------------------------- families
@pytest.mark.parametrize("V", [5, 1000, 51865])
def test_families_hold_what_their_names_say(V):
    for family in NF.FAMILIES:
        clean, rows = NF.family_rows(family, V)
        assert rows.shape == (NF.ROWS_B, V) and NF.ROWS_B >= 3 and 0 < NF.ROW_U < NF.ROWS_B - 1
        keep = [b for b in range(NF.ROWS_B) if b != NF.ROW_U]
        assert torch.equal(rows[keep], clean[keep]) and bool(torch.isfinite(clean).all())
        row, nan = rows[NF.ROW_U], rows[NF.ROW_U].isnan()
        if family == "all_nan":
            assert bool(nan.all())
        elif family == "all_neginf":
            assert bool((row == -INF).all())
        elif family.startswith("nan_"):
            at = {"nan_first": 0, "nan_last": V - 1, "nan_tile_edge": NF.tile_edge(V)}[family]
            assert nan.nonzero().flatten().tolist() == [at] and bool(torch.isfinite(row[~nan]).all())
        elif family == "two_posinf":
            a, b = (row == INF).nonzero().flatten().tolist()
            assert (a // NF.TILE != b // NF.TILE) or V <= NF.TILE
            assert int(torch.isfinite(row).sum()) == V - 2
        else:
            assert bool((row == row[0]).all()) and bool(torch.isfinite(row).all())
    assert NF.tile_edge(1000) % NF.TILE == 0 and NF.tile_edge(51865) % NF.TILE == 0
    row = NF.family_rows("one_finite", V, NF.BEAM_W * NF.BEAM_CLIPS, 2)[1][2]
    assert int(torch.isfinite(row).sum()) == 1 < NF.BEAM_W and int(row.isnan().sum()) == V - 1
    assert "one_finite" in NF.DECISIONS["dec_beam"].families and NF.DECISIONS["dec_beam"].distinct == ("cand_tok",)


@pytest.mark.parametrize("V", [5, 200])
def test_gemm_rows_are_what_the_product_gives(V):
    for family in NF.FAMILIES:
        h0, h, w, rows = NF.gemm_rows(family, V)
        got = h.float() @ w.float().t()
        assert torch.equal(got.isnan(), rows.isnan()) and torch.equal(got.nan_to_num(7.0), rows.nan_to_num(7.0)), family
        clean = h0.float() @ w.float().t()
        keep = [b for b in range(NF.ROWS_B) if b != NF.ROW_U]
        assert torch.equal(clean[keep], rows[keep]) and bool(torch.isfinite(clean[keep]).all())
        assert bool(torch.isfinite(w.float()).all()), "a weight is shared: it stays finite"


def test_torch_gives_the_decisions_the_contract_states():
    for V in (5, 1000):
        for family in ("all_neginf", "all_equal"):
            row = NF.family_rows(family, V)[1][NF.ROW_U]
            assert NF.lowest_argmax(row) == 0 and NF.top_order(row, 3) == [0, 1, 2]
        row = NF.family_rows("two_posinf", V)[1][NF.ROW_U]
        assert [NF.lowest_argmax(row)] == NF.top_order(row, 1) and NF.top_order(row, 2) == list(NF.two_columns(V))
        assert set(NF.top_order(row, 2)) == set(torch.topk(row, 2).indices.tolist())
        # torch treats NaN as the maximum: the arg-max of a row with a NaN is the NaN's index, which is why the contract asks a
        # kernel for "a valid index" there and nothing more
        for family, at in (("nan_first", 0), ("nan_last", V - 1), ("nan_tile_edge", NF.tile_edge(V))):
            assert int(torch.argmax(NF.family_rows(family, V)[1][NF.ROW_U])) == at
        g = NF.gaussian_rows(V)[0]
        assert NF.lowest_argmax(g) == int(g.argmax()) and NF.top_order(g, 3) == torch.topk(g, 3).indices.tolist()


def test_tile_winners_are_the_kernels_loop():
    for family in NF.FAMILIES:
        _, rows = NF.family_rows(family, 1000)
        val, idx = NF.tile_winners(rows)
        for b in range(NF.ROWS_B):
            for t in range(val.shape[1]):
                bv, bi = -INF, NF.NONE_IDX
                for i in range(t * NF.TILE, min((t + 1) * NF.TILE, 1000)):
                    if float(rows[b, i]) > bv:
                        bv, bi = float(rows[b, i]), i
                assert (float(val[b, t]), int(idx[b, t])) == (bv, bi), (family, b, t)


# ---------------------------------------------------------------------------------------------------------------------- models
CPU_MODELS = ("ViT", "WhisperEncoder", "WhisperDecoder", "Whisper")  # the classes pytorch_models/_cpu.py serves


@pytest.mark.parametrize("key", CPU_MODELS)
@pytest.mark.parametrize("poison", NF.POISONS)
def test_models_with_a_cpu_form_run_the_protocol(key, poison):
    case, mp = GC.MODELS[key], NF.MODELS_POISON[key]
    k = NF.model_geometry(case)
    m = CC.filled(case.make(k), 411)
    kw = {f"x{i}": x for i, x in enumerate(case.inputs(k, 411))}
    assert kw["x0"].shape[0] == 3
    problems = NF.check_isolation(NF.model_run(m), kw, NF.model_unit(mp), poison, swallows=NF.swallowed(key))
    assert problems == [], problems
