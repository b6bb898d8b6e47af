"""Keeps the adversarial decode-step suite (tests/test_hip_decode_adversarial.py) honest without a GPU: a correct kernel
(decode_cases.emulate: fp32 torch in its own summation order over the explicit three-term split) passes every assertion the GPU test
makes (decode_cases.judge, the same function) at MARGIN 1.0, the exact cases bit for bit; every defect in decode_cases.MUTANTS fails at
least one case decisively; the input families' preconditions hold; the three-term split is exact where the contract says it is and is
not where it says it is not; and, with the library built, the host-only pm_dec_linear_plan sends every case to the instantiation it is
listed under and the case list reaches every path tag - the switches' cases in one child process each (the children call the query only)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import decode_cases as DC

torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = DC.build(case)
            cache[case.id] = (inp, DC.reference(case, inp))
        return cache[case.id]

    return get


LAUNCHED = [c for c in DC.CASES if not c.refused]


@pytest.mark.parametrize("case", LAUNCHED, ids=lambda c: c.id)
def test_correct_kernel_passes(solved, case):
    inp, ref = solved(case)
    rec = DC.judge(case, inp, ref, DC.emulate, margin=1.0)
    assert rec["ok"], DC.explain(rec)
    if case.family == "exact":
        assert rec["ratio"] == 0.0


@pytest.mark.parametrize("case", [c for c in LAUNCHED if c.family == "exact" and c.op in DC.MODE], ids=lambda c: c.id)
def test_exact_family_preconditions(solved, case):
    inp, ref = solved(case)
    pre = DC.exact_preconditions(case, inp, ref)
    assert pre["integral"] and pre["limit"] < 2 ** 24, pre  # every partial sum, in any order, is an integer below 2^24
    assert pre["zeros"] > 0.3 and pre["mid_share"] > 0.25 and pre["lo_rows"] and pre["w_varies"], pre
    if case.op == "qkv":
        assert pre["wide_share"] >= 0.10, pre  # k / v values that need more than 8 significant bits
        assert pre["ties"] >= 4 and 0 < pre["ties_even_down"] < pre["ties"], pre  # exact halfway points, rounding down and up


@pytest.mark.parametrize("case", [c for c in LAUNCHED if c.family == "tie"], ids=lambda c: c.id)
def test_tie_family_preconditions(solved, case):
    pre = DC.tie_preconditions(case, solved(case)[1])
    assert pre["decisive"] and pre["global_decisive"], pre  # every logit that is not a planted copy: >= 4 x the bound below the winner
    assert pre["tied_tiles"] >= 3 and pre["global_tied"] == 2, pre  # tiles 0, 1 and the last hold an exact tie; so do the tile winners


@pytest.mark.parametrize("case", [c for c in LAUNCHED if c.family == "scale"], ids=lambda c: c.id)
def test_scale_family_stays_in_range(solved, case):
    pre = DC.scale_preconditions(case, solved(case)[0])
    assert pre["ok"], pre


def test_offset_family_is_offset(solved):
    for case in (c for c in LAUNCHED if c.family == "offset"):
        x = solved(case)[0]["x"].double()
        r = (x.mean(-1).abs() / x.std(-1, unbiased=False))
        assert case.ln and case.K <= 192 and float(r.min()) > 3000 and float(r.max()) < 6000, (case.id, float(r.min()), float(r.max()))


def test_three_term_split_is_exact_where_the_contract_says():
    g = torch.Generator().manual_seed(5)
    ints = torch.cat([torch.arange(0, 1 << 24, 7), torch.arange((1 << 24) - 70000, 1 << 24), torch.randint(0, 1 << 24, (1 << 20,), generator=g)]).float()
    gauss = torch.randn(1 << 20, generator=g)
    for name, x, exact in (("integers below 2^24", ints, True), ("Gaussian", gauss, True), ("Gaussian x 2^100", gauss * 2.0 ** 100, True),
                           ("Gaussian x 2^-90", gauss.abs().clamp_min(1.0) * 2.0 ** -90, True), ("Gaussian x 2^-100", gauss * 2.0 ** -100, False)):
        hi, mid, lo = DC.split3(x)
        same = bool((hi.double() + mid.double() + lo.double() == x.double()).all())
        assert same == exact, f"split3 on {name}: exact = {same}"


def _applies(mutant: str, c: DC.Case) -> bool:
    gemm = c.op in ("linear", "qkv", "ksplit", "kparts", "argmax")
    return {
        "drop_lo": gemm and c.family == "exact", "drop_mid": gemm and c.family == "exact", "trunc_cache": c.op in ("qkv", "fself") and not c.kv32, "kv_row_off": c.op in ("qkv", "fself"),
        "onepass": c.ln and c.family == "offset", "act_after_resid": c.resid and c.act != "none", "bias_shift": c.bias and c.op != "argmax",
        "parts_missing": c.op == "ksplit", "tie_high": c.op in ("argmax", "reduce", "next"), "embed_pos_row": c.op == "embed" and c.pos > 0,
        "tail_pos_row": c.op in ("next", "sample"), "no_forcing": c.op in DC.TOK_OPS and c.pos + 1 < c.P, "margin_top2": c.op in ("next", "reduce"),
        "newest_dropped": c.op == "fself",
    }[mutant]


@pytest.mark.parametrize("mutant", DC.MUTANTS)
def test_mutant_is_rejected(solved, mutant):
    """Smallest applicable cases first; the first DECISIVE rejection (a bit difference of an exact output, or > 10 x the bound) ends the search."""
    tried = []
    for case in sorted((c for c in LAUNCHED if _applies(mutant, c)), key=lambda c: c.M * c.N * c.K):
        inp, ref = solved(case)
        rec = DC.judge(case, inp, ref, lambda c, P: DC.emulate(c, P, mutant))
        tried.append(case.id)
        if not rec["ok"] and (rec["notes"] or rec["ratio"] > 10):
            print(f"{mutant}: rejected by {DC.explain(rec)}")
            return
    pytest.fail(f"{mutant}: accepted by all of {tried}")


def test_one_pass_variance_is_orders_of_magnitude_out(solved):
    for case in (c for c in LAUNCHED if c.family == "offset"):
        inp, ref = solved(case)
        good = DC.judge(case, inp, ref, DC.emulate, margin=1.0)
        bad = DC.judge(case, inp, ref, lambda c, P: DC.emulate(c, P, "onepass"))
        # over many rows the worst is orders of magnitude out; a single row is one draw of the variance's rounding error - still decisive
        assert good["ok"] and bad["ratio"] > (100 if case.M >= 17 else 10), (DC.explain(good), DC.explain(bad))


def test_tie_high_fails_the_tile_winners_and_the_planted_tails(solved):
    """Breaking a tie to the highest index is caught on both sides: per tile and over all tiles (arg-max), and by the planted tile lists."""
    for op in ("argmax", "next", "reduce"):
        case = next(c for c in LAUNCHED if c.op == op and (op == "argmax" or (c.N > 4 and c.pos + 1 >= c.P)))
        inp, ref = solved(case)
        assert not DC.judge(case, inp, ref, lambda c, P: DC.emulate(c, P, "tie_high"))["ok"], case.id


@pytest.mark.parametrize("case", [c for c in LAUNCHED if c.op == "sample"], ids=lambda c: c.id)
def test_sampling_draws_stay_clear_of_every_cumulative_boundary(solved, case):
    """The reference alone shows that no draw of the case list lies within 1e-4 (x the sum) of a cumulative boundary - the share of
    undecidable draws is 0 (the contract allows 1 %) - so the sampled token must equal the reference's for every sequence."""
    inp = solved(case)[0]
    toks, near = DC.sample_pick(case, inp["logits"], inp["seed"])
    assert near > 1e-4 and len(toks) == case.M, (near, inp["seed"])
    lg = inp["logits"]
    assert int(torch.isfinite(lg).sum(-1).min()) >= case.topk  # the -inf entries lie below the top k
    for b, tok in enumerate(toks):  # the pick is one of the k largest
        assert float(lg[b, tok]) >= float(lg[b].topk(case.topk).values[-1])
    v, u = DC.ds_uniform(inp["seed"], case.pos, 0)
    assert 0 <= v < 1 << 24 and u == v / 2 ** 24


@pytest.mark.parametrize("case", [c for c in LAUNCHED if c.family == "needle"], ids=lambda c: c.id)
def test_a_lost_needle_moves_the_fused_self_block_by_ten_bounds(solved, case):
    """The decisive key - the newest one (from LDS), key 0, key Lc - 1, either side of the 256-key group boundary - carries the
    output: a kernel that loses it is >= 10 x the bound out, the correct stand-in stays inside."""
    inp, ref = solved(case)
    assert DC.judge(case, inp, ref, DC.emulate, margin=1.0)["ok"]
    bad = DC.judge(case, inp, ref, lambda c, P: DC.emulate(c, P, "needle_dropped"))
    assert not bad["ok"] and bad["ratio"] >= 10, DC.explain(bad)


def test_no_case_is_a_refusal_in_disguise(solved):
    for case in LAUNCHED:
        inp = solved(case)[0]
        for poison in ((False, True) if case.family == "poison" else (False,)):
            why = DC.abi_refusal(case, DC.place(case, inp, poison=poison))
            assert why is None, f"{case.id} (poison={poison}): {why}"
    assert all(c.M * c.N * c.K <= 80e6 and c.N * c.K * 2 <= 5e6 for c in DC.CASES if c.op in DC.MODE), "a case outgrew the suite's size limits"


# --------------------------------------------------------------------------------------------------------------- dispatch
def _lib_built() -> bool:
    from pytorch_models import _hip

    return os.path.exists(_hip.LIB_PATH)


@pytest.fixture(scope="module")
def reports():
    """case id -> pm_dec_linear_plan's report: the default-dispatch cases asked here, each switch's cases in a fresh child (host only)."""
    assert _lib_built(), "build the library first (the dispatch check needs pm_dec_linear_plan)"
    from pytorch_models._hip import ops

    out = {c.id: ops.dec_linear_plan(**DC.plan_args(c)) for c in DC.CASES if not c.env and c.op in DC.MODE}
    for env, switches in DC.ENVS.items():
        if not env:
            continue
        r = subprocess.run([sys.executable, os.path.join(HERE, "decode_child.py"), "plan", env], env=dict(os.environ, **switches),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert set(got) == {c.id for c in DC.CASES if c.env == env}
        out.update(got)
    return out


def test_every_case_goes_where_the_table_says(reports):
    wrong = {}
    for c in DC.CASES:
        if c.op not in DC.MODE:
            continue
        rep = reports[c.id]
        if c.refused:
            if rep != {"refused": c.refused}:
                wrong[c.id] = rep
            continue
        bad = {k: (v, rep.get(k)) for k, v in c.expect if rep.get(k) != v}
        if bad or "refused" in rep:
            wrong[c.id] = bad or rep
    assert not wrong, f"pm_dec_linear_plan sends these cases elsewhere (field: (listed, reported)): {wrong}"


def test_every_path_is_reached(reports):
    reached = set().union(*(DC.paths(c, reports.get(c.id, {})) for c in DC.CASES))
    assert not DC.REQUIRED_PATHS - reached, sorted(DC.REQUIRED_PATHS - reached)


def test_plan_matches_the_launchers_arithmetic(reports):
    """The report against the launcher's documented arithmetic, restated here: grid = (feature tiles, K parts, row tiles on their own)."""
    for c in DC.CASES:
        if c.op not in DC.MODE or c.refused:
            continue
        rep = reports[c.id]
        if rep["kernel"] == "logits":
            assert rep["tiles"] == c.ntiles and rep["gx"] <= rep["tiles"] and rep["gy"] == rep["gz"] == 1 and rep["waves"] * rep["NSTEP"] == 16, (c.id, rep)
            continue
        feats = 16 * rep["FT"]
        assert rep["gx"] == rep["tiles"] == (c.N + feats - 1) // feats and rep["gy"] == max(c.k_split, 1) and rep["waves"] == 4, (c.id, rep)
        assert rep["gz"] * rep["MT"] * 16 >= c.M and (rep["gz"] == 1 or rep["MT"] == 1) and rep["LN"] == int(c.ln), (c.id, rep)
        if c.op == "argmax":
            assert 16 * rep["FT"] == c.tile, (c.id, rep)


def test_plan_is_host_only_and_refuses_like_the_launchers():
    assert _lib_built()
    from pytorch_models._hip import lib

    L = lib()
    rep = (ctypes.c_int32 * 10)()
    p = ctypes.addressof(rep)
    assert L.pm_dec_linear_plan(17, 130, 160, 0, 0, 0, None) == 1  # no report: PM_EINVAL
    assert L.pm_dec_linear_plan(65, 130, 160, 0, 0, 0, p) == 2 and L.pm_dec_linear_plan(17, 130, 168, 0, 0, 0, p) == 2  # M > 64, K % 32
    assert L.pm_dec_linear_plan(17, 130, 1312, 1, 0, 0, p) == 2  # LayerNorm beyond K = 1280
    assert L.pm_dec_linear_plan(49, 2752, 544, 1, 0, 0, p) == 2  # LayerNorm, more than two row tiles and more than 4 K steps per wave
    assert L.pm_dec_linear_plan(17, 130, 160, 0, 4, 0, p) == 1 and L.pm_dec_linear_plan(17, 130, 64, 0, 0, 3, p) == 1  # mode, K / 32 < k_split
    assert L.pm_dec_linear_plan(17, 130, 160, 1, 0, 2, p) == 1  # the K split has no LayerNorm
    assert L.pm_dec_linear_plan(17, 130, 160, 0, 0, 0, p) == 0 and list(rep)[:6] == [0, 1, 1, 4, 0, 4]


def test_gpu_file_calls_every_entry_point_of_the_table():
    """The entry points this suite covers are called by decode_cases.run; the rest of decode.hip's pm_dec_* keep their own tests."""
    src = open(os.path.join(HERE, "decode_cases.py")).read()
    for name in ("pm_dec_linear", "pm_dec_linear_ksplit", "pm_dec_linear_kparts", "pm_dec_embed", "pm_dec_argmax_reduce", "pm_dec_next_token",
                 "pm_dec_sample_topk", "pm_dec_attention_fused", "pm_dec_attention_fused_kv32", "pm_dec_attention_chain"):
        assert re.search(rf"L\.{name}\b(?!_)", src), name
