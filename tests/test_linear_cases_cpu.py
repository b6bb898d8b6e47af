"""Keeps the adversarial GEMM / LayerNorm-fold suite (tests/test_hip_linear_adversarial.py) honest without a GPU: a correct kernel
(linear_cases.emulate: fp32 torch in its own summation order, the epilogue in fp32, one store) passes every assertion the GPU test
makes (linear_cases.judge, the same function) at MARGIN 1.0; every defect in linear_cases.MUTANTS fails at least one case; the case
lists reach every path they are named for; the exact family's preconditions hold; and, with the library built, the host-only
pm_linear_bf16_plan sends every case to the kernel it is listed under - unforced for the default-dispatch cases, in one child
process per PM_GEMM_KERNEL value for the forced ones (the children call the query only: nothing is launched).

Far operands (linear_cases, "far operands"): every far case keeps the exact family's preconditions and satisfies the arena's
containment rule as pure arithmetic (no memory is mapped); the reach table is asserted against pm_linear_bf16_plan - for arguments
just beyond a kernel id's reach in one operand the plan never returns that id, forced or not -; and every reach bound whose operand
fits the arena has a far case that crosses it, so the table is tied to the kernels on the GPU and not only to itself."""
import json
import os
import subprocess
import sys

import pytest
import torch

import linear_cases as LC

torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def solved():
    """(inputs, reference) per case id, computed once and left unchanged (the big forced shapes are dropped again after use)."""
    cache = {}

    def get(case):
        if case.id in cache:
            return cache[case.id]
        inp = LC.build(case)
        hit = (inp, LC.reference(case, inp))
        if case.M * case.N <= 1 << 20:
            cache[case.id] = hit
        return hit

    return get


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_correct_kernel_passes(solved, case):
    inp, ref = solved(case)
    rec = LC.judge(case, inp, ref, LC.emulate, margin=1.0)
    assert rec["ok"], LC.explain(rec)
    if case.family == "exact" and case.op == "linear":
        pre = LC.exact_preconditions(case, inp, ref)
        assert pre["limit"] < 2 ** 24 and pre["integral"], pre
        assert pre["share"] >= 0.10, f"{case.id}: only {pre['share']:.3f} of the pre-residual values exceed 256"
        w = inp["w"].float()
        assert (w[1:] != w[:-1]).any(1).all() if case.N > 1 else True, "w must differ along n"
        assert (w[:, 1:] != w[:, :-1]).any(), "w must differ along k"


def _applies(mutant: str, c: LC.Case) -> bool:
    gemm = c.op in ("linear", "linear_f32")
    return {
        "ktail": gemm and c.K % 64 != 0, "biaslane": gemm and c.bias and not c.consumer, "residrow": gemm and bool(c.resid),
        "padstore": c.op in ("linear", "linear_f32", "layernorm"), "trunc": c.ydt == "bf16" and c.op in ("linear", "layernorm"),
        "round_first": bool(c.resid) and c.ydt == "bf16", "resid_first": gemm and bool(c.resid) and c.act != "none",
        "lns_shift": c.consumer and c.N > 64, "meanrstd": c.consumer, "rows_unrounded": c.rows, "rows_block": c.rows and c.N > 64,
        "onepass": c.op in ("layernorm", "row_stats"), "fin_drop": c.op == "finalize", "kswap": gemm and c.K >= 16,
        "tileswap": c.kid in (6, 7) and c.N > 256, "gelu_tail": c.op == "linear" and c.act == "gelu" and c.ydt == "bf16",
    }[mutant]


@pytest.mark.parametrize("mutant", LC.MUTANTS)
def test_mutant_is_rejected(solved, mutant):
    """Smallest applicable cases first; the first rejection ends the search."""
    tried = []
    for case in sorted((c for c in LC.CASES if _applies(mutant, c)), key=lambda c: c.M * c.N * max(c.K, 1)):
        inp, ref = solved(case)
        rec = LC.judge(case, inp, ref, lambda c, P: LC.emulate(c, P, mutant))
        tried.append(case.id)
        if not rec["ok"]:
            print(f"{mutant}: rejected by {LC.explain(rec)}")
            return
    pytest.fail(f"{mutant}: accepted by all of {tried}")


def test_gelu_tail_fails_the_sweep(solved):
    """Today's contract rejects yesterday's gelu_poly: the unclamped outer factor leaves +4.0e-6 |x| for x <= -4.5."""
    case = next(c for c in LC.CASES if c.family == "actsweep" and c.kid == 1 and c.act == "gelu" and c.ydt == "bf16")
    inp, ref = solved(case)
    assert LC.judge(case, inp, ref, LC.emulate, margin=1.0)["ok"]
    rec = LC.judge(case, inp, ref, lambda c, P: LC.emulate(c, P, "gelu_tail"))
    assert not rec["ok"] and rec["ratio"] > 5, LC.explain(rec)
    x = LC.sweep().double()
    err = (LC.gelu_poly32(x.float()).double() - ref["pre"][0]).abs()
    assert float(err.max()) <= LC.GELU_POLY_ABS, f"gelu_poly's stated bound fails in the fp32 emulation: {float(err.max()):.3e} at x = {float(x[err.argmax()])}"


def test_no_case_is_a_refusal_in_disguise(solved):
    for case in LC.CASES:
        inp = solved(case)[0] if case.M * case.N <= 1 << 20 else LC.build(case)
        for poison in ((False, True) if case.family == "poison" else (False,)):
            why = LC.abi_refusal(case, LC.place(case, inp, poison=poison))
            assert why is None, f"{case.id} (poison={poison}): {why}"


def test_every_path_is_reached():
    reached = set().union(*(LC.paths(c) for c in LC.CASES))
    assert not LC.REQUIRED_PATHS - reached, sorted(LC.REQUIRED_PATHS - reached)
    for k in LC.FORCED_IDS:
        assert LC.FORCED_CASES[k], k
    assert all(c.M * max(c.K, c.N) * 2 <= 26e6 and c.M * c.N * max(c.K, 1) <= 1.1e9 for c in LC.CASES), "a case outgrew the suite's size limits"


# --------------------------------------------------------------------------------------------------------------- dispatch
def _lib_built() -> bool:
    from pytorch_models import _hip

    return os.path.exists(_hip.LIB_PATH)


def test_default_cases_dispatch_to_their_kernel():
    assert _lib_built(), "build the library first (the dispatch check needs pm_linear_bf16_plan)"
    from pytorch_models._hip import ops

    wrong = {}
    for case in LC.DEFAULT_CASES:
        if case.op != "linear":
            continue
        P = LC.place(case, LC.build(case))
        for Q in (P, LC.place(case, LC.build(case), poison=True)) if case.family == "poison" else (P,):
            got = LC.plan(ops, case, Q)
            if got != case.kid:
                wrong[case.id] = got
    assert not wrong, f"the default dispatcher sends these cases elsewhere: {wrong}"


@pytest.mark.parametrize("kid", LC.FORCED_IDS)
def test_forced_cases_dispatch_to_their_kernel(kid):
    """PM_GEMM_KERNEL is read once per process and falls through silently: a fresh child per value asks the host-only query."""
    assert _lib_built(), "build the library first (the dispatch check needs pm_linear_bf16_plan)"
    env = dict(os.environ, PM_GEMM_KERNEL=str(kid))
    r = subprocess.run([sys.executable, os.path.join(HERE, "linear_child.py"), "plan", str(kid)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(got) == {c.id for c in LC.FORCED_CASES[kid]}
    wrong = {k: v for k, v in got.items() if v != kid}
    assert not wrong, f"PM_GEMM_KERNEL={kid} does not reach kernel {kid} on: {wrong}"


# --------------------------------------------------------------------------------------------------------------- far operands
@pytest.fixture(scope="module")
def far_arena():
    import wrapper_cases as WC
    a = WC.Arena(WC.Arena.bytes_for(32), "cpu", poisoned=False)  # torch.empty maps lazily, and nothing below writes to it
    yield a
    del a.words


@pytest.mark.parametrize("case", LC.FAR_CASES, ids=lambda c: c.id)
def test_far_case_is_exact_and_contained(case, far_arena):
    inp = LC.build(case)
    pre = LC.exact_preconditions(case, inp, LC.reference(case, inp))
    assert pre["limit"] < 2 ** 24 and pre["integral"] and pre["share"] >= 0.10, pre
    name, shape, st = LC.far_geometry(case)
    assert (shape[0] - 1) * st[0] * 2 > LC.FAR_DIST[case.far.split(":")[1]] and st[0] % 64 == 0 and st[0] >= shape[1], (name, shape, st)
    P = LC.place_far(case, inp, far_arena, touch=False)
    assert not far_arena.holds(P["far_case"]), far_arena.holds(P["far_case"])
    assert P["far_view"].data_ptr() == far_arena.words.data_ptr() + far_arena.base and P["far_view"].stride() == st
    assert LC.abi_refusal(case, P) is None
    assert LC.plan(ops_module(), case, P) != 0  # the host-only query takes the far call: a kernel id, or minus an error code


def ops_module():
    from pytorch_models._hip import ops

    return ops


def _reach_violations(kid: int, got: dict) -> list[str]:
    bad = [f"{name}: pm_linear_bf16_plan returns kernel {kid} for {g}, beyond its reach in {operand} "
           f"({LC.reach(kid, **g)[operand]} >= 2^32)" for name, (g, operand) in LC.reach_probes(kid).items()
           if operand and got[name] == kid]
    for name, (g, operand) in LC.reach_probes(kid).items():
        assert operand is None or LC.reach(kid, **g)[operand] >= LC.LIMIT32
    return bad


@pytest.mark.parametrize("kid", (3, 6, 7))
def test_plan_never_returns_a_kernel_beyond_its_reach(kid):
    """forced (a child with PM_GEMM_KERNEL=<id>: the packed base call must reach the id, so the probes are live) and unforced"""
    assert _lib_built(), "build the library first (the reach check needs pm_linear_bf16_plan)"
    from pytorch_models._hip import lib

    env = dict(os.environ, PM_GEMM_KERNEL=str(kid))
    r = subprocess.run([sys.executable, os.path.join(HERE, "linear_child.py"), "reach", str(kid)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    forced = json.loads(r.stdout.strip().splitlines()[-1])
    assert forced["base"] == kid, f"PM_GEMM_KERNEL={kid} does not reach kernel {kid} on the probes' packed base call: {forced['base']}"
    free = {name: int(lib().pm_linear_bf16_plan(*LC.plan_args(**g))) for name, (g, _) in LC.reach_probes(kid).items()}
    bad = _reach_violations(kid, forced) + _reach_violations(kid, free)
    assert not bad, "\n".join(bad)


def test_every_reach_bound_that_fits_the_arena_has_a_far_case():
    import wrapper_cases as WC
    after = WC.Arena.bytes_for(32) // 2
    lacking = []
    for kid in (3, 6, 7):
        for name, (g, operand) in LC.reach_probes(kid).items():
            if operand is None or not LC.reach_fits_arena(g, operand, after):
                continue
            form = lambda c: ("win" if c.window else f"residp{c.period}" if c.period else c.far.split(":")[0])  # noqa: E731
            hit = [c for c in LC.FAR_FORCED[kid] if form(c) == name and c.far.split(":")[0] in (name, "residp", "win")
                   and LC.reach(kid, **LC.far_lds(c))[operand] >= LC.LIMIT32]
            if not hit:
                lacking.append((kid, name))
    assert not lacking, f"reach bounds that fit the arena and have no far case crossing them: {lacking}"
    assert {(k, n) for k in (3, 6, 7) for n, (g, o) in LC.reach_probes(k).items() if o and LC.reach_fits_arena(g, o, after)} >= \
        {(3, "x"), (3, "w"), (6, "w"), (7, "w"), (6, "residp2"), (7, "residp3")}
