"""GPU: the aliasing contract on the device (tests/alias_cases.py; the CPU half, which proves what is refused
before a launch, is tests/test_alias_cases_cpu.py).  This file launches only what the CPU audit saw accepted - the ALIAS_OK pairs as
the same view and disjoint column ranges of one parent - and re-checks every refusal: no launch here reads memory that another
workgroup is writing, and none addresses by overwritten integers.

Refusals and ``columns``, per row (ten rows to a test, as tests/test_hip_empty.py groups them): the canonical call, every case of the
row - a refusal is a ValueError naming the wrapper and both operands with nothing recorded in ops.LAUNCH_LOG and the written operands
and the arena unchanged; a ``columns`` case gives the bits of the apart call and leaves the parent alone outside W -, the canonical
call again, bit-identical to the first.

ALIAS_OK pairs: a single-workgroup shape proves nothing, so each pair runs at the smallest shape that gives at least two workgroups
along every grid dimension of the kernel, a ragged last one and two K steps, read off the launchers' tile constants
(linear_cases.tile_rows / tile_cols; mixer_token_mix_plan).  ``linear`` runs once per kernel id the default dispatcher reaches
with a residual (1, 2, 3, 6, 7 - asserted through linear_plan; the persistent kernels start at M = 4096, so those shapes have a few
thousand rows) and at the 70000 x 1032 x 128 problem of tests/test_hip_kernels.py.  Each is compared bit for bit with the same call
on a cloned T, and replayed as a HIP graph (graph_cases.check_replay).  ``pytest -s`` prints one FIGURE line per case."""
import pytest
import torch

import alias_cases as AC
import graph_cases as GC
import linear_cases as LC
import wrapper_cases as WC
from test_alias_cases_cpu import accepted
from test_hip_graph_ops import allocated, capture, replay, warm
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def seen():
    """what the CPU audit accepted (run on the recording stub, in this process, before anything here launches)"""
    return accepted()


def _guard(what, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{what}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise


class _Log:
    """the recorder check_row asks for a launch count: ops.LAUNCH_LOG, which every wrapped launch writes into"""

    def begin(self) -> None:
        ops.LAUNCH_LOG = self.log = {}

    @property
    def launches(self) -> list:
        n = [k for k, v in self.log.items() for _ in v]
        ops.LAUNCH_LOG = None
        return n


def _sandwich(rid: str, seen: set) -> list[str]:
    r = WC.ROWS[rid]

    def canonical():
        kw = r.build(DEV)
        return WC.snapshot(r, kw, WC.call(ops, r, kw))

    first = _guard(rid, canonical)
    try:
        problems, outcomes = _guard(rid, lambda: AC.check_row(ops, r, DEV, compare=True, hook=_Log(), only=seen))
    finally:
        ops.LAUNCH_LOG = None
    again = _guard(rid, canonical)
    for o in outcomes:
        print("FIGURE alias", *[str(x).replace(" ", "_") for x in o])
    want = sum(1 for _ in AC.cases(r, torch.device("cpu")))
    if len({o[:4] for o in outcomes}) != want:
        problems.append(f"{rid}: {len(outcomes)} outcomes, the generator has {want} cases")
    for o in outcomes:
        if o[4] == "copied":
            problems.append(f"{rid}: {o}: a device tensor cannot have been copied")
    bad = WC._diff(again, first)
    if bad:
        problems.append(f"{rid}: the canonical call after the aliasing cases differs from the one in front of them in {bad}")
    return problems


_ROWS = [rid for rid, r in WC.ROWS.items() if r.inplace]
ROW_GROUPS = [_ROWS[i:i + 10] for i in range(0, len(_ROWS), 10)]


@pytest.mark.parametrize("rids", ROW_GROUPS, ids=[f"{g[0]}..{g[-1]}" for g in ROW_GROUPS])
def test_aliasing_cases_between_two_canonical_calls(rids, seen):
    problems = [p for rid in rids for p in _sandwich(rid, seen)]
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


# ------------------------------------------------------------------------------------------------------- the ALIAS_OK pairs
def _honoured(what: str, run, sets, w: str, t: str) -> None:
    """``run(kw)`` with kw[w] the very tensor kw[t] (one buffer, holding T's values) against the same call with T cloned first and W
    a tensor of its own, then as a HIP graph"""
    a, b = sets(0), sets(1)
    ka = GC.clone_kw(a)
    ka[w] = ka[t]
    kc = GC.clone_kw(a)
    kc[w] = torch.full_like(kc[w], float("nan"))
    kc[t] = a[t].clone()
    _guard(what, lambda: (run(ka), run(kc)))
    assert ka[t] is ka[w] and kc[t].data_ptr() != kc[w].data_ptr() and WC.same_bits(kc[t], a[t])
    assert WC.same_bits(ka[w], kc[w]), f"{what}: {w} aliased with {t} differs from the call with {t} cloned first"
    assert not WC.same_bits(ka[w], a[t]), f"{what}: the call changed nothing"
    del ka, kc

    def aliased(kw):  # the static set holds the shared buffer once, under T's name
        kw = dict(kw)
        kw[w] = kw[t]
        return run(kw)

    drop = lambda kw: {k: v for k, v in kw.items() if k != w}  # noqa: E731
    problems = _guard(what, lambda: GC.check_replay(
        aliased, drop(a), drop(b), GC.overwrite_kw, capture=capture, replay=replay, clone=GC.clone_kw,
        snap=lambda kw, res: [(t, kw[t].clone())], inplace=True, warm=warm, allocated=allocated))
    assert not problems, "\n".join([f"{what}: {len(problems)} problems:"] + problems)


# kernel id -> (M, N, K): two tile rows and two tile columns at least, ragged in both, two K steps of 64; ids 2, 3, 6, 7 are served
# from M = 4096 on, the tile kernels (6, 7) need M % 8 == 0 and the dispatcher prefers them there, so the wide kernel (3) takes
# M % 8 != 0.  Read off linear_cases.tile_rows / tile_cols and checked below against them and against linear_plan.
LINEAR_SHAPES = {1: (300, 264, 128), 2: (4616, 1032, 128), 3: (4612, 2056, 128), 6: (4616, 2056, 128), 7: (5384, 3080, 128)}


def _linear_sets(M, N, K):
    def sets(i):
        g = WC.Gen(DEV, WC.SEED + 500 + i)
        return dict(x=g.b(M, K), w=g.b(N, K, scale=0.1), bias=g.f(N), resid=g.b(M, N), out=g.z(M, N, dtype=WC.BF))
    return sets


def _linear(kw):
    return ops.linear(kw["x"], kw["w"], kw["bias"], act="gelu", resid=kw["resid"], out=kw["out"])


def test_linear_shapes_cover_every_kernel_id_linear_cases_reaches():
    assert set(LINEAR_SHAPES) == {1} | set(LC.FORCED_IDS)
    for kid, (M, N, K) in LINEAR_SHAPES.items():
        tr, tc = LC.tile_rows(kid), LC.tile_cols(kid)
        assert M > tr and N > tc and M % tr and N % tc and K >= 128, (kid, M, N, K)


@pytest.mark.parametrize("kid", list(LINEAR_SHAPES))
def test_linear_residual_aliased_with_out_per_kernel(kid, seen):
    assert ("linear", "out", "resid", "same") in seen
    M, N, K = LINEAR_SHAPES[kid]
    sets = _linear_sets(M, N, K)
    kw = sets(0)
    kw["resid"] = kw["out"]
    got = ops.linear_plan(kw["x"], kw["w"], kw["bias"], act="gelu", resid=kw["resid"], out=kw["out"])
    print(f"FIGURE alias linear out resid same kernel {got} M {M} N {N} K {K}")
    assert got == kid, f"linear_plan answers kernel {got} for {M} x {N} x {K}; the shape was chosen for kernel {kid}"
    _honoured(f"linear kernel {kid}", _linear, sets, "out", "resid")


def test_linear_residual_aliased_with_out_at_the_wide_problem(seen):
    """the 70000 x 1032 x 128 problem of test_linear_wide_256x256_kernel, residual in place; whichever kernel the dispatcher gives it"""
    assert ("linear", "out", "resid", "same") in seen
    M, N, K = 70000, 1032, 128
    sets = _linear_sets(M, N, K)
    kw = sets(0)
    got = ops.linear_plan(kw["x"], kw["w"], kw["bias"], act="gelu", resid=kw["out"], out=kw["out"])
    print(f"FIGURE alias linear out resid same kernel {got} M {M} N {N} K {K}")
    assert got in LINEAR_SHAPES, got
    del kw
    _honoured("linear 70000 x 1032 x 128", _linear, sets, "out", "resid")


def test_linear_periodic_residual_aliased_with_out_is_refused():
    M, N, K = LINEAR_SHAPES[1]
    kw = _linear_sets(M, N, K)(0)
    before = kw["out"].clone()
    log: dict = {}
    ops.LAUNCH_LOG = log
    try:
        with pytest.raises(ValueError, match=r"linear: out \(written\) shares memory with resid"):
            ops.linear(kw["x"], kw["w"], kw["bias"], resid=kw["out"], out=kw["out"], resid_period=M)
        with pytest.raises(ValueError, match=r"linear: out \(written\) shares memory with x"):
            ops.linear(kw["out"][:, :K], kw["w"], kw["bias"], out=kw["out"])  # linear(x, w, out=x), x a column range of out
    finally:
        ops.LAUNCH_LOG = None
    assert not log and WC.same_bits(kw["out"], before)


def test_mixer_token_mix_in_place(seen):
    assert ("mixer_token_mix", "out", "x", "same") in seen
    N, T, C, Dt = 2, 50, 256, 64
    plan = ops.mixer_token_mix_plan(T, Dt, C)
    assert "refused" not in plan, plan
    # grid (C / (32 NB), N): two channel slabs and two images at least; T = 50 is a ragged last strip of 32 tokens and a ragged K of
    # the first product (nk1 steps of 16), nk2 steps of the second
    assert C // (32 * plan["NB"]) >= 2 and N >= 2 and plan["nt"] >= 2 and T % 32 and plan["nk1"] >= 2 and plan["nk2"] >= 2, plan

    def sets(i):
        g = WC.Gen(DEV, WC.SEED + 600 + i)
        x = g.b(N, T, C)
        return dict(x=x, stats=ops.row_stats(x.view(N * T, C), WC.EPS), gamma=g.f(C), beta=g.f(C),
                    w1f=ops.mixer_pack_weight(g.b(Dt, T, scale=0.2)), b1=g.f(Dt), w2f=ops.mixer_pack_weight(g.b(T, Dt, scale=0.2)), b2=g.f(T),
                    out=g.z(N, T, C, dtype=WC.BF))

    def run(kw):
        return ops.mixer_token_mix(kw["x"], kw["stats"], kw["gamma"], kw["beta"], kw["w1f"], kw["b1"], kw["w2f"], kw["b2"], out=kw["out"])

    _honoured("mixer_token_mix", run, sets, "out", "x")  # the in-place call: out is x itself
