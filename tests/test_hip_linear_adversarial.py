"""Adversarial fp64 parity of the GEMM and LayerNorm-fold kernels, through pytorch_models._hip.ops: linear on every dispatch target
that ships (ids 1, 2, 3, 6, 7), linear_strided, the fold's consumer and producer, ln_stats_finalize, linear_f32, layernorm, row_stats.
References, bounds, input families and case lists live in tests/linear_cases.py (its docstring maps every kernel path to the cases
that reach it); tests/test_linear_cases_cpu.py proves on the CPU that a correct kernel satisfies every assertion made here, that each
defect in linear_cases.MUTANTS does not, and that pm_linear_bf16_plan sends every case to the kernel it is listed under.

Per case (linear_cases.judge): shape and dtype; the exact family EQUALS want.to(out dtype), row partials included; every other family
stays within 1.5 x the derived bound (linear_cases.MARGIN; no measured number enters an assertion); every sentinel of the y buffer -
the rows before and after, the columns N .. ldy - unchanged; poison: finite and bit-identical on operands cut out of NaN-filled
buffers; perm: y[p] bit for bit on permuted rows; actsweep: every row equal to row 0, and the bf16 GELU rows of ids 2, 3, 6, 7 equal
to id 1's bit for bit.  Each case prints "FIGURE <op><id> <family> <case id> ratio <max |err| / bound>" (pytest -s).

Default-dispatch cases run in this process.  PM_GEMM_KERNEL is read once per process, so the forced ids run in one child each
(tests/linear_child.py, started with sys.executable under a time limit; it asserts ops.linear_plan == id on every placement - plain, poisoned, permuted - before it runs and writes
one JSON record per case).  A child that times out, dies on a signal or exits with an error ends the forced part: no further child
is started and the remaining forced tests fail, naming it; a HIP error in this process ends the rest of the file the same way.

Measured on an MI355X (worst max |err| / bound per kernel; the exact family is bit-equal everywhere): see DESIGN.md, "2d. GEMM and
LayerNorm-fold numerics contract".
    op                 output  cancel  offset  poison  perm    actsweep
    linear id 1        bf16    0.334   -       0.997   0.991   1.000
    linear id 1        f32     0.002   -       0.004   0.012   0.863
    linear id 2        bf16    0.526   0.995   0.999   0.998   1.000
    linear id 2        f32     0.002   -       0.013   -       0.863
    linear id 3        bf16    0.543   0.991   0.998   0.996   0.957
    linear id 6        bf16    0.543   0.995   0.999   0.998   0.957
    linear id 7        bf16    0.553   0.995   0.999   0.998   0.957
    linear_f32         f32     0.056   -       0.126   0.132   -
    ln_stats_finalize  f32     -       0.237   -       -       -
    layernorm          bf16    -       0.784   0.998   -       -
    layernorm          f32     -       0.005   0.089   -       -
    row_stats          f32     -       0.020   0.001   -       -
With a bf16 output the half-ulp store term dominates the bound and a correct store reaches it; the f32 rows show the arithmetic
alone.  174 tests, 16 s (12 s of it the four child processes).  The assertions do not depend on these numbers.

Far operands (linear_cases, "far operands"): 58 more tests, 13 s (10 s of it four more children).  Exact-family
operands with one operand a view into a poisoned 16 GiB arena, its last row - last batch of the window form, last row of a periodic
residual - just past 2^31 / 2^32 bytes, and 2^33 where kernel id 3's reach lies.  Refused (nothing written), or equal to want bit for
bit with sentinels and arena intact, whichever kernel the dispatcher chose: `planned` is recorded, not asserted.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import linear_cases as LC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240  # seconds: a child takes ~20 s, most of it the float64 references on the CPU
FAULT: list[str] = []  # the first HIP error seen in this process: after it nothing more of this file touches the GPU


def _on_gpu(what: str, fn):
    assert not FAULT, f"not run: {FAULT[0]}"
    try:
        return fn()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory" in str(e):
            FAULT.append(f"{what} raised a HIP error: {str(e)[:200]}")
        raise


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from pytorch_models._hip import ops as o

    return o


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    """kernel id -> {case id: record} from one child process per forced id, or a string that says why there are none."""
    out = {}
    broken = None
    for kid in LC.FORCED_IDS:
        broken = broken or (FAULT[0] if FAULT else None)
        if broken:
            out[kid] = f"not started: {broken}"
            continue
        path = str(tmp_path_factory.mktemp("linear") / f"id{kid}.jsonl")
        env = dict(os.environ, PM_GEMM_KERNEL=str(kid))
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "linear_child.py"), "run", str(kid), path], env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            rc, log = r.returncode, r.stdout + r.stderr[-3000:]
        except subprocess.TimeoutExpired as e:
            rc, log = None, f"{e.stdout or ''}"
        print(log)
        recs = {}
        if os.path.exists(path):
            recs = {d["id"]: d for d in map(json.loads, open(path).read().splitlines())}
        if rc is None or rc < 0:  # a hang or a fault: nothing more of this file touches the GPU (FAULT)
            broken = f"the child of kernel id {kid} " + ("timed out" if rc is None else f"died on signal {-rc}") + f" after {len(recs)} cases"
            out[kid] = recs or broken
            out[f"broken{kid}"] = broken
            FAULT.append(broken)
        elif rc != 0:  # an exception in the child - a HIP error included: nothing more is started on the GPU either
            broken = f"the child of kernel id {kid} exited with {rc} after {len(recs)} cases: {log[-1500:]}"
            out[kid] = recs
            out[f"broken{kid}"] = broken
            FAULT.append(broken)
        else:
            out[kid] = recs
    return out


@pytest.mark.parametrize("case", LC.DEFAULT_CASES, ids=lambda c: c.id)
def test_default_dispatch(ops, case):
    inp = LC.build(case)
    if case.op == "linear":
        assert LC.plan(ops, case, LC.place(case, inp, "cuda")) == case.kid, f"{case.id}: the default dispatcher does not pick kernel {case.kid}"
    rec = _on_gpu(case.id, lambda: LC.judge(case, inp, LC.reference(case, inp), lambda c, P: LC.run(ops, c, P), dev="cuda"))
    print(LC.figure(rec))
    assert rec["ok"], LC.explain(rec)


@pytest.mark.parametrize("case", [c for k in LC.FORCED_IDS for c in LC.FORCED_CASES[k]], ids=lambda c: c.id)
def test_forced_kernel(forced, case):
    recs = forced[case.kid]
    assert not isinstance(recs, str), recs
    rec = recs.get(case.id)
    assert rec is not None, forced.get(f"broken{case.kid}", f"{case.id}: the child of kernel id {case.kid} left no record")
    print(LC.figure(rec))
    assert rec["planned"] == case.kid, f"{case.id}: PM_GEMM_KERNEL={case.kid} reached kernel {rec['planned']}"
    assert rec["ok"], LC.explain(rec)


# ---------------------------------------------------------------------------------------------------------------- far operands
# linear_cases, "far operands": exact-family operands, one of them a view into a poisoned arena with its last row (batch, period
# row) just past 2^31 / 2^32 bytes - 2^33 where kernel id 3's reach lies.  Refused, or bit-equal to want whichever kernel ran.
@pytest.fixture(scope="module")
def far_arena(forced):  # behind the forced children: one 16 GiB allocation at a time
    import wrapper_cases as WC

    assert not FAULT, f"not run: {FAULT[0]}"
    need = WC.Arena.bytes_for(32)
    free, _ = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"far operands need an arena of {need} bytes plus 2 GiB: {free} bytes of device memory are free")
    a = WC.Arena(need, "cuda")
    yield a
    del a.words
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", LC.FAR_DEFAULT, ids=lambda c: c.id)
def test_far_default_dispatch(ops, far_arena, case):
    inp = LC.build(case)
    rec = _on_gpu(case.id, lambda: LC.judge_far(case, inp, LC.reference(case, inp), ops, far_arena))
    print(LC.figure(rec), "planned", rec.get("planned"), "refused" if rec.get("refused") else "ran")
    assert rec["ok"], LC.explain(rec)


@pytest.fixture(scope="module")
def far_forced(tmp_path_factory, forced, far_arena):
    """as `forced`, for the far cases: one child per kernel id, each with an arena of its own"""
    out = {}
    for kid in LC.FORCED_IDS:
        if FAULT:
            out[kid] = f"not started: {FAULT[0]}"
            continue
        path = str(tmp_path_factory.mktemp("linear_far") / f"id{kid}.jsonl")
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "linear_child.py"), "far", str(kid), path],
                               env=dict(os.environ, PM_GEMM_KERNEL=str(kid)), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            rc, log = r.returncode, r.stdout + r.stderr[-3000:]
        except subprocess.TimeoutExpired as e:
            rc, log = None, f"{e.stdout or ''}"
        print(log)
        out[kid] = {d["id"]: d for d in map(json.loads, open(path).read().splitlines())} if os.path.exists(path) else {}
        if rc != 0:  # a hang, a signal or an exception - a HIP error included: nothing more of this file touches the GPU
            out[f"broken{kid}"] = f"the far child of kernel id {kid} " + ("timed out" if rc is None else f"ended with {rc}") + \
                f" after {len(out[kid])} cases: {log[-1500:]}"
            FAULT.append(out[f"broken{kid}"])
    return out


@pytest.mark.parametrize("case", [c for k in LC.FORCED_IDS for c in LC.FAR_FORCED[k]], ids=lambda c: c.id)
def test_far_forced_kernel(far_forced, case):
    recs = far_forced[case.kid]
    assert not isinstance(recs, str), recs
    rec = recs.get(case.id)
    assert rec is not None, far_forced.get(f"broken{case.kid}", f"{case.id}: the far child of kernel id {case.kid} left no record")
    print(LC.figure(rec), "planned", rec.get("planned"), "refused" if rec.get("refused") else "ran")
    assert rec["ok"], LC.explain(rec)


@pytest.fixture(scope="module")
def id1_gelu_bits(ops, forced):
    """The bf16 GELU sweep on kernel id 1, once; `forced` goes first, so a child that hung or faulted leaves this unlaunched."""
    c1 = next(c for c in LC.DEFAULT_CASES if c.family == "actsweep" and c.kid == 1 and c.act == "gelu" and c.ydt == "bf16")
    inp = LC.build(c1)
    return _on_gpu(c1.id, lambda: LC.judge(c1, inp, LC.reference(c1, inp), lambda c, P: LC.run(ops, c, P), dev="cuda"))["gelu_bits"]


@pytest.mark.parametrize("kid", LC.FORCED_IDS)
def test_gelu_sweep_bits_equal_id1(forced, id1_gelu_bits, kid):
    """gelu_poly2 (the 256-wide kernels' packed form) against gelu_poly (ids 1 and 2) on the whole sweep, bit for bit."""
    recs = forced[kid]
    assert not isinstance(recs, str), recs
    ck = next(c for c in LC.FORCED_CASES[kid] if c.family == "actsweep" and c.act == "gelu" and c.ydt == "bf16")
    assert ck.id in recs, forced.get(f"broken{kid}", f"{ck.id}: no record")
    one, got = id1_gelu_bits, recs[ck.id]["gelu_bits"]
    sw = LC.sweep()
    diff = [float(sw[i]) for i in range(len(one)) if one[i] != got[i]]
    assert not diff, f"kernel id {kid}: GELU differs from id 1 at pre-activations {diff[:8]} ({len(diff)} of {len(one)})"
