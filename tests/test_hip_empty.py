"""GPU: the empty-batch contract on the device (tests/empty_cases.py; the CPU half, which proves that no
empty case reaches the library, is tests/test_empty_cases_cpu.py).  Nothing here launches with a zero extent: the only launches
are the canonical, already-tested shapes of wrapper_cases.ROWS and graph_cases.MODELS.

Per row: the canonical call, every empty case of the row (the table's outcome, results on the operands' device, ``out=`` identity,
every operand bit-unchanged, a clean synchronize), the canonical call again - bit-identical to the first, so workspaces, tickets
and caches are undisturbed.  The rows that own per-stream state repeat that on a side stream.  Per MODEL_EMPTY entry, on a warm
module: the empty call with ops.LAUNCH_LOG switched on (it must record nothing), then the canonical input again, bit-identical
to the first run.  ``pytest -s`` prints one FIGURE line per case.

The rows run ten to a test and every model class is one test (its dtypes and its further entry points inside it): the cases are
many and small, and each test reports all the problems of its group together."""
import pytest
import torch

import empty_cases as EC
import graph_cases as GC
import wrapper_cases as WC
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)
PER_STREAM = ("linear:ln_fold", "dec_linear_ksplit")  # the stream-K workspace of (device, stream); the K-split tickets


def _guard(what, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{what}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise


def _sandwich(rid: str) -> list[str]:
    """the problems of one row: its empty cases between two canonical calls"""
    r = WC.ROWS[rid]

    def canonical():
        kw = r.build(DEV)
        return WC.snapshot(r, kw, WC.call(ops, r, kw))

    first = _guard(rid, canonical)
    problems, cases = _guard(rid, lambda: EC.check_row(ops, r, DEV))
    again = _guard(rid, canonical)
    for row, axis, outcome in cases:
        print(f"FIGURE empty {row} {axis.replace(' ', '_')} {outcome}")
    if len(cases) != len(EC.AXES[rid]):
        problems.append(f"{rid}: {len(cases)} cases ran, the table has {len(EC.AXES[rid])}")
    bad = WC._diff(again, first)
    if bad:
        problems.append(f"{rid}: the canonical call after the empty cases differs from the one in front of them in {bad}")
    return problems


_ROWS = list(WC.ROWS)
ROW_GROUPS = [_ROWS[i:i + 10] for i in range(0, len(_ROWS), 10)]


@pytest.mark.parametrize("rids", ROW_GROUPS, ids=[f"{g[0]}..{g[-1]}" for g in ROW_GROUPS])
def test_empty_cases_between_two_canonical_calls(rids):
    problems = [p for rid in rids for p in _sandwich(rid)]
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


def test_empty_cases_on_a_side_stream():
    assert set(PER_STREAM) <= set(WC.ROWS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        problems = [p for rid in PER_STREAM for p in _sandwich(rid)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


# ------------------------------------------------------------------------------------------------------------------ the models
def _entry(key: str, dtype: str, mod, inputs, run, first) -> None:
    """one entry of MODEL_EMPTY on the warm module ``mod``; asserts"""
    e = EC.MODEL_EMPTY[key]
    case = GC.MODELS[e.model]
    want, shapes = EC.expected_model_outcome(key)
    log: dict = {}
    ops.LAUNCH_LOG = log
    try:
        res, exc = _guard(key, lambda: e.call(mod, inputs)), None
    except Exception as err:  # noqa: BLE001 - classified below
        res, exc = None, err
    finally:
        ops.LAUNCH_LOG = None
    print(f"FIGURE empty {key}-{dtype} batch {want}")
    assert not log, f"{key}: the empty call launched {sorted(log)}"
    if want == "refuse":
        assert exc is not None, f"{key}: accepted; the table says refuse"
        # a clean refusal names the model and the empty batch; a zero length is refused by seq_lens' bound, which names the lengths
        words = ("lengths",) if key.endswith("0s)") else (case.cls.split(".")[0], "empty")
        assert type(exc) is ValueError and all(w in str(exc) for w in words), f"{key}: not a clean refusal: {type(exc).__name__}: {exc}"
    else:
        assert exc is None, f"{key}: raised {type(exc).__name__}: {exc}; expected an empty result"
        got = [(tuple(t.shape), t.dtype, t.device.type) for _, t in GC.flat(res)]
        if shapes is not None:
            assert [g[0] for g in got] == [s for s, _ in shapes], (key, got, shapes)
        assert got and all(0 in g[0] or key.endswith("0s)") for g in got) and all(g[2] == "cuda" for g in got), (key, got)
        if key in GC.MODELS:
            assert [g[1] for g in got] == [t.dtype for t in first], (key, got)
    again = _guard(key, lambda: [t for _, t in GC.flat(run())])
    assert len(again) == len(first) and all(WC.same_bits(a, b) for a, b in zip(again, first)), f"{key}: the canonical input gives other bits after the empty call"


def test_every_model_entry_belongs_to_a_model_test():
    assert {e.model for e in EC.MODEL_EMPTY.values()} == set(GC.MODELS)


@pytest.mark.parametrize("model", list(GC.MODELS))
def test_model_entry_points_on_an_empty_batch(model):
    case = GC.MODELS[model]
    problems, n = [], 0
    for dtype in case.dtypes:
        mod, inputs = EC.hip_module(model, dtype)
        run = (lambda: getattr(mod, case.method)(*inputs)) if case.method else (lambda: mod(*inputs))
        first = _guard(model, lambda: [t.clone() for _, t in GC.flat(run())])
        # the forward on every dtype of the family; the further entry points (generate, score, align, lengths= ...) on the first
        for key, e in EC.MODEL_EMPTY.items():
            if e.model != model or (key != model and dtype != case.dtypes[0]):
                continue
            n += 1
            try:
                _entry(key, dtype, mod, inputs, run, first)
            except AssertionError as err:
                problems.append(f"{key}-{dtype}: {err}")
    assert n >= len(case.dtypes)
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)
