"""CPU: the empty-batch contract without a GPU (tests/empty_cases.py).

The library is the recording stub of tests/test_wrapper_cases_cpu.py; canonical operands are CPU tensors.  Asserted:
  * completeness: every row has axes; every dimension of every tensor operand of every row's canonical build is zeroed by an axis
    or exempt with a reason; no count axis is exempt; every count axis outside the decode-step family is honoured;
  * every (row, axis): the table's outcome as the contract defines it - for "empty" the stated shapes, the canonical call's dtypes,
    ``out=`` identity, every operand bit-unchanged and no recorded call; for "refuse" a ValueError that names the wrapper, no
    recorded call, nothing modified; no recorded call of any case carries a null pointer where the canonical call carried one;
  * every mutant of MUTANTS is reported, with the words that belong to its defect;
  * the host-only queries (the real library, host arithmetic only) answer what their docstrings say for a zero extent and never
    a negative byte count;
  * MODEL_EMPTY: the fp32 CPU module of every MODELS entry decides the expected outcome of its forward (returns or raises); the
    table may refuse at most 4 forwards the CPU module honours, each with a reason."""
import os
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "pytorch-models_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import empty_cases as EC  # noqa: E402
import graph_cases as GC  # noqa: E402
import wrapper_cases as WC  # noqa: E402
from test_wrapper_cases_cpu import _install  # noqa: E402  (the recording stub, shared)
from pytorch_models._hip import LIB_PATH, ops  # noqa: E402

torch.set_grad_enabled(False)
CPU = torch.device("cpu")


@pytest.fixture
def rec(monkeypatch):
    return _install(monkeypatch)


# ------------------------------------------------------------------------------------------------------------ completeness
def test_every_row_has_axes_and_every_axis_a_class(rec):
    assert set(EC.AXES) == set(WC.ROWS), (set(WC.ROWS) - set(EC.AXES), set(EC.AXES) - set(WC.ROWS))
    for rid, axes in EC.AXES.items():
        assert axes, f"{rid}: no axis"
        names = [a.name for a in axes]
        assert len(names) == len(set(names)), (rid, names)
        assert any(a.kind == "count" for a in axes), f"{rid}: no count axis"
        for a in axes:
            assert a.kind in EC.KINDS and a.outcome in ("empty", "refuse"), (rid, a.name)
            assert a.dims or a.ints or a.seq is not None, f"{rid} {a.name}: an axis that zeroes nothing"
            family = WC.ROWS[rid].fn in EC.DECODE_FAMILY
            if a.kind == "count" and a.outcome == "refuse":
                assert family and a.why, f"{rid} {a.name}: a count axis outside the decode-step family must be honoured"
            if a.kind == "inner":
                assert a.outcome == "refuse", f"{rid} {a.name}: inner extents are refused"


def test_every_operand_dimension_is_zeroed_or_exempt(rec):
    missing = {rid: EC.missing_dims(rid, r.build(CPU)) for rid, r in WC.ROWS.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, f"operand dimensions that no axis of tests/empty_cases.py zeroes: {missing}"
    for (rid, operand, d), why in EC.EXEMPT_DIMS.items():
        assert rid in WC.ROWS and why, (rid, operand, d)
        kw = WC.ROWS[rid].build(CPU)
        t = {WC.path_name(p): t for p, t in WC.operands(kw)}[operand]
        assert d < t.dim(), "stale exemption"
        counted = [a.name for a in EC.AXES[rid] if a.kind == "count" and any(WC.path_name(p) == operand and dd == d for p, dd in a.dims)]
        assert not counted, f"{rid} {operand}:{d} is exempt and a count axis {counted}"
    # an exempt dimension is never the only carrier of a count: every count axis zeroes something that is not exempt
    for rid, axes in EC.AXES.items():
        for a in axes:
            if a.kind == "count":
                assert not any((rid, WC.path_name(p), d) in EC.EXEMPT_DIMS for p, d in a.dims), (rid, a.name)


def test_shrink_zeroes_what_the_axis_names(rec):
    for rid, r in WC.ROWS.items():
        for a in EC.AXES[rid]:
            kw0, kw = r.build(CPU), a.shrink(r.build(CPU))
            for path, t in WC.operands(kw0):
                want = [0 if (path, d) in a.dims else n for d, n in enumerate(t.shape)]
                got = WC.get(kw, path)
                assert list(got.shape) == want and got.dtype == t.dtype, (rid, a.name, path)
                if 0 in want:
                    assert got.data_ptr() == 0, "an empty tensor's pointer is null: the premise of the contract"
            for k, v in a.ints.items():
                assert k in kw0 and kw[k] == v == 0, (rid, a.name, k)


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("rid", list(WC.ROWS))
def test_empty_cases_are_honoured_or_refused_without_a_call(rid, rec):
    problems, cases = EC.check_row(ops, WC.ROWS[rid], CPU, rec)
    assert len(cases) == len(EC.AXES[rid])
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


@pytest.mark.parametrize("name", list(EC.MUTANTS))
def test_every_mutant_is_caught(name, rec):
    rid, broken = EC.mutant_ops(ops, name)
    clean, _ = EC.check_row(ops, WC.ROWS[rid], CPU, rec)
    assert not clean, clean
    problems, _ = EC.check_row(broken, WC.ROWS[rid], CPU, rec, canon_ops=ops)
    words = EC.MUTANTS[name][3]
    assert any(words in p for p in problems), f"mutant '{name}' was not reported with '{words}': {problems}"


# ---------------------------------------------------------------------------------------------------------- host-only queries
def test_host_only_queries_on_a_zero_extent():
    assert os.path.exists(LIB_PATH), "build the library first (the host-only queries are asked of the real one)"
    bf = torch.bfloat16
    x, w = torch.empty((0, 128), dtype=bf), torch.zeros((64, 128), dtype=bf)
    assert ops.linear_plan(x, w) == 0, "linear_plan documents 0 for M == 0"
    assert ops.linear_plan(torch.zeros((16, 128), dtype=bf), w) in range(1, 8)
    for bad in ((torch.zeros((16, 0), dtype=bf), torch.zeros((64, 0), dtype=bf)), (torch.zeros((16, 128), dtype=bf), torch.zeros((0, 128), dtype=bf))):
        with pytest.raises(ValueError, match="linear_plan"):
            ops.linear_plan(*bad)
    xs = torch.zeros((2, 10, 64), dtype=bf)
    geom = dict(K=128, row_stride=128, rows_per_batch=4, batch_stride=640, w=torch.zeros((32, 128), dtype=bf))
    assert ops.linear_strided_plan(xs[:0], M=0, **geom) == 0 and ops.linear_strided_plan(xs, M=8, **geom) in range(1, 8)
    # byte counts: 0 or more, and no more than the smallest non-empty problem needs
    assert 0 <= ops.lm_score_ws_bytes(0, 11) <= ops.lm_score_ws_bytes(1, 11)
    assert 0 <= ops.align_ws_bytes(0, 5, 12) <= ops.align_ws_bytes(1, 5, 12)
    assert 0 <= ops.ctc_ws_bytes(0, 0, 3) <= ops.ctc_ws_bytes(1, 1, 3)
    L = ops.lib()
    assert 0 <= L.pm_lstm_workspace_floats(0, 3, 64) <= L.pm_lstm_workspace_floats(1, 3, 64)
    assert 0 <= L.pm_groupnorm1_workspace_doubles(0, 40) <= L.pm_groupnorm1_workspace_doubles(1, 40)
    assert 0 <= L.pm_w2v_stem0_scratch_floats(0, 17) <= L.pm_w2v_stem0_scratch_floats(1, 17)
    assert L.pm_linear_ws_bytes() >= 0
    # *_supported: a shape with a zero extent is not a served shape
    assert not ops.mixer_token_mix_supported(0, 32, 64) and not ops.mixer_token_mix_supported(12, 0, 64) and not ops.mixer_token_mix_supported(12, 32, 0)
    assert not ops.conv1d_supported(0, 4, 8, 3, 1, 1, 1)
    assert not ops.cls_attend_supported(0, 64, 3) and not ops.cls_attend_supported(5, 0, 3)
    assert not ops.grouped_conv_supported(0, 8)
    assert not ops.linear_ln_supported(0, 64, 128, "none", False)
    # the plan queries refuse a zero extent with a code, as their docstrings say ({"refused": code})
    for kw in (dict(M=0, N=48, K=64), dict(M=3, N=0, K=64), dict(M=3, N=48, K=0)):
        assert ops.dec_linear_plan(**kw).get("refused"), kw
    for T, Dt, C in ((0, 32, 64), (12, 0, 64), (12, 32, 0)):
        assert ops.mixer_token_mix_plan(T, Dt, C).get("refused"), (T, Dt, C)


# ------------------------------------------------------------------------------------------------------------------ the models
def test_model_table_covers_every_entry_point_and_agrees_with_the_cpu_modules():
    assert set(GC.MODELS) <= set(EC.MODEL_EMPTY)
    # every entry point of NOT_GRAPHED that takes a batch (the tokenizer loop and the host pipeline take strings and images)
    for name in GC.NOT_GRAPHED:
        if name.split(".")[-1] in ("generate", "score", "align", "encode", "embed") and name.split(".")[0] not in ("DecoderGenerator", "audio2text"):
            assert name in EC.MODEL_EMPTY, name
        if name.endswith("forward(lengths)"):
            k = name.split(".")[0]
            assert f"{k}.forward(lengths=[])" in EC.MODEL_EMPTY and f"{k}.forward(lengths=0s)" in EC.MODEL_EMPTY, name
    assert set(EC.MODEL_REFUSALS) <= set(GC.MODELS) and len(EC.MODEL_REFUSALS) <= 4 and all(EC.MODEL_REFUSALS.values()), EC.MODEL_REFUSALS
    design = open(os.path.join(os.path.dirname(_HERE), "DESIGN.md")).read()
    for key, e in EC.MODEL_EMPTY.items():
        assert e.model in GC.MODELS and e.outcome in (None, "empty", "refuse"), key
        assert e.outcome != "refuse" or e.why, f"{key}: a refusal needs its reason"
        if key not in GC.MODELS:
            assert e.outcome is not None, f"{key}: an entry point outside MODELS states its outcome"
            continue
        kind, what = EC.cpu_outcome(key)  # the reference's verdict
        if kind == "none":
            assert e.outcome is not None and e.why and key not in EC.MODEL_REFUSALS, f"{key}: no CPU form, so the table states the outcome and why"
        elif key in EC.MODEL_REFUSALS:
            assert kind == "empty" and e.outcome is None, f"{key}: listed as refused against the CPU module, which {kind}s"
            assert f"`{key}`" in design, f"{key}: a forward refused against the CPU module needs its reason in DESIGN.md too"
        else:
            assert e.outcome is None, f"{key}: the CPU module decides ({kind}); the table may not state another outcome"
            assert EC.expected_model_outcome(key)[0] == kind
        if kind == "empty":
            assert what and all(shape[0] == 0 for shape, _ in what), (key, what)
