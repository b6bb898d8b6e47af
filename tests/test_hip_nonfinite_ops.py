"""GPU: the non-finite operand contract on the kernels (tests/nonfinite_cases.py; the CPU half, which
proves that the protocol reports each planted defect and that the tables are complete, is tests/test_nonfinite_cases_cpu.py).

One test per (row of UNITS, poison): the canonical call of tests/wrapper_cases.py runs clean, then once per per-sample float
operand with ONE element of a middle sample set to NaN, +inf, -inf or the largest finite value.  Every other sample keeps its
bits, every integer result stays inside its declared range, and under NaN the sample shows a non-finite float unless the row is
listed in SWALLOWS.  One test per row of IGNORED, and one per row of PAD_COLUMNS (operands re-laid into a NaN parent with a
leading dimension): NaN in the regions the documented contract says are not read changes no bit.
One test per (decision, family, size): a row of NaN, of -inf, with one NaN, with two +inf or of equal values among Gaussian
rows - the decision is torch's where the row has no NaN, a valid index where it has one, the float companions are non-finite
there, and the other rows keep their bits.  All failing operands of a row are reported together."""
import pytest
import torch

import nonfinite_cases as NF
import wrapper_cases as WC
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)


def _guard(what: str, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{what}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise


@pytest.mark.parametrize("poison", NF.POISONS)
@pytest.mark.parametrize("rid", list(NF.UNITS))
def test_one_poisoned_sample_stays_alone_and_is_seen(rid, poison):
    r = WC.ROWS[rid]
    problems = _guard(f"{rid} {poison}", lambda: NF.check_isolation(NF.row_run(ops, r), r.build(DEV), NF.UNITS[rid], poison,
                                                                     swallows=NF.swallowed(rid)))
    print(f"{rid} {poison}: {len(NF.UNITS[rid].operands)} operands, {len(problems)} problems")
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


@pytest.mark.parametrize("rid", list(NF.IGNORED))
def test_nan_in_an_ignored_region_changes_no_bit(rid):
    r = WC.ROWS[rid]
    problems = _guard(rid, lambda: NF.check_ignored(NF.row_run(ops, r), r.build(DEV), NF.IGNORED[rid]))
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


@pytest.mark.parametrize("rid", list(NF.PAD_COLUMNS))
def test_nan_in_the_pad_columns_of_a_leading_dimension_changes_no_bit(rid):
    r = WC.ROWS[rid]
    problems = _guard(rid, lambda: NF.check_pad_columns(NF.row_run(ops, r), r.build(DEV), NF.PAD_COLUMNS[rid]))
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


DECIDE = [(d.id, f, V) for d in NF.DECISIONS.values() for V in d.sizes for f in d.families]


@pytest.mark.parametrize("did,family,V", DECIDE, ids=[f"{d}-{f}-{V}" for d, f, V in DECIDE])
def test_decision_on_a_row_that_is_not_finite(did, family, V):
    problems = _guard(f"{did} {family} {V}", lambda: NF.check_decision(NF.DECISIONS[did], DEV, family, V))
    assert not problems, "\n".join([f"{did} {family} V={V}: {len(problems)} problems:"] + problems)
