"""GPU: the launch plan of every decoder form (tools/decode_plan.py: CASES) points only into memory the decoder keeps alive.

A plan holds raw pointers and is captured into a graph, so a tensor it points into must live as long as the decoder: as an
attribute, in a list or tuple of one, or in ``_keep`` (pytorch_models/_hip/decode_plan.py).  A pointer that resolves only into
the MODEL's tensors is a defect too - the decoder must not depend on its caller keeping the model (or a derived copy of a
weight, which the model rebuilds and frees when the parameter changes) alive.  Nothing is launched: the plans are built on tiny
synthetic models (1-2 layers, vocabulary 300, memory 24, prompt 2, 3 new tokens) and read."""
import importlib.util
import os

import pytest
import torch

from pytorch_models import _hip

_spec = importlib.util.spec_from_file_location(
    "decode_plan_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "decode_plan.py"))
DP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DP)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TICKETS = {"pm_dec_linear_ksplit": 15, "pm_dec_layers": 17}  # the argument that is a K-split ticket array


@pytest.mark.parametrize("case", list(DP.CASES))
def test_every_pointer_of_the_plan_resolves_into_a_kept_tensor(case, monkeypatch):
    if DP.needs_experiments(case) and not _hip.has_experiments():
        pytest.skip("experiments build only (make experiments; PM_MI355X_LIB)")
    dec, model = DP.CASES[case](monkeypatch.setenv)
    lines, dangling = DP.plan(dec, model)
    assert not dangling, f"kept alive by the model only: {dangling}"
    assert len([ln for ln in lines if not ln.startswith(" ")]) == len(dec.launches) > 0
    # every ticket array a launch counts on is one reset() zeroes
    zeroed = {c.data_ptr() for c in dec._ks_cnts}
    for fn, args in dec.launches:
        if fn.__name__ in TICKETS:
            assert args[TICKETS[fn.__name__]] in zeroed, fn.__name__
