"""GPU: every model forward replays as one HIP graph, bit for bit, through pytorch_models.graph.GraphedForward - the class users
are told to use (tests/graph_cases.py: MODELS / NOT_GRAPHED).

Every model is built at the smallest geometry its family's tests build, batch 2, in bf16 and - where the family has one - on
its fp32 path; batch x tokens stays far below the two-stream threshold, so every graph is a linear chain (the fork / join
capture keeps its own test in tests/test_hip_vit.py).  The protocol is graph_cases.check_replay with GraphedForward as capture
and replay: g(x_a) == m(x_a), g(x_b) == m(x_b), g(x_b) again.  Then the ordinary serving pattern (failure class 5): the SAME
module runs eagerly at another batch and another sequence length or image size, and a second instance of the class runs at a
third geometry; the next g(x_b) must still be m(x_b) as computed before, from the same graph object - a shape change is no
weight update, so nothing is recaptured.  Three more replays leave the memory in use unchanged.  The forwards that also take
device lengths must raise the capture guard instead of dying inside the HIP runtime."""
import pytest
import torch
from torch import nn

import coherence_cases as CC
import graph_cases as GC
import wrapper_cases as WC
from pytorch_models.graph import GraphedForward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)
SEED_A, SEED_B, SEED_OTHER = 311, 312, 313
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


class Method(nn.Module):
    """an entry point other than forward as a module GraphedForward can call; the model is a child: its parameters are watched"""

    def __init__(self, model: nn.Module, method: str) -> None:
        super().__init__()
        self.model, self.method = model, method

    def forward(self, *inputs):
        return getattr(self.model, self.method)(*inputs)


def build(case: GC.Model, dtype: str, k: int, seed: int) -> nn.Module:
    m = CC.filled(case.make(k), seed)
    m = (m.to(torch.bfloat16) if dtype == "bf16" else m).to(DEV)
    return Method(m, case.method) if case.method else m


def inputs(case: GC.Model, dtype: str, k: int, seed: int) -> list:
    return [(x.to(DTYPES[dtype]) if i in case.cast else x).to(DEV) for i, x in enumerate(case.inputs(k, seed))]


CASES = [(key, dtype) for key, case in GC.MODELS.items() for dtype in case.dtypes]


@pytest.mark.parametrize("key,dtype", CASES, ids=[f"{k}-{d}" for k, d in CASES])
def test_model_forward_replays_bit_for_bit(key, dtype):
    case = GC.MODELS[key]
    m, other = build(case, dtype, 0, SEED_A), build(case, dtype, 2, SEED_OTHER)
    x_a, x_b = inputs(case, dtype, 0, SEED_A), inputs(case, dtype, 0, SEED_B)
    x_1, x_2 = inputs(case, dtype, 1, SEED_OTHER), inputs(case, dtype, 2, SEED_OTHER)
    assert x_a[0].shape[0] == 2 and x_1[0].shape[0] != 2 and x_1[0].shape != x_2[0].shape
    graphs = []

    def capture(run, static) -> GC.Handle:
        g = GraphedForward(m, *static, warmup=case.warmup)
        graphs.append(g.graph)
        return GC.Handle(g, g.output, static)

    def replay(h: GC.Handle) -> None:
        h.result = h.graph(*h.static)  # the inputs are copied into the captured buffers, the signature is compared, one graph launch
        graphs.append(h.graph.graph)

    def serve_other_shapes() -> None:
        first = [t.clone() for _, t in GC.flat(m(*x_1))]  # the same module, eagerly, at another geometry
        second = [t.clone() for _, t in GC.flat(other(*x_2))]  # a second instance at a third
        again = [t for _, t in GC.flat(m(*x_1))]
        assert first and second and all(torch.equal(p, q) for p, q in zip(first, again))

    def allocated() -> int:
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    try:
        problems = GC.check_replay(lambda xs: m(*xs), x_a, x_b, lambda st, src: [d.copy_(s) for d, s in zip(st, src)],
                                   capture=capture, replay=replay, clone=lambda xs: [x.clone() for x in xs],
                                   snap=lambda xs, res: [(n, t.clone()) for n, t in GC.flat(res)], allocated=allocated,
                                   hook=serve_other_shapes)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        if WC.is_fault(e):
            pytest.exit(f"{key}-{dtype}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    assert not problems, "\n".join([f"{key} {dtype}: {len(problems)} problems:"] + problems)
    assert all(g is graphs[0] for g in graphs), "a shape change is not a weight update: nothing may be recaptured"


WITH_LENGTHS = [key for key, case in GC.MODELS.items() if case.lengths is not None]


@pytest.mark.parametrize("key", WITH_LENGTHS)
def test_forward_with_device_lengths_raises_the_guard(key):
    case = GC.MODELS[key]
    assert f"{case.cls}.forward(lengths)" in GC.NOT_GRAPHED
    m = build(case, "bf16", 0, SEED_A)
    xs = inputs(case, "bf16", 0, SEED_A) + [case.lengths(0).to(DEV)]
    want = [t.clone() for _, t in GC.flat(m(*xs))]  # the eager call serves device lengths
    try:
        with pytest.raises(RuntimeError, match=r"(?s)seq_lens.*capture") as info:
            GraphedForward(m, *xs)
    except Exception as e:  # noqa: BLE001
        if WC.is_fault(e):
            pytest.exit(f"{key}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    assert not WC.is_fault(info.value)
    assert all(torch.equal(p, q) for p, (_, q) in zip(want, GC.flat(m(*xs))))  # the refused capture left the module usable
