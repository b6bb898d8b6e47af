"""GPU: every op wrapper replays as one HIP graph, bit for bit (tests/graph_cases.py; the CPU half, which
plants each defect in a toy op and checks the tables, is tests/test_graph_cases_cpu.py).

One test per captured row of wrapper_cases.ROWS at the row's canonical shape.  The call runs eagerly on two operand sets (the
wanted bits, which must differ in every result), is warmed up on a side stream and captured with torch.cuda.graph on static
operands, and is replayed: on the captured data, on the second set written over the static operands with ``copy_`` (in-place
operands restored to their pre-call content), again on the same data, three more times with the memory in use unchanged, and on
the first set once more.  Every comparison is of bits.  A wrapper that needs the host (HOST_BOUND) must say so instead: under
capture it raises the RuntimeError of ops.no_capture - tested with the capture flag forced on, so that a missing guard fails
the test by running eagerly, not by making an illegal call inside a real capture."""
import re

import pytest
import torch

import graph_cases as GC
import wrapper_cases as WC
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)


def warm(fn) -> None:
    """as GraphedForward._capture: twice on a side stream, so that everything lazy happens in front of the capture"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(side)


def capture(run, static) -> GC.Handle:
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = run(static)
    return GC.Handle(graph, result)


def replay(handle: GC.Handle) -> None:
    handle.graph.replay()


def allocated() -> int:
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated()


def stop_on_fault(rid: str, e: BaseException) -> None:
    if isinstance(e, WC.GpuFault) or WC.is_fault(e):
        pytest.exit(f"{rid}: device error, nothing more is started on this GPU: {e}", returncode=3)


@pytest.mark.parametrize("rid", GC.CAPTURED)
def test_wrapper_replays_bit_for_bit(rid):
    r = WC.ROWS[rid]
    try:
        a, b = GC.row_sets(r, DEV)
        problems = GC.check_replay(lambda kw: WC.call(ops, r, kw), a, b, GC.overwrite_kw, capture=capture, replay=replay,
                                   clone=GC.clone_kw, snap=lambda kw, res: WC.snapshot(r, kw, res), inplace=bool(r.inplace), warm=warm,
                                   allocated=allocated, same_ok=GC.SAME_OK.get(rid, ()))
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        stop_on_fault(rid, e)
        raise
    assert not problems, "\n".join([f"{rid}: {len(problems)} problems:"] + problems)


@pytest.mark.parametrize("rid", list(GC.HOST_BOUND))
def test_host_bound_wrapper_raises_the_guard_under_capture(rid, monkeypatch):
    r = WC.ROWS[rid]
    kw = GC.host_kw(r, r.build(DEV))
    before = WC.snapshot(r, kw, None)
    monkeypatch.setattr(ops, "capturing", lambda: True)
    try:
        with pytest.raises(RuntimeError, match=rf"(?s){re.escape(r.fn)}.*capture") as info:
            WC.call(ops, r, kw)
    except Exception as e:  # noqa: BLE001
        stop_on_fault(rid, e)
        raise
    assert not WC.is_fault(info.value)  # a HIP error text is never a refusal
    torch.cuda.synchronize()
    after = WC.snapshot(r, kw, None)
    assert [n for n, _ in before] == [n for n, _ in after] and all(WC.same_bits(x, y) for (_, x), (_, y) in zip(before, after))
