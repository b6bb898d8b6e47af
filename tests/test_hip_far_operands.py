"""GPU: far operands on the kernels (tests/wrapper_cases.py; the CPU half, which gates every case by the
containment arithmetic and audits the launch, is tests/test_wrapper_cases_cpu.py).

One test per row of the wrapper table (and of wrapper_cases.FAR_ROWS, two-row forms whose stride itself passes 2^31 elements).  The canonical call runs once; then, for every operand and every stride-carrying
leading dimension, the operand becomes a view into one poisoned arena whose stride in that dimension carries the last index
just past 2^31 bytes, 2^32 bytes or 2^31 elements from the base - where the last rows of a batch large enough would lie.  The
call is refused (in-place operands unchanged, the arena still all poison outside the view), or its outputs and in-place results
are bit-identical to the canonical call's and the arena outside the view is unchanged; a far ``out=`` holds the canonical bits in
the view.  The arena is sized so that any single 32-bit misreading of the far term stays inside it (wrapper_cases.FarCase.needs):
a wrapped offset reads NaN or writes where the scan finds it; it does not leave the allocation.  Cost per case: one read of the
arena.  All failing variants of a wrapper are reported together; a device error ends the run."""
import pytest
import torch

import wrapper_cases as WC
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)
HEADROOM = 2 << 30


@pytest.fixture(scope="module")
def arena():
    need = WC.Arena.bytes_for(32)
    free, _ = torch.cuda.mem_get_info()
    if free < need + HEADROOM:
        pytest.skip(f"far operands need an arena of {need} bytes plus {HEADROOM}: {free} bytes of device memory are free")
    a = WC.Arena(need, DEV)
    torch.cuda.synchronize()
    yield a
    del a.words
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rid", list(WC.ALL_FAR_ROWS))
def test_wrapper_honours_or_refuses_every_far_operand(rid, arena):
    r = WC.ALL_FAR_ROWS[rid]
    try:
        problems, accepted, refused = WC.check_row_far(ops, r, DEV, arena, compare=True)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{rid}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    print(f"{rid}: {len(accepted)} far variants accepted bit-identically, {len(refused)} refused cleanly; {len(problems)} problems")
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)
