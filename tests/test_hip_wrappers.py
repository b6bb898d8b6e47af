"""GPU: the wrapper operand contract on the kernels (tests/wrapper_cases.py; the CPU half, which audits
every accepted variant against the launch it makes, is tests/test_wrapper_cases_cpu.py).

One test per row of the table.  The canonical call runs once; then every generated variant of every tensor operand - a stride-2
last dimension, padded leading dimensions, permuted strides, a stride-0 broadcast, an unaligned pointer, every other dtype of
the family, one rank more or fewer - either raises (ValueError / TypeError / IndexError / RuntimeError, a refusal of the C ABI
such as PM_EALIGN included) with every in-place operand untouched, or returns outputs and in-place results bit-identical to
the same call on a fresh contiguous tensor holding the variant's values, and leaves the variant's parent buffer alone outside
the view.  All failing variants of a wrapper are reported together.  Every variant is a view into a NaN / sentinel parent
large enough for a packed read of the widest dtype (wrapper_cases.Variant.check_bounds), so a layout a kernel ignores poisons
the result; it cannot leave the buffer."""
import pytest
import torch

import wrapper_cases as WC
from pytorch_models._hip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)


@pytest.mark.parametrize("rid", list(WC.ROWS))
def test_wrapper_honours_or_refuses_every_operand_layout(rid):
    r = WC.ROWS[rid]
    try:
        problems, accepted = WC.check_row(ops, r, DEV, compare=True)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{rid}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    print(f"{rid}: {len(accepted)} variants accepted bit-identically or refused cleanly; {len(problems)} problems")
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)
