"""Adversarial fp64 parity of the EnCodec kernels through pytorch_models._hip.ops: conv1d_f32 (plain and transposed form), lstm_f32
(one, two - wavefront and plain - and three layers, residual), rvq_encode, rvq_decode, groupnorm1_, encodec_scale, scale_clips.
References, bounds, input families and case lists live in tests/encodec_cases.py (its docstring maps every kernel path to the case
that reaches it); tests/test_encodec_cases_cpu.py proves on the CPU that a correct kernel satisfies every assertion made here and
that each defect in encodec_cases.MUTANTS does not.

Per case (encodec_cases.verify): shape and dtype; the exact family EQUALS the reference; every other family stays within 1.5 x the
derived bound (MARGIN; no measured number enters an assertion; a zero bound means exact); the LSTM step by step against the
reference fed with the kernel's own h_(t-1); RVQ codes by the decided rule; batch: every clip / row bit-identical to its run alone.
poison: a second launch through lib(), the C ABI, on operands cut out of NaN-filled buffers (a NaN gap between the clips of a
convolution) into a sentinel-filled output with a NaN-filled workspace: finite, bit-identical to the plain run, every sentinel
intact.  Each case prints "FIGURE <op> <family> <id> ratio <max |err| / bound>" (pytest -s).

Measured on an MI355X (worst ratio per op and family): see profiles/encodec_parity/README.md and DESIGN.md, "2f. EnCodec numerics
contract".  The assertions do not depend on those numbers.
"""
import ctypes

import pytest
import torch

import encodec_cases as EC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from pytorch_models._hip import ops as o

    return o


@pytest.fixture(scope="module")
def solved():
    """(inputs, float64 reference) per case id: computed once, shared, left unchanged."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = EC.build(case)
            cache[case.id] = (inp, EC.reference(case, inp))
        return cache[case.id]

    return get


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.int64 else torch.int32)


def _parity(ops, solved, case):
    inp, ref = solved(case)
    be = EC.Device(ops, DEV)
    ok, r, msg = EC.verify(case, inp, ref, be)
    print(f"FIGURE {case.op} {case.family} {case.id} ratio {r:.3f}")
    assert ok, f"{case.id}: {msg}"
    if case.family == "poison":  # through the C ABI: NaN around every operand and in the workspace, sentinels around the output
        y = EC.run_plain(be, case, inp)
        again = EC.run_abi(ops, case, inp, DEV)
        torch.cuda.synchronize()
        assert again["y"].dtype == torch.int64 or torch.isfinite(again["y"]).all(), f"{case.id}: picked up a NaN from outside its operands"
        assert torch.equal(_bits(again["y"]), _bits(y)), f"{case.id}: the output depends on where the operands lie"
        assert not again["guard_bad"], f"{case.id}: wrote outside its output"
        if case.op == "scale":
            for key, divide in (("div", True), ("mul", False)):
                assert torch.equal(_bits(again[key]), _bits(be.scale_clips(inp["x"], y, divide))), f"{case.id}: scale_clips {key}"


def _of(*ops_):
    return [c for c in EC.CASES if c.op in ops_]


@pytest.mark.parametrize("case", _of("conv", "convT"), ids=lambda c: c.id)
def test_conv_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("lstm"), ids=lambda c: c.id)
def test_lstm_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("rvq_encode", "rvq_decode"), ids=lambda c: c.id)
def test_rvq_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("groupnorm", "scale"), ids=lambda c: c.id)
def test_groupnorm_and_scale_parity(ops, solved, case):
    _parity(ops, solved, case)


def test_refusals(ops):
    """Each is answered by the launcher's own argument checks (PM_EINVAL 1, PM_EUNSUPPORTED 2, PM_EALIGN 4) before any launch."""
    L = ops.lib()
    x = torch.zeros(2, 4, 4, device=DEV)
    w = torch.zeros(8, 9 * 4, device=DEV)
    y = torch.zeros(2, 16, 4, device=DEV)
    conv = lambda xp, xbs, res, k, left, right, zero, up, trim, tout: L.pm_conv1d_f32(  # noqa: E731
        xp, xbs, w.data_ptr(), None, res, y.data_ptr(), 2, 4, 4, 4, k, 1, left, right, zero, 0, up, trim, tout, None)
    assert conv(x.data_ptr(), 16, None, 7, 4, 2, 0, 1, 0, 4) == 2           # left >= Tin
    assert conv(x.data_ptr(), 16, None, 9, 2, 2, 0, 1, 0, 1) == 2           # Tin + left + right < k
    assert conv(x.data_ptr(), 16, y.data_ptr(), 2, 1, 1, 1, 2, 0, 10) == 1  # residual with up != 1
    assert conv(x.data_ptr(), 16, None, 2, 1, 1, 1, 2, 3, 8) == 1           # trim + Tout > Mr up
    assert conv(x.data_ptr() + 4, 16, None, 3, 1, 1, 0, 1, 0, 4) == 4       # a misaligned x with Cin % 4 == 0
    assert conv(x.data_ptr(), 18, None, 3, 1, 1, 0, 1, 0, 4) == 4           # x_batch_stride % 4 != 0 with Cin % 4 == 0
    big, out = torch.zeros(2, 1 << 16, device=DEV)  # encodec_cases.REFUSED itself, every buffer far larger than the case asks for
    for case, rc in zip(EC.REFUSED, EC.REFUSED_RC):
        if case.op == "lstm":
            one = (ctypes.c_void_p * 1)(big.data_ptr())
            got = L.pm_lstm_f32(big.data_ptr(), one, one, one, case.layers, out.data_ptr(), out.data_ptr(), 0, case.B, case.T, case.C, None)
        else:
            g = EC.conv_geometry(case)
            got = L.pm_conv1d_f32(big.data_ptr(), case.T * case.C, big.data_ptr(), None, out.data_ptr() if case.resid else None,
                                  out.data_ptr(), case.B, case.T, case.C, case.Cout, g["k"], g["stride"], g["left"], g["right"],
                                  int(g["zero_pad"]), int(case.elu), g["up"], g["trim"], g["Tout"], None)
        assert got == rc, (case.id, got)
    with pytest.raises(ValueError, match="not served"):
        ops.conv1d_f32(x, w[:, :28].contiguous(), None, k=7, left=4, right=2)
    with pytest.raises(ValueError, match="resid"):
        ops.conv1d_f32(x, w[:, :8].contiguous(), None, k=2, left=1, right=1, zero_pad=True, up=2, resid=y[:, :10].contiguous())
    wl = [torch.zeros(4 * 96, 96, device=DEV)]
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.lstm_f32(torch.zeros(1, 2, 96, device=DEV), wl, wl, [torch.zeros(4 * 96, device=DEV)])
    ptrs = (ctypes.c_void_p * 1)(wl[0].data_ptr())
    assert L.pm_lstm_f32(x.data_ptr(), ptrs, ptrs, ptrs, 1, y.data_ptr(), y.data_ptr(), 0, 1, 2, 96, None) == 2  # H = 96
    z = torch.zeros(4, 64, device=DEV)
    codes = torch.zeros(1, 4, dtype=torch.int64, device=DEV)
    assert L.pm_rvq_encode_f32(z.data_ptr(), z.data_ptr(), z.data_ptr(), codes.data_ptr(), 4, 1, 64, 1024, None) == 2  # dim != 128
    assert L.pm_rvq_decode_f32(codes.data_ptr(), 4, 4, 1, z.data_ptr(), y.data_ptr(), 1, 4, 1, 64, 1024, None) == 2
    work = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert L.pm_groupnorm1_f32(y.data_ptr(), z.data_ptr(), z.data_ptr(), None, work.data_ptr(), 1, 10, 4, 1e-5, None) == 1  # n % C != 0
