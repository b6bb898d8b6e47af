"""Adversarial fp64 parity of the 2-D convolution kernels and stems, through pytorch_models._hip.ops: conv_bf16, resnet_stem,
dwconv7_ln, convnext_stem, dwconv3_bn_act (y, psum, gate, write_y=False), maxvit_stem, im2col3x3, avgpool2x2, conv2d_nhwc.
References, bounds, input families and case lists live in tests/conv_cases.py (its docstring maps every kernel path to the case
that reaches it); tests/test_conv_cases_cpu.py proves on the CPU that a correct kernel satisfies every assertion made here and
that each defect in conv_cases.MUTANTS does not.

Per case: shape and dtype; pad columns exact zeros; the exact family EQUALS want.to(out dtype); every other family stays within
1.5 x the derived bound (conv_cases.MARGIN; no measured number enters an assertion); poison: finite and bit-identical on operands
cut out of NaN-filled buffers; batch: every image bit-identical to its single-image run; dwconv3: psum by its own bound and
write_y=False equal to the psum of the full run.  Each case prints "FIGURE <op> <family> <id> ratio <max |err| / bound>" (pytest -s).

Measured on an MI355X (worst max |err| / bound per kernel, over the cancel / offset / poison / batch families; the exact family
is bit-equal everywhere): see DESIGN.md, "2c. Convolution numerics contract".
    op             output  cancel  offset  poison  batch
    conv_bf16      bf16    0.956   -       0.995   0.992
    conv2d_nhwc    bf16    0.999   -       0.999   0.999
    resnet_stem    bf16    0.989   -       0.990   0.993
    dwconv7_ln     bf16    0.998   0.349   0.996   0.992
    dwconv7_ln     f32     0.527   0.072   0.125   0.065
    convnext_stem  bf16    0.995   0.383   0.996   0.994
    convnext_stem  f32     0.012   0.054   0.046   0.014
    dwconv3        bf16    0.998   -       0.999   0.999
    dwconv3        f32     0.144   -       0.214   0.190
    maxvit_stem    bf16    0.997   -       0.998   0.999
    maxvit_stem    f32     0.031   -       0.119   0.093
    im2col3x3      bf16    -       -       0.997   0.999    (f32: exact copies)
    avgpool2x2     bf16    -       -       1.000   1.000    (f32: 0.136, 0.131)
With a bf16 output the half-ulp store term dominates the bound and a correct store reaches it; the f32 rows show the arithmetic
alone.  224 tests, 3.5 s.  The assertions do not depend on these numbers.
"""
import pytest
import torch

import conv_cases as CC

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
            inp = CC.build(case)
            cache[case.id] = (inp, CC.reference(case, inp))
        return cache[case.id]

    return get


def _cpu(out: dict) -> dict:
    return {k: v.cpu() for k, v in out.items() if v is not None}


def _check(case, out, ref):
    y = out["y"]
    assert tuple(y.shape) == CC.out_shape(case) and y.dtype == CC.DT[case.ydt], (y.shape, y.dtype)
    ldy, width = CC.default_ldy(case), (9 * case.C if case.op == "im2col3x3" else case.Cout or case.C)
    if ldy is not None and ldy > width:
        assert (y[..., width:].float() == 0).all(), f"{case.id}: pad columns must be written as zeros"
    if "psum" in out:
        assert out["psum"].dtype == torch.float32 and out["psum"].shape == ref["psum"].shape
        assert torch.equal(out["psum_only"], out["psum"]), "write_y=False returns the psum of the full run"
    ok, r = CC.accepts(case, out, ref)
    print(f"FIGURE {case.op} {case.family} {case.id} ratio {r:.3f}")
    if case.family == "exact":
        bad = int((y.double() != CC.store(ref["want"], case.ydt).double()).sum())
        assert ok, f"{case.id}: {bad} of {y.numel()} outputs differ from the exact result"
    else:
        assert ok, f"{case.id}: {r:.3f} x the bound (allowed {CC.MARGIN})"


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_parity(ops, solved, case):
    inp, ref = solved(case)
    out = CC.run(ops, case, CC.to_device(case, inp, DEV))
    got = _cpu(out)
    _check(case, got, ref)
    if case.family == "poison":  # every operand cut out of a NaN-filled buffer, one image of NaNs on each side
        again = _cpu(CC.run(ops, case, CC.to_device(case, inp, DEV, poison=True)))
        for k, v in got.items():
            assert torch.isfinite(again[k]).all(), f"{case.id}: {k} picked up a NaN from outside its operands"
            assert torch.equal(again[k], v), f"{case.id}: {k} depends on where the operands lie"
    if case.family == "batch":  # tiles, strips and workgroups that span images
        for n in range(case.N):
            c1, one = CC.image(case, inp, n)
            alone = _cpu(CC.run(ops, c1, CC.to_device(c1, one, DEV)))
            for k, v in got.items():
                assert torch.equal(CC.rows_of_image(case, v, n), alone[k].reshape(-1)), f"{case.id}: image {n} of the batch differs in {k}"
