"""Adversarial fp64 parity of the Mixer and ViT token-path kernels through lib(), the C ABI: pm_mixer_token_mix_bf16, pm_ln_mean,
pm_transpose_add_f32, pm_cls_head_gemm, pm_cls_attend, pm_vit_tokens, pm_vit_tokens_generic and the row reductions pm_mean_ln,
pm_ln_space_to_depth, pm_se_gate, pm_mean_rows_bf16, pm_rmsnorm, pm_geglu.  References, bounds, input families and case lists live in
tests/token_cases.py (its docstring maps every kernel path to the case that reaches it); tests/test_token_cases_cpu.py proves on
the CPU that a correct kernel satisfies every assertion made here and that each defect in token_cases.MUTANTS does not.

Per case (token_cases.verify): shape and dtype; every run writes into a sentinel-guarded output; the exact, locate and move
families EQUAL the reference; every other family stays within 1.5 x the derived bound (MARGIN; no measured number enters an
assertion; a zero bound means exact; a non-finite output is an infinite ratio; no element is excluded); token mixing's row partials
against sums over the kernel's own rounded output; perm: a permutation of the images, each image alone and (token mixing) out = x
give the batch's bits.  poison: a second launch on operands cut out of NaN-filled buffers (cls_attend: NaN between the rows and the
images of a strided x; the generic ViT weight: NaN beyond Kpad): finite, bit-identical to the plain run, every sentinel intact.
Token mixing asks pm_mixer_token_mix_plan again before it launches.  Each case prints
"FIGURE <op> <family> <id> ratio <max |err| / bound>" (pytest -s).

Measured on an MI355X (worst ratio per op and family): profiles/token_parity/README.md.  The assertions do not depend on those numbers.
"""
import pytest
import torch

import token_cases as TC

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
            inp = TC.build(case)
            cache[case.id] = (inp, TC.reference(case, inp))
        return cache[case.id]

    return get


def _parity(ops, solved, case):
    inp, ref = solved(case)
    be = TC.Device(ops, DEV)
    if case.op == "token_mix":  # the launcher's own word on where this case goes
        rep = ops.mixer_token_mix_plan(case.d["T"], case.d["Dt"], case.d["C"])
        assert rep == TC.tm_plan(case.d["T"], case.d["Dt"], case.d["C"]) and TC.paths(case, rep) == TC.paths(case), (case.id, rep)
    ok, r, msg = TC.verify(case, inp, ref, be)
    print(f"FIGURE {case.op} {case.family} {case.id} ratio {r:.3f}")
    assert ok, f"{case.id}: {msg}"
    if case.family == "poison":
        plain = be.run(case, inp)
        again = TC.run_abi(ops, case, inp, DEV)
        torch.cuda.synchronize()
        for key in ("y", "rows"):
            if plain.get(key) is None:
                continue
            assert torch.isfinite(again[key].float()).all(), f"{case.id}: {key} picked up a NaN from outside its operands"
            assert torch.equal(TC.bits(again[key]), TC.bits(plain[key])), f"{case.id}: {key} depends on where the operands lie"
        assert again["guard_ok"], f"{case.id}: wrote outside its output"


def _of(*ops_):
    return [c for c in TC.CASES if c.op in ops_]


@pytest.mark.parametrize("case", _of("token_mix"), ids=lambda c: c.id)
def test_token_mix_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("ln_mean", "transpose"), ids=lambda c: c.id)
def test_ln_mean_and_transpose_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("cls_head_gemm", "cls_attend"), ids=lambda c: c.id)
def test_cls_tail_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of("vit_tokens"), ids=lambda c: c.id)
def test_vit_tokens_parity(ops, solved, case):
    _parity(ops, solved, case)


@pytest.mark.parametrize("case", _of(*TC.ROW_OPS), ids=lambda c: c.id)
def test_row_reduction_parity(ops, solved, case):
    _parity(ops, solved, case)


def test_refusals(ops):
    """Each is answered by the launcher's own argument checks (PM_EINVAL 1, PM_EUNSUPPORTED 2, PM_EALIGN 4) before any launch."""
    L = ops.lib()
    big = torch.zeros(1 << 18, device=DEV)
    p = big.data_ptr()
    obuf, out = TC.embedded(torch.empty(1 << 12, dtype=torch.bfloat16), DEV, sentinel=True)
    for T, Dt, C in TC.REFUSED_TOKEN_MIX:  # (16, 1024, 128) first: one step past the largest served Dt
        assert not ops.mixer_token_mix_supported(T, Dt, C)
        assert L.pm_mixer_token_mix_bf16(p, p, p, p, p, p, p, p, out.data_ptr(), None, 1, T, Dt, C, None) == 2, (T, Dt, C)
    torch.cuda.synchronize()
    assert TC.sentinels_intact(obuf, out[:0]), "a refused call wrote to its output"
    with pytest.raises(ValueError, match="do not fit"):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        ops.mixer_token_mix(z(1, 16, 128, dt=torch.bfloat16), z(16, 2), z(128), z(128), z(32, 1, 64, 8, dt=torch.bfloat16), z(1024),
                            z(1, 64, 64, 8, dt=torch.bfloat16), z(16))
    assert L.pm_mixer_token_mix_bf16(p + 2, p, p, p, p, p, p, p, out.data_ptr(), None, 1, 16, 32, 64, None) == 4  # a misaligned x
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 1, 16384, 1, None) == 2   # (C + R) * 4 bytes of LDS above 64 KiB: refused, not PM_ELAUNCH
    assert L.pm_se_gate(p, 1, 1, p, p, p, p, p, 1, 12289, 4096, None) == 2
    assert L.pm_ln_mean(p, 0, p, p, p, p, 0, 1, 0, 4, None) == 1 and L.pm_transpose_add_f32(p, None, p, 3, 1, 4, 4, None) == 1  # T = 0; ldy < R
    assert L.pm_cls_head_gemm(p, 64, 32, p, None, p, 64, 64, 1, 64, 48, 1, None) == 1   # K % 32
    assert L.pm_cls_head_gemm(p, 36, 32, p, None, p, 64, 64, 1, 64, 32, 1, None) == 4   # ldx % 8
    assert L.pm_cls_attend(p, 1088, 1088, None, p, p, 1, 1, 1088, 1, 0.125, 1e-6, None) == 2   # d > 1024
    assert L.pm_cls_attend(p, 64, 64, None, p, p, 1, 1, 64, 17, 0.125, 1e-6, None) == 1       # H > 16
    assert L.pm_vit_tokens(p, p, p, p, None, p, 1, 32, 40, 16, 64, None) == 2                 # W % 16
    assert L.pm_vit_tokens_generic(p, p, 576, p, p, None, p, 1, 28, 28, 14, 64, None) == 1    # ldw < Kpad = 640
    assert L.pm_geglu(p, 16, p, 8, 1, 12, None) == 1 and L.pm_geglu(p, 32, p, 16, 1, 12, None) == 2  # ldh < 2 F; F % 8
    assert L.pm_rmsnorm(p, 12, 0, p, 1e-6, p, 12, 0, 1, 12, None) == 2                        # d % 8
    torch.cuda.synchronize()
