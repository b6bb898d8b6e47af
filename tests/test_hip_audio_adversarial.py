"""Adversarial fp64 parity of the audio front-end kernels through pytorch_models._hip.ops: w2v_stem0 (none / layer / instance),
whisper_stem1, grouped_conv, group_windows, avgpool_time2, stft_mel (power, mel, log-mel).  References, bounds, input families and case lists live in
tests/audio_cases.py (its docstring maps every kernel path to the case that reaches it); tests/test_audio_cases_cpu.py proves on the
CPU that a correct kernel satisfies every assertion made here and that each defect in audio_cases.MUTANTS does not.

Per case: shape and dtype; the exact family EQUALS want.to(bf16); every other family stays within 1.5 x the derived bound
(audio_cases.MARGIN; no measured number enters an assertion; a zero bound - whisper_stem1's rows 0 and T + 1, group_windows' pad rows
and channels - means exact, and those are checked to be +0 bit patterns); poison: a second launch through lib(), the C ABI, on
operands cut out of NaN-filled buffers into a sentinel-filled output: finite, bit-identical to the plain run, every sentinel
intact; batch: every clip bit-identical to its single-clip run.  Each case prints
"FIGURE <op> <family> <id> ratio <max |err| / bound>" (pytest -s).

Measured on an MI355X (worst max |err| / bound per op and family; the exact family is bit-equal everywhere): see DESIGN.md,
"2e. Audio front-end numerics contract".  The assertions do not depend on those numbers.
"""
import pytest
import torch

import audio_cases as AC

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
            inp = AC.build(case)
            cache[case.id] = (inp, AC.reference(case, inp))
        return cache[case.id]

    return get


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(case, y, ref):
    assert tuple(y.shape) == AC.out_shape(case) and y.dtype == torch.bfloat16, (y.shape, y.dtype)
    zero = (ref["bound"] == 0) & (ref["want"] == 0)
    if case.op in ("whisper_stem1", "group_windows"):
        assert bool((_bits(y)[zero] == 0).all()), f"{case.id}: padding must be written as +0"
    ok, r = AC.accepts(case, {"y": y}, ref)
    print(f"FIGURE {case.op} {case.family} {case.id} ratio {r:.3f}")
    if case.family == "exact":
        bad = int((y.double() != AC.store(ref["want"], "bf16").double()).sum())
        assert ok, f"{case.id}: {bad} of {y.numel()} outputs differ from the exact result"
    else:
        assert ok, f"{case.id}: {r:.3f} x the bound (allowed {AC.MARGIN})"


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_parity(ops, solved, case):
    inp, ref = solved(case)
    y = AC.run(ops, case, AC.to_device(case, inp, DEV))["y"].cpu()
    _check(case, y, ref)
    if case.family == "poison":  # through the C ABI: NaN around every operand, sentinels around the output
        again = AC.run_abi(ops, case, inp, DEV)
        torch.cuda.synchronize()
        assert torch.isfinite(again["y"].float()).all(), f"{case.id}: picked up a NaN or a sentinel from outside its operands"
        assert torch.equal(_bits(again["y"]), _bits(y)), f"{case.id}: the output depends on where the operands lie"
        assert not again["guard_bad"], f"{case.id}: wrote outside its output"
    if case.family == "batch":
        for b in range(case.B):
            c1, one = AC.clip(case, inp, b)
            alone = AC.run(ops, c1, AC.to_device(c1, one, DEV))["y"].cpu()
            assert torch.equal(_bits(AC.rows_of_clip(case, y, b)), _bits(alone.reshape(-1))), f"{case.id}: clip {b} of the batch differs"


def test_refusals(ops):
    """cg = 20, cg = 6 and a span above 160 KiB are answered by the launcher's own argument checks, before any launch."""
    assert not ops.grouped_conv_supported(20, 24) and not ops.grouped_conv_supported(6, 8)
    for case in AC.REFUSED:
        assert AC.abi_refusal(case)
        xg = torch.zeros(case.B, case.G, AC.tp(case), case.cgp, dtype=torch.bfloat16, device=DEV)
        w = torch.zeros(case.G, case.cg, AC.kp(case), dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError, match="pm_grouped_conv_bf16"):
            ops.grouped_conv(xg, w, None, case.k, case.stride, case.cg)


# --------------------------------------------------------------------------------------------------------------- STFT / mel / log-mel
@pytest.fixture(scope="module")
def stft_solved(ops):
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = AC.stft_build(case, ops.stft_tables)
            cache[case.id] = (inp, AC.stft_forward(case, inp))
        return cache[case.id]

    return get


@pytest.mark.parametrize("case", AC.STFT_CASES, ids=lambda c: c.id)
def test_stft_parity(ops, stft_solved, case):
    """pm_stft_mel / pm_stft_mel_folded (+ pm_logmel_finalize) against the float64 contraction of the same tables: integer tables EQUAL,
    everything else within 1.5 x the derived bound, -inf (an all-silent clip) met exactly."""
    inp, ref = stft_solved(case)
    y = AC.stft_run(ops, case, inp, DEV).cpu()
    assert y.shape == ref["want"].shape
    ok, r = AC.stft_accepts(case, y, ref)
    print(f"FIGURE stft_mode{case.mode} {case.family} {case.id} ratio {r:.3f}")
    if case.family == "exact":
        assert ok, f"{case.id}: {int((y.double() != ref['want']).sum())} of {y.numel()} outputs differ from the exact result"
    assert ok, f"{case.id}: {r:.3f} x the bound (allowed {AC.MARGIN})"
    if case.family == "poison":
        again = AC.stft_run_abi(ops, case, inp, DEV)
        torch.cuda.synchronize()
        assert torch.equal(again["y"].view(torch.int32), y.view(torch.int32)), f"{case.id}: the output depends on where the operands lie"
        assert not torch.isnan(again["y"]).any() and not again["guard_bad"], f"{case.id}: read or wrote outside its operands"
    if case.family in ("batch", "loudness"):  # the per-clip peak: every clip alone gives the same bits
        flat = y.reshape(case.clips, -1)
        for b in range(case.clips):
            c1 = AC.StftCase(**{**case.__dict__, "B": 1, "lead": ()})
            alone = AC.stft_run(ops, c1, inp, DEV, x=inp["x"][b:b + 1]).cpu()
            assert torch.equal(alone.reshape(-1).view(torch.int32), flat[b].view(torch.int32)), f"{case.id}: clip {b} of the batch differs"


def test_stft_refusals(ops):
    """(1024, 256) with a mel phase and (2048, 512) exceed 64 KiB of LDS; mode 2 needs n_mels n_frames % 4 == 0: the launchers' own checks."""
    for case in AC.STFT_REFUSED:
        assert AC.stft_refusal(case)
        inp = AC.stft_build(case, ops.stft_tables)
        with pytest.raises(RuntimeError, match="pm_stft_mel|pm_logmel_finalize"):
            AC.stft_run(ops, case, inp, DEV)
