"""GPU: the non-finite operand contract on whole models and decoding entry points (tests/nonfinite_cases.py: MODELS_POISON,
ENTRY_POINTS).

Every model of graph_cases.MODELS with a float input runs at its family's smallest geometry with a batch of three (two where the
family has none), clean and with ONE element of the middle sample's input set to each of the four poisons: the other samples keep
their bits, integer results stay in range and the poisoned sample shows a non-finite float unless the model is listed in
SWALLOWS.  The decoding entry points run the same protocol on the encoder memory, the log-mel or the waveform: a healthy row's
ids, log-probs and beam scores keep their bits over their whole length (no eos is set), the poisoned row's ids stay inside the
vocabulary.  Where a forward takes ``lengths=``, NaN in the padded tail of the input changes no bit."""
import pytest
import torch

import coherence_cases as CC
import graph_cases as GC
import nonfinite_cases as NF
import wrapper_cases as WC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
torch.set_grad_enabled(False)
SEED = 2931
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _guard(what: str, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{what}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise


def _module(case: GC.Model, k: int, dtype: str):
    m = CC.filled(case.make(k), SEED)
    return (m.to(torch.bfloat16) if dtype == "bf16" else m).to(DEV)


def _inputs(case: GC.Model, k: int, dtype: str) -> dict:
    return {f"x{i}": (x.to(DTYPES[dtype]) if i in case.cast else x).to(DEV) for i, x in enumerate(case.inputs(k, SEED))}


FORWARDS = [key for key, mp in NF.MODELS_POISON.items() if mp.input is not None]


@pytest.mark.parametrize("poison", NF.POISONS)
@pytest.mark.parametrize("key", FORWARDS)
def test_one_poisoned_sample_of_a_model_stays_alone_and_is_seen(key, poison):
    case, mp = GC.MODELS[key], NF.MODELS_POISON[key]
    k, dtype = NF.model_geometry(case), case.dtypes[0]
    m, kw = _module(case, k, dtype), _inputs(case, k, dtype)
    run = (lambda kw: [(n, t.clone()) for n, t in GC.flat(getattr(m, case.method)(*kw.values()))]) if case.method else NF.model_run(m)
    problems = _guard(f"{key} {poison}", lambda: NF.check_isolation(run, kw, NF.model_unit(mp), poison, swallows=NF.swallowed(key)))
    assert not problems, "\n".join([f"{key} {dtype} {poison}: {len(problems)} problems:"] + problems)


def test_models_without_a_float_input_say_why():
    for table in (NF.MODELS_POISON, NF.ENTRY_POINTS):
        for key, mp in table.items():
            assert (mp.input is None) == bool(mp.why), key
            if mp.input is None and key in GC.MODELS:
                assert not any(x.is_floating_point() for x in GC.MODELS[key].inputs(0, SEED)), key


# ---------------------------------------------------------------------------------------------------------- the entry points
V, N_NEW = 300, 6


def _whisper():
    case = GC.MODELS["Whisper"]
    w = _module(case, 1, "bf16")
    mel, tokens = (x.to(DEV) for x in case.inputs(1, SEED))
    return w, mel.to(torch.bfloat16), tokens


def _tensors(res) -> list:
    res = res if isinstance(res, (tuple, list)) else (res,)
    return [(f"output {i}", t.clone()) for i, t in enumerate(res) if isinstance(t, torch.Tensor)]


def _entry(key: str, lengths=None):
    """(run, operands, ranges) of an entry point; ``lengths``: passed on as lengths= (the Wav2Vec2CTC entry points)"""
    if key.startswith("Whisper"):
        w, mel, tokens = _whisper()
        prompt = tokens[:, :2].contiguous()
        if key == "Whisper.generate":
            return (lambda kw: _tensors(w.generate(kw["x0"], prompt, N_NEW, return_logprobs=True))), {"x0": mel}, {"output 0": (0, V)}
        if key == "Whisper.align":
            return (lambda kw: _tensors(w.align(kw["x0"], tokens))), {"x0": mel}, {"output 0": (-1, mel.shape[2] // 2)}
        memory = w.encoder(mel)
        how = {"greedy": dict(return_logprobs=True), "sampled": dict(topk=0, temperature=0.7, top_p=0.9, seed=3, return_logprobs=True),
               "beam": dict(beams=2, return_beams=True)}[key.split(":")[1]]
        return (lambda kw: _tensors(w.decoder.generate(kw["x0"], prompt, N_NEW, **how))), {"x0": memory}, {"output 0": (0, V)}
    case = GC.MODELS["Wav2Vec2CTC"]
    m, (x,) = _module(case, 1, "bf16"), case.inputs(1, SEED)
    targets, tl = torch.tensor([[3, 4], [5, 6], [7, 8]]), [2, 1, 2]
    frames = 64  # above any frame count of these clips
    if key == "Wav2Vec2CTC.decode":
        return (lambda kw: _tensors(m.decode(kw["x0"], lengths))), {"x0": x.to(DEV)}, {"output 0": (-1, 32), "output 1": (0, frames), "output 2": (-1, frames)}
    if key == "Wav2Vec2CTC.score":
        return (lambda kw: _tensors(m.score(kw["x0"], targets, tl, lengths))), {"x0": x.to(DEV)}, {}
    return (lambda kw: _tensors(m.align(kw["x0"], targets, tl, lengths))), {"x0": x.to(DEV)}, {"output 0": (-1, frames), "output 1": (-1, frames)}


ENTRIES = [key for key, mp in NF.ENTRY_POINTS.items() if mp.input is not None]


@pytest.mark.parametrize("poison", NF.POISONS)
@pytest.mark.parametrize("key", ENTRIES)
def test_one_poisoned_sample_of_a_decoding_call_stays_alone_and_is_seen(key, poison):
    run, kw, ranges = _guard(key, lambda: _entry(key))
    assert kw["x0"].shape[0] == 3
    unit = NF.U("x0", ranges=ranges)
    problems = _guard(f"{key} {poison}", lambda: NF.check_isolation(run, kw, unit, poison, swallows=NF.swallowed(key)))
    assert not problems, "\n".join([f"{key} {poison}: {len(problems)} problems:"] + problems)


WITH_LENGTHS = [key for key, case in GC.MODELS.items() if case.lengths is not None and NF.MODELS_POISON[key].input is not None]


@pytest.mark.parametrize("key", WITH_LENGTHS)
def test_nan_behind_a_clips_length_changes_no_bit(key):
    case = GC.MODELS[key]
    m, kw = _module(case, 1, "bf16"), _inputs(case, 1, "bf16")
    lengths = case.lengths(1)
    masks = {"x0": lambda k: (torch.arange(k["x0"].shape[1])[None, :] >= lengths[:, None])}
    problems = _guard(key, lambda: NF.check_ignored(lambda k: [(n, t.clone()) for n, t in GC.flat(m(k["x0"], lengths.to(DEV)))], kw, masks))
    assert not problems, "\n".join([f"{key}: {len(problems)} problems:"] + problems)


@pytest.mark.parametrize("key", ["Wav2Vec2CTC.decode", "Wav2Vec2CTC.score", "Wav2Vec2CTC.align"])
def test_nan_behind_a_clips_length_changes_no_id_start_or_score(key):
    """the entry points where the padded samples meet the packed ctc_* kernels: ids, counts, first frames, path and target scores"""
    lengths = GC.MODELS["Wav2Vec2CTC"].lengths(1)
    run, kw, _ = _guard(key, lambda: _entry(key, lengths.to(DEV)))
    masks = {"x0": lambda k: (torch.arange(k["x0"].shape[1])[None, :] >= lengths[:, None])}
    problems = _guard(key, lambda: NF.check_ignored(run, kw, masks))
    assert not problems, "\n".join([f"{key}: {len(problems)} problems:"] + problems)
