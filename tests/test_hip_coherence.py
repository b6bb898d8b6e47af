"""GPU: derived-state coherence of the HIP paths (tests/coherence_cases.py; the CPU half is tests/test_coherence_cases_cpu.py).

Every test changes the weights of a module that has already run - which no parity suite does - and compares bit for bit with
what must come out:
  * one tensor at a time: after an in-place write the warm module computes what it computes once clear_derived() has dropped
    every cache (a dependency missing from a derived() tuple fails here), and the output moved (the write was not ignored);
  * a whole checkpoint, a .float() / .to(bfloat16) round trip and a .cpu() / update / .cuda() round trip: every entry point
    equals a freshly built module that never saw the old weights (a cache clear_derived does not know about fails here);
  * GraphedForward recaptures after an update and replays unchanged otherwise; GreedyDecoder / BeamDecoder refuse rebind() and
    run() after an update, and a new decoder equals greedy_decode / beam_decode on the updated model.
Every call is one the family tests already make, with other weights."""
import pytest
import torch

import coherence_cases as CC
from pytorch_models.transformer import clear_derived

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_grad_enabled(False)


def hip_model(fam, seed=CC.SEED):
    m = fam.make(seed)
    return (m.to(torch.bfloat16) if fam.dtype == "bf16" else m).to(DEV)


def on_dev(fam):
    return {k: v.to(DEV) for k, v in fam.inputs().items()}


def derived_keys(model) -> set:
    return {str(k) for mod in model.modules() for k in mod.__dict__.get("_pm_derived", {})}


def derived_objects(model) -> dict:
    """(module name, key) -> the cached value object of every derived() entry"""
    return {(n, str(k)): hit[1] for n, mod in model.named_modules() for k, hit in mod.__dict__.get("_pm_derived", {}).items()}


_FRESH: dict = {}


def fresh_outputs(fam) -> dict:
    """every entry point of a module built from the second checkpoint that never held another: computed once per family"""
    if fam.id not in _FRESH:
        m, inp = hip_model(fam, CC.SEED + 1), on_dev(fam)
        _FRESH[fam.id] = {name: tuple(o.cpu() for o in CC.outputs(fam, name, m, inp)) for name in fam.entries}
    return _FRESH[fam.id]


def assert_fresh(fam, model, inp, what: str) -> None:
    want = fresh_outputs(fam)
    for name in fam.entries:
        got = tuple(o.cpu() for o in CC.outputs(fam, name, model, inp))
        assert CC.same(got, want[name]), f"{fam.id}.{name} after {what}: not what a fresh module computes"


CASES = [(fid, name) for fid, fam in CC.FAMILIES.items() for name in fam.entries]


@pytest.mark.parametrize("fid,name", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_one_tensor_at_a_time(fid, name):
    fam = CC.FAMILIES[fid]
    model, inp = hip_model(fam), on_dev(fam)
    prev = CC.outputs(fam, name, model, inp)  # warm: every derived value is built from the first weights
    if name == next(iter(fam.entries)):
        assert set(fam.expect) <= derived_keys(model), (fam.expect, sorted(derived_keys(model)))  # the path the row is about ran
    if fid in ("encoder_fold", "encoder_pre"):  # the LayerNorm fold engages at the one large size and not at the tiny one
        from pytorch_models._hip import ops

        x = inp["x"]
        M, d, hid = x.shape[0] * x.shape[1], x.shape[2], 4 * x.shape[2]
        folds = bool(ops.linear_ln_supported(M, d, d, "none", True) and ops.linear_ln_supported(M, d, hid, "none", True))
        assert folds == (fid == "encoder_fold") and model[0].chain_ok(x.to(torch.bfloat16)) == folds
    kept = derived_objects(model)
    CC.outputs(fam, name, model, inp)  # a second warm run rebuilds nothing: no dependency is a fresh object on every call
    again = derived_objects(model)
    assert kept.keys() == again.keys() and all(again[k] is v for k, v in kept.items()), \
        [k[1] for k, v in kept.items() if again.get(k) is not v]
    stale, ignored = [], []
    for key in fam.keys(model):
        CC.overwrite(model, key)
        warm = CC.outputs(fam, name, model, inp)
        clear_derived(model)
        cold = CC.outputs(fam, name, model, inp)
        if not CC.same(warm, cold):
            stale.append(key)
        if fam.entries[name].moves and not fam.is_quiet(key) and CC.same(cold, prev):
            ignored.append(key)
        prev = cold
    assert not stale, f"{fid}.{name}: stale derived state after an in-place write to {stale}"
    assert not ignored, f"{fid}.{name}: the output did not move after a write to {ignored}"


WHOLE = [f.id for f in CC.FAMILIES.values() if f.whole]


@pytest.mark.parametrize("fid", WHOLE)
def test_whole_checkpoint_equals_a_fresh_module(fid):
    fam = CC.FAMILIES[fid]
    model, inp = hip_model(fam), on_dev(fam)
    first = {name: tuple(o.cpu() for o in CC.outputs(fam, name, model, inp)) for name in fam.entries}
    CC.load_state(model, CC.second_state(fam))  # copy_ into the warm parameters and buffers
    assert_fresh(fam, model, inp, "load_state_dict")
    for name, e in fam.entries.items():
        if e.moves:
            assert not CC.same(first[name], fresh_outputs(fam)[name]), name  # the two checkpoints do differ at the output


@pytest.mark.parametrize("assign", [False, True], ids=["copy", "assign"])
@pytest.mark.parametrize("fid", WHOLE)
def test_cpu_round_trip_equals_a_fresh_module(fid, assign):
    """.cpu() frees the device copies, .cuda() allocates new ones - by preference at the addresses just freed.  With
    ``assign`` the update swaps in new Parameter objects, whose version counters start again: address, version, dtype and
    device of a tensor can all repeat, and only the identity of the dependencies tells the two states apart."""
    fam = CC.FAMILIES[fid]
    model, inp = hip_model(fam), on_dev(fam)
    for name in fam.entries:
        CC.outputs(fam, name, model, inp)
    model.cpu()
    CC.load_state(model, CC.second_state(fam), assign=assign)  # the update happens on the CPU
    model.to(DEV)
    assert_fresh(fam, model, inp, ".cpu(), an update, .cuda()")


@pytest.mark.parametrize("fid", [f.id for f in CC.FAMILIES.values() if f.fp32 and f.dtype == "bf16" and f.whole])
def test_dtype_round_trip_equals_a_fresh_module(fid):
    fam = CC.FAMILIES[fid]
    model, inp = hip_model(fam), on_dev(fam)
    for name in fam.entries:
        CC.outputs(fam, name, model, inp)
    model.float()
    CC.load_state(model, CC.second_state(fam))
    got = CC.outputs(fam, "forward", model, inp)
    want = CC.outputs(fam, "forward", fam.make(CC.SEED + 1).to(DEV), inp)  # an fp32 module that never was anything else
    assert CC.same(got, want), f"{fid}: .float() after a bf16 run is not the fp32 module"
    model.to(torch.bfloat16)
    assert_fresh(fam, model, inp, ".float(), an update, .to(bfloat16)")


# ---- holders of raw pointers
@pytest.mark.parametrize("fid", ["encoder_pre", "vit", "mixer_bf16", "convnext"])
def test_graphed_forward_recaptures_after_an_update(fid):
    from pytorch_models.graph import GraphedForward

    fam = CC.FAMILIES[fid]
    model, inp = hip_model(fam), on_dev(fam)
    (x,) = inp.values()
    x = x.to(torch.bfloat16) if fid == "encoder_pre" else x
    g = GraphedForward(model, x)
    graph0 = g.graph
    assert torch.equal(g(x), model(x))
    assert g.graph is graph0 and torch.equal(g(x), model(x)) and g.graph is graph0  # no update: no recapture
    CC.load_state(model, CC.second_state(fam))  # every tensor, in place
    got = g(x).clone()
    assert g.graph is not graph0
    assert torch.equal(got, model(x)), f"{fid}: the replay after an update is not the eager forward of the updated module"
    assert CC.same((got.cpu(),), fresh_outputs(fam)["forward"])
    graph1 = g.graph
    assert torch.equal(g(x), got) and g.graph is graph1
    bias = next(k for k in CC.float_keys(model) if k.endswith(".bias"))  # second update: one tensor the kernels read as an f32 copy
    CC.overwrite(model, bias, CC.SEED + 1)  # (the second checkpoint IS the draw of SEED + 1: take the one after it)
    got2 = g(x).clone()
    assert g.graph is not graph1 and torch.equal(got2, model(x)) and not torch.equal(got2, got)


def _decoders(kind):
    """(family, the module whose parameters the decoder reads, build(memory, prompt) -> decoder, decode(...) -> tokens)"""
    from pytorch_models.audio2text.generate import BeamDecoder, GreedyDecoder, beam_decode, greedy_decode

    n_new = 5
    if kind == "gpt2_greedy":
        return (CC.FAMILIES["gpt2"], lambda m: m, lambda dec, mem, p: GreedyDecoder(dec, None, p, n_new),
                lambda dec, mem, p: greedy_decode(dec, None, p, n_new))
    if kind == "whisper_greedy":
        return (CC.FAMILIES["whisper"], lambda m: m.decoder, lambda dec, mem, p: GreedyDecoder(dec, mem, p, n_new),
                lambda dec, mem, p: greedy_decode(dec, mem, p, n_new))
    return (CC.FAMILIES["whisper"], lambda m: m.decoder, lambda dec, mem, p: BeamDecoder(dec, mem, p, n_new, 2),
            lambda dec, mem, p: beam_decode(dec, mem, p, n_new, beams=2, return_beams=True)[0])


@pytest.mark.parametrize("kind", ["gpt2_greedy", "whisper_greedy", "whisper_beam"])
def test_held_decoders_refuse_a_changed_model(kind):
    fam, dec_of, build, decode = _decoders(kind)
    model, inp = hip_model(fam), on_dev(fam)
    dec = dec_of(model)
    prompt = inp["tok"][:, :3].contiguous()

    def memory():
        return model.encoder(inp["mel"].to(torch.bfloat16)) if "mel" in inp else None

    def tokens(st):
        st.run()
        return (st.beams()[0] if kind == "whisper_beam" else st.tokens).clone()

    st = build(dec, memory(), prompt)
    first = tokens(st)
    assert torch.equal(first, decode(dec, memory(), prompt))
    st.rebind(memory(), prompt)  # nothing changed: the captured step serves the next prompt
    assert torch.equal(tokens(st), first)
    CC.load_state(model, CC.second_state(fam))
    with pytest.raises(RuntimeError, match="parameters changed.*build a new decoder"):
        st.rebind(memory(), prompt)
    with pytest.raises(RuntimeError, match="parameters changed.*build a new decoder"):
        st.run()
    new = tokens(build(dec, memory(), prompt))
    assert torch.equal(new, decode(dec, memory(), prompt))
    fresh = hip_model(fam, CC.SEED + 1)
    fmem = fresh.encoder(inp["mel"].to(torch.bfloat16)) if "mel" in inp else None
    assert torch.equal(new, decode(dec_of(fresh), fmem, prompt))
