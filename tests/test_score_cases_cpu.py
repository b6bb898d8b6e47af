"""CPU: the sequence-scoring contract without a GPU (tests/score_cases.py) - the stand-in inside 1.0 x the derived bounds on every
case, every mutant caught, the arg-max cap, the ABI of pm_lm_score_bf16 / pm_lm_score_ws_bytes and their host-side refusals, the
``score`` methods, and Whisper.score's CPU form against its own forward."""
import ctypes
import functools

import pytest
import torch

import score_cases as sc
from pytorch_models import _hip

CASES = sc.cases()


@functools.lru_cache(maxsize=None)
def _data(i: int):
    case = CASES[i]
    h, w, t = sc.build(case)
    return case, h, w, t, sc.reference(h, w, t)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_standin_inside_the_bound(i):
    case, h, w, t, ref = _data(i)
    v = sc.judge(case, ref, *sc.standin(h, w, t))
    print(f"{case.id}: logprob {v.r_lp:.3f} lse {v.r_lse:.3f} of the bound")
    assert v.passed(1.0), v


def test_case_list_reaches_every_edge():
    Ms, Vs, Ks = ({getattr(c, a) for c in CASES if c.family == "gauss"} for a in "MVK")
    assert {1, 127, 129, 300} <= Ms and {8, 64, 72, 200, 768} <= Ks
    assert {1, 127, 128, 129, sc.NC - 1, sc.NC, sc.NC + 1, 2 * sc.NC + 37, 50257} <= Vs
    assert {c.family for c in CASES} == {"gauss", "edges", "peaked", "offset", "flat", "ties"}
    assert {c.family for c in sc.gpu_only_cases()} == {"poison", "perm"}


def test_families_are_what_they_claim():
    for i, case in enumerate(CASES):
        if case.V > 10000 and case.family not in ("peaked", "flat"):
            continue
        _, h, w, t, ref = _data(i)
        if case.family == "edges":
            assert int((t == -1).sum()) == case.M // 4 and (ref.logprob[t == -1] == 0).all()
            if case.M >= 64:
                assert set(sc._edge_columns(case.V)) <= set(t.tolist())
        elif case.family == "peaked":
            top = ref.x.topk(2, -1).values
            assert (top[:, 0] - top[:, 1] > 20).all() and (ref.logprob < -20).all()
            assert ((ref.argmax // sc.NC) != (t // sc.NC)).all()  # the peak sits in another chunk than the target
            if case.M >= 4:
                assert {0, sc.NC - 1, (case.V - 1) // sc.NC * sc.NC, case.V - 1} <= set(ref.argmax.tolist())
        elif case.family == "offset":
            assert (ref.x.abs().min(-1).values > 150).all() and ((ref.x.max(-1).values - ref.x.min(-1).values) < 60).all()
        elif case.family == "flat":
            assert (ref.x == 0).all() and (ref.delta == 0).all()
        elif case.family == "ties":
            assert torch.equal(ref.argmax, case.want_argmax)  # the duplicate is the maximum and the lower index is expected
            assert (ref.gap == 0).all()
            assert torch.equal(w[sc.TILE], w[sc.TILE - 1]) and torch.equal(w[sc.NC], w[sc.NC - 1])


def test_gauss_rows_fall_under_the_exact_argmax_rule():
    for i, case in enumerate(CASES):
        if case.family in sc.GAUSS_FAMILIES and case.V > 1:
            ref = _data(i)[4]
            frac = float(sc.exact_rows(ref).double().mean())
            assert frac >= 0.9 or case.M < 10 and frac * case.M >= case.M - 1, (case.id, frac)


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for i, case in enumerate(CASES):
        if case.V > 10000 or case.K > 200:  # the small cases are enough to catch every mutant
            continue
        _, h, w, t, ref = _data(i)
        if not sc.judge(case, ref, *sc.standin(h, w, t, mutant)).passed(sc.MARGIN):
            caught.append(case.id)
    print(mutant, "caught by", len(caught), "cases:", caught[:4])
    assert caught, f"no case catches the mutant {mutant}"


def test_entry_points_declared_with_signatures():
    declared = _hip.header_functions()
    for name in ("pm_lm_score_bf16", "pm_lm_score_ws_bytes"):
        assert name in declared and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["pm_lm_score_bf16"][0]) == 13 and _hip.SIGNATURES["pm_lm_score_ws_bytes"][1] is ctypes.c_int64


def test_workspace_size_and_chunk_constant():
    L = _hip.lib()  # loadable without a GPU
    for M, V in ((1, 1), (7, sc.NC), (7, sc.NC + 1), (300, 50257), (32768, 50257)):
        n = L.pm_lm_score_ws_bytes(M, V)
        assert 0 < n <= 32 * M * sc.nchunks(V), (M, V, n)
    # the helper's NC is the build's: one more column than a chunk costs one more partial per row
    assert L.pm_lm_score_ws_bytes(1, sc.NC + 1) == 2 * L.pm_lm_score_ws_bytes(1, sc.NC)
    assert L.pm_lm_score_ws_bytes(1, sc.NC) == L.pm_lm_score_ws_bytes(1, 1)
    assert L.pm_lm_score_ws_bytes(32768, 50257) < 64 << 20


def test_host_side_refusals_launch_nothing():
    """Rejected calls return their code before any HIP call, so this is safe without a GPU."""
    L = _hip.lib()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    ok = dict(h=p, ldh=64, w=p, ldw=64, t=p, lp=p, lse=None, am=None, ws=p, M=4, V=8, K=64)

    def call(**kw):
        a = {**ok, **kw}
        return L.pm_lm_score_bf16(a["h"], a["ldh"], a["w"], a["ldw"], a["t"], a["lp"], a["lse"], a["am"], a["ws"], a["M"], a["V"], a["K"], None)

    for name in ("h", "w", "t", "lp", "ws"):
        assert call(**{name: None}) == 1, name  # PM_EINVAL
    assert call(V=0) == 1 and call(K=0) == 1
    assert call(K=68, ldh=72, ldw=72) == 2  # K not a multiple of 8: PM_EUNSUPPORTED
    assert call(ldh=65) == 4 and call(ldw=68) == 4  # PM_EALIGN
    assert call(h=p + 8) == 4 and call(w=p + 2) == 4
    assert call(ldh=56) == 1  # a row stride below K


def test_score_methods_exist():
    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from pytorch_models.text import GPT, GPT2, T5Model

    for cls in (GPT2, GPT, WhisperDecoder, Whisper, T5Model):
        assert hasattr(cls, "score"), cls


def test_whisper_score_on_the_cpu_is_log_softmax_of_forward():
    from synthweights import synth_input, synth_tokens

    m = sc.small_whisper()
    mel = synth_input("score_mel", (2, 80, 100), 3)
    tokens = synth_tokens("score_tokens", (2, 7), 1000, 3)
    lengths = torch.tensor([7, 4])
    with torch.no_grad():
        logits = m(mel, tokens)
    got, am = m.score(mel, tokens, lengths, return_argmax=True)
    want = torch.log_softmax(logits[:, :-1].double(), -1).gather(-1, tokens[:, 1:, None])[..., 0]
    keep = torch.arange(1, 7)[None, :] < lengths[:, None]
    assert got.shape == (2, 6) and got.dtype == torch.float32
    assert (got[~keep] == 0).all()
    assert float((got.double() - want)[keep].abs().max()) < 1e-5
    assert torch.equal(am, logits[:, :-1].argmax(-1))
    assert torch.equal(m.score(mel, tokens), m.decoder.score(tokens, m.encoder(mel)))


def test_score_refuses_what_forward_refuses():
    m = sc.small_gpt2()
    tokens = torch.zeros((1, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError):  # a CPU model: the device error, as forward raises it
        m.score(tokens)
    with pytest.raises(RuntimeError):
        m(tokens)
    with pytest.raises(RuntimeError):
        sc.small_t5().score(tokens, tokens)
