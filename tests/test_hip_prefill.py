"""GPU, end to end: the prompt pass of the KV-cached decoders (prefill=True) - caches and first logits against the fp32 oracle,
greedy / top-k / rules / beam ids of GPT-2 and Whisper, and the refusals that need a device.

Contract ("Prompt prefill"): the prompt pass rounds to bf16 where forward() does and keeps the stream in f32, so it
carries forward()'s contract - rel-L2 <= 2e-2 against the fp32 oracle on the same bf16-rounded weights (test_hip_text.py,
test_hip_blocks.py) - not the step path's fp32-exact projections.  Ids are therefore compared with the oracle's under the rule

    a sequence may first differ from the oracle at a position whose oracle top-2 margin is below tau,
    tau = 2 x the largest |model forward logit - oracle logit| over the compared positions (teacher-forced on the oracle's ids),

since a top-2 flip needs the two logits to move by at least the margin between them and the prompt pass rounds nowhere
forward() does not; at most ONE sequence per case may use the exception.  Seeds: GPT2(2, 128) fill_module seed 72 with
synth_tokens("prefill_tok", ., 2000, 91) and ("prefill_tok3", ., 2000, 92); the CPU emulation of the all-rounded oracle loop
(every named rounding point except the stream in bf16) needs the exception for no sequence on either: smallest oracle margins
0.013 / 0.049, largest logit perturbation 0.022 / 0.024."""
import pytest
import torch

from oracle import ref_text as RX
from oracle import ref_transformer as RT
from oracle import ref_whisper as RW
from oracle import ref_whisper_rules as RR
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def rel(got, want):
    got, want = got.float().cpu(), want.float()
    return ((got - want).norm() / want.norm()).item()


@pytest.fixture(scope="module")
def gpt2():
    from pytorch_models.text import GPT2

    m = GPT2(2, 128)
    fill_module(m, 72)
    bf16_round_(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(torch.bfloat16).cuda().eval(), sd


@pytest.fixture(scope="module")
def whisper():
    """(decoder, state dict, bf16 memory (2, 96, 384)) of Whisper tiny, seed 55"""
    from pytorch_models.audio2text import Whisper

    w = Whisper.from_openai("tiny").eval()
    fill_module(w, 55)
    bf16_round_(w)
    sd = {k: v.clone() for k, v in w.state_dict().items()}
    w = w.to(torch.bfloat16).cuda()
    memory = synth_input("prefill_memory", (2, 96, 384), 55).to(torch.bfloat16).cuda()
    return w.decoder, sd, memory


def _tau(model_logits, oracle_logits):
    return 2.0 * float((model_logits.float().cpu() - oracle_logits.float()).abs().max())


def _obeys(got, want, margin_at, P, tau, what):
    """the rule of the module docstring; margin_at(b, t) = the reference's top-2 margin where token t of sequence b was chosen.
    Returns how many sequences used the exception."""
    got = got.cpu()
    assert got.shape == want.shape and torch.equal(got[:, :P], want[:, :P]), f"{what}: the prompt must be kept"
    used = 0
    for b in range(got.shape[0]):
        diff = (got[b] != want[b]).nonzero()
        if len(diff):
            t = int(diff[0])
            m = float(margin_at(b, t))
            print(f"{what}: sequence {b} first differs at position {t}: got {int(got[b, t])} reference {int(want[b, t])} margin {m:.3e} tau {tau:.3e}")
            assert m < tau, f"{what}: sequence {b} differs at position {t} at a decisive margin ({m:.3e} >= tau {tau:.3e})"
            used += 1
    assert used <= 1, f"{what}: {used} sequences needed the near-tie exception"
    return used


# ------------------------------------------------------------------------------------------------ 1. caches and first logits
def test_gpt2_caches_and_first_logits_match_the_oracle(gpt2):
    from pytorch_models.audio2text.generate import BeamDecoder

    m, sd = gpt2
    tok = synth_tokens("prefill_tok", (2, 64), 2000, 91)
    P, H = 40, 2
    rec = {"k": [], "v": []}

    def hook(name, t):
        if name in rec:
            rec[name].append(t)
        return t

    want_logits = RX.gpt2(sd, tok[:, :P], rp=hook)[:, -1]
    want_k = [RT.split_heads(t, H) for t in rec["k"]]  # per layer (B, H, P, 64)
    want_v = [RT.split_heads(t, H) for t in rec["v"]]
    assert len(want_k) == 2

    def errors(**kw):
        st = BeamDecoder(m, None, tok[:, :P].cuda(), 1, 1, **kw)
        st.run()
        ek = max(rel(st.self_k[l][:, :, : P - 1], want_k[l][:, :, : P - 1]) for l in range(2))
        ev = max(rel(st.self_v[l][:, :, : P - 1], want_v[l][:, :, : P - 1]) for l in range(2))
        return st, max(ek, ev), rel(st.logits, want_logits)

    st0, kv0, lg0 = errors()
    print(f"prefill=False (yardstick, not asserted): K/V rel-L2 {kv0:.3e}, first logits rel-L2 {lg0:.3e}, steps {st0.n_steps}")
    assert st0.n_steps == P
    for kw in (dict(prefill=True), dict(prefill=True, prefill_chunk=16)):
        st, kv, lg = errors(**kw)
        print(f"{kw}: chunks {st._pre_chunks}: K/V rel-L2 {kv:.3e}, first logits rel-L2 {lg:.3e}")
        assert st.n_steps == 1
        assert kv <= 2e-2 and lg <= 2e-2
    assert st._pre_chunks == [(0, 16), (16, 16), (32, 7)]  # three chunks, the last ragged


# ------------------------------------------------------------------------------------------------ 2. ids, GPT-2
@pytest.mark.parametrize("name,seed,shape,P,n_new", [("prefill_tok", 91, (2, 64), 40, 16), ("prefill_tok3", 92, (3, 80), 67, 12)])
def test_gpt2_prefilled_ids_follow_the_oracle(gpt2, name, seed, shape, P, n_new):
    from pytorch_models.audio2text.generate import greedy_decode

    m, sd = gpt2
    prompt = synth_tokens(name, shape, 2000, seed)[:, :P]
    want, margins = RX.greedy(RX.gpt2, sd, prompt, n_new)
    # tau: the existing forward against the oracle, teacher-forced on the oracle's ids, at the positions that choose a new token
    tau = _tau(m(want[:, :-1].cuda())[:, P - 1 :], RX.gpt2(sd, want[:, :-1])[:, P - 1 :])
    print(f"tau = {tau:.3e}; smallest oracle margin {float(margins.min()):.3e}")
    margin_at = lambda b, t: margins[b, t - P]  # noqa: E731
    got = m.generate(prompt.cuda(), n_new, prefill=True)
    _obeys(got, want, margin_at, P, tau, "prefill")
    assert torch.equal(m.generate(prompt.cuda(), n_new, prefill=True, graph=False), got)  # eager == graph replay
    for chunk in (16, 25):  # other chunkings: the same rule against the oracle (bit equality between chunkings is not promised)
        _obeys(greedy_decode(m, None, prompt.cuda(), n_new, prefill=True, prefill_chunk=chunk), want, margin_at, P, tau, f"chunk {chunk}")
    if shape[0] == 3:  # rows are value-independent: a sequence alone decodes as it does inside the batch (same P, same chunking)
        for b in range(3):
            assert torch.equal(m.generate(prompt[b : b + 1].cuda(), n_new, prefill=True)[0], got[b]), b


# ------------------------------------------------------------------------------------------------ 3. Whisper
def _rules():
    from pytorch_models.audio2text.generate import WhisperRules

    kw = dict(eot=50257, timestamp_begin=50364, no_timestamps=50363, max_initial_timestamp=50, suppress=(1, 2, 7, 50258, 50259),
              blank=(220, 50257))
    return WhisperRules(**kw), RR.Rules(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})


def test_whisper_prefilled_greedy_rules_and_beams(whisper):
    dec, sd, memory = whisper
    P, n_new = 37, 12
    prompt = synth_tokens("prefill_wprompt", (2, P), 51865, 55)
    mem32 = memory.float().cpu()
    want, margins = RW.greedy_cached(sd, "decoder.", prompt, mem32, n_new)
    tau = _tau(dec(want[:, :-1].cuda(), memory)[:, P - 1 :], RW.decoder(sd, "decoder.", want[:, :-1], mem32)[:, P - 1 :])
    print(f"tau = {tau:.3e}; smallest oracle margin {float(margins.min()):.3e}")
    got = dec.generate(memory, prompt.cuda(), n_new, prefill=True)
    _obeys(got, want, lambda b, t: margins[b, t - P], P, tau, "whisper prefill")

    # under the rules (they act on positions >= P only): against the prefill=False ids; the margin at a first difference is
    # the top-2 gap of the decoder's own forward logits for that prefix after the oracle's rules (off from the step's by at most tau / 2)
    rules, oracle_rules = _rules()
    base = dec.generate(memory, prompt.cuda(), n_new, rules=rules).cpu()
    lg = dec(base[:, :-1].cuda(), memory).float().cpu()

    def ruled_margin(b, t):
        top2 = RR.apply(oracle_rules, lg[b, t - 1], base[b, P:t].tolist()).topk(2).values
        return top2[0] - top2[1]

    _obeys(dec.generate(memory, prompt.cuda(), n_new, rules=rules, prefill=True), base, ruled_margin, P, tau, "whisper prefill + rules")

    # beams: scores best first; the best hypothesis against the prefill=False beam run, the margin at a first difference being
    # the gap between the two runs' tokens in the decoder's own forward logits for the shared prefix
    b0, _ = dec.generate(memory, prompt.cuda(), n_new, beams=2, return_beams=True)
    b1, s1 = dec.generate(memory, prompt.cuda(), n_new, beams=2, return_beams=True, prefill=True)
    assert b1.shape == (2, 2, P + n_new) and bool((s1[:, 0] >= s1[:, 1]).all()) and bool(torch.isfinite(s1[:, 0]).all())
    best0, best1 = b0[:, 0].cpu(), b1[:, 0].cpu()
    lgb = dec(best0[:, :-1].cuda(), memory).float().cpu()
    _obeys(best1, best0, lambda b, t: (lgb[b, t - 1, best0[b, t]] - lgb[b, t - 1, best1[b, t]]).abs(), P, tau, "whisper prefill + beams")


# ------------------------------------------------------------------------------------------------ 4. top-k
def test_gpt2_prefilled_topk_sampling_stays_inside_the_oracle_top_k(gpt2):
    """as test_hip_text.py::test_gpt2_topk_sampling_stays_inside_the_oracle_top_k does for the step path, with the prompt
    prefilled: repeatable for a seed, every drawn id one of the oracle's five most likely continuations (near-ties excepted)"""
    m, sd = gpt2
    P, n_new, k = 40, 16, 5
    prompt = synth_tokens("prefill_tok", (2, 64), 2000, 91)[:, :P]
    a = m.generate(prompt.cuda(), n_new, topk=k, seed=3, prefill=True).cpu()
    assert torch.equal(m.generate(prompt.cuda(), n_new, topk=k, seed=3, prefill=True).cpu(), a) and torch.equal(a[:, :P], prompt)
    lg = RX.gpt2(sd, a[:, :-1])
    tau = _tau(m(a[:, :-1].cuda())[:, P - 1 :], lg[:, P - 1 :])
    for b in range(2):
        for t in range(P, P + n_new):
            row = lg[b, t - 1]
            assert row[a[b, t]] >= row.topk(k).values[-1] - tau, (b, t)


# ------------------------------------------------------------------------------------------------ 5. refusals on the device
def test_refusals_and_the_one_token_prompt(gpt2, whisper):
    from pytorch_models.audio2text.generate import greedy_decode

    m, _ = gpt2
    dec, _, memory = whisper
    prompt = synth_tokens("prefill_tok", (2, 64), 2000, 91)[:, :8].cuda()
    with pytest.raises(NotImplementedError, match="persistent"):
        greedy_decode(m, None, prompt, 4, path="persistent", prefill=True)
    with pytest.raises(NotImplementedError, match="kv32"):
        greedy_decode(dec, memory.float(), prompt, 4, kv32=True, prefill=True)
    one = prompt[:, :1]
    assert torch.equal(m.generate(one, 6, prefill=True), m.generate(one, 6))  # nothing to prefill: the plain run, exactly
