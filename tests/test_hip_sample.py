"""GPU, end to end: temperature / top-p / whole-vocabulary sampling and token log-probs through the KV-cached decoders (DESIGN.md
section 27), on GPT2(2, 128) and Whisper tiny with the peaked weights of tests/sample_cases.py.

  defaults     passing the defaults explicitly gives the bits of passing nothing, and the launch list holds no pm_dec_sample;
  seeds        the same seed twice: the same tokens and log-probs, bit for bit; another seed differs somewhere;
  graph/eager  bit for bit;
  arg-max      temperature=0 through the new tail equals the plain greedy run wherever that run's top-2 margin exceeds 2e-5 (the two
               logits kernels agree to 1e-5 per value: ADVICE.md's logits note); at most 5 % of the positions may use the exception
               (the oracle's own smallest margin is 0.21: tests/test_sample_cases_cpu.py);
  log-probs    against float64 log_softmax of the K/V-rounded oracle's logits, gathered at the produced tokens: LP_TOL;
  sampled run  at every new position the oracle's distribution for the PRODUCED prefix: the token lies in the reference nucleus (up to
               LP_TOL at tau) and equals the reference pick wherever the reference's edge distances exceed 1e-3; at most 10 % of the
               positions may be unclear (the seeds are chosen on the CPU: the reference alone has none);
  combinations prefill=True and lengths=; rebind(); every refusal.

LP_TOL: the score tests hold score() to a bound derived from its own hidden rows; the step has no such rows to offer, so the figure
is 4 x the worst |log-prob - oracle| measured over these runs: 2.918e-2 -> 1.2e-1 (profiles/sampling/README.md).  That distance is the
STEP's, not the tail's: the peaked weights multiply every logit, and its error against the oracle, by 8, and
test_logprob_is_exact_on_the_steps_own_logits holds the tail to 1e-5 on the logits the step actually produced."""
import copy

import pytest
import torch

import sample_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LP_TOL = 1.2e-1  # 4 x the measured worst case (2.918e-2), see the module docstring
PAD = 7
N = 8


@pytest.fixture(scope="module")
def gpt2():
    m, sd, prompt = S.gpt2_setup()
    return copy.deepcopy(m).to(torch.bfloat16).cuda().eval(), sd, prompt


@pytest.fixture(scope="module")
def whisper():
    from pytorch_models.audio2text.generate import WhisperRules

    w, sd, memory, prompt = S.whisper_setup()
    w = copy.deepcopy(w).to(torch.bfloat16).cuda().eval()
    return w, sd, memory, memory.to(torch.bfloat16).cuda(), prompt, WhisperRules(**S.WHISPER_RULES)


def _names(st):
    return [fn.__name__ for fn, _ in st.launches]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _oracle_lp(logits, toks, P):
    """float64 log-probabilities of toks[:, P:] under (B, L - 1, V) teacher-forced logits of toks[:, :-1]"""
    lsm = torch.log_softmax(logits[:, P - 1 :].double(), -1)
    return lsm.gather(2, toks[:, P:, None])[..., 0]


def _check_sampled(what, toks, lps, logits, run, P, t0, rows=None):
    """toks (B, P + n) produced, logits (B, L - 1, V) the oracle's for that prefix (after its rules); cache position of new token i
    is t0 + i.  Asserts nucleus membership, equality where clear, the cap and the log-probs; returns the worst log-prob error."""
    B, n = toks.shape[0], toks.shape[1] - P
    unclear, worst = 0, 0.0
    for b in range(B):
        for i in range(n):
            l = logits[b, P - 1 + i]
            rr, want, edge = S.position_reference(l, run, t0 + i, b if rows is None else rows[b])
            tok = int(toks[b, P + i])
            assert float(l[tok]) >= rr.tau - LP_TOL, f"{what}: row {b} token {i} = {tok} lies outside the reference nucleus"
            assert float(l[tok]) > -float("inf"), f"{what}: row {b} token {i}: a token the rules forbid"
            if edge > S.DRAW_MARGIN:
                assert tok == want, f"{what}: row {b} token {i}: got {tok}, reference {want} at edge distance {edge:.3e}"
            else:
                unclear += 1
    lp_want = _oracle_lp(logits, toks, P)
    worst = float((lps.double().cpu() - lp_want).abs().max())
    print(f"{what}: {unclear} of {B * n} positions unclear (cap {S.EDGE_CAP:.0%}); worst |log-prob - oracle| {worst:.3e} (LP_TOL {LP_TOL:.1e})")
    assert worst <= LP_TOL
    if rows is None:
        assert unclear <= S.EDGE_CAP * B * n
    return unclear


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_defaults_build_the_launch_list_they_always_built(gpt2, whisper):
    from pytorch_models.audio2text.generate import GreedyDecoder

    m, _, prompt = gpt2
    p = prompt.cuda()
    explicit = dict(topk=1, seed=0, temperature=1.0, top_p=1.0, return_logprobs=False)
    assert _same(m.generate(p, N), m.generate(p, N, **explicit))
    assert _same(m.generate(p, N, topk=4, seed=3), m.generate(p, N, **{**explicit, "topk": 4, "seed": 3}))
    for kw, tail in ((dict(), "pm_dec_next_token"), (dict(topk=4), "pm_dec_sample_topk"), (dict(lengths=(23, 9, 1)), "pm_dec_next_token_ragged")):
        names = _names(GreedyDecoder(m, None, p, N, **kw, temperature=1.0, top_p=1.0, return_logprobs=False))
        assert names == _names(GreedyDecoder(m, None, p, N, **kw)) and names[-1] == tail
        assert "pm_dec_sample" not in names and "pm_dec_sample_ragged" not in names
    names = _names(GreedyDecoder(m, None, p, N, return_logprobs=True))
    assert names[-1] == "pm_dec_sample" and names.count("pm_dec_sample") == 1 and "pm_dec_next_token" not in names
    assert _names(GreedyDecoder(m, None, p, N, lengths=(23, 9, 1), top_p=0.5))[-1] == "pm_dec_sample_ragged"
    w, _, _, mem, wp, rules = whisper
    wp = wp.cuda()
    assert _same(w.decoder.generate(mem, wp, N, rules=rules), w.decoder.generate(mem, wp, N, rules=rules, **explicit))
    assert _same(w.decoder.generate(mem, wp, N), w.decoder.generate(mem, wp, N, **explicit))


# ----------------------------------------------------------------------------------------------------- seeds, graph and eager
def test_seeds_and_graph_replay(gpt2):
    m, _, prompt = gpt2
    p = prompt.cuda()
    kw = dict(topk=0, temperature=0.7, top_p=0.9, return_logprobs=True)
    a, la = m.generate(p, N, seed=11, **kw)
    b, lb = m.generate(p, N, seed=11, **kw)
    assert a.shape == (3, 23 + N) and la.shape == (3, N) and la.dtype == torch.float32 and bool((la <= 0).all())
    assert _same(a, b) and _same(la, lb)
    c, lc = m.generate(p, N, seed=12, **kw)
    assert not torch.equal(a, c), "another seed must differ somewhere"
    e, le = m.generate(p, N, seed=11, graph=False, **kw)
    assert _same(a, e) and _same(la, le), "graph replay and eager launches differ"
    assert _same(m.generate(p, N, seed=11, **{**kw, "return_logprobs": False}), a)  # the log-prob buffer does not move a token


# ------------------------------------------------------------------------------------------------------------ the arg-max tail
def test_temperature_zero_is_the_greedy_run_with_logprobs(gpt2, whisper):
    from pytorch_models.audio2text.generate import greedy_decode
    from oracle import ref_text as RX

    m, sd, prompt = gpt2
    w, wsd, memory, mem, wp, _ = whisper
    skipped = total = 0
    for what, dec, memo, p, logits_of in (
            ("gpt2", m, None, prompt, lambda t: RX.gpt2(sd, t, rp=S.kv_round)),
            ("whisper", w.decoder, mem, wp, lambda t: S.whisper_logits(wsd, memory, t, wp.shape[1], False))):
        P = p.shape[1]
        plain, marg = greedy_decode(dec, memo, p.cuda(), N, margins=True)
        got, lp = greedy_decode(dec, memo, p.cuda(), N, temperature=0.0, return_logprobs=True)
        # topk and top_p are ignored at temperature 0
        assert _same(greedy_decode(dec, memo, p.cuda(), N, temperature=0.0, topk=50, top_p=0.5, seed=9), got)
        for b in range(p.shape[0]):
            diff = (got[b] != plain[b]).nonzero()
            total += N
            if len(diff):
                t = int(diff[0])
                assert t >= P and float(marg[b, t]) <= 2e-5, f"{what}: row {b} differs at {t} at margin {float(marg[b, t]):.3e}"
                skipped += P + N - t
        toks = got.cpu()
        worst = float((lp.double().cpu() - _oracle_lp(logits_of(toks[:, :-1]), toks, P)).abs().max())
        print(f"{what}: temperature 0: worst |log-prob - oracle| {worst:.3e} (LP_TOL {LP_TOL:.1e})")
        assert worst <= LP_TOL
    print(f"arg-max tail: {skipped} of {total} positions behind a near-tie (cap 5 %)")
    assert skipped <= 0.05 * total


def test_logprob_is_exact_on_the_steps_own_logits(gpt2):
    """the last step's logits stay in the decoder: the log-prob of the last token is float64 log_softmax of THOSE within 1e-5 (the
    kernel tests derive the bound; here |lse| ~ 30), and their distance to the oracle's logits is printed"""
    from oracle import ref_text as RX
    from pytorch_models.audio2text.generate import GreedyDecoder

    m, sd, prompt = gpt2
    st = GreedyDecoder(m, None, prompt.cuda(), N, topk=0, temperature=0.7, top_p=0.9, seed=11, return_logprobs=True)
    st.run()
    toks, lp = st.output()[0].cpu(), st.output_logprobs().cpu()
    own = torch.log_softmax(st.logits.double().cpu(), -1).gather(1, toks[:, -1:])[:, 0]
    err = float((lp[:, -1].double() - own).abs().max())
    far = float((st.logits.float().cpu() - RX.gpt2(sd, toks[:, :-1], rp=S.kv_round)[:, -1]).abs().max())
    print(f"last step: |log-prob - float64 log_softmax of the step's logits| {err:.3e}; |step logits - oracle logits| {far:.3e}")
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------------------- the sampled runs
def test_gpt2_sampled_run_follows_the_reference(gpt2):
    from oracle import ref_text as RX

    m, sd, prompt = gpt2
    run, P = S.GPT2_RUN, prompt.shape[1]
    kw = dict(topk=run["topk"], temperature=run["temperature"], top_p=run["top_p"], seed=run["seed"], return_logprobs=True)
    toks, lps = m.generate(prompt.cuda(), run["n_new"], **kw)
    toks = toks.cpu()
    _check_sampled("gpt2 sampled", toks, lps, RX.gpt2(sd, toks[:, :-1], rp=S.kv_round), run, P, P - 1)
    # prefill: the prompt pass rounds where forward() does; a first difference from the step run only where the reference's edge
    # is closer than the mass those logit differences can move: 2 x max |forward - oracle| / temperature
    pre, lpre = m.generate(prompt.cuda(), run["n_new"], prefill=True, **kw)
    pre = pre.cpu()
    logits = RX.gpt2(sd, toks[:, :-1], rp=S.kv_round)
    tau = 2.0 * float((m(toks[:, :-1].cuda())[:, P - 1 :].float().cpu() - logits[:, P - 1 :]).abs().max()) / run["temperature"]
    print(f"gpt2 prefill: tau = {tau:.3e}")
    for b in range(3):
        diff = (pre[b] != toks[b]).nonzero()
        if len(diff):
            t = int(diff[0])
            edge = S.position_reference(logits[b, t - 1], run, t - 1, b)[2]
            assert t >= P and edge < tau, f"prefill: row {b} differs at {t} at edge distance {edge:.3e} >= tau {tau:.3e}"
        else:
            assert float((lpre[b] - lps[b]).abs().max()) <= tau * run["temperature"]


def test_whisper_sampled_run_with_rules_follows_the_reference(whisper):
    w, sd, memory, mem, wp, rules = whisper
    run, P = S.WHISPER_RUN, wp.shape[1]
    kw = dict(topk=run["topk"], temperature=run["temperature"], top_p=run["top_p"], seed=run["seed"], return_logprobs=True, rules=rules)
    toks, lps = w.decoder.generate(mem, wp.cuda(), run["n_new"], **kw)
    toks = toks.cpu()
    _check_sampled("whisper sampled, rules", toks, lps, S.whisper_logits(sd, memory, toks[:, :-1], P, True), run, P, P - 1)
    # Whisper.generate passes everything through (the encoder's output is another memory: only the plumbing is checked)
    mel = torch.zeros(2, 80, 200, device="cuda")
    a = w.generate(mel, wp.cuda(), 4, **kw)
    assert isinstance(a, tuple) and a[0].shape == (2, P + 4) and a[1].shape == (2, 4) and _same(a[0], w.generate(mel, wp.cuda(), 4, **kw)[0])


# --------------------------------------------------------------------------------------------------------- ragged, rebind, text
def test_ragged_rows_follow_their_own_oracle(gpt2):
    from oracle import ref_text as RX

    m, sd, prompt = gpt2
    run, lens, Pm = S.GPT2_RUN, S.RAGGED_LENGTHS, max(S.RAGGED_LENGTHS)
    kw = dict(topk=run["topk"], temperature=run["temperature"], top_p=run["top_p"], seed=run["seed"], return_logprobs=True)
    n = run["n_new"]
    got, lps = m.generate(prompt.cuda(), n, lengths=lens, pad_token_id=PAD, **kw)
    got = got.cpu()
    assert got.shape == (3, 23 + n) and lps.shape == (3, n)
    unclear = 0
    for b, ln in enumerate(lens):  # output()'s rule: the prompt, the new ids, then pad ids; the log-probs in the caller's row order
        assert torch.equal(got[b, :ln], prompt[b, :ln]) and bool((got[b, ln + n :] == PAD).all())
        row = got[b : b + 1, : ln + n]
        # the draw is keyed by the CACHE position: the new token i of every row sits at Pm + i
        unclear += _check_sampled(f"ragged row {b}", row, lps[b : b + 1], RX.gpt2(sd, row[:, :-1], rp=S.kv_round), run, ln, Pm - 1, rows=[b])
    assert unclear <= S.EDGE_CAP * 3 * n
    pre, lpre = m.generate(prompt.cuda(), n, lengths=lens, pad_token_id=PAD, prefill=True, **kw)
    assert pre.shape == got.shape and lpre.shape == lps.shape and bool((lpre <= 0).all())


def test_rebind_then_run_keeps_the_graph_and_the_logprobs(gpt2):
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode
    from synthweights import synth_tokens

    m, _, prompt = gpt2
    kw = dict(topk=0, temperature=0.7, top_p=0.9, seed=11, return_logprobs=True)
    st = GreedyDecoder(m, None, prompt.cuda(), N, **kw)
    st.run()
    first, lp1 = st.output()[0].clone(), st.output_logprobs()
    graph = st._graph
    want, lpw = greedy_decode(m, None, prompt.cuda(), N, **kw)
    assert graph is not None and _same(first, want) and _same(lp1, lpw)
    other = synth_tokens("sample_rebind", tuple(prompt.shape), 2000, 5)
    st.rebind(None, other.cuda())
    st.run()
    want, lpw = greedy_decode(m, None, other.cuda(), N, **kw)
    assert st._graph is graph and _same(st.output()[0], want) and _same(st.output_logprobs(), lpw)
    with pytest.raises(ValueError, match="return_logprobs"):
        GreedyDecoder(m, None, prompt.cuda(), N).output_logprobs()


def test_decoder_generator_passes_temperature_and_top_p(gpt2):
    from pytorch_models.text.generator import DecoderGenerator

    m, _, prompt = gpt2
    gen = DecoderGenerator(m, None)
    ids = prompt[0].tolist()
    want = m.generate(prompt[:1].cuda(), N, topk=0, seed=4, temperature=0.7, top_p=0.9)[0].tolist()
    assert gen.generate_ids(ids, N, 0, seed=4, temperature=0.7, top_p=0.9) == want
    assert gen.generate_ids(ids, N) == m.generate(prompt[:1].cuda(), N)[0].tolist()
    batch = gen.generate_ids_batch([ids, ids[:5]], N, 0, seed=4, temperature=0.7, top_p=0.9)
    assert [len(r) for r in batch] == [23 + N, 5 + N] and batch[0][:23] == ids
    with pytest.raises(ValueError):
        gen.generate_ids(ids, N, temperature=-1.0)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal(gpt2, whisper):
    from pytorch_models.audio2text.generate import greedy_decode

    m, _, prompt = gpt2
    w, _, _, mem, wp, rules = whisper
    p, wp = prompt.cuda(), wp.cuda()
    mel = torch.zeros(2, 80, 200, device="cuda")
    for bad in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=1.01),
                dict(topk=65), dict(topk=-1)):
        with pytest.raises(ValueError):
            m.generate(p, 2, **bad)
        with pytest.raises(ValueError):
            w.decoder.generate(mem, wp, 2, **bad)
    for call in (lambda: m.generate(p, 2, beams=2, temperature=0.5), lambda: m.generate(p, 2, beams=2, return_beams=True, return_logprobs=True),
                 lambda: w.decoder.generate(mem, wp, 2, beams=2, top_p=0.5), lambda: w.generate(mel, wp, 2, beams=2, topk=0),
                 lambda: greedy_decode(m, None, p, 2, margins=True, top_p=0.5), lambda: greedy_decode(m, None, p, 2, margins=True, return_logprobs=True)):
        with pytest.raises(ValueError, match="beams=1|return_logprobs=True"):
            call()
    for call in (lambda: m.generate(p, 2, path="persistent", temperature=0.5), lambda: w.decoder.generate(mem, wp, 2, path="persistent", topk=0),
                 lambda: w.generate(mel, wp, 2, exact=True, temperature=0.5), lambda: w.generate(mel, wp, 2, exact=True, return_logprobs=True),
                 lambda: greedy_decode(w.decoder, mem.float(), wp, 2, kv32=True, top_p=0.5),
                 lambda: copy.deepcopy(m).float().generate(p, 2, return_logprobs=True),
                 lambda: copy.deepcopy(w).float().decoder.generate(mem.float(), wp, 2, temperature=0.5)):
        with pytest.raises(NotImplementedError, match="launches|exact=False|bfloat16"):
            call()
