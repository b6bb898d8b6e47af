"""GPU, end to end: eos stopping and the repetition controls through the KV-cached decoders, on GPT2(2, 128) and
Whisper tiny with the peaked weights of tests/sample_cases.py and the prompts, eos ids and settings tests/control_cases.py chose on
the CPU; N = 12 new tokens.

  defaults     passing every default explicitly gives the bits and the launch-name list of passing nothing (arg-max, top-k, ragged and
               sampling tails): no pm_dec_controls, no pm_dec_finish;
  eos          tokens (and margins, log-probs) up to and including each row's eos EQUAL the run without eos_token_id bit for bit, then
               pad ids and exactly 0.0; n_new is the reference's (control_cases.cut_at_eos of the uncut run); logprobs.sum(-1) equals
               the uncut run's sum over the same positions - on the default tail with margins, top-k, the sampling tail, prefill=True,
               lengths=, rules=; an eos inside the prompt finishes nothing;
  early exit   POLL_EVERY patched to 1 and above N: the same bits, steps_run < n_steps in the first; rebind() starts unfinished;
  no-repeat    the produced rows hold no repeated n-gram, prompt included, where the plain run on the same prompt does;
  oracle       for the PRODUCED prefix the oracle's logits go through the reference controls and rules: the token equals the lowest-index
               arg-max wherever the reference's top-2 margin exceeds 2 max(r, 1 / r) LP_TOL; at most EDGE_CAP of the positions may be
               left out (tests/test_control_cases_cpu.py shows the reference alone inside the cap); the sampled run by
               test_hip_sample._check_sampled's logic on the controlled logits;
  graph/eager  bit for bit, and two identical calls are bit-identical;
  refusals     every one of DESIGN.md section 31's table."""
import copy

import pytest
import torch

import control_cases as C
import sample_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
N, PAD = C.N, C.PAD
DEFAULTS = dict(eos_token_id=None, pad_token_id=0, return_lengths=False, min_new_tokens=0, repetition_penalty=1.0, no_repeat_ngram_size=0)


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
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_defaults_build_the_launch_list_they_always_built(gpt2, whisper):
    from pytorch_models.audio2text.generate import GreedyDecoder

    m, _, prompt = gpt2
    p = prompt.cuda()
    dec_defaults = dict(eos=None, pad_token_id=0, min_new_tokens=0, repetition_penalty=1.0, no_repeat_ngram_size=0)
    new = ("pm_dec_controls", "pm_dec_finish")
    for kw, tail in ((dict(), "pm_dec_next_token"), (dict(topk=4, seed=3), "pm_dec_sample_topk"), (dict(lengths=(23, 9, 1)), "pm_dec_next_token_ragged"),
                     (dict(topk=0, temperature=0.7, top_p=0.9, seed=11, return_logprobs=True), "pm_dec_sample")):
        assert _same(m.generate(p, N, **kw), m.generate(p, N, **kw, **DEFAULTS)), kw
        build = {k: v for k, v in kw.items()}
        names = _names(GreedyDecoder(m, None, p, N, **build, **dec_defaults))
        assert names == _names(GreedyDecoder(m, None, p, N, **build)) and names[-1] == tail and not set(new) & set(names), kw
        # the eos alone: the same list with the finish launch behind it; a control: the full-logits route with one pm_dec_controls
        with_eos = _names(GreedyDecoder(m, None, p, N, **build, eos=5))
        assert with_eos == names + ["pm_dec_finish"], kw
        ctl = _names(GreedyDecoder(m, None, p, N, **build, no_repeat_ngram_size=2))
        assert ctl.count("pm_dec_controls") == 1 and "pm_dec_finish" not in ctl and "pm_dec_next_token" not in ctl, kw
    assert _names(GreedyDecoder(m, None, p, N, repetition_penalty=1.3))[-1] == "pm_dec_sample_topk"  # k = 1: the arg-max
    w, _, _, mem, wp, rules = whisper
    wp = wp.cuda()
    assert _same(w.decoder.generate(mem, wp, N, rules=rules), w.decoder.generate(mem, wp, N, rules=rules, **DEFAULTS))
    assert _same(w.decoder.generate(mem, wp, N), w.decoder.generate(mem, wp, N, **DEFAULTS))
    names = _names(GreedyDecoder(w.decoder, mem, wp, N, rules=rules, eos=5, min_new_tokens=2, repetition_penalty=1.3))
    assert names[-4:] == ["pm_dec_linear", "pm_dec_controls", "pm_dec_whisper_rules", "pm_dec_sample_topk", "pm_dec_finish"][-4:]
    assert names.index("pm_dec_controls") == names.index("pm_dec_whisper_rules") - 1  # the rules come after: their -inf wins


# ----------------------------------------------------------------------------------------------------------------------- eos
def _split(res, lp, marg):
    """(tokens, log-probs or margins or None, n_new or None) of a result tuple"""
    if not isinstance(res, tuple):
        return res, None, None
    res = list(res)
    toks = res.pop(0)
    aux = res.pop(0) if (lp or marg) else None
    return toks, aux, (res.pop(0) if res else None)


def _check_eos(what, run, eos, Ps, *, lp=False, marg=False, must_finish=True):
    """run(**kw) -> the decoder's result; Ps[b] = the width of row b's real prompt (its new ids follow at once).  Returns n_new."""
    uncut, aux0, none = _split(run(), lp, marg)
    got, aux, n_new = _split(run(eos_token_id=eos, pad_token_id=PAD, return_lengths=True), lp, marg)
    assert none is None and n_new.dtype == torch.int64 and n_new.shape == (uncut.shape[0],) and got.shape == uncut.shape
    uncut, got, n_new = uncut.cpu(), got.cpu(), n_new.cpu().tolist()
    for b, P in enumerate(Ps):
        want, k = C.cut_at_eos(uncut[b, P : P + N].tolist(), eos, PAD)
        assert got[b, :P].tolist() == uncut[b, :P].tolist() and got[b, P : P + N].tolist() == want, f"{what}: row {b}: {got[b, P:P + N].tolist()} != {want}"
        assert n_new[b] == k, f"{what}: row {b}: n_new {n_new[b]}, reference {k}"
        if aux is not None:
            a, a0 = aux[b].cpu(), aux0[b].cpu()
            a, a0 = (a, a0) if lp else (a[P : P + N], a0[P : P + N])
            assert _same(a[:k], a0[:k]) and bool((a[k:] == 0).all()), f"{what}: row {b}: {'log-probs' if lp else 'margins'}"
    if lp:
        keep = torch.arange(N)[None, :] < torch.tensor(n_new)[:, None]
        assert _same(aux.cpu().sum(-1), torch.where(keep, aux0.cpu(), torch.zeros(())).sum(-1)), f"{what}: logprobs.sum(-1)"
    print(f"{what}: eos {eos}: n_new {n_new}")
    if must_finish:
        assert min(n_new) < N, f"{what}: no row finished: the test does not bite"
    return n_new


def _own_eos(run, Ps, lp=False, marg=False):
    """an eos that the variant's OWN uncut run emits (its draws differ from the oracle's greedy run): control_cases.pick_eos, else
    the third new token of row 0"""
    toks = _split(run(), lp, marg)[0].cpu()
    rows = [toks[b, P : P + N].tolist() for b, P in enumerate(Ps)]
    return C.pick_eos(rows) or rows[0][2]


def test_eos_on_gpt2_every_tail(gpt2):
    from pytorch_models.audio2text.generate import greedy_decode

    m, _, prompt = gpt2
    p = prompt[list(C.GPT2_EOS_ROWS)].cuda()
    eos, Ps = C.gpt2_eos(), [23, 23]
    # the default tail, with margins: the oracle's eos finishes both rows, at different positions
    n_new = _check_eos("default tail + margins", lambda **kw: greedy_decode(m, None, p, N, margins=True, **kw), eos, Ps, marg=True)
    assert len(set(n_new)) == 2 and max(n_new) < N
    _check_eos("default tail", lambda **kw: m.generate(p, N, **kw), eos, Ps)
    _check_eos("prefill", lambda **kw: m.generate(p, N, prefill=True, **kw), eos, Ps)
    for what, base in (("top-k", dict(topk=4, seed=3)), ("sampling tail", dict(topk=0, temperature=0.7, top_p=0.9, seed=11, return_logprobs=True)),
                       ("arg-max + log-probs", dict(return_logprobs=True)), ("controls", dict(no_repeat_ngram_size=2, repetition_penalty=1.3))):
        lp = "return_logprobs" in base
        run = lambda base=base, **kw: m.generate(p, N, **base, **kw)  # noqa: E731
        _check_eos(what, run, eos, Ps, lp=lp, must_finish=False)
        _check_eos(what + ", its own eos", run, _own_eos(run, Ps, lp=lp), Ps, lp=lp)
    # ragged: rows of 23 and 9 real tokens
    lens = (23, 9)
    run = lambda **kw: m.generate(p, N, lengths=lens, **({"pad_token_id": PAD} if "pad_token_id" not in kw else {}), **kw)  # noqa: E731
    n_new = _check_eos("ragged", run, _own_eos(run, lens), lens)
    run = lambda **kw: m.generate(p, N, lengths=lens, prefill=True, return_logprobs=True, **({"pad_token_id": PAD} if "pad_token_id" not in kw else {}), **kw)  # noqa: E731
    _check_eos("ragged + prefill + log-probs", run, _own_eos(run, lens, lp=True), lens, lp=True)
    # an eos inside the prompt finishes nothing: the prompt is forced, not generated
    q = p.clone()
    q[:, 5], q[0, 22] = eos, eos
    n_new = _check_eos("eos in the prompt", lambda **kw: m.generate(q, N, **kw), eos, Ps, must_finish=False)
    assert min(n_new) >= 1


def test_eos_on_whisper_with_and_without_rules(whisper):
    w, _, _, mem, wp, rules = whisper
    n_new = _check_eos("whisper", lambda **kw: w.decoder.generate(mem, wp.cuda(), N, **kw), C.whisper_eos(False), [4, 4])
    assert len(set(n_new)) == 2 and max(n_new) < N
    cp = C.whisper_ctl_prompt().cuda()
    n_new = _check_eos("whisper, rules, log-probs", lambda **kw: w.decoder.generate(mem, cp, N, rules=rules, return_logprobs=True, **kw),
                       C.whisper_eos(True), [4, 4], lp=True)
    assert len(set(n_new)) == 2 and max(n_new) < N
    # Whisper.generate passes everything through (the encoder's output is another memory: only the plumbing is checked); avg_logprob
    mel = torch.zeros(2, 80, 200, device="cuda")
    kw = dict(rules=rules, return_logprobs=True, eos_token_id=C.whisper_eos(True), pad_token_id=PAD, return_lengths=True, min_new_tokens=2,
              repetition_penalty=1.3, no_repeat_ngram_size=2)
    toks, lps, n_new = w.generate(mel, cp, 6, **kw)
    assert toks.shape == (2, 10) and lps.shape == (2, 6) and n_new.shape == (2,) and bool((n_new >= 2).all()) and _same(w.generate(mel, cp, 6, **kw)[0], toks)
    avg = lps.sum(-1) / n_new
    assert bool(torch.isfinite(avg).all()) and bool((avg <= 0).all())


# ---------------------------------------------------------------------------------------------------------------- early exit
def test_early_exit_polls_and_rebind_starts_unfinished(gpt2, monkeypatch):
    from pytorch_models.audio2text import generate as G

    m, _, prompt = gpt2
    p = prompt[list(C.GPT2_EOS_ROWS)].cuda()
    eos = C.gpt2_eos()
    kw = dict(eos=eos, pad_token_id=PAD, return_logprobs=True)
    outs = {}
    for poll in (1, N + 50):
        monkeypatch.setattr(G, "POLL_EVERY", poll)
        st = G.GreedyDecoder(m, None, p.clone(), N, **kw)  # (a decoder keeps the device prompt it is given: rebind() writes into it)
        st.run()
        outs[poll] = (st.output()[0].clone(), st.output_logprobs(), st.output_lengths(), st.steps_run, st.n_steps)
    a, b = outs[1], outs[N + 50]
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])
    assert a[3] < a[4] and b[3] == b[4] == 22 + N, (a[3:], b[3:])
    assert a[3] == 22 + int(a[2].max()), "the run stops at the step that finished the last row"
    # the same decoder again after rebind(): no row starts finished, the graph is kept, the result is a fresh decoder's
    monkeypatch.setattr(G, "POLL_EVERY", 1)
    graph = st._graph
    other = prompt[[0, 2]].cuda()
    st.rebind(None, other)
    assert int(st.finished.abs().sum()) == 0
    st.run()
    want = G.greedy_decode(m, None, other, N, eos_token_id=eos, pad_token_id=PAD, return_logprobs=True, return_lengths=True)
    assert st._graph is graph and _same((st.output()[0], st.output_logprobs(), st.output_lengths()), want)
    st.rebind(None, p)
    st.run()
    assert _same(st.output()[0], a[0]) and _same(st.output_logprobs(), a[1]) and _same(st.output_lengths(), a[2])
    # a decoder without eos reports n_new for every row
    plain = G.GreedyDecoder(m, None, p, N)
    plain.run()
    assert plain.output_lengths().tolist() == [N, N] and plain.steps_run == plain.n_steps


# ------------------------------------------------------------------------------------------------------------------ no-repeat
def test_no_repeat_ngram_leaves_no_repeated_ngram(gpt2, whisper):
    m, _, _ = gpt2
    p = C.gpt2_ctl_prompt().cuda()
    plain = m.generate(p, N).cpu().tolist()
    assert any(C.has_repeat(r, C.NGRAM) for r in plain), "the plain run repeats nothing: the test does not bite"
    for kw in (dict(), dict(prefill=True), dict(topk=4, seed=3), dict(topk=0, temperature=0.7, top_p=0.9, seed=11), dict(repetition_penalty=1.3)):
        rows = m.generate(p, N, no_repeat_ngram_size=C.NGRAM, **kw).cpu().tolist()
        assert not any(C.has_repeat(r, C.NGRAM) for r in rows), kw
    for n in (1, 3):
        assert not any(C.has_repeat(r, n) for r in m.generate(p, N, no_repeat_ngram_size=n).cpu().tolist()), n
    lens = (23, 9, 1)  # ragged: every row's REAL tokens (the padding is not history, and repeats of the pad id do not count)
    got = m.generate(p, N, lengths=lens, pad_token_id=int(p[0, 0]), no_repeat_ngram_size=C.NGRAM).cpu()
    for b, ln in enumerate(lens):
        assert not C.has_repeat(got[b, : ln + N].tolist(), C.NGRAM), b
    w, _, _, mem, _, rules = whisper
    cp = C.whisper_ctl_prompt().cuda()
    assert any(C.has_repeat(r, C.NGRAM) for r in w.decoder.generate(mem, cp, N, rules=rules).cpu().tolist())
    assert not any(C.has_repeat(r, C.NGRAM) for r in w.decoder.generate(mem, cp, N, rules=rules, no_repeat_ngram_size=C.NGRAM).cpu().tolist())


# --------------------------------------------------------------------------------------------------------- against the oracle
def _check_argmax(what, toks, n_new, logits, P, c, post=None):
    """toks (B, P + N) produced, logits (B, L - 1, V) the oracle's teacher-forced ones for that prefix (before controls and rules)"""
    unclear = total = 0
    bound = C.margin_bound(c.r)
    for b in range(toks.shape[0]):
        row = toks[b].tolist()
        for i in range(n_new[b]):
            out, want, margin = C.position(logits[b, P - 1 + i], row[: P + i], i, c, post)
            tok = row[P + i]
            assert float(out[tok]) > -float("inf"), f"{what}: row {b} token {i} = {tok} is banned by the reference"
            total += 1
            if margin > bound:
                assert tok == want, f"{what}: row {b} token {i}: got {tok}, reference {want} at margin {margin:.3e} (bound {bound:.3e})"
            else:
                unclear += 1
    print(f"{what}: {unclear} of {total} positions within {bound:.3f} of a tie (cap {S.EDGE_CAP:.0%})")
    assert unclear <= S.EDGE_CAP * total


@pytest.mark.parametrize("name", list(C.RUNS))
def test_controlled_run_follows_the_reference(name, gpt2, whisper):
    from oracle import ref_text as RX

    prompt, c, _, _ = C.run_case(name)
    P = prompt.shape[1]
    kw = dict(c.kwargs(), pad_token_id=PAD, return_lengths=True)
    if name.startswith("gpt2"):
        m, sd, _ = gpt2
        toks, n_new = m.generate(prompt.cuda(), N, **kw)
        toks = toks.cpu()
        logits, post = RX.gpt2(sd, toks[:, :-1], rp=S.kv_round), None
    else:
        w, sd, memory, mem, _, rules = whisper
        toks, n_new = w.decoder.generate(mem, prompt.cuda(), N, rules=rules, **kw)
        toks = toks.cpu()
        logits, post = S.whisper_logits(sd, memory, toks[:, :-1], P, False), C.whisper_post(True)
    n_new = n_new.tolist()
    if c.eos is None:
        assert n_new == [N] * len(n_new)
    else:
        for b, k in enumerate(n_new):
            new = toks[b, P:].tolist()
            assert k >= min(c.min_new + 1, N) or c.eos not in new and k == N, f"row {b} finished after {k} < min_new_tokens + 1 tokens"
            assert new == C.cut_at_eos(new, c.eos, PAD)[0]
    _check_argmax(name, toks, n_new, logits, P, c, post)


def test_sampled_run_under_the_controls_follows_the_reference(gpt2):
    from oracle import ref_text as RX
    from test_hip_sample import _check_sampled

    m, sd, _ = gpt2
    run, c, prompt = C.sampled_run(), C.SAMPLED_CTL, C.gpt2_ctl_prompt()
    P = prompt.shape[1]
    toks, lps = m.generate(prompt.cuda(), N, topk=run["topk"], temperature=run["temperature"], top_p=run["top_p"], seed=run["seed"],
                           return_logprobs=True, repetition_penalty=c.r, no_repeat_ngram_size=c.n)
    toks = toks.cpu()
    logits = RX.gpt2(sd, toks[:, :-1], rp=S.kv_round)
    for b in range(toks.shape[0]):  # the controlled logits of the produced prefix: what the tail saw, and what its log-prob is of
        for i in range(N):
            logits[b, P - 1 + i] = C.apply_controls(logits[b, P - 1 + i].float(), toks[b, : P + i].tolist(), i, c)
    unclear = _check_sampled("sampled under the controls", toks, lps, logits, run, P, P - 1, rows=list(range(toks.shape[0])))
    assert unclear <= S.EDGE_CAP * toks.shape[0] * N
    assert not any(C.has_repeat(r, c.n) for r in toks.tolist())


# ---------------------------------------------------------------------------------------------------------- graph and eager
def test_graph_replay_equals_eager_and_two_calls_agree(gpt2, whisper):
    m, _, _ = gpt2
    prompt, c, _, _ = C.run_case("gpt2_all")
    kw = dict(c.kwargs(), pad_token_id=PAD, return_lengths=True, return_logprobs=True)
    a = m.generate(prompt.cuda(), N, **kw)
    assert _same(a, m.generate(prompt.cuda(), N, **kw)) and _same(a, m.generate(prompt.cuda(), N, graph=False, **kw))
    assert len(a) == 3 and a[1].shape == (3, N) and a[2].dtype == torch.int64
    kw.update(topk=0, temperature=0.7, top_p=0.9, seed=11, lengths=(23, 9, 1))
    a = m.generate(prompt.cuda(), N, **kw)
    assert _same(a, m.generate(prompt.cuda(), N, **kw)) and _same(a, m.generate(prompt.cuda(), N, graph=False, **kw))
    w, _, _, mem, _, rules = whisper
    prompt, c, _, _ = C.run_case("whisper_all_rules")
    kw = dict(c.kwargs(), pad_token_id=PAD, return_lengths=True, return_logprobs=True, rules=rules)
    a = w.decoder.generate(mem, prompt.cuda(), N, **kw)
    assert _same(a, w.decoder.generate(mem, prompt.cuda(), N, **kw)) and _same(a, w.decoder.generate(mem, prompt.cuda(), N, graph=False, **kw))


def test_decoder_generator_passes_the_controls(gpt2):
    from pytorch_models.text.generator import DecoderGenerator

    m, _, _ = gpt2
    prompt = C.gpt2_ctl_prompt()
    gen = DecoderGenerator(m, None)
    ids = prompt[0].tolist()
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    want = m.generate(prompt[:1].cuda(), N, **kw)[0].tolist()
    assert gen.generate_ids(ids, N, **kw) == want and want != m.generate(prompt[:1].cuda(), N)[0].tolist()
    eos = want[23 + 4]
    stopped = m.generate(prompt[:1].cuda(), N, eos_token_id=eos, min_new_tokens=2, **kw)[0].tolist()
    cut = gen.generate_ids(ids, N, eos_token_id=eos, min_new_tokens=2, **kw)
    assert eos in stopped[23 + 2 :] and eos not in stopped[23 : 23 + 2] and cut == stopped[: 23 + stopped[23:].index(eos) + 1]
    batch = gen.generate_ids_batch([ids, ids[:5]], N, **kw)
    assert batch[0] == want and len(batch[1]) == 5 + N and not C.has_repeat(batch[1], 2)
    with pytest.raises(ValueError):
        gen.generate_ids(ids, N, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        gen.generate_ids(ids, N, min_new_tokens=2)  # no eos_token_id


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal(gpt2, whisper):
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode

    m, _, prompt = gpt2
    w, _, _, mem, wp, rules = whisper
    p, wp = prompt.cuda(), wp.cuda()
    mel = torch.zeros(2, 80, 200, device="cuda")
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9), dict(min_new_tokens=3), dict(min_new_tokens=-1, eos_token_id=5),
                dict(eos_token_id=50257), dict(eos_token_id=-1), dict(eos_token_id=5, pad_token_id=50257), dict(eos_token_id=5, pad_token_id=-1)):
        calls = [lambda: m.generate(p, 2, **bad), lambda: greedy_decode(m, None, p, 2, **bad),
                 lambda: GreedyDecoder(m, None, p, 2, **{("eos" if k == "eos_token_id" else k): v for k, v in bad.items()})]
        if 50257 not in bad.values():  # an id of Whisper's larger vocabulary
            calls.append(lambda: w.generate(mel, wp, 2, **bad))
        for call in calls:
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        w.decoder.generate(mem, wp, 2, eos_token_id=51865)
    for new in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(return_lengths=True), dict(min_new_tokens=1, eos_token_id=5)):
        for call in (lambda: m.generate(p, 2, beams=2, **new), lambda: m.generate(p, 2, return_beams=True, **new),
                     lambda: w.decoder.generate(mem, wp, 2, beams=2, **new), lambda: w.generate(mel, wp, 2, beams=2, **new)):
            with pytest.raises(ValueError, match="beams=1"):
                call()
    assert m.generate(p, 2, beams=2, eos_token_id=5).shape == (3, 25)  # beam search keeps its own eos_token_id
    for new in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1, eos_token_id=5)):
        with pytest.raises(ValueError, match="margins=False"):
            greedy_decode(m, None, p, 2, margins=True, **new)
    for new in (dict(eos_token_id=5), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(return_lengths=True)):
        for call in (lambda: m.generate(p, 2, path="persistent", **new), lambda: w.decoder.generate(mem, wp, 2, path="persistent", **new),
                     lambda: w.generate(mel, wp, 2, exact=True, **new), lambda: greedy_decode(w.decoder, mem.float(), wp, 2, kv32=True, **new),
                     lambda: copy.deepcopy(m).float().generate(p, 2, **new),
                     lambda: copy.deepcopy(w).float().decoder.generate(mem.float(), wp, 2, **new)):
            with pytest.raises(NotImplementedError, match="launches|exact=False|bfloat16"):
                call()
