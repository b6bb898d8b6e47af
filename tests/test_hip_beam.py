"""GPU: batched beam search end to end (generate.BeamDecoder / beam_decode / the ``beams`` keyword of the generate methods) on
Whisper(1000, 2, 128), bf16 with synthetic weights, B = 2, P = 3, 12 new tokens:
  * beams=1 is today's generate; graph replay == eager stepping;
  * the STEP AUDIT: after every eager step the recorded (parents, tokens, scores) are the float64 step reference applied to the
    device's own logits and the previous scores, and every layer's K / V rows are the parent's rows bit for bit;
  * exact=True at W = 4 against the reference search on the CPU (tests/beam_cases.py): tokens and parents equal, scores within
    BC.SCORE_TOL; Whisper's logit rules; the refusals; a decoder-only stack."""
import pytest
import torch

import beam_cases as BC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
N = BC.N_NEW


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(seed):
        if seed not in cache:
            w, _, mel, prompt = BC.small_whisper(seed)
            cache[seed] = (w.to(torch.bfloat16).cuda(), mel.cuda(), prompt.cuda())
        return cache[seed]

    return get


def _run_launches(st, launches):
    from pytorch_models._hip import check

    stream = torch.cuda.current_stream().cuda_stream
    for fn, args in launches:
        check(fn(*args[:-1], stream), fn.__name__)


def audit(st, eos):
    """Eager stepping with every step checked.  Returns (parents per generated step (n, B, W), smallest separation / bound)."""
    B, W, P, V = st.clips, st.W, st.P, st.logits.shape[1]
    ident = torch.arange(W).expand(B, W)
    st.reset()
    all_par, worst = [], float("inf")
    for t in range(st.n_steps):
        sc0, fin0 = st.scores.cpu(), st.finished.cpu().bool()
        k0 = [k.clone() for k in st.self_k + st.self_v]
        _run_launches(st, st.launches[:-1])  # everything but the reorder: the caches hold position t of every row, unmoved
        k1 = [k.clone() for k in st.self_k + st.self_v]
        _run_launches(st, st.launches[-1:])
        torch.cuda.synchronize()
        par, sc, fin = st.parents.cpu().long(), st.scores.cpu(), st.finished.cpu().bool()
        tok = st.tokens[:, t + 1].cpu().view(B, W)
        assert int(st.pos.item()) == t + 1
        if t + 1 < P:  # the prompt is forced: nothing moves
            assert torch.equal(par, ident) and torch.equal(sc, sc0) and torch.equal(fin, fin0)
            assert torch.equal(tok.reshape(-1), st.prompt[:, t + 1].cpu())
        else:
            logits = st.logits.cpu()
            w_par, w_tok, w_sc, w_fin, top = BC.step_ref(sc0, fin0, logits, W, eos)
            bound = BC.logits_bound(logits, sc0, V)
            sep = BC.min_separation(top)
            assert sep > 2 * bound, (t, sep, bound)  # both sides within `bound` of the exact scores: decided
            worst = min(worst, sep / bound)
            assert torch.equal(par, w_par) and torch.equal(tok, w_tok) and torch.equal(fin, w_fin), t
            err = sc.double() - w_sc
            assert torch.equal(torch.isinf(sc), torch.isinf(w_sc))
            assert float(torch.where(torch.isnan(err), torch.zeros_like(err), err).abs().max()) <= bound, t
            all_par.append(par)
        rows = (par + torch.arange(B)[:, None] * W).reshape(-1).cuda()
        for now, mid, old in zip(st.self_k + st.self_v, k1, k0):  # bitwise: compared as integers
            bits = torch.int16 if now.dtype == torch.bfloat16 else torch.int32
            now, mid, old = now.view(bits), mid.view(bits), old.view(bits)
            assert torch.equal(mid[:, :, :t], old[:, :, :t])  # the step appends position t and touches nothing below it
            assert torch.equal(now[:, :, : t + 1], mid[rows][:, :, : t + 1]), (t, "K/V rows are not the parents'")
            assert torch.equal(now[:, :, t + 1 :], mid[:, :, t + 1 :]), (t, "positions above t were written")
        hist = st.tokens[:, : t + 2].cpu().view(B, W, -1)
        assert torch.equal(hist[:, :, -1], tok)
    return torch.stack(all_par), worst


def test_beams_1_is_todays_generate(models):
    from pytorch_models.audio2text.generate import beam_decode

    w, mel, prompt = models(BC.SEEDS[0])
    want = w.generate(mel, prompt, N)
    assert torch.equal(w.generate(mel, prompt, N, beams=1), want)
    want_x = w.generate(mel, prompt, N, exact=True)
    assert torch.equal(w.generate(mel, prompt, N, exact=True, beams=1), want_x)
    # width 1 THROUGH the beam kernels is the arg-max too (lowest index on ties, as pm_dec_next_token)
    toks, scores = beam_decode(w.decoder, w.encoder(mel), prompt, N, beams=1, return_beams=True)
    assert torch.equal(toks[:, 0], want) and bool((scores < 0).all())


@pytest.mark.parametrize("W", [4, 5])
def test_graph_replay_equals_eager_stepping(models, W):
    from pytorch_models.audio2text.generate import BeamDecoder

    w, mel, prompt = models(BC.SEEDS[0])
    st = BeamDecoder(w.decoder, w.encoder(mel), prompt, N, W)
    st.run(graph=True)
    replayed = (st.tokens.clone(), st.scores.clone())
    st.reset()
    par_g = []
    for _ in range(st.n_steps):
        st._graph.replay()
        par_g.append(st.parents.clone())
    assert torch.equal(st.tokens, replayed[0]) and torch.equal(st.scores, replayed[1])  # a second replay of the same graph
    st.reset()
    par_e = []
    for _ in range(st.n_steps):
        st.step()
        par_e.append(st.parents.clone())
    assert torch.equal(st.tokens, replayed[0]) and torch.equal(st.scores, replayed[1])
    assert torch.equal(torch.stack(par_g), torch.stack(par_e))
    toks, scores = w.generate(mel, prompt, N, beams=W, return_beams=True)
    assert torch.equal(toks.view(-1, toks.shape[-1]), replayed[0]) and torch.equal(scores, replayed[1])
    assert torch.equal(w.generate(mel, prompt, N, beams=W), toks[:, 0])
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()) and len({tuple(r.tolist()) for r in toks[0]}) == W


@pytest.mark.parametrize("seed", BC.SEEDS)
@pytest.mark.parametrize("W", [4, 5])
def test_step_audit_bf16(models, seed, W):
    from pytorch_models.audio2text.generate import BeamDecoder

    w, mel, prompt = models(seed)
    st = BeamDecoder(w.decoder, w.encoder(mel), prompt, N, W)
    parents, worst = audit(st, None)
    print(f"seed {seed} W {W}: smallest separation = {worst:.1f} bounds")
    assert parents.shape == (N, BC.CLIPS, W) and bool((parents[0] == 0).all())
    assert bool((parents != torch.arange(W)).any())  # the caches really moved


@pytest.mark.parametrize("seed", BC.SEEDS)
def test_exact_path_against_the_cpu_reference_search(models, seed):
    """exact=True (fp32 encoder twin, fp32 K/V caches) at W = 4 against the reference's fp32 full-prefix search: the two sum in
    different orders, so only decisions further apart than BC.GAP_MIN are comparable - test_beam_cases_cpu.py shows that every
    decision of these seeds is."""
    from pytorch_models.audio2text.generate import BeamDecoder

    W = 4
    w, mel, prompt = models(seed)
    *_, (r_toks, r_scores, r_parents, r_gaps) = BC.reference_case(seed, W)
    assert float(r_gaps.min()) >= BC.GAP_MIN
    toks, scores = w.generate(mel, prompt, N, exact=True, beams=W, return_beams=True)
    err = float((scores.cpu().double() - r_scores).abs().max())
    print(f"seed {seed}: max |device score - reference score| = {err:.3e} (tolerance {BC.SCORE_TOL:.3e}); "
          f"min reference gap {float(r_gaps.min()):.3e}")
    assert torch.equal(toks.cpu(), r_toks)
    assert err <= BC.SCORE_TOL
    st = BeamDecoder(w.decoder, w.exact_copy().encoder(mel), prompt, N, W, kv32=True)
    parents, _ = audit(st, None)  # the fp32-cache reorder, bit for bit, on the way
    assert torch.equal(parents, r_parents)
    assert torch.equal(st.tokens.view(BC.CLIPS, W, -1), toks) and torch.equal(st.scores, scores)


def _rules():
    from pytorch_models.audio2text.generate import WhisperRules

    sup = (0, 1, 2, 3, 17, 40, 901)
    return WhisperRules(eot=5, timestamp_begin=900, suppress=sup, blank=(7, 5)), sup


@pytest.mark.parametrize("seed", BC.SEEDS)
def test_beam_search_under_whisper_rules(models, seed):
    from pytorch_models.audio2text.generate import BeamDecoder

    W = 4
    w, mel, prompt = models(seed)
    rules, sup = _rules()
    st = BeamDecoder(w.decoder, w.encoder(mel), prompt, N, W, rules=rules)
    assert st.eos == rules.eot
    audit(st, rules.eot)  # the same audit on the filtered logits (-inf entries and all)
    toks, scores = st.beams()
    toks, scores = toks.cpu(), scores.cpu()
    got = w.generate(mel, prompt, N, beams=W, rules=rules, return_beams=True)
    assert torch.equal(got[0].cpu(), toks) and torch.equal(got[1].cpu(), scores)
    gen = toks[:, :, BC.PROMPT :]
    assert not bool(torch.isin(gen, torch.tensor(sup)).any())
    assert bool((gen[:, :, 0] >= 900).all())  # a transcript starts with a timestamp
    for row in gen.reshape(-1, N).tolist():
        if 5 in row:
            assert all(t == 5 for t in row[row.index(5):])


def test_a_finished_beam_holds_eos_at_a_frozen_score(models):
    """eos = a token the unconstrained best beam emits early, so a hypothesis does finish: from there on it is extended with
    eos, and its score is, bit for bit, the score it finished with"""
    from pytorch_models.audio2text.generate import BeamDecoder

    W = 4
    w, mel, prompt = models(BC.SEEDS[0])
    memory = w.encoder(mel)
    free = w.decoder.generate(memory, prompt, N, beams=W)
    eos = int(free[0, BC.PROMPT + 2])
    st = BeamDecoder(w.decoder, memory, prompt, N, W, eos=eos)
    st.reset()
    frozen = torch.full((BC.CLIPS, W), float("nan"))  # the score each finished row finished with, carried along its parents
    was = torch.zeros(BC.CLIPS, W, dtype=torch.bool)
    for t in range(st.n_steps):
        st.step()
        par, sc, fin = st.parents.cpu().long(), st.scores.cpu(), st.finished.cpu().bool()
        frozen = torch.where(was.gather(1, par), frozen.gather(1, par), torch.where(fin, sc, frozen))
        assert bool((fin.int() >= was.gather(1, par).int()).all())  # a finished parent's survivor stays finished
        was = fin
    assert bool(was.any())
    assert torch.equal(st.scores.cpu()[was], frozen[was])
    for row, f in zip(st.tokens[:, BC.PROMPT :].cpu().tolist(), was.reshape(-1).tolist()):
        assert f == (eos in row)
        if f:
            assert all(t == eos for t in row[row.index(eos):])
    assert torch.equal(st.tokens, BeamDecoder(w.decoder, memory, prompt, N, W, eos=eos).run(graph=True))


def test_refusals(models):
    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.generate import BeamDecoder, GreedyDecoder, beam_decode

    w, mel, prompt = models(BC.SEEDS[0])
    memory = w.encoder(mel)
    with pytest.raises(ValueError, match="beams must be in 1..8"):
        w.generate(mel, prompt, N, beams=9)
    with pytest.raises(ValueError, match="beams must be in 1..8"):
        beam_decode(w.decoder, memory, prompt, N, beams=0)
    with pytest.raises(NotImplementedError, match="at most 64 rows"):
        w.decoder.generate(memory[:1].expand(13, -1, -1).contiguous(), prompt[:1].expand(13, -1).contiguous(), N, beams=5)
    with pytest.raises(NotImplementedError, match="persistent"):
        w.generate(mel, prompt, N, beams=4, path="persistent")
    with pytest.raises(ValueError, match="BeamDecoder"):
        GreedyDecoder(w.decoder, memory, prompt, N, beams=2)
    with pytest.raises(ValueError, match="eos_token_id"):
        w.generate(mel, prompt, N, beams=2, eos_token_id=BC.VOCAB)
    w32, _, mel32, prompt32 = BC.small_whisper(BC.SEEDS[0])
    w32 = w32.cuda()
    with pytest.raises(NotImplementedError, match="bf16 weights"):
        w32.generate(mel32.cuda(), prompt32.cuda(), N, beams=4)
    with pytest.raises(NotImplementedError, match="bf16 weights"):
        w32.decoder.generate(w32.encoder(mel32.cuda()), prompt32.cuda(), N, beams=4)
    wcpu = BC.small_whisper(BC.SEEDS[0])[0].to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bf16 weights on a HIP device"):
        wcpu.generate(mel32, prompt32, N, beams=4)
    with pytest.raises(NotImplementedError, match="bf16 weights on a HIP device"):
        BeamDecoder(wcpu.decoder, torch.zeros(2, 10, BC.D_MODEL, dtype=torch.bfloat16), prompt32, N, 4)


def test_exact_limit_on_rows_times_heads():
    """B * W * n_heads <= 256 with fp32 caches: d_model 576 = 9 heads, 6 x 5 rows -> 270 pairs"""
    from pytorch_models.audio2text.generate import BeamDecoder
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from synthweights import fill_module

    d = WhisperDecoder(300, 1, 576).eval()
    fill_module(d, 3)
    d = d.to(torch.bfloat16).cuda()
    mem = torch.zeros(6, 8, 576, device="cuda")
    with pytest.raises(NotImplementedError, match="n_heads <= 256"):
        BeamDecoder(d, mem, torch.zeros(6, 2, dtype=torch.int64, device="cuda"), 4, 5, kv32=True)


def test_decoder_only_stack_passes_the_step_audit():
    """a 2-layer GPT-2-shaped decoder (no memory, 50257 ids: 50 terms per thread in the log-sum-exp) at W = 3"""
    from pytorch_models.audio2text.generate import BeamDecoder
    from pytorch_models.text import GPT2
    from synthweights import bf16_round_, fill_module, synth_tokens

    m = GPT2(2, 128).eval()
    fill_module(m, 81)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    prompt = synth_tokens("beam_gpt2", (2, 3), 50257, 81).cuda()
    st = BeamDecoder(m, None, prompt, 8, 3)
    parents, worst = audit(st, None)
    print(f"GPT-2 shaped: smallest separation = {worst:.1f} bounds")
    toks, scores = m.generate(prompt, 8, beams=3, return_beams=True)
    assert torch.equal(toks.view(-1, toks.shape[-1]), st.tokens) and torch.equal(scores, st.scores)
    assert torch.equal(m.generate(prompt, 8, beams=1), m.generate(prompt, 8))


def test_rebind_keeps_the_captured_graph(models):
    """new clips of the same geometry: the cross K / V are re-projected into the existing rows and the replayed graph decodes them"""
    from pytorch_models.audio2text.generate import BeamDecoder

    W = 4
    w, mel, prompt = models(BC.SEEDS[0])
    memory = w.encoder(mel)
    st = BeamDecoder(w.decoder, memory, prompt, N, W)
    first = (st.run(graph=True).clone(), st.scores.clone())
    st.rebind(memory.flip(0).contiguous(), prompt.flip(0).contiguous())  # the two clips swapped
    again = (st.run(graph=True).clone(), st.scores.clone())
    assert not torch.equal(again[0], first[0])
    assert torch.equal(again[0].view(2, W, -1).flip(0), first[0].view(2, W, -1)) and torch.equal(again[1].flip(0), first[1])
