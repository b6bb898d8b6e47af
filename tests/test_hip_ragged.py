"""GPU, end to end: ragged prompt batches (``lengths=``) through the KV-cached decoders.

Definition of correct: row b of a ragged run is what generate() returns for prompt[b:b+1, :len_b] on its own.  The oracle is
therefore called per row on the unpadded prompt (oracle/ref_text.greedy, oracle/ref_whisper), and the rules are the existing ones:

  step path (prefill=False)   : tests/test_hip_decode.py's - a row may first differ from the K/V-rounded oracle only where the oracle's
                                top-2 margin is below 2e-4;
  prompt pass (prefill=True)  : tests/test_hip_prefill.py's - a first difference only where the reference margin is below tau,
                                tau = 2 x the largest |model forward logit - oracle logit| at the positions that choose a token,
                                at most ONE sequence per case.

Seeds: GPT2(2, 128) fill_module seed 72 with ragged_cases.gpt2_prompt() (lengths 40 / 23 / 1), Whisper tiny seed 55 with
ragged_cases.whisper_prompt() (lengths 4 / 2).  tests/test_ragged_cases_cpu.py pins that the all-rounded CPU oracle loop keeps the
unrounded ids of EVERY row (smallest oracle margins 0.046 / 0.078), so the reference alone needs no exception."""
import pytest
import torch

import ragged_cases as RC
from oracle import ref_text as RX
from oracle import ref_whisper as RW
from oracle import ref_whisper_rules as RR
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
PAD = 7  # the id the output is padded with (any id of the vocabulary)


def kv_round(name, t):  # the cache holds bf16 k / v (the rounding point of the decode kernels)
    return t.to(torch.bfloat16).float() if name == "kv" else t


@pytest.fixture(scope="module")
def gpt2():
    """(model, state dict, the ragged prompt, per row: (K/V-rounded oracle ids (1, len + n_new), margins (1, n_new)))"""
    from pytorch_models.text import GPT2

    m = GPT2(2, 128)
    fill_module(m, RC.GPT2_SEED)
    bf16_round_(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    prompt = RC.gpt2_prompt()
    rows = [RX.greedy(RX.gpt2, sd, prompt[b : b + 1, :n], RC.GPT2_NEW, rp=kv_round) for b, n in enumerate(RC.GPT2_LENGTHS)]
    return m.to(torch.bfloat16).cuda().eval(), sd, prompt, rows


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


def _layout(got, prompt, lengths, n_new, pad=PAD):
    """(B, P + n_new): row b = its prompt, n_new new ids, then P - len_b pad ids; returns the rows without their padding"""
    got = got.cpu()
    B, P = prompt.shape
    assert got.shape == (B, P + n_new) and got.dtype == torch.int64
    rows = []
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :n], prompt[b, :n]), f"row {b}: the prompt must be kept"
        assert bool((got[b, n + n_new :] == pad).all()), f"row {b}: pad ids behind the new ones"
        rows.append(got[b, : n + n_new])
    return rows


def _obeys(rows, wants, margin_at, lengths, tau, what, most=1):
    """rows / wants: per sequence 1-D ids; a first difference only where margin_at(b, t) < tau; at most ``most`` sequences use it"""
    used = 0
    for b, (got, want) in enumerate(zip(rows, wants)):
        assert got.shape == want.shape, (what, b)
        diff = (got != want).nonzero()
        if len(diff):
            t = int(diff[0])
            assert t >= lengths[b], f"{what}: sequence {b} lost its prompt"
            m = float(margin_at(b, t))
            print(f"{what}: sequence {b} first differs at position {t}: got {int(got[t])} reference {int(want[t])} margin {m:.3e} tau {tau:.3e}")
            assert m < tau, f"{what}: sequence {b} differs at position {t} at a decisive margin ({m:.3e} >= tau {tau:.3e})"
            used += 1
    assert used <= most, f"{what}: {used} sequences needed the near-tie exception"


# ------------------------------------------------------------------------------------------------ 1. GPT-2
def test_gpt2_ragged_rows_follow_their_own_oracle(gpt2):
    from pytorch_models.audio2text.generate import greedy_decode

    m, sd, prompt, oracle = gpt2
    lens, n_new = RC.GPT2_LENGTHS, RC.GPT2_NEW
    wants = [w[0] for w, _ in oracle]
    margin_at = lambda b, t: oracle[b][1][0, t - lens[b]]  # noqa: E731
    print(f"smallest oracle margin {min(float(mg.min()) for _, mg in oracle):.3e}")
    # the step path: prompt positions forced one step each, the padded ones too
    got = m.generate(prompt.cuda(), n_new, lengths=lens, pad_token_id=PAD)
    _obeys(_layout(got, prompt, lens, n_new), wants, margin_at, lens, 2e-4, "ragged steps", most=len(lens))
    assert torch.equal(m.generate(prompt.cuda(), n_new, lengths=torch.tensor(lens), pad_token_id=PAD, graph=False), got)  # eager == replay
    toks, marg = greedy_decode(m, None, prompt.cuda(), n_new, lengths=lens, pad_token_id=PAD, margins=True)
    assert torch.equal(toks, got) and marg.shape == got.shape
    for b, n in enumerate(lens):  # margins aligned like the ids: the chosen tokens' right behind the prompt, zeros over the padding
        assert bool((marg[b, n + n_new :] == 0).all()) and bool((marg[b, n : n + n_new] > 0).all())
        alone = greedy_decode(m, None, prompt[b : b + 1, :n].cuda(), n_new, margins=True, fused=False)[1]
        torch.testing.assert_close(marg[b, n : n + n_new], alone[0, n:], rtol=0, atol=2e-4)
    # the padding ids are ignored: other ids behind the prompts, the same rows
    other = prompt.clone()
    for b, n in enumerate(lens):
        other[b, n:] = (other[b, n:] + 1000) % 2000
    assert torch.equal(m.generate(other.cuda(), n_new, lengths=lens, pad_token_id=PAD), got)
    # the prompt pass: tau from the forward of each row alone, teacher-forced on its oracle's ids
    tau = 2.0 * max(float((m(w[:, :-1].cuda())[:, n - 1 :].float().cpu() - RX.gpt2(sd, w[:, :-1])[:, n - 1 :]).abs().max())
                    for (w, _), n in zip(oracle, lens))
    print(f"tau = {tau:.3e}")
    for chunk in (512, 16):  # 16: starts inside chunks (23 tokens from position 17), whole chunks of padding for the one-token row
        got = greedy_decode(m, None, prompt.cuda(), n_new, lengths=lens, pad_token_id=PAD, prefill=True, prefill_chunk=chunk)
        _obeys(_layout(got, prompt, lens, n_new), wants, margin_at, lens, tau, f"ragged prefill, chunk {chunk}")


def test_all_lengths_equal_is_the_rectangular_run_in_the_unfused_form(gpt2, whisper):
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode

    m, _, prompt, _ = gpt2
    p = prompt[:, :23].cuda()
    full = (23,) * p.shape[0]
    st = GreedyDecoder(m, None, p, 8, lengths=full)
    names = [fn.__name__ for fn, _ in st.launches]
    assert "pm_dec_attention_ragged" in names and "pm_dec_next_token_ragged" in names and "pm_dec_attention_fused" not in names
    assert not any(n.endswith("_ragged") for fn, _ in GreedyDecoder(m, None, p, 8).launches for n in (fn.__name__,))  # lengths=None: as ever
    assert torch.equal(greedy_decode(m, None, p, 8, lengths=full), greedy_decode(m, None, p, 8, fused=False))
    assert torch.equal(greedy_decode(m, None, p, 8, lengths=full, prefill=True, prefill_chunk=16),
                       greedy_decode(m, None, p, 8, fused=False, prefill=True, prefill_chunk=16))
    # Whisper: the cross block stays fused, the self block and the chain are off
    dec, _, memory = whisper
    wp = RC.whisper_prompt().cuda()
    st = GreedyDecoder(dec, memory, wp, 8, lengths=(4, 4))
    names = [fn.__name__ for fn, _ in st.launches]
    assert names.count("pm_dec_attention_fused") == len(dec.layers) and "pm_dec_attention_chain" not in names
    assert names.count("pm_dec_attention_ragged") == len(dec.layers)


def test_whisper_all_lengths_equal_matches_the_unfused_self_block(whisper, monkeypatch):
    from pytorch_models.audio2text.generate import greedy_decode

    dec, _, memory = whisper
    wp = RC.whisper_prompt().cuda()
    got = greedy_decode(dec, memory, wp, 8, lengths=(4, 4))
    monkeypatch.setenv("PM_DEC_FUSE_SELF", "0")
    assert torch.equal(got, greedy_decode(dec, memory, wp, 8))


def test_rebind_other_lengths_replays_the_same_graph(gpt2):
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode

    m, _, prompt, _ = gpt2
    n_new = 6
    st = GreedyDecoder(m, None, prompt.cuda(), n_new, lengths=RC.GPT2_LENGTHS, pad_token_id=PAD)
    st.run()
    first = st.output()[0].clone()
    graph = st._graph
    assert graph is not None and torch.equal(first, greedy_decode(m, None, prompt.cuda(), n_new, lengths=RC.GPT2_LENGTHS, pad_token_id=PAD))
    other = synth_tokens("ragged_tok_rebind", (3, RC.GPT2_P), 2000, 5)
    lens = (17, 40, 5)
    st.rebind(None, other.cuda(), lengths=lens)
    st.run()
    assert st._graph is graph
    assert torch.equal(st.output()[0], greedy_decode(m, None, other.cuda(), n_new, lengths=lens, pad_token_id=PAD))
    st.rebind(None, prompt.cuda(), lengths=RC.GPT2_LENGTHS)  # and back
    st.run()
    assert torch.equal(st.output()[0], first)
    with pytest.raises(ValueError, match="lengths="):
        st.rebind(None, other.cuda())
    with pytest.raises(ValueError, match="length"):
        st.rebind(None, other.cuda(), lengths=(17, 41, 5))


# ------------------------------------------------------------------------------------------------ 2. Whisper
def _rules():
    from pytorch_models.audio2text.generate import WhisperRules

    kw = dict(eot=50257, timestamp_begin=50364, no_timestamps=50363, max_initial_timestamp=50, suppress=(1, 2, 7, 50258, 50259),
              blank=(220, 50257))
    return WhisperRules(**kw), RR.Rules(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})


def test_whisper_ragged_rows_are_the_rows_alone(whisper):
    """each row against the rectangular device run of that row alone (its own clip, its unpadded prompt); the margin at a first
    difference is the top-2 gap of the decoder's own forward logits for that prefix (after the oracle's rules, when they apply)"""
    dec, sd, memory = whisper
    prompt, lens, n_new = RC.whisper_prompt(), RC.WHISPER_LENGTHS, RC.WHISPER_NEW
    mem32 = memory.float().cpu()
    rules, oracle_rules = _rules()
    for name, kw, orules in (("plain", {}, None), ("rules", dict(rules=rules), oracle_rules), ("prefill", dict(prefill=True), None)):
        got = dec.generate(memory, prompt.cuda(), n_new, lengths=lens, pad_token_id=PAD, **kw)
        rows = _layout(got, prompt, lens, n_new)
        alone = {k: v for k, v in kw.items() if k != "prefill"}  # the yardstick is the step path of the row alone
        base = [dec.generate(memory[b : b + 1], prompt[b : b + 1, :n].cuda(), n_new, **alone).cpu() for b, n in enumerate(lens)]
        lg = [dec(w[:, :-1].cuda(), memory[b : b + 1]).float().cpu()[0] for b, w in enumerate(base)]
        tau = 2.0 * max(float((lg[b][n - 1 :] - RW.decoder(sd, "decoder.", base[b][:, :-1], mem32[b : b + 1])[0, n - 1 :]).abs().max())
                        for b, n in enumerate(lens))

        def margin_at(b, t):
            row = lg[b][t - 1] if orules is None else RR.apply(orules, lg[b][t - 1], base[b][0, lens[b] : t].tolist())
            top2 = row.topk(2).values
            return top2[0] - top2[1]

        print(f"whisper ragged {name}: tau = {tau:.3e}")
        _obeys(rows, [w[0] for w in base], margin_at, lens, tau, f"whisper ragged {name}")


# ------------------------------------------------------------------------------------------------ 3. top-k
def test_gpt2_ragged_topk_sampling_stays_inside_each_rows_oracle_top_k(gpt2):
    """repeatable for a seed; every drawn id one of the oracle's k most likely continuations of ITS ROW's prefix (minus tau).  The
    draw is keyed by (seed, cache position, row), so the ids are not those of the row decoded alone - only the property holds."""
    m, sd, prompt, _ = gpt2
    lens, n_new, k = RC.GPT2_LENGTHS, RC.GPT2_NEW, 8
    a = m.generate(prompt.cuda(), n_new, topk=k, seed=3, lengths=lens, pad_token_id=PAD)
    assert torch.equal(m.generate(prompt.cuda(), n_new, topk=k, seed=3, lengths=lens, pad_token_id=PAD), a)
    assert not torch.equal(m.generate(prompt.cuda(), n_new, topk=k, seed=4, lengths=lens, pad_token_id=PAD), a)
    for b, row in enumerate(_layout(a, prompt, lens, n_new)):
        n = lens[b]
        lg = RX.gpt2(sd, row[None, :-1])[0]
        tau = 2.0 * float((m(row[None, :-1].cuda())[0, n - 1 :].float().cpu() - lg[n - 1 :]).abs().max())
        for t in range(n, n + n_new):
            assert lg[t - 1][row[t]] >= lg[t - 1].topk(k).values[-1] - tau, (b, t)


# ------------------------------------------------------------------------------------------------ 4. refusals on the device
def test_refusals_name_the_form_that_runs(gpt2, whisper):
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode
    from pytorch_models.text import GPT2

    m, _, prompt, _ = gpt2
    dec, _, memory = whisper
    p, lens = prompt.cuda(), RC.GPT2_LENGTHS
    wp, wl = RC.whisper_prompt().cuda(), RC.WHISPER_LENGTHS
    for build, match, names in (
            (lambda: m.generate(p, 4, lengths=lens, beams=2), "beam", "beams=1"),
            (lambda: dec.generate(memory, wp, 4, lengths=wl, beams=2), "beam", "beams=1"),
            (lambda: GreedyDecoder(m, None, p, 4, lengths=lens, beams=2), "beam", "beams=1"),
            (lambda: m.generate(p, 4, lengths=lens, path="persistent"), "persistent", "path='launches'"),
            (lambda: greedy_decode(dec, memory.float(), wp, 4, lengths=wl, kv32=True), "kv32", "without lengths="),
            (lambda: dec.generate(memory.float(), wp, 4, lengths=wl), "kv32", "without lengths="),
            (lambda: GPT2(1, 64).cuda().generate(p[:, :8], 4, lengths=(8, 3, 1)), "bf16 parameters", "greedy_exact")):
        with pytest.raises(NotImplementedError, match=match) as e:
            build()
        assert names in str(e.value)
    for bad in ((40, 23), (40, 23, 0), (41, 23, 1), (40.0, 23.0, 1.0), torch.tensor([[40, 23, 1]])):
        with pytest.raises(ValueError, match="length"):
            m.generate(p, 4, lengths=bad)
    with pytest.raises(ValueError, match="max_seq_len"):
        m.generate(p, 1024 - 40 + 1, lengths=lens)
    with pytest.raises(ValueError, match="out of range"):
        bad = prompt.clone()
        bad[2, 30] = 50257  # a padding id outside the vocabulary
        m.generate(bad.cuda(), 4, lengths=lens)


# ------------------------------------------------------------------------------------------------ 5. the generator front end
class Tok:
    eos_token_id = None

    def encode(self, s):
        return [int(t) for t in s.split()]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def test_generator_batches_ragged_prompts(gpt2):
    from pytorch_models.text import GPT, DecoderGenerator

    m, _, prompt, oracle = gpt2
    lens, n_new = RC.GPT2_LENGTHS, RC.GPT2_NEW
    gen = DecoderGenerator(m, Tok())
    prompts = [prompt[b, :n].tolist() for b, n in enumerate(lens)]
    base = gen.generate_ids_batch(prompts, max_tokens=n_new)
    margin_at = lambda b, t: oracle[b][1][0, t - lens[b]]  # noqa: E731
    _obeys([torch.tensor(r) for r in base], [w[0] for w, _ in oracle], margin_at, lens, 2e-4, "generate_ids_batch", most=len(lens))
    assert gen.generate_ids_batch(prompts, max_tokens=n_new, prefill=True)[0][: lens[0]] == prompts[0]
    assert gen.generate_batch([Tok().decode(p) for p in prompts], max_tokens=n_new) == [Tok().decode(r) for r in base]
    assert base[2] == gen.generate_ids(prompts[2], max_tokens=n_new)  # the one-token row: generate_ids' own run
    # an eos the first row emits mid-row: that row ends with it (kept), the others are cut where they emit it themselves, if at all
    new0 = base[0][lens[0] :]
    j = next(i for i in range(3, n_new) if new0[i] not in new0[:i])
    eos = new0[j]
    cut = gen.generate_ids_batch(prompts, max_tokens=n_new, eos_token_id=eos)
    assert cut[0] == base[0][: lens[0] + j + 1] and cut[0][-1] == eos
    for b in (1, 2):
        new = base[b][lens[b] :]
        assert cut[b] == base[b][: lens[b] + (new.index(eos) + 1 if eos in new else n_new)]
    # a model without the KV-cached step (post-norm GPT): generate_ids per row, never a refusal
    g = GPT(n_layers=2, d_model=128)
    fill_module(g, 74)
    bf16_round_(g)
    g = g.to(torch.bfloat16).cuda().eval()
    gg = DecoderGenerator(g, Tok())
    short = [prompts[0][:5], prompts[1][:3], prompts[2]]
    assert gg.generate_ids_batch(short, max_tokens=4) == [gg.generate_ids(p, max_tokens=4) for p in short]
