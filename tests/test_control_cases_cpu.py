"""No GPU: the reference of the repetition controls and the finish rule (tests/control_cases.py) pinned on hand-written examples and
against a brute-force n-gram set, the argument checks of pytorch_models._hip.controls, and the case selection: everything the GPU
suites (tests/test_hip_control_kernels.py, tests/test_hip_controls.py) take for granted is shown here from the oracle alone."""
import math
import random

import pytest
import torch

import control_cases as C
import sample_cases as S

torch.set_grad_enabled(False)
INF = math.inf


def _row(*vals):
    return torch.tensor(vals, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------ reference
def test_penalty_hits_every_distinct_id_once():
    l = _row(2.0, -2.0, 0.0, 4.0, -INF, 1.0)
    out = C.apply_controls(l, [0, 0, 0, 1, 1, 4, 0], 0, C.Ctl(r=2.0))
    assert out.tolist() == [1.0, -4.0, 0.0, 4.0, -INF, 1.0]  # id 0 three times: 2 / 2 once, not 2 / 8
    out = C.apply_controls(l, [3, 3], 0, C.Ctl(r=0.5))
    assert out.tolist() == [2.0, -2.0, 0.0, 8.0, -INF, 1.0]
    r = C.f32(1.3)
    out = C.apply_controls(l, [5, 1], 0, C.Ctl(r=1.3))
    assert out[5] == torch.tensor(1.0) / r and out[1] == torch.tensor(-2.0) * r and out[0] == 2.0
    # signed zeros, NaN and ids outside the vocabulary
    z = C.apply_controls(_row(0.0, -0.0, float("nan")), [0, 1, 2, 7, -1], 0, C.Ctl(r=3.0))
    assert math.copysign(1, float(z[0])) == 1 and math.copysign(1, float(z[1])) == -1 and math.isnan(float(z[2]))


def test_ngram_ban_by_hand():
    assert C.banned([5, 6, 7, 5, 6], 3) == {7}
    assert C.banned([5, 6, 7, 5, 6], 2) == {7}            # the open 1-gram (6) was followed by 7
    assert C.banned([5, 6, 5, 7, 5], 2) == {6, 7}
    assert C.banned([1, 2, 3], 1) == {1, 2, 3}            # n = 1 bans the whole history
    assert C.banned([1, 2], 4) == set()                   # n - 1 = 3 longer than the history
    assert C.banned([1, 2, 3], 4) == set()                # m = n - 1: the open gram is the whole history, nothing completes it yet
    assert C.banned([1, 1, 1], 2) == {1} and C.banned([1], 2) == set() and C.banned([9], 1) == {9}
    assert C.banned([4, 4, 4, 4], 0) == set()
    out = C.apply_controls(_row(1, 2, 3, 4), [0, 1, 0], 1, C.Ctl(r=2.0, n=2))
    assert out.tolist() == [0.5, -INF, 3.0, 4.0]          # the ban wins over the penalty


def test_ngram_ban_equals_the_brute_force_set():
    rng = random.Random(5)
    for _ in range(400):
        hist = [rng.randrange(4) for _ in range(rng.randrange(1, 24))]
        for n in range(0, C.MAX_NGRAM + 1):
            assert C.banned(hist, n) == C.brute_banned(hist, n), (hist, n)
            if n >= 1:  # the invariant the ban buys: appending any id that is NOT banned creates no repeated n-gram at the end
                grams = {tuple(hist[i:i + n]) for i in range(len(hist) - n + 1)}
                for v in range(4):
                    again = len(hist) >= n - 1 and tuple((hist + [v])[len(hist) + 1 - n:]) in grams
                    assert again == (v in C.banned(hist, n)), (hist, n, v)


def test_min_new_tokens_and_the_finish_rule():
    l = _row(1, 2, 3)
    assert C.apply_controls(l, [0], 1, C.Ctl(min_new=2, eos=2)).tolist() == [1, 2, -INF]
    assert C.apply_controls(l, [0], 2, C.Ctl(min_new=2, eos=2)).tolist() == [1, 2, 3]
    # a scripted stream: P = 2, eos = 9 in the prompt (no finish), then generated at position 3 (the second new token)
    toks, lps, fin = [9, 1, 4, 9, 5, 9, 6], [0.0, 0.0, -1.0, -2.0, -3.0, -4.0, -5.0], 0
    for t1 in range(1, 7):
        fin = C.finish_step(toks, lps, fin, t1, 2, 9, 7)
    assert fin == 3 and toks == [9, 1, 4, 9, 7, 7, 7] and lps == [0.0, 0.0, -1.0, -2.0, 0.0, 0.0, 0.0]
    toks, fin = [1, 2, 9, 3], 0  # eos at the first generated position
    for t1 in range(1, 4):
        fin = C.finish_step(toks, None, fin, t1, 2, 9, 0)
    assert fin == 2 and toks == [1, 2, 9, 0]
    assert C.cut_at_eos([4, 9, 5, 9], 9, 7) == ([4, 9, 7, 7], 2) and C.cut_at_eos([4, 5], 9, 7) == ([4, 5], 2)
    assert C.cut_at_eos([9, 5], 9, 7) == ([9, 7], 1) and C.cut_at_eos([4, 5], None, 7) == ([4, 5], 2)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_touch_no_device():
    from pytorch_models._hip.controls import MAX_NGRAM, check_controls, wants_logit_controls

    assert MAX_NGRAM == C.MAX_NGRAM
    assert check_controls("x", None, 0, 0, 1.0, 0) == (False, False) and not wants_logit_controls(0, 1.0, 0)
    assert check_controls("x", 5, 0, 0, 1.0, 0, vocab=10) == (True, False)
    assert check_controls("x", 5, 0, 2, 1.3, 3, vocab=10) == (True, True)
    assert check_controls("x", None, 0, 0, 1.0, 1, return_lengths=True) == (False, True)
    assert check_controls("x", 5, 0, 0, 1.0, 0, beams=3) == (False, False)  # beam search's own eos
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty=float("inf")), dict(repetition_penalty=1e-60), dict(repetition_penalty="a"),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=MAX_NGRAM + 1), dict(no_repeat_ngram_size=1.5),
                dict(min_new_tokens=-1), dict(min_new_tokens=2), dict(min_new_tokens=True)):
        kw = dict(eos_token_id=None, pad_token_id=0, min_new_tokens=0, repetition_penalty=1.0, no_repeat_ngram_size=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_controls("x", **kw)
    for eos, pad in ((10, 0), (-1, 0), (3, 10), (3, -1)):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            check_controls("x", eos, pad, 0, 1.0, 0, vocab=10)
    with pytest.raises(ValueError, match="beams=1"):
        check_controls("x", None, 0, 0, 1.3, 0, beams=2)
    with pytest.raises(ValueError, match="beams=1"):
        check_controls("x", 3, 0, 0, 1.0, 0, return_lengths=True, beams=2)
    with pytest.raises(ValueError, match="margins=False"):
        check_controls("x", None, 0, 0, 1.0, 2, margins=True)
    assert check_controls("x", 3, 0, 0, 1.0, 0, vocab=10, margins=True) == (True, False)  # eos alone keeps the margins
    for kw, match in ((dict(path="persistent"), "launches"), (dict(kv32=True), "exact=False"), (dict(fp32=True), "bfloat16")):
        with pytest.raises(NotImplementedError, match=match):
            check_controls("x", 3, 0, 0, 1.0, 0, **kw)


def test_generate_signatures_carry_the_new_keywords_with_their_defaults():
    import inspect

    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.generate import GreedyDecoder, POLL_EVERY, greedy_decode
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from pytorch_models.text import GPT2
    from pytorch_models.text.generator import DecoderGenerator

    want = dict(eos_token_id=None, pad_token_id=0, return_lengths=False, min_new_tokens=0, repetition_penalty=1.0, no_repeat_ngram_size=0)
    for fn in (GPT2.generate, Whisper.generate, WhisperDecoder.generate, greedy_decode):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want, fn
    sig = inspect.signature(GreedyDecoder.__init__).parameters
    assert [sig[k].default for k in ("eos", "min_new_tokens", "repetition_penalty", "no_repeat_ngram_size")] == [None, 0, 1.0, 0]
    for fn in (DecoderGenerator.generate_ids, DecoderGenerator.generate_ids_batch, DecoderGenerator.generate, DecoderGenerator.generate_batch):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in ("min_new_tokens", "repetition_penalty", "no_repeat_ngram_size")] == [0, 1.0, 0], fn
    assert POLL_EVERY == 32


# ------------------------------------------------------------------------------------------------------------- case selection
def test_plain_runs_repeat_a_2gram_so_the_ban_bites():
    _, rows, margins = C.gpt2_plain()
    assert all(C.has_repeat(r, C.NGRAM) for r in rows) and C.unclear_share(margins, 1.0) <= S.EDGE_CAP
    assert all(C.has_repeat(r, C.NGRAM) for r in C.gpt2_plain(True)[1])
    assert all(C.has_repeat(r, C.NGRAM) for r in C.whisper_plain(True, True)[1])
    assert any(C.has_repeat(r, C.NGRAM) for r in C.whisper_plain(False)[1])


def test_the_eos_finishes_every_row_at_a_different_position_before_the_end():
    cases = (([C.gpt2_plain()[1][b][23:] for b in C.GPT2_EOS_ROWS], C.gpt2_eos(), 21947),
             ([r[4:] for r in C.whisper_plain(False)[1]], C.whisper_eos(False), 48078),
             ([r[4:] for r in C.whisper_plain(True, True)[1]], C.whisper_eos(True), 12433))
    for rows, eos, recorded in cases:
        assert eos == recorded
        at = [r.index(eos) for r in rows]
        assert len(set(at)) == len(at) and max(at) < C.N - 1, at
    # the uncut plain runs that the eos runs are compared with are clear of near-ties (the GPU's arg-max is the oracle's)
    assert C.unclear_share(C.whisper_plain(False)[2], 1.0) <= S.EDGE_CAP and C.unclear_share(C.whisper_plain(True, True)[2], 1.0) <= S.EDGE_CAP


@pytest.mark.parametrize("name", list(C.RUNS))
def test_controlled_runs_stay_inside_the_cap_by_the_reference_alone(name):
    prompt, c, rows, margins = C.run_case(name)
    P = prompt.shape[1]
    share = C.unclear_share(margins, c.r)
    print(f"{name}: {c}: {share:.3f} of {margins.numel()} positions within {C.margin_bound(c.r):.3f} of a tie (cap {S.EDGE_CAP})")
    assert share <= S.EDGE_CAP
    if c.n:
        assert not any(C.has_repeat(r, c.n) for r in rows), "the reference's own run repeats an n-gram"
    if c.min_new:
        for r in rows:
            assert c.eos not in r[P:P + c.min_new]
        assert min(C.cut_at_eos(r[P:], c.eos, C.PAD)[1] for r in rows) < C.N  # some row still finishes: the eos run is not vacuous
    plain = C.gpt2_plain(True)[1] if name.startswith("gpt2") else C.whisper_plain(True, True)[1]
    assert rows != plain, "the controls change nothing on this prompt"


def test_the_sampled_controlled_run_is_clear_of_its_draw_edges():
    _, rows, edges = C.sampled_case()
    unclear = int((edges <= S.DRAW_MARGIN).sum())
    print(f"sampled run under {C.SAMPLED_CTL}, seed {C.SAMPLED_SEED}: {unclear} of {edges.numel()} positions unclear, smallest edge {float(edges.min()):.3e}")
    assert unclear <= S.EDGE_CAP * edges.numel() and not any(C.has_repeat(r, C.NGRAM) for r in rows)
