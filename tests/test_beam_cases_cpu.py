"""CPU: the beam-search reference of tests/beam_cases.py is what the GPU tests take it for - W = 1 is the greedy loop, beams are
distinct and ordered, a score is the teacher-forced log-probability of its tokens - and, for the seeds the GPU tests use, its
decision gaps stay above the threshold under which a different summation order may decide differently (no GPU test skips)."""
import math

import pytest
import torch

import beam_cases as BC
from oracle import ref_whisper

torch.set_grad_enabled(False)


def test_step_reference_follows_the_tie_rule_and_the_finished_rule():
    V, W = 6, 2
    logits = torch.zeros(2 * W, V)  # clip 0: two identical rows, equal logits; clip 1: row 0 finished, eos = 4
    scores = torch.tensor([[0.0, 0.0], [-1.0, -1.0 - 0.5]])
    fin = torch.tensor([[False, False], [True, False]])
    logits[3] = torch.tensor([0.0, 3.0, 0.0, 0.0, 0.0, 0.0])
    par, tok, s, f, top = BC.step_ref(scores, fin, logits, W, 4)
    assert par[0].tolist() == [0, 0] and tok[0].tolist() == [0, 1]  # lowest flattened index first
    assert torch.allclose(s[0], torch.full((2,), -math.log(6.0), dtype=torch.float64))
    # clip 1: the finished row's single (eos, -1.0) candidate wins, then the live row's best
    assert par[1].tolist() == [0, 1] and tok[1].tolist() == [4, 1]
    assert s[1, 0] == -1.0 and f[1].tolist() == [True, False]
    par, tok, s, f, _ = BC.step_ref(torch.tensor([[0.0, BC.NEG_INF]]), torch.zeros(1, 2), torch.randn(2, V), W, None)
    assert par[0].tolist() == [0, 0] and tok[0, 0] != tok[0, 1]  # first generated position: W continuations of beam 0


@pytest.mark.parametrize("seed", BC.SEEDS)
def test_width_one_is_the_greedy_loop(seed):
    sd, _, prompt, memory, (toks, scores, parents, _) = BC.reference_case(seed, 1)
    want, _ = ref_whisper.greedy_recompute(sd, "decoder.", prompt, memory, BC.N_NEW)
    assert torch.equal(toks[:, 0], want)
    assert int(parents.max()) == 0 and bool((scores < 0).all())


@pytest.mark.parametrize("seed", BC.SEEDS)
@pytest.mark.parametrize("W", [4, 5])
def test_beams_are_distinct_ordered_and_scored_by_their_tokens(seed, W):
    sd, _, prompt, memory, (toks, scores, parents, gaps) = BC.reference_case(seed, W)
    B, P = prompt.shape
    assert toks.shape == (B, W, P + BC.N_NEW) and parents.shape == (BC.N_NEW, B, W)
    assert torch.equal(toks[:, :, :P], prompt[:, None].expand(-1, W, -1))
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    for b in range(B):
        assert len({tuple(t.tolist()) for t in toks[b]}) == W
    # teacher-forced: the same fp32 forward on the finished hypotheses; 12 log-probabilities whose logits another call shape
    # may sum in another order (a few fp32 ulp of |logit| <= 8 each, ~1e-5): 2e-4
    lp = torch.log_softmax(ref_whisper.decoder(sd, "decoder.", toks.view(B * W, -1), memory.repeat_interleave(W, 0)).double(), -1)
    tf = lp[:, P - 1 : -1].gather(-1, toks.view(B * W, -1)[:, P:, None])[..., 0].sum(-1).view(B, W)
    assert float((tf - scores).abs().max()) < 2e-4
    assert bool((parents[0] == 0).all())  # the first generated position continues beam 0 only


@pytest.mark.parametrize("seed", BC.SEEDS)
def test_the_gpu_tests_seeds_stay_clear_of_near_ties(seed):
    """tests/test_hip_beam.py compares tokens and parents of the exact=True path with this reference at W = 4: a decision
    closer than GAP_MIN could go either way between two fp32 summation orders, so the seeds in use must not have one."""
    *_, (toks, scores, parents, gaps) = BC.reference_case(seed, 4)
    print(f"seed {seed}: min decision gap {float(gaps.min()):.3e} (GAP_MIN {BC.GAP_MIN:.1e})")
    assert float(gaps.min()) >= BC.GAP_MIN


def test_eos_freezes_a_hypothesis():
    """with an eos that is reached, the hypothesis holds eos from there on and its score stops moving"""
    sd, _, prompt, memory, _ = BC.reference_case(BC.SEEDS[0], 4)
    free = BC.reference_case(BC.SEEDS[0], 4)[4][0]
    eos = int(free[0, 0, prompt.shape[1] + 2])  # a token the unconstrained best beam emits early
    toks, scores, _, _ = BC.ref_beam_search(sd, "decoder.", prompt, memory, BC.N_NEW, 4, eos)
    hit = False
    for row in toks.view(-1, toks.shape[-1]):
        gen = row[prompt.shape[1]:].tolist()
        if eos in gen:
            hit = True
            assert all(t == eos for t in gen[gen.index(eos):])
    assert hit
