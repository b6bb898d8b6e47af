"""CPU: the references, bounds and case tables of tests/ctc_cases.py hold together, and the plain-torch / numpy forms of
pytorch_models/_cpu.py and audio.Wav2Vec2CTC on the CPU agree with them.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_cases as cc

torch.set_grad_enabled(False)


def _ctc_loss64(logp: np.ndarray, target, blank: int) -> float:
    lp = torch.from_numpy(np.asarray(logp, dtype=np.float64))[:, None, :]
    t = torch.as_tensor(np.asarray(target, dtype=np.int64))[None, :]
    loss = F.ctc_loss(lp, t, torch.tensor([lp.shape[0]]), torch.tensor([len(target)]), blank=blank, reduction="none")
    return -float(loss[0])


def _close(a: float, b: float, rtol: float = 1e-12) -> bool:
    if not (np.isfinite(a) and np.isfinite(b)):
        return a == b
    return abs(a - b) <= rtol * max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("case", cc.rec_cases(), ids=lambda c: c.id)
def test_alpha_reference_is_ctc_loss_in_float64(case):
    lp, tgt = cc.rec_logp(case), cc.rec_target(case.kind, case.U)
    ll, bound = cc.alpha_reference(lp, tgt, cc.REC_BLANK)
    want = _ctc_loss64(lp, tgt, cc.REC_BLANK)
    assert _close(ll, want), (ll, want)
    assert np.isfinite(ll) == cc.feasible(tgt, case.T)
    assert bound >= 0 and (not np.isfinite(ll) or bound < 1e-2 * max(abs(ll), 1.0)), "the bound must mean something"
    _, _, score = cc.viterbi_reference(lp, tgt, cc.REC_BLANK)
    assert np.isfinite(score) == np.isfinite(ll)
    assert float(score) <= ll + 1e-6 * max(abs(ll), 1.0) if np.isfinite(ll) else score == -np.inf


def test_the_table_holds_the_edge_pairs():
    ids = {c.id for c in cc.rec_cases()}
    assert {"random-U0-T1", "random-U1-T1", "random-U511-T1000", "repeat-U2-T3", "repeat-U2-T2", "repeat-U511-T1000"} <= ids
    assert _ctc_loss64(np.full((1, 4), -1.0), [], 0) == -1.0 == cc.alpha_reference(np.full((1, 4), -1.0), [], 0)[0]  # T = 1, U = 0
    ll, _ = cc.alpha_reference(np.log(np.full((3, 4), 0.25)), [2, 2], 0)
    assert np.isfinite(ll) and _close(ll, _ctc_loss64(np.log(np.full((3, 4), 0.25)), [2, 2], 0))  # just feasible
    ll, _ = cc.alpha_reference(np.log(np.full((2, 4), 0.25)), [2, 2], 0)
    assert ll == -np.inf and _ctc_loss64(np.log(np.full((2, 4), 0.25)), [2, 2], 0) == -np.inf  # infeasible: both inf
    n_inf = sum(not cc.feasible(cc.rec_target(c.kind, c.U), c.T) for c in cc.rec_cases())
    assert n_inf >= 10 and len(cc.rec_cases()) - n_inf >= 40


@pytest.mark.parametrize("frames,target,is_collapse", cc.ONE_HOT)
def test_one_hot_families_are_exact(frames, target, is_collapse):
    lp = cc.one_hot_logp(frames)
    ids, _ = cc.collapse(np.asarray(frames), cc.REC_BLANK)
    assert (list(ids) == list(target)) == is_collapse
    ll, _ = cc.alpha_reference(lp, target, cc.REC_BLANK)
    assert ll == (0.0 if is_collapse else -np.inf)
    _, _, score = cc.viterbi_reference(lp, target, cc.REC_BLANK)
    assert score == (0.0 if is_collapse else -np.inf)
    got = _cpu().ctc_forward(torch.from_numpy(lp), [len(frames)], torch.tensor([target + [0] * (3 - len(target))], dtype=torch.int32),
                             [len(target)], cc.REC_BLANK)
    assert float(got[0]) == ll


def _cpu():
    from pytorch_models import _cpu

    return _cpu


def test_greedy_collapse_is_the_numpy_restatement():
    for name, clips in cc.greedy_batches().items():
        packed = torch.from_numpy(np.concatenate(clips))
        frames = [len(c) for c in clips]
        blp = -torch.rand(len(packed))
        ids, n, start, path = _cpu().ctc_greedy(packed, frames, 300, blp, 0)
        assert ids.dtype == n.dtype == start.dtype == torch.int32 and path.dtype == torch.float32
        r0 = 0
        for b, a in enumerate(clips):
            keep = (a != 0) & np.r_[True, a[1:] != a[:-1]][: len(a)]  # the restatement
            f = np.nonzero(keep)[0]
            want_ids, want_f = cc.collapse(a, 0)
            assert np.array_equal(want_ids, a[f]) and np.array_equal(want_f, f)
            k = len(f)
            assert int(n[b]) == k and np.array_equal(ids[b, :k].numpy(), a[f]) and np.array_equal(start[b, :k].numpy(), f), name
            assert bool((ids[b, k:] == -1).all()) and bool((start[b, k:] == -1).all())
            assert abs(float(path[b]) - float(blp[r0 : r0 + len(a)].double().sum())) <= 1e-4
            r0 += len(a)
    b = cc.greedy_batches()["boundaries"]
    assert len(cc.collapse(b[0], 0)[0]) == 2 and len(cc.collapse(b[1], 0)[0]) == 1 and len(cc.collapse(b[2], 0)[0]) == 1


def test_cpu_forms_agree_with_the_references():
    cases = [c for c in cc.rec_cases() if c.T <= 130 and c.U <= 129][::3]
    assert len(cases) >= 10
    frames = [c.T for c in cases]
    Umax = max(c.U for c in cases)
    tg = torch.zeros((len(cases), Umax), dtype=torch.int32)
    for b, c in enumerate(cases):
        tg[b, : c.U] = torch.from_numpy(cc.rec_target(c.kind, c.U)).to(torch.int32)
    lp = torch.from_numpy(np.concatenate([cc.rec_logp(c) for c in cases]))
    tl = [c.U for c in cases]
    ll = _cpu().ctc_forward(lp, frames, tg, tl, cc.REC_BLANK)
    start, stop, score = _cpu().ctc_viterbi(lp, frames, tg, tl, cc.REC_BLANK)
    assert ll.dtype == score.dtype == torch.float32 and start.dtype == stop.dtype == torch.int32 and start.shape == (len(cases), Umax)
    for b, c in enumerate(cases):
        t = cc.rec_target(c.kind, c.U)
        want, _ = cc.alpha_reference(cc.rec_logp(c), t, cc.REC_BLANK)
        assert _close(float(ll[b]), float(np.float32(want)), 1e-6), c.id
        s0, s1, sc = cc.viterbi_reference(cc.rec_logp(c), t, cc.REC_BLANK)
        assert np.array_equal(start[b, : c.U].numpy(), s0) and np.array_equal(stop[b, : c.U].numpy(), s1) and float(score[b]) == float(sc), c.id
        assert bool((start[b, c.U :] == -1).all()) and bool((stop[b, c.U :] == -1).all())
        if np.isfinite(sc) and c.U:
            assert bool((s0 < s1).all()) and bool((s1[:-1] <= s0[1:]).all()) and s0[0] >= 0 and s1[-1] <= c.T


def test_viterbi_tie_rule_on_constant_logp():
    """every comparison between reachable states ties: stay wins, then s - 1: the tokens sit as EARLY as the states allow"""
    lp = np.full((10, cc.REC_V), np.float32(-2.0))
    start, stop, score = cc.viterbi_reference(lp, [3, 4, 4], 0)
    assert score == np.float32(-20.0)
    # reachable states of one frame all hold the same score, so "stay" wins wherever the state was reachable the frame before: the
    # walk back leaves a state at the FIRST frame it could be reached (state 6 at frame 4 via 1 -> 3 -> 4 -> 5 -> 6; the two 4s
    # forbid the skip 3 -> 5), then s - 1 beats s - 2 on a tie and the -inf stay: 6, 5, 4, 3 at frames 4 .. 1, state 1 at frame 0
    assert (list(start), list(stop)) == ([0, 1, 3], [1, 2, 4])
    s2, e2, sc2 = _cpu().ctc_viterbi(torch.from_numpy(lp), [10], torch.tensor([[3, 4, 4]], dtype=torch.int32), [3], 0)
    assert np.array_equal(s2[0].numpy(), start) and np.array_equal(e2[0].numpy(), stop) and float(sc2[0]) == float(score)


@pytest.mark.parametrize("case", cc.head_cases(), ids=lambda c: c.id)
def test_head_case_table_meets_its_conditions(case):
    h, w, b = cc.head_build(case)
    ref = cc.head_reference(h, w, b)
    excluded = float((ref.gap <= ref.margin).double().mean())
    if case.family != "exact":
        assert excluded <= cc.EXCLUDED_CAP, (case.id, excluded)
    if case.family == "lead":
        assert bool((ref.gap > 104).all())
    if case.family == "exact":
        assert bool((ref.x == ref.x.round()).all()) and float(ref.x.abs().max()) < 2 ** 24
    assert bool(torch.isfinite(ref.logp_bound).all()) and bool((ref.logp_bound > 0).all())
    logp, best, blp = _cpu().ctc_head(h.float(), w.float(), b)
    assert logp.dtype == blp.dtype == torch.float32 and best.dtype == torch.int32
    assert float((logp.double() - ref.logp).abs().max()) < 1e-3 * max(1.0, float(ref.logp.abs().max()))
    ex = ref.gap > 1e-3
    assert torch.equal(best.long()[ex], ref.best[ex])
    if case.family == "exact":
        assert torch.equal(best.long(), ref.best)


def test_exact_family_has_ties():
    n = 0
    for c in cc.head_cases():
        if c.family == "exact":
            ref = cc.head_reference(*cc.head_build(c))
            n += int((ref.gap == 0).sum())
    assert n >= 20


def test_model_head_is_not_a_constant_and_the_loader_and_cpu_path_work(capsys):
    from pytorch_models.audio import Wav2Vec2, Wav2Vec2CTC
    from synthweights import synth_input

    m, sd = cc.model_ctc()
    assert Wav2Vec2CTC.frame_stride == 320
    # the 2e-2 contract means something on the oracle side: perturbing hidden rows by 2e-2 moves log-softmax by a like amount
    g = torch.Generator().manual_seed(3)
    hrows = torch.randn(61, 128, generator=g)
    W, b = sd["lm_head.weight"].float(), sd["lm_head.bias"].float()
    base = torch.log_softmax(hrows @ W.T + b, -1)
    pert = torch.log_softmax((hrows + 2e-2 * torch.randn(61, 128, generator=g)) @ W.T + b, -1)
    moved = float((pert - base).norm() / base.norm())
    spread = float((base - base.mean(-1, keepdim=True)).norm() / base.norm())
    print(f"head sensitivity: 2e-2 on the rows moves logp by {moved:.3e}; spread of logp around its row mean {spread:.3e}")
    assert moved > 2e-3 and spread > 0.1
    # CPU module path: same shapes and dtypes as the HIP one
    x = synth_input("ctc_wave", (4, 9600), 81)
    lp = m.log_probs(x, lengths=cc.MODEL_LENGTHS)
    frames = [Wav2Vec2.frame_length(n) for n in cc.MODEL_LENGTHS]
    assert lp.shape == (4, 29, cc.MODEL_V) and lp.dtype == torch.float32
    for bb, f in enumerate(frames):
        assert bool((lp[bb, f:] == 0).all()) and abs(float(lp[bb, :f].exp().sum(-1).mean()) - 1) < 1e-4
    ids, n, start, path = m.decode(x, lengths=cc.MODEL_LENGTHS)
    assert ids.shape == start.shape == (4, 29) and n.shape == path.shape == (4,)
    assert ids.dtype == n.dtype == start.dtype == torch.int32 and path.dtype == torch.float32
    for bb, f in enumerate(frames):
        want, wf = cc.collapse(lp[bb, :f].argmax(-1).numpy(), 0)
        assert int(n[bb]) == len(want) and np.array_equal(ids[bb, : len(want)].numpy(), want) and np.array_equal(start[bb, : len(want)].numpy(), wf)
    t, tl = cc.model_targets()
    sc = m.score(x, t, tl, lengths=cc.MODEL_LENGTHS)
    s0, s1, vs = m.align(x, t, tl, lengths=cc.MODEL_LENGTHS)
    assert sc.shape == vs.shape == (4,) and sc.dtype == vs.dtype == torch.float32 and s0.shape == s1.shape == (4, 6) and s0.dtype == torch.int32
    for bb, f in enumerate(frames):
        want = _ctc_loss64(lp[bb, :f].numpy(), t[bb, : tl[bb]].numpy(), 0)
        assert abs(float(sc[bb]) - want) <= 1e-4 * max(1.0, abs(want)) and float(vs[bb]) <= float(sc[bb]) + 1e-5
    assert m.log_probs(x[:2]).shape == (2, 29, cc.MODEL_V)
    # refusals
    for bad_t, bad_l in ((torch.tensor([[0, 1]] * 4), [2] * 4), (torch.tensor([[32, 1]] * 4), [2] * 4), (torch.tensor([[-1, 1]] * 4), [2] * 4),
                         (t, [6, 4, 2]), (torch.ones((4, 600), dtype=torch.int64), [512, 1, 1, 1])):
        with pytest.raises(ValueError):
            m.score(x, bad_t, bad_l, lengths=cc.MODEL_LENGTHS)
    # loader: a synthesised Wav2Vec2ForCTC state dict
    hf = _hf_ctc_state_dict(m)
    m2 = Wav2Vec2CTC.from_hf("synth/ctc", config=dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, conv_bias=True,
                                                       feat_extract_norm="layer", do_stable_layer_norm=True, vocab_size=cc.MODEL_V, pad_token_id=3))
    assert m2.blank == 3 and m2.vocab_size == cc.MODEL_V
    capsys.readouterr()
    m2.load_hf_state_dict(hf)
    assert capsys.readouterr().out.strip() == "dict_keys([])", "every key of the state dict must be used"
    for k, v in m.state_dict().items():
        assert torch.allclose(m2.state_dict()[k].float(), v.float(), atol=1e-6), k
    with pytest.raises(NotImplementedError):
        Wav2Vec2CTC.from_hf("synth/ctc")


def test_align_keeps_the_width_of_the_targets_passed_in():
    """targets wider than max(target_lengths): start / stop are (B, U) for the U passed in, -1 in the columns no clip uses"""
    from synthweights import synth_input

    m, _ = cc.model_ctc()
    x = synth_input("ctc_wave", (4, 9600), 81)
    t, tl = cc.model_targets()
    s0, s1, vs = m.align(x, t, tl, lengths=cc.MODEL_LENGTHS)
    wide = torch.cat([t, torch.full((4, 3), 99)], 1)  # ids out of range where no clip reads them
    w0, w1, wv = m.align(x, wide, tl, lengths=cc.MODEL_LENGTHS)
    assert w0.shape == w1.shape == (4, 9) and w0.dtype == w1.dtype == torch.int32
    assert torch.equal(w0[:, :6], s0) and torch.equal(w1[:, :6], s1) and torch.equal(wv, vs)
    assert bool((w0[:, 6:] == -1).all()) and bool((w1[:, 6:] == -1).all())
    assert torch.equal(m.score(x, wide, tl, lengths=cc.MODEL_LENGTHS), m.score(x, t, tl, lengths=cc.MODEL_LENGTHS))
    e0, e1, _ = m.align(x, torch.full((4, 2), 99), [0, 0, 0, 0], lengths=cc.MODEL_LENGTHS)
    assert e0.shape == e1.shape == (4, 2) and bool((e0 == -1).all()) and bool((e1 == -1).all())


def test_the_cpu_head_keeps_fp32_logits_for_a_bf16_module():
    """bf16 h, w, b on the CPU: the logits are formed in fp32 from the widened operands (as the kernel keeps them), not rounded to
    bf16 in front of the log-softmax and the arg-max"""
    from pytorch_models import _cpu

    g = torch.Generator().manual_seed(9)
    h = torch.randn(65, 72, generator=g).bfloat16()
    w = (4 * torch.randn(29, 72, generator=g)).bfloat16()
    b = torch.randn(29, generator=g).bfloat16()
    x = h.float() @ w.float().T + b.float()
    logp, best, blp = _cpu.ctc_head(h, w, b)
    assert logp.dtype == blp.dtype == torch.float32 and best.dtype == torch.int32
    assert torch.allclose(logp, torch.log_softmax(x, -1), rtol=0, atol=1e-5)
    assert torch.equal(best.long(), cc.lowest_argmax(x))
    rounded = torch.log_softmax(x.bfloat16().float(), -1)
    assert float((logp - rounded).abs().max()) > 1e-3, "the case must tell fp32 logits from bf16-rounded ones"


def _hf_ctc_state_dict(m) -> dict:
    """Hugging Face Wav2Vec2ForCTC names for the parameters of a Wav2Vec2CTC(Wav2Vec2) instance (weight-normed positional conv)"""
    e = m.encoder
    sd = {"lm_head.weight": m.lm_head.weight.clone(), "lm_head.bias": m.lm_head.bias.clone()}
    p = "wav2vec2."
    for i, blk in enumerate(e.feature_encoder):
        sd[f"{p}feature_extractor.conv_layers.{i}.conv.weight"] = blk[0].weight.clone()
        sd[f"{p}feature_extractor.conv_layers.{i}.conv.bias"] = blk[0].bias.clone()
        sd[f"{p}feature_extractor.conv_layers.{i}.layer_norm.weight"] = blk[2].weight.clone()
        sd[f"{p}feature_extractor.conv_layers.{i}.layer_norm.bias"] = blk[2].bias.clone()
    sd[p + "feature_projection.layer_norm.weight"] = e.proj[0].weight.clone()
    sd[p + "feature_projection.layer_norm.bias"] = e.proj[0].bias.clone()
    sd[p + "feature_projection.projection.weight"] = e.proj[1].weight.clone()
    sd[p + "feature_projection.projection.bias"] = e.proj[1].bias.clone()
    v = e.pe_conv[1].weight.clone()
    sd[p + "encoder.pos_conv_embed.conv.weight_v"] = v
    sd[p + "encoder.pos_conv_embed.conv.weight_g"] = v.float().pow(2).sum((0, 1), keepdim=True).sqrt().to(v.dtype)
    sd[p + "encoder.pos_conv_embed.conv.bias"] = e.pe_conv[1].bias.clone()
    sd[p + "encoder.layer_norm.weight"] = e.norm.weight.clone()
    sd[p + "encoder.layer_norm.bias"] = e.norm.bias.clone()
    from pytorch_models.converters import _W2V_LAYER

    for i, layer in enumerate(e.layers):
        for path, name in _W2V_LAYER:
            mod = layer.get_submodule(path)
            sd[f"{p}encoder.layers.{i}.{name}.weight"] = mod.weight.clone()
            sd[f"{p}encoder.layers.{i}.{name}.bias"] = mod.bias.clone()
    return sd
