"""GPU: audio.Wav2Vec2CTC end to end - Wav2Vec2CTC(Wav2Vec2(2, 128), 32) on synthweights, waves (4, 9600) with lengths
[9600, 6400, 4000, 400] (29 .. 1 frames): log_probs against ops.ctc_head on forward's own rows (bit for bit) and against the fp32
oracle per clip alone (rel-L2 <= 2e-2, the contract tests/test_hip_audio_enc.py puts on these encoders), decode against the
collapse of its own arg-max, score against float64 ctc_loss on the returned log_probs within the kernel bound, align against the
float32 loop, the refusals, the untouched Wav2Vec2.forward(x, lengths=) and the CPU module path.  Bounds: tests/ctc_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_cases as cc
from oracle import ref_audio as RA
from synthweights import bf16_round_, fill_module, synth_input

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def rel(got, want):
    got, want = got.double().cpu(), want.double()
    return ((got - want).norm() / want.norm()).item()


@pytest.fixture(scope="module")
def ctc():
    from pytorch_models.audio import Wav2Vec2

    cpu, sd = cc.model_ctc()
    m, _ = cc.model_ctc()
    m = m.to(torch.bfloat16).cuda().eval()
    x = synth_input("ctc_wave", (4, 9600), 81)
    frames = [Wav2Vec2.frame_length(n) for n in cc.MODEL_LENGTHS]
    lp = m.log_probs(x.cuda(), lengths=cc.MODEL_LENGTHS)
    return m, cpu, sd, x, frames, lp


def _ctc_loss64(logp: torch.Tensor, target) -> float:
    loss = F.ctc_loss(logp.double()[:, None, :], torch.as_tensor(target, dtype=torch.int64)[None, :], torch.tensor([logp.shape[0]]),
                      torch.tensor([len(target)]), blank=0, reduction="none")
    return -float(loss[0])


def test_log_probs_without_lengths_is_the_head_on_forwards_rows(ctc):
    from pytorch_models._hip import ops
    from pytorch_models.transformer import _f32

    m, _, _, x, _, _ = ctc
    xc = x.cuda()
    h = m.encoder(xc)
    want, _, _ = ops.ctc_head(h.reshape(-1, h.shape[-1]), m.lm_head.weight, _f32(m.lm_head, "b", m.lm_head.bias))
    got = m.log_probs(xc)
    assert got.shape == (4, 29, cc.MODEL_V) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(4, 29, cc.MODEL_V).view(torch.int32))
    assert torch.equal(m(xc), got)


def test_log_probs_against_the_oracle_per_clip_alone(ctc):
    m, _, sd, x, frames, lp = ctc
    assert lp.shape == (4, 29, cc.MODEL_V) and lp.dtype == torch.float32
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    W, b = sd["lm_head.weight"].float(), sd["lm_head.bias"].float()
    for i, (n, f) in enumerate(zip(cc.MODEL_LENGTHS, frames)):
        rows = RA.wav2vec2(enc, x[i : i + 1, :n])[0].float()
        assert rows.shape[0] == f
        want = torch.log_softmax(rows @ W.T + b, -1)
        r = rel(lp[i, :f], want)
        print(f"REL ctc log_probs clip {i} ({n} samples, {f} frames) {r:.3e} (asserted < 2e-2)")
        assert r < 2e-2
        assert bool((lp[i, f:] == 0).all()), "padded frames must be exactly 0"
        alone = m.log_probs(x[i : i + 1, :n].cuda())
        assert alone.shape == (1, f, cc.MODEL_V) and rel(alone[0], want) < 2e-2


def test_decode_is_the_collapse_of_its_own_arg_max(ctc):
    m, _, _, x, frames, lp = ctc
    ids, n, start, path = [t.cpu() for t in m.decode(x.cuda(), lengths=cc.MODEL_LENGTHS)]
    assert ids.shape == start.shape == (4, 29) and ids.dtype == n.dtype == start.dtype == torch.int32 and path.dtype == torch.float32
    lpc = lp.cpu()
    for i, f in enumerate(frames):
        am = cc.lowest_argmax(lpc[i, :f]).numpy()
        want, wf = cc.collapse(am, 0)
        k = len(want)
        assert int(n[i]) == k and np.array_equal(ids[i, :k].numpy(), want) and np.array_equal(start[i, :k].numpy(), wf)
        assert bool((ids[i, k:] == -1).all()) and bool((start[i, k:] == -1).all())
        seg = lpc[i, :f].max(-1).values.numpy()
        assert abs(float(path[i]) - float(seg.astype(np.float64).sum())) <= cc.MARGIN * cc.path_bound(seg)


def test_score_and_align_against_their_references(ctc):
    """Two inequalities hold exactly only between exact values: score(align) <= score and, per clip,
    |score_batch - score_alone| <= sum_t max_v |d logp|.  The kernels' fp32 results each sit within their derived bound of the
    exact value on their own logp, so both are asserted with that slack ADDED on purpose: MARGIN x bound for the first (one
    forward result), MARGIN x (bound of the batch run + bound of the run alone) for the second.  Nothing else is widened.
    align is also given targets wider than max(target_lengths): its outputs keep the width passed in, -1 in the extra columns."""
    m, _, _, x, frames, lp = ctc
    t, tl = cc.model_targets()
    xc, lpc = x.cuda(), lp.cpu()
    score = m.score(xc, t, tl, lengths=cc.MODEL_LENGTHS).cpu()
    start, stop, vs = [v.cpu() for v in m.align(xc, t.cuda(), torch.tensor(tl), lengths=cc.MODEL_LENGTHS)]
    assert score.shape == vs.shape == (4,) and score.dtype == vs.dtype == torch.float32
    assert start.shape == stop.shape == (4, 6) and start.dtype == stop.dtype == torch.int32
    for i, f in enumerate(frames):
        tgt = t[i, : tl[i]].numpy()
        want, bound = cc.alpha_reference(lpc[i, :f].numpy(), tgt, 0)
        loss = _ctc_loss64(lpc[i, :f], tgt)
        assert abs(want - loss) <= 1e-12 * max(1.0, abs(loss))
        print(f"RATIO ctc score clip {i}: {float(score[i]):.6f} vs {loss:.6f}: {abs(float(score[i]) - loss) / bound:.3f} of the bound")
        assert abs(float(score[i]) - loss) <= cc.MARGIN * bound
        s0, s1, sc = cc.viterbi_reference(lpc[i, :f].numpy(), tgt, 0)
        assert np.array_equal(start[i, : tl[i]].numpy(), s0) and np.array_equal(stop[i, : tl[i]].numpy(), s1) and float(vs[i]) == float(sc)
        assert bool((start[i, tl[i] :] == -1).all()) and bool((stop[i, tl[i] :] == -1).all())
        assert float(vs[i]) <= float(score[i]) + cc.MARGIN * bound
        # alone: the likelihood moves by at most the largest per-frame change of logp, frame by frame (each kernel within its bound)
        n = cc.MODEL_LENGTHS[i]
        lp1 = m.log_probs(xc[i : i + 1, :n]).cpu()[0]
        s1_ = float(m.score(xc[i : i + 1, :n], t[i : i + 1], tl[i : i + 1]).cpu()[0])
        _, b1 = cc.alpha_reference(lp1.numpy(), tgt, 0)
        moved = float((lp1 - lpc[i, :f]).abs().max(-1).values.double().sum())
        print(f"ctc score clip {i}: batch {float(score[i]):.6f} alone {s1_:.6f}, sum_t max_v |d logp| = {moved:.3e}")
        assert abs(float(score[i]) - s1_) <= moved + cc.MARGIN * (bound + b1)
    wide = torch.cat([t, torch.full((4, 3), 99)], 1)  # three columns no clip uses, ids out of range in them
    w0, w1, wv = [v.cpu() for v in m.align(xc, wide, tl, lengths=cc.MODEL_LENGTHS)]
    assert w0.shape == w1.shape == (4, 9) and w0.dtype == w1.dtype == torch.int32
    assert torch.equal(w0[:, :6], start) and torch.equal(w1[:, :6], stop) and torch.equal(wv.view(torch.int32), vs.view(torch.int32))
    assert bool((w0[:, 6:] == -1).all()) and bool((w1[:, 6:] == -1).all())
    assert torch.equal(m.score(xc, wide, tl, lengths=cc.MODEL_LENGTHS).cpu().view(torch.int32), score.view(torch.int32))
    inf = m.score(xc, torch.tensor([[5, 5, 9, 1, 30, 2]] * 4), [6, 6, 6, 6], lengths=cc.MODEL_LENGTHS).cpu()
    assert torch.isfinite(inf[:3]).all() and float(inf[3]) == -np.inf, "one frame cannot carry six labels"


def test_refusals(ctc):
    from pytorch_models.audio import SEW, Wav2Vec2, Wav2Vec2CTC

    m, _, _, x, _, _ = ctc
    xc = x.cuda()
    t, tl = cc.model_targets()
    for bad_t, bad_l in ((torch.tensor([[0, 1]] * 4), [2] * 4), (torch.tensor([[32, 1]] * 4), [2] * 4), (torch.tensor([[-1, 1]] * 4), [2] * 4),
                         (t, [6, 4, 2]), (torch.ones((4, 600), dtype=torch.int64), [512, 1, 1, 1])):
        for fn in (m.score, m.align):
            with pytest.raises(ValueError):
                fn(xc, bad_t, bad_l, lengths=cc.MODEL_LENGTHS)
    m32 = Wav2Vec2CTC(Wav2Vec2(1, 128), 32).cuda().eval()
    for fn in (lambda: m32.log_probs(xc), lambda: m32.score(xc, t, tl, lengths=cc.MODEL_LENGTHS), lambda: m32.align(xc, t, tl)):
        with pytest.raises(NotImplementedError, match="bf16"):
            fn()
    sew = Wav2Vec2CTC(SEW(1, 128), 32).to(torch.bfloat16).cuda().eval()
    with pytest.raises(NotImplementedError, match="variable-length"):
        sew.log_probs(xc, lengths=cc.MODEL_LENGTHS)
    with pytest.raises(ValueError):
        m.log_probs(xc, lengths=[9600, 6400, 4000, 399])


@pytest.mark.parametrize("pre_norm", [True, False])
def test_forward_with_lengths_is_bit_for_bit_what_it_was(ctc, pre_norm):
    """Wav2Vec2._forward_lengths was split for the head (_packed_rows): its launches restated here as they stood, for both norm
    orders.  A guard on the split only - it calls the helpers _packed_rows calls; what forward(x, lengths=) COMPUTES is held by the
    unchanged tests/test_hip_varlen.py."""
    from pytorch_models._hip import ops
    from pytorch_models.audio import Wav2Vec2

    m, _, _, x, frames, _ = ctc
    e, xc = m.encoder, x.cuda()
    if not pre_norm:
        e = Wav2Vec2(1, 128, pre_norm=False).eval()
        fill_module(e, 87)
        bf16_round_(e)
        e = e.to(torch.bfloat16).cuda()
    h = e._features(xc)
    seq = ops.seq_lens(frames, h.shape[1], h.device, lo=1)
    pad = e.pe_conv[0].padding
    h = ops.rows_zero_tail(h, seq)
    h = ops.rows_pack(e.grouped_conv(e.pe_conv[1], h, (pad[0], pad[1]), "gelu", h), seq)
    if pre_norm:
        h = e.norm(e.layers.forward_packed(h, seq), e.norm.weight.dtype)
    else:
        h = e.layers.forward_packed(e.norm(h), seq).to(e.norm.weight.dtype)
    assert torch.equal(e(xc, lengths=cc.MODEL_LENGTHS), ops.rows_unpack(h, seq))


def test_a_sew_encoder_works_without_lengths():
    from pytorch_models.audio import SEW, Wav2Vec2CTC

    m = Wav2Vec2CTC(SEW(2, 128), 29, blank=28).eval()
    fill_module(m, 85)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    x = synth_input("w2v_x", (2, 6400), 81).cuda()
    lp = m.log_probs(x)
    T = m.encoder(x).shape[1]
    assert lp.shape == (2, T, 29) and bool(torch.isfinite(lp).all()) and float((lp.exp().sum(-1) - 1).abs().max()) < 1e-4
    ids, n, start, path = m.decode(x)
    for i in range(2):
        want, wf = cc.collapse(cc.lowest_argmax(lp[i].cpu()).numpy(), 28)
        assert int(n[i]) == len(want) and np.array_equal(ids[i, : len(want)].cpu().numpy(), want)
    sc = m.score(x, torch.tensor([[1, 2], [3, 3]]), [2, 2])
    s0, s1, vs = m.align(x, torch.tensor([[1, 2], [3, 3]]), [2, 2])
    assert bool(torch.isfinite(sc).all()) and bool((s0 < s1).all())
    for i, tgt in enumerate(([1, 2], [3, 3])):
        want, bound = cc.alpha_reference(lp[i].cpu().numpy(), tgt, 28)
        assert abs(float(sc[i]) - want) <= cc.MARGIN * bound and float(vs[i]) <= float(sc[i]) + cc.MARGIN * bound


def test_a_vocabulary_that_is_no_multiple_of_four_with_lengths(ctc):
    """29 columns: the packed log-probabilities are unpacked through rows padded to 32 floats; same bits as each clip alone"""
    from pytorch_models.audio import Wav2Vec2, Wav2Vec2CTC

    _, _, _, x, frames, _ = ctc
    m = Wav2Vec2CTC(Wav2Vec2(1, 128), 29, blank=28).eval()
    fill_module(m, 86)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    lp = m.log_probs(x.cuda(), lengths=cc.MODEL_LENGTHS)
    assert lp.shape == (4, 29, 29) and lp.dtype == torch.float32
    for i, (n, f) in enumerate(zip(cc.MODEL_LENGTHS, frames)):
        alone = m.log_probs(x[i : i + 1, :n].cuda())[0]
        assert torch.equal(lp[i, :f].contiguous().view(torch.int32), alone.contiguous().view(torch.int32)) and bool((lp[i, f:] == 0).all())
        assert float((lp[i, :f].exp().sum(-1) - 1).abs().max()) < 1e-4


def test_the_cpu_module_path_returns_the_same_shapes_and_dtypes(ctc):
    m, cpu, _, x, frames, lp = ctc
    t, tl = cc.model_targets()
    got = (lp, *m.decode(x.cuda(), lengths=cc.MODEL_LENGTHS), m.score(x.cuda(), t, tl, lengths=cc.MODEL_LENGTHS),
           *m.align(x.cuda(), t, tl, lengths=cc.MODEL_LENGTHS))
    want = (cpu.log_probs(x, lengths=cc.MODEL_LENGTHS), *cpu.decode(x, lengths=cc.MODEL_LENGTHS), cpu.score(x, t, tl, lengths=cc.MODEL_LENGTHS),
            *cpu.align(x, t, tl, lengths=cc.MODEL_LENGTHS))
    assert len(got) == len(want) == 9
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.is_cuda and not w.is_cuda
    r = rel(got[0], want[0])
    print(f"REL ctc log_probs HIP vs the CPU module path {r:.3e}")
    assert r < 2e-2
