"""GPU: the four CTC kernels (csrc/ctc.hip) through ops.ctc_head / ctc_greedy / ctc_forward / ctc_viterbi on the cases of
tests/ctc_cases.py.
  * head: logp within MARGIN = 1.5 x the derived per-element bound of the float64 reference (operands in padded buffers, 3e38 in
    their padding, NaN-patterned pad columns of logp untouched), best exact wherever the reference's gap exceeds the margin and on
    every row of the exact family, best_logp = logp[m, best] bit for bit;
  * greedy: ids, n, start equal the numpy collapse, path_logp within its summation bound;
  * forward: within the derived bound of the float64 alpha recursion on the same fp32 logp, exactly -inf when infeasible, exactly
    0.0 / -inf on the one-hot families; * viterbi: start, stop, score EQUAL the float32 loop;
  * both: a clip's outputs are bit-identical alone and at every position of a batch of 5 whose other rows are NaN.
No number measured on a kernel enters an assertion; each test prints the figure it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

import ctc_cases as cc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_REF = {}
NAN_BITS = 0x7FC12345
POISON = 3e38


def _ops():
    from pytorch_models._hip import ops

    return ops


def _head_ref(case):
    """inputs and float64 reference of a head case, computed once and shared (never modified)"""
    if case.id not in _REF:
        h, w, b = cc.head_build(case)
        _REF[case.id] = (h, w, b, cc.head_reference(h, w, b))
    return _REF[case.id]


def _run_head(h, w, b, pad_l: int):
    """ops.ctc_head on operands inside poisoned padded buffers -> (logp, best, best_logp) on the CPU; checks the pad columns"""
    M, K = h.shape
    V = w.shape[0]
    hbuf = torch.full((M + 8, K + 16), POISON, dtype=torch.bfloat16, device="cuda")
    wbuf = torch.full((V + 8, K + 24), POISON, dtype=torch.bfloat16, device="cuda")
    hs, ws = hbuf[4 : 4 + M, 8 : 8 + K], wbuf[4 : 4 + V, 16 : 16 + K]
    hs.copy_(h)
    ws.copy_(w)
    lbuf = torch.full((M, V + pad_l), NAN_BITS, dtype=torch.int32, device="cuda")
    out = lbuf.view(torch.float32)[:, :V]
    logp, best, blp = _ops().ctc_head(hs, ws, None if b is None else b.cuda(), out=out)
    torch.cuda.synchronize()
    assert logp.data_ptr() == out.data_ptr()
    assert bool((lbuf[:, V:] == NAN_BITS).all()), "a pad column of logp was written"
    return logp.cpu().clone(), best.cpu().clone(), blp.cpu().clone()


@pytest.mark.parametrize("case", cc.head_cases(), ids=lambda c: c.id)
def test_head_parity_with_the_fp64_reference(case):
    h, w, b, ref = _head_ref(case)
    logp, best, blp = _run_head(h, w, b, 8 if case.M % 2 else 5)
    r = cc.ratio(logp, ref.logp, ref.logp_bound)
    exact = ref.gap > ref.margin
    print(f"RATIO {case.id}: logp {r:.3f} of the bound (asserted <= {cc.MARGIN}); rows under the exact arg-max rule {int(exact.sum())}/{case.M}")
    assert r <= cc.MARGIN
    assert float((~exact).double().mean()) <= cc.EXCLUDED_CAP or case.family == "exact"
    assert bool(((best >= 0) & (best < case.V)).all())
    assert torch.equal(best.long()[exact], ref.best[exact])
    if case.family == "exact":
        assert torch.equal(best.long(), ref.best), "integer logits: the arg-max is exact, ties to the lowest index"
    assert torch.equal(blp.view(torch.int32), logp.gather(1, best.long()[:, None])[:, 0].view(torch.int32))


def test_head_rows_do_not_depend_on_their_place():
    case = cc.HeadCase("scale1", 130, 29, 136, True)
    h, w, b, _ = _head_ref(case)
    base = _run_head(h, w, b, 3)
    p = torch.randperm(case.M, generator=torch.Generator().manual_seed(11))
    perm = _run_head(h[p], w, b, 3)
    head = _run_head(h[:17].contiguous(), w, b, 4)  # another M and the 16-byte store path
    for a, q, c in zip(base, perm, head):
        assert torch.equal(a[p].view(torch.int32), q.view(torch.int32)) and torch.equal(a[:17].view(torch.int32), c.view(torch.int32))


def test_head_refusals():
    ops = _ops()
    h = torch.zeros((4, 16), dtype=torch.bfloat16, device="cuda")
    for V, K in ((1, 16), (257, 16)):
        with pytest.raises(ValueError):
            ops.ctc_head(h[:, :K], torch.zeros((V, K), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        ops.ctc_head(h[:, :12].contiguous(), torch.zeros((8, 12), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        ops.ctc_head(h.float(), torch.zeros((8, 16), dtype=torch.bfloat16, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------- greedy
@pytest.mark.parametrize("name", list(cc.greedy_batches()))
def test_greedy_is_the_numpy_collapse(name):
    ops = _ops()
    clips = cc.greedy_batches()[name]
    frames = [len(c) for c in clips]
    packed = torch.from_numpy(np.concatenate(clips)).cuda()
    g = torch.Generator().manual_seed(5)
    blp = -10 * torch.rand(len(packed), generator=g)
    seq = ops.seq_lens(frames, 300, "cuda")
    ids, n, start, path = [t.cpu() for t in ops.ctc_greedy(packed, seq, blp.cuda(), 0)]
    assert ids.shape == start.shape == (len(clips), 300) and ids.dtype == start.dtype == n.dtype == torch.int32
    r0 = 0
    for b, a in enumerate(clips):
        want, wf = cc.collapse(a, 0)
        k = len(want)
        assert int(n[b]) == k and np.array_equal(ids[b, :k].numpy(), want) and np.array_equal(start[b, :k].numpy(), wf), (name, b)
        assert bool((ids[b, k:] == -1).all()) and bool((start[b, k:] == -1).all())
        seg = blp[r0 : r0 + len(a)].numpy()
        err, bound = abs(float(path[b]) - float(seg.astype(np.float64).sum())), cc.path_bound(seg)
        print(f"RATIO greedy {name} clip {b} (T={len(a)}): path_logp error {err:.3e}, bound {bound:.3e}")
        assert err <= cc.MARGIN * bound
        r0 += len(a)
    ids2, n2, start2, none = ops.ctc_greedy(packed, seq, None, 0)
    assert none is None and torch.equal(ids2.cpu(), ids) and torch.equal(n2.cpu(), n) and torch.equal(start2.cpu(), start)


# ------------------------------------------------------------------------------------------------------------------- recursion
def _rec_ref(case):
    if case.id not in _REF:
        lp, tgt = cc.rec_logp(case), cc.rec_target(case.kind, case.U)
        _REF[case.id] = (lp, tgt, cc.alpha_reference(lp, tgt, cc.REC_BLANK), cc.viterbi_reference(lp, tgt, cc.REC_BLANK))
    return _REF[case.id]


def _batch(clips, pad_ids=(10 ** 6, -5)):
    """clips: [(logp (T, V) f32 numpy, target)] -> (packed logp on the device, seq, targets int32 on the device right-padded with
    out-of-range ids, target lengths)"""
    ops = _ops()
    frames = [lp.shape[0] for lp, _ in clips]
    Umax = max(len(t) for _, t in clips)
    tg = torch.empty((len(clips), Umax), dtype=torch.int32)
    for b, (_, t) in enumerate(clips):
        tg[b] = torch.tensor([pad_ids[(b + u) % 2] for u in range(Umax)], dtype=torch.int32)
        tg[b, : len(t)] = torch.as_tensor(np.asarray(t, dtype=np.int32))
    lp = torch.from_numpy(np.concatenate([lp for lp, _ in clips]).astype(np.float32)).cuda()
    return lp, ops.seq_lens(frames, max(frames), "cuda", lo=1), tg.cuda(), [len(t) for _, t in clips]


@pytest.mark.parametrize("case", cc.rec_cases(), ids=lambda c: c.id)
def test_forward_and_viterbi_against_their_references(case):
    ops = _ops()
    lp, tgt, (ll, bound), (s0, s1, sc) = _rec_ref(case)
    logp, seq, tg, tl = _batch([(lp, tgt)])
    got = float(ops.ctc_forward(logp, seq, tg, tl, cc.REC_BLANK).cpu()[0])
    start, stop, score = [t.cpu() for t in ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)]
    if np.isfinite(ll):
        err = abs(got - ll)
        print(f"RATIO {case.id}: loglik {got:.6f} vs {ll:.6f}: error {err:.3e} = {err / bound:.3f} of the bound (asserted <= {cc.MARGIN})")
        assert np.isfinite(got) and err <= cc.MARGIN * bound
    else:
        assert got == -np.inf, "an infeasible pair gives exactly -inf"
    assert np.array_equal(start[0].numpy(), s0) and np.array_equal(stop[0].numpy(), s1), "the path differs from the float32 loop"
    assert np.float32(score[0]).tobytes() == np.float32(sc).tobytes()
    if not np.isfinite(ll):
        assert float(score[0]) == -np.inf and bool((start == -1).all()) and bool((stop == -1).all())
    else:
        assert float(score[0]) <= got + cc.MARGIN * bound


@pytest.mark.parametrize("frames,target,is_collapse", cc.ONE_HOT)
def test_one_hot_families_are_exact(frames, target, is_collapse):
    ops = _ops()
    logp, seq, tg, tl = _batch([(cc.one_hot_logp(frames), target + [7] * (3 - len(target)))])
    tl = [len(target)]
    got = float(ops.ctc_forward(logp, seq, tg, tl, cc.REC_BLANK).cpu()[0])
    start, stop, score = [t.cpu() for t in ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)]
    want = 0.0 if is_collapse else -np.inf
    assert got == want and float(score[0]) == want
    s0, s1, _ = cc.viterbi_reference(cc.one_hot_logp(frames), target, cc.REC_BLANK)
    assert np.array_equal(start[0, : len(target)].numpy(), s0) and np.array_equal(stop[0, : len(target)].numpy(), s1)


def test_an_all_minus_inf_column_gives_no_nan():
    ops = _ops()
    c = cc.RecCase("random", 33, 100)
    lp = cc.rec_logp(c).copy()
    tgt = cc.rec_target(c.kind, c.U)
    lp[:, int(tgt[5])] = -np.inf  # a label of the target can never be emitted: the pair has probability 0
    lp2 = cc.rec_logp(c).copy()
    lp2[:, 8] = -np.inf  # a label the second target does not use: its likelihood stays finite
    tgt2 = np.where(tgt > 6, 1, tgt)
    logp, seq, tg, tl = _batch([(lp, tgt), (lp2, tgt2)])
    got = ops.ctc_forward(logp, seq, tg, tl, cc.REC_BLANK).cpu()
    _, _, score = ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(score).any())
    assert float(got[0]) == -np.inf and float(score.cpu()[0]) == -np.inf
    ll, bound = cc.alpha_reference(lp2, tgt2, cc.REC_BLANK)
    assert np.isfinite(ll) and abs(float(got[1]) - ll) <= cc.MARGIN * bound


def test_viterbi_tie_rule_on_constant_logp():
    ops = _ops()
    clips = []
    for T, tgt in ((10, [3, 4, 4]), (16, [2, 2]), (17, [1, 2, 3, 4]), (33, [5]), (7, [])):
        clips.append((np.full((T, cc.REC_V), np.float32(-2.0)), tgt))
    logp, seq, tg, tl = _batch(clips)
    start, stop, score = [t.cpu() for t in ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)]
    for b, (lp, tgt) in enumerate(clips):
        s0, s1, sc = cc.viterbi_reference(lp, tgt, cc.REC_BLANK)
        assert np.array_equal(start[b, : len(tgt)].numpy(), s0) and np.array_equal(stop[b, : len(tgt)].numpy(), s1), (b, start[b], s0)
        assert float(score[b]) == float(sc) and bool((start[b, len(tgt) :] == -1).all())
    assert (start[0, :3].tolist(), stop[0, :3].tolist()) == ([0, 1, 3], [1, 2, 4])


@pytest.mark.parametrize("T", [cc.WORD_FRAMES - 1, cc.WORD_FRAMES, cc.WORD_FRAMES + 1, 2 * cc.WORD_FRAMES - 1, 2 * cc.WORD_FRAMES, 2 * cc.WORD_FRAMES + 1])
def test_back_pointer_words_at_their_edges(T):
    """T around the 16 frames of a word, S = 2 U + 1 = 3, 5, 7, 9 around the 4 and 8 states of one and two threads"""
    ops = _ops()
    clips = []
    for U in (1, 2, 3, 4):
        c = cc.RecCase("random", U, T)
        g = np.random.default_rng(10 * T + U)
        clips.append((cc.rec_logp(c), g.integers(1, cc.REC_V, U)))
    logp, seq, tg, tl = _batch(clips)
    start, stop, score = [t.cpu() for t in ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)]
    for b, (lp, tgt) in enumerate(clips):
        s0, s1, sc = cc.viterbi_reference(lp, tgt, cc.REC_BLANK)
        assert np.array_equal(start[b, : len(tgt)].numpy(), s0) and np.array_equal(stop[b, : len(tgt)].numpy(), s1) and float(score[b]) == float(sc)


def test_ragged_batch_and_position_independence():
    """ragged T_b and U_b in one batch, out-of-range ids in the target padding; clip b alone (a launch with B = 1), in the ragged
    batch of 5 and at every position of a batch of 5 whose other clips are NaN: the same bits"""
    ops = _ops()
    picks = [cc.RecCase("random", 33, 100), cc.RecCase("random", 129, 1000), cc.RecCase("repeat", 2, 3), cc.RecCase("random", 0, 100),
             cc.RecCase("repeat", 31, 64)]
    clips = [(cc.rec_logp(c), cc.rec_target(c.kind, c.U)) for c in picks]
    logp, seq, tg, tl = _batch(clips)
    ll = ops.ctc_forward(logp, seq, tg, tl, cc.REC_BLANK).cpu()
    start, stop, score = [t.cpu() for t in ops.ctc_viterbi(logp, seq, tg, tl, cc.REC_BLANK)]
    for b, (lp, tgt) in enumerate(clips):
        want, bound = cc.alpha_reference(lp, tgt, cc.REC_BLANK)
        s0, s1, sc = cc.viterbi_reference(lp, tgt, cc.REC_BLANK)
        print(f"RATIO ragged clip {b} ({picks[b].id}): {abs(float(ll[b]) - want) / bound:.3f} of the bound")
        assert abs(float(ll[b]) - want) <= cc.MARGIN * bound
        assert np.array_equal(start[b, : len(tgt)].numpy(), s0) and np.array_equal(stop[b, : len(tgt)].numpy(), s1) and float(score[b]) == float(sc)
        assert bool((start[b, len(tgt) :] == -1).all()) and bool((stop[b, len(tgt) :] == -1).all())
    for b, (lp, tgt) in enumerate(clips):  # every clip ALONE (B = 1): the bits it has in the ragged batch of 5
        lg, sq, t1, l1 = _batch([(lp, tgt)])
        ll1 = ops.ctc_forward(lg, sq, t1, l1, cc.REC_BLANK).cpu()
        s1, e1, c1 = [t.cpu() for t in ops.ctc_viterbi(lg, sq, t1, l1, cc.REC_BLANK)]
        assert ll1.shape == c1.shape == (1,) and s1.shape == e1.shape == (1, len(tgt))
        assert ll1[0].view(torch.int32) == ll[b].view(torch.int32) and c1[0].view(torch.int32) == score[b].view(torch.int32), b
        assert torch.equal(s1[0], start[b, : len(tgt)]) and torch.equal(e1[0], stop[b, : len(tgt)]), b
    for b in (0, 2, 4):
        lp, tgt = clips[b]
        nan = (np.full((5, cc.REC_V), np.nan, dtype=np.float32), [1])
        for pos in range(5):
            batch = [nan] * pos + [(lp, tgt)] + [nan] * (4 - pos)
            lg, sq, t2, l2 = _batch(batch)
            ll2 = ops.ctc_forward(lg, sq, t2, l2, cc.REC_BLANK).cpu()
            s2, e2, c2 = [t.cpu() for t in ops.ctc_viterbi(lg, sq, t2, l2, cc.REC_BLANK)]
            assert ll2[pos].view(torch.int32) == ll[b].view(torch.int32) and c2[pos].view(torch.int32) == score[b].view(torch.int32)
            assert torch.equal(s2[pos, : len(tgt)], start[b, : len(tgt)]) and torch.equal(e2[pos, : len(tgt)], stop[b, : len(tgt)])


def test_recursion_refusals():
    ops = _ops()
    lp = torch.zeros((4, cc.REC_V), device="cuda")
    seq = ops.seq_lens([4], 4, "cuda", lo=1)
    t = torch.ones((1, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.ctc_forward(lp, seq, torch.ones((1, 512), dtype=torch.int32, device="cuda"), [2])
    with pytest.raises(ValueError):
        ops.ctc_forward(lp, seq, t, [3])
    with pytest.raises(ValueError):
        ops.ctc_forward(lp, seq, t, [2], blank=cc.REC_V)
    with pytest.raises(ValueError):
        ops.ctc_viterbi(lp, ops.seq_lens([3], 4, "cuda", lo=1), t, [2])
    with pytest.raises(ValueError):
        ops.ctc_forward(lp, seq, t.long(), [2])
    assert ops.ctc_ws_bytes(2, 17, 3) == 2 * 2 * 2 * 16
