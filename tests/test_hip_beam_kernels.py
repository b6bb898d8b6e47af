"""GPU: the three beam-step kernels (csrc/decode_beam.hip) on their own - pm_dec_beam_topw + pm_dec_beam_select against the
float64 step reference of tests/beam_cases.py (ids, parents and flags equal, scores within the bound derived from the kernel's
summation shape, on inputs whose decisions are >= 100 bounds apart), exact ties by the tie rule, prompt forcing, and the
in-place re-gathers of token histories and K / V caches bit for bit."""
import pytest
import torch

import beam_cases as BC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
D = 16  # width of the embedding rows the select kernel writes for the next step


def _state(B, W, V, t, P, seed, Ttot=None):
    """device-side state of one step at position t: random histories, embedding and position tables"""
    g = torch.Generator().manual_seed(1000 + seed)
    R = B * W
    Ttot = Ttot or t + 3
    tokens = torch.randint(0, V, (R, Ttot), generator=g)
    prompt = tokens[:, :P].clone()
    emb = (torch.randn(V, D, generator=g)).to(torch.bfloat16)
    pos_tab = torch.randn(Ttot, D, generator=g)
    return dict(tokens=tokens.cuda(), prompt=prompt.cuda(), tok_cur=torch.zeros(R, dtype=torch.int64).cuda(), emb=emb.cuda(),
                pos_tab=pos_tab.cuda(), x=torch.full((R, D), float("nan")).cuda(), ticket=torch.zeros(1, dtype=torch.int32).cuda(),
                pos=torch.tensor([t], dtype=torch.int32).cuda(), parents=torch.full((B, W), -1, dtype=torch.int32).cuda())


def _step(logits, scores, finished, eos, t=5, P=2, seed=0, cands=None):
    """topw + select on the device -> (parents, tokens chosen, scores, finished, state before, state after)"""
    from pytorch_models._hip import ops

    B, W = scores.shape
    V = logits.shape[1]
    st = _state(B, W, V, t, P, seed)
    before = {k: v.clone() for k, v in st.items()}
    sc, fin = scores.clone().cuda(), finished.to(torch.int32).cuda()
    if cands is None:
        cands = ops.dec_beam_topw(logits.cuda(), sc, fin, st["pos"], P, eos)
    ops.dec_beam_select(cands[0], cands[1], sc, fin, st["parents"], st["tokens"], st["pos"], st["prompt"], st["tok_cur"], st["emb"],
                        st["pos_tab"], st["x"], st["ticket"], eos)
    torch.cuda.synchronize()
    return st["parents"].cpu().long(), st["tokens"][:, t + 1].cpu().view(B, W), sc.cpu(), fin.cpu().bool(), before, st


def _check_tail(par, tok, before, st, t):
    """what select does besides choosing: histories re-gathered bit for bit, the new token appended, tok_cur, the next x rows
    (bf16 embedding row + f32 position row: one exact f32 add per element), the position moved and the ticket back at 0"""
    B, W = par.shape
    rows = (par + torch.arange(B)[:, None] * W).reshape(-1)
    assert torch.equal(st["tokens"][:, : t + 1].cpu(), before["tokens"].cpu()[rows, : t + 1])
    assert torch.equal(st["tokens"][:, t + 2 :].cpu(), before["tokens"][:, t + 2 :].cpu())
    assert torch.equal(st["tok_cur"].cpu(), tok.reshape(-1))
    want_x = st["emb"].cpu().float()[tok.reshape(-1)] + st["pos_tab"].cpu()[t + 1]
    assert torch.equal(st["x"].cpu(), want_x)
    assert int(st["pos"].item()) == t + 1 and int(st["ticket"].item()) == 0


def _inputs(kind, B, W, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * W, V, generator=g) * 3.0
    scores = -torch.rand(B, W, generator=g).sort(-1).values * 3.0
    finished = torch.zeros(B, W, dtype=torch.bool)
    eos = None
    if kind == "mixed":  # some rows finished (every clip keeps a live row when it has more than one)
        eos = 3
        finished = torch.rand(B, W, generator=g) < 0.4
        if W > 1:
            finished[:, -1] = False
            finished[0, 0] = True
    elif kind == "first":  # the first generated position: only beam 0 is live
        scores = torch.full((B, W), BC.NEG_INF)
        scores[:, 0] = 0.0
    elif kind == "neginf":  # what the rules leave: masked entries, and one row masked altogether
        logits[torch.rand(B * W, V, generator=g) < 0.3] = BC.NEG_INF
        if W > 1:
            logits[1] = BC.NEG_INF
    elif kind == "eoswins":  # a finished row on top, and a live row whose best continuation is eos
        eos = V - 1
        finished[:, 0] = True
        logits[W - 1 :: W, eos] = 30.0
    return logits, scores, finished, eos


CASES = [(1, 1, 70), (2, 2, 300), (3, 5, 1000), (2, 4, 51865), (8, 8, 257)]


@pytest.mark.parametrize("kind", ["plain", "mixed", "first", "neginf", "eoswins"])
@pytest.mark.parametrize("B,W,V", CASES, ids=lambda v: str(v))
def test_topw_and_select_match_the_float64_step(B, W, V, kind):
    for seed in range(64):  # inputs are BUILT to be decidable: the first seed whose decisions are >= 100 bounds apart
        logits, scores, finished, eos = _inputs(kind, B, W, V, seed)
        want = BC.step_ref(scores, finished, logits, W, eos)
        bound = BC.logits_bound(logits, scores, V)
        if BC.min_separation(want[4]) >= 100 * bound:
            break
    sep = BC.min_separation(want[4])
    assert sep >= 100 * bound, (sep, bound)  # in float64, before anything is compared
    t = 5
    par, tok, sc, fin, before, st = _step(logits, scores, finished, eos, t=t, seed=seed)
    w_par, w_tok, w_sc, w_fin, _ = want
    err = (sc.double() - w_sc)
    err = float(torch.where(torch.isnan(err), torch.zeros_like(err), err).abs().max())  # -inf against -inf
    print(f"{kind} B={B} W={W} V={V} seed={seed}: separation {sep:.3e}, bound {bound:.3e}, score error {err:.3e}")
    assert torch.equal(par, w_par) and torch.equal(tok, w_tok) and torch.equal(fin, w_fin)
    assert torch.equal(torch.isinf(sc), torch.isinf(w_sc)) and err <= bound
    if kind == "eoswins":
        assert bool((tok[:, 0] == eos).all()) and bool(fin[:, 0].all())
    if kind == "first":
        assert bool((par == 0).all()) and all(len(set(r.tolist())) == W for r in tok)
    _check_tail(par, tok, before, st, t)


def test_exact_ties_follow_the_tie_rule():
    """two bit-identical rows with equal scores, equal logits inside a row: lower parent beam first, then lower token id"""
    W, V = 3, 300
    for hot, want_par, want_tok in (((5, 17, 200), [0, 0, 0], [5, 17, 200]), ((5, 17), [0, 0, 1], [5, 17, 5])):
        logits = torch.zeros(W, V)
        logits[:2, list(hot)] = 2.0
        logits[2] = torch.randn(V)
        scores = torch.tensor([[-1.0, -1.0, -30.0]])
        par, tok, sc, fin, before, st = _step(logits, scores, torch.zeros(1, W, dtype=torch.bool), None)
        w_par, w_tok, w_sc, _, _ = BC.step_ref(scores, torch.zeros(1, W), logits, W, None)
        assert par[0].tolist() == want_par == w_par[0].tolist() and tok[0].tolist() == want_tok == w_tok[0].tolist()
        assert float(sc[0, 0]) == float(sc[0, 1]) == float(sc[0, 2])  # the same arithmetic on the same bits
        assert float((sc.double() - w_sc).abs().max()) <= BC.logits_bound(logits, scores, V)
        _check_tail(par, tok, before, st, 5)
    # every continuation at -inf (a clip whose rows are all masked): tokens 0 .. W - 1 of beam 0, by the same rule
    logits = torch.full((W, V), BC.NEG_INF)
    scores = torch.tensor([[-1.0, -2.0, -3.0]])
    par, tok, sc, *_ = _step(logits, scores, torch.zeros(1, W, dtype=torch.bool), None)
    w_par, w_tok, *_ = BC.step_ref(scores, torch.zeros(1, W), logits, W, None)
    assert torch.equal(par, w_par) and torch.equal(tok, w_tok) and par[0].tolist() == [0, 0, 0] and tok[0].tolist() == [0, 1, 2]
    assert bool(torch.isinf(sc).all())


def test_prompt_positions_are_forced_with_identity_parents():
    B, W, V, P, t = 2, 4, 100, 4, 1  # t + 1 < P
    logits = torch.randn(B * W, V)
    scores = torch.full((B, W), BC.NEG_INF)
    scores[:, 0] = 0.0
    finished = torch.zeros(B, W, dtype=torch.bool)
    par, tok, sc, fin, before, st = _step(logits, scores, finished, 7, t=t, P=P)
    assert torch.equal(par, torch.arange(W).expand(B, W))
    assert torch.equal(sc, scores) and not bool(fin.any())
    assert torch.equal(tok.reshape(-1), before["prompt"][:, t + 1].cpu())
    _check_tail(par, tok, before, st, t)


def _cands_for(parents, W):
    """candidates whose survivors are exactly (parents[b][j], token 10 + j) in order j"""
    B = len(parents)
    cs = torch.full((B * W, W), BC.NEG_INF)
    ct = torch.arange(W, dtype=torch.int32).repeat(B * W, 1)
    for b, par in enumerate(parents):
        used = [0] * W
        for j, p in enumerate(par):
            cs[b * W + p, used[p]] = -float(j)
            ct[b * W + p, used[p]] = 10 + j
            used[p] += 1
    return cs.cuda(), ct.cuda()


PARENTS4 = ([0, 0, 0, 0], [1, 0, 3, 2], [3, 3, 0, 1], [0, 1, 2, 3])
PARENTS5 = ([4, 0, 0, 2, 1],)


@pytest.mark.parametrize("t", [0, 9])
@pytest.mark.parametrize("pattern", PARENTS4 + PARENTS5, ids=lambda p: "".join(map(str, p)))
def test_token_histories_are_regathered_in_place(pattern, t):
    W = len(pattern)
    other = PARENTS4[2] if W == 4 else list(range(W))  # the second clip moves differently (W = 5: stays, the early return)
    parents = [list(pattern), list(other)]
    scores = torch.zeros(2, W)
    par, tok, sc, fin, before, st = _step(torch.zeros(2 * W, 50), scores, torch.zeros(2, W, dtype=torch.bool), None, t=t,
                                          P=1, cands=_cands_for(parents, W))
    assert par.tolist() == parents and tok.tolist() == [[10 + j for j in range(W)]] * 2
    assert sc.tolist() == [[-float(j) for j in range(W)]] * 2
    _check_tail(par, tok, before, st, t)


@pytest.mark.parametrize("dtype,rows,H,Tmax,t", [(torch.bfloat16, 8, 2, 40, 0), (torch.bfloat16, 10, 6, 24, 23), (torch.float32, 8, 2, 40, 17)],
                         ids=["bf16-t0", "bf16-last", "f32"])
def test_cache_reorder_is_bitwise_and_leaves_later_positions(dtype, rows, H, Tmax, t):
    from pytorch_models._hip import ops

    patterns = PARENTS4 if rows == 8 else PARENTS5 + ([0, 1, 2, 3, 4], [2, 2, 2, 2, 2])
    W = len(patterns[0])
    B = rows // W
    ibits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for k, pattern in enumerate(patterns):
        parents = torch.tensor([list(pattern), list(patterns[(k + 1) % len(patterns)])][:B], dtype=torch.int32)
        g = torch.Generator().manual_seed(k)
        # three layers = six caches of random BITS (NaN patterns included: the copy is not arithmetic)
        lim = 2 ** 15 if ibits == torch.int16 else 2 ** 31
        caches = [torch.randint(-lim, lim, (rows, H, Tmax, 64), generator=g).to(ibits).cuda().view(dtype) for _ in range(6)]
        before = [c.clone().view(ibits).cpu() for c in caches]
        ops.dec_beam_reorder(caches, parents.cuda(), torch.tensor([t + 1], dtype=torch.int32).cuda())
        src = (parents.long() + torch.arange(B)[:, None] * W).reshape(-1)
        for c, b4 in zip(caches, before):
            got = c.view(ibits).cpu()
            assert torch.equal(got[:, :, : t + 1], b4[src][:, :, : t + 1]), (pattern, "moved rows")
            assert torch.equal(got[:, :, t + 1 :], b4[:, :, t + 1 :]), (pattern, "positions above t")
