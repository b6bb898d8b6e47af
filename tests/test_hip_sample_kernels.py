"""GPU: pm_dec_sample / pm_dec_sample_ragged (csrc/sample.hip) through the C ABI on explicit state, against the float64 reference of
tests/sample_cases.py.  The table is sample_cases.kept(): every case is clear of its decision edges by the reference alone, so
  * the token must EQUAL the reference's (tok_cur, the written column of tokens_out; every other column keeps its sentinel);
  * the log-probability lies within MARGIN = 1.5 x the bound derived in sample_cases (the worst ratio is printed), is never NaN,
    and only its column t + 1 is written;
  * the next row x is emb[token] + pos[t + 1] (ragged: pos[max(0, t + 1 - key_start)]) bit for bit, the position advanced, the ticket 0;
  * a second launch on the same state gives the same bits;
  * logits sit in rows of ldl > V floats whose unused columns hold NaN.
At temperature 1, top_p 1, topk = k the token equals pm_dec_sample_topk's on the same state for every seed tried; the refusals
of the C entry points come before any launch."""
import pytest
import torch

import sample_cases as S
from pytorch_models._hip import decode_plan as plan
from pytorch_models._hip import lib, ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")
GROUPS = sorted({(c.family, c.V, c.B) for c in S.cases()})


def _state(c, inp, with_lp=True):
    """the launch's operands on the device: logits in rows of ldl > V with NaN behind them, sentinels in every output"""
    B, V = c.B, c.V
    ldl = V + 3
    buf = torch.full((B, ldl), float("nan"), device=DEV)
    buf[:, :V] = inp["logits"].to(DEV)
    st = dict(logits=buf[:, :V], pos=torch.tensor([c.pos], dtype=torch.int32, device=DEV), prompt=inp["prompt"].to(DEV),
              tok_cur=torch.full((B,), -7, dtype=torch.int64, device=DEV), tokens=torch.full((B, c.Ttot), -7, dtype=torch.int64, device=DEV),
              logprobs=torch.full((B, c.Ttot), 123.0, device=DEV) if with_lp else None, emb=inp["emb"].to(DEV),
              postab=inp["postab"].to(DEV), x=torch.full((B, c.d), float("nan"), device=DEV),
              ticket=torch.zeros(1, dtype=torch.int32, device=DEV), key_start=inp["key_start"].to(DEV))
    return st


def _launch(c, st, seed, topk=None, temperature=None, top_p=None):
    L = lib()
    k, T, p = (c.topk if topk is None else topk), (c.temperature if temperature is None else temperature), (c.top_p if top_p is None else top_p)
    head = (st["logits"], k, T, p, seed, st["pos"], st["prompt"], st["tok_cur"], st["tokens"], st["logprobs"], st["emb"], st["postab"])
    if c.ragged:
        plan.call(L.pm_dec_sample_ragged, plan.ragged_sample_args(*head, st["key_start"], st["x"], st["ticket"]))
    else:
        plan.call(L.pm_dec_sample, plan.sample_args(*head, st["x"], st["ticket"]))
    torch.cuda.synchronize()


def _bits(st):
    return [st[n].clone() for n in ("tok_cur", "tokens", "logprobs", "x", "pos", "ticket")]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}-V{g[1]}-B{g[2]}")
def test_token_equals_reference_and_logprob_is_inside_its_bound(group):
    worst, n = 0.0, 0
    for c in S.kept():
        if (c.family, c.V, c.B) != group:
            continue
        inp = S.build(c)
        for i, seed in enumerate(inp["seeds"]):
            want = S.expected(c, inp, seed)
            st = _state(c, inp)
            _launch(c, st, seed)
            t1 = c.pos + 1
            got = st["tok_cur"].cpu()
            assert torch.equal(got, want["next"]), f"{c.id} seed {seed}: tokens {got.tolist()} reference {want['next'].tolist()}"
            toks = st["tokens"].cpu()
            assert torch.equal(toks[:, t1], want["next"]) and bool((toks[:, :t1] == -7).all()) and bool((toks[:, t1 + 1:] == -7).all()), c.id
            lp = st["logprobs"].cpu()
            assert bool((lp[:, :t1] == 123.0).all()) and bool((lp[:, t1 + 1:] == 123.0).all()), f"{c.id}: log-prob written outside its column"
            col = lp[:, t1].double()
            assert not bool(torch.isnan(col).any()), f"{c.id}: NaN log-prob"
            fin = torch.isfinite(want["logprob"])
            assert torch.equal(col[~fin], want["logprob"][~fin]), c.id  # a forced token under a -inf logit: -inf exactly
            if fin.any():
                worst = max(worst, float(((col[fin] - want["logprob"][fin]).abs() / want["bound"][fin]).max()))
            assert torch.equal(st["x"].cpu(), want["x"]), f"{c.id}: the next step's row"
            assert int(st["pos"]) == want["pos"] and int(st["ticket"]) == 0, c.id
            if i == 0:  # the same state again: the same bits; and without a log-prob buffer the same token
                first = _bits(st)
                st2 = _state(c, inp)
                _launch(c, st2, seed)
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, _bits(st2))), f"{c.id}: two launches differ"
                st3 = _state(c, inp, with_lp=False)
                _launch(c, st3, seed)
                assert torch.equal(st3["tok_cur"], st["tok_cur"]), c.id
            n += 1
    print(f"RATIO {group}: {n} launches, worst log-prob error {worst:.3f} of the bound (asserted <= {S.MARGIN})")
    assert n > 0 and worst <= S.MARGIN


@pytest.mark.parametrize("family,B,V", [("planted", 3, 1000), ("gauss", 3, 1000), ("planted", 3, 50257), ("planted", 64, 257), ("neginf", 3, 257)])
def test_topk_at_temperature_one_is_pm_dec_sample_topk(family, B, V):
    """temperature 1, top_p 1, topk = k: the same token as pm_dec_sample_topk on the same state - for every seed, no margin: both
    sides form the same fp32 sums in the same order"""
    n = 0
    for k in (1, 2, 50, 64):
        if k > V:
            continue
        c = S.Case(family, B, V, k, 1.0, 1.0)
        inp = S.build(c)
        for seed in list(range(S.SEED0, S.SEED0 + 24)) + [2 ** 63 + 5, 2 ** 64 - 1]:
            st = _state(c, inp)
            _launch(c, st, seed)
            ref = _state(c, inp)
            ops.dec_sample_topk(ref["logits"], k, seed, ref["pos"], ref["prompt"], ref["tok_cur"], ref["tokens"], ref["emb"], ref["postab"],
                                ref["ticket"])
            torch.cuda.synchronize()
            assert torch.equal(st["tok_cur"], ref["tok_cur"]) and torch.equal(st["tokens"], ref["tokens"]), (family, k, seed)
            n += 1
    print(f"{family} B={B} V={V}: {n} launches equal pm_dec_sample_topk's token")


def test_the_draw_is_ignored_at_a_forced_position_and_keyed_by_the_seed():
    c = S.Case("gauss", 3, 1000, 0, 1.0, 1.0)
    inp = S.build(c)
    seen = set()
    for seed in range(16):
        st = _state(c, inp)
        _launch(c, st, seed)
        seen.add(tuple(st["tok_cur"].tolist()))
    assert len(seen) > 8, "sixteen seeds must not give the same three tokens"
    forced = S.Case("gauss", 3, 1000, 0, 1.0, 1.0, pos=1, P=4)
    inp = S.build(forced)
    for seed in (1, 2):
        st = _state(forced, inp)
        _launch(forced, st, seed)
        assert torch.equal(st["tok_cur"].cpu(), inp["prompt"][:, 2]) and int(st["pos"]) == 2


def test_refusals_come_before_any_launch():
    L = lib()
    c = S.Case("planted", 3, 257, 0, 0.7, 0.9)
    inp = S.build(c)
    st = _state(c, inp)
    before = _bits(st)
    good = list(plan.sample_args(st["logits"], 0, 0.7, 0.9, 1, st["pos"], st["prompt"], st["tok_cur"], st["tokens"], st["logprobs"], st["emb"],
                                 st["postab"], st["x"], st["ticket"]))
    good[-1] = torch.cuda.current_stream().cuda_stream
    EINVAL = 1

    def rc(**at):
        a = list(good)
        for i, v in at.items():
            a[int(i[1:])] = v
        return L.pm_dec_sample(*a)

    # argument positions: 0 logits 1 ldl 2 V 3 topk 4 temperature 5 top_p 6 seed 7 pos 8 prompt 9 P 10 tok_cur 11 tokens 12 Ttot 13 logprobs
    # 14 emb 15 pos table 16 x 17 d 18 ticket 19 B
    for i in (0, 7, 8, 10, 11, 14, 15, 16, 18):
        assert rc(**{f"a{i}": None}) == EINVAL, f"null argument {i}"
    for at in (dict(a2=0), dict(a2=-5), dict(a1=100), dict(a3=-1), dict(a3=65), dict(a4=-0.5), dict(a4=float("nan")), dict(a4=float("inf")),
               dict(a5=0.0), dict(a5=1.5), dict(a5=float("nan")), dict(a5=-1.0), dict(a17=28), dict(a17=0), dict(a19=0)):
        assert rc(**at) == EINVAL, at
    rag = list(plan.ragged_sample_args(st["logits"], 0, 0.7, 0.9, 1, st["pos"], st["prompt"], st["tok_cur"], st["tokens"], st["logprobs"],
                                       st["emb"], st["postab"], st["key_start"], st["x"], st["ticket"]))
    rag[-1] = good[-1]
    rag[16] = None
    assert L.pm_dec_sample_ragged(*rag) == EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, _bits(st))), "a refused call wrote"
    assert rc(a13=None) == 0  # the log-prob buffer is optional
    torch.cuda.synchronize()
    assert int(st["pos"]) == c.pos + 1 and bool((st["logprobs"] == 123.0).all())
    assert EINVAL == 1 and L.pm_strerror(EINVAL)


@pytest.mark.parametrize("form", ("plain", "ragged", "topk"))
def test_wrapper_honours_or_refuses_every_operand_layout(form):
    """tests/wrapper_cases.py's layout machinery on the new wrapper (which lives outside ops.py): every variant of every operand is
    refused cleanly or accepted with the bits of the contiguous call"""
    import wrapper_cases as WC
    from pytorch_models._hip import sampling

    r = S.wrapper_rows()[form]
    try:
        problems, accepted = WC.check_row(sampling, r, DEV, compare=True)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"dec_sample {form}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    print(f"dec_sample {form}: {len(accepted)} variants accepted bit-identically or refused cleanly; {len(problems)} problems")
    assert accepted and not problems, "\n".join([f"{len(problems)} problems:"] + problems)
