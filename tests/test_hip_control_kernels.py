"""GPU: pm_dec_controls / pm_dec_finish (csrc/controls.hip) through the C ABI on explicit state, against the reference of
tests/control_cases.py.
  * the controlled logits are BIT-equal to the reference (torch's fp32 l / r and l * r on the CPU; NaN stays NaN): rows of -inf, +inf,
    +-0 and NaN mixed in, B 1 / 3 / 64, V 5 / 257 / 1000 / 50257 / 51865, histories of 1, 2, 63, 64, 65, 255, 256, 257 and 1024 ids (the
    kernel strides by its 256 threads; 64 is the wave), one id repeated / ids 0 and V - 1 / all distinct / random, n 0..4 and 8,
    r 1 / 1.3 / 0.5 / 10, min_new_tokens either side of its edge; quotients and products are normal, zero or infinite (no subnormals);
  * logits sit in rows of ldl > V floats whose unused columns hold a sentinel that must come back untouched;
  * a prompt-forced position changes nothing; the padding of a ragged batch is not history; a row does not depend on the others;
  * pm_dec_finish follows the reference step by step over a scripted stream, with and without a log-prob buffer;
  * eager launches equal a captured-graph replay, bit for bit; the refusals of the C entry points come before any launch;
  * the wrappers of pytorch_models._hip.controls honour or refuse every operand layout (tests/wrapper_cases.check_row)."""
import math

import pytest
import torch

import control_cases as C
from pytorch_models._hip import decode_plan as plan
from pytorch_models._hip import lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")
SENTINEL = 777.0
HLENS = (1, 2, 63, 64, 65, 255, 256, 257, 1024)
PATTERNS = ("one", "edges", "distinct", "random")
NS = (0, 1, 2, 3, 4, C.MAX_NGRAM)
RS = (1.0, 1.3, 0.5, 10.0)
BS, VS = (1, 3, 64), (5, 257, 1000, 50257, 51865)


def _logits(B, V, g):
    """normal values times 4 with -inf, +inf, +0, -0 and NaN planted (at least 1e-3 in magnitude otherwise: r <= 10 leaves them normal)"""
    lg = torch.randn(B, V, generator=g) * 4.0
    lg = torch.where(lg.abs() < 1e-3, torch.full_like(lg, 0.5), lg)
    special = torch.tensor([-math.inf, math.inf, 0.0, -0.0, float("nan")])
    for k, v in enumerate(special):
        cols = torch.randint(0, V, (B, max(1, V // 9)), generator=g)
        lg.scatter_(1, cols[:, k::5] if cols.shape[1] > k else cols[:, :1], float(v))
    return lg


def _history(pattern, B, m, V, g):
    if pattern == "one":
        return torch.randint(0, V, (B, 1), generator=g).expand(B, m).contiguous()
    if pattern == "edges":
        return torch.where(torch.rand(B, m, generator=g) < 0.5, 0, V - 1)
    if pattern == "distinct":  # all distinct while V allows, then the permutation again
        return torch.stack([torch.randperm(V, generator=g).repeat(-(-m // V))[:m] for _ in range(B)])
    return torch.randint(0, min(V, 7), (B, m), generator=g)  # few ids: n-grams repeat


def _launch(lg, tokens, pos, P, c, key_start=None):
    """the kernel on rows of ldl = V + 3 floats; returns the (B, V) result on the CPU after checking the sentinel columns"""
    B, V = lg.shape
    buf = torch.full((B, V + 3), SENTINEL, device=DEV)
    buf[:, :V] = lg.to(DEV)
    st = dict(tokens=tokens.to(DEV), pos=torch.tensor([pos], dtype=torch.int32, device=DEV),
              key_start=None if key_start is None else key_start.to(DEV))
    plan.call(lib().pm_dec_controls, plan.controls_args(buf[:, :V], st["tokens"], st["pos"], P, st["key_start"], repetition_penalty=c.r,
                                                        no_repeat_ngram=c.n, min_new_tokens=c.min_new, eos=c.eos))
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:, V:] == SENTINEL).all()), "columns >= V were written"
    assert torch.equal(st["tokens"].cpu(), tokens) and int(st["pos"]) == pos
    return out[:, :V].contiguous()


def _reference(lg, tokens, pos, P, c, key_start=None):
    out = lg.clone()
    if pos + 1 < P:
        return out
    for b in range(lg.shape[0]):
        s = 0 if key_start is None else min(max(int(key_start[b]), 0), pos)
        out[b] = C.apply_controls(lg[b], tokens[b, s : pos + 1].tolist(), pos + 1 - P, c)
    return out


def _same_bits(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN columns differ"
    a, b = got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]
    if not torch.equal(a, b):
        bad = (a != b).nonzero()[:4, 0].tolist()
        raise AssertionError(f"{what}: {int((a != b).sum())} values differ, e.g. {[(got[~nan][i].item(), want[~nan][i].item()) for i in bad]}")


def _case(B, V, m, pattern, n, r, edge, g):
    """history of m ids at positions 0 .. m - 1 (pos = m - 1), one prompt token; min_new_tokens on side ``edge`` of n_gen"""
    tokens = torch.full((B, m + 2), -5, dtype=torch.int64)
    tokens[:, :m] = _history(pattern, B, m, V, g)
    n_gen = m - 1
    return tokens, C.Ctl(r=r, n=n, min_new=max(0, n_gen + edge), eos=(V - 1, 0)[m % 2])


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_controlled_logits_are_bit_equal_to_the_reference(B, V):
    g = torch.Generator().manual_seed(1000 * B + V)
    lg = _logits(B, V, g)
    salt = BS.index(B) * len(VS) + VS.index(V)
    for i, m in enumerate(HLENS):  # every history length; the other settings take turns (each combination of (B, V) starts elsewhere)
        k = i + salt
        pattern, n, r, edge = PATTERNS[k % 4], NS[k % 6], RS[(k // 2) % 4], (0, 1)[k % 2]
        tokens, c = _case(B, V, m, pattern, n, r, edge, g)
        got = _launch(lg, tokens, m - 1, 1, c)
        _same_bits(got, _reference(lg, tokens, m - 1, 1, c), f"B={B} V={V} m={m} {pattern} {c}")


def test_every_setting_at_the_small_size():
    """B = 3, V = 257: every history length with every pattern, every n with every r either side of min_new_tokens' edge"""
    B, V = 3, 257
    g = torch.Generator().manual_seed(77)
    lg = _logits(B, V, g)
    n_launch = 0
    for i, m in enumerate(HLENS):
        for j, pattern in enumerate(PATTERNS):
            tokens, c = _case(B, V, m, pattern, NS[(i + j) % 6], RS[(i + 2 * j) % 4], (i + j) % 2, g)
            _same_bits(_launch(lg, tokens, m - 1, 1, c), _reference(lg, tokens, m - 1, 1, c), f"m={m} {pattern} {c}")
            n_launch += 1
    for n in NS:
        for r in RS:
            for edge in (0, 1):
                tokens, c = _case(B, V, 65, "random", n, r, edge, g)
                want = _reference(lg, tokens, 64, 1, c)
                _same_bits(_launch(lg, tokens, 64, 1, c), want, f"{c}")
                if edge:  # below the minimum length: the eos is out
                    assert bool((want[:, c.eos] == -math.inf).all())
                n_launch += 1
    # the penalty divides ONCE: an id 1024 times in the history
    tokens = torch.full((1, 1026), 3, dtype=torch.int64)
    one = torch.full((1, V), 8.0)
    got = _launch(one, tokens, 1023, 1, C.Ctl(r=2.0))
    assert float(got[0, 3]) == 4.0 and bool((got[0, :3] == 8.0).all()) and bool((got[0, 4:] == 8.0).all())
    print(f"{n_launch + 1} launches bit-equal")


def test_forced_positions_ragged_padding_and_row_independence():
    B, V, m = 3, 1000, 70
    g = torch.Generator().manual_seed(5)
    lg = _logits(B, V, g)
    tokens, c = _case(B, V, m, "random", 2, 1.3, 1, g)
    # prompt-forced: t + 1 < P - nothing changes, whatever is asked for
    _same_bits(_launch(lg, tokens, m - 1, m + 1, c), lg, "forced position")
    _same_bits(_launch(lg, tokens, m - 1, m, c), _reference(lg, tokens, m - 1, m, c), "the first generated position")
    assert not torch.equal(_reference(lg, tokens, m - 1, m, c).nan_to_num(), lg.nan_to_num())
    # ragged: ids 900 .. 999 sit only in the padding in front of key_start and must not count
    ks = torch.tensor([0, 37, 69], dtype=torch.int32)
    for b in range(B):
        tokens[b, : int(ks[b])] = torch.randint(900, 1000, (int(ks[b]),), generator=g)
    for c2 in (C.Ctl(r=10.0), C.Ctl(n=1), C.Ctl(r=0.5, n=3, min_new=3, eos=5)):
        got = _launch(lg, tokens, m - 1, m - 8, c2, ks)
        _same_bits(got, _reference(lg, tokens, m - 1, m - 8, c2, ks), f"ragged {c2}")
        for b in (1, 2):
            _same_bits(got[b, 900:], lg[b, 900:], f"ragged {c2}: the padding's ids were touched in row {b}")
        assert not torch.equal(_launch(lg, tokens, m - 1, m - 8, c2).nan_to_num(), got.nan_to_num()), "key_start changed nothing"
        # a row alone gives the row of the batch
        for b in range(B):
            alone = _launch(lg[b : b + 1], tokens[b : b + 1], m - 1, m - 8, c2, ks[b : b + 1])
            _same_bits(alone, got[b : b + 1], f"row {b} alone {c2}")
    # ids outside the vocabulary are skipped
    tokens[0, 10], tokens[1, 40] = V, -1
    _same_bits(_launch(lg, tokens, m - 1, 1, C.Ctl(r=1.3, n=1)), _reference(lg, tokens, m - 1, 1, C.Ctl(r=1.3, n=1)), "ids outside [0, V)")


def _finish_state(with_lp):
    """three rows, P = 2, eos 9, pad 7: row 0 holds the eos in its prompt and generates it at position 4, row 1 at position 2 (its first
    generated one), row 2 never"""
    stream = torch.tensor([[9, 1, 4, 5, 9, 3, 9, 2], [1, 2, 9, 9, 4, 4, 4, 4], [3, 9, 1, 2, 3, 4, 5, 6]])
    lps = -torch.arange(1, 25, dtype=torch.float32).view(3, 8) if with_lp else None
    return stream, lps


@pytest.mark.parametrize("with_lp", (True, False))
def test_finish_follows_the_reference_step_by_step(with_lp):
    stream, lps = _finish_state(with_lp)
    B, T, P, EOS, PADID = 3, 8, 2, 9, 7
    tokens = torch.full((B, T), -5, dtype=torch.int64, device=DEV)
    tok_cur = torch.full((B,), -5, dtype=torch.int64, device=DEV)
    lp = torch.full((B, T), 55.0, device=DEV) if with_lp else None
    fin = torch.zeros(B, dtype=torch.int32, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    r_tok, r_lp, r_fin = [[-5] * T for _ in range(B)], [[55.0] * T for _ in range(B)], [0] * B
    r_cur = [-5] * B
    for t1 in range(1, T):  # the tail wrote position t1 and advanced to it; then the finish kernel
        tokens[:, t1] = stream[:, t1].to(DEV)
        tok_cur.copy_(stream[:, t1])
        if with_lp:
            lp[:, t1] = lps[:, t1].to(DEV)
        pos.fill_(t1)
        plan.call(lib().pm_dec_finish, plan.finish_args(tokens, tok_cur, lp, fin, pos, P, EOS, PADID))
        torch.cuda.synchronize()
        for b in range(B):
            r_tok[b][t1], r_lp[b][t1], r_cur[b] = int(stream[b, t1]), float(lps[b, t1]) if with_lp else 55.0, int(stream[b, t1])
            was = r_fin[b]
            r_fin[b] = C.finish_step(r_tok[b], r_lp[b] if with_lp else None, r_fin[b], t1, P, EOS, PADID)
            if was and t1 >= P:
                r_cur[b] = PADID
        assert tokens.cpu().tolist() == r_tok and fin.cpu().tolist() == r_fin and tok_cur.cpu().tolist() == r_cur, f"position {t1}"
        if with_lp:
            assert lp.cpu().tolist() == r_lp, f"position {t1}"
        assert int(pos) == t1
    assert r_fin == [4, 2, 0] and r_tok[0][4:] == [9, 7, 7, 7] and r_tok[1][2:] == [9, 7, 7, 7, 7, 7] and r_tok[2] == [-5] + stream[2, 1:].tolist()


def test_eager_launches_equal_a_captured_graph_replay():
    B, V, m = 3, 1000, 300
    g = torch.Generator().manual_seed(9)
    lg0 = _logits(B, V, g).to(DEV)
    tokens0, c = _case(B, V, m, "random", 3, 1.3, 1, g)
    tokens0[:, m] = torch.tensor([c.eos, 4, c.eos])  # the position the finish launch looks at
    fin0 = torch.tensor([0, 0, 5], dtype=torch.int32)
    st = dict(lg=lg0.clone(), tokens=tokens0.to(DEV), cur=torch.zeros(B, dtype=torch.int64, device=DEV), lp=torch.full((B, m + 2), -1.0, device=DEV),
              fin=fin0.to(DEV), pos=torch.tensor([m - 1], dtype=torch.int32, device=DEV), pos1=torch.tensor([m], dtype=torch.int32, device=DEV))

    def restore():
        st["lg"].copy_(lg0)
        st["tokens"].copy_(tokens0)
        st["cur"].zero_()
        st["lp"].fill_(-1.0)
        st["fin"].copy_(fin0)

    def both():
        plan.call(lib().pm_dec_controls, plan.controls_args(st["lg"], st["tokens"], st["pos"], 1, None, repetition_penalty=c.r, no_repeat_ngram=c.n,
                                                            min_new_tokens=c.min_new, eos=c.eos))
        plan.call(lib().pm_dec_finish, plan.finish_args(st["tokens"], st["cur"], st["lp"], st["fin"], st["pos1"], 1, c.eos, C.PAD))

    def bits():
        torch.cuda.synchronize()
        return [st[k].clone().view(torch.uint8) for k in ("lg", "tokens", "cur", "lp", "fin")]

    both()
    eager = bits()
    _same_bits(st["lg"].cpu(), _reference(lg0.cpu(), tokens0, m - 1, 1, c), "eager")
    assert st["fin"].tolist() == [m, 0, 5] and st["tokens"][:, m].tolist() == [c.eos, 4, C.PAD] and st["lp"][:, m].tolist() == [-1.0, -1.0, 0.0]
    restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        restore()
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(eager, bits())), "graph replay and eager launches differ"


def test_refusals_come_before_any_launch():
    L = lib()
    EINVAL = 1
    lg = torch.ones(2, 16, device=DEV)
    tokens = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    pos = torch.tensor([3], dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    good = list(plan.controls_args(lg, tokens, pos, 2, None, repetition_penalty=1.3, no_repeat_ngram=2, min_new_tokens=1, eos=5))
    good[-1] = stream

    def rc(fn, base, **at):
        a = list(base)
        for i, v in at.items():
            a[int(i[1:])] = v
        return fn(*a)

    # 0 logits 1 ldl 2 V 3 tokens 4 Ttot 5 pos 6 P 7 key_start 8 r 9 n 10 min_new 11 eos 12 B
    for i in (0, 3, 5):
        assert rc(L.pm_dec_controls, good, **{f"a{i}": None}) == EINVAL, f"null argument {i}"
    for at in (dict(a8=0.0), dict(a8=-1.0), dict(a8=float("nan")), dict(a8=float("inf")), dict(a9=-1), dict(a9=C.MAX_NGRAM + 1), dict(a2=0),
               dict(a2=-3), dict(a2=(1 << 18) + 1, a1=1 << 20), dict(a1=8), dict(a10=-1), dict(a11=16), dict(a11=-2), dict(a11=-1), dict(a6=0),
               dict(a4=1), dict(a12=0)):
        assert rc(L.pm_dec_controls, good, **at) == EINVAL, at
    fin = torch.zeros(2, dtype=torch.int32, device=DEV)
    cur = torch.zeros(2, dtype=torch.int64, device=DEV)
    fgood = list(plan.finish_args(tokens, cur, None, fin, pos, 2, 5, 7))
    fgood[-1] = stream
    # 0 tokens 1 Ttot 2 tok_cur 3 logprobs 4 finished 5 pos 6 P 7 eos 8 pad 9 B
    for i in (0, 2, 4, 5):
        assert rc(L.pm_dec_finish, fgood, **{f"a{i}": None}) == EINVAL, f"finish: null argument {i}"
    for at in (dict(a7=-1), dict(a8=-1), dict(a6=0), dict(a1=1), dict(a9=0)):
        assert rc(L.pm_dec_finish, fgood, **at) == EINVAL, at
    torch.cuda.synchronize()
    assert bool((lg == 1.0).all()) and bool((tokens == 0).all()) and bool((fin == 0).all()), "a refused call wrote"
    assert rc(L.pm_dec_controls, good) == 0 and rc(L.pm_dec_finish, fgood) == 0  # and the good calls run (no log-prob buffer, no key_start)
    torch.cuda.synchronize()
    assert L.pm_strerror(EINVAL)


@pytest.mark.parametrize("form", ("controls:plain", "controls:ragged", "finish:plain", "finish:logprobs"))
def test_wrappers_honour_or_refuse_every_operand_layout(form):
    """tests/wrapper_cases.py's layout machinery on the new wrappers (which live outside ops.py): every variant of every operand is
    refused cleanly or accepted with the bits of the contiguous call"""
    import wrapper_cases as WC
    from pytorch_models._hip import controls

    r = C.wrapper_rows()[form]
    try:
        problems, accepted = WC.check_row(controls, r, DEV, compare=True)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        if isinstance(e, WC.GpuFault) or WC.is_fault(e):
            pytest.exit(f"{form}: device error, nothing more is started on this GPU: {e}", returncode=3)
        raise
    print(f"{form}: {len(accepted)} variants accepted bit-identically or refused cleanly; {len(problems)} problems")
    assert accepted and not problems, "\n".join([f"{len(problems)} problems:"] + problems)
