"""GPU: T5Model.generate (text/t5_generate.py over csrc/decode_t5.hip) - the KV-cached, batched, graph-replayed greedy step -
against the oracle (oracle/ref_t5.py, fp32, CPU) on the same bf16-rounded weights.

Bounds: step logits rel-L2 <= 2e-2 per row (the project's whole-stack bound against the oracle, test_hip_t5.py); the arg-max
must agree at every decision whose oracle top-2 margin is >= 0.05 (the near-tie rule of test_hip_t5.py / test_hip_exact.py;
tests/test_t5_generate_cpu.py shows that this covers most decisions).  What the path promises about itself - replay against
eager launches, a row in any batch, the content of padded source columns, a second call - is checked bit for bit."""
import pytest
import torch

import t5_generate_cases as TC
from oracle import ref_t5 as R5

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_MODELS = {}


def gpu_model(case):
    if case not in _MODELS:
        m, sd = TC.build(case)
        _MODELS[case] = (m.to(torch.bfloat16).cuda().eval(), sd)
    return _MODELS[case]


def rel(got, want):
    got, want = got.float().cpu(), want.float()
    return ((got - want).norm() / want.norm()).item()


def state(m):
    return m.__dict__["_pm_t5_decode"][1]


def first_near_tie(margins, n):
    low = (margins[:n] < TC.MARGIN).nonzero()
    return int(low[0]) if len(low) else n


@pytest.mark.parametrize("case", TC.TEACHER_FORCED)
def test_teacher_forced_logits_against_the_oracle(case):
    """The main guard: the oracle's ids forced as the decoder prompt over a batch padded to mixed lengths; row b's step logits
    against R5.model(sd, ids_b[:len_b], oracle_ids_b)."""
    m, _ = gpu_model(case)
    tok, lengths, n = TC.sources(case)
    o = TC.oracle(case)
    ids, out_len, logits = m.generate(tok.cuda(), lengths=lengths, max_new_tokens=1, eos_id=-1, decoder_prompt=o["ids"].cuda(),
                                      return_logits=True)
    B = len(lengths)
    assert ids.shape == (B, n + 2) and logits.shape == (B, n + 1, 2000) and logits.dtype == torch.float32
    assert state(m).fuse_self == (case != "unfused")  # B * heads > 256 takes the projection + attention pair
    assert torch.equal(ids[:, : n + 1].cpu(), o["ids"]) and torch.equal(out_len.cpu(), torch.full((B,), n + 2))
    logits = logits.cpu()
    errs = [rel(logits[b], o["logits"][b]) for b in range(B)]
    decided = o["margins"] >= TC.MARGIN
    same = logits.argmax(-1) == o["logits"].argmax(-1)
    print(f"{case}: rel-L2 max {max(errs):.3e}, decided {int(decided.sum())} of {decided.numel()}, "
          f"arg-max differs at {int((~same).sum())} (decided: {int((~same & decided).sum())})")
    assert torch.isfinite(logits).all()
    assert max(errs) <= 2e-2, errs
    assert same[decided].all(), (~same & decided).nonzero()
    assert torch.equal(ids[:, n + 1].cpu(), logits[:, n].argmax(-1))  # the one free decision is the arg-max of its own logits


def test_free_run_follows_the_oracle_up_to_the_first_near_tie():
    m, _ = gpu_model("h8_l4")
    tok, lengths, _ = TC.sources("h8_l4")
    o, n = TC.oracle("h8_l4"), 24
    ids, out_len = m.generate(tok.cuda(), lengths=lengths, max_new_tokens=n, eos_id=-1)
    assert ids.shape == (8, n + 1) and ids.dtype == torch.int64 and torch.equal(out_len.cpu(), torch.full((8,), n + 1))
    kept = 0
    for b in range(8):
        first = first_near_tie(o["margins"][b], n)  # decisions 0 .. first - 1 are decided: positions 1 .. first
        kept += first
        assert torch.equal(ids[b, : first + 1].cpu(), o["ids"][b, : first + 1]), (b, first)
    print(f"free run: {kept} of {8 * n} decisions precede the first near-tie")


def test_rows_stop_at_their_own_eos():
    m, _ = gpu_model("h8_l4")
    tok, lengths, n = TC.sources("h8_l4")
    o = TC.oracle("h8_l4")
    # what row 0 emits at its 6th decision; then the token the oracle generates most often over the batch (more rows stop)
    for eos in (int(o["ids"][0, 6]), int(o["ids"][:, 1:].flatten().mode().values)):
        _check_stopping(m, tok, lengths, n, o, eos, row0=eos == int(o["ids"][0, 6]))


def _check_stopping(m, tok, lengths, n, o, eos, row0):
    want_len = TC.oracle_lengths(o["ids"], eos)
    ids, out_len = m.generate(tok.cuda(), lengths=lengths, max_new_tokens=n, pad_id=0, eos_id=eos)
    ids, out_len = ids.cpu(), out_len.cpu()
    print("eos", eos, "oracle lengths", want_len.tolist(), "got", out_len.tolist())
    assert (not row0 or want_len[0] <= 7) and len(set(want_len.tolist())) > 1  # rows stop at different steps
    for b in range(8):
        L = int(out_len[b])
        assert 2 <= L <= n + 1 and (ids[b, L:] == 0).all()  # everything after a row's eos is the pad id
        assert L == n + 1 or ids[b, L - 1] == eos
        assert not (ids[b, 1 : L - 1] == eos).any()
        Lw = int(want_len[b])
        if first_near_tie(o["margins"][b], Lw - 1) == Lw - 1:  # every decision up to the oracle's last one is decided
            assert L == Lw and torch.equal(ids[b, :L], o["ids"][b, :L]), b
    if row0:  # row 0 itself is such a row
        assert first_near_tie(o["margins"][0], int(want_len[0]) - 1) == int(want_len[0]) - 1


def test_the_path_is_invariant_bit_for_bit():
    m, _ = gpu_model("inner_ne_d")
    tok, lengths, _ = TC.sources("inner_ne_d")
    tok, n = tok.cuda(), 12
    kw = dict(max_new_tokens=n, eos_id=-1, return_logits=True)
    ids, _, lg = m.generate(tok, lengths=lengths, graph=True, **kw)
    # replayed == launched
    ids_e, _, lg_e = m.generate(tok, lengths=lengths, graph=False, **kw)
    assert torch.equal(ids, ids_e) and torch.equal(lg, lg_e)
    # a second call on the same state: the tickets and counters went back to zero
    st = state(m)
    assert int(st.ticket) == 0 and all(int(c.abs().sum()) == 0 for c in st._ks_cnts) and int(st.pos) == st.n_steps
    ids_2, _, lg_2 = m.generate(tok, lengths=lengths, graph=True, **kw)
    assert state(m) is st and torch.equal(ids, ids_2) and torch.equal(lg, lg_2)
    # whatever sits in the padded source columns
    other = tok.clone()
    for b, ln in enumerate(lengths):
        other[b, ln:] = (other[b, ln:] + 17 + b) % 1000
    assert not torch.equal(other, tok)
    ids_o, _, lg_o = m.generate(other, lengths=lengths, graph=True, **kw)
    assert torch.equal(ids, ids_o) and torch.equal(lg, lg_o)
    # lengths as a tensor == as a list
    ids_t, _, lg_t = m.generate(tok, lengths=torch.tensor(lengths), graph=True, **kw)
    assert torch.equal(ids, ids_t) and torch.equal(lg, lg_t)
    # a row in a batch of 8 == the row in a batch of 2 with the same S_max
    ids_s, _, lg_s = m.generate(tok[2:4], lengths=lengths[2:4], graph=True, **kw)
    assert torch.equal(ids[2:4], ids_s) and torch.equal(lg[2:4], lg_s)


def test_padding_amount():
    """A row alone and unpadded against the same row padded to S_max, teacher-forced so that every step is comparable: the
    decode step's own key partition depends on the row's length alone, but the encoder's attention and GEMM tiles see another
    problem size, so two schedules of one fp32 sum: rtol = atol = 1e-5, and equal choices where decided."""
    m, _ = gpu_model("inner_ne_d")
    tok, lengths, n = TC.sources("inner_ne_d")
    o = TC.oracle("inner_ne_d")
    for b in (1, 2):
        ln = lengths[b]
        prompt = o["ids"][b : b + 1].cuda()
        kw = dict(max_new_tokens=1, eos_id=-1, decoder_prompt=prompt, return_logits=True)
        _, _, lg_alone = m.generate(tok[b : b + 1, :ln].cuda(), **kw)
        _, _, lg_pad = m.generate(tok[b : b + 1].cuda(), lengths=[ln], **kw)
        print(f"row {b} (length {ln} of {tok.shape[1]}): max |diff| {(lg_alone - lg_pad).abs().max().item():.3e}, "
              f"max |logit| {lg_alone.abs().max().item():.3e}")
        decided = (o["margins"][b] >= TC.MARGIN).cuda()
        assert torch.equal(lg_alone[0].argmax(-1)[decided], lg_pad[0].argmax(-1)[decided])
        torch.testing.assert_close(lg_alone, lg_pad, rtol=1e-5, atol=1e-5)


def test_refusals_and_generate_ids_unchanged():
    from pytorch_models.text import T5Model
    from synthweights import fill_module

    m, sd = gpu_model("inner_ne_d")
    tok, _, _ = TC.sources("inner_ne_d")
    m32 = T5Model(2000, 512, 6, 2, 1024)
    fill_module(m32, 94)
    with pytest.raises(NotImplementedError, match="bf16 parameters only"):
        m32.cuda().eval().generate(tok.cuda())
    with pytest.raises(RuntimeError, match="HIP devices only"):
        m.generate(tok)
    with pytest.raises(NotImplementedError, match="at most 64 sequences"):
        m.generate(tok[:1].expand(65, -1).contiguous().cuda())
    for bad in ([65] + [1] * 7, [-1] + [1] * 7, [1] * 7):
        with pytest.raises(ValueError, match="lengths"):
            m.generate(tok.cuda(), lengths=bad)
    with pytest.raises(NotImplementedError, match="2048"):
        m.generate(tok.cuda(), max_new_tokens=2048)
    # generate_ids (the reference's loop, one sequence) still returns what it returned; generate on that row agrees with it
    # under the near-tie rule
    want, margins = R5.greedy(sd, tok[0], 12)
    old = m.generate_ids(tok[0].cuda(), 12).cpu()
    new, new_len = m.generate(tok[:1].cuda(), max_new_tokens=11)
    first = first_near_tie(torch.tensor(margins), len(margins))
    assert torch.equal(old[: first + 1], want[: first + 1]) and torch.equal(new[0, : first + 1].cpu(), want[: first + 1])
    if first == len(margins):
        assert len(old) == len(want) == int(new_len[0])
