"""Kernel-level float64 parity of csrc/decode_t5.hip, every entry point called through the C ABI (pytorch_models._hip.lib / check).
Cases, references and the tolerance live in tests/t5_decode_cases.py; tests/test_t5_decode_cases_cpu.py proves on the CPU that a
correct kernel meets every assertion made here and that a subtly wrong one (index off by one in the distance table, a lost key,
the second column group ignored, gate and value exchanged, erf for tanh, eps or the mean's count wrong, another score scale) misses it
tenfold.  rtol = atol = 1e-5 against float64 for q, the GEGLU output and every attention output; the cached row a step appends
within one bf16 rounding of the float64 projection; everything a kernel must not touch compared bit for bit, with a sentinel row
in front of and behind every cache so that a write outside it is seen inside the allocation.  Every tolerance assertion prints
the used fraction of its allowance first ("USED <kernel> <case> <what> <fraction>", pytest -s); the largest per kernel are in
DESIGN.md, section 15."""
import pytest
import torch

import t5_decode_cases as TD

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PM_EINVAL, PM_EUNSUPPORTED, PM_EALIGN = 1, 2, 4
SENTINEL = 123.0  # exact in bf16 and fp32
BF, I32, I64 = torch.bfloat16, torch.int32, torch.int64


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pytorch_models._hip import lib

    return lib()


def _check(rc, what):
    from pytorch_models._hip import check

    check(rc, what)
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _assert_close(kernel, case_id, what, got, want):
    f = TD.used(got.cpu(), want)
    print(f"USED {kernel} {case_id} {what} {f:.3f}")
    assert f <= 1.0, f"{kernel} {case_id} {what}: {f:.3f} of rtol = atol = {TD.TOL}"


def _assert_row(kernel, case_id, what, got, want):
    f = TD.row_ok(got.cpu(), want)
    print(f"USED {kernel} {case_id} {what} {f:.3f} (of one bf16 rounding)")
    assert f <= 1.0, f"{kernel} {case_id} {what}: {f:.3f} of 2^-8 |want| + 1e-6"


def _pos(t):
    return torch.tensor([t], dtype=I32, device="cuda")


class Cache:
    """A (B, H, Tmax, 64) bf16 cache with one sentinel row in front and one behind, inside ONE allocation; the kernels get the interior
    pointer (rows are 128 bytes, so it is 16-byte aligned).  Rows >= t hold NaN: nothing may read them before they are written."""

    def __init__(self, rows: torch.Tensor, t: int):
        B, H, Tmax, _ = rows.shape
        self.buf = torch.full((B * H * Tmax + 2, 64), SENTINEL, dtype=BF, device="cuda")
        self.view = self.buf[1:-1].view(B, H, Tmax, 64)
        self.view.copy_(rows.to(BF))
        self.view[:, :, max(t, 0):] = float("nan")
        self.before = self.buf.clone()
        assert self.ptr() % 16 == 0

    def ptr(self, b: int = 0):
        return self.view[b].data_ptr()

    def slack_intact(self):
        return bool((self.buf[0] == SENTINEL).all() and (self.buf[-1] == SENTINEL).all())

    def untouched_except(self, t=None):
        """bit equality with the state before the launch, row t of every (b, h) excepted"""
        now, was = self.buf[1:-1].view(self.view.shape), self.before[1:-1].view(self.view.shape)
        if t is None:
            return _same_bits(now, was) and self.slack_intact()
        return _same_bits(now[:, :, :t], was[:, :, :t]) and _same_bits(now[:, :, t + 1:], was[:, :, t + 1:]) and self.slack_intact()


def _self_dev(c, inp, t=None):
    t = c.t if t is None else t
    return dict(x=inp["x"].cuda(), g=inp["g"].cuda(), w=inp["w"].to(BF).cuda(), lut=inp["lut"].cuda().contiguous(), pos=_pos(t),
                kc=Cache(inp["kc"], t), vc=Cache(inp["vc"], t),
                q=torch.full((c.B, c.inner), SENTINEL, device="cuda"), att=torch.full((c.B, c.inner), SENTINEL, device="cuda"))


def _self_fused(L, c, dv, b=None):
    """the whole batch, or row b alone through pointers into the same buffers"""
    o, B = (0, c.B) if b is None else (b, 1)
    return L.pm_t5_dec_self_fused(dv["x"][o:].data_ptr(), c.d, dv["g"].data_ptr(), TD.EPS, dv["w"].data_ptr(), dv["kc"].ptr(o), dv["vc"].ptr(o),
                                  c.Tmax, dv["pos"].data_ptr(), dv["lut"].data_ptr(), dv["att"][o:].data_ptr(), B, c.H, None)


def _rms_qkv(L, c, dv, b=None):
    o, B = (0, c.B) if b is None else (b, 1)
    return L.pm_t5_dec_rms_qkv(dv["x"][o:].data_ptr(), c.d, dv["g"].data_ptr(), TD.EPS, dv["w"].data_ptr(), dv["q"][o:].data_ptr(),
                               dv["kc"].ptr(o), dv["vc"].ptr(o), c.Tmax, dv["pos"].data_ptr(), B, c.H, None)


def _self_attention(L, c, dv, b=None):
    o, B = (0, c.B) if b is None else (b, 1)
    return L.pm_t5_dec_self_attention(dv["q"][o:].data_ptr(), dv["kc"].ptr(o), dv["vc"].ptr(o), c.Tmax, dv["pos"].data_ptr(),
                                      dv["lut"].data_ptr(), dv["att"][o:].data_ptr(), B, c.H, None)


def _check_appended_rows(kernel, c, dv, ref_of):
    """Row t of both caches: one bf16 rounding from the float64 projection; every other row and the slack rows keep their bits.
    Returns the float64 reference that reads THESE rows as its key / value t."""
    own = (dv["kc"].view[:, :, c.t].float().cpu(), dv["vc"].view[:, :, c.t].float().cpu())
    ref = ref_of(own)
    _assert_row(kernel, c.id, "k_row", own[0], ref["k_new"])
    _assert_row(kernel, c.id, "v_row", own[1], ref["v_new"])
    assert dv["kc"].untouched_except(c.t) and dv["vc"].untouched_except(c.t), "a cache row other than t changed"
    return ref


@pytest.mark.parametrize("c", TD.SELF_CASES, ids=lambda c: c.id)
def test_self_fused(L, c):
    inp = TD.build_self(c)
    dv = _self_dev(c, inp)
    _check(_self_fused(L, c, dv), "pm_t5_dec_self_fused")
    ref = _check_appended_rows("self_fused", c, dv, lambda own: TD.ref_self(c, inp, own=own))
    assert torch.isfinite(dv["att"]).all(), "rows beyond t are NaN and must not be read"
    _assert_close("self_fused", c.id, "att", dv["att"], ref["att"])
    att = dv["att"].clone()
    dv2 = _self_dev(c, inp)
    _check(_self_fused(L, c, dv2), "pm_t5_dec_self_fused")
    assert _same_bits(dv2["att"], att) and _same_bits(dv2["kc"].buf, dv["kc"].buf), "a second launch gives the same bits"


@pytest.mark.parametrize("c", TD.SELF_CASES, ids=lambda c: c.id)
def test_rms_qkv_then_self_attention(L, c):
    inp = TD.build_self(c)
    dv = _self_dev(c, inp)
    _check(_rms_qkv(L, c, dv), "pm_t5_dec_rms_qkv")
    ref = _check_appended_rows("rms_qkv", c, dv, lambda own: TD.ref_self(c, inp, own=own))
    _assert_close("rms_qkv", c.id, "q", dv["q"], ref["q"])
    assert (dv["att"] == SENTINEL).all()
    before = (dv["kc"].buf.clone(), dv["vc"].buf.clone(), dv["q"].clone())
    _check(_self_attention(L, c, dv), "pm_t5_dec_self_attention")
    assert _same_bits(dv["kc"].buf, before[0]) and _same_bits(dv["vc"].buf, before[1]) and _same_bits(dv["q"], before[2]), "inputs are read only"
    assert torch.isfinite(dv["att"]).all(), "rows beyond t are NaN and must not be read"
    _assert_close("self_attention", c.id, "att", dv["att"], ref["att"])
    # The fused kernel computes the same thing, not the same bits: its norm reduces across four waves, this one inside one, so q
    # differs in the last place - and so may k / v BEFORE their rounding, which can then fall on either side of a bf16 boundary
    # (2^-8 apart; checked per path above).  Such a flip is not an attention error, so the attention launch of the pair runs once
    # more on the FUSED kernel's caches with the pair's q: the two forms then differ by q's last place and by where key t is read
    # (LDS there, the cache here) only, and must agree at 1e-5.
    dvf = _self_dev(c, inp)
    _check(_self_fused(L, c, dvf), "pm_t5_dec_self_fused")
    flips = int((_bits(dvf["kc"].buf) != _bits(dv["kc"].buf)).sum() + (_bits(dvf["vc"].buf) != _bits(dv["vc"].buf)).sum())
    print(f"INFO {c.id}: {flips} of {2 * c.B * c.inner} appended elements round differently in the two forms")
    fused_att = dvf["att"].clone()
    dvf["q"].copy_(dv["q"])
    _check(_self_attention(L, c, dvf), "pm_t5_dec_self_attention")
    _assert_close("self_fused_vs_pair", c.id, "att", dvf["att"], fused_att.cpu().double())
    # the attention launch alone: q handed over as the reference's own (rounded to fp32, which moves att by ~1e-7)
    dv["q"].copy_(ref["q"].float())
    dv["att"].fill_(SENTINEL)
    _check(_self_attention(L, c, dv), "pm_t5_dec_self_attention")
    _assert_close("self_attention", c.id, "att_given_q", dv["att"], ref["att"])


# ---------------------------------------------------------------------------------------------------------------------------------


def _cross_dev(c, inp, src_len=None):
    kv = inp["kv"].to(BF).cuda()
    for b in range(c.B):
        kv[b, c.keys(b):] = float("nan")  # rows beyond src_len[b] are never to be read
    return dict(x=inp["x"].cuda(), g=inp["g"].cuda(), w=inp["w"].to(BF).cuda(), kv=kv,
                src_len=torch.tensor(c.src_len if src_len is None else src_len, dtype=I32, device="cuda"),
                att=torch.full((c.B, c.inner), float("nan"), device="cuda"))


def _cross(L, c, dv, b=None):
    o, B = (0, c.B) if b is None else (b, 1)
    return L.pm_t5_dec_cross_fused(dv["x"][o:].data_ptr(), c.d, dv["g"].data_ptr(), TD.EPS, dv["w"].data_ptr(), dv["kv"][o:].data_ptr(), c.S,
                                   dv["src_len"][o:].data_ptr(), dv["att"][o:].data_ptr(), B, c.H, None)


@pytest.mark.parametrize("c", TD.CROSS_CASES, ids=lambda c: c.id)
def test_cross_fused(L, c):
    inp = TD.build_cross(c)
    dv = _cross_dev(c, inp)
    kv_before = dv["kv"].clone()
    _check(_cross(L, c, dv), "pm_t5_dec_cross_fused")
    assert _same_bits(dv["kv"], kv_before)
    assert torch.isfinite(dv["att"]).all(), "rows beyond src_len are NaN and must not be read"
    for b in range(c.B):
        if c.src_len[b] <= 0:
            assert (dv["att"][b] == 0).all(), "src_len <= 0 gives exact zeros"
    _assert_close("cross_fused", c.id, "att", dv["att"], TD.ref_cross(c, inp)["att"])
    if any(ln > c.S for ln in c.src_len):  # src_len > S is src_len = S
        dv2 = _cross_dev(c, inp, [min(ln, c.S) for ln in c.src_len])
        _check(_cross(L, c, dv2), "pm_t5_dec_cross_fused")
        assert _same_bits(dv2["att"], dv["att"])


# ---------------------------------------------------------------------------------------------------------------------------------


def _geglu_dev(c, inp):
    from pytorch_models.text.t5 import GEGLU
    from pytorch_models.text.t5_generate import _interleaved_wv

    m = GEGLU(c.d, c.F)
    m.w.weight.copy_(inp["w"])
    m.v.weight.copy_(inp["v"])
    wv = _interleaved_wv(m.to(BF).cuda())  # the layout as the generation path derives it
    assert torch.equal(wv.float().cpu(), TD.interleave(inp["w"], inp["v"]))
    return dict(x=inp["x"].cuda(), g=inp["g"].cuda(), wv=wv, h=torch.full((c.B, c.ldh), SENTINEL, device="cuda"))


def _geglu(L, c, dv, b=None):
    o, B = (0, c.B) if b is None else (b, 1)
    return L.pm_t5_dec_geglu(dv["x"][o:].data_ptr(), c.d, dv["g"].data_ptr(), TD.EPS, dv["wv"].data_ptr(), dv["h"][o:].data_ptr(), c.ldh, B, c.F, None)


@pytest.mark.parametrize("c", TD.GEGLU_CASES, ids=lambda c: c.id)
def test_geglu(L, c):
    inp = TD.build_geglu(c)
    dv = _geglu_dev(c, inp)
    _check(_geglu(L, c, dv), "pm_t5_dec_geglu")
    assert (dv["h"][:, c.F:] == SENTINEL).all(), "the ldh - F padding columns are not written"
    _assert_close("geglu", c.id, "h", dv["h"][:, :c.F], TD.ref_geglu(c, inp))


# ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pos", [-1, 64, 65, 1 << 20])
def test_a_position_outside_the_caches_writes_nothing(L, pos):
    c = TD.SELF["d512_h6_b8_t63_last"]
    assert c.Tmax == 64
    inp = TD.build_self(c)
    for launch in (_self_fused, _rms_qkv, _self_attention):
        dv = _self_dev(c, inp, t=0)  # every cache row NaN
        dv["pos"].fill_(pos)
        _check(launch(L, c, dv), launch.__name__)
        assert dv["kc"].untouched_except() and dv["vc"].untouched_except(), launch.__name__
        assert (dv["q"] == SENTINEL).all() and (dv["att"] == SENTINEL).all(), launch.__name__


def test_batch_invariance_bit_for_bit(L):
    """Row b of a B = 64 launch == the same row launched alone (through pointers to row b of the same buffers), for every kernel
    with a batch: the file header of decode_t5.hip promises it."""
    rows = (0, 7, 8, 9, 63)
    c = TD.SELF["d520_h2_b64_t40"]
    inp = TD.build_self(c)
    for name, launches in (("fused", (_self_fused,)), ("pair", (_rms_qkv, _self_attention))):
        full, alone = _self_dev(c, inp), _self_dev(c, inp)
        for launch in launches:
            _check(launch(L, c, full), launch.__name__)
        for b in rows:
            for launch in launches:
                _check(launch(L, c, alone, b), launch.__name__)
        for b in rows:
            assert _same_bits(alone["att"][b], full["att"][b]), (name, b)
            assert _same_bits(alone["kc"].view[b], full["kc"].view[b]) and _same_bits(alone["vc"].view[b], full["vc"].view[b]), (name, b)
            if name == "pair":
                assert _same_bits(alone["q"][b], full["q"][b]), b
        untouched = [b for b in range(c.B) if b not in rows]
        assert (alone["att"][untouched] == SENTINEL).all() and alone["kc"].slack_intact() and alone["vc"].slack_intact()
    c = TD.CROSS["s16_d384_h1_b64"]
    inp = TD.build_cross(c)
    full, alone = _cross_dev(c, inp), _cross_dev(c, inp)
    _check(_cross(L, c, full), "pm_t5_dec_cross_fused")
    for b in rows:
        _check(_cross(L, c, alone, b), "pm_t5_dec_cross_fused")
        assert _same_bits(alone["att"][b], full["att"][b]), b
    c = TD.GEGLU["f1032_d1024_b64_pad"]
    inp = TD.build_geglu(c)
    full, alone = _geglu_dev(c, inp), _geglu_dev(c, inp)
    _check(_geglu(L, c, full), "pm_t5_dec_geglu")
    for b in rows:
        _check(_geglu(L, c, alone, b), "pm_t5_dec_geglu")
        assert _same_bits(alone["h"][b], full["h"][b]), b


# ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", TD.NEXT_CASES, ids=lambda c: c.id)
def test_next_token(L, c):
    inp = TD.build_next(c)
    want = TD.ref_next(c, inp)
    B, V, d, P, Ttot = c.B, c.V, c.d, TD.NEXT_P, TD.NEXT_TTOT
    E = inp["E"].to(BF).cuda()
    prompt = inp["prompt"].cuda()
    for with_logits in (False, True):
        for run in range(2):  # a second run over the same buffers: the ticket came back to zero by itself
            if run == 0:
                ticket = torch.zeros(1, dtype=I32, device="cuda")
            pos = _pos(0)
            tok_buf = torch.full((B + 2, Ttot), -7, dtype=I64, device="cuda")  # one slack row in front and behind
            tokens = tok_buf[1:-1]
            tokens.fill_(TD.PAD_ID)
            tokens[:, :P] = prompt
            finished = torch.zeros(B, dtype=I32, device="cuda")
            out_len = torch.full((B,), Ttot, dtype=I64, device="cuda")
            x = torch.full((B, d), float("nan"), device="cuda")
            step = torch.empty(B, V, device="cuda") if with_logits else None
            filed = torch.full((B, Ttot - 1, V), float("nan"), device="cuda") if with_logits else None
            for t in range(Ttot):
                val, idx = (a.cuda() for a in inp["steps"][t])
                if with_logits:
                    step.copy_(torch.arange(B * V, device="cuda").view(B, V) * 0.5 + t)
                _check(L.pm_t5_dec_next_token(val.data_ptr(), idx.data_ptr(), c.nt, pos.data_ptr(), prompt.data_ptr(), P, tokens.data_ptr(),
                                              Ttot, TD.PAD_ID, inp["eos_id"], finished.data_ptr(), out_len.data_ptr(), E.data_ptr(),
                                              x.data_ptr(), d, V, ticket.data_ptr(), step.data_ptr() if with_logits else None,
                                              filed.data_ptr() if with_logits else None, B, None), "pm_t5_dec_next_token")
                assert int(pos) == t + 1 and int(ticket) == 0, (t, int(pos), int(ticket))
                assert torch.equal(x.cpu(), inp["E"][want["nexts"][t]]), f"x[b] == E[next] at step {t}"
                if with_logits and t < Ttot - 1:
                    assert torch.equal(filed[:, t], step) and torch.isnan(filed[:, t + 1:]).all(), t
            assert torch.equal(tokens.cpu(), want["tokens"])
            assert (tok_buf[0] == -7).all() and (tok_buf[-1] == -7).all(), "the step at t + 1 == Ttot writes no token"
            assert torch.equal(finished.cpu(), want["finished"]) and torch.equal(out_len.cpu(), want["out_len"])
            if with_logits:  # filed at steps 0 .. Ttot - 2 only; the last step's row went nowhere
                assert not torch.isnan(filed).any() and torch.equal(filed[:, Ttot - 2], step - 1)
    if c.eos:
        assert want["finished"][B - 1] == 1
    else:
        assert not want["finished"].any()


@pytest.mark.parametrize("d", [8, 520, 1024])
def test_embed(L, d):
    B, V, ld = 9, 50, 3
    E = TD.bf16r(TD.synth_input("t5e_E", (V, d), 61))
    tok = TD.synth_tokens("t5e_tok", (B, ld), V, 62)
    tok[0, 1], tok[1, 1], tok[2, 1], tok[3, 1], tok[4, 1] = -5, V + 3, 0, V - 1, V  # clamped at both ends
    want = E[tok[:, 1].clamp(0, V - 1)]
    xb = torch.full((B + 2, d), SENTINEL, device="cuda")
    Ed, tokd = E.to(BF).cuda(), tok.cuda()
    _check(L.pm_t5_dec_embed(tokd[:, 1:].data_ptr(), ld, Ed.data_ptr(), xb[1:].data_ptr(), B, d, V, None), "pm_t5_dec_embed")
    assert torch.equal(xb[1:-1].cpu(), want), "x[b] = E[token[b * ldtok]], exact"
    assert (xb[0] == SENTINEL).all() and (xb[-1] == SENTINEL).all()
    assert not torch.equal(want, E[tok[:, 2].clamp(0, V - 1)]), "another column of the token matrix would give other rows"


# ---------------------------------------------------------------------------------------------------------------------------------


def test_refusals(L):
    """Each returns its documented code before any launch (the buffers are large enough for every geometry named here anyway)."""
    from pytorch_models._hip import check

    buf = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda")  # every pointer argument; a zero position / length / id
    p, odd = buf.data_ptr(), buf.data_ptr() + 4
    eps = TD.EPS

    def fused(B=2, d=64, Tmax=8, H=1, x=p, kc=p, att=p):
        return L.pm_t5_dec_self_fused(x, d, p, eps, p, kc, p, Tmax, p, p, att, B, H, None)

    def qkv(B=2, d=64, Tmax=8, H=1, x=p):
        return L.pm_t5_dec_rms_qkv(x, d, p, eps, p, p, p, p, Tmax, p, B, H, None)

    def attn(B=2, Tmax=8, H=1, q=p):
        return L.pm_t5_dec_self_attention(q, p, p, Tmax, p, p, p, B, H, None)

    def cross(B=2, d=64, S=8, H=1, kv=p, w=p):
        return L.pm_t5_dec_cross_fused(p, d, p, eps, w, kv, S, p, p, B, H, None)

    def geglu(B=2, d=64, F=8, ldh=8, g=p):
        return L.pm_t5_dec_geglu(p, d, g, eps, p, p, ldh, B, F, None)

    def nxt(step=None, filed=None, d=64, E=p):
        return L.pm_t5_dec_next_token(p, p, 1, p, p, 1, p, 2, 0, 1, p, p, E, p, d, 64, p, step, filed, 2, None)

    def embed(d=64, x=p):
        return L.pm_t5_dec_embed(p, 1, p, x, 2, d, 64, None)

    cases = [
        ("B = 65", PM_EUNSUPPORTED, [fused(B=65), qkv(B=65), cross(B=65), geglu(B=65)]),
        ("d = 1032", PM_EUNSUPPORTED, [fused(d=1032), qkv(d=1032), cross(d=1032), geglu(d=1032)]),
        ("d % 8 != 0", PM_EUNSUPPORTED, [fused(d=60), qkv(d=60), cross(d=60), geglu(d=60), nxt(d=60), embed(d=60)]),
        ("Tmax = 2049", PM_EUNSUPPORTED, [fused(Tmax=2049), attn(Tmax=2049)]),
        ("S = 2049", PM_EUNSUPPORTED, [cross(S=2049)]),
        ("F % 8 != 0", PM_EUNSUPPORTED, [geglu(F=12, ldh=12)]),
        ("ldh < F", PM_EINVAL, [geglu(F=16, ldh=8)]),
        ("misaligned pointer", PM_EALIGN, [fused(x=odd), fused(kc=odd), fused(att=odd), qkv(x=odd), attn(q=odd), cross(kv=odd), cross(w=odd),
                                          geglu(g=odd), nxt(E=odd), embed(x=odd)]),
        ("logits_step without logits_all", PM_EINVAL, [nxt(step=p), nxt(filed=p)]),
        ("null pointer", PM_EINVAL, [fused(x=None), attn(q=None), cross(kv=None), embed(x=None)]),
    ]
    for what, code, rcs in cases:
        assert rcs == [code] * len(rcs), (what, rcs)
        with pytest.raises(RuntimeError, match=f"pm_mi355x error {code}"):
            check(rcs[0], what)
    torch.cuda.synchronize()
    assert not buf.any(), "a refusal launches nothing"
