"""GPU: the six ragged-prompt kernels on the cases of tests/ragged_cases.py, through the eager wrappers of
_hip/ops.py.
  * pm_dec_attention_ragged: row by row the bits of pm_dec_attention on the caches advanced by lo_b keys; inside the derived bound
    1.5 u (A + |want|) of the float64 reference; a clamped start (>= Lk) gives a finite row;
  * pm_prefill_attention_ragged_bf16: key_start = 0 is pm_prefill_attention_bf16 bit for bit (outputs and caches); bound_ratio <= 1.5
    on the rows at positions >= start_b; padded rows finite and within the bound of their own V row; the caches inside
    [p0, p0 + C) are bit copies of the chunk's k / v, everything outside is untouched (NaN before, compared as integers);
  * pm_embed_tokens_ragged, pm_dec_embed_ragged and the two tails: emb[tok].float() + pos[max(0, t - start)] bit for bit (one fp32
    add); the tails' token choice, prompt forcing, ticket and position advance equal the plain kernels' on the same inputs.
Each parity test prints the figure it asserts ("RATIO ..." lines, pytest -s)."""
import pytest
import torch

import attn_cases as AC
import ragged_cases as RC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_REF, _SREF = {}, {}


def _reference(case):
    """inputs and float64 reference of a case, computed once and shared (never modified)"""
    if case.id not in _REF:
        inp = RC.build(case)
        _REF[case.id] = (inp, *RC.reference(case, inp))
    return _REF[case.id]


def _step_reference(case):
    if case.id not in _SREF:
        inp = RC.build_step(case)
        _SREF[case.id] = (inp, *RC.reference_step(case, inp))
    return _SREF[case.id]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _i32(starts):
    return torch.as_tensor(starts, dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------ pm_dec_attention_ragged
@pytest.mark.parametrize("case", RC.SCASES, ids=lambda c: c.id)
def test_step_attention_is_the_plain_kernel_on_the_advanced_caches(case):
    from pytorch_models._hip import ops

    inp, want, A = _step_reference(case)
    q = inp["q"].cuda()
    k, v = inp["k"].to(torch.bfloat16).cuda(), inp["v"].to(torch.bfloat16).cuda()
    out = ops.dec_attention_ragged(q, k, v, case.Lk, _i32(case.starts))
    torch.cuda.synchronize()
    assert out.shape == q.shape and torch.isfinite(out).all(), f"{case.id}: the clamped start (row 3) must give a finite row too"
    ratio = AC.bound_ratio(out.float().cpu(), want, A)
    print(f"RATIO ragged step {case.id} parity {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"
    for b, lo in enumerate(RC.step_lo(case)):  # the same arithmetic from another base pointer: bit for bit
        plain = ops.dec_attention(q[b : b + 1], k[b : b + 1, :, lo:], v[b : b + 1, :, lo:], case.Lk - lo)
        assert torch.equal(out[b : b + 1].view(torch.int32), plain.view(torch.int32)), f"{case.id}: row {b} (first key {lo})"


# ------------------------------------------------------------------------------------------------ pm_prefill_attention_ragged_bf16
def _launch(case, inp, starts):
    """(out (B, C, H*64), kc, vc after the call, kc, vc before it, the qkv rows) - all on the device; starts None = the plain kernel"""
    from pytorch_models._hip import ops

    B, H, p0, C, T = RC.B, RC.H, case.p0, case.C, case.lk_max
    inner = H * 64
    pad = 8 if p0 % 2 else 0  # odd p0: rows of a wider buffer (leading dimension 3 * H * 64 + 8), NaN in the padding
    buf = torch.full((B * C, 3 * inner + pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    qkv = buf[:, : 3 * inner]
    qkv.copy_(torch.cat([inp["q"], inp["k"], inp["v"]], -1).view(B * C, 3 * inner))
    kc = torch.full((B, H, T, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    vc = torch.full((B, H, T, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    kc[:, :, :p0] = inp["k_old"]
    vc[:, :, :p0] = inp["v_old"]
    kc0, vc0 = kc.clone(), vc.clone()
    if starts is None:
        out = ops.prefill_attention(qkv, kc, vc, H, p0)
    else:
        out = ops.prefill_attention_ragged(qkv, kc, vc, H, p0, _i32(starts))
    torch.cuda.synchronize()
    assert out.shape == (B * C, inner) and out.dtype == torch.bfloat16
    return out.view(B, C, inner), kc, vc, kc0, vc0, qkv


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_prefill_parity_append_and_untouched_caches(case):
    inp, want, A = _reference(case)
    B, H, p0, C = RC.B, RC.H, case.p0, case.C
    out, kc, vc, kc0, vc0, qkv = _launch(case, inp, case.starts)
    got = out.float().cpu()
    assert torch.isfinite(got).all(), f"{case.id}: non-finite output: a NaN cache slot was read into a live product, or a row saw no key"
    valid = RC.valid_rows(p0, C, case.starts)
    ratio = AC.bound_ratio(got[valid], want[valid], A[valid]) if valid.any() else 0.0
    print(f"RATIO ragged prefill {case.id} valid rows {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound on the rows at positions >= start"
    if (~valid).any():  # a padded query sees itself only: its own V row
        own = inp["v"][~valid].double()
        pratio = AC.bound_ratio(got[~valid], own, own.abs())
        print(f"RATIO ragged prefill {case.id} padded rows {pratio:.3f}")
        assert pratio <= 1.5, f"{case.id}: a padded row left its own V row ({pratio:.3f} x bf16_bound)"
    # appended rows: bit copies of the chunk's k / v, the padded ones too
    inner = H * 64
    k_rows = qkv[:, inner : 2 * inner].reshape(B, C, H, 64).transpose(1, 2)
    v_rows = qkv[:, 2 * inner :].reshape(B, C, H, 64).transpose(1, 2)
    assert torch.equal(_bits(kc[:, :, p0 : p0 + C]), _bits(k_rows)) and torch.equal(_bits(vc[:, :, p0 : p0 + C]), _bits(v_rows))
    # everything else: bitwise as before (NaN payloads included)
    for now, before in ((kc, kc0), (vc, vc0)):
        assert torch.equal(_bits(now[:, :, :p0]), _bits(before[:, :, :p0])), f"{case.id}: an old cache row changed"
        assert torch.equal(_bits(now[:, :, p0 + C :]), _bits(before[:, :, p0 + C :])), f"{case.id}: a row behind the chunk was written"


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_prefill_with_zero_starts_is_the_plain_kernel_bit_for_bit(case):
    inp, _, _ = _reference(case)
    plain = _launch(case, inp, None)
    zero = _launch(case, inp, (0,) * RC.B)
    for a, b, what in zip(plain[:3], zero[:3], ("out", "kc", "vc")):
        assert torch.equal(_bits(a), _bits(b)), f"{case.id}: {what} differs from pm_prefill_attention_bf16"


def test_prefill_refuses_a_null_key_start():
    """PM_EINVAL, as every refusal of the plain entry point (tests/test_ragged_cases_cpu.py walks the list without a device)"""
    from pytorch_models import _hip
    from pytorch_models._hip import decode_plan as plan

    H, C, T = 3, 4, 8
    qkv = torch.zeros(2 * C, 3 * H * 64, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(2, H, T, 64, dtype=torch.bfloat16, device="cuda")
    vc, out = torch.zeros_like(kc), torch.zeros(2 * C, H * 64, dtype=torch.bfloat16, device="cuda")
    args = plan.prefill_attention_args(qkv, plan.cache_kv(kc, vc), out, 2, H, C, 2, T)[:-1]
    assert _hip.lib().pm_prefill_attention_ragged_bf16(*args, None, None) == 1
    assert _hip.lib().pm_prefill_attention_ragged_bf16(*args[:-1], 5, _i32((0, 0)).data_ptr(), None) == 1  # p0 + C = 6 > lk_max


# ------------------------------------------------------------------------------------------------ the embedding rows
V, D = 300, 128


def _tables():
    from synthweights import synth_input

    E = synth_input("rg_emb", (V, D), 7).to(torch.bfloat16).cuda()
    pos = synth_input("rg_pos", (40, D), 8).cuda()
    return E, pos


def test_embed_tokens_ragged_is_one_fp32_add():
    from pytorch_models._hip import ops
    from synthweights import synth_tokens

    E, pos = _tables()
    tok = synth_tokens("rg_tok", (3, 7), V, 9).cuda()
    for pos0, starts in ((0, (0, 3, 30)), (5, (0, 8, 30)), (5, (5, 11, 12))):
        st = torch.tensor(starts)
        row = (pos0 + torch.arange(7)[None, :] - st[:, None]).clamp(min=0).cuda()
        want = E[tok].float() + pos[row]
        got = ops.embed_tokens_ragged(tok, E, pos, _i32(starts), pos0=pos0, out_dtype=torch.float32)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (pos0, starts)
        got16 = ops.embed_tokens_ragged(tok, E, pos, _i32(starts), pos0=pos0)
        assert torch.equal(_bits(got16), _bits(want.to(torch.bfloat16))), (pos0, starts)
    zero = ops.embed_tokens_ragged(tok, E, pos, _i32((0, 0, 0)), pos0=5, out_dtype=torch.float32)
    assert torch.equal(zero, ops.embed_tokens(tok, E, pos, pos0=5, out_dtype=torch.float32))


def test_dec_embed_ragged_is_one_fp32_add():
    from pytorch_models._hip import ops

    E, pos = _tables()
    tok = torch.tensor([5, 299, 0, 17, 42], device="cuda")
    starts = (0, 4, 9, 12, 30)
    for t in (0, 9, 20):
        p = torch.tensor([t], dtype=torch.int32, device="cuda")
        row = (t - torch.tensor(starts)).clamp(min=0).cuda()
        got = ops.dec_embed_ragged(tok, E, pos, p, _i32(starts))
        assert torch.equal(got.view(torch.int32), (E[tok].float() + pos[row]).view(torch.int32)), t


# ------------------------------------------------------------------------------------------------ the two token tails
def _tail_state(t, P=6, Ttot=10, B=3):
    from synthweights import synth_tokens

    dev = "cuda"
    return dict(pos=torch.tensor([t], dtype=torch.int32, device=dev), prompt=synth_tokens("rg_tail_prompt", (B, P), V, 3).to(dev),
                tok_cur=torch.zeros(B, dtype=torch.int64, device=dev), tokens=torch.full((B, Ttot), -7, dtype=torch.int64, device=dev),
                ticket=torch.zeros(1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("t", [2, 5, 8])  # the next token is forced (t + 1 < P), the first free one (t + 1 == P), a later one
def test_next_token_ragged_chooses_like_the_plain_tail_and_shifts_the_positional_row(t):
    from pytorch_models._hip import ops
    from synthweights import synth_input

    E, pos_tab = _tables()
    B, n_tiles, starts = 3, 5, (0, 4, 30)
    ws_val = synth_input("rg_ws", (B, n_tiles), 11 + t).cuda()
    ws_val[1, 3] = ws_val[1, 1] = ws_val[1].max() + 1.0  # a tie between tiles 1 (id 40) and 3 (id 12): the lower id wins
    ws_idx = torch.tensor([[7, 250, 31, 9, 120], [88, 40, 3, 12, 299], [1, 2, 3, 4, 5]], dtype=torch.int32, device="cuda")
    plain, ragged = _tail_state(t), _tail_state(t)
    mp, mr = (torch.zeros(B, 10, device="cuda") for _ in range(2))
    xp = ops.dec_next_token(ws_val, ws_idx, plain["pos"], plain["prompt"], plain["tok_cur"], plain["tokens"], E, pos_tab, plain["ticket"],
                            margins=mp)
    xr = ops.dec_next_token(ws_val, ws_idx, ragged["pos"], ragged["prompt"], ragged["tok_cur"], ragged["tokens"], E, pos_tab,
                            ragged["ticket"], margins=mr, key_start=_i32(starts))
    torch.cuda.synchronize()
    for name in plain:
        assert torch.equal(plain[name], ragged[name]), name
    assert torch.equal(mp, mr) and int(ragged["pos"]) == t + 1 and int(ragged["ticket"]) == 0
    nxt = ragged["tok_cur"]
    if t + 1 < 6:
        assert torch.equal(nxt, ragged["prompt"][:, t + 1])
    else:
        assert nxt.tolist() == [int(ws_idx[0, ws_val[0].argmax()]), 12, int(ws_idx[2, ws_val[2].argmax()])]
    assert torch.equal(ragged["tokens"][:, t + 1], nxt) and int((ragged["tokens"] != -7).sum()) == B
    row = (t + 1 - torch.tensor(starts)).clamp(min=0).cuda()
    assert torch.equal(xr.view(torch.int32), (E[nxt].float() + pos_tab[row]).view(torch.int32))
    assert torch.equal(xp.view(torch.int32), (E[nxt].float() + pos_tab[t + 1]).view(torch.int32))


@pytest.mark.parametrize("t", [2, 5, 8])
def test_sample_topk_ragged_draws_like_the_plain_tail_and_shifts_the_positional_row(t):
    from pytorch_models._hip import ops
    from synthweights import synth_input

    E, pos_tab = _tables()
    B, starts = 3, (0, 4, 30)
    logits = synth_input("rg_logits", (B, V), 21, scale=3.0).cuda()
    for k, seed in ((1, 0), (8, 3), (64, 2**63 + 5)):
        plain, ragged = _tail_state(t), _tail_state(t)
        xp = ops.dec_sample_topk(logits, k, seed, plain["pos"], plain["prompt"], plain["tok_cur"], plain["tokens"], E, pos_tab, plain["ticket"])
        xr = ops.dec_sample_topk(logits, k, seed, ragged["pos"], ragged["prompt"], ragged["tok_cur"], ragged["tokens"], E, pos_tab,
                                 ragged["ticket"], key_start=_i32(starts))
        torch.cuda.synchronize()
        for name in plain:
            assert torch.equal(plain[name], ragged[name]), (k, name)
        nxt = ragged["tok_cur"]
        assert int(ragged["pos"]) == t + 1 and int(ragged["ticket"]) == 0
        if t + 1 < 6:
            assert torch.equal(nxt, ragged["prompt"][:, t + 1])
        else:
            kth = logits.topk(k).values[:, -1]
            assert bool((logits.gather(1, nxt[:, None])[:, 0] >= kth).all())
            if k == 1:
                assert torch.equal(nxt, logits.argmax(-1))
        row = (t + 1 - torch.tensor(starts)).clamp(min=0).cuda()
        assert torch.equal(xr.view(torch.int32), (E[nxt].float() + pos_tab[row]).view(torch.int32))
        assert torch.equal(xp.view(torch.int32), (E[nxt].float() + pos_tab[t + 1]).view(torch.int32))
