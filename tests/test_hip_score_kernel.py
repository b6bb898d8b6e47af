"""GPU: pm_lm_score_bf16 (csrc/lm_score.hip) through ops.lm_score on every case of tests/score_cases.py.
  * logprob and lse within MARGIN = 1.5 x the derived bounds of the float64 reference (no measured number enters them), the arg-max
    under the arg-max rule; flat and ties assert their indices exactly;
  * EVERY run writes into sentinel-guarded logprob / lse / argmax / workspace buffers: the guards must be unchanged;
  * poison: operands as the middle slice of larger buffers (ldh > K, ldw > K) whose every other element is 3e38 - finite results,
    bit-identical to the run on plain copies, inside the bound;
  * perm: a fixed permutation of the rows and the first 37 rows alone give the same bits per row.
Each test prints the figure it asserts ("RATIO ..." lines, pytest -s)."""
import pytest
import torch

import score_cases as sc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_REF = {}
GUARD = 16


def _reference(case):
    """inputs and float64 reference of a case, computed once and shared (never modified)"""
    if case.id not in _REF:
        h, w, t = sc.build(case)
        _REF[case.id] = (h, w, t, sc.reference(h, w, t))
    return _REF[case.id]


def _guarded(n, dtype):
    """(buffer filled with the sentinel, its middle n elements)"""
    buf = torch.full((n + 2 * GUARD,), sc.SENTINEL if dtype != torch.uint8 else 0x4B, dtype=torch.int32 if dtype != torch.uint8 else dtype,
                     device="cuda")
    return buf, buf.view(dtype)[GUARD:GUARD + n]


def _guards_intact(buf, n) -> bool:
    want = sc.SENTINEL if buf.dtype != torch.uint8 else 0x4B
    return bool((buf[:GUARD] == want).all()) and bool((buf[GUARD + n:] == want).all())


def _run(h, w, t):
    """ops.lm_score on device operands with sentinel-guarded outputs and workspace -> (logprob, lse, argmax) on the CPU"""
    from pytorch_models._hip import ops

    M, V = h.shape[0], w.shape[0]
    nws = ops.lm_score_ws_bytes(M, V)
    assert 0 < nws <= 32 * M * sc.nchunks(V)
    (b_lp, lp), (b_lse, lse), (b_am, am), (b_ws, ws) = (_guarded(M, torch.float32), _guarded(M, torch.float32),
                                                        _guarded(M, torch.int32), _guarded(nws, torch.uint8))
    res = ops.lm_score(h, w, t, out=lp, lse_out=lse, argmax_out=am, ws=ws)
    torch.cuda.synchronize()
    assert len(res) == 3 and res[0].data_ptr() == lp.data_ptr()
    assert _guards_intact(b_lp, M) and _guards_intact(b_lse, M) and _guards_intact(b_am, M), "a write outside an output"
    assert _guards_intact(b_ws, nws), "a write outside the workspace"
    return lp.cpu().clone(), lse.cpu().clone(), am.cpu().clone()


@pytest.mark.parametrize("case", sc.cases(), ids=lambda c: c.id)
def test_parity_with_the_fp64_reference(case):
    h, w, t, ref = _reference(case)
    lp, lse, am = _run(h.cuda(), w.cuda(), t.cuda())
    v = sc.judge(case, ref, lp, lse, am)
    print(f"RATIO {case.id}: logprob {v.r_lp:.3f} lse {v.r_lse:.3f} of the bound (asserted <= {sc.MARGIN}); argmax rule {v.am_ok}, "
          f"exact indices {v.exact_ok}")
    assert v.passed(sc.MARGIN), v
    if case.family == "flat":
        assert torch.equal(lp, -lse) and bool((am == 0).all())
    if case.family == "edges":
        assert bool((lp[t == -1] == 0).all())


def test_optional_outputs_and_fresh_buffers_agree():
    from pytorch_models._hip import ops

    case = sc.Case("gauss", 129, sc.NC + 1, 64)
    h, w, t, _ = _reference(case)
    lp, lse, am = _run(h.cuda(), w.cuda(), t.cuda())
    only = ops.lm_score(h.cuda(), w.cuda(), t.cuda())
    assert isinstance(only, torch.Tensor) and torch.equal(only.cpu(), lp)
    lp2, lse2 = ops.lm_score(h.cuda(), w.cuda(), t.cuda(), want_lse=True)
    lp3, am3 = ops.lm_score(h.cuda(), w.cuda(), t.cuda(), want_argmax=True)
    assert torch.equal(lp2.cpu(), lp) and torch.equal(lse2.cpu(), lse) and torch.equal(lp3.cpu(), lp) and torch.equal(am3.cpu(), am)
    with pytest.raises(IndexError):
        ops.lm_score(h.cuda(), w.cuda(), torch.full_like(t, case.V).cuda())


@pytest.mark.parametrize("case", [c for c in sc.gpu_only_cases() if c.family == "poison"], ids=lambda c: c.id)
def test_poison_around_every_operand(case):
    h, w, t, ref = _reference(case)
    M, V, K = case.M, case.V, case.K
    plain = _run(h.cuda(), w.cuda(), t.cuda())
    hbuf = torch.full((M + 8, K + 16), sc.POISON, dtype=torch.bfloat16, device="cuda")
    wbuf = torch.full((V + 8, K + 24), sc.POISON, dtype=torch.bfloat16, device="cuda")
    hs, ws = hbuf[4:4 + M, 8:8 + K], wbuf[4:4 + V, 16:16 + K]
    hs.copy_(h)
    ws.copy_(w)
    assert hs.stride(0) > K and ws.stride(0) > K and hs.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    got = _run(hs, ws, t.cuda())
    assert all(torch.isfinite(g.float()).all() for g in got[:2]), "poison was read into a live logit"
    for a, b, name in zip(got, plain, ("logprob", "lse", "argmax")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} differs from the run on plain copies"
    v = sc.judge(case, ref, *got)
    print(f"RATIO {case.id}: logprob {v.r_lp:.3f} lse {v.r_lse:.3f} of the bound (asserted <= {sc.MARGIN})")
    assert v.passed(sc.MARGIN), v


@pytest.mark.parametrize("case", [c for c in sc.gpu_only_cases() if c.family == "perm"], ids=lambda c: c.id)
def test_rows_do_not_depend_on_their_place_in_the_batch(case):
    h, w, t, ref = _reference(case)
    base = _run(h.cuda(), w.cuda(), t.cuda())
    v = sc.judge(case, ref, *base)
    print(f"RATIO {case.id}: logprob {v.r_lp:.3f} lse {v.r_lse:.3f} of the bound (asserted <= {sc.MARGIN})")
    assert v.passed(sc.MARGIN), v
    p = torch.randperm(case.M, generator=torch.Generator().manual_seed(11))
    perm = _run(h[p].cuda(), w.cuda(), t[p].cuda())
    n = min(37, case.M)
    head = _run(h[:n].contiguous().cuda(), w.cuda(), t[:n].cuda())
    for a, b, c, name in zip(base, perm, head, ("logprob", "lse", "argmax")):
        assert torch.equal(a[p].view(torch.int32), b.view(torch.int32)), f"{name}: a row's bits depend on its position"
        assert torch.equal(a[:n].view(torch.int32), c.view(torch.int32)), f"{name}: a row's bits depend on M"
