"""GPU: the token-timestamp kernels of csrc/align.hip through ops.align_lse / align_matrix / align_dtw on every case of
tests/align_cases.py.
  * lse and m within MARGIN = 1.5 x the derived bounds of the float64 reference (no measured number enters them); entries whose
    bound is 0 - columns whose reference std is exactly 0, everything at or beyond len_b and F_b - exactly 0;
  * EVERY run reads q and k as slices of larger buffers whose every other element is 3e38 (k with the row stride 2 * inner of the
    packed k|v projection), rows at or beyond len_b / F_b included, and writes into sentinel-guarded lse / m / start / workspace
    buffers; m starts as NaN: the guards must be unchanged and the results finite;
  * `first` overwrites, a later launch adds; a permutation and a subset of the batch give the same bits per clip;
  * start equals the float32 run of the published DTW loop exactly, nothing excluded.
Each test prints the figure it asserts ("RATIO ..." lines, pytest -s)."""
import math

import pytest
import torch

import align_cases as ac

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_REF = {}
GUARD = 64


def _reference(case):
    """inputs and float64 reference of a case, computed once and shared (never modified)"""
    if case.id not in _REF:
        groups = ac.build(case)
        _REF[case.id] = (groups, ac.reference(groups, case.lens, case.frs))
    return _REF[case.id]


def _guarded(n, dtype, fill=None):
    """(int32 / uint8 buffer filled with the sentinel, its middle n elements as ``dtype``, optionally pre-filled)"""
    raw = torch.uint8 if dtype == torch.uint8 else torch.int32
    buf = torch.full((n + 2 * GUARD,), 0x4B if raw == torch.uint8 else ac.SENTINEL, dtype=raw, device="cuda")
    mid = buf.view(dtype)[GUARD:GUARD + n]
    if fill is not None:
        mid.fill_(fill)
    return buf, mid


def _guards_intact(buf, n) -> bool:
    want = 0x4B if buf.dtype == torch.uint8 else ac.SENTINEL
    return bool((buf[:GUARD] == want).all()) and bool((buf[GUARD + n:] == want).all())


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def _poisoned(q, k, lens, frs):
    """q, k as the middle of 3e38-filled buffers: q with a row stride of inner + 8, k with 2 * inner (the k half of a packed k|v
    projection); token rows at or beyond len_b and frames at or beyond F_b are 3e38 too."""
    B, L, inner = q.shape
    S = k.shape[1]
    qb = torch.full((B, L + 2, inner + 8), ac.POISON, dtype=torch.bfloat16, device="cuda")
    kb = torch.full((B, S + 2, 2 * inner), ac.POISON, dtype=torch.bfloat16, device="cuda")
    qs, ks = qb[:, 1:1 + L, 8:], kb[:, 1:1 + S, :inner]
    qs.copy_(q)
    ks.copy_(k)
    for b in range(B):
        qs[b, lens[b]:] = ac.POISON
        ks[b, frs[b]:] = ac.POISON
    assert qs.stride(1) == inner + 8 and ks.stride(1) == 2 * inner and qs.data_ptr() % 16 == 0 and ks.data_ptr() % 16 == 0
    return qs, ks


def _run(groups, lens, frs, return_dev=False):
    """every group's lse, then the matrix launches in order (first, then adding) -> ([lse (B, n, L) cpu], m (B, L, S) cpu)"""
    from pytorch_models._hip import ops

    B, L = groups[0][0].shape[:2]
    S = groups[0][1].shape[1]
    A = sum(len(g[2]) for g in groups)
    lens_d, frs_d = _i32(lens), _i32(frs)
    b_m, m = _guarded(B * L * S, torch.float32, math.nan)
    m = m.view(B, L, S)
    lses = []
    for i, (q, k, heads) in enumerate(groups):
        qs, ks = _poisoned(q, k, lens, frs)
        heads_d = _i32(heads)
        n = len(heads)
        b_l, lse = _guarded(B * n * L, torch.float32)
        lse = lse.view(B, n, L)
        assert ops.align_lse(qs, ks, heads_d, lens_d, frs_d, out=lse).data_ptr() == lse.data_ptr()
        ops.align_matrix(qs, ks, heads_d, lens_d, frs_d, lse, m, 1.0 / A, i == 0)
        torch.cuda.synchronize()
        assert _guards_intact(b_l, B * n * L), "a write outside lse"
        out = lse.cpu().clone()
        for b in range(B):  # rows at or beyond len_b are not written
            assert bool((out[b, :, lens[b]:].view(torch.int32) == ac.SENTINEL).all())
            out[b, :, lens[b]:] = math.nan
        lses.append(out)
    assert _guards_intact(b_m, B * L * S), "a write outside m"
    return lses, m.cpu().clone()


def _assert_zeros(case, ref, m):
    for b in range(case.B):
        assert bool((m[b, case.lens[b]:] == 0).all()) and bool((m[b, :, case.frs[b]:] == 0).all()), "entries beyond len_b / F_b"
        assert bool((m[b][:, ref.zero_std[b]] == 0).all()), "a column whose reference std is exactly 0"


@pytest.mark.parametrize("case", ac.cases(), ids=lambda c: c.id)
def test_lse_and_matrix_parity_with_the_fp64_reference(case):
    groups, ref = _reference(case)
    lses, m = _run(groups, case.lens, case.frs)
    r_lse = max(ac.ratio(g, w, b) for g, w, b in zip(lses, ref.lse, ref.lse_bound))
    r_m = ac.ratio(m, ref.m, ref.m_bound)
    print(f"RATIO {case.id}: lse {r_lse:.3f}, m {r_m:.3f} of the bound (asserted <= {ac.MARGIN}); cond {ref.cond:.2e}")
    assert bool(torch.isfinite(m).all()), "NaN left in m, or poison read into a live value"
    assert r_lse <= ac.MARGIN and r_m <= ac.MARGIN
    _assert_zeros(case, ref, m)
    if case.family in ("flat", "smallest"):
        assert bool((m == 0).all())


def test_first_overwrites_and_later_launches_add():
    from pytorch_models._hip import ops

    case = next(c for c in ac.cases() if c.family == "ragged")
    (q, k, heads), = _reference(case)[0]
    _, base = _run([(q, k, heads)], case.lens, case.frs)
    qs, ks = _poisoned(q, k, case.lens, case.frs)
    lens_d, frs_d, heads_d = _i32(case.lens), _i32(case.frs), _i32(heads)
    lse = ops.align_lse(qs, ks, heads_d, lens_d, frs_d)
    m = torch.full((case.B, case.L, case.S), math.nan, device="cuda")
    ops.align_matrix(qs, ks, heads_d, lens_d, frs_d, lse, m, 1.0 / len(heads), True)
    assert torch.equal(m.cpu().view(torch.int32), base.view(torch.int32))
    ops.align_matrix(qs, ks, heads_d, lens_d, frs_d, lse, m, 1.0 / len(heads), False)
    assert torch.equal(m.cpu(), 2 * base)  # x + x is exact
    ops.align_matrix(qs, ks, heads_d, lens_d, frs_d, lse, m, 1.0 / len(heads), True)
    assert torch.equal(m.cpu().view(torch.int32), base.view(torch.int32))


def test_clips_do_not_depend_on_their_place_in_the_batch():
    case = next(c for c in ac.cases() if c.family == "ragged")
    groups, _ = _reference(case)
    lses, m = _run(groups, case.lens, case.frs)
    perm = [2, 0, 3, 1]
    for idx in (perm, [3], [1, 2]):
        sub = [(q[idx], k[idx], heads) for q, k, heads in groups]
        l2, m2 = _run(sub, [case.lens[i] for i in idx], [case.frs[i] for i in idx])
        assert torch.equal(m2.view(torch.int32), m[idx].view(torch.int32)), "m: a clip's bits depend on its position or on B"
        assert torch.equal(l2[0].view(torch.int32), lses[0][idx].view(torch.int32)), "lse: a clip's bits depend on its position or on B"


def _dtw(m, lens, frs, s0, s1):
    from pytorch_models._hip import ops

    B, L, S = m.shape
    nws = ops.align_ws_bytes(B, L, S)
    assert 0 < nws <= B * L * ((L + S) // 32 + 1) * 8
    b_s, start = _guarded(B * L, torch.int32)
    b_w, ws = _guarded(nws, torch.uint8)
    mb = torch.full((B, L + 2, S + 5), ac.POISON, device="cuda")  # m as a slice: rows of S + 5 floats
    ms = mb[:, 1:1 + L, :S]
    ms.copy_(m)
    for b in range(B):  # what lies outside a clip's len_b x F_b is never read
        ms[b, lens[b]:] = ac.POISON
        ms[b, :, frs[b]:] = ac.POISON
    out = ops.align_dtw(ms, list(lens), list(frs), s0, s1, out=start.view(B, L), ws=ws)
    torch.cuda.synchronize()
    assert out.data_ptr() == start.data_ptr()
    assert _guards_intact(b_s, B * L), "a write outside start"
    assert _guards_intact(b_w, nws), "a write outside the workspace"
    return start.view(B, L).cpu().clone()


@pytest.mark.parametrize("dc", ac.dtw_cases(), ids=lambda c: c[0])
def test_dtw_equals_the_fp32_loop_exactly(dc):
    name, m, lens, frs, s0, s1 = dc
    want = ac.dtw_start(m, lens, frs, s0, s1)
    got = _dtw(m, lens, frs, s0, s1)
    print(f"DTW {name}: {int((got != want).sum())} of {got.numel()} entries differ (asserted 0); aligned rows {int((want >= 0).sum())}")
    assert torch.equal(got, want)
    if name == "planted":
        assert got[0].tolist() == ac.planted()[2][:-1]
    if name == "ragged":
        assert bool((got[2] == -1).all()) and bool((got[3] == -1).all())  # windows that leave N = -1 and N = 0


def test_dtw_clips_do_not_depend_on_their_place_in_the_batch():
    name, m, lens, frs, s0, s1 = next(c for c in ac.dtw_cases() if c[0] == "ints")
    base = _dtw(m, lens, frs, s0, s1)
    idx = [2, 0, 1]
    assert torch.equal(_dtw(m[idx], [lens[i] for i in idx], [frs[i] for i in idx], s0, s1), base[idx])
    assert torch.equal(_dtw(m[1:2], lens[1:2], frs[1:2], s0, s1), base[1:2])
