"""GPU: pm_attention_varlen_relbias_bf16 through ops.attention_varlen(..., rel_lut=, radius=) - the packed attention with a
relative-position bias read by distance - against the float64 reference of tests/relbias_cases.py (bound_ratio <= 1.5, the
contract of tests/attn_cases.py; tests/test_relbias_cases_cpu.py shows on the CPU that a correct kernel satisfies it), its
isolation, extents, position invariance, the bit identity with pm_attention_bias_bf16 on the gathered dense table that sharing
the tile body gives, dead rows, and the operand checks.  Each parity test prints the figure it asserts ("RATIO ..." lines,
pytest -s)."""
import pytest
import torch

import relbias_cases as RC
import varlen_cases as VC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
PATTERN = 0x7FC1  # a bf16 NaN payload no kernel produces from finite inputs: marks what was never written


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from pytorch_models._hip import ops as o

    return o


def _seq(ops, lengths):
    return ops.seq_lens(list(lengths), max(max(lengths), 1), "cuda")


def _lut(case):
    return RC.table(case).cuda()


def _run(ops, case, buf, out=None, lut=None):
    """buf: a (T_total + SLACK, 3 * H * 64) bf16 device buffer laid out like varlen_cases.build's."""
    q, k, v = VC.qkv(case.vc, buf)
    return ops.attention_varlen(q, k, v, case.H, _seq(ops, case.lengths), case.causal, out,
                                rel_lut=_lut(case) if lut is None else lut, radius=case.R)


def _dev(case):
    return VC.build(case.vc).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_parity(ops, case):
    want, A = RC.reference(case)
    buf = _dev(case)
    got = _run(ops, case, buf)
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    ratio = RC.bound_ratio(got.float().cpu(), want, A)
    print(f"RATIO relbias {case.id} {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"
    assert torch.equal(got, _run(ops, case, buf)), "rerun must give the same bits"


@pytest.mark.parametrize("case", RC.LIVE_CASES, ids=lambda c: c.id)
def test_isolation(ops, case):
    """NaN in the q / k / v rows of every second sequence and in the slack rows: the other sequences do not see them."""
    buf = _dev(case)
    clean = _run(ops, case, buf)
    dirty = buf.clone()
    dirty[case.total:] = float("nan")
    for b, r0, n in VC.sequences(case.vc):
        if b % 2:
            dirty[r0 : r0 + n] = float("nan")
    got = _run(ops, case, dirty)
    kept = [(r0, n) for b, r0, n in VC.sequences(case.vc) if b % 2 == 0]
    assert kept
    for r0, n in kept:
        assert torch.isfinite(got[r0 : r0 + n].float()).all()
        assert torch.equal(got[r0 : r0 + n], clean[r0 : r0 + n])


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_extents(ops, case):
    """Every row of a live sequence is written in full (dead rows too: with zeros); rows past T_total keep their pattern."""
    T, D = case.total, case.H * 64
    out = torch.full((T + VC.SLACK, D), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    got = _run(ops, case, _dev(case), out=out[:T])
    assert got.data_ptr() == out.data_ptr()
    bits = out.view(torch.int16)
    assert (bits[T:] == PATTERN).all(), "rows past T_total were written"
    assert not (bits[:T] == PATTERN).any(), "a live row was not written in full"
    want, A = RC.reference(case)
    assert RC.bound_ratio(out[:T].float().cpu(), want, A) <= 1.5


@pytest.mark.parametrize("case", RC.LIVE_CASES, ids=lambda c: c.id)
def test_position_invariance(ops, case):
    """A sequence's rows do not depend on where it sits in the batch: the same bits as the call on it alone (B = 1)."""
    buf = _dev(case)
    got = _run(ops, case, buf)
    D, lut = case.H * 64, _lut(case)
    for _, r0, n in VC.sequences(case.vc):
        rows = buf[r0 : r0 + n]
        alone = ops.attention_varlen(rows[:, :D], rows[:, D : 2 * D], rows[:, 2 * D :], case.H, _seq(ops, [n]), case.causal,
                                     rel_lut=lut, radius=case.R)
        assert torch.equal(got[r0 : r0 + n], alone), f"{case.id}: sequence at row {r0}, length {n}"


@pytest.mark.parametrize("case", RC.LIVE_CASES, ids=lambda c: c.id)
def test_shared_tile_body(ops, case):
    """The bias path of ops.attention is the tiled kernel at every length, and the distance-table form shares its tile body
    behind the bias fetch: a sequence's rows are the bits pm_attention_bias_bf16 gives on that sequence alone with the dense
    (1, H, n, n) table gathered from the same values."""
    buf = _dev(case)
    got = _run(ops, case, buf)
    D, lut = case.H * 64, _lut(case)
    for _, r0, n in VC.sequences(case.vc):
        rows = buf[r0 : r0 + n][None]
        bias = RC.dense(lut, n, case.R)[None].contiguous()
        alone = ops.attention(rows[..., :D], rows[..., D : 2 * D], rows[..., 2 * D :], case.H, case.causal, bias)[0]
        assert torch.equal(got[r0 : r0 + n], alone), f"{case.id}: length {n}"


def test_a_wider_table_and_a_row_stride(ops):
    """The table may be wider than 2R + 1 and its rows may be a view: only [h, 0 .. 2R] is read."""
    case = next(c for c in RC.LIVE_CASES if c.R == 5 and c.table == "distinct" and c.lengths == (31, 32, 65, 127, 128) and not c.causal)
    buf = _dev(case)
    want = _run(ops, case, buf)
    wide = torch.full((case.H, 40), float("nan"), device="cuda")
    wide[:, : 2 * case.R + 1] = _lut(case)
    assert torch.equal(_run(ops, case, buf, lut=wide), want)
    assert torch.equal(_run(ops, case, buf, lut=wide[:, : 2 * case.R + 1]), want)


@pytest.mark.parametrize("case", RC.DEAD_CASES, ids=lambda c: c.id)
def test_dead_rows_are_zero(ops, case):
    got = _run(ops, case, _dev(case))
    assert torch.isfinite(got.float()).all() and (got.view(torch.int16) == 0).all()


def test_without_a_table_the_call_is_the_one_it_was(ops):
    case = VC.CASES[0]
    buf = VC.build(case).to(torch.bfloat16).cuda()
    q, k, v = VC.qkv(case, buf)
    seq = _seq(ops, case.lengths)
    assert torch.equal(ops.attention_varlen(q, k, v, case.H, seq, rel_lut=None, radius=None), ops.attention_varlen(q, k, v, case.H, seq))


def test_operand_checks(ops):
    """Each refusal is a ValueError raised on the host, in front of any launch: the output keeps its pattern."""
    case = next(c for c in RC.LIVE_CASES if c.R == 5)
    buf = _dev(case)
    q, k, v = VC.qkv(case.vc, buf)
    seq = _seq(ops, case.lengths)
    lut, R, H = _lut(case), case.R, case.H
    out = torch.full((case.total, H * 64), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    wide = torch.zeros(H, 4 * R + 2, device="cuda")
    bad = [
        dict(rel_lut=lut.double(), radius=R),                  # dtype
        dict(rel_lut=lut.to(torch.bfloat16), radius=R),
        dict(rel_lut=lut[0], radius=R),                        # shape: one dimension
        dict(rel_lut=torch.cat([lut, lut[:1]], 0), radius=R),  # shape: H + 1 rows
        dict(rel_lut=lut.cpu(), radius=R),                     # device
        dict(rel_lut=wide[:, ::2], radius=R),                  # strided last dimension
        dict(rel_lut=lut, radius=-1),
        dict(rel_lut=lut, radius=R + 1),                       # narrower than 2R + 1
        dict(rel_lut=lut[:, :-1], radius=R),
        dict(rel_lut=lut, radius=None),                        # one without the other
        dict(rel_lut=None, radius=R),
        dict(rel_lut=lut, radius=2.0),
        dict(rel_lut=torch.zeros(H, 2 * 513 + 1, device="cuda"), radius=513),  # past the LDS budget
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.attention_varlen(q, k, v, H, seq, case.causal, out, **kw)
    assert (out.view(torch.int16) == PATTERN).all()
    ok = ops.attention_varlen(q, k, v, H, seq, case.causal, out, rel_lut=torch.zeros(H, 1025, device="cuda"), radius=512)
    assert torch.isfinite(ok.float()).all()  # the largest table
