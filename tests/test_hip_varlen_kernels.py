"""GPU: the kernels of variable-length (packed) encoder batches through the C ABI - pm_attention_varlen_bf16 against the float64
reference of tests/varlen_cases.py (bound_ratio <= 1.5, the contract of tests/attn_cases.py; tests/test_varlen_cases_cpu.py
shows on the CPU that a correct kernel satisfies it), its isolation, extents, position invariance and the bit identity with the
tiled kernel of pm_attention_bf16 that sharing the tile body gives; the row movers, the segment mean and the packed embedding.
Each test prints the figure it asserts ("RATIO ..." lines, pytest -s)."""
import pytest
import torch

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


def _run(ops, case, buf, out=None):
    """buf: a (T_total + SLACK, 3 * H * 64) bf16 device buffer laid out like VC.build's."""
    q, k, v = VC.qkv(case, buf)
    return ops.attention_varlen(q, k, v, case.H, _seq(ops, case.lengths), case.causal, out)


def _dev(case):
    return VC.build(case).to(torch.bfloat16).cuda()


SCALE1 = [c for c in VC.CASES if c.family == "scale" and c.scale == 1.0]


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.id)
def test_parity(ops, case):
    want, A = VC.reference(case)
    buf = _dev(case)
    got = _run(ops, case, buf)
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    ratio = VC.bound_ratio(got.float().cpu(), want, A)
    print(f"RATIO varlen {case.id} {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"
    assert torch.equal(got, _run(ops, case, buf)), "rerun must give the same bits"


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.id)
def test_isolation(ops, case):
    """NaN in the q / k / v rows of every second sequence and in the slack rows: the other sequences do not see them."""
    buf = _dev(case)
    clean = _run(ops, case, buf)
    dirty = buf.clone()
    dirty[case.total:] = float("nan")
    for b, r0, n in VC.sequences(case):
        if b % 2:
            dirty[r0 : r0 + n] = float("nan")
    got = _run(ops, case, dirty)
    kept = [(r0, n) for b, r0, n in VC.sequences(case) if b % 2 == 0]
    assert kept
    for r0, n in kept:
        assert torch.isfinite(got[r0 : r0 + n].float()).all()
        assert torch.equal(got[r0 : r0 + n], clean[r0 : r0 + n])


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.id)
def test_extents(ops, case):
    """Every row of a live sequence is written in full; rows past T_total - the only rows that belong to nothing: a sequence of
    length 0 owns none - keep the pattern they held."""
    T, D = case.total, case.H * 64
    out = torch.full((T + VC.SLACK, D), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    got = _run(ops, case, _dev(case), out=out[:T])
    assert got.data_ptr() == out.data_ptr()
    bits = out.view(torch.int16)
    assert (bits[T:] == PATTERN).all(), "rows past T_total were written"
    assert not (bits[:T] == PATTERN).any(), "a live row was not written in full"
    want, A = VC.reference(case)
    assert VC.bound_ratio(out[:T].float().cpu(), want, A) <= 1.5


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.id)
def test_position_invariance(ops, case):
    """A sequence's rows do not depend on where it sits in the batch: the same bits as the varlen call on it alone (B = 1)."""
    buf = _dev(case)
    got = _run(ops, case, buf)
    D = case.H * 64
    for _, r0, n in VC.sequences(case):
        rows = buf[r0 : r0 + n]
        alone = ops.attention_varlen(rows[:, :D], rows[:, D : 2 * D], rows[:, 2 * D :], case.H, _seq(ops, [n]), case.causal)
        assert torch.equal(got[r0 : r0 + n], alone), f"{case.id}: sequence at row {r0}, length {n}"


@pytest.mark.parametrize("case", [c for c in VC.CASES if c.lengths == (257, 1, 300)], ids=lambda c: c.id)
def test_shared_tile_body(ops, case):
    """Above 256 tokens ops.attention is the tiled kernel; the variable-length form shares its tile body, so a sequence's rows
    are the bits pm_attention_bf16 gives on that sequence alone."""
    buf = _dev(case)
    got = _run(ops, case, buf)
    D = case.H * 64
    for _, r0, n in VC.sequences(case):
        if n <= 256:
            continue
        rows = buf[r0 : r0 + n][None]
        alone = ops.attention(rows[..., :D], rows[..., D : 2 * D], rows[..., 2 * D :], case.H, case.causal)[0]
        assert torch.equal(got[r0 : r0 + n], alone), f"{case.id}: length {n}"


def test_attention_varlen_checks_its_operands(ops):
    case = SCALE1[0]
    buf = _dev(case)
    q, k, v = VC.qkv(case, buf)
    seq = _seq(ops, case.lengths)
    with pytest.raises(ValueError):
        ops.attention_varlen(q[:-1], k[:-1], v[:-1], case.H, seq)       # rows != sum(lengths)
    with pytest.raises(ValueError):
        ops.attention_varlen(q, k, v, case.H * 2, seq)                   # head_dim 32
    with pytest.raises(ValueError):
        ops.attention_varlen(q.float(), k.float(), v.float(), case.H, seq)
    with pytest.raises(RuntimeError):
        ops.attention_varlen(q.cpu(), k.cpu(), v.cpu(), case.H, seq)
    empty = ops.attention_varlen(q[:0], k[:0], v[:0], case.H, _seq(ops, [0, 0]))
    assert empty.shape == (0, case.H * 64)


ROW_LENGTHS = (5, 0, 9, 1, 9)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("d", [64, 72])
def test_rows_pack_unpack_zero_tail(ops, dtype, d):
    from synthweights import synth_input

    B, L = len(ROW_LENGTHS), 9
    big = synth_input("rows_x", (B, L + 3, d), 91).to(dtype).cuda()
    x = big[:, :L]  # a batch stride that is not L * d
    assert not x.is_contiguous()
    seq = ops.seq_lens(list(ROW_LENGTHS), L, "cuda")
    want_packed = torch.cat([x[b, :n] for b, n in enumerate(ROW_LENGTHS)], 0)
    packed = ops.rows_pack(x, seq)
    assert packed.shape == (sum(ROW_LENGTHS), d) and torch.equal(packed, want_packed)
    want_padded = torch.zeros(B, L, d, dtype=dtype, device="cuda")
    for b, n in enumerate(ROW_LENGTHS):
        want_padded[b, :n] = x[b, :n]
    assert torch.equal(ops.rows_unpack(packed, seq), want_padded)
    # NaN behind the lengths: pack does not read it, zero_tail removes it, in place, and touches nothing else
    y = big.clone()
    for b, n in enumerate(ROW_LENGTHS):
        y[b, n:L] = float("nan")
    assert torch.equal(ops.rows_pack(y[:, :L], seq), want_packed)
    z = ops.rows_zero_tail(y[:, :L], seq)
    assert z.data_ptr() == y.data_ptr() and torch.equal(y[:, :L], want_padded) and torch.equal(y[:, L:], big[:, L:])
    with pytest.raises(ValueError):
        ops.rows_pack(x[:, :, :58], seq)  # rows that are no multiple of 16 bytes
    with pytest.raises(ValueError):
        ops.rows_unpack(packed[:-1], seq)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_segment_mean(ops, dtype):
    """fp32 sums in row order and one divide: |got - want| <= gamma_n mean|x| + 2^-24 |want|, gamma_n = n u / (1 - n u), u = 2^-24
    (the standard bound of recursive summation, n the sequence's length); a second run gives the same bits."""
    from synthweights import synth_input

    lengths = (300, 1, 0, 77, 512)
    d = 72
    x = synth_input("segmean_x", (sum(lengths), d), 92, scale=3.0).to(dtype)
    seq = ops.seq_lens(list(lengths), 512, "cuda")
    got = ops.segment_mean(x.cuda(), seq)
    assert got.shape == (len(lengths), d) and got.dtype == torch.float32
    assert torch.equal(got, ops.segment_mean(x.cuda(), seq))
    got, u, r0 = got.cpu().double(), 2.0 ** -24, 0
    for b, n in enumerate(lengths):
        if n == 0:
            assert (got[b] == 0).all()
            continue
        rows = x[r0 : r0 + n].double()
        want = rows.mean(0)
        bound = n * u / (1 - n * u) * rows.abs().mean(0) + u * want.abs()
        err = (got[b] - want).abs()
        print(f"RATIO segment_mean {dtype} n={n} {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        r0 += n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_embed_tokens_varlen(ops, dtype):
    from synthweights import synth_input, synth_tokens

    V, d, L = 500, 72 if dtype == torch.float32 else 64, 9
    E = synth_input("vemb_E", (V, d), 93).to(dtype).cuda()
    pos = synth_input("vemb_pos", (L + 2, d), 94).cuda()
    tok = synth_tokens("vemb_tok", (len(ROW_LENGTHS), L), V, 95).cuda()
    seq = ops.seq_lens(list(ROW_LENGTHS), L, "cuda")
    got = ops.embed_tokens_varlen(tok, E, pos, seq)
    assert got.shape == (sum(ROW_LENGTHS), d) and got.dtype == dtype
    r0 = 0
    for b, n in enumerate(ROW_LENGTHS):
        if n:
            assert torch.equal(got[r0 : r0 + n], ops.embed_tokens(tok[b : b + 1, :n], E, pos)[0])
        r0 += n
    assert torch.equal(ops.embed_tokens_varlen(tok, E, None, seq), torch.cat([E[tok[b, :n]] for b, n in enumerate(ROW_LENGTHS)], 0))
    # the id range check covers valid positions only: padding may hold anything, a bad id inside a sequence raises
    bad = tok.clone()
    for b, n in enumerate(ROW_LENGTHS):
        bad[b, n:] = V + 7
    assert torch.equal(ops.embed_tokens_varlen(bad, E, pos, seq), got)
    bad[2, 3] = V
    with pytest.raises(IndexError):
        ops.embed_tokens_varlen(bad, E, pos, seq)
