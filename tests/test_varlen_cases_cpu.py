"""CPU: the variable-length (packed) encoder path without a GPU.
  * every assertion tests/test_hip_varlen_kernels.py makes about pm_attention_varlen_bf16 is satisfiable: the bf16 kernels'
    arithmetic, emulated per sequence, stays within the asserted 1.5 x bf16_bound of the float64 reference on every case;
  * the new entry points validate on the host (PM_EINVAL / PM_EALIGN, nothing launched), ops.seq_lens rejects bad lengths, the
    wav2vec2 frame-length formula;
  * the CPU forms of BERT.forward / BERT.embed / Wav2Vec2.forward with lengths= against the oracles on each row alone, at the
    tolerances of tests/test_text_cpu.py and tests/test_audio_enc_cpu.py."""
import ctypes

import pytest
import torch

import varlen_cases as VC
from oracle import ref_audio as RA
from oracle import ref_text as RX
from synthweights import fill_module, synth_input, synth_tokens

torch.set_grad_enabled(False)
TOL = dict(rtol=2e-5, atol=2e-5)          # tests/test_text_cpu.py
TOL_AUDIO = dict(rtol=2e-5, atol=1e-4)    # tests/test_audio_enc_cpu.py (full forward)
EINVAL, EUNSUPPORTED, EALIGN = 1, 2, 4


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.id)
def test_emulated_kernel_stays_within_the_asserted_bound(case):
    want, A = VC.reference(case)
    got = VC.emulate(case)
    assert got.shape == want.shape == (case.total, case.H * 64)
    ratio = VC.bound_ratio(got, want, A)
    print(f"RATIO emulated {case.id} {ratio:.3f}")
    assert ratio <= 1.5


def test_cases_cover_the_kernel_edges():
    ids = [c.id for c in VC.CASES]
    assert len(set(ids)) == len(ids) == 48
    lens = {n for c in VC.CASES for n in c.lengths}
    assert {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 300} <= lens
    buf = VC.build(VC.CASES[0])
    assert buf.shape == (VC.CASES[0].total + VC.SLACK, 3 * VC.CASES[0].H * 64) and torch.equal(buf, VC.bf16r(buf))


def test_host_side_validation_launches_nothing():
    """Rejected calls return before any HIP call, so this runs without a GPU (tests/test_abi.py style)."""
    from pytorch_models import _hip

    L = _hip.lib()
    raw = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(raw) // 16 * 16 + 16
    att = L.pm_attention_varlen_bf16
    ok = dict(q=p, qs=384, k=p + 256, ks=384, v=p + 512, vs=384, o=p, os=128, cu=p, B=2, H=2, max_len=40, causal=0)

    def call(**kw):
        a = {**ok, **kw}
        return att(a["q"], a["qs"], a["k"], a["ks"], a["v"], a["vs"], a["o"], a["os"], a["cu"], a["B"], a["H"], a["max_len"], a["causal"], None)

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(cu=None), dict(B=-1), dict(H=0), dict(max_len=0),
               dict(max_len=-3), dict(qs=64), dict(os=64)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(qs=388), dict(ks=386), dict(vs=391), dict(os=130), dict(q=p + 8), dict(v=p + 2), dict(o=p + 4), dict(cu=p + 2)):
        assert call(**kw) == EALIGN, kw
    assert call(B=0) == 0  # nothing to do, nothing launched

    assert L.pm_embed_tokens_varlen(None, p, 0, p, p, p, 0, 2, 8, 64, 100, None) == EINVAL
    assert L.pm_embed_tokens_varlen(p, p, 0, p, None, p, 0, 2, 8, 64, 100, None) == EINVAL
    assert L.pm_embed_tokens_varlen(p, p, 7, p, p, p, 0, 2, 8, 64, 100, None) == EINVAL
    assert L.pm_embed_tokens_varlen(p, p, 1, p, p, p, 0, 2, 8, 64, 100, None) == EUNSUPPORTED  # f32 table, bf16 rows
    assert L.pm_embed_tokens_varlen(p, p, 0, p, p, p, 0, 2, 8, 68, 100, None) == EUNSUPPORTED
    assert L.pm_embed_tokens_varlen(p, p + 8, 0, p, p, p, 0, 2, 8, 64, 100, None) == EALIGN
    assert L.pm_embed_tokens_varlen(p, p, 0, p, p, p, 0, 0, 8, 64, 100, None) == 0

    assert L.pm_rows_pack(None, 512, 64, p, p, 64, 2, 8, 64, 2, None) == EINVAL
    assert L.pm_rows_pack(p, 512, 64, p, p, 64, 2, 8, 64, 3, None) == EINVAL        # element width
    assert L.pm_rows_pack(p, 512, 32, p, p, 64, 2, 8, 64, 2, None) == EINVAL        # rows overlap
    assert L.pm_rows_pack(p, 512, 68, p, p, 68, 2, 8, 68, 2, None) == EUNSUPPORTED  # 136-byte rows
    assert L.pm_rows_pack(p, 516, 64, p, p, 64, 2, 8, 64, 2, None) == EALIGN
    assert L.pm_rows_pack(p, 512, 64, p, p + 4, 64, 2, 8, 64, 2, None) == EALIGN
    assert L.pm_rows_unpack(p, 64, None, p, 512, 64, 2, 8, 64, 2, None) == EINVAL
    assert L.pm_rows_unpack(p, 66, p, p, 512, 64, 2, 8, 64, 4, None) == EALIGN
    assert L.pm_rows_zero_tail(None, 512, 64, p, 2, 8, 64, 2, None) == EINVAL
    assert L.pm_rows_zero_tail(p + 2, 512, 64, p, 2, 8, 64, 2, None) == EALIGN
    assert L.pm_rows_zero_tail(p, 512, 64, p, 2, 0, 64, 2, None) == 0

    assert L.pm_segment_mean(None, 64, 0, p, p, 2, 64, None) == EINVAL
    assert L.pm_segment_mean(p, 64, 5, p, p, 2, 64, None) == EINVAL
    assert L.pm_segment_mean(p, 32, 0, p, p, 2, 64, None) == EINVAL
    assert L.pm_segment_mean(p, 68, 0, p, p, 2, 68, None) == EUNSUPPORTED
    assert L.pm_segment_mean(p, 68, 0, p, p, 2, 64, None) == EALIGN
    assert L.pm_segment_mean(p, 64, 1, p, p + 8, 2, 64, None) == EALIGN
    assert L.pm_segment_mean(p, 64, 0, p, p, 0, 64, None) == 0


def test_seq_lens_validates_on_the_host():
    from pytorch_models._hip import ops

    s = ops.seq_lens([3, 0, 5], 5, "cpu")
    assert s.lengths == [3, 0, 5] and s.cu.tolist() == [0, 3, 3, 8] and s.cu.dtype == torch.int32
    assert (s.B, s.L, s.total, s.max_len) == (3, 5, 8, 5)
    assert ops.seq_lens(torch.tensor([2, 1]), 4, "cpu").cu.tolist() == [0, 2, 3]
    for bad in ([6], [-1], [2.0], [True], torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError):
            ops.seq_lens(bad, 5, "cpu")
    with pytest.raises(ValueError):
        ops.seq_lens([0, 3], 5, "cpu", lo=1)


def test_frame_length_follows_the_stem():
    from pytorch_models.audio import Wav2Vec2

    assert [Wav2Vec2.frame_length(n) for n in (9600, 6400, 4000, 400)] == [29, 19, 12, 1]
    assert Wav2Vec2.frame_length(399) == 0 and Wav2Vec2.frame_length(0) == 0


BERT_LENGTHS = [70, 33, 1, 64]


@pytest.fixture(scope="module")
def bert():
    from pytorch_models.text import BERT

    m = BERT(2000, 2, 128).eval()
    fill_module(m, 74)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = synth_tokens("varlen_tok", (4, 70), 2000, 75)
    rows = [RX.bert(sd, x[b : b + 1, :n])[0] for b, n in enumerate(BERT_LENGTHS)]
    return m, x, rows


def test_cpu_bert_forward_with_lengths_is_each_row_alone(bert):
    m, x, rows = bert
    y = m(x, lengths=BERT_LENGTHS)
    assert y.shape == (4, 70, 128)
    for b, n in enumerate(BERT_LENGTHS):
        torch.testing.assert_close(y[b, :n], rows[b], **TOL)
        assert (y[b, n:] == 0).all()
    torch.testing.assert_close(m(x, lengths=torch.tensor(BERT_LENGTHS)), y, rtol=0, atol=0)
    # what sits in the padding does not matter
    x2 = x.clone()
    for b, n in enumerate(BERT_LENGTHS):
        x2[b, n:] = 1999 - x2[b, n:]
    assert torch.equal(m(x2, lengths=BERT_LENGTHS), y)


def test_cpu_bert_embed_pools_the_valid_rows(bert):
    m, x, rows = bert
    mean, cls = m.embed(x, BERT_LENGTHS), m.embed(x, BERT_LENGTHS, pool="cls")
    assert mean.shape == cls.shape == (4, 128) and mean.dtype == cls.dtype == torch.float32
    torch.testing.assert_close(mean, torch.stack([r.double().mean(0) for r in rows]).float(), **TOL)
    torch.testing.assert_close(cls, torch.stack([r[0] for r in rows]), **TOL)
    full = m.embed(x[:2, :16])  # lengths=None: every row is full
    torch.testing.assert_close(full, RX.bert({k: v for k, v in m.state_dict().items()}, x[:2, :16]).mean(1), **TOL)
    with pytest.raises(ValueError):
        m.embed(x, BERT_LENGTHS, pool="max")


def test_cpu_bert_refuses_bad_lengths(bert):
    m, x, _ = bert
    for bad in ([70, 33, 0, 64], [71, 33, 1, 64], [70, 33, 1], [70, 33, 1, 64, 2], [70.0, 33, 1, 64]):
        with pytest.raises(ValueError):
            m(x, lengths=bad)


def test_cpu_wav2vec2_forward_with_lengths_is_each_clip_alone():
    from pytorch_models.audio import Wav2Vec2

    lengths = [9600, 6400, 4000, 400]
    for pre_norm, seed in ((True, 82), (False, 87)):
        m = Wav2Vec2(2, 64, pre_norm=pre_norm).eval()
        fill_module(m, seed)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        x = synth_input("varlen_wave", (4, 9600), 81)
        y = m(x, lengths=lengths)
        assert y.shape == (4, 29, 64)
        for b, n in enumerate(lengths):
            want = RA.wav2vec2(sd, x[b : b + 1, :n], pre_norm=pre_norm)[0]
            assert want.shape[0] == Wav2Vec2.frame_length(n)
            torch.testing.assert_close(y[b, : want.shape[0]], want, **TOL_AUDIO)
            assert (y[b, want.shape[0]:] == 0).all()
    for bad in ([9600, 6400, 4000, 399], [9601, 6400, 4000, 400], [9600, 6400, 4000]):
        with pytest.raises(ValueError):
            m(x, lengths=bad)
    legacy = Wav2Vec2(1, 64, stem_bias=False, stem_legacy=True).eval()
    with pytest.raises(NotImplementedError, match="over TIME"):
        legacy(x, lengths=lengths)
    with pytest.raises(RuntimeError, match="HIP devices only"):  # a call without lengths is the call it was
        m(torch.zeros(1, 400))
