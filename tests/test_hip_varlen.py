"""GPU: variable-length batches through the models - BERT.forward / BERT.embed and Wav2Vec2.forward with lengths= against the
fp32 oracles on every row ALONE (the same bf16-rounded weights), at the contracts tests/test_hip_text.py and
tests/test_hip_audio_enc.py apply to these models (rel-L2 < 2e-2); padded rows exactly 0; a call without lengths is bit for bit
the call it was; the refusals."""
import pytest
import torch

from oracle import ref_audio as RA
from oracle import ref_text as RX
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def rel(got, want):
    got, want = got.double().cpu(), want.double()
    return ((got - want).norm() / want.norm()).item()


def prep(m, seed):
    fill_module(m, seed)
    bf16_round_(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(torch.bfloat16).cuda().eval(), sd


BERT_LENGTHS = [70, 33, 1, 64]


@pytest.fixture(scope="module")
def bert():
    from pytorch_models.text import BERT

    m, sd = prep(BERT(2000, 2, 128), 74)
    x = synth_tokens("varlen_tok", (4, 70), 2000, 75)
    rows = [RX.bert(sd, x[b : b + 1, :n])[0] for b, n in enumerate(BERT_LENGTHS)]
    return m, x, rows, sd


def test_bert_forward_with_lengths_is_each_row_alone(bert):
    m, x, rows, sd = bert
    y = m(x.cuda(), lengths=BERT_LENGTHS)
    assert y.shape == (4, 70, 128) and y.dtype == torch.bfloat16
    for b, n in enumerate(BERT_LENGTHS):
        r = rel(y[b, :n], rows[b])
        print(f"REL bert row {b} (length {n}) {r:.3e}")
        assert r < 2e-2
        assert (y[b, n:] == 0).all(), "padded rows must be exactly 0"
    assert torch.equal(m(x.cuda(), lengths=torch.tensor(BERT_LENGTHS)), y)
    x2 = x.clone()  # the ids in the padding are never read
    for b, n in enumerate(BERT_LENGTHS):
        x2[b, n:] = 5000
    assert torch.equal(m(x2.cuda(), lengths=BERT_LENGTHS), y)


def test_bert_embed_pools_the_valid_rows(bert):
    m, x, rows, sd = bert
    mean, cls = m.embed(x.cuda(), BERT_LENGTHS), m.embed(x.cuda(), BERT_LENGTHS, pool="cls")
    assert mean.shape == cls.shape == (4, 128) and mean.dtype == cls.dtype == torch.float32
    r_mean = rel(mean, torch.stack([r.double().mean(0) for r in rows]))
    r_cls = rel(cls, torch.stack([r[0].double() for r in rows]))
    print(f"REL bert embed mean {r_mean:.3e} cls {r_cls:.3e}")
    assert r_mean < 2e-2 and r_cls < 2e-2
    y = m(x.cuda(), lengths=BERT_LENGTHS)
    assert torch.equal(cls, y[:, 0].float())
    full = m.embed(x[:2, :16].cuda())  # lengths=None: every row is full
    assert rel(full, RX.bert(sd, x[:2, :16]).double().mean(1)) < 2e-2


def test_bert_without_lengths_is_the_call_it_was(bert):
    from pytorch_models._hip import ops
    from pytorch_models.transformer import _f32

    m, x, _, _ = bert
    xc = x.cuda()
    old = m.layers(m.norm(ops.embed_tokens(xc, m.token_embs.weight, _f32(m, "pos", m.pos_embs))))  # the forward before lengths=
    assert torch.equal(m(xc), old) and torch.equal(m(xc, lengths=None), old) and torch.equal(m(xc, None), old)


def test_bert_refusals(bert):
    from pytorch_models.text import BERT

    m, x, _, _ = bert
    xc = x.cuda()
    for bad in ([70, 33, 0, 64], [71, 33, 1, 64], [70, 33, 1], [70.0, 33.0, 1.0, 64.0]):
        with pytest.raises(ValueError):
            m(xc, lengths=bad)
    with pytest.raises(ValueError):
        m(xc[None], lengths=BERT_LENGTHS)
    m32 = BERT(2000, 1, 128).cuda().eval()
    with pytest.raises(NotImplementedError, match="bf16"):
        m32(xc, lengths=BERT_LENGTHS)
    with pytest.raises(NotImplementedError, match="bf16"):
        m32.embed(xc, BERT_LENGTHS)


W2V_LENGTHS = [9600, 6400, 4000, 400]


def test_wav2vec2_forward_with_lengths_is_each_clip_alone():
    from pytorch_models.audio import Wav2Vec2

    m, sd = prep(Wav2Vec2(2, 128), 82)
    x = synth_input("varlen_wave", (4, 9600), 81)
    y = m(x.cuda(), lengths=W2V_LENGTHS)
    assert y.shape == (4, 29, 128) and y.dtype == torch.bfloat16
    for b, n in enumerate(W2V_LENGTHS):
        want = RA.wav2vec2(sd, x[b : b + 1, :n])[0]
        f = want.shape[0]
        assert f == Wav2Vec2.frame_length(n)
        r = rel(y[b, :f], want)
        print(f"REL wav2vec2 clip {b} ({n} samples, {f} frames) {r:.3e}")
        assert r < 2e-2
        assert (y[b, f:] == 0).all(), "padded frames must be exactly 0"
    x2 = x.clone()  # the samples behind a clip's end do not reach its frames
    for b, n in enumerate(W2V_LENGTHS):
        x2[b, n:] = 0.5
    y2 = m(x2.cuda(), lengths=W2V_LENGTHS)
    for b, n in enumerate(W2V_LENGTHS):
        f = Wav2Vec2.frame_length(n)
        assert torch.equal(y2[b, :f], y[b, :f])
    assert torch.equal(m(x.cuda()), m(x.cuda(), lengths=None))


def test_wav2vec2_refusals():
    from pytorch_models.audio import Wav2Vec2

    x = synth_input("varlen_wave", (4, 9600), 81).cuda()
    legacy = Wav2Vec2(1, 128, stem_bias=False, stem_legacy=True).to(torch.bfloat16).cuda().eval()
    with pytest.raises(NotImplementedError, match="over TIME"):
        legacy(x, lengths=W2V_LENGTHS)
    m = Wav2Vec2(1, 128).to(torch.bfloat16).cuda().eval()
    for bad in ([9600, 6400, 4000, 0], [9600, 6400, 4000, 399], [9601, 6400, 4000, 400], [9600, 6400]):
        with pytest.raises(ValueError):
            m(x, lengths=bad)
    with pytest.raises(NotImplementedError, match="bf16"):
        Wav2Vec2(1, 128).cuda().eval()(x, lengths=W2V_LENGTHS)
