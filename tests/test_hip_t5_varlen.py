"""GPU: ragged source batches through T5 - T5Model.encode(x, lengths), score / forward(..., src_lengths=) and
generate(..., lengths=, packed=True) - on the small geometries of tests/t5_generate_cases.py (one with heads * 64 != d) and the
scoring model of tests/score_cases.py, against oracle/ref_t5.py (fp32, CPU) on the same bf16-rounded weights.

Bounds.  encode: every row on [:len_b] within rel-L2 2e-2 of the oracle's encoder on that row alone (forward's contract in this
project), rows past len_b exactly 0, padding ids irrelevant bit for bit.  forward with src_lengths: row b's logits within rel-L2
2e-2 of the oracle's model on (x[b, :len_b], targets[b]).  score with src_lengths: against float64 log_softmax of forward with the
same src_lengths under score_cases.model_reference at MARGIN = 1.5, and row b against score on the row alone, x[b:b+1, :len_b],
BIT FOR BIT - what tests/test_hip_score.py asserts of its ragged rows (test_a_lengths_row_equals_the_row_scored_alone).  The
encoder side of that identity is by construction (the packed attention shares the dense-bias kernel's tile body, everything else
is row-wise); the masked cross-attention runs the tiled bias kernel where the row alone runs the short-sequence one, and the two
agree in every stored bf16 value at these pinned shapes.  On top of it, loosely, both sides against the oracle's log-probabilities
on the row alone (forward's 2e-2 contract on the logits, twice the largest logit error on a log-probability).
generate: ids follow the oracle up to each row's first decision under MARGIN = 0.05 (test_hip_t5_generate.py's rule).
Calls without lengths are compared bit for bit with the code path they had."""
import pytest
import torch

import score_cases as sc
import t5_generate_cases as TC
from oracle import ref_t5 as R5
from synthweights import synth_tokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
S = 130
LENGTHS = [0, 1, 63, 65, 127, 130]  # none, one, either side of the 64-key tile and of the 128-query block, S itself
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


@pytest.mark.parametrize("case", ["inner_ne_d", "h8_l4"])
def test_encode_with_lengths_is_each_row_alone(case):
    m, sd = gpu_model(case)
    tok = synth_tokens("t5_varlen_tok", (len(LENGTHS), S), 1000, 101)
    y = m.encode(tok.cuda(), LENGTHS)
    assert y.shape == (len(LENGTHS), S, 512) and y.dtype == torch.bfloat16
    E = sd["token_embs.weight"]
    errs = []
    for b, n in enumerate(LENGTHS):
        assert (y[b, n:].view(torch.int16) == 0).all(), f"row {b}: rows past its length must be exactly zero"
        if n:
            errs.append(rel(y[b, :n], R5.encoder(sd, "encoder.", E[tok[b, :n]])))
    print(f"RATIO t5 encode lengths {case}: rel-L2 per row {[f'{e:.2e}' for e in errs]} (asserted <= 2e-2)")
    assert max(errs) <= 2e-2, errs
    # lengths as a tensor (host or device) == as a list; a second call gives the same bits
    assert torch.equal(m.encode(tok.cuda(), torch.tensor(LENGTHS)), y) and torch.equal(m.encode(tok.cuda(), torch.tensor(LENGTHS).cuda()), y)
    # whatever sits in the padding: never read
    other = tok.clone()
    for b, n in enumerate(LENGTHS):
        other[b, n:] = (other[b, n:] + 17 + b) % 1000
    assert not torch.equal(other, tok) and torch.equal(m.encode(other.cuda(), LENGTHS), y)
    # full rows through the packed route against the dense route: two schedules of the same arithmetic, forward's contract
    full = m.encode(tok[:2].cuda(), [S, S])
    dense = m.encode(tok[:2].cuda())
    assert rel(full, dense.float().cpu()) <= 2e-2
    assert torch.equal(m.encode(tok[:2].cuda(), [0, 0]), torch.zeros_like(dense))


def test_calls_without_lengths_are_the_calls_they_were():
    m, _ = gpu_model("inner_ne_d")
    tok = synth_tokens("t5_varlen_tok", (3, S), 1000, 101).cuda()
    tgt = synth_tokens("t5_varlen_tgt", (3, 7), 1000, 102).cuda()
    want = m.encoder(m._embed(tok))
    assert torch.equal(m.encode(tok), want) and torch.equal(m.encode(tok, lengths=None), want) and torch.equal(m.encode(tok, None), want)
    logits = m.decode(tgt, want)
    assert torch.equal(m(tok, tgt), logits) and torch.equal(m(tok, tgt, src_lengths=None), logits) and torch.equal(m.forward(tok, tgt, None), logits)
    # the decoder with the default memory_bias launches what it launched
    h = m.decoder(m._embed(tgt), want)
    assert torch.equal(m.decoder(m._embed(tgt), want, None), h) and torch.equal(m.decoder(m._embed(tgt), want, memory_bias=None), h)
    blk = m.decoder.layers[0]
    x = m._embed(tgt)
    assert torch.equal(blk(x, want, causal=True), blk(x, want, causal=True, memory_bias=None))
    # a key mask without a masked key changes the kernel, not the result beyond forward's contract
    zero = torch.zeros(3, 1, 1, S, device="cuda")
    assert rel(m.decoder(m._embed(tgt), want, zero), h.float().cpu()) <= 2e-2


SRC_LENGTHS = [70, 33, 1]
TGT_LENGTHS = [9, 5, 2]


@pytest.fixture(scope="module")
def scoring():
    cpu = sc.small_t5()
    sd = {k: v.clone() for k, v in cpu.state_dict().items()}
    m = sc.small_t5().to(torch.bfloat16).cuda()
    src = synth_tokens("t5_varlen_src", (3, 70), 1001, 23)
    tgt = synth_tokens("t5_varlen_score", (3, 9), 1001, 24)
    return m, sd, src, tgt


def test_forward_with_src_lengths_is_each_row_alone(scoring):
    m, sd, src, tgt = scoring
    logits = m(src.cuda(), tgt.cuda(), src_lengths=SRC_LENGTHS)
    assert logits.shape == (3, 9, 1001) and logits.dtype == torch.float32 and torch.isfinite(logits).all()
    errs = [rel(logits[b], R5.model(sd, src[b, :n], tgt[b])) for b, n in enumerate(SRC_LENGTHS)]
    print(f"RATIO t5 forward src_lengths: rel-L2 per row {[f'{e:.2e}' for e in errs]} (asserted <= 2e-2)")
    assert max(errs) <= 2e-2, errs
    # without src_lengths the padding is attended to: the short rows are then NOT the rows alone (what the argument is for)
    plain = m(src.cuda(), tgt.cuda())
    assert rel(plain[0], R5.model(sd, src[0], tgt[0])) <= 2e-2
    assert rel(plain[2], R5.model(sd, src[2, :1], tgt[2])) > 2e-2
    other = src.clone()
    for b, n in enumerate(SRC_LENGTHS):
        other[b, n:] = (other[b, n:] + 17 + b) % 1001
    assert torch.equal(m(other.cuda(), tgt.cuda(), src_lengths=SRC_LENGTHS), logits)
    assert torch.equal(m(src.cuda(), tgt.cuda(), src_lengths=torch.tensor(SRC_LENGTHS)), logits)


@pytest.mark.parametrize("ragged", (False, True), ids=("full", "lengths"))
def test_score_with_src_lengths(scoring, ragged):
    m, sd, src, tgt = scoring
    src, tgt = src.cuda(), tgt.cuda()
    lengths = TGT_LENGTHS if ragged else None
    got, am = m.score(src, tgt, lengths, src_lengths=SRC_LENGTHS, return_argmax=True)
    assert got.shape == (3, 8) and got.dtype == torch.float32 and am.shape == (3, 8)
    # (1) test_hip_score.py's tolerance: float64 log_softmax(forward) of the SAME model and call form, on the shared hidden rows
    logits = m(src, tgt, src_lengths=SRC_LENGTHS)
    h, W = m.hidden_rows(tgt, *m._encode_src(src, SRC_LENGTHS, "test"))
    want, bound, ref, _ = sc.model_reference(logits, h, W, tgt.cpu(), lengths)
    r = sc.ratio(got.cpu(), want, bound)
    print(f"RATIO t5 score src_lengths {'lengths' if ragged else 'full'}: vs fp64 log_softmax(forward) {r:.3f} of the bound (asserted <= {sc.MARGIN})")
    assert r <= sc.MARGIN
    assert sc.argmax_ok(ref, am.reshape(-1))
    assert torch.equal(m.score(src, tgt, lengths, src_lengths=SRC_LENGTHS), got)
    # (2) the row alone, cut to its own source length, through the call without src_lengths, and the oracle on that row
    for b, n in enumerate(SRC_LENGTHS):
        nt = TGT_LENGTHS[b] if ragged else 9
        alone = m.score(src[b : b + 1, :n].contiguous(), tgt[b : b + 1], None if lengths is None else [nt])
        o = R5.model(sd, src[b, :n].cpu(), tgt[b].cpu()).double()
        want_b = torch.log_softmax(o, -1)[:-1].gather(1, tgt[b, 1:].cpu()[:, None])[:, 0]
        tol = 2 * 2e-2 * o[:-1].norm(dim=-1)
        keep = torch.arange(1, 9) < nt
        e_got, e_alone = (got[b].cpu().double() - want_b).abs(), (alone[0].cpu().double() - want_b).abs()
        print(f"RATIO t5 score src_lengths row {b}: |score - oracle| / tol max {float((e_got / tol)[keep].max()) if keep.any() else 0.0:.3f}, "
              f"row alone {float((e_alone / tol)[keep].max()) if keep.any() else 0.0:.3f}, "
              f"|score - alone| max {float((got[b] - alone[0]).abs().max()):.3e}")
        assert torch.equal(got[b : b + 1].view(torch.int32), alone.view(torch.int32)), f"row {b} is not the row scored alone"
        assert (e_got[keep] <= tol[keep]).all() and (e_alone[keep] <= tol[keep]).all()
        assert (got[b].cpu()[~keep] == 0).all() and (got[b].cpu()[keep] < 0).all()
    # without src_lengths: today's bits
    assert torch.equal(m.score(src, tgt, lengths), m.score(src, tgt, lengths, src_lengths=None))


def test_generate_with_the_packed_encoder():
    m, _ = gpu_model("h8_l4")
    tok, lengths, _ = TC.sources("h8_l4")
    o, n = TC.oracle("h8_l4"), 24
    tok = tok.cuda()
    ids, out_len = m.generate(tok, lengths=lengths, max_new_tokens=n, eos_id=-1, packed=True)
    assert state(m).encoder_bias_bytes == 0
    assert ids.shape == (8, n + 1) and torch.equal(out_len.cpu(), torch.full((8,), n + 1))
    kept = 0
    for b in range(8):
        low = (o["margins"][b][:n] < TC.MARGIN).nonzero()
        first = int(low[0]) if len(low) else n  # decisions 0 .. first - 1 are decided: positions 1 .. first
        kept += first
        assert torch.equal(ids[b, : first + 1].cpu(), o["ids"][b, : first + 1]), (b, first)
    print(f"packed free run: {kept} of {8 * n} decisions precede the first near-tie")
    # the default stays the dense-table encoder, and packed=False is that call
    kw = dict(max_new_tokens=8, eos_id=-1, return_logits=True)
    ids_d, _, lg_d = m.generate(tok, lengths=lengths, **kw)
    assert state(m).encoder_bias_bytes == 8 * 8 * 64 * 64 * 4
    ids_f, _, lg_f = m.generate(tok, lengths=lengths, packed=False, **kw)
    assert state(m).encoder_bias_bytes == 8 * 8 * 64 * 64 * 4 and torch.equal(ids_d, ids_f) and torch.equal(lg_d, lg_f)
    ids_p, _, lg_p = m.generate(tok, lengths=lengths, packed=True, **kw)
    assert state(m).encoder_bias_bytes == 0 and torch.isfinite(lg_p).all()
    assert max(rel(lg_p[b], lg_d[b].cpu()) for b in range(8)) <= 2e-2
    # packed=True without lengths is packed=False
    ids_a, _, lg_a = m.generate(tok, packed=True, **kw)
    ids_b, _, lg_b = m.generate(tok, **kw)
    assert torch.equal(ids_a, ids_b) and torch.equal(lg_a, lg_b)
    # a source of length 0 keeps working on the packed route (its row attends to nothing)
    zl = [0] + list(lengths[1:])
    ids_z, _, lg_z = m.generate(tok, lengths=zl, packed=True, **kw)
    assert state(m).encoder_bias_bytes == 0 and torch.isfinite(lg_z).all()
    assert max(rel(lg_z[b], lg_p[b].cpu()) for b in range(1, 8)) <= 2e-2


def test_refusals():
    from pytorch_models.text import T5Model
    from pytorch_models.transformer import MHA
    from pytorch_models._hip import ops
    from synthweights import fill_module

    m, _ = gpu_model("inner_ne_d")
    tok = synth_tokens("t5_varlen_tok", (3, S), 1000, 101)
    tgt = synth_tokens("t5_varlen_tgt", (3, 7), 1000, 102)
    lens = [S, 5, 1]
    m32 = T5Model(2000, 512, 6, 2, 1024).eval()
    fill_module(m32, 94)
    with pytest.raises(RuntimeError, match="HIP devices only"):  # a CPU module: what T5 raises today
        m32.encode(tok, lens)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        m32(tok, tgt, src_lengths=lens)
    m32 = m32.cuda()
    for call in (lambda: m32.encode(tok.cuda(), lens), lambda: m32(tok.cuda(), tgt.cuda(), src_lengths=lens),
                 lambda: m32.score(tok.cuda(), tgt.cuda(), src_lengths=lens),
                 lambda: m32.generate(tok.cuda(), lengths=lens, packed=True)):
        with pytest.raises(NotImplementedError, match="bf16 parameters only"):
            call()
    with pytest.raises(RuntimeError):  # a CPU input against a GPU module
        m.encode(tok, lens)
    for bad in ([S + 1, 5, 1], [-1, 5, 1], [S, 5], [S, 5, 1, 1], [float(S), 5, 1]):
        with pytest.raises(ValueError):
            m.encode(tok.cuda(), bad)
    for bad in ([S, 0, 1], [S + 1, 5, 1], [S, 5]):  # a row without a source token has no key for the cross-attention
        with pytest.raises(ValueError):
            m(tok.cuda(), tgt.cuda(), src_lengths=bad)
        with pytest.raises(ValueError):
            m.score(tok.cuda(), tgt.cuda(), src_lengths=bad)
    # head dims other than 64
    att = MHA(128, n_heads=4, head_dim=32, bias=False).to(torch.bfloat16).cuda()
    seq = ops.seq_lens([3, 2], 3, "cuda")
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        att.attend_packed(torch.zeros(5, 128, dtype=torch.bfloat16, device="cuda"), seq, rel_lut=torch.zeros(4, 3, device="cuda"), radius=1)
    with pytest.raises(NotImplementedError, match="encoder blocks only"):
        m.decoder.layers[0].forward_packed(torch.zeros(5, 512, dtype=torch.bfloat16, device="cuda"), seq, torch.zeros(6, 3, device="cuda"), 1)
