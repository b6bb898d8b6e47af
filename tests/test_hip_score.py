"""GPU: the ``score`` methods of GPT2, GPT, Whisper and T5 on tiny synthetic models (V ~ 1000, d = 128, 2 layers; tests/score_cases.py).
  * score against float64 log_softmax(forward(...)) + gather from the SAME model.  forward and score share their hidden rows
    (``hidden_rows``), so the tolerance is the kernel bound evaluated on those rows plus forward's own accumulation term
    (score_cases.model_reference), asserted at MARGIN = 1.5;
  * a ``lengths`` row equals the row scored alone, bit for bit; ignored positions are exactly 0;
  * return_argmax equals forward's arg-max under the arg-max rule;
  * fp32 parameters raise NotImplementedError;
  * peak device memory of one GPT2.score call at B = 8, L = 64 with the real V = 50257 stays below the size of the logits matrix
    the call never builds (8 x 64 x 50257 x 4 = 103 MB).
Each test prints the figure it asserts."""
import pytest
import torch

import score_cases as sc
from synthweights import synth_input, synth_tokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B, L = 3, 9
LENGTHS = [9, 5, 1]


class _Model:
    """One model family behind one face: forward logits, hidden rows, score - all from decoder input ids (B, L)."""

    def __init__(self, name: str):
        self.name = name
        build = {"gpt2": sc.small_gpt2, "gpt": sc.small_gpt, "whisper": sc.small_whisper, "t5": sc.small_t5}[name]
        self.cpu_model = build()
        self.m = build().to(torch.bfloat16).cuda()
        self.V = {"gpt2": 1000, "gpt": 1003, "whisper": 1000, "t5": 1001}[name]
        self.tokens = synth_tokens("score_" + name, (B, L), self.V, 21).cuda()
        self.mel = synth_input("score_mel", (B, 80, 100), 21).cuda() if name == "whisper" else None
        self.src = synth_tokens("score_src", (B, 6), self.V, 22).cuda() if name == "t5" else None

    def _rows(self, sel):
        return (None if self.mel is None else self.mel[sel]), (None if self.src is None else self.src[sel])

    def logits(self):
        if self.name == "whisper":
            return self.m(self.mel, self.tokens)
        if self.name == "t5":
            return self.m(self.src, self.tokens)
        return self.m(self.tokens)

    def hidden(self):
        if self.name == "whisper":
            return self.m.decoder.hidden_rows(self.tokens, self.m.encoder(self.mel))
        if self.name == "t5":
            return self.m.hidden_rows(self.tokens, self.m.encode(self.src))
        return self.m.hidden_rows(self.tokens)

    def score(self, tokens=None, lengths=None, sel=slice(None), model=None, **kw):
        m = self.m if model is None else model
        tokens = self.tokens if tokens is None else tokens
        mel, src = self._rows(sel)
        if self.name == "whisper":
            return m.score(mel, tokens, lengths, **kw)
        if self.name == "t5":
            return m.score(src, tokens, lengths, **kw)
        return m.score(tokens, lengths, **kw)


_MODELS = {}


def _model(name) -> _Model:
    if name not in _MODELS:
        _MODELS[name] = _Model(name)
    return _MODELS[name]


NAMES = ("gpt2", "gpt", "whisper", "t5")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ragged", (False, True), ids=("full", "lengths"))
def test_score_is_log_softmax_of_forward(name, ragged):
    mod = _model(name)
    lengths = LENGTHS if ragged else None
    logits = mod.logits()
    h, W = mod.hidden()
    assert h.dtype == torch.bfloat16 and h.shape[:2] == (B, L) and W.shape[0] == mod.V == logits.shape[-1]
    want, bound, ref, tgt = sc.model_reference(logits, h, W, mod.tokens.cpu(), lengths)
    got, am = mod.score(lengths=lengths, return_argmax=True)
    assert got.shape == (B, L - 1) and got.dtype == torch.float32 and am.shape == (B, L - 1) and am.dtype == torch.int64
    r = sc.ratio(got.cpu(), want, bound)
    print(f"RATIO {name} {'lengths' if ragged else 'full'}: score vs fp64 log_softmax(forward) {r:.3f} of the bound (asserted <= {sc.MARGIN})")
    assert r <= sc.MARGIN
    assert torch.equal(mod.score(lengths=lengths), got)  # with and without the arg-max: the same bits
    if ragged:
        keep = torch.arange(1, L)[None, :] < torch.tensor(LENGTHS)[:, None]
        assert bool((got.cpu()[~keep] == 0).all()) and bool((got.cpu()[keep] < 0).all())
    # the arg-max rule, for score's predictions and forward's own
    fam = logits[:, :-1].argmax(-1).reshape(-1).cpu()
    assert sc.argmax_ok(ref, am.reshape(-1)) and sc.argmax_ok(ref, fam)
    ex = sc.exact_rows(ref)
    assert torch.equal(am.reshape(-1).cpu()[ex], fam[ex])
    print(f"RATIO {name}: {int(ex.sum())} of {ex.numel()} positions under the exact arg-max rule")


@pytest.mark.parametrize("name", NAMES)
def test_a_lengths_row_equals_the_row_scored_alone(name):
    mod = _model(name)
    got = mod.score(lengths=LENGTHS)
    for b, n in enumerate(LENGTHS):
        alone = mod.score(mod.tokens[b:b + 1], [n], slice(b, b + 1))
        assert torch.equal(alone.view(torch.int32), got[b:b + 1].view(torch.int32)), f"{name}: row {b} depends on its batch"
        assert bool((got[b, max(n - 1, 0):] == 0).all())
        if n >= 2:  # and the row cut to its own length, without lengths
            cut = mod.score(mod.tokens[b:b + 1, :n].contiguous(), None, slice(b, b + 1))
            assert torch.equal(cut.view(torch.int32), got[b:b + 1, :n - 1].view(torch.int32)), f"{name}: row {b} depends on the padding"


@pytest.mark.parametrize("name", NAMES)
def test_fp32_parameters_are_refused(name):
    mod = _model(name)
    m32 = mod.cpu_model.float().cuda()
    with pytest.raises(NotImplementedError):
        mod.score(model=m32)


def test_lengths_are_validated():
    mod = _model("gpt2")
    for bad in ([9, 5], [9, 5, 0], [9, 5, 10]):
        with pytest.raises(ValueError):
            mod.score(lengths=bad)
    with pytest.raises(ValueError):
        mod.score(mod.tokens[0])


def test_peak_memory_stays_below_the_logits_matrix():
    from pytorch_models.text import GPT2
    from synthweights import bf16_round_, fill_module

    m = GPT2(2, 128).eval()  # the real vocabulary: 50257
    fill_module(m, 9)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    tokens = synth_tokens("score_peak", (8, 64), GPT2.vocab_size, 9).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.score(tokens)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    logits_bytes = 8 * 64 * GPT2.vocab_size * 4
    print(f"RATIO GPT2.score B=8 L=64 V=50257: peak {peak / 1e6:.1f} MB above the model, the logits matrix would be {logits_bytes / 1e6:.1f} MB")
    assert out.shape == (8, 63) and bool(torch.isfinite(out).all()) and bool((out < 0).all())
    assert peak < logits_bytes
