"""GPU: Whisper.align / WhisperDecoder.align on bf16 models (2 layers d = 128 and 4 layers d = 256, synthetic weights, three
clips ragged in tokens and frames):
  * m against the alignment reference (tests/align_cases.py, float64) run on the fp32 oracle's q / k: rel-L2 within
    E2E_BOUND = 2 x the worst figure of tools/align_tolerance.py (the oracle with bf16 rounding at the HIP path's storage points);
  * start equals the float32 DTW loop run on the DEVICE's own m, exactly; agreement with the oracle's own path is printed, not
    asserted (bf16 can legitimately move a path);
  * each clip alone reproduces its batch row bit for bit; an explicit heads= subset and the default; Whisper.align ==
    decoder.align(encoder(mel)); forward() logits bit-identical before and after an align() call."""
import pytest
import torch

import align_cases as ac

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_CACHE = {}


def _setup(name):
    """(bf16 device model, state dict, mel, tokens, lens, frs, the oracle's fp32 memory), built once per geometry"""
    if name not in _CACHE:
        from oracle import ref_whisper

        w, sd, mel, tokens, lens, frs = ac.model_inputs(name)
        memory = ref_whisper.encoder(sd, "encoder.", mel)
        _CACHE[name] = (w.to(torch.bfloat16).cuda(), sd, mel, tokens, lens, frs, memory)
    return _CACHE[name]


@pytest.mark.parametrize("name", [c[0] for c in ac.MODEL_CASES])
def test_matrix_against_the_oracle_and_start_against_the_device_matrix(name):
    from pytorch_models.audio2text.align import default_heads

    w, sd, mel, tokens, lens, frs, memory = _setup(name)
    n_layers, H = len(w.decoder.layers), w.decoder.layers[0].sa.n_heads
    for heads in (None, [(n_layers - 1, H - 1), (0, 0), (n_layers - 1, 0)]):
        start, m = w.align(mel.cuda(), tokens.cuda(), lengths=lens, frames=frs, heads=heads, skip_first=1, skip_last=1, return_matrix=True)
        assert start.dtype == torch.int32 and start.shape == tokens.shape and m.dtype == torch.float32
        start, m = start.cpu(), m.cpu()
        hs = default_heads(n_layers, H) if heads is None else heads
        want = ac.oracle_matrix(sd, tokens, memory, hs, lens, frs)
        err = ac.rel_l2(m, want)
        oracle_start = ac.dtw_start(want.float(), lens, frs, 1, 1)
        print(f"RATIO {name} heads {'default' if heads is None else heads}: rel-L2 of m {err:.4e} (asserted <= {ac.E2E_BOUND[name]:.4e}); "
              f"start agrees with the oracle's path in {int(((start == oracle_start) & (start >= 0)).sum())} of {int((start >= 0).sum())} rows")
        assert err <= ac.E2E_BOUND[name]
        for b in range(3):
            assert bool((m[b, lens[b]:] == 0).all()) and bool((m[b, :, frs[b]:] == 0).all())
        assert torch.equal(start, ac.dtw_start(m, lens, frs, 1, 1))


@pytest.mark.parametrize("name", [c[0] for c in ac.MODEL_CASES])
def test_each_clip_alone_reproduces_its_batch_row(name):
    w, sd, mel, tokens, lens, frs, _ = _setup(name)
    memory = w.encoder(mel.cuda())
    start, m = w.decoder.align(tokens.cuda(), memory, lengths=lens, frames=frs, skip_first=2, skip_last=1, return_matrix=True)
    s2, m2 = w.align(mel.cuda(), tokens.cuda(), lengths=lens, frames=frs, skip_first=2, skip_last=1, return_matrix=True)
    assert torch.equal(start, s2) and torch.equal(m.view(torch.int32), m2.view(torch.int32))  # Whisper.align == decoder.align(encoder(mel))
    for b in range(3):
        s1, m1 = w.decoder.align(tokens[b:b + 1].cuda(), memory[b:b + 1], lengths=[lens[b]], frames=frs[b], skip_first=2, skip_last=1,
                                 return_matrix=True)
        assert torch.equal(m1[0].view(torch.int32), m[b].view(torch.int32)), f"clip {b}: m depends on the batch"
        assert torch.equal(s1[0], start[b]), f"clip {b}: start depends on the batch"
    assert torch.equal(w.decoder.align(tokens.cuda(), memory), w.decoder.align(tokens.cuda(), memory, lengths=20, frames=memory.shape[1]))


def test_forward_is_bit_identical_around_an_align_call():
    w, sd, mel, tokens, lens, frs, _ = _setup("w2x128")
    before = w(mel.cuda(), tokens.cuda())
    w.align(mel.cuda(), tokens.cuda(), lengths=lens, frames=frs)
    after = w(mel.cuda(), tokens.cuda())
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))


def test_fp32_parameters_are_refused():
    w, sd, mel, tokens, lens, frs, _ = _setup("w2x128")
    w32, _ = ac.small_whisper()
    w32 = w32.cuda()
    with pytest.raises(NotImplementedError, match="bf16 weights on a HIP device only"):
        w32.decoder.align(tokens.cuda(), w.encoder(mel.cuda()))
    with pytest.raises(ValueError):
        w.decoder.align(tokens.cuda(), w.encoder(mel.cuda()), frames=[3, 250, 250])
