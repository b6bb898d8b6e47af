"""Without a GPU: the reference of the ragged-prompt kernels is pinned to the feature's definition ("row b of a ragged batch is that row
alone"), the case list covers every class of start, the end-to-end seeds of tests/test_hip_ragged.py are decisive on the CPU, the
six entry points are declared, bound and exported, and the decoders refuse a ragged batch where it does not run."""
import ctypes
import os

import pytest
import torch

import attn_cases as AC
import prefill_cases as PC
import ragged_cases as RC
from pytorch_models import _hip

torch.set_grad_enabled(False)
PM_EINVAL = 1
ENTRY_POINTS = ("pm_dec_attention_ragged", "pm_prefill_attention_ragged_bf16", "pm_embed_tokens_ragged", "pm_dec_embed_ragged",
                "pm_dec_next_token_ragged", "pm_dec_sample_topk_ragged")


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_ragged_prefill_reference_is_the_row_alone(case):
    """Row b at positions >= start_b equals prefill_cases.ref_prefill (the plain, trusted reference) of that row with its padding
    cut away, in float64 to 1e-12; padded queries return their own V row exactly."""
    inp = RC.build(case)
    want, A = RC.reference(case, inp)
    p0, C = case.p0, case.C
    valid = RC.valid_rows(p0, C, case.starts)
    checked = 0
    for b, st in enumerate(case.starts):
        row = slice(b, b + 1)
        if st < p0 + C:
            i0 = max(0, st - p0)  # the row's first valid chunk row
            old = slice(min(st, p0), p0)  # its unpadded old keys
            w1, A1, _, _ = PC.ref_prefill(inp["q"][row, i0:], inp["k"][row, i0:], inp["v"][row, i0:], inp["k_old"][row, :, old],
                                          inp["v_old"][row, :, old])
            torch.testing.assert_close(want[row, i0:], w1, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(A[row, i0:], A1, rtol=1e-12, atol=1e-12)
            assert bool(valid[b, i0:].all()) and not bool(valid[b, :i0].any())
            checked += C - i0
        pad = ~valid[b]
        assert torch.equal(want[b, pad], inp["v"][b, pad].double()) and torch.equal(A[b, pad], inp["v"][b, pad].double().abs())
    assert checked == int(valid.sum())


@pytest.mark.parametrize("case", RC.SCASES, ids=lambda c: c.id)
def test_ragged_step_reference_is_the_row_alone(case):
    inp = RC.build_step(case)
    want, A = RC.reference_step(case, inp)
    for b, lo in enumerate(RC.step_lo(case)):
        w1, A1, _ = AC.ref_attention(inp["q"][b].view(1, RC.H, 1, 64), inp["k"][b : b + 1, :, lo : case.Lk], inp["v"][b : b + 1, :, lo : case.Lk])
        torch.testing.assert_close(want[b], w1.reshape(-1), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(A[b], A1.reshape(-1), rtol=1e-12, atol=1e-12)
    assert RC.step_lo(case)[3] == case.Lk - 1  # the clamped start leaves the newest key


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_a_correct_bf16_kernel_meets_the_bound_and_a_mask_off_by_one_does_not(case):
    """attn_cases.emulate_bf16_kernel (the kernels' arithmetic on the CPU) under the keep-mask stays inside 1.5 x the bound; on
    the planted family the same arithmetic with the lower edge moved by one position, either way, does not."""
    inp = RC.build(case)
    want, A = RC.reference(case, inp)
    qh = AC.split_heads(inp["q"], RC.H)
    kh = torch.cat([inp["k_old"], AC.split_heads(inp["k"], RC.H)], 2)
    vh = torch.cat([inp["v_old"], AC.split_heads(inp["v"], RC.H)], 2)
    run = lambda shift: AC.merge_heads(AC.emulate_bf16_kernel(qh, kh, vh, RC._bias(case.p0, case.C, case.starts, shift).float()))  # noqa: E731
    assert AC.bound_ratio(run(0), want, A) <= 1.5
    if case.family == "planted" and any(0 < st < case.p0 + case.C for st in case.starts):  # a valid query with a key below its start
        assert AC.bound_ratio(run(-1), want, A) > 50
        if case.C >= 8:  # ... and one aimed at the start itself (chunk rows 4, 12, ...) with more keys above it
            assert AC.bound_ratio(run(1), want, A) > 50


# ------------------------------------------------------------------------------------------------ 2. coverage
def test_case_list_covers_every_class_of_start():
    assert {(c.p0, c.C) for c in RC.CASES} == {(0, 1), (0, 33), (0, 65), (0, 130), (63, 2), (64, 64), (200, 130)}
    assert {(c.family, c.scale) for c in RC.CASES} == {("scale", 1.0), ("scale", 30.0), ("planted", 1.0)}
    pairs = [(p0, C, st) for (p0, C), sts in RC.STARTS.items() for st in sts]
    assert all(len(sts) == RC.B for sts in RC.STARTS.values())
    assert any(st == 0 for _, _, st in pairs)
    assert any(p0 < st < p0 + C and st % 64 not in (0, 63) for p0, C, st in pairs)                   # inside the chunk, off a tile edge
    assert {63, 64, 65} <= {st for _, _, st in pairs}
    assert any(0 < st < p0 and st % 64 not in (0, 63) for p0, _, st in pairs)                          # inside the old keys, mid-tile
    assert any(st >= p0 + C for p0, C, st in pairs)                                                    # the whole chunk is padding
    # a query whose first visible key lies in a later key tile than another query's of the same 16-query wave
    assert any(p0 < st < p0 + C and st % 64 and (st - p0) // 16 == (st // 64 * 64 - 1 - p0) // 16 and st // 64 * 64 > p0 for p0, C, st in pairs)
    assert any(c.lk_max == c.p0 + c.C for c in RC.CASES) and any(c.lk_max > c.p0 + c.C for c in RC.CASES)
    for c in RC.CASES:
        if c.family == "planted":
            for b, st in enumerate(c.starts):
                keys = [RC.planted_key(c, b, i) for i in range(c.C) if c.p0 + i >= st]
                if len(keys) >= 8 and st >= 1:
                    assert st - 1 in keys and st in keys, (c.id, b)
            assert any(RC.planted_key(c, 0, i) == c.p0 + i + 1 for i in range(c.C)) or c.C < 4  # the existing targets stay
    assert {c.Lk for c in RC.SCASES} == {1, 5, 129, 300}
    for c in RC.SCASES:
        assert c.starts == (0, 3, c.Lk - 1, c.Lk + 2)


# ------------------------------------------------------------------------------------------------ 3. the end-to-end seeds
def _round_all(name, t):
    """every named rounding point of the oracle except the residual stream in bf16 (DESIGN.md section 18 pinned its seeds so)"""
    return t if name == "resid" else t.to(torch.bfloat16).float()


def test_end_to_end_seeds_are_decisive_under_every_rounding():
    """The all-rounded CPU loop reproduces the unrounded per-row oracle ids for EVERY row of the end-to-end runs, so the reference
    alone needs none of the near-tie exceptions the GPU tests allow.  Prints the smallest oracle margin."""
    from oracle import ref_text as RX
    from oracle import ref_whisper as RW
    from pytorch_models.audio2text import Whisper
    from pytorch_models.text import GPT2
    from synthweights import bf16_round_, fill_module, synth_input

    m = GPT2(2, 128)
    fill_module(m, RC.GPT2_SEED)
    bf16_round_(m)
    sd = m.state_dict()
    prompt = RC.gpt2_prompt()
    smallest = float("inf")
    for b, n in enumerate(RC.GPT2_LENGTHS):
        want, margins = RX.greedy(RX.gpt2, sd, prompt[b : b + 1, :n], RC.GPT2_NEW)
        got, _ = RX.greedy(RX.gpt2, sd, prompt[b : b + 1, :n], RC.GPT2_NEW, rp=_round_all)
        assert torch.equal(got, want), f"GPT-2 row {b}: the all-rounded loop leaves the oracle's ids"
        smallest = min(smallest, float(margins.min()))
    print(f"GPT-2 ragged seeds: smallest oracle margin {smallest:.3e}")
    assert smallest > 2e-4  # test_hip_decode.py's near-tie threshold is never in play

    w = Whisper.from_openai("tiny")
    fill_module(w, 55)
    bf16_round_(w)
    sd = w.state_dict()
    memory = synth_input("prefill_memory", (2, 96, 384), 55).to(torch.bfloat16).float()
    prompt = RC.whisper_prompt()
    smallest = float("inf")
    for b, n in enumerate(RC.WHISPER_LENGTHS):
        fwd = lambda sd_, toks, rp=None, b=b: RW.decoder(sd_, "decoder.", toks, memory[b : b + 1], rp=rp)  # noqa: E731
        want, margins = RX.greedy(fwd, sd, prompt[b : b + 1, :n], RC.WHISPER_NEW)
        got, _ = RX.greedy(fwd, sd, prompt[b : b + 1, :n], RC.WHISPER_NEW, rp=_round_all)
        assert torch.equal(got, want), f"Whisper row {b}: the all-rounded loop leaves the oracle's ids"
        smallest = min(smallest, float(margins.min()))
    print(f"Whisper ragged seeds: smallest oracle margin {smallest:.3e}")


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_ragged_entry_points_are_declared_bound_and_exported():
    """in the manner of tests/test_abi.py: the header declares the six entry points, the built library exports them, the ABI is 1"""
    assert os.path.exists(_hip.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    declared = _hip.header_functions()
    L = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/pm_mi355x.h"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(L, name), f"{name} is not exported"
    assert _hip.lib().pm_abi_version() == 1


def test_ragged_entry_points_refuse_a_null_key_start_before_any_launch():
    """PM_EINVAL for a null key_start (and the plain entry point's refusals stay), before any HIP call: safe without a GPU."""
    L = _hip.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    Hh, C, p0, T = 3, 4, 2, 8
    ld = 3 * Hh * 64
    good = [p, ld, p, p, Hh * T * 64, T * 64, 64, p, Hh * 64, 2, Hh, C, p0, T, p, None]
    fn = L.pm_prefill_attention_ragged_bf16
    for i, bad in ((14, None), (0, None), (2, None), (11, 0), (12, -1), (13, 4097), (1, ld + 4), (6, 68), (7, p + 4)):
        a = list(good)
        a[i] = bad
        assert fn(*a) == PM_EINVAL, (i, bad)
    a = list(good)
    a[9] = 0
    assert fn(*a) == 0  # an empty batch is no error and launches nothing
    assert L.pm_dec_attention_ragged(p, p, p, 64, 64, 64, None, 1, 8, None, p, 1, 1, None) == PM_EINVAL
    assert L.pm_embed_tokens_ragged(p, p, p, None, p, 1, 1, 1, 0, 64, 10, None) == PM_EINVAL
    assert L.pm_dec_embed_ragged(p, p, p, p, None, p, 1, 64, 10, None) == PM_EINVAL
    assert L.pm_dec_next_token_ragged(p, p, 1, p, p, 1, p, p, 2, None, p, p, None, p, 64, 10, p, 1, None) == PM_EINVAL
    assert L.pm_dec_sample_topk_ragged(p, 10, 10, 1, 0, p, p, 1, p, p, 2, p, p, None, p, 64, p, 1, None) == PM_EINVAL


# ------------------------------------------------------------------------------------------------ 5. refusals and arguments
def _cpu_gpt2():
    from pytorch_models.text import GPT2

    return GPT2(1, 64).eval()


@pytest.mark.parametrize("kw,match,names", [(dict(path="persistent"), "persistent", "path='launches'"), (dict(kv32=True), "kv32", "without lengths="),
                                            (dict(beams=2), "beam", "beams=1"), (dict(), "bf16 parameters", "greedy_exact")])
def test_decoders_refuse_a_ragged_batch_where_it_does_not_run(kw, match, names):
    """beams, the persistent path, fp32 caches, fp32 parameters: NotImplementedError naming the form that does run - raised before
    anything touches a device, so a CPU-constructed model shows it."""
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode

    m = _cpu_gpt2()
    if kw:
        m = m.to(torch.bfloat16)
    prompt = torch.zeros(2, 4, dtype=torch.int64)
    builds = [lambda: GreedyDecoder(m, None, prompt, 2, lengths=(4, 2), **kw)]
    if "beams" not in kw:
        builds.append(lambda: greedy_decode(m, None, prompt, 2, lengths=(4, 2), **kw))
    if "kv32" not in kw:
        builds.append(lambda: m.generate(prompt, 2, lengths=(4, 2), **kw))
    for build in builds:
        with pytest.raises(NotImplementedError, match=match) as e:
            build()
        assert names in str(e.value)


def test_whisper_entry_points_refuse_a_ragged_batch_with_exact_or_beams():
    from pytorch_models.audio2text import Whisper

    w = Whisper(100, 1, 64).eval().to(torch.bfloat16)
    prompt, mel, mem = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 80, 16), torch.zeros(2, 8, 64)
    with pytest.raises(NotImplementedError, match="exact=True"):
        w.generate(mel, prompt, 2, lengths=(4, 2), exact=True)
    with pytest.raises(NotImplementedError, match="beams=1"):
        w.generate(mel, prompt, 2, lengths=(4, 2), beams=2)
    with pytest.raises(NotImplementedError, match="beams=1"):
        w.decoder.generate(mem.to(torch.bfloat16), prompt, 2, lengths=(4, 2), return_beams=True)
    with pytest.raises(NotImplementedError, match="kv32"):
        w.decoder.generate(mem, prompt, 2, lengths=(4, 2))  # an fp32 memory is the fp32-cache step's
    with pytest.raises(NotImplementedError, match="bf16 parameters"):
        Whisper(100, 1, 64).eval().decoder.generate(mem.to(torch.bfloat16), prompt, 2, lengths=(4, 2))


@pytest.mark.parametrize("lengths", [(4,), (4, 2, 1), ((4, 2),), (4.0, 2.0), (0, 2), (4, 5), (-1, 2), torch.tensor([[4, 2]]), torch.tensor([4.0, 2.0])])
def test_bad_lengths_are_value_errors(lengths):
    from pytorch_models.audio2text.generate import greedy_decode

    m = _cpu_gpt2().to(torch.bfloat16)
    with pytest.raises(ValueError, match="length"):
        greedy_decode(m, None, torch.zeros(2, 4, dtype=torch.int64), 2, lengths=lengths)


def test_the_longest_prompt_bounds_the_positions_not_the_padded_width():
    from pytorch_models.audio2text.generate import greedy_decode

    m = _cpu_gpt2().to(torch.bfloat16)
    prompt = torch.zeros(2, 1000, dtype=torch.int64)
    with pytest.raises(ValueError, match="max_seq_len"):
        greedy_decode(m, None, prompt, 30, lengths=(1000, 3))  # 1030 > 1024
    with pytest.raises(NotImplementedError, match="HIP device"):  # 990 + 30 fits: the request gets as far as the device check
        greedy_decode(m, None, prompt, 30, lengths=(990, 3))
    with pytest.raises(ValueError, match="pad_token_id"):
        greedy_decode(m, None, prompt, 30, lengths=(990, 3), pad_token_id=50257)


def test_right_alignment_and_its_inverse():
    from pytorch_models.audio2text.generate import _ragged_lengths, _right_align

    prompt = torch.tensor([[5, 6, 7, 8], [9, 1, 2, 3], [4, 0, 0, 0]])
    lens = _ragged_lengths(prompt, torch.tensor([3, 2, 1], dtype=torch.int32))
    assert _right_align(prompt, lens, 3, 77).tolist() == [[5, 6, 7], [77, 9, 1], [77, 77, 4]]


def test_public_entry_points_take_lengths():
    import inspect

    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.generate import GreedyDecoder, greedy_decode
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from pytorch_models.text import GPT2, DecoderGenerator

    for fn in (greedy_decode, WhisperDecoder.generate, Whisper.generate, GPT2.generate, GreedyDecoder.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["lengths"].default is None and sig["pad_token_id"].default == 0, fn
    assert inspect.signature(GreedyDecoder.rebind).parameters["lengths"].default is None
    sig = inspect.signature(DecoderGenerator.generate_ids_batch).parameters
    assert [sig[n].default for n in ("max_tokens", "topk", "eos_token_id", "seed", "prefill")] == [100, 1, None, 0, False]
    assert "prompts" in inspect.signature(DecoderGenerator.generate_batch).parameters
