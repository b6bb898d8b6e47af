"""Without a GPU: the reference of the prompt-pass attention kernel is pinned (chunk after chunk it IS full causal attention, and a
correct bf16 kernel meets the bound the GPU file asserts on every case), pm_prefill_attention_bf16 is declared, exported and
refuses every invalid argument form before any HIP call, and the decoders refuse prefill=True where it does not run."""
import ctypes

import pytest
import torch

import attn_cases as AC
import prefill_cases as PC
from pytorch_models import _hip

torch.set_grad_enabled(False)
PM_EINVAL = 1


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_chunked_reference_is_full_causal_attention(case):
    """The whole sequence 0 .. p0 + C - 1 in consecutive chunks of at most C positions (the last one is the case's own chunk, at
    the case's own p0), each appending to the caches of the ones before: float64-equal to one causal attention."""
    inp = PC.build(case)
    p0, C = case.p0, case.C
    k_all = torch.cat([inp["k_old"], AC.split_heads(inp["k"], PC.H)], 2)
    v_all = torch.cat([inp["v_old"], AC.split_heads(inp["v"], PC.H)], 2)
    q_old = AC.bf16r(torch.randn(PC.B, PC.H, p0, 64, generator=torch.Generator().manual_seed(p0 + C)))
    q_all = torch.cat([q_old, AC.split_heads(inp["q"], PC.H)], 2)
    full, A_full, _ = AC.ref_attention(q_all, k_all, v_all, causal=True)
    kc, vc = k_all[:, :, :0], v_all[:, :, :0]
    outs, As = [], []
    edges = list(range(0, p0, C)) + [p0, p0 + C]
    for a, b in zip(edges[:-1], edges[1:]):
        want, A, kc, vc = PC.ref_prefill(AC.merge_heads(q_all[:, :, a:b]), AC.merge_heads(k_all[:, :, a:b]),
                                         AC.merge_heads(v_all[:, :, a:b]), kc, vc)
        outs.append(want)
        As.append(A)
    assert torch.equal(kc, k_all) and torch.equal(vc, v_all)
    torch.testing.assert_close(torch.cat(outs, 1), AC.merge_heads(full), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(torch.cat(As, 1), AC.merge_heads(A_full), rtol=1e-12, atol=1e-12)
    # the case's own launch is the last chunk
    want, A = PC.reference(case, inp)
    assert torch.equal(want, outs[-1]) and torch.equal(A, As[-1])


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_a_correct_bf16_kernel_meets_the_bound_and_a_leak_by_one_does_not(case):
    """attn_cases.emulate_bf16_kernel (the kernels' arithmetic on the CPU) under the absolute-position mask stays inside
    1.5 x the bound; on the planted family the same arithmetic with the mask moved by one position, either way, does not."""
    inp = PC.build(case)
    want, A = PC.reference(case, inp)
    p0, C = case.p0, case.C
    qh = AC.split_heads(inp["q"], PC.H)
    kh = torch.cat([inp["k_old"], AC.split_heads(inp["k"], PC.H)], 2)
    vh = torch.cat([inp["v_old"], AC.split_heads(inp["v"], PC.H)], 2)

    def run(shift):
        keep = torch.arange(p0 + C)[None, :] <= (p0 + torch.arange(C))[:, None] + shift
        keep[:, 0] = True
        bias = torch.zeros(1, 1, C, p0 + C).masked_fill(~keep[None, None], AC.NEG_INF)
        return AC.merge_heads(AC.emulate_bf16_kernel(qh, kh, vh, bias))

    assert AC.bound_ratio(run(0), want, A) <= 1.5
    if case.family == "planted" and C >= 4:
        assert AC.bound_ratio(run(1), want, A) > 50 and AC.bound_ratio(run(-1), want, A) > 50


def test_case_list_covers_what_the_kernel_can_get_wrong():
    chunks = {(c.p0, c.C) for c in PC.CASES}
    assert chunks == set(PC.CHUNKS) and {c.family for c in PC.CASES} == {"scale", "planted"}
    assert any(c.lk_max == c.p0 + c.C for c in PC.CASES) and any(c.lk_max > c.p0 + c.C for c in PC.CASES)
    assert any(c.p0 % 64 and c.p0 > 64 for c in PC.CASES) and any(c.C > 128 for c in PC.CASES) and (0, 1) in chunks
    for c in PC.CASES:
        if c.family == "planted" and c.C >= 4:
            keys = [PC.planted_key(c, i) for i in range(c.C)]
            assert any(k == c.p0 + i + 1 for i, k in enumerate(keys)) and any(k == c.p0 + i for i, k in enumerate(keys))
    sc = PC.build(PC.PCase(0, 130, "scale", 30.0))
    s = (AC.split_heads(sc["q"], PC.H) @ AC.split_heads(sc["k"], PC.H).transpose(-1, -2)) / 8
    assert 100 < float(s.abs().max()) < 300  # scores up to |s| ~ 200


def test_prefill_attention_is_declared_bound_and_exported():
    assert "pm_prefill_attention_bf16" in _hip.header_functions()
    assert "pm_prefill_attention_bf16" in _hip.SIGNATURES
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "pm_prefill_attention_bf16")


def test_prefill_attention_host_side_validation_launches_nothing():
    """Every refusal is PM_EINVAL and comes before any HIP call, so this is safe without a GPU."""
    fn = _hip.lib().pm_prefill_attention_bf16
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    Hh, C, p0, T = 3, 4, 2, 8
    ld = 3 * Hh * 64
    good = dict(qkv=p, ld_qkv=ld, kc=p, vc=p, sb=Hh * T * 64, sh=T * 64, sk=64, out=p, ld_out=Hh * 64, B=2, H=Hh, C=C, p0=p0, lk_max=T)

    def call(**kw):
        a = {**good, **kw}
        return fn(a["qkv"], a["ld_qkv"], a["kc"], a["vc"], a["sb"], a["sh"], a["sk"], a["out"], a["ld_out"], a["B"], a["H"], a["C"],
                  a["p0"], a["lk_max"], None)

    bad = [dict(qkv=None), dict(kc=None), dict(vc=None), dict(out=None),          # null pointers
           dict(C=0), dict(C=-1), dict(p0=-1), dict(p0=T - C + 1), dict(C=T - p0 + 1),  # C < 1, p0 < 0, p0 + C > lk_max
           dict(lk_max=4097, p0=4000), dict(lk_max=4097),                         # lk_max > 4096
           dict(ld_qkv=ld - 8), dict(ld_qkv=0), dict(ld_out=Hh * 64 - 4), dict(H=0),   # rows too narrow for the heads
           dict(ld_qkv=ld + 4), dict(sb=Hh * T * 64 + 4), dict(sh=T * 64 + 2), dict(sk=68), dict(sk=32), dict(ld_out=Hh * 64 + 2),
           dict(qkv=p + 8), dict(kc=p + 2), dict(vc=p + 8), dict(out=p + 4)]       # strides and pointers off the vector alignment
    for kw in bad:
        assert call(**kw) == PM_EINVAL, kw
    assert call(B=0) == 0  # an empty batch is no error and launches nothing


def _cpu_gpt2():
    from pytorch_models.text import GPT2

    return GPT2(1, 64).eval()


@pytest.mark.parametrize("kw,match", [(dict(path="persistent"), "persistent"), (dict(kv32=True), "kv32"), (dict(), "bf16 parameters")])
def test_decoders_refuse_prefill_where_it_does_not_run(kw, match):
    """persistent path, fp32 caches, fp32 parameters: NotImplementedError naming the alternative - raised before anything touches
    a device, so a CPU-constructed model shows it.  (The same requests with prefill=False fail later, for being on the CPU.)"""
    from pytorch_models.audio2text.generate import BeamDecoder, GreedyDecoder, beam_decode, greedy_decode

    m = _cpu_gpt2()
    if "path" in kw or "kv32" in kw:
        m = m.to(torch.bfloat16)
    prompt = torch.zeros(1, 4, dtype=torch.int64)
    for build in (lambda: GreedyDecoder(m, None, prompt, 2, prefill=True, **kw), lambda: greedy_decode(m, None, prompt, 2, prefill=True, **kw),
                  lambda: BeamDecoder(m, None, prompt, 2, 2, prefill=True, **kw), lambda: beam_decode(m, None, prompt, 2, beams=2, prefill=True, **kw)):
        with pytest.raises(NotImplementedError, match=match) as e:
            build()
        assert "prefill=False" in str(e.value)


def test_public_entry_points_take_prefill_and_refuse_it_on_fp32_parameters():
    import inspect

    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.generate import beam_decode, greedy_decode
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from pytorch_models.text import GPT2, DecoderGenerator

    for fn in (greedy_decode, beam_decode, WhisperDecoder.generate, Whisper.generate, GPT2.generate, DecoderGenerator.generate_ids,
               DecoderGenerator.generate):
        assert inspect.signature(fn).parameters["prefill"].default is False, fn
    for fn in (greedy_decode, beam_decode):
        assert inspect.signature(fn).parameters["prefill_chunk"].default is None
    with pytest.raises(NotImplementedError, match="prefill=False"):
        _cpu_gpt2().generate(torch.zeros(1, 4, dtype=torch.int64), 2, prefill=True)
    w = Whisper(100, 1, 64).eval()
    with pytest.raises(NotImplementedError, match="prefill=False"):
        w.decoder.generate(torch.zeros(1, 8, 64), torch.zeros(1, 4, dtype=torch.int64), 2, prefill=True)
    with pytest.raises(NotImplementedError, match="exact=True"):
        w.generate(torch.zeros(1, 80, 16), torch.zeros(1, 4, dtype=torch.int64), 2, prefill=True, exact=True)
