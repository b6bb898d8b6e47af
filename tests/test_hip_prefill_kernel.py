"""GPU: pm_prefill_attention_bf16 (csrc/prefill.hip) on every case of tests/prefill_cases.py, through ops.prefill_attention.
  * |got - want| <= 1.5 x u (A + |want|) per element against the float64 reference (bound_ratio <= 1.5: the derived bound of
    tests/attn_cases.py; no measured number enters it);
  * the appended cache rows are the chunk's k / v bit for bit;
  * every other cache element is bitwise unchanged.  Before the call the positions >= p0 are bf16 NaN (the chunk's own slots
    too: the kernel reads the chunk's keys from the qkv rows, never from the caches) and the positions < p0 hold the old keys;
    afterwards they are compared as integers, and ``out`` must be finite - which proves the mask; finite input could not;
  * at p0 = 0 the result agrees with ops.attention(q, k, v, H, causal=True) on the same rows within the same bound.
Each test prints the figure it asserts ("RATIO ..." lines, pytest -s)."""
import pytest
import torch

import attn_cases as AC
import prefill_cases as PC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_REF = {}


def _reference(case):
    """inputs and float64 reference of a case, computed once and shared (never modified)"""
    if case.id not in _REF:
        inp = PC.build(case)
        _REF[case.id] = (inp, *PC.reference(case, inp))
    return _REF[case.id]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(case, inp):
    """(out (B, C, H*64), kc, vc after the call, kc, vc before it, the qkv rows) - all on the device"""
    from pytorch_models._hip import ops

    B, H, p0, C, T = PC.B, PC.H, case.p0, case.C, case.lk_max
    inner = H * 64
    pad = 8 if p0 % 2 else 0  # odd p0: rows of a wider buffer (leading dimension 3 * H * 64 + 8), NaN in the padding
    buf = torch.full((B * C, 3 * inner + pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    qkv = buf[:, : 3 * inner]
    qkv.copy_(torch.cat([inp["q"], inp["k"], inp["v"]], -1).view(B * C, 3 * inner))
    kc = torch.full((B, H, T, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    vc = torch.full((B, H, T, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    kc[:, :, :p0] = inp["k_old"]
    vc[:, :, :p0] = inp["v_old"]
    kc0, vc0 = kc.clone(), vc.clone()
    out = ops.prefill_attention(qkv, kc, vc, H, p0)
    torch.cuda.synchronize()
    assert out.shape == (B * C, inner) and out.dtype == torch.bfloat16
    return out.view(B, C, inner), kc, vc, kc0, vc0, qkv


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_parity_append_and_untouched_caches(case):
    inp, want, A = _reference(case)
    B, H, p0, C = PC.B, PC.H, case.p0, case.C
    out, kc, vc, kc0, vc0, qkv = _launch(case, inp)
    got = out.float().cpu()
    assert torch.isfinite(got).all(), f"{case.id}: non-finite output: a NaN cache slot or padding was read into a live product"
    ratio = AC.bound_ratio(got, want, A)
    print(f"RATIO prefill {case.id} parity {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound"
    # appended rows: bit copies of the chunk's k / v
    inner = H * 64
    k_rows = qkv[:, inner : 2 * inner].reshape(B, C, H, 64).transpose(1, 2)
    v_rows = qkv[:, 2 * inner :].reshape(B, C, H, 64).transpose(1, 2)
    assert torch.equal(_bits(kc[:, :, p0 : p0 + C]), _bits(k_rows)) and torch.equal(_bits(vc[:, :, p0 : p0 + C]), _bits(v_rows))
    # everything else: bitwise as before (NaN payloads included)
    for now, before in ((kc, kc0), (vc, vc0)):
        assert torch.equal(_bits(now[:, :, :p0]), _bits(before[:, :, :p0])), f"{case.id}: an old cache row changed"
        assert torch.equal(_bits(now[:, :, p0 + C :]), _bits(before[:, :, p0 + C :])), f"{case.id}: a row behind the chunk was written"


@pytest.mark.parametrize("case", [c for c in PC.CASES if c.p0 == 0], ids=lambda c: c.id)
def test_first_chunk_agrees_with_the_top_left_causal_kernel(case):
    """At p0 = 0 absolute and top-left alignment coincide: the difference to pm_attention_bf16(causal) on the same rows stays
    inside the same 1.5 x u (A + |want|)."""
    from pytorch_models._hip import ops

    inp, want, A = _reference(case)
    out, *_ = _launch(case, inp)
    q, k, v = (inp[n].to(torch.bfloat16).cuda() for n in ("q", "k", "v"))
    other = ops.attention(q, k, v, PC.H, causal=True).float().cpu()
    got = out.float().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(other).all()
    err = (got.double() - other.double()).abs()
    bnd = AC.bf16_bound(want, A)
    assert (err[bnd == 0] == 0).all()
    ratio = float((err[bnd > 0] / bnd[bnd > 0]).max())
    print(f"RATIO prefill {case.id} vs-causal {ratio:.3f}")
    assert ratio <= 1.5, f"{case.id}: {ratio:.3f} x bf16_bound between the two kernels"
