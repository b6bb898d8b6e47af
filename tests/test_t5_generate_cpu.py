"""CPU: what the T5 generation tests stand on.  The oracle's greedy loop and full model (oracle/ref_t5.py) against the
reference's own run (tests/golden/t5_generate.npz, made by tests/golden/make_golden_t5_generate.py), the decode step's
relative-position table by distance against the (heads, L, L) table of the full-sequence path, the non-vacuity of the GPU
tests' arg-max rule on the oracle alone, and the host-side refusals of T5Model.generate that need no device."""
import pytest
import torch

import t5_generate_cases as TC
from oracle import ref_t5 as R5

torch.set_grad_enabled(False)


def test_oracle_reproduces_the_reference_loop(golden):
    g = golden("t5_generate")
    case = g["meta"]["case"]
    assert tuple(g["meta"]["geometry"]) == TC.CASES[case][0] and g["meta"]["seed"] == TC.CASES[case][1]
    _, sd = TC.build(case, rounded=False)  # the reference ran on the unrounded fp32 weights
    tok, lengths, n = TC.sources(case)
    assert lengths == g["meta"]["lengths"] and n == g["meta"]["decisions"]
    for b, ln in enumerate(lengths):
        ids, margins = R5.greedy(sd, tok[b, :ln], n + 1, eos_id=-1)
        assert torch.equal(ids, g["ids"][b].long()), b
        # a margin is the difference of two logits that each agree at the defaults (1e-5 + 1.3e-6 |x|, |x| < 30): 2 * 5e-5
        torch.testing.assert_close(torch.tensor(margins), g["margins"][b], rtol=0, atol=1e-4)
        torch.testing.assert_close(R5.model(sd, tok[b, :ln], ids)[:, ::16], g["logits_s16"][b])


@pytest.mark.parametrize("L", [8, 64, 200])
def test_distance_table_equals_the_full_bias(L):
    """lut[h, dist] == RelativePositionBias.forward(L, False)[h, L - 1, L - 1 - dist], including the range clipped beyond
    max_distance = 128 (L = 200); every causal entry (t, j) of the full table is lut[h, t - j]."""
    from pytorch_models.text.t5 import RelativePositionBias
    from pytorch_models.text.t5_generate import distance_lut

    rp = RelativePositionBias(6)
    rp.bias.copy_(torch.randn(6, 32, generator=torch.Generator().manual_seed(L)))
    lut = distance_lut(rp, L)
    full = rp(L, False)
    assert lut.shape == (6, L) and lut.dtype == torch.float32
    for dist in range(L):
        assert torch.equal(lut[:, dist], full[:, L - 1, L - 1 - dist]), dist
    t, j = torch.tril_indices(L, L)
    assert torch.equal(full[:, t, j], lut[:, t - j])
    if L > 129:
        assert torch.equal(lut[:, 128:], lut[:, 128:129].expand(-1, L - 128))  # clipped: one bucket from max_distance on


def test_arg_max_rule_is_not_vacuous():
    """Over the GPU test's teacher-forced cases at least half of all decisions have an oracle top-2 margin >= 0.05 - a
    condition on the oracle alone: an arg-max rule that exempted most decisions would check nothing."""
    decided = total = 0
    for case in TC.TEACHER_FORCED:
        m = TC.oracle(case)["margins"]
        print(case, "decided", int((m >= TC.MARGIN).sum()), "of", m.numel())
        decided += int((m >= TC.MARGIN).sum())
        total += m.numel()
    assert 2 * decided >= total, (decided, total)


def test_generate_refuses_what_needs_no_device_to_refuse():
    from pytorch_models.text import T5Model

    m = T5Model(100, 64, 1, 1, 64)
    assert callable(m.generate)
    with pytest.raises(RuntimeError, match="HIP devices only"):  # a CPU model, whatever its dtype
        m.generate(torch.zeros(1, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        m.to(torch.bfloat16).generate(torch.zeros(1, 4, dtype=torch.int64))
