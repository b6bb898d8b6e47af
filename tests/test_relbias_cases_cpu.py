"""CPU: the packed attention with a relative-position bias by distance, without a GPU.
  (a) every assertion tests/test_hip_relbias_kernels.py makes about pm_attention_varlen_relbias_bf16 is satisfiable: the bf16
      kernels' arithmetic, emulated per sequence with the bias gathered from the table, stays within 1.0 x bf16_bound of the
      float64 reference on every case of tests/relbias_cases.py (the GPU test asserts 1.5 x);
  (b) RelativePositionBias.lut, gathered to (H, L, L), is RelativePositionBias.forward bit for bit, both directions;
  (c) the table follows a rewrite of the parameter;
  and the new entry point validates on the host (PM_EINVAL / PM_EALIGN, nothing launched)."""
import ctypes

import pytest
import torch

import relbias_cases as RC

torch.set_grad_enabled(False)
EINVAL, EALIGN = 1, 4


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_emulated_kernel_stays_within_the_bound(case):
    want, A = RC.reference(case)
    got = RC.emulate(case)
    assert got.shape == want.shape == (case.total, case.H * 64)
    ratio = RC.bound_ratio(got, want, A)
    print(f"RATIO emulated relbias {case.id} {ratio:.3f}")
    assert ratio <= 1.0
    if case.table == "dead":
        assert (want == 0).all() and (got == 0).all()


def test_cases_cover_the_radii_and_the_tables():
    ids = [c.id for c in RC.CASES]
    assert len(set(ids)) == len(ids)
    assert {c.R for c in RC.CASES} == {0, 5, 128}
    assert {c.table for c in RC.CASES} == {"t5", "distinct", "window", "dead"}
    assert {c.lengths for c in RC.CASES} == set(RC.LENGTH_SETS) and {c.H for c in RC.CASES} == set(RC.HEADS)
    assert all(c.causal for c in RC.DEAD_CASES)
    assert any(c.family == "planted" for c in RC.CASES)
    for table in ("t5", "distinct", "window"):
        assert {c.causal for c in RC.CASES if c.table == table} == {False, True}
    for c in RC.CASES:
        lut = RC.table(c)
        assert lut.shape == (c.H, 2 * c.R + 1) and lut.dtype == torch.float32
    c = next(c for c in RC.CASES if c.table == "distinct" and c.R == 5)
    assert RC.table(c).unique().numel() == c.H * 11  # every entry a different draw
    # the gather: [h, q, k] = lut[h, clamp(k - q)]
    d = RC.dense(RC.table(c), 9, 5)
    assert d[1, 2, 4] == RC.table(c)[1, 7] and d[1, 8, 0] == RC.table(c)[1, 0] and d[0, 0, 8] == RC.table(c)[0, 10]


def _rp(H=3, seed=5, **kw):
    from pytorch_models.text.t5 import RelativePositionBias

    rp = RelativePositionBias(H, **kw)
    rp.bias.copy_(2.0 * torch.randn(H, rp.n_buckets, generator=torch.Generator().manual_seed(seed)))
    return rp


@pytest.mark.parametrize("bidirection", [True, False], ids=["two-sided", "one-sided"])
@pytest.mark.parametrize("L", [1, 2, 129, 300, 600])
def test_lut_gathered_is_the_dense_table_bit_for_bit(L, bidirection):
    rp = _rp()
    lut = rp.lut(bidirection)
    R = rp.max_distance
    assert lut.shape == (3, 2 * R + 1) and lut.dtype == torch.float32 and lut.is_contiguous()
    got, want = RC.dense(lut, L, R), rp(L, bidirection).float()
    assert got.shape == want.shape == (3, L, L)
    if bidirection:
        assert torch.equal(got, want)
    else:  # above the diagonal the causal mask hides the value; the table still holds what the dense one holds: bucket 0
        keep = torch.ones(L, L, dtype=torch.bool).tril()
        assert torch.equal(got[:, keep], want[:, keep])
        assert torch.equal(lut[:, R + 1 :], rp.bias[:, :1].float().expand(3, R))


def test_lut_other_geometry():
    rp = _rp(H=2, seed=6, n_buckets=16, max_distance=20)
    assert rp.lut(True).shape == (2, 41)
    assert torch.equal(RC.dense(rp.lut(True), 50, 20), rp(50, True).float())


def test_lut_follows_the_parameter():
    rp = _rp()
    a = rp.lut(True)
    assert rp.lut(True) is a  # cached
    rp.bias.mul_(-0.5)
    b = rp.lut(True)
    assert not torch.equal(a, b) and torch.equal(RC.dense(b, 140, 128), rp(140, True).float())
    rp.bias.data = torch.ones_like(rp.bias)  # a new storage
    assert (rp.lut(True) == 1).all() and (rp.lut(False) == 1).all()
    rp = rp.to(torch.bfloat16)
    assert rp.lut(True).dtype == torch.float32


def test_host_side_validation_launches_nothing():
    """Rejected calls return before any HIP call, so this runs without a GPU (tests/test_abi.py style)."""
    from pytorch_models import _hip

    L = _hip.lib()
    raw = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(raw) // 16 * 16 + 16
    att = L.pm_attention_varlen_relbias_bf16
    ok = dict(q=p, qs=384, k=p + 256, ks=384, v=p + 512, vs=384, o=p, os=128, cu=p, B=2, H=2, max_len=40, causal=0, lut=p, ls=257, R=128)

    def call(**kw):
        a = {**ok, **kw}
        return att(a["q"], a["qs"], a["k"], a["ks"], a["v"], a["vs"], a["o"], a["os"], a["cu"], a["B"], a["H"], a["max_len"], a["causal"],
                   a["lut"], a["ls"], a["R"], None)

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(cu=None), dict(lut=None), dict(B=-1), dict(H=0),
               dict(max_len=0), dict(qs=64), dict(os=64), dict(R=-1), dict(ls=256), dict(R=513, ls=2000), dict(R=1 << 40, ls=1 << 42)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(qs=388), dict(os=130), dict(q=p + 8), dict(o=p + 4), dict(cu=p + 2), dict(lut=p + 2), dict(lut=p + 1)):
        assert call(**kw) == EALIGN, kw
    assert call(B=0) == 0 and call(B=0, R=512, ls=1025) == 0 and call(B=0, R=0, ls=1) == 0  # nothing to do, nothing launched
