"""Keeps the kernel-level suite of csrc/decode_t5.hip (tests/test_hip_t5_decode.py) honest without a GPU: on every case it runs the
tolerance is satisfiable (the same formulas evaluated by torch in float32 meet it against the float64 reference), every named
mutant of the reference misses it by 10 x on the case built for it (a mutant no case catches means a case is missing), the needle
keys carry the mass they were planted for, the case lists reach every geometry the kernels branch on, and the two host-side
helpers of text/t5_generate.py (the distance table, the interleaved GEGLU weight) are what the kernels are documented to read."""
import os

import pytest
import torch

import t5_decode_cases as TD
from oracle import ref_t5 as R5

torch.set_grad_enabled(False)
MUTANT_MARGIN = 10.0


def _self_pair(c, **mut):
    """(float32 evaluation, float64 reference reading the SAME cached row t), as the GPU file pairs kernel and reference"""
    inp = TD.build_self(c)
    lo = TD.ref_self(c, inp, torch.float32)
    own = (TD.bf16r(lo["k_new"]), TD.bf16r(lo["v_new"]))
    return lo, TD.ref_self(c, inp, torch.float64, own=own), own


@pytest.mark.parametrize("c", TD.SELF_CASES, ids=lambda c: c.id)
def test_self_cases_tolerance_is_satisfiable(c):
    lo, hi, own = _self_pair(c)
    assert 0.4 < float(hi["att"].square().mean().sqrt()) < 2.5 and 0.4 < float(hi["q"].square().mean().sqrt()) < 2.5, "unit-rms outputs"
    f = dict(q=TD.used(lo["q"], hi["q"]), att=TD.used(lo["att"], hi["att"]), k_row=TD.row_ok(own[0], hi["k_new"]),
             v_row=TD.row_ok(own[1], hi["v_new"]))
    print(c.id, {k: round(v, 3) for k, v in f.items()})
    assert max(f.values()) <= 1.0, f
    p = hi["p"]
    for b, j in enumerate(c.needles):
        assert float(p[b, :, j].min()) > 0.5, "the planted key holds most of the mass in every head"
    if c.own:
        assert float(p[0, :, c.t].min()) > 0.5


@pytest.mark.parametrize("c", TD.CROSS_CASES, ids=lambda c: c.id)
def test_cross_cases_tolerance_is_satisfiable(c):
    inp = TD.build_cross(c)
    lo, hi = TD.ref_cross(c, inp, torch.float32), TD.ref_cross(c, inp)
    live = torch.tensor([c.keys(b) > 0 for b in range(c.B)])
    assert (hi["att"][~live] == 0).all() and 0.4 < float(hi["att"][live].square().mean().sqrt()) < 2.5
    f = TD.used(lo["att"], hi["att"])
    print(c.id, round(f, 3))
    assert f <= 1.0
    for b, j in enumerate(c.needles):
        assert float(hi["p"][b][:, j].min()) > 0.5


@pytest.mark.parametrize("c", TD.GEGLU_CASES, ids=lambda c: c.id)
def test_geglu_cases_tolerance_is_satisfiable(c):
    inp = TD.build_geglu(c)
    hi = TD.ref_geglu(c, inp)
    assert 0.4 < float(hi.square().mean().sqrt()) < 2.5
    f = TD.used(TD.ref_geglu(c, inp, torch.float32), hi)
    print(c.id, round(f, 3))
    assert f <= 1.0


def _mutate(family, cid, kw):
    if family == "self":
        c = TD.SELF[cid]
        inp = TD.build_self(c)
        want = TD.ref_self(c, inp)
        got = TD.ref_self(c, inp, own=(TD.bf16r(want["k_new"]), TD.bf16r(want["v_new"])), **kw)  # the row at t held fixed
        return torch.cat([got["q"], got["att"]], 1), torch.cat([want["q"], want["att"]], 1)  # both are asserted on the GPU
    if family == "cross":
        c = TD.CROSS[cid]
        inp = TD.build_cross(c)
        return TD.ref_cross(c, inp, **kw)["att"], TD.ref_cross(c, inp)["att"]
    c = TD.GEGLU[cid]
    inp = TD.build_geglu(c)
    return TD.ref_geglu(c, inp, **kw), TD.ref_geglu(c, inp)


@pytest.mark.parametrize("name,family,cid,kw", TD.MUTANTS, ids=[f"{m[0]}-{m[1]}-{m[2]}" for m in TD.MUTANTS])
def test_every_named_mutant_misses_the_tolerance_tenfold(name, family, cid, kw):
    got, want = _mutate(family, cid, kw)
    f = TD.used(got, want)
    print(name, family, cid, f"{f:.3g} x the allowance")
    assert f >= MUTANT_MARGIN


def test_mutant_list_names_every_kind_for_every_kernel_that_has_it():
    shared = ("columns_ge_512_dropped", "eps_omitted", "mean_over")
    for family, kinds in (("self", shared + ("lut_index_plus_1", "lut_index_minus_1", "scale")), ("cross", shared + ("scale",)),
                          ("geglu", shared + ("gate_and_value_swapped", "erf_gelu"))):
        for kind in kinds:
            assert any(m[1] == family and m[0].startswith(kind) for m in TD.MUTANTS), (family, kind)


@pytest.mark.parametrize("c", [c for c in TD.SELF_CASES if c.needles or c.own], ids=lambda c: c.id)
def test_each_dropped_self_needle_misses_the_tolerance_tenfold(c):
    inp = TD.build_self(c)
    want = TD.ref_self(c, inp)
    own = (TD.bf16r(want["k_new"]), TD.bf16r(want["v_new"]))
    got = TD.ref_self(c, inp, own=own, drop_key=c.needles or (c.t,))
    for b in range(c.B):  # every row has its own needle: every row must notice
        f = TD.used(got["att"][b], want["att"][b])
        print(c.id, "row", b, "key", (c.needles or (c.t,))[b], f"{f:.3g} x the allowance")
        assert f >= MUTANT_MARGIN


@pytest.mark.parametrize("c", [c for c in TD.CROSS_CASES if c.needles], ids=lambda c: c.id)
def test_each_dropped_cross_needle_misses_the_tolerance_tenfold(c):
    inp = TD.build_cross(c)
    want, got = TD.ref_cross(c, inp), TD.ref_cross(c, inp, drop_key=c.needles)
    for b in range(c.B):
        f = TD.used(got["att"][b], want["att"][b])
        print(c.id, "row", b, "key", c.needles[b], f"{f:.3g} x the allowance")
        assert f >= MUTANT_MARGIN


def test_a_lost_random_key_moves_the_output_a_hundred_times_less_than_a_lost_needle():
    """Why the needles exist: among 2048 random keys a dropped one moves some head by a few hundred allowances, a dropped needle
    moves every head of its row by more than 5e4 (the tests above print 8e4)."""
    c = TD.SELF["d1024_h2_t2047_last"]
    inp = TD.build_self(c)
    want = TD.ref_self(c, inp)
    got = TD.ref_self(c, inp, own=(TD.bf16r(want["k_new"]), TD.bf16r(want["v_new"])), drop_key=(256,) * c.B)
    fracs = [TD.used(got["att"][b, h * 64:(h + 1) * 64], want["att"][b, h * 64:(h + 1) * 64]) for b in range(c.B) for h in range(c.H)]
    print("dropped key 256 of 2048, per (row, head):", [f"{f:.3g}" for f in fracs])
    assert min(fracs) < 500
    n = TD.SELF["needle_n2048"]
    inp = TD.build_self(n)
    want = TD.ref_self(n, inp)
    got = TD.ref_self(n, inp, own=(TD.bf16r(want["k_new"]), TD.bf16r(want["v_new"])), drop_key=n.needles)
    assert min(TD.used(got["att"][b, h * 64:(h + 1) * 64], want["att"][b, h * 64:(h + 1) * 64]) for b in range(n.B) for h in range(n.H)) > 5e4


def test_case_lists_reach_every_geometry_the_kernels_branch_on():
    S, C, G = TD.SELF_CASES, TD.CROSS_CASES, TD.GEGLU_CASES
    for cases in (S, C, G):
        ds = {c.d for c in cases}
        assert any(d < 512 for d in ds) and 512 in ds and 520 in ds and 1024 in ds      # ragged / full first group, 1 chunk / full second
        assert {1, 9, 64} <= {c.B for c in cases} and any(c.B == 8 for c in cases)
        assert any(c.tiny_row is not None for c in cases)
    assert {c.H for c in S if c.d == 512} >= {1, 6, 12} and {c.H for c in C} >= {1, 6, 12}
    assert {c.Tmax for c in S} == {64, 300, 2048}
    assert {c.t for c in S} >= {0, 1, 31, 32, 255, 256, 257}
    assert all(any(c.t == c.Tmax - 1 and c.Tmax == T for c in S) for T in (64, 300, 2048))
    planted = {j for c in S for j in c.needles} | {c.t for c in S if c.own}
    assert planted >= {0, 31, 32, 255, 256, 257, 2046, 2047} and all(any(c.n - 2 in c.needles for c in S if c.n == n) for n in (33, 258, 2048))
    assert {c.S for c in C} == {16, 300, 2048}
    lens = {(ln if ln <= 0 else "S" if ln == c.S else "S+5" if ln == c.S + 5 else ln) for c in C for ln in c.src_len}
    assert lens >= {0, -3, 1, 255, 256, 257, "S", "S+5"}
    assert {j for c in C for j in c.needles} >= {0, 31, 32, 255, 256, 257, 2046, 2047}
    assert {c.F for c in G} == {8, 24, 1024, 1032} and {c.ldh - c.F for c in G} == {0, 4}
    assert {c.nt for c in TD.NEXT_CASES} == {1, 4, 125, 300} and {c.B for c in TD.NEXT_CASES} >= {1, 64}


def test_next_token_reference_plants_what_it_says():
    c = next(c for c in TD.NEXT_CASES if c.id == "nt300_b64")
    inp = TD.build_next(c)
    r = TD.ref_next(c, inp)
    for val, idx in inp["steps"]:
        for row, (a, b) in enumerate(((3, 5), (10, 70), (34, 290))):
            assert val[row, a] == val[row, b] == val[row].max() and idx[row, b] < idx[row, a]  # the later tile has the lower index
            assert TD.argmax_lowest(val[row], idx[row]) == int(idx[row, b])
        assert torch.isinf(val[3]).all() and TD.argmax_lowest(val[3], idx[3]) == int(idx[3].min())
    assert torch.equal(r["tokens"][:, :TD.NEXT_P], inp["prompt"]) and torch.equal(r["nexts"][0], inp["prompt"][:, 1])
    assert r["finished"][c.B - 1] == 1 and r["out_len"][c.B - 1] == TD.NEXT_P + 1 and not r["finished"].all()
    done = r["finished"].bool() & (r["out_len"] == TD.NEXT_P + 1)
    assert (r["tokens"][done, TD.NEXT_P + 1] == TD.PAD_ID).all(), "a finished row emits the pad id"
    c2 = next(c for c in TD.NEXT_CASES if not c.eos)
    assert not TD.ref_next(c2, TD.build_next(c2))["finished"].any()


def test_distance_lut_is_the_bias_of_every_causal_pair_up_to_2048():
    """distance_lut(rp, Tmax)[h, t - j] == bias[h, buckets(Tmax, one-sided)[t, j]] for EVERY j <= t < 2048 (the oracle's bucket
    function, not the module's), not only for the last row the table is built from."""
    from pytorch_models.text.t5 import RelativePositionBias
    from pytorch_models.text.t5_generate import distance_lut

    Tmax, H = 2048, 3
    rp = RelativePositionBias(H)
    rp.bias.copy_(torch.randn(H, 32, generator=torch.Generator().manual_seed(7)))
    lut = distance_lut(rp, Tmax)
    assert lut.shape == (H, Tmax) and lut.dtype == torch.float32 and lut.is_contiguous()
    bk = R5.buckets(Tmax, False)
    t, j = torch.tril_indices(Tmax, Tmax)
    assert torch.equal(lut[:, t - j], rp.bias.detach()[:, bk[t, j]])
    assert len(set(bk[Tmax - 1].tolist())) == 32 and int(bk[Tmax - 1, 0]) == 31  # every bucket is in use, the far end is the last


def test_interleaved_wv_is_gate_row_then_value_row():
    from pytorch_models.text.t5 import GEGLU
    from pytorch_models.text.t5_generate import _interleaved_wv

    c = TD.GEGLU["f24_d520_b9_pad"]
    inp = TD.build_geglu(c)
    m = GEGLU(c.d, c.F)
    m.w.weight.copy_(inp["w"])
    m.v.weight.copy_(inp["v"])
    wv = _interleaved_wv(m)
    assert wv.dtype == torch.bfloat16 and wv.shape == (2 * c.F, c.d) and wv.is_contiguous()
    assert torch.equal(wv.float(), TD.interleave(inp["w"], inp["v"]))
    for f in (0, 1, c.F - 1):
        assert torch.equal(wv[2 * f].float(), inp["w"][f]) and torch.equal(wv[2 * f + 1].float(), inp["v"][f])


def test_the_gpu_file_calls_every_entry_point():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_t5_decode.py")).read()
    for name in ("pm_t5_dec_embed", "pm_t5_dec_self_fused", "pm_t5_dec_rms_qkv", "pm_t5_dec_self_attention", "pm_t5_dec_cross_fused",
                 "pm_t5_dec_geglu", "pm_t5_dec_next_token"):
        assert f"L.{name}(" in src, name
