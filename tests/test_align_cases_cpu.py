"""CPU: the token-timestamp reference of tests/align_cases.py against brute force, the planted case, the conditioning of every
kernel case, Whisper.align on a CPU model against the reference run on the oracle's q / k, the ABI of the pm_align_* entry points
and the refusals that must come before any launch."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import align_cases as ac
from pytorch_models import _hip

torch.set_grad_enabled(False)


def test_reference_median_against_brute_force():
    g = torch.Generator().manual_seed(5)
    for F in (4, 5, 7, 8, 13, 40):
        n = torch.randn((3, F), generator=g, dtype=torch.float64)
        got = ac.median7(n)
        for r in range(3):
            for f in range(F):
                win = []
                for i in range(-3, 4):
                    j = f + i
                    j = -j if j < 0 else j
                    j = 2 * (F - 1) - j if j > F - 1 else j
                    win.append(float(n[r, j]))
                assert float(got[r, f]) == sorted(win)[3], (F, r, f)


def test_selection_network_of_the_kernel_is_a_median():
    """csrc/align.hip's 13 exchanges: by the zero-one principle a network that selects the median of every 0/1 input selects it
    of every input."""
    net = ((0, 5), (0, 3), (1, 6), (2, 4), (0, 1), (3, 5), (2, 6), (2, 3), (3, 6), (4, 5), (1, 4), (1, 3), (3, 4))
    src = open(os.path.join(_hip.REPO_PKG_ROOT, "csrc", "align.hip")).read()
    body = src[src.index("al_med7(float p0"):]
    body = body[: body.index("return p3")]
    assert tuple((int(a), int(b)) for a, b in re.findall(r"AL_SORT2\(p(\d), p(\d)\)", body)) == net
    for bits in itertools.product((0.0, 1.0), repeat=7):
        p = list(bits)
        for a, b in net:
            p[a], p[b] = min(p[a], p[b]), max(p[a], p[b])
        assert p[3] == sorted(bits)[3], bits


def test_reference_dtw_cost_against_every_path():
    g = np.random.default_rng(3)
    for N, M in itertools.product((1, 2, 3), (1, 2, 3, 4)):
        for trial in range(4):
            x = g.standard_normal((N, M)) if trial < 3 else g.integers(-2, 3, (N, M)).astype(np.float64)
            path, cost = ac.dtw_path(x)
            assert math.isclose(cost, ac.brute_force_cost(x), rel_tol=0, abs_tol=1e-12), (N, M)
            assert path[0] == (N - 1, M - 1) and path[-1] == (0, 0)
            assert math.isclose(sum(x[i, j] for i, j in path), cost, rel_tol=0, abs_tol=1e-12)
            for (i1, j1), (i0, j0) in zip(path, path[1:]):
                assert (i1 - i0, j1 - j0) in ((1, 1), (1, 0), (0, 1))


def test_fp32_and_fp64_dtw_agree_on_integer_matrices():
    name, m, lens, frs, s0, s1 = next(c for c in ac.dtw_cases() if c[0] == "ints")
    assert torch.equal(ac.dtw_start(m, lens, frs, s0, s1, np.float32), ac.dtw_start(m, lens, frs, s0, s1, np.float64))


def test_planted_case_recovers_its_boundaries():
    q, k, bounds = ac.planted()
    ref = ac.reference([(q, k, (0, 1, 2))], (12,), (k.shape[1],))
    start = ac.dtw_start(ref.m.float(), (12,), (k.shape[1],), 0, 0)
    assert start[0].tolist() == bounds[:-1]


def test_single_row_gives_an_all_zero_matrix():
    case = ac.Case("single", 1, 1, 30, 2, ((0, 1),), (1,), (30,))
    ref = ac.reference(ac.build(case), case.lens, case.frs)
    assert bool((ref.m == 0).all()) and bool((ref.m_bound == 0).all()) and bool(ref.zero_std.all())
    assert ac.dtw_start(ref.m.float(), (1,), (30,), 0, 0)[0].tolist() == [0]


@pytest.mark.parametrize("case", ac.cases(), ids=lambda c: c.id)
def test_every_kernel_case_is_well_conditioned(case):
    """On the reference alone: no column with a finite std sits where the bound stops being informative, the bound is finite, and
    the logits' standard deviation over the tokens is in the stated range."""
    groups = ac.build(case)
    ref = ac.reference(groups, case.lens, case.frs)
    print(f"COND {case.id}: max dstd / std {ref.cond:.3e} (asserted <= {ac.COND_MAX}); bound max {float(ref.m_bound.max()):.3e}, "
          f"|m| rms {float(ref.m.square().mean().sqrt()):.3e}")
    assert ref.cond <= ac.COND_MAX
    assert bool(torch.isfinite(ref.m_bound).all()) and float(ref.m_bound.max()) < 1e-2
    if case.family not in ("flat", "dominant") and min(case.lens) > 4:
        q, k, heads = groups[0]
        h = heads[0]
        x = q[0, : case.lens[0], 64 * h : 64 * h + 64].double() @ k[0, : case.frs[0], 64 * h : 64 * h + 64].double().T / 8
        sd = float(x.std(0).mean())
        assert 0.3 <= sd <= 1.0, sd
    for b in range(case.B):
        assert bool((ref.m[b, case.lens[b]:] == 0).all()) and bool((ref.m[b, :, case.frs[b]:] == 0).all())
    if case.family == "flat":
        assert bool((ref.m == 0).all())


def test_bound_admits_fp32_arithmetic_and_catches_mutants():
    """The plain-torch fp32 form of the package stays inside 1.0 x the bound; an unbiased std, a zero-padded median and a
    median of 5 do not stay inside MARGIN x."""
    from pytorch_models.audio2text.align import head_matrix_torch

    case = next(c for c in ac.cases() if c.family == "odd")
    (q, k, heads), = ac.build(case)
    ref = ac.reference([(q, k, heads)], case.lens, case.frs)
    ln, F = case.lens[0], case.frs[0]

    def run(fn):
        m = torch.zeros((1, case.L, case.S))
        for h in heads:
            m[0, :ln, :F] += fn(q[0, :ln, 64 * h : 64 * h + 64], k[0, :F, 64 * h : 64 * h + 64])
        return m / len(heads)

    def mutant(unbiased=False, pad="reflect", width=7):
        def fn(qh, kh):
            p = torch.softmax(qh.float() @ kh.float().T * 0.125, -1)
            n = (p - p.mean(0)) / p.std(0, unbiased=unbiased)
            w = width // 2
            return torch.nn.functional.pad(n[None], (w, w), mode=pad)[0].unfold(-1, width, 1).sort(-1).values[..., w]
        return fn

    r = ac.ratio(run(head_matrix_torch), ref.m, ref.m_bound)
    print(f"RATIO fp32 torch form: {r:.3f} of the bound")
    assert r <= 1.0
    assert ac.ratio(run(mutant()), ref.m, ref.m_bound) <= 1.0
    for kw in (dict(unbiased=True), dict(pad="constant"), dict(width=5)):
        rm = ac.ratio(run(mutant(**kw)), ref.m, ref.m_bound)
        print(f"RATIO mutant {kw}: {rm:.3e}")
        assert rm > ac.MARGIN, kw


def test_whisper_align_on_the_cpu_equals_the_reference_on_the_oracle():
    from oracle import ref_whisper
    from synthweights import synth_input, synth_tokens

    w, sd = ac.small_whisper()
    mel = synth_input("align_mel", (2, 80, 120), 7)
    tokens = synth_tokens("align_tokens", (2, 9), 1000, 7)
    lens, frs = (9, 6), (60, 41)
    heads = [(1, 0), (1, 1), (0, 1)]
    start, m = w.align(mel, tokens, lengths=lens, frames=frs, heads=heads, skip_first=1, skip_last=1, return_matrix=True)
    assert start.shape == (2, 9) and start.dtype == torch.int32 and m.shape == (2, 9, 60) and m.dtype == torch.float32
    memory = ref_whisper.encoder(sd, "encoder.", mel)
    want = ac.oracle_matrix(sd, tokens, memory, heads, lens, frs)
    err = float((m.double() - want).abs().max())
    print(f"CPU align: max |m - reference on the oracle's q / k| = {err:.3e} (|m| max {float(want.abs().max()):.2f})")
    torch.testing.assert_close(m.double(), want, rtol=5e-5, atol=5e-5)  # the Whisper tolerance of the CPU forms (test_cpu_device.py)
    assert bool((m[1, 6:] == 0).all()) and bool((m[1, :, 41:] == 0).all())
    assert torch.equal(start, ac.dtw_start(m, lens, frs, 1, 1))
    assert bool((start[:, 0] == -1).all()) and int(start[0, 8]) == -1 and bool((start[1, 5:] == -1).all())
    assert bool((start[0, 1:8] >= 0).all())
    # defaults: every row, every frame, the upper half of the layers
    s2 = w.align(mel, tokens)
    m2 = w.decoder.align(tokens, w.encoder(mel), return_matrix=True)[1]
    want2 = ac.oracle_matrix(sd, tokens, memory, [(1, 0), (1, 1)], (9, 9), (60, 60))
    torch.testing.assert_close(m2.double(), want2, rtol=5e-5, atol=5e-5)
    assert torch.equal(s2, ac.dtw_start(m2, (9, 9), (60, 60), 0, 0))
    assert type(w).SECONDS_PER_FRAME == 0.02


def test_entry_points_declared_with_signatures():
    declared = _hip.header_functions()
    for name in ("pm_align_lse_bf16", "pm_align_matrix_bf16", "pm_align_dtw_f32", "pm_align_ws_bytes"):
        assert name in declared and name in _hip.SIGNATURES
    assert _hip.SIGNATURES["pm_align_ws_bytes"][1] is ctypes.c_int64
    L = _hip.lib()  # loadable without a GPU
    assert L.pm_align_ws_bytes(32, 448, 1500) == 32 * 448 * 61 * 8 and L.pm_align_ws_bytes(1, 1, 4) == 8
    assert L.pm_abi_version() == 1


def test_host_side_refusals_launch_nothing():
    """Rejected calls return their code before any HIP call, so this is safe without a GPU."""
    L = _hip.lib()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    ok = dict(q=p, ldq=128, qbs=1024, k=p, ldk=256, kbs=2048, heads=p, lens=p, frs=p, lse=p, m=p, ldm=8, mbs=64, B=1, L=4, S=8, n=1, H=2)

    def lse(**kw):
        a = {**ok, **kw}
        return L.pm_align_lse_bf16(a["q"], a["ldq"], a["qbs"], a["k"], a["ldk"], a["kbs"], a["heads"], a["lens"], a["frs"], a["lse"],
                                   a["B"], a["L"], a["S"], a["n"], a["H"], None)

    def mat(**kw):
        a = {**ok, **kw}
        return L.pm_align_matrix_bf16(a["q"], a["ldq"], a["qbs"], a["k"], a["ldk"], a["kbs"], a["heads"], a["lens"], a["frs"], a["lse"],
                                      a["m"], a["ldm"], a["mbs"], a["B"], a["L"], a["S"], a["n"], a["H"], 1.0, 1, None)

    def dtw(**kw):
        a = {**ok, "ws": p, "start": p, "s0": 0, "s1": 0, **kw}
        return L.pm_align_dtw_f32(a["m"], a["ldm"], a["mbs"], a["lens"], a["frs"], a["start"], a["ws"], a["B"], a["L"], a["S"], a["s0"],
                                  a["s1"], None)

    for f in (lse, mat):
        for name in ("q", "k", "heads", "lens", "frs", "lse"):
            assert f(**{name: None}) == 1, name  # PM_EINVAL
        assert f(ldq=64) == 1 and f(ldk=120) == 1 and f(L=0) == 1 and f(n=0) == 1  # a row shorter than the heads
        assert f(ldq=132) == 4 and f(kbs=2052) == 4 and f(q=p + 8) == 4 and f(k=p + 2) == 4  # PM_EALIGN
    assert mat(m=None) == 1 and mat(ldm=7) == 1 and mat(L=449) == 2  # PM_EUNSUPPORTED
    for name in ("m", "lens", "frs", "start", "ws"):
        assert dtw(**{name: None}) == 1, name
    assert dtw(s0=-1) == 1 and dtw(ldm=7) == 1 and dtw(L=449) == 2 and dtw(ws=p + 4) == 4


def test_align_refuses_before_any_launch(monkeypatch):
    from pytorch_models._hip import ops
    from pytorch_models.audio2text import align as al

    launched = []
    for name in ("align_lse", "align_matrix", "align_dtw", "embed_tokens", "linear"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    w, _ = ac.small_whisper()
    tokens = torch.zeros((2, 5), dtype=torch.int64)
    memory = torch.zeros((2, 30, 128))
    for kw in (dict(heads=[(2, 0)]), dict(heads=[(0, 2)]), dict(heads=[]), dict(heads=[(0, 0), (0, 0)]), dict(lengths=[5, 6]),
               dict(lengths=[0, 5]), dict(lengths=[5]), dict(frames=[3, 30]), dict(frames=[30, 31]), dict(skip_first=-1),
               dict(skip_last=1.5)):
        with pytest.raises(ValueError):
            w.decoder.align(tokens, memory, **kw)
    with pytest.raises(ValueError):
        w.decoder.align(tokens.int(), memory)
    with pytest.raises(ValueError):
        w.decoder.align(tokens, memory[:, :3])
    # fp32 parameters on a (pretended) HIP device: refused in the style of score_gate; a head dim other than 64 likewise
    monkeypatch.setattr(ops, "check_devices", lambda *ts: None)
    with pytest.raises(NotImplementedError, match="bf16 weights on a HIP device only"):
        al.align_gate("WhisperDecoder.align", w.decoder.token_embs.weight, 64, tokens, memory)
    with pytest.raises(NotImplementedError, match="head dim 64 only"):
        al.align_gate("WhisperDecoder.align", w.decoder.token_embs.weight.bfloat16(), 32, tokens, memory)
    al.align_gate("WhisperDecoder.align", w.decoder.token_embs.weight.bfloat16(), 64, tokens, memory)
    assert not launched
