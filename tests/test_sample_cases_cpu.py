"""No GPU: the sampling tail's float64 reference (tests/sample_cases.py) against brute force, before the GPU tests rely on it, and
the host side of the new arguments.
  * the nucleus of row_reference equals the one found by torch.sort + cumsum in float64, written independently;
  * the replayed draws of a V = 8 row over 16384 (position, row) keys hit every token with its exact probability (the draws are
    counter-based, so the counts are deterministic; the bound is 5 sigma of the binomial);
  * the kept case table is clear of every edge by the reference alone and still covers every size, setting and family;
  * check_sampling / dec_sample / GreedyDecoder refuse bad arguments before anything touches a device."""
import math

import pytest
import torch

import sample_cases as S

torch.set_grad_enabled(False)


def _rows():
    g = torch.Generator().manual_seed(11)
    for V in (5, 64, 257, 1000):
        lg = torch.randn(4, V, generator=g) * 3
        lg[1, ::3] = -math.inf
        lg[2, : V // 2] = lg[2, V // 2 : 2 * (V // 2)]  # ties everywhere
        lg[3] = 0.5
        yield from lg


@pytest.mark.parametrize("topk", S.TOPKS)
def test_nucleus_equals_sort_and_cumsum(topk):
    n = 0
    for l in _rows():
        for T in S.TEMPS[1:]:
            for p in S.TOP_PS:
                rr = S.row_reference(l, topk, T, p)
                if rr.nucleus_edge <= 1e-9:  # the two float64 summation orders may disagree only AT an edge
                    continue
                assert set(rr.order.tolist()) == S.brute_nucleus(l, topk, T, p), (topk, T, p, l.numel())
                if topk == 0:
                    assert rr.order.tolist() == sorted(rr.order.tolist())
                n += 1
    assert n > 200


def test_draw_frequencies_match_the_distribution():
    l = torch.tensor([0.3, -1.0, 2.0, -math.inf, 0.3, 1.1, -2.5, 0.0])
    N = 16384
    for topk, T, p in ((0, 1.0, 1.0), (0, 0.7, 0.9), (5, 1.3, 1.0), (3, 0.7, 0.5)):
        rr = S.row_reference(l, topk, T, p)
        probs = torch.zeros(8, dtype=torch.float64)
        probs[rr.order] = torch.diff(rr.cum, prepend=torch.zeros(1, dtype=torch.float64)) / rr.cum[-1]
        counts = torch.zeros(8)
        for key in range(N):
            counts[S.draw(rr, 77, key % 128, key // 128)[0]] += 1
        sigma = torch.sqrt(N * probs * (1 - probs))
        worst = float(((counts - N * probs).abs() / sigma.clamp(min=1e-9))[probs > 0].max())
        print(f"topk {topk} T {T} p {p}: worst deviation {worst:.2f} sigma over {N} draws")
        assert counts[probs == 0].sum() == 0, "a token outside the nucleus (or of weight 0) was drawn"
        assert worst < 5.0


def test_the_kept_table_is_clear_and_covers_the_issue():
    kept = S.kept()
    for c in kept:
        inp = S.build(c)
        assert inp["nucleus_edge"] > S.DRAW_MARGIN and all(inp["draw_edge"][s] > S.DRAW_MARGIN for s in inp["seeds"]), c.id
    for attr, want in (("B", {1, 3, 64}), ("V", {5, 257, 1000, 50257}), ("topk", set(S.TOPKS)), ("temperature", set(S.TEMPS)),
                       ("top_p", set(S.TOP_PS)), ("family", {"planted", "gauss", "equal", "dominant", "neginf", "huge"})):
        assert {getattr(c, attr) for c in kept} == want, attr
    whole = {(c.temperature, c.top_p) for c in kept if c.V == 50257 and c.B == 64 and c.topk == 0}
    assert (0.7, 0.9) in whole and (1.0, 1.0) in whole, "the real vocabulary at the full batch must keep its whole-vocabulary cases"
    assert any(c.ragged for c in kept) and any(c.pos + 1 < c.P for c in kept)
    print(f"{len(kept)} of {len(S.cases())} candidate cases kept")


def test_dominant_and_neginf_rows_have_one_answer():
    for c in S.kept():
        inp = S.build(c)
        if c.family == "dominant":
            want = inp["logits"].argmax(-1)
            assert all(torch.equal(inp["picks"][s], want) for s in inp["seeds"]) and len(inp["seeds"]) == 4
        if c.family == "neginf":
            for s in inp["seeds"]:
                assert bool(torch.isfinite(inp["logits"].gather(1, inp["picks"][s][:, None])).all())


def test_the_model_level_runs_are_clear_by_the_oracle_alone():
    """the seeds, weights and prompts of tests/test_hip_sample.py: the reference decoding by itself meets no unclear position (cap 10 %),
    and its greedy margins are far above the 2e-5 of the arg-max rule (cap 5 %)"""
    from oracle import ref_text as RX
    from oracle import ref_whisper as RW

    _, sd, prompt = S.gpt2_setup()
    _, edges = S.oracle_sampled_run(S.gpt2_last_logits(sd), prompt, S.GPT2_RUN)
    print(f"gpt2 sampled: smallest edge distance {float(edges.min()):.3e}")
    assert float((edges <= S.DRAW_MARGIN).float().mean()) <= S.EDGE_CAP / 2
    unclear = 0
    for b, n in enumerate(S.RAGGED_LENGTHS):
        _, e = S.oracle_sampled_run(S.gpt2_last_logits(sd), prompt[b : b + 1, :n], S.GPT2_RUN, t_shift=max(S.RAGGED_LENGTHS) - n, rows=[b])
        unclear += int((e <= S.DRAW_MARGIN).sum())
    print(f"gpt2 ragged sampled: {unclear} unclear positions")
    assert unclear <= S.EDGE_CAP / 2 * 3 * S.GPT2_RUN["n_new"]
    margins = RX.greedy(RX.gpt2, sd, prompt, 8, rp=S.kv_round)[1]
    assert float(margins.min()) > 1e-2
    _, wsd, memory, wp = S.whisper_setup()
    _, edges = S.oracle_sampled_run(S.whisper_last_logits(wsd, memory, wp.shape[1], True), wp, S.WHISPER_RUN)
    print(f"whisper sampled: smallest edge distance {float(edges.min()):.3e}")
    assert float((edges <= S.DRAW_MARGIN).float().mean()) <= S.EDGE_CAP / 2
    wm = RW.greedy_cached(wsd, "decoder.", wp, memory, 8, rp=S.kv_round)[1]
    print(f"smallest greedy margins: gpt2 {float(margins.min()):.3e} whisper {float(wm.min()):.3e}")
    assert float(wm.min()) > 1e-2


# ------------------------------------------------------------------------------------------------------------------- host side
BAD = [dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=1.5),
       dict(top_p=float("nan")), dict(top_p=-0.1), dict(topk=-1), dict(topk=65), dict(topk=2.0), dict(temperature=1e-60)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_check_sampling_refuses(bad):
    from pytorch_models._hip.sampling import check_sampling, dec_sample

    args = dict(topk=0, temperature=0.7, top_p=0.9)
    check_sampling("t", **args)
    args.update(bad)
    with pytest.raises(ValueError):
        check_sampling("t", **args)
    z = torch.zeros(1)
    with pytest.raises(ValueError):  # before the device check: CPU tensors never get that far
        dec_sample(z, z, z, z, z, z, z, z, **args)


@pytest.mark.parametrize("form", ("plain", "ragged", "topk"))
def test_wrapper_variants_are_refused_before_a_launch_or_reach_it_whole(form, monkeypatch):
    """the CPU stage of tests/wrapper_cases.py on the new wrapper: the library is test_wrapper_cases_cpu's recording stub; a refusal
    records no launch and leaves the in-place operands alone, an accepted variant changes the launch or is the canonical one"""
    import wrapper_cases as WC
    from pytorch_models._hip import sampling
    from test_wrapper_cases_cpu import _install

    rec = _install(monkeypatch)
    monkeypatch.setattr(sampling, "lib", lambda: rec)
    monkeypatch.setattr(sampling, "_stream", lambda: 0)
    r = S.wrapper_rows()[form]
    kw = r.build(torch.device("cpu"))
    rec.begin()
    WC.call(sampling, r, kw)
    assert [n for n, _ in rec.launches] == ["pm_dec_sample_ragged" if form == "ragged" else "pm_dec_sample"]
    early = {i for i, n in rec.seen if n == 0}
    assert all(id(t) in early for _, t in WC.operands(kw)), "an operand check_devices has not seen before the launch"
    problems, accepted = WC.check_row(sampling, r, torch.device("cpu"), compare=False, hook=rec)
    assert accepted and not problems, "\n".join([f"{len(problems)} problems:"] + problems)


def test_dec_sample_has_no_cpu_path():
    from pytorch_models._hip.sampling import dec_sample

    z = torch.zeros(1)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        dec_sample(z, z, z, z, z, z, z, z, topk=0, temperature=0.7, top_p=0.9)


def test_defaults_do_not_ask_for_the_tail():
    from pytorch_models._hip.sampling import wants_sampling_tail

    assert not wants_sampling_tail(1, 1.0, 1.0, False) and not wants_sampling_tail(50, 1.0, 1.0, False)
    for kw in (dict(topk=0), dict(temperature=0.0), dict(temperature=0.7), dict(top_p=0.9), dict(return_logprobs=True)):
        assert wants_sampling_tail(**{**dict(topk=1, temperature=1.0, top_p=1.0, return_logprobs=False), **kw})


class _Dec:  # what the refusals read of a decoder before they touch a device
    def __init__(self, dtype):
        self.token_embs = torch.nn.Embedding(16, 8).to(dtype)


def test_greedy_decoder_refusals_come_first():
    from pytorch_models.audio2text.generate import GreedyDecoder, check_sampling_tail

    prompt = torch.zeros(1, 2, dtype=torch.int64)
    bf, f32 = _Dec(torch.bfloat16), _Dec(torch.float32)
    for kw, exc in ((dict(temperature=-1.0), ValueError), (dict(top_p=0.0), ValueError), (dict(topk=0, margins=True), ValueError),
                    (dict(return_logprobs=True, beams=2), ValueError), (dict(temperature=0.5, path="persistent"), NotImplementedError),
                    (dict(top_p=0.5, kv32=True), NotImplementedError)):
        with pytest.raises(exc) as e:
            GreedyDecoder(bf, None, prompt, 2, **kw)
        assert "greedy decode" in str(e.value)
    with pytest.raises(NotImplementedError, match="bf16 parameters"):
        GreedyDecoder(f32, None, prompt, 2, return_logprobs=True)
    assert check_sampling_tail("x", 1, 1.0, 1.0, False, beams=4, path="persistent", kv32=True, fp32=True) is False  # the defaults ask nothing
    for kw, exc, names in ((dict(beams=2), ValueError, "beams=1"), (dict(margins=True), ValueError, "return_logprobs"),
                           (dict(path="persistent"), NotImplementedError, "launches"), (dict(kv32=True), NotImplementedError, "exact=False"),
                           (dict(fp32=True), NotImplementedError, "bfloat16")):
        with pytest.raises(exc, match=names):  # each names the form that does run
            check_sampling_tail("x", 0, 0.7, 0.9, True, **kw)


def test_entry_points_take_the_keywords():
    import inspect

    from pytorch_models.audio2text import Whisper
    from pytorch_models.audio2text.generate import greedy_decode
    from pytorch_models.audio2text.whisper import WhisperDecoder
    from pytorch_models.text import GPT2
    from pytorch_models.text.generator import DecoderGenerator

    for fn in (greedy_decode, GPT2.generate, WhisperDecoder.generate, Whisper.generate):
        ps = inspect.signature(fn).parameters
        for name, default in (("topk", 1), ("seed", 0), ("temperature", 1.0), ("top_p", 1.0), ("return_logprobs", False)):
            assert ps[name].default == default and ps[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, name)
    for fn in (DecoderGenerator.generate_ids, DecoderGenerator.generate_ids_batch, DecoderGenerator.generate_batch, DecoderGenerator.generate):
        ps = inspect.signature(fn).parameters
        assert ps["temperature"].default == 1.0 and ps["top_p"].default == 1.0 and "return_logprobs" not in ps, fn.__qualname__
