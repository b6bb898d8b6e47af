"""CPU: the graph replay contract without a GPU (tests/graph_cases.py; the kernels and the models are in
tests/test_hip_graph_ops.py and tests/test_hip_graph_models.py).

Three things are checked here.  The tables are complete: every row of wrapper_cases.ROWS is replayed or refused with a reason,
and so is every exported model class and every entry point README.md names.  The protocol has teeth: driven with a recording
fake in place of stream capture, each of the defects a replay can hide is planted in a toy op and must be reported, and the
honest op must pass.  And the capture guard answers first: with the capture flag forced on, every host-bound wrapper raises
its RuntimeError on CPU operands - in front of the device check, hence in front of any device access."""
import inspect
import os
import re

import pytest
import torch
from torch import nn

import graph_cases as GC
import wrapper_cases as WC
from pytorch_models._hip import ops

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ completeness
def test_every_wrapper_row_is_captured_or_host_bound():
    assert len(set(GC.CAPTURED)) == len(GC.CAPTURED)
    assert set(GC.CAPTURED) | set(GC.HOST_BOUND) == set(WC.ROWS), sorted(set(WC.ROWS) ^ (set(GC.CAPTURED) | set(GC.HOST_BOUND)))
    assert all(isinstance(why, str) and why and "\n" not in why for why in GC.HOST_BOUND.values())
    # in both tables: only the rows whose host form is an operand choice (host_ok); a row with host_ok operands is in HOST_BOUND
    assert {r for r in GC.HOST_BOUND if r in GC.CAPTURED} == {r.id for r in WC.ROWS.values() if r.host_ok}
    assert set(GC.SAME_OK) <= set(GC.CAPTURED) and {rid for rid, _ in GC.SHARED} <= set(GC.CAPTURED)
    for rid, names in GC.SAME_OK.items():
        assert set(names) <= set(WC.ROWS[rid].inplace), rid


def _exported_modules() -> dict:
    from pytorch_models import audio, audio2text, image, text

    out = {}
    for pkg in (image, audio, audio2text, text):
        for name, obj in vars(pkg).items():
            if inspect.isclass(obj) and not name.startswith("_") and obj.__module__.startswith("pytorch_models."):
                out[name] = obj
    return out


def _covered(name: str) -> bool:
    keys = list(GC.NOT_GRAPHED) + [m.cls if m.method is None else f"{m.cls}.{m.method}" for m in GC.MODELS.values()]
    return any(k == name or k.startswith(name + ".") for k in keys)


def test_every_exported_model_class_is_replayed_or_listed():
    exported = _exported_modules()
    assert {"ViT", "DETR", "Wav2Vec2CTC", "Whisper", "T5Model", "EnCodec"} <= set(exported)
    missing = [n for n in exported if not _covered(n)]
    assert not missing, f"neither in MODELS nor in NOT_GRAPHED: {missing}"
    for key, m in GC.MODELS.items():
        assert m.cls in exported and issubclass(exported[m.cls], nn.Module), key
        assert hasattr(exported[m.cls], m.method or "forward"), key
    assert all(isinstance(why, str) and why and "\n" not in why for why in GC.NOT_GRAPHED.values())


def test_every_entry_point_the_readme_names_is_replayed_or_listed():
    text = open(os.path.join(ROOT, "README.md")).read()
    named = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*\.(?:%s))\b" % "|".join(GC.ENTRY_WORDS), text))
    exported = set(_exported_modules()) | {"audio2text"}
    named = {n for n in named if n.split(".")[0] in exported}
    assert {"BERT.forward", "T5Model.generate", "Whisper.align", "GPT2.score"} <= named  # the pattern still finds them
    replayed = {m.cls + "." + (m.method or "forward") for m in GC.MODELS.values()}
    missing = sorted(n for n in named if n not in replayed and n not in GC.NOT_GRAPHED)
    assert not missing, f"named in README.md, neither replayed nor listed: {missing}"


# ------------------------------------------------------------------------------------------------------------ the protocol's teeth
class Toy:
    """y = 2 x + 1 into a fresh tensor, through a FakeGraphs: host code runs at the call, 'kernels' go through launch()"""

    def __init__(self, fake: GC.FakeGraphs, defect: str | None) -> None:
        self.fake, self.defect = fake, defect
        self.counter = torch.zeros(1)
        self.buf = {}

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        d = self.defect
        if d == "recycled_output":  # one private buffer handed out again and again: the next call overwrites the last result
            out = self.buf.setdefault(tuple(x.shape), torch.empty_like(x))
        else:
            out = torch.empty_like(x)
        scale = float(x.flatten()[0]) if d == "baked_scalar" else None  # a host read of device data, baked into the launch
        src = x.clone() if d == "private_copy" else x  # the launch reads a copy made on the host, at capture
        if d == "wrapper_reset":
            self.counter.zero_()  # host side: happens at capture only

        def kernel():
            y = 2.0 * src + 1.0
            if d == "baked_scalar":
                y = y + (scale - x.flatten()[0])  # zero for the data the scalar was read from
            if d == "wrapper_reset":
                y = y + self.counter  # the kernel expects to find it zero and leaves it non-zero
                self.counter.add_(1.0)
            if d == "allocates":
                self.fake.bytes += x.numel() * 4
            out.copy_(y)

        self.fake.launch(kernel)
        return out


def _drive(defect, set_b=None):
    fake = GC.FakeGraphs()
    op = Toy(fake, defect)
    g = torch.Generator().manual_seed(5)
    a = [torch.randn(2, 3, generator=g)]
    b = [torch.randn(2, 3, generator=g)] if set_b is None else set_b(a)
    return GC.check_replay(lambda s: op(s[0]), a, b, lambda st, src: st[0].copy_(src[0]), capture=fake.capture, replay=fake.replay,
                           clone=lambda s: [t.clone() for t in s], snap=lambda s, res: [("output 0", res.clone())],
                           allocated=fake.allocated, hook=lambda: op(torch.ones(4, 5)))


def test_the_honest_toy_op_replays():
    assert _drive(None) == []


@pytest.mark.parametrize("defect,word", [("baked_scalar", "replay on new operands"), ("private_copy", "replay on new operands"),
                                         ("wrapper_reset", "second replay"), ("allocates", "memory in use"),
                                         ("recycled_output", "does not own its memory")])
def test_each_planted_defect_is_reported(defect, word):
    problems = _drive(defect)
    assert problems and any(word in p for p in problems), problems


def test_a_case_whose_two_sets_agree_is_a_failure_of_the_case():
    with pytest.raises(GC.CaseProvesNothing):
        _drive(None, set_b=lambda a: [a[0].clone()])


def test_the_second_operand_set_of_every_row_differs_in_every_floating_operand():
    for rid in GC.CAPTURED:
        r = WC.ROWS[rid]
        a, b = GC.row_sets(r, CPU)  # raises CaseProvesNothing on a floating operand the two builds share
        assert [p for p, _ in WC.operands(a)] == [p for p, _ in WC.operands(b)], rid
        for path, t in WC.operands(a):
            assert WC.get(b, path).shape == t.shape, (rid, path)
        c = GC.clone_kw(a)
        GC.overwrite_kw(c, b)
        assert all(WC.same_bits(WC.get(c, p), t) for p, t in WC.operands(b)), rid
        assert all(WC.same_bits(WC.get(r.build(CPU), p), t) for p, t in WC.operands(a)), rid  # the canonical build: unchanged


# ------------------------------------------------------------------------------------------------------------------- the guard
@pytest.fixture
def capturing(monkeypatch):
    monkeypatch.setattr(ops, "capturing", lambda: True)


def _guarded(who: str):
    return pytest.raises(RuntimeError, match=rf"(?s){re.escape(who)}.*capture")


@pytest.mark.parametrize("rid", list(GC.HOST_BOUND))
def test_host_bound_wrappers_raise_the_guard_in_front_of_any_device_access(rid, monkeypatch):
    r = WC.ROWS[rid]
    kw = GC.host_kw(r, r.build(CPU))  # CPU operands: past the guard the device check would refuse them with another message
    monkeypatch.setattr(ops, "capturing", lambda: True)
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail(f"{rid}: reached the library under capture"))
    with _guarded(r.fn):
        WC.call(ops, r, kw)


def test_host_helpers_and_entry_points_raise_the_guard(capturing):
    from pytorch_models.audio2text import align as A
    from pytorch_models.text import gpt2, t5_generate

    with _guarded("seq_lens"):
        ops.seq_lens([3, 5], 6, CPU)
    with _guarded("stft_tables"):
        ops.stft_tables(torch.hann_window(64), 64)
    with _guarded("mel_csr"):
        ops.mel_csr(torch.rand(6, 33))
    with _guarded("my_op"):
        ops.align_counts([1, 2], 2, 0, 5, "my_op: counts", CPU)
    tok = torch.zeros((2, 5), dtype=torch.int64)
    with _guarded("GPT2.score"):
        gpt2.score_targets(tok, [5, 4], "GPT2.score")
    assert gpt2.score_targets(tok, None, "GPT2.score").shape == (2, 4)  # without lengths nothing is read: no guard
    with _guarded("T5Model.generate"):
        t5_generate.generate(None, tok)
    with _guarded("WhisperDecoder.align"):
        A.align(None, tok, torch.zeros(2, 8, 64))


def test_the_guard_is_silent_outside_a_capture():
    assert ops.capturing() is False  # no HIP context in this process: nothing can be capturing
    assert ops.seq_lens([3, 5], 6, CPU).total == 8
    ops.no_capture("anything", "reads nothing")
