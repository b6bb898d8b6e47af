"""Non-finite operand contract: what a NaN or an infinity INSIDE an operand may do, the protocol that
checks it and the tables that say which wrappers, decisions and models go through it.

Every other suite feeds the kernels finite operands (the poison families put NaN AROUND an operand, never inside it).  Two
properties of a batched call cannot be seen that way:

  isolation   one bad sample changes no bit of any other sample of the batch;
  visibility  a bad sample does not come back looking healthy: a NaN inside it leaves a non-finite value among its float
              results, and every integer it produces (token id, beam parent, label, code, frame) is still a valid index.

``check_isolation`` is written once over callables: tests/test_hip_nonfinite_ops.py and tests/test_hip_nonfinite_models.py pass
the kernels, tests/test_nonfinite_cases_cpu.py toy ops with each defect planted.  Everything is compared as bits, ranges or
finiteness; nothing here has a tolerance.

The tables: UNITS (id of wrapper_cases.ROWS -> which float operands carry samples and how every result is sliced into them),
NO_UNITS (row -> why no float operand is per-sample), SWALLOWS (row or model -> why a NaN may end finite: a maxNum clamp that
IS the operation, or an entry point without float results; per operand), IGNORED (row -> operand regions the documented
contract says are not read), PAD_COLUMNS (row -> operands re-laid with a leading dimension into a NaN parent), DECISIONS (the
entry points whose result is a choice, over row families built for it) and MODELS_POISON / ENTRY_POINTS (every entry of
graph_cases.MODELS and every decoding entry point README.md names).  UNITS | NO_UNITS is every row."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import torch
from torch import Tensor

import graph_cases as GC
import wrapper_cases as WC
from graph_cases import CaseProvesNothing  # noqa: F401 - the same failure of a case, not of an op

NAN, INF = float("nan"), float("inf")
POISONS = ("nan", "+inf", "-inf", "max")
NONE_IDX = 0x7FFFFFFF  # what an arg-max that found nothing used to write
SHARED, SKIP = "shared", "skip"  # a result no sample owns (it must keep its bits) / a workspace (its content is unspecified)
I32, I64, BF = torch.int32, torch.int64, torch.bfloat16


def poison_value(name: str, dtype) -> float:
    return {"nan": NAN, "+inf": INF, "-inf": -INF}[name] if name != "max" else torch.finfo(dtype).max


# ---------------------------------------------------------------------------------------------------------------- the protocol
@dataclass
class Unit:
    """``operands``: (name or path, sample dimension[, at]) of every per-sample float operand - ``at`` places the poisoned element
    inside sample u: {dimension: index} over the default of index 0 everywhere, or a callable (kw, rows of u, poison) -> full index;
    ``outs``: result name -> its sample dimension, SHARED or SKIP (None, or a missing name: dimension 0); ``samples``: how many
    samples the call holds (None: the extent of the first operand, or the sequences of ``seq``); ``packed``: an extent equal to
    seq.total maps rows to samples through the lengths of the call's SeqLens; an extent that is a multiple k S of the sample count
    holds k consecutive rows per sample (M = B x L); ``ranges``: integer result -> (lo, hi), lo <= value < hi; ``writes_neginf``:
    the op's own results hold -inf by definition (a logit filter): -inf in the clean run proves nothing wrong, and visibility is a
    non-finite value where the clean run holds a finite one."""
    operands: tuple
    outs: dict | None = None
    samples: object = None
    packed: bool = False
    ranges: dict = field(default_factory=dict)
    writes_neginf: bool = False


def U(*operands, outs=None, samples=None, packed=False, ranges=None, writes_neginf=False) -> Unit:
    norm = []
    for o in operands:
        o = (o,) if isinstance(o, str) else tuple(o)
        path = (o[0],) if isinstance(o[0], str) else tuple(o[0])
        norm.append((path, o[1] if len(o) > 1 else 0, o[2] if len(o) > 2 else None))
    return Unit(tuple(norm), outs, samples, packed, dict(ranges or {}), writes_neginf)


def n_samples(unit: Unit, kw: dict) -> int:
    if callable(unit.samples):
        return int(unit.samples(kw))
    if unit.samples is not None:
        return int(unit.samples)
    if unit.packed:
        return len(kw["seq"].lengths)
    path, dim, _ = unit.operands[0]
    return int(WC.get(kw, path).shape[dim])


def sample_ids(extent: int, S: int, lengths=None) -> Tensor:
    """the sample every index of a dimension of ``extent`` belongs to"""
    if extent == S:
        return torch.arange(S)
    if lengths is not None and extent == sum(lengths):
        return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(list(lengths)))
    if S > 0 and extent % S == 0:
        return torch.repeat_interleave(torch.arange(S), extent // S)
    raise ValueError(f"an extent of {extent} does not hold {S} samples")


def unit_sample(S: int) -> int:
    """a middle sample, never the first or the last; of two, the second"""
    assert S >= 2, S
    return S // 2 if S >= 3 else 1


def _lengths(unit: Unit, kw: dict):
    return list(kw["seq"].lengths) if unit.packed else None


def poisoned(kw: dict, unit: Unit, which: int, value: float, u: int, S: int, poison: str = "nan") -> tuple[dict, tuple]:
    """``kw`` with ONE element of sample u of operand ``which`` set to ``value`` (the tensor is cloned first); and its index"""
    path, dim, at = unit.operands[which]
    t = WC.get(kw, path).clone()
    rows = (sample_ids(t.shape[dim], S, _lengths(unit, kw)) == u).nonzero().flatten()
    if callable(at):
        idx = tuple(int(i) for i in at(kw, rows, poison))
    else:
        idx = [0] * t.dim()
        idx[dim] = int(rows[0])
        for d, i in (at or {}).items():
            idx[d] = i
        idx = tuple(idx)
    assert int(idx[dim]) in rows.tolist(), (path, idx)
    t[idx] = value
    return WC.replaced(kw, path, t), idx


def _finite(t: Tensor) -> bool:
    return not t.is_floating_point() or bool(torch.isfinite(t.float()).all())


def compare(unit: Unit, kw: dict, clean, got, u: int, S: int) -> tuple[list[str], bool, bool]:
    """(problems, sample u shows a non-finite float, every result keeps the clean bits)"""
    problems: list[str] = []
    if [n for n, _ in clean] != [n for n, _ in got]:
        return [f"results differ in kind: {[n for n, _ in clean]} vs {[n for n, _ in got]}"], False, False
    outs, visible, same = unit.outs or {}, False, True
    for (name, c), (_, g) in zip(clean, got):
        spec = outs.get(name, 0)
        if spec == SKIP:
            continue
        if name in unit.ranges:
            lo, hi = unit.ranges[name]
            if g.numel() and not bool(((g >= lo) & (g < hi)).all()):
                bad = g[(g < lo) | (g >= hi)].flatten()[0].item()
                problems.append(f"{name}: {bad} lies outside [{lo}, {hi})")
        if c.shape != g.shape or c.dtype != g.dtype:
            problems.append(f"{name}: shape or dtype changed")
            same = False
            continue
        if not WC.same_bits(c, g):
            same = False
        if spec == SHARED:
            if not WC.same_bits(c, g):
                problems.append(f"{name}: a result no sample owns changed")
            continue
        ids = sample_ids(c.shape[spec], S, _lengths(unit, kw)).to(c.device)
        others, mine = (ids != u).nonzero().flatten(), (ids == u).nonzero().flatten()
        co, go = c.index_select(spec, others), g.index_select(spec, others)
        if not WC.same_bits(co, go):
            new = go.is_floating_point() and bool((~torch.isfinite(go.float()) & torch.isfinite(co.float())).any())
            problems.append(f"{name}: another sample " + ("holds a non-finite value the clean run did not" if new else "differs in a bit"))
        cm, gm = c.index_select(spec, mine), g.index_select(spec, mine)
        if unit.writes_neginf and cm.is_floating_point():
            if bool((cm.isnan() | (cm == INF)).any()):
                raise CaseProvesNothing(f"{name}: the clean run already holds NaN or +inf in sample {u}")
            visible = visible or bool((~torch.isfinite(gm.float()) & torch.isfinite(cm.float())).any())
            continue
        if not _finite(cm):
            raise CaseProvesNothing(f"{name}: the clean run is already non-finite in sample {u}")
        if not _finite(gm):
            visible = True
    return problems, visible, same


def check_isolation(run, operands: dict, unit: Unit, poison: str, *, swallows=False, clone=GC.clone_kw) -> list[str]:
    """``run(kw) -> [(name, tensor clone)]`` once on a clone of ``operands`` and once per operand of ``unit`` with one element of
    sample u poisoned; returns the problems found (an empty list: isolated, in range, visible).  A HIP error is GpuFault.
    ``swallows``: what ``swallowed(key)`` says - False, True (every operand) or the names of the operands whose NaN may end finite.
    A listed operand must need its entry: one whose NaN comes back visible is reported as stale; an operand that is not listed
    is held to visibility although its row is."""
    S = n_samples(unit, operands)
    u = unit_sample(S)
    problems: list[str] = []

    def call(kw, what):
        try:
            return run(kw)
        except Exception as e:  # noqa: BLE001
            if isinstance(e, WC.GpuFault) or WC.is_fault(e):
                raise WC.GpuFault(f"{what}: {e}") from e
            if isinstance(e, CaseProvesNothing):
                raise
            problems.append(f"{what}: raised {type(e).__name__}: {e}")
            return None

    clean = call(clone(operands), "clean run")
    if clean is None:
        return problems
    if not clean:
        raise CaseProvesNothing("the call returns nothing and writes nothing")
    for which, (path, dim, _) in enumerate(unit.operands):
        t = WC.get(operands, path)
        if not t.is_floating_point():
            raise CaseProvesNothing(f"{WC.path_name(path)} is no float operand")
        kw, idx = poisoned(clone(operands), unit, which, poison_value(poison, t.dtype), u, S, poison)
        where = f"{WC.path_name(path)}{list(idx)} = {poison}"
        got = call(kw, where)
        if got is None:
            continue
        found, visible, same = compare(unit, operands, clean, got, u, S)
        problems += [f"{where}: {p}" for p in found]
        if same:
            raise CaseProvesNothing(f"{where}: every result keeps the clean bits: the poisoned element is not read")
        listed = swallows is True or (swallows is not False and WC.path_name(path) in swallows)
        if poison == "nan" and not visible and not listed:
            problems.append(f"{where}: sample {u} comes back without a non-finite float: the NaN was swallowed")
        if poison == "nan" and visible and listed:
            problems.append(f"{where}: listed in SWALLOWS, but the NaN comes back visible: the entry is stale")
    return problems


def check_ignored(run, operands: dict, masks: dict, *, clone=GC.clone_kw) -> list[str]:
    """``masks``: operand name -> (kw) -> bool tensor of the elements the contract says are not read.  NaN in all of them must
    leave every result bit-identical to the clean run (an in-place operand is compared outside its own mask)."""
    problems: list[str] = []
    clean = run(clone(operands))
    for name, mask_of in masks.items():
        kw = clone(operands)
        mask = mask_of(kw).to(kw[name].device)
        if not bool(mask.any()):
            raise CaseProvesNothing(f"{name}: the ignored region is empty")
        kw[name][mask] = NAN
        try:
            got = run(kw)
        except Exception as e:  # noqa: BLE001
            if WC.is_fault(e):
                raise WC.GpuFault(f"{name}: {e}") from e
            problems.append(f"{name}: raised {type(e).__name__}: {e}")
            continue
        for (n, c), (_, g) in zip(clean, got):
            if n == name:
                c, g = c.masked_fill(mask, 0), g.masked_fill(mask, 0)
            if not WC.same_bits(c, g):
                problems.append(f"NaN in the ignored region of {name} changed {n}")
    return problems


def row_run(ops, r: WC.Row):
    return lambda kw: WC.snapshot(r, kw, WC.call(ops, r, kw))


# ------------------------------------------------------------------------------------------------------------------ the tables
def _at_argmax(name: str):
    """the column of sample u's first row that changes the choice: the row's maximum for NaN and -inf, its minimum for +inf and the
    largest finite value (which at the maximum's place would leave the winner the winner)"""
    def at(kw, rows, poison):
        r, row = int(rows[0]), kw[name][int(rows[0])].float()
        return (r, int(row.argmin() if poison in ("+inf", "max") else row.argmax()))
    return at


def _at_best_candidate(kw, rows, poison):
    block = kw["cand_score"][rows].float()
    i = int(block.flatten().argmin() if poison in ("+inf", "max") else block.flatten().argmax())
    return (int(rows[i // block.shape[1]]), i % block.shape[1])


def _at_positive_result(fn: str):
    """an element of a residual whose clean result is positive: behind a ReLU a poisoned residual is read visibly only there (the
    clean call itself says where; the first element where nothing is positive)"""
    def at(kw, rows, poison):
        from pytorch_models._hip import ops
        out = getattr(ops, fn)(**GC.clone_kw(kw))
        hit = (out[rows].float() > 0).nonzero()
        if not hit.numel() or out.shape != kw["resid"].shape:
            return (int(rows[0]),) + (0,) * (kw["resid"].dim() - 1)
        return (int(rows[int(hit[0, 0])]),) + tuple(int(i) for i in hit[0, 1:])
    return at


def _at_live_logit(kw, rows, poison):
    """a column of the row that pm_dec_whisper_rules leaves alone, a timestamp if there is one (a NaN there also reaches the
    timestamp-probability rule's sum); a suppressed column is overwritten with -inf whatever it held"""
    from oracle import ref_whisper_rules as RR

    r, P, n = int(rows[0]), kw["P"], int(kw["pos"]) + 1
    rules = RR.Rules(eot=kw["eot"], timestamp_begin=kw["timestamp_begin"], suppress=list(kw["suppress"]), blank=list(kw["blank"]))
    live = torch.isfinite(RR.apply(rules, kw["logits"][r].cpu(), kw["tokens"][r, P:n].tolist())).nonzero().flatten().tolist()
    ts = [c for c in live if c >= kw["timestamp_begin"]]
    return (r, (ts or live)[0])


_TAIL = {"pos": SHARED, "ticket": SHARED}
_TOK = {"tok_cur": (0, 11), "tokens": (0, 11)}

UNITS: dict[str, Unit] = {
    "ln_stats_finalize": U("partials"),
    "linear": U("x", "resid"),
    "linear:ln_fold": U("x", "ln_stats"),
    "linear_f32": U("x", "resid"),
    "attention_f32": U("q", "k", "v", "bias"),
    "layernorm": U("x", "resid"),
    "layernorm:plain": U("x"),
    "rmsnorm": U("x"),
    "geglu": U("h"),
    "attention": U("q", "k", "v", "bias"),
    "conv2d_nhwc": U("x", "resid"),
    "mean_rows": U("x"),
    "vit_tokens": U("imgs"),
    "linear_strided": U("x", "resid", samples=2),
    "w2v_stem0": U("x"),
    "group_windows": U("x"),
    "grouped_conv": U("xg", "resid", samples=2),
    "avgpool_time2": U("x"),
    "stft_mel": U("x"),
    "whisper_stem1": U("x"),
    "dec_linear": U("x", "resid"),
    "dec_linear_ksplit": U("x", "resid"),
    "dec_argmax": U("x", ranges={"output 0": (0, 200)}),
    "dec_attention": U("q", "k", "v"),
    "prefill_attention": U("qkv", "kc", "vc", samples=2),
    # row 1 starts at key 3 (dec) / key 2 (prefill): the keys in front of it are not read
    "dec_attention_ragged": U("q", ("k", 0, {2: 3}), ("v", 0, {2: 3})),
    "prefill_attention_ragged": U("qkv", ("kc", 0, {2: 2}), ("vc", 0, {2: 2}), samples=2),
    "dec_next_token": U(("ws_val", 0, _at_argmax("ws_val")), outs=_TAIL, ranges=_TOK),
    "dec_next_token:plain": U(("ws_val", 0, _at_argmax("ws_val")), outs=_TAIL, ranges=_TOK),
    "dec_sample_topk": U(("logits", 0, _at_argmax("logits")), outs=_TAIL, ranges=_TOK),
    "dec_sample_topk:plain": U(("logits", 0, _at_argmax("logits")), outs=_TAIL, ranges=_TOK),
    "dec_whisper_rules": U(("logits", 0, _at_live_logit), writes_neginf=True),
    # a sample is a clip: its W rows of logits, candidates, token histories and cache rows
    "dec_beam_topw": U("logits", "scores", samples=2, ranges={"output 1": (-1, 11)}),
    "dec_beam_select": U(("cand_score", 0, _at_best_candidate), samples=2, outs=_TAIL,
                         ranges={"parents": (0, 3), "tokens": (0, 11), "tok_cur": (0, 11)}),
    "dec_beam_reorder": U((("caches", 0), 0), (("caches", 1), 0), samples=2),
    "dwconv7_ln": U("x"),
    "ln_space_to_depth": U("x"),
    "convnext_stem": U("imgs"),
    "mean_ln": U("x"),
    "window_attention": U("q", "k", "v", samples=2),
    "dwconv3_bn_act": U("x", "gate"),
    "se_gate": U("psum"),
    "maxvit_stem": U("imgs"),
    "im2col3x3": U("x"),
    "avgpool2x2": U("x"),
    "conv_bf16": U("x", ("resid", 0, _at_positive_result("conv_bf16"))),
    "resnet_stem": U("imgs"),
    "attention_hd32": U("q", "k", "v"),
    "mixer_token_mix": U("x", "stats", samples=2),
    "row_stats": U("x"),
    "ln_mean": U("x", "stats", samples=2),
    "transpose_add_f32": U("x", "resid"),
    "conv1d_f32": U("x", "resid"),
    "lstm_f32": U("x"),
    "rvq_encode": U("z", outs={"output 0": 1}, ranges={"output 0": (0, 1024)}),
    "groupnorm1_": U("x", "resid"),
    "encodec_scale": U("x"),
    "scale_clips": U("x", "scale"),
    "cls_head_gemm": U("x"),
    "cls_attend": U("x", "stats", "u", samples=2),
    "lm_score": U("h", outs={"ws": SKIP}, ranges={"output 2": (0, 11), "argmax_out": (0, 11)}),
    "align_lse": U("q", "k"),
    "align_matrix": U("q", "k", "lse"),
    "align_dtw": U("m", outs={"ws": SKIP}, ranges={"output 0": (-1, 12), "out": (-1, 12)}),
    "attention_varlen": U("q", "k", "v", packed=True),
    "attention_varlen:plain": U("q", "k", "v", packed=True),
    "rows_pack": U("x", packed=True, samples=2),
    "rows_unpack": U("x", packed=True),
    "rows_zero_tail": U("x"),
    "segment_mean": U("x", packed=True),
    "ctc_head": U("h", ranges={"output 1": (0, 7), "best_out": (0, 7)}),
    "ctc_greedy": U("best_logp", packed=True, ranges={"output 0": (-1, 7), "output 1": (0, 7), "output 2": (-1, 6)}),
    "ctc_forward": U("logp", packed=True),
    "ctc_viterbi": U("logp", packed=True, outs={"ws": SKIP}, ranges={"output 0": (-1, 5), "output 1": (-1, 6)}),
}

_TABLES = "its float operands are tables every sample shares (emb, pos): a NaN in one poisons every sample that looks it up, by definition"
NO_UNITS: dict[str, str] = {
    "embed_tokens": _TABLES,
    "embed_tokens:f32_table": _TABLES,
    "embed_tokens_ragged": _TABLES,
    "dec_embed_ragged": _TABLES,
    "embed_tokens_varlen": _TABLES,
    "rvq_decode": "codes are integers; the codebooks are tables every sample shares",
}

_RELU = ("ends in ReLU = fmaxf(x, 0) (%s), an IEEE maxNum clamp: fmaxf(NaN, 0) = 0 where torch.relu(NaN) = NaN - the hot epilogues "
         "keep the one-instruction form")
_NO_FLOAT = "no float result depends on the operand (%s): visibility is the range of its integer results"
SWALLOWS_CLAMP: dict[str, str] = {
    "linear_f32": _RELU % "csrc/common.h:177, act = relu in the canonical row",
    "conv_bf16": _RELU % "csrc/resnet.hip:222, after the residual add",
    "resnet_stem": _RELU % "csrc/resnet.hip:276, then the 3 x 3 max-pool of csrc/resnet.hip:305, fmaxf again",
    "stft_mel": "the log-mel floor max(x, peak - 8) is fmaxf (csrc/logmel.hip:160) and the peak is a running fmaxf (csrc/logmel.hip:143): "
                "a NaN frame is floored like a silent one, where torch.maximum would keep the NaN",
    "DETR": _RELU % "the ResNet backbone: csrc/resnet.hip:276 / 222",
    "WhisperPreprocessor": "the log-mel floor of stft_mel, fmaxf (csrc/logmel.hip:160)",
}
SWALLOWS_NO_FLOAT: dict[str, str] = {
    "dec_sample_topk": _NO_FLOAT % "x is an embedding row of a valid id",
    "dec_sample_topk:plain": _NO_FLOAT % "x is an embedding row of a valid id",
    "rvq_encode": _NO_FLOAT % "int64 codes only",
    "align_dtw": _NO_FLOAT % "int32 frames only",
    "EnCodec.encode": _NO_FLOAT % "int64 codes; the scale is None",
    "Whisper.align": _NO_FLOAT % "int32 encoder positions only",
}
SWALLOWS: dict[str, str] = {**SWALLOWS_CLAMP, **SWALLOWS_NO_FLOAT}
# A clamp swallows the operands in front of it only: linear_f32 adds its residual BEHIND the ReLU, conv_bf16 in front of it.
SWALLOWED_OPERANDS: dict[str, tuple] = {"linear_f32": ("x",), "conv_bf16": ("x", "resid")}


def swallowed(key: str):
    """False (not listed), the names of the listed operands, or True (every operand of the call)"""
    return SWALLOWED_OPERANDS.get(key, True) if key in SWALLOWS else False


def _rows_from(name: str, dim: int, first: Callable):
    """rows >= first(kw)[b] along ``dim`` of sample b (dimension 0)"""
    def mask(kw):
        t = kw[name]
        lo = torch.as_tensor(first(kw)).view(-1, *([1] * (t.dim() - 1)))
        shape = [1] * t.dim()
        shape[dim] = t.shape[dim]
        return (torch.arange(t.shape[dim]).view(shape) >= lo).expand(t.shape).clone()
    return mask


def _seq_len(kw):
    return list(kw["seq"].lengths)


def _same(n):
    return lambda kw: [n(kw)] * kw[next(k for k in ("k", "kc") if k in kw)].shape[0]


# operand -> the elements the documented contract says are not read (DESIGN.md sections 18, 19, 21, 22)
IGNORED: dict[str, dict] = {
    "rows_pack": {"x": _rows_from("x", 1, _seq_len)},          # section 22: "padded rows are not read"
    "rows_zero_tail": {"x": _rows_from("x", 1, _seq_len)},     # section 22: rows past the length are overwritten with zeros
    "dec_attention": {"k": _rows_from("k", 2, _same(lambda kw: kw["lk"])), "v": _rows_from("v", 2, _same(lambda kw: kw["lk"]))},
    "dec_attention_ragged": {"k": _rows_from("k", 2, _same(lambda kw: kw["lk"])), "v": _rows_from("v", 2, _same(lambda kw: kw["lk"]))},
    # section 18: the chunk attends over the caches' keys < p0 and its own rows, and writes [p0, p0 + C) only
    "prefill_attention": {"kc": _rows_from("kc", 2, _same(lambda kw: kw["p0"] + kw["qkv"].shape[0] // kw["kc"].shape[0])),
                          "vc": _rows_from("vc", 2, _same(lambda kw: kw["p0"] + kw["qkv"].shape[0] // kw["kc"].shape[0]))},
    "prefill_attention_ragged": {"kc": _rows_from("kc", 2, _same(lambda kw: kw["p0"] + kw["qkv"].shape[0] // kw["kc"].shape[0])),
                                 "vc": _rows_from("vc", 2, _same(lambda kw: kw["p0"] + kw["qkv"].shape[0] // kw["kc"].shape[0]))},
    # section 21: "entries with t >= len_b or f >= F_b are exactly 0": token rows past the length, frames past the clip's
    "align_lse": {"q": _rows_from("q", 1, lambda kw: kw["lengths"].tolist()), "k": _rows_from("k", 1, lambda kw: kw["frames"].tolist())},
    "align_matrix": {"q": _rows_from("q", 1, lambda kw: kw["lengths"].tolist()), "k": _rows_from("k", 1, lambda kw: kw["frames"].tolist())},
    "align_dtw": {"m": lambda kw: _rows_from("m", 1, lambda k: k["lengths"].tolist())(kw) | _rows_from("m", 2, lambda k: k["frames"].tolist())(kw)},
}


# Pad columns up to a leading dimension: row -> the operands whose canonical tensor is re-laid as wrapper_cases' "rowpad" variant
# (the values in the first K columns of a (..., K + 8) parent whose other elements are NaN).  The wrapper
# must accept the layout, and every result must keep the bits of the packed call.
PAD_COLUMNS: dict[str, tuple] = {
    "linear": ("x", "resid"), "linear_f32": ("x", "resid"), "layernorm": ("x", "resid"), "attention": ("q", "k", "v"),
    "dec_linear": ("x", "resid"), "lm_score": ("h",), "ctc_head": ("h",), "ctc_forward": ("logp",), "ctc_viterbi": ("logp",),
    "align_lse": ("q", "k"), "align_dtw": ("m",),
}


def check_pad_columns(run, operands: dict, names, *, clone=GC.clone_kw) -> list[str]:
    problems: list[str] = []
    clean = run(clone(operands))
    for name in names:
        v = next(v for v in WC.variants(operands[name].clone()) if v.tag == "rowpad")
        assert bool(v.parent.isnan().any())
        try:
            got = run(WC.replaced(clone(operands), (name,), v.tensor))
        except Exception as e:  # noqa: BLE001
            if WC.is_fault(e):
                raise WC.GpuFault(f"{name}: {e}") from e
            problems.append(f"{name}: the padded layout raised {type(e).__name__}: {e}")
            continue
        problems += [f"NaN in the pad columns of {name} changed {n}" for (n, c), (_, g) in zip(clean, got) if not WC.same_bits(c, g)]
    return problems


# ---------------------------------------------------------------------------------------------------------------- decisions
FAMILIES = ("all_nan", "all_neginf", "nan_first", "nan_last", "nan_tile_edge", "two_posinf", "all_equal")
SIZES = (5, 1000, 51865)  # below a tile, no multiple of a tile, Whisper's vocabulary
TILE = 64
ROWS_B, ROW_U = 4, 1  # a batch of four rows, the second one is the family's


def tile_edge(V: int) -> int:
    return TILE if V > TILE else V // 2


def two_columns(V: int) -> tuple[int, int]:
    return (V // 3, V - 2) if V > 2 * TILE else (1, V - 1)  # in different tiles wherever the row has two


def family_row(family: str, V: int, base: Tensor) -> Tensor:
    """the family's row: ``base`` (V Gaussian values) with the family's pattern"""
    row = base.clone()
    if family == "all_nan":
        row[:] = NAN
    elif family == "all_neginf":
        row[:] = -INF
    elif family == "nan_first":
        row[0] = NAN
    elif family == "nan_last":
        row[V - 1] = NAN
    elif family == "nan_tile_edge":
        row[tile_edge(V)] = NAN
    elif family == "two_posinf":
        a, b = two_columns(V)
        row[a] = row[b] = INF
    elif family == "all_equal":
        row[:] = 0.5
    elif family == "one_finite":  # (beam only: fewer comparable logits than beams)
        keep = row[1].clone()
        row[:] = NAN
        row[1] = keep
    else:
        raise KeyError(family)
    return row


def gaussian_rows(V: int, B: int = ROWS_B, seed: int = 2911) -> Tensor:
    g = torch.Generator().manual_seed(seed + V)
    return torch.randn((B, V), generator=g)


def family_rows(family: str, V: int, B: int = ROWS_B, u: int = ROW_U) -> tuple[Tensor, Tensor]:
    """(clean rows, the same rows with row u the family's)"""
    clean = gaussian_rows(V, B)
    rows = clean.clone()
    rows[u] = family_row(family, V, clean[u])
    return clean, rows


def lowest_argmax(row: Tensor) -> int:
    """the contract's decision for a row without NaN: torch.argmax, the lowest index on ties (0 for a row of -inf)"""
    assert not bool(row.isnan().any())
    return int(torch.argmax(row))


def top_order(row: Tensor, k: int) -> list[int]:
    """the first k indices in (value descending, index ascending): torch's stable sort, which is torch.topk's order without its
    freedom on ties"""
    assert not bool(row.isnan().any())
    return torch.sort(row, descending=True, stable=True).indices[:k].tolist()


def tile_winners(rows: Tensor, tile: int = TILE) -> tuple[Tensor, Tensor]:
    """what the arg-max tiles of the vocabulary projection publish for logits ``rows``: per tile the maximum and its lowest index,
    found by strict ``>`` from (-inf, none) - so a tile of -inf or NaN only publishes (-inf, NONE_IDX), and a NaN is skipped"""
    B, V = rows.shape
    nt = (V + tile - 1) // tile
    pad = torch.full((B, nt * tile), -INF)
    pad[:, :V] = torch.where(rows.isnan(), torch.tensor(-INF), rows)
    val, idx = pad.view(B, nt, tile).max(-1)
    first = (pad.view(B, nt, tile) == val[..., None]).float().argmax(-1)  # the lowest index of the maximum
    idx = first + torch.arange(nt) * tile
    idx = torch.where(val == -INF, torch.tensor(NONE_IDX), idx)
    return val.contiguous(), idx.to(I32).contiguous()


def gemm_rows(family: str, V: int, K: int = 16, B: int = ROWS_B, u: int = ROW_U) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(h clean, h, w, the logits h @ w.T holds) for the entry points that compute their rows: row b of h is the unit vector e_b and
    column b of w the row's values, all exact in bf16.  A weight is shared, so 0 x NaN would reach every row: the family's row can
    only be made through h - NaN everywhere (all_nan), +inf x (a column of -1, +1 or 0) for rows of -inf, +inf and NaN; all_equal
    is the zero vector.  'One NaN among finite values' cannot exist behind a GEMM: the NaN sits among -inf."""
    clean = gaussian_rows(V, B).to(BF).float()
    w = torch.zeros(V, K)
    w[:, :B] = clean.t()
    h0 = torch.zeros(B, K)
    h0[torch.arange(B), torch.arange(B)] = 1.0
    h, rows = h0.clone(), clean.clone()
    if family == "all_nan":
        h[u] = NAN
        rows[u] = NAN
    elif family == "all_equal":
        h[u] = 0.0
        rows[u] = 0.0
    else:
        sign = torch.full((V,), -1.0)
        if family == "two_posinf":
            a, b = two_columns(V)
            sign[a] = sign[b] = 1.0
        elif family != "all_neginf":
            sign[{"nan_first": 0, "nan_last": V - 1, "nan_tile_edge": tile_edge(V)}[family]] = 0.0
        w[:, u] = sign
        h[u, u] = INF
        rows[u] = torch.where(sign == 0, torch.tensor(NAN), sign * INF)
    return h0.to(BF), h.to(BF), w.to(BF), rows


@dataclass
class Decision:
    """``run(dev, family, V, clean: bool) -> (ints, floats, rows)``: ints name -> (tensor, lo, hi), floats name -> tensor, every
    tensor with the rows (or their groups: an extent that divides the row count) along dimension 0; rows = the CPU rows the call
    decided over; ``pick``: (ints, row index) -> the decision as a list of ints, ``ref``: (row) -> the list wanted or a set the
    single pick must lie in - checked for a family row without NaN; ``rows_b``: how many rows the call holds; ``distinct``: integer
    results whose every row must hold pairwise different values (a row's beam candidates)"""
    id: str
    run: Callable
    sizes: tuple = SIZES
    families: tuple = FAMILIES
    pick: Callable | None = None
    ref: Callable | None = None
    rows_b: int = ROWS_B
    row_u: int = ROW_U
    distinct: tuple = ()


def check_decision(d: Decision, dev, family: str, V: int) -> list[str]:
    problems: list[str] = []
    ints0, floats0, _ = d.run(dev, family, V, True)
    ints, floats, rows = d.run(dev, family, V, False)
    B, u = d.rows_b, d.row_u
    row = rows[u]
    has_nan = bool(row.isnan().any())
    for name, (t, lo, hi) in ints.items():
        if not bool(((t >= lo) & (t < hi)).all()):
            problems.append(f"{name}: {t[(t < lo) | (t >= hi)].flatten()[0].item()} lies outside [{lo}, {hi})")
        if name in d.distinct and any(len(set(r.tolist())) != r.numel() for r in t):
            problems.append(f"{name}: a row repeats a value: {t.tolist()}")
    for name, t in list(floats.items()) + [(n, v[0]) for n, v in ints.items()]:
        t0 = floats0[name] if name in floats0 else ints0[name][0]
        g = u * t.shape[0] // B  # the row's group
        keep = [i for i in range(t.shape[0]) if i != g]
        if not WC.same_bits(t[keep], t0[keep]):
            problems.append(f"{name}: another row differs from the clean run")
        if has_nan and name in floats and bool(torch.isfinite(t[g]).all()):
            problems.append(f"{name}: the row holds a NaN and its {name} is finite: {t[g].flatten().tolist()[:4]}")
    if not has_nan and d.ref is not None:
        want, got = d.ref(row), d.pick(ints, u)
        if isinstance(want, set):
            if not set(got) <= want:
                problems.append(f"decision {got} outside {sorted(want)[:8]}")
        elif list(got) != list(want):
            problems.append(f"decision {got}, torch gives {want}")
    return problems


def _tail_state(dev, B: int, V: int):
    g = WC.Gen(dev, 2911)
    return dict(pos=g.t([3], I32), prompt=g.i(V, B, 2), tok_cur=g.i(V, B), tokens=g.i(V, B, 8), emb=g.b(V, 32), pos_tab=g.f(9, 32),
                ticket=g.t([0], I32))


def _rows_for(family, V, clean, B=ROWS_B, u=ROW_U):
    c, r = family_rows(family, V, B, u)
    return c if clean else r


def published(rows: Tensor) -> tuple[Tensor, Tensor]:
    """``rows`` as the per-tile (maximum, index) workspace of the arg-max tiles, tile t's winner being token t: a tile without a
    maximum (-inf, or NaN here) carries no index, as tile_winners shows"""
    idx = torch.arange(rows.shape[1]).expand(rows.shape)
    idx = torch.where(rows.isnan() | (rows == -INF), torch.tensor(NONE_IDX), idx)
    return rows.contiguous(), idx.to(I32).contiguous()


def _run_next_token(ragged: bool):
    """the family's row is a row of the tile maxima the tail reduces (the vocabulary projection writes no NaN there: its tiles
    skip one - and a row of operands with a NaN is a row of NaN logits, the all_nan family)"""
    def run(dev, family, V, clean):
        from pytorch_models._hip import ops
        rows = _rows_for(family, V, clean)
        val, idx = published(rows)
        st = _tail_state(dev, ROWS_B, V)
        margins = torch.zeros(ROWS_B, 8, device=dev)
        extra = dict(key_start=torch.tensor([0, 1, 0, 2], dtype=I32, device=dev)) if ragged else {}
        ops.dec_next_token(val.to(dev), idx.to(dev), margins=margins, **st, **extra)
        return ({"tok_cur": (st["tok_cur"].cpu(), 0, V), "tokens": (st["tokens"].cpu(), 0, V)},
                {"margin": margins[:, 4].cpu()}, rows)
    return run


def _run_sample_topk(ragged: bool):
    def run(dev, family, V, clean):
        from pytorch_models._hip import ops
        rows = _rows_for(family, V, clean)
        st = _tail_state(dev, ROWS_B, V)
        extra = dict(key_start=torch.tensor([0, 1, 0, 2], dtype=I32, device=dev)) if ragged else {}
        ops.dec_sample_topk(rows.to(dev), 3, 5, **st, **extra)
        return {"tok_cur": (st["tok_cur"].cpu(), 0, V), "tokens": (st["tokens"].cpu(), 0, V)}, {}, rows
    return run


def _run_sample(topk: int, temperature: float, top_p: float):
    def run(dev, family, V, clean):
        from pytorch_models._hip import sampling
        rows = _rows_for(family, V, clean)
        st = _tail_state(dev, ROWS_B, V)
        lp = torch.zeros(ROWS_B, 8, device=dev)
        sampling.dec_sample(rows.to(dev), **st, topk=topk, temperature=temperature, top_p=top_p, seed=7, logprobs=lp)
        return {"tok_cur": (st["tok_cur"].cpu(), 0, V), "tokens": (st["tokens"].cpu(), 0, V)}, {"logprob": lp[:, 4].cpu()}, rows
    return run


def _survivors(k: int):
    def ref(row):
        if k:
            return set(top_order(row, min(k, row.numel())))
        live = (row > -INF).nonzero().flatten().tolist()
        return set(live or range(row.numel()))
    return ref


BEAM_W, BEAM_CLIPS = 2, 3


def _run_beam(dev, family, V, clean):
    from pytorch_models._hip import ops
    W, B = BEAM_W, BEAM_CLIPS
    rows = _rows_for(family, V, clean, B * W, 2)  # row 2 = clip 1, beam 0
    g = WC.Gen(dev, 2917)
    scores, finished, pos = g.f(B, W), g.z(B, W, dtype=I32), g.t([3], I32)
    cs, ct = ops.dec_beam_topw(rows.to(dev), scores, finished, pos, 2, None)
    st = _tail_state(dev, B * W, V)
    state = dict(scores=scores.clone(), finished=finished, parents=g.z(B, W, dtype=I32), x=g.z(B * W, 32))
    ops.dec_beam_select(cs, ct, tokens=st["tokens"], pos=pos, prompt=st["prompt"], tok_cur=st["tok_cur"], emb=st["emb"],
                        pos_tab=st["pos_tab"], ticket=st["ticket"], eos=None, **state)
    ints = {"cand_tok": (ct.cpu(), 0, V), "parents": (state["parents"].cpu(), 0, W), "tok_cur": (st["tok_cur"].cpu().view(B, W), 0, V),
            "tokens": (st["tokens"].cpu().view(B, W * 8), 0, V)}
    return ints, {"cand_score": cs.cpu()}, rows


def _run_t5_tail(dev, family, V, clean):
    from pytorch_models._hip import check, lib
    rows = _rows_for(family, V, clean)
    val, idx = published(rows)
    val, idx = val.to(dev), idx.to(dev)
    g = WC.Gen(dev, 2919)
    B, P, Ttot, d = ROWS_B, 2, 8, 32
    E, prompt, tokens = g.b(V, d), g.i(V, B, P), g.i(V, B, Ttot)
    pos, ticket, finished = g.t([3], I32), g.t([0], I32), g.z(B, dtype=I32)
    out_len, x = torch.full((B,), Ttot, dtype=I64, device=dev), g.z(B, d)
    check(lib().pm_t5_dec_next_token(val.data_ptr(), idx.data_ptr(), val.shape[1], pos.data_ptr(), prompt.data_ptr(), P, tokens.data_ptr(),
                                     Ttot, 0, -1, finished.data_ptr(), out_len.data_ptr(), E.data_ptr(), x.data_ptr(), d, V,
                                     ticket.data_ptr(), None, None, B, torch.cuda.current_stream().cuda_stream), "pm_t5_dec_next_token")
    return {"tokens": (tokens.cpu(), 0, V)}, {}, rows


def _run_dec_argmax(dev, family, V, clean):
    """the arg-max tiles of the vocabulary projection themselves.  LayerNorm stands in front of them, so one operand row shapes
    one family only: a NaN (or an infinity) anywhere in the row makes every logit of it NaN"""
    from pytorch_models._hip import ops
    g = WC.Gen(dev, 2933)
    x, w, ln = g.f(ROWS_B, 64), g.b(V, 64, scale=0.1), (g.f(64), g.f(64), 1e-5)
    if not clean:
        x[ROW_U] = NAN
    idx, mx = ops.dec_argmax(x, w, ln)
    rows = torch.zeros(ROWS_B, V)
    if not clean:
        rows[ROW_U] = NAN
    return {"argmax": (idx.cpu(), 0, V)}, {"max": mx.cpu()}, rows


def _run_ctc_head(dev, family, V, clean):
    from pytorch_models._hip import ops
    h0, h, w, rows = gemm_rows(family, V)
    out, best, blp = ops.ctc_head((h0 if clean else h).to(dev), w.to(dev))
    return {"best": (best.cpu(), 0, V)}, {"best_logp": blp.cpu(), "logp": out.cpu()}, rows


def _run_lm_score(dev, family, V, clean):
    from pytorch_models._hip import ops
    h0, h, w, rows = gemm_rows(family, V)
    targets = torch.tensor([1, 2, 3, 4], device=dev) % V
    lp, lse, am = ops.lm_score((h0 if clean else h).to(dev), w.to(dev), targets, want_lse=True, want_argmax=True)
    return {"argmax": (am.cpu(), 0, V)}, {"logprob": lp.cpu(), "lse": lse.cpu()}, rows


def _run_ctc_greedy(dev, family, V, clean):
    """one frame per clip: best / best_logp as pm_ctc_head_bf16 hands them on (a NaN row: index 0, NaN)"""
    from pytorch_models._hip import ops
    rows = _rows_for(family, V, clean)
    best = torch.tensor([0 if bool(r.isnan().any()) else lowest_argmax(r) for r in rows], dtype=I32)
    blp = rows.max(-1).values - torch.logsumexp(rows, -1)
    ids, n, start, path = ops.ctc_greedy(best.to(dev), ops.seq_lens([1] * ROWS_B, 2, dev), blp.to(dev), blank=0)
    return {"ids": (ids.cpu(), -1, V), "n": (n.cpu(), 0, 3), "start": (start.cpu(), -1, 2)}, {"path_logp": path.cpu()}, rows


def _run_ctc_viterbi(dev, family, V, clean):
    """three frames per clip, the family's row in the middle; one target label, the column at the tile edge (the recursion gathers the
    blank's and the labels' columns only: a NaN in the last column is not read, so that family is left out)"""
    from pytorch_models._hip import ops
    rows = _rows_for(family, V, clean)
    around = torch.log_softmax(gaussian_rows(V, 2 * ROWS_B, seed=2923), -1).view(ROWS_B, 2, V)
    logp = torch.stack([around[:, 0], rows, around[:, 1]], 1).reshape(3 * ROWS_B, V).contiguous()
    targets = torch.full((ROWS_B, 1), tile_edge(V), dtype=I32, device=dev)
    start, stop, score = ops.ctc_viterbi(logp.to(dev), ops.seq_lens([3] * ROWS_B, 3, dev), targets, torch.ones(ROWS_B, dtype=I32, device=dev))
    return {"start": (start.cpu(), -1, 3), "stop": (stop.cpu(), -1, 4)}, {"score": score.cpu()}, rows


def _run_align_dtw(dev, family, V, clean):
    """clips of four token rows over V frames, the family's row second"""
    from pytorch_models._hip import ops
    rows = _rows_for(family, V, clean)
    m = gaussian_rows(V, 4 * ROWS_B, seed=2927).view(ROWS_B, 4, V).clone()
    m[:, 1] = rows
    out = ops.align_dtw(m.to(dev), torch.full((ROWS_B,), 4, dtype=I32, device=dev), torch.full((ROWS_B,), V, dtype=I32, device=dev))
    return {"start": (out.cpu(), -1, V)}, {}, rows


def _run_rvq(dev, family, V, clean):
    from pytorch_models._hip import ops
    g = WC.Gen(dev, 2929)
    cb = g.f(2, 1024, 128)
    rows = _rows_for(family, 128, clean)
    codes = ops.rvq_encode(rows.to(dev), cb, (cb * cb).sum(-1).contiguous(), 2)
    return {"codes": (codes.t().contiguous().cpu(), 0, 1024)}, {}, rows


_ONE = lambda name: (lambda ints, u: [int(ints[name][0][u])])  # noqa: E731
_ARG = lambda row: [lowest_argmax(row)]  # noqa: E731
_ROWS = ("all_nan", "nan_first", "nan_last", "nan_tile_edge", "all_equal")  # what a row of operands (not of scores) can hold

DECISIONS: dict[str, Decision] = {d.id: d for d in (
    Decision("dec_argmax", _run_dec_argmax, families=("all_nan",)),  # the other families: dec_next_token, over the tiles' workspace
    Decision("dec_next_token", _run_next_token(False), pick=_ONE("tok_cur"), ref=_ARG),
    Decision("dec_next_token:ragged", _run_next_token(True), pick=_ONE("tok_cur"), ref=_ARG),
    Decision("dec_sample_topk", _run_sample_topk(False), pick=_ONE("tok_cur"), ref=_survivors(3)),
    Decision("dec_sample_topk:ragged", _run_sample_topk(True), pick=_ONE("tok_cur"), ref=_survivors(3)),
    Decision("dec_sample:k0", _run_sample(0, 0.7, 0.9), pick=_ONE("tok_cur"), ref=_survivors(0)),
    Decision("dec_sample:k3", _run_sample(3, 0.7, 0.9), pick=_ONE("tok_cur"), ref=_survivors(3)),
    Decision("dec_sample:T0", _run_sample(0, 0.0, 1.0), pick=_ONE("tok_cur"), ref=_ARG),
    Decision("dec_beam", _run_beam, pick=lambda ints, u: ints["cand_tok"][0][u].tolist(), ref=lambda row: top_order(row, BEAM_W),
             rows_b=BEAM_W * BEAM_CLIPS, row_u=2, families=FAMILIES + ("one_finite",), distinct=("cand_tok",)),
    Decision("t5_next_token", _run_t5_tail, pick=lambda ints, u: [int(ints["tokens"][0][u, 4])], ref=_ARG),
    # pm_ctc_head_bf16 serves 2 <= V <= 256 (ops.CTC_MAX_VOCAB: its rows of the weight stay in LDS): 200 is its "no multiple of a tile"
    Decision("ctc_head", _run_ctc_head, sizes=(5, 200), pick=_ONE("best"), ref=_ARG),
    Decision("ctc_greedy", _run_ctc_greedy, sizes=(5, 1000)),
    Decision("ctc_viterbi", _run_ctc_viterbi, sizes=(5, 1000), families=tuple(f for f in FAMILIES if f != "nan_last")),
    Decision("lm_score", _run_lm_score, pick=_ONE("argmax"), ref=_ARG),
    Decision("rvq_encode", _run_rvq, sizes=(128,), families=_ROWS),
    Decision("align_dtw", _run_align_dtw, sizes=(5, 1000)),
)}


# -------------------------------------------------------------------------------------------------------------------- models
@dataclass
class ModelPoison:
    """``input``: the index of the float input that is poisoned at sample 1 of the first batch-3 geometry (batch 2 where the
    family's inputs have none), element 0 of the sample; or ``why``: no input can be.  ``ranges``: output name -> (lo, hi)."""
    input: int | None = None
    why: str = ""
    ranges: dict = field(default_factory=dict)


_INTS = "its inputs are token ids: integers only"
MODELS_POISON: dict[str, ModelPoison] = {
    **{k: ModelPoison(0) for k in ("ViT", "MLPMixer", "MLPMixer:warmup1", "ConvNeXt", "MaxViT", "MobileViT", "DETR", "Wav2Vec2",
                                   "Wav2Vec2:hubert", "Data2VecAudio", "SEW", "Wav2Vec2CTC", "EnCodecEncoder", "EnCodecDecoder",
                                   "WhisperPreprocessor", "WhisperEncoder", "Whisper", "T5Encoder", "T5Decoder")},
    "EnCodec.encode": ModelPoison(0, ranges={"output 0": (0, 1024)}),
    "EnCodec.decode": ModelPoison(why="its input is the int64 codes"),
    "WhisperDecoder": ModelPoison(1),  # the encoder memory
    "BERT": ModelPoison(why=_INTS), "GPT": ModelPoison(why=_INTS), "GPT2": ModelPoison(why=_INTS), "T5Model": ModelPoison(why=_INTS),
}


def model_geometry(case: GC.Model) -> int:
    """the first geometry of the family with a batch of three, else the captured one (batch 2)"""
    for k in (1, 2, 0):
        if case.inputs(k, 0)[0].shape[0] == 3:
            return k
    return 0


def model_unit(mp: ModelPoison) -> Unit:
    return U((f"x{mp.input}", 0), ranges=mp.ranges)


def model_run(module):
    return lambda kw: [(n, t.clone()) for n, t in GC.flat(module(*kw.values()))]


# The decoding entry points README.md names, beside the forwards of MODELS: which float input is poisoned at sample 1 of a batch
# of three, or why none can be.  The runners live in tests/test_hip_nonfinite_models.py.  A generating entry point stops when every
# row has finished and a poisoned row may never emit eos: no eos is set, so every healthy row is compared over its whole length.
ENTRY_POINTS: dict[str, ModelPoison] = {
    "WhisperDecoder.generate:greedy": ModelPoison(0),   # the encoder memory; ids and, with return_logprobs, their log-probs
    "WhisperDecoder.generate:sampled": ModelPoison(0),
    "WhisperDecoder.generate:beam": ModelPoison(0),
    "Whisper.generate": ModelPoison(0),                 # the log-mel
    "Whisper.align": ModelPoison(0),
    "Wav2Vec2CTC.decode": ModelPoison(0),               # the waveform
    "Wav2Vec2CTC.score": ModelPoison(0),
    "Wav2Vec2CTC.align": ModelPoison(0),
    "T5Model.generate": ModelPoison(why=_INTS),
    "GPT2.generate": ModelPoison(why=_INTS + "; it takes no float memory"),
}
