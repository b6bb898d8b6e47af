"""Aliasing contract: for every row of wrapper_cases.ROWS, every operand W the call writes (the row's
``inplace`` list, list operands entry by entry) against every other tensor operand T of the same call, placed so that they share
memory.  Two outcomes only: the call raises ValueError naming the wrapper and both operands before the first launch and leaves
every written operand alone, or - for the pairs of ALIAS_OK, as the same view, and for disjoint column ranges of one parent - its
results are bit-identical to the same call with T cloned first.  tests/test_alias_cases_cpu.py (no GPU: the recording stub) and
tests/test_hip_aliasing.py (the kernels; it launches only what the CPU audit saw accepted).

The placements (``tags_for``):
  same     T is W's view where dtype, shape and strides agree, else T is based at W's first byte;
  head     T starts inside W, at the smallest multiple of 256 bytes that is at least one row of W and less than W's extent
           (skipped when W spans 256 bytes or less);
  tail     W starts inside T, by the same rule with the roles swapped;
  columns  2-D unit-last-stride operands only: W and T are disjoint column ranges of one parent.
W and T are views into ONE arena of POISON32 words (NaN as bf16 and as f32, absurd as an integer) with room on both sides for
the canonical numel at the widest dtype, so nothing is ever out of bounds; every offset is a multiple of 256 bytes, so every
alignment the canonical operand has survives and a PM_EALIGN refusal cannot pass for an aliasing refusal."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import Callable

import torch
from torch import Tensor

import wrapper_cases as WC

TAGS = ("same", "head", "tail", "columns")
STEP = 256


@dataclass
class Ok:
    cond: Callable      # kw -> bool: the scalar arguments under which the pair is honoured
    cond_text: str
    broken: dict        # keyword overrides that break the condition (the call must then be refused)
    code: str           # the kernel file and lines that make the pair safe
    why: str


# (wrapper, written operand, other operand) -> the pairs a call may pass as the SAME view.  Each: the region of T that overlaps an
# output region is read only by the workgroup that writes that region, before its first store there.
ALIAS_OK: dict[tuple[str, str, str], Ok] = {
    ("linear", "out", "resid"): Ok(
        lambda kw: kw.get("resid_period", 0) == 0, "resid_period == 0 (and no PM_GEMM_HYBRID / PM_GEMM_STREAMK / PM_GEMM_KERNEL=4|5)",
        dict(resid_period=16),
        "csrc/linear_bf16.hip:171-198 (128 x 128), :320-335 + :437-461 and :466-487 (256 x 128); csrc/linear_bf16_wide.hip:196-250; "
        "csrc/linear_bf16_tile.hip:163-196 + :388-445",
        "every kernel linear_plan can return (ids 1, 2, 3, 6 and 7 of the product build; the K-cut ids 4 / 5 exist in experiment builds "
        "only and the wrapper refuses the alias while their switches are on) adds the residual in the epilogue of the workgroup that owns the "
        "output tile: a residual element is loaded by the wave that stores the same (row, column), and the value reaches the store "
        "through registers (128 x 128, the unstaged 256 x 128 path: the same thread, the load in front of its store) or through the "
        "wave's own LDS staging, which the whole wave has waited for (s_waitcnt on the residual loads) before any lane stores the "
        "block.  Lanes past M or N load a clamped address of the same tile row and discard the value.  A periodic residual row is "
        "read by every tile of period-many rows: refused."),
    ("mixer_token_mix", "out", "x"): Ok(
        lambda kw: True, "always", {},
        "csrc/mixer.hip:146-172 (phase 0 + barrier), :212-222 and :252-253 (phase 2)",
        "workgroup (image n, channel slab c0) reads only its own slab of x: phase 0 stages it in LDS and ends in __syncthreads; in "
        "phase 2 each thread loads the 2 x 8 residual channels of its own token row in front of the strip's MFMAs and is the only "
        "one to store them.  A lane without a live row loads row 0 of the slab and discards it."),
}


def is_control(name: str, t: Tensor) -> bool:
    """an addressing or control operand: any integer tensor (ids, positions, lengths, parents, flags, targets, offsets), a ticket
    or counter, a caller-supplied workspace"""
    return not t.dtype.is_floating_point or name.split("[")[0] in ("ws", "ticket")


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(kw: dict):
    """wrapper_cases.operands plus the cu_seqlens tensor inside a SeqLens (an addressing operand like any other)"""
    yield from WC.operands(kw)
    if hasattr(kw.get("seq"), "cu"):
        yield ("seq", "cu"), kw["seq"].cu


def path_name(path) -> str:
    return "seq.cu" if path == ("seq", "cu") else WC.path_name(path)


def get(kw: dict, path) -> Tensor:
    return kw["seq"].cu if path == ("seq", "cu") else WC.get(kw, path)


def replaced(kw: dict, path, t: Tensor) -> dict:
    if path != ("seq", "cu"):
        return WC.replaced(kw, path, t)
    kw, s = dict(kw), kw["seq"]
    kw["seq"] = type(s)(list(s.lengths), t, s.L)
    return kw


def written_paths(r: WC.Row, kw: dict) -> list:
    return [p for p, _ in operands(kw) if p[0] in r.inplace]


# -------------------------------------------------------------------------------------------------------------- placements
def _extent(t: Tensor) -> int:
    """bytes from the first to one past the last element of a contiguous canonical operand"""
    return t.numel() * t.element_size()


def _row_bytes(t: Tensor) -> int:
    return (t.shape[-1] if t.dim() >= 2 else 1) * t.element_size()


def head_offset(a: Tensor) -> int | None:
    """bytes into ``a`` at which the other operand starts: the smallest multiple of 256 >= one row of ``a`` and < its extent"""
    if _extent(a) <= STEP:
        return None
    off = -(-_row_bytes(a) // STEP) * STEP
    return off if off < _extent(a) else None


def _two_d(t: Tensor) -> bool:
    return t.dim() == 2 and t.shape[0] > 1 and t.numel() > 0


def tags_for(w: Tensor, t: Tensor) -> list[str]:
    """the placements that apply to canonical operands ``w`` (written) and ``t``, from the contract's table alone"""
    if w.numel() == 0 or t.numel() == 0:
        return []
    tags = ["same"]
    if head_offset(w) is not None:
        tags.append("head")
    if head_offset(t) is not None:
        tags.append("tail")
    if _two_d(w) and _two_d(t):
        tags.append("columns")
    return tags


@dataclass
class Case:
    tag: str
    wpath: tuple
    tpath: tuple
    w: Tensor           # the view handed to the wrapper as W
    t: Tensor           # the view handed to the wrapper as T (``w`` itself for an identical view)
    words: Tensor       # the arena
    identical: bool     # T is W's very view

    @property
    def name(self) -> str:
        return f"{path_name(self.wpath)} x {path_name(self.tpath)} {self.tag}"

    def inside(self) -> Tensor:
        """byte mask of the arena: True where W or T lives"""
        m = torch.zeros(self.words.numel() * 4, dtype=torch.bool, device=self.words.device)
        base = self.words.data_ptr()
        for v in (self.w, self.t):
            it = v.element_size()
            first = m.as_strided(tuple(v.shape) + (it,), tuple(s * it for s in v.stride()) + (1,), v.data_ptr() - base)
            first.fill_(True)
        return m

    def check_bounds(self) -> None:
        base, n = self.words.data_ptr(), self.words.numel() * 4
        for v in (self.w, self.t):
            lo = v.data_ptr() - base
            hi = lo + (1 + sum((k - 1) * s for k, s in zip(v.shape, v.stride()))) * v.element_size()
            assert lo >= v.numel() * WC.WIDEST and hi + v.numel() * WC.WIDEST <= n, (self.name, lo, hi, n)
            assert lo % STEP == 0, (self.name, lo)


def _arena(nbytes: int, device) -> Tensor:
    return torch.full((-(-nbytes // STEP) * STEP // 4,), WC.POISON32, dtype=WC.I32, device=device)


def _view(words: Tensor, dtype, shape, strides, byte_off: int) -> Tensor:
    it = torch.empty(0, dtype=dtype).element_size()
    assert byte_off % it == 0
    return words.view(dtype).as_strided(tuple(shape), tuple(strides), byte_off // it)


def place(tag: str, wpath, tpath, w: Tensor, t: Tensor) -> Case:
    """``w`` and ``t`` (canonical, contiguous) as views of one fresh arena in placement ``tag``, holding their values (T's where
    they overlap: an addressing operand keeps the canonical ids, so a refusal is the alias check's and not a range check's)"""
    assert w.is_contiguous() and t.is_contiguous()
    ew, et = _extent(w), _extent(t)
    room = -(-(w.numel() + t.numel()) * WC.WIDEST // STEP) * STEP + STEP
    if tag == "columns":
        cw, ct = -(-_row_bytes(w) // STEP) * STEP, -(-_row_bytes(t) // STEP) * STEP
        pitch, rows = cw + ct, max(w.shape[0], t.shape[0])
        words = _arena(2 * room + rows * pitch, w.device)
        wv = _view(words, w.dtype, w.shape, (pitch // w.element_size(), 1), room)
        tv = _view(words, t.dtype, t.shape, (pitch // t.element_size(), 1), room + cw)
        wv.copy_(w)
        tv.copy_(t)
        return Case(tag, wpath, tpath, wv, tv, words, False)
    words = _arena(2 * room + ew + et + STEP, w.device)
    wo = to = room
    if tag == "head":
        to = room + head_offset(w)
    elif tag == "tail":
        wo = room + head_offset(t)
    wv = _view(words, w.dtype, w.shape, w.stride(), wo)
    identical = tag == "same" and w.dtype == t.dtype and w.shape == t.shape
    tv = wv if identical else _view(words, t.dtype, t.shape, t.stride(), to)
    wv.copy_(w)
    tv.copy_(t)
    return Case(tag, wpath, tpath, wv, tv, words, identical)


def cases(r: WC.Row, dev):
    """every (W, T, tag) of one row; each case on a fresh build of the row"""
    kw = r.build(dev)
    ops_ = list(operands(kw))
    for wpath in written_paths(r, kw):
        for tpath, t in ops_:
            if tpath == wpath:
                continue
            for tag in tags_for(get(kw, wpath), t):
                yield place(tag, wpath, tpath, get(kw, wpath).clone(), t.clone())


def expected(r: WC.Row, c: Case, kw: dict) -> str:
    """'honoured' or 'refused', from the contract and ALIAS_OK alone"""
    if c.tag == "columns":
        return "honoured"
    ok = ALIAS_OK.get((r.fn, path_name(c.wpath), path_name(c.tpath)))
    if c.tag == "same" and c.identical and ok is not None and ok.cond(kw) and not is_control(path_name(c.tpath), c.t):
        return "honoured"
    return "refused"


# ------------------------------------------------------------------------------------------------------------------ driver
def _kw(r: WC.Row, dev, c: Case, **over) -> dict:
    kw = replaced(replaced(r.build(dev), c.wpath, c.w), c.tpath, c.t)
    kw.update(over)
    return kw


def _snap(r: WC.Row, kw: dict, res) -> list:
    return WC.snapshot(r, kw, res)


def _columns_serves(ops, r: WC.Row, dev, c: Case) -> str | None:
    """None if the wrapper takes W's and T's column views each on its own (operand apart from everything); else the refusal: such a
    pair has no ``columns`` case to honour - the layout contract (section 26) refuses the view itself"""
    for path, v in ((c.wpath, c.w), (c.tpath, c.t)):
        lone = place("columns", c.wpath, c.tpath, get(r.build(dev), c.wpath).clone(), get(r.build(dev), c.tpath).clone())
        kw = replaced(r.build(dev), path, lone.w if path == c.wpath else lone.t)
        try:
            WC.call(ops, r, kw)
        except WC.REFUSALS as e:
            if WC.is_fault(e):
                raise WC.GpuFault(f"{r.id} {c.name}: {e}") from e
            return f"{path_name(path)}: {e}"
    return None


def check_row(ops, r: WC.Row, dev, compare: bool, hook=None, only=None, launch: bool = True):
    """Every case of one row: (problems, outcomes) with outcomes a list of (row, W, T, tag, outcome).  ``hook``: the CPU stage's
    recorder (begin() / launches).  ``only``: a set of (row, W, T, tag) - cases outside it that the contract honours are not
    launched (the GPU stage launches what the CPU audit saw accepted and nothing else).  ``compare``: an honoured call must give
    the bits of the same call with T cloned first."""
    problems, outcomes = [], []
    for c in cases(r, dev):
        where = f"{r.id} {c.name}"
        key = (r.id, path_name(c.wpath), path_name(c.tpath), c.tag)
        c.check_bounds()
        kw = _kw(r, dev, c)
        want = expected(r, c, kw)
        if c.tag == "columns":
            why = _columns_serves(ops, r, dev, c)
            if why is not None:
                outcomes.append(key + ("layout",))
                continue
        runs = [("", kw, want)]
        ok = ALIAS_OK.get((r.fn, path_name(c.wpath), path_name(c.tpath)))
        if want == "honoured" and c.tag == "same" and ok.broken:
            runs.append((" with the condition broken", _kw(r, dev, c, **ok.broken), "refused"))
        for note, kw, want in runs:
            if want == "honoured" and only is not None and key not in only:
                problems.append(f"{where}{note}: the contract honours it but the CPU audit did not see it accepted: not launched")
                continue
            host_t = path_name(c.tpath) in r.host_ok and not c.t.is_cuda  # read back and uploaded: the launch never sees T
            arena_before = c.words.clone()
            before = _snap(r, kw, None)
            if hook:
                hook.begin()
            try:
                res, exc = WC.call(ops, r, kw), None
            except WC.REFUSALS as e:
                if WC.is_fault(e):
                    raise WC.GpuFault(f"{where}: {e}") from e
                res, exc = None, e
            except Exception as e:  # noqa: BLE001
                problems.append(f"{where}{note}: raised {type(e).__name__}: {e}")
                continue
            n_launch = len(hook.launches) if hook else 0
            if exc is not None:
                outcomes.append(key + ("refused" + note,))
                if n_launch:
                    problems.append(f"{where}{note}: refused after {n_launch} launches")
                if want != "refused":
                    problems.append(f"{where}{note}: refused ({exc}); the contract honours it")
                    continue
                names = (r.fn, path_name(c.wpath).split("[")[0], path_name(c.tpath).split("[")[0])
                if type(exc) is not ValueError or not all(n in str(exc) for n in names):
                    problems.append(f"{where}{note}: not an aliasing refusal naming {names}: {type(exc).__name__}: {exc}")
                changed = WC._diff(before, _snap(r, kw, None))
                if changed or not WC.same_bits(c.words, arena_before):
                    problems.append(f"{where}{note}: refused but wrote {changed or 'into the arena'}")
                continue
            outcomes.append(key + ("honoured" + note,))
            if want == "refused":
                if host_t:  # "host ints or a device tensor": a CPU tensor's values were read and uploaded into a buffer of the wrapper's own
                    outcomes[-1] = key + ("copied",)
                    continue
                problems.append(f"{where}{note}: REACHED A LAUNCH: {path_name(c.wpath)} (written) shares memory with "
                                f"{path_name(c.tpath)}" + (" (an addressing or control operand)" if is_control(path_name(c.tpath), c.t) else ""))
                continue
            if not compare:
                continue
            got = _snap(r, kw, res)
            if c.tag == "columns":
                kwr = r.build(dev)
            else:  # the same call with T cloned first
                fresh = place(c.tag, c.wpath, c.tpath, get(r.build(dev), c.wpath).clone(), get(r.build(dev), c.tpath).clone())
                kwr = replaced(replaced(r.build(dev), c.wpath, fresh.w), c.tpath, fresh.t.clone())
            ref = _snap(r, kwr, WC.call(ops, r, kwr))
            bad = WC._diff(got, ref)
            if bad:
                problems.append(f"{where}: honoured but {bad} differ from the call with {path_name(c.tpath)} cloned first")
            m = c.inside()
            if not WC.same_bits(c.words.view(torch.uint8)[~m], arena_before.view(torch.uint8)[~m]):
                problems.append(f"{where}: wrote outside its operands")
            if c.tag == "columns" and path_name(c.tpath).split("[")[0] not in r.inplace and not WC.same_bits(c.t, get(r.build(dev), c.tpath)):
                problems.append(f"{where}: wrote into {path_name(c.tpath)}, the neighbouring columns")
    return problems, outcomes


def _ints(args) -> list:
    import ctypes
    out = []
    for a in args:
        for v in (a if isinstance(a, ctypes.Array) else [a]):
            if isinstance(v, int) and not isinstance(v, bool):
                out.append(v)
    return out


# ------------------------------------------------------------------------------------------- the header's non-const pointers
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pm_mi355x.h")


def writable_params(path: str = HEADER) -> dict[str, list[bool]]:
    """function -> per parameter: a pointer the prototype does not mark const (the callee may write through it)"""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for _, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(pm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        ps = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        out[name] = ["*" in p and not p.startswith("const") for p in ps]
    return out
