"""Reference and case selection of eos stopping and the repetition controls (pm_dec_controls / pm_dec_finish, csrc/controls.hip;
DESIGN.md section 31), shared by tests/test_control_cases_cpu.py (no GPU), tests/test_hip_control_kernels.py and
tests/test_hip_controls.py.  A plain helper.

Reference, one row (plain Python over torch fp32 scalars; h = the row's history, prompt included, padding excluded):
  penalty    every DISTINCT in-range id v of h, once: l[v] = l[v] / r if l[v] > 0 else l[v] * r, r the fp32 value the C ABI receives -
             one fp32 operation, so the kernel's row must be BIT-equal;
  no-repeat  m = len(h) >= n - 1: for every 0 <= i <= m - n with h[i : i + n - 1] == h[m - n + 1 : m]: l[h[i + n - 1]] = -inf;
  min length n_gen < min_new_tokens: l[eos] = -inf;
  finish     at position t1 >= P: a finished row gets pad and log-prob 0, else a row whose token is eos records t1.

Case selection, on the CPU from the K/V-rounded oracle alone (tests/test_control_cases_cpu.py asserts every property):
  * the oracle's plain greedy run of N = 12 new tokens repeats a 2-gram (GPT-2 loops, notoriously), so NGRAM = 2 bites: with
    sample_cases' prompts already, and in every row with the prompts of the controlled runs (GPT2_CTL_SEED, WHISPER_CTL_SEED below);
  * the eos: the id whose FIRST generated occurrence differs from row to row and lies before the last position in every row.
    Whisper's plain run has one (48078).  GPT-2's three rows share no token (nor do those of 64 other synthetic prompts that were
    scanned), but rows 1 and 2 of the existing prompt do (21947, first at positions 3 and 4): the GPT-2 eos runs take those two rows
    (GPT2_EOS_ROWS);
  * the margins: the oracle's top-1 minus top-2 after the controls (and the rules), along the oracle's own controlled run; a position is
    CLEAR when it exceeds margin_bound(r) = 2 max(r, 1 / r) LP_TOL (LP_TOL = 1.2e-1, the step-against-oracle distance of
    tests/test_hip_sample.py; the penalty scales a logit's error by at most max(r, 1 / r)); at most sample_cases.EDGE_CAP of the
    positions of a run may be unclear.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

import sample_cases as S

LP_TOL = 1.2e-1
N = 12
NGRAM = 2
MAX_NGRAM = 8
PAD = 7


def f32(x: float) -> torch.Tensor:
    return torch.tensor(float(x), dtype=torch.float32)


def margin_bound(r: float) -> float:
    return 2.0 * max(r, 1.0 / r) * LP_TOL


@dataclass(frozen=True)
class Ctl:
    r: float = 1.0
    n: int = 0
    min_new: int = 0
    eos: int | None = None

    def kwargs(self) -> dict:
        """the public keywords"""
        return dict(repetition_penalty=self.r, no_repeat_ngram_size=self.n, min_new_tokens=self.min_new, eos_token_id=self.eos)


# ------------------------------------------------------------------------------------------------------------------ reference
def banned(hist: list[int], n: int) -> set[int]:
    """the ids that would complete an n-gram the history already holds"""
    m = len(hist)
    out = set()
    if n < 1 or m < n - 1:
        return out
    tail = hist[m - n + 1:] if n > 1 else []
    for i in range(0, m - n + 1):
        if hist[i:i + n - 1] == tail:
            out.add(hist[i + n - 1])
    return out


def brute_banned(hist: list[int], n: int) -> set[int]:
    """written independently: the set of every n-gram of the history, then every candidate id tried against it"""
    if n < 1 or len(hist) < n - 1:
        return set()
    grams = {tuple(hist[i:i + n]) for i in range(len(hist) - n + 1)}
    open_gram = tuple(hist[len(hist) - (n - 1):]) if n > 1 else ()
    return {v for v in set(hist) if open_gram + (v,) in grams}


def apply_controls(l: torch.Tensor, hist: list[int], n_gen: int, c: Ctl) -> torch.Tensor:
    """the row after the controls; ``hist`` = the row's real tokens up to the current one, ``n_gen`` = tokens generated so far"""
    assert l.dtype == torch.float32 and l.dim() == 1
    V = l.numel()
    out = l.clone()
    if c.r != 1.0:
        r = f32(c.r)
        ids = torch.tensor(sorted(v for v in set(hist) if 0 <= v < V), dtype=torch.int64)  # every distinct id, once
        x = l[ids]
        out[ids] = torch.where(x > 0, x / r, x * r)  # torch's fp32 quotient and product, elementwise
    for v in banned(hist, c.n):
        if 0 <= v < V:
            out[v] = -math.inf
    if c.eos is not None and n_gen < c.min_new:
        out[c.eos] = -math.inf
    return out


def finish_step(tokens: list[int], logprobs: list[float] | None, finished: int, t1: int, P: int, eos: int, pad: int) -> int:
    """pm_dec_finish for one row at position t1 (already written by the tail): edits the lists in place, returns ``finished``"""
    if t1 < P:
        return finished
    if finished != 0:
        tokens[t1] = pad
        if logprobs is not None:
            logprobs[t1] = 0.0
        return finished
    return t1 if tokens[t1] == eos else 0


def cut_at_eos(new: list[int], eos: int | None, pad: int) -> tuple[list[int], int]:
    """(what a run with eos_token_id returns for a row whose uncut new ids are ``new``, its n_new)"""
    if eos is None or eos not in new:
        return list(new), len(new)
    k = new.index(eos) + 1
    return new[:k] + [pad] * (len(new) - k), k


def has_repeat(row: list[int], n: int) -> bool:
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) != len(set(grams))


def top2(l: torch.Tensor) -> tuple[int, float]:
    """(the lowest arg-max index, top-1 minus top-2; inf when a single id is left)"""
    v = l.topk(2).values
    m = float(v[0] - v[1]) if float(v[1]) > -math.inf else math.inf
    return S.lowest_argmax(l), m


def position(l: torch.Tensor, hist: list[int], n_gen: int, c: Ctl, post=None) -> tuple[torch.Tensor, int, float]:
    """(the row after controls and ``post`` (the rules: post(row, generated ids)), its arg-max, its top-2 margin)"""
    out = apply_controls(l.float(), hist, n_gen, c)
    if post is not None:
        out = post(out, hist[len(hist) - n_gen:])
    return (out, *top2(out))


def controlled_run(last_logits, prompt: torch.Tensor, n_new: int, c: Ctl, post=None, lens=None):
    """the oracle decoding by itself under the controls, WITHOUT stopping at the eos (the uncut run): ``last_logits(tokens (1, L)) ->
    (1, V)``; row b's prompt is prompt[b, :lens[b]].  Returns (rows: list of id lists (prompt + n_new), margins (B, n_new))"""
    rows, margins = [], []
    for b in range(prompt.shape[0]):
        row = prompt[b, : (prompt.shape[1] if lens is None else lens[b])].tolist()
        ms = []
        for i in range(n_new):
            l = last_logits(torch.tensor([row]))[0]
            _, tok, m = position(l, row, i, c, post)
            row.append(tok)
            ms.append(m)
        rows.append(row)
        margins.append(ms)
    return rows, torch.tensor(margins)


def unclear_share(margins: torch.Tensor, r: float) -> float:
    return float((margins <= margin_bound(r)).float().mean())


# ------------------------------------------------------------------------------------------------------------- chosen inputs
def whisper_post(rules: bool):
    if not rules:
        return None
    from oracle import ref_whisper_rules as RR

    orules = RR.Rules(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in S.WHISPER_RULES.items()})
    return lambda row, gen: RR.apply(orules, row, list(gen))


def whisper_last(sd, memory, b: int):
    """last-position oracle logits of clip b, no rules (they come after the controls)"""
    return lambda toks: S.whisper_logits(sd, memory[b:b + 1], toks, toks.shape[1], False)[:, -1]


def first_positions(rows_new: list[list[int]]) -> dict[int, list[int]]:
    """id -> its first generated position in every row, for the ids every row generates"""
    common = set(rows_new[0]).intersection(*map(set, rows_new[1:]))
    return {v: [r.index(v) for r in rows_new] for v in sorted(common)}


def pick_eos(rows_new: list[list[int]]) -> int | None:
    """the lowest id every row emits, first at pairwise DIFFERENT positions, each before the last position"""
    for v, at in first_positions(rows_new).items():
        if len(set(at)) == len(at) and max(at) < len(rows_new[0]) - 1:
            return v
    return None


GPT2_EOS_ROWS = (1, 2)  # of gpt2_setup()'s prompt: the rows whose plain runs share a token
# the prompts of the CONTROLLED runs: the first seeds of synth_tokens("control_prompt" / "control_wprompt", ...) (scanned from 0) for
# which the reference alone keeps every run of RUNS inside EDGE_CAP, every row's plain run repeats a 2-gram and (Whisper, under the
# rules) pick_eos finds an eos; with the prompts of sample_cases the controlled runs have 14-22 % of their positions unclear
GPT2_CTL_SEED = 24
WHISPER_CTL_SEED = 2
R = 1.3


def gpt2_ctl_prompt() -> torch.Tensor:
    from synthweights import synth_tokens

    return synth_tokens("control_prompt", (3, 23), 2000, GPT2_CTL_SEED)


def whisper_ctl_prompt() -> torch.Tensor:
    from synthweights import synth_tokens

    return synth_tokens("control_wprompt", (2, 4), 51865, WHISPER_CTL_SEED)


def _whisper_run(prompt: torch.Tensor, c: Ctl, rules: bool):
    _, sd, memory, _ = S.whisper_setup()
    rows, margins = [], []
    for b in range(prompt.shape[0]):
        r, m = controlled_run(whisper_last(sd, memory, b), prompt[b:b + 1], N, c, whisper_post(rules))
        rows += r
        margins.append(m[0])
    return rows, torch.stack(margins)


@functools.lru_cache(maxsize=None)
def gpt2_plain(ctl_prompt: bool = False):
    """(prompt (3, 23), the oracle's plain greedy rows, margins (3, N)): sample_cases' prompt, or the controlled runs' prompt"""
    _, sd, prompt = S.gpt2_setup()
    if ctl_prompt:
        prompt = gpt2_ctl_prompt()
    rows, margins = controlled_run(S.gpt2_last_logits(sd), prompt, N, Ctl())
    return prompt, rows, margins


@functools.lru_cache(maxsize=None)
def whisper_plain(rules: bool, ctl_prompt: bool = False):
    """(prompt (2, 4), the oracle's plain greedy rows, margins): whisper_setup()'s prompt, or the controlled runs' prompt"""
    prompt = whisper_ctl_prompt() if ctl_prompt else S.whisper_setup()[3]
    return (prompt, *_whisper_run(prompt, Ctl(), rules))


def gpt2_eos() -> int:
    """of rows GPT2_EOS_ROWS of sample_cases' prompt"""
    return pick_eos([gpt2_plain()[1][b][23:] for b in GPT2_EOS_ROWS])


def whisper_eos(rules: bool) -> int:
    """without the rules: of whisper_setup()'s prompt; under the rules: of the controlled runs' prompt"""
    return pick_eos([r[4:] for r in whisper_plain(rules, ctl_prompt=rules)[1]])


# the controlled runs of the end-to-end suite: name -> (model, Ctl without its eos, rules)
RUNS = {
    "gpt2_ngram": ("gpt2", Ctl(n=NGRAM), False),
    "gpt2_penalty": ("gpt2", Ctl(r=R), False),
    "gpt2_all": ("gpt2", Ctl(r=R, n=NGRAM, min_new=4), False),
    "whisper_all_rules": ("whisper", Ctl(r=R, n=NGRAM, min_new=3), True),
}


@functools.lru_cache(maxsize=None)
def run_case(name: str):
    """(prompt, Ctl - with an eos where min_new asks for one -, the oracle's controlled uncut rows, margins).  The eos of the GPT-2
    run is the first token row 0's plain run generates: without the minimum length that row would finish at once, so the control
    visibly moves it; Whisper's is whisper_eos(True)"""
    model, c, rules = RUNS[name]
    if model == "gpt2":
        _, sd, _ = S.gpt2_setup()
        prompt = gpt2_ctl_prompt()
        if c.min_new:
            c = Ctl(c.r, c.n, c.min_new, gpt2_plain(True)[1][0][23])
        return (prompt, c, *controlled_run(S.gpt2_last_logits(sd), prompt, N, c))
    prompt = whisper_ctl_prompt()
    if c.min_new:
        c = Ctl(c.r, c.n, c.min_new, whisper_eos(rules))
    return (prompt, c, *_whisper_run(prompt, c, rules))


# the sampled run under the controls: sample_cases.GPT2_RUN's settings on the controlled runs' prompt, its seed the first (from 0)
# for which the oracle's own run has no position closer than DRAW_MARGIN to an edge of the draw
SAMPLED_CTL = Ctl(r=R, n=NGRAM)
SAMPLED_SEED = 6


def sampled_run() -> dict:
    return dict(S.GPT2_RUN, seed=SAMPLED_SEED, n_new=N)


@functools.lru_cache(maxsize=None)
def sampled_case(seed: int = SAMPLED_SEED):
    """(prompt, the oracle's sampled rows under SAMPLED_CTL, edge distances (3, N)): every draw keyed by (seed, cache position, row)"""
    _, sd, _ = S.gpt2_setup()
    last, prompt, run = S.gpt2_last_logits(sd), gpt2_ctl_prompt(), dict(sampled_run(), seed=seed)
    rows, edges = [], []
    for b in range(prompt.shape[0]):
        row, es = prompt[b].tolist(), []
        for i in range(N):
            l = apply_controls(last(torch.tensor([row]))[0], row, i, SAMPLED_CTL)
            _, tok, e = S.position_reference(l, run, len(row) - 1, b)
            row.append(tok)
            es.append(e)
        rows.append(row)
        edges.append(es)
    return prompt, rows, torch.tensor(edges)


# --------------------------------------------------------------------------------------------- the wrappers' operand layouts
def wrapper_rows() -> dict:
    """rows for tests/wrapper_cases.check_row on pytorch_models._hip.controls (the wrappers live outside ops.py, so their rows live
    here and are not registered in wrapper_cases.ROWS)"""
    import wrapper_cases as WC

    def controls(form):
        def make(dev):
            g = WC.Gen(dev, WC.SEED + 5000)
            kw = dict(logits=g.f(2, 11), tokens=g.i(11, 2, 8), pos=g.t([5], WC.I32), P=2, repetition_penalty=1.3, no_repeat_ngram_size=2,
                      min_new_tokens=6, eos_token_id=4)
            if form == "ragged":
                kw["key_start"] = g.t([0, 2], WC.I32)
            return kw
        return make

    def finish(form):
        def make(dev):
            g = WC.Gen(dev, WC.SEED + 5001)
            tokens = g.i(11, 2, 8)
            tokens[0, 5] = 4
            kw = dict(tokens=tokens, tok_cur=g.i(11, 2), finished=g.t([0, 3], WC.I32), pos=g.t([5], WC.I32), P=2, eos_token_id=4, pad_token_id=9)
            if form == "logprobs":
                kw["logprobs"] = g.f(2, 8)
            return kw
        return make

    rows = {f"controls:{f}": WC.Row(f"dec_controls:{f}", "dec_controls", controls(f), ("logits",)) for f in ("plain", "ragged")}
    rows.update({f"finish:{f}": WC.Row(f"dec_finish:{f}", "dec_finish", finish(f), ("tokens", "tok_cur", "finished", "logprobs"))
                 for f in ("plain", "logprobs")})
    return rows
