"""Reference, edge distances, log-prob bound, input families and the case table of the sampling tail (pm_dec_sample, csrc/sample.hip;
DESIGN.md section 27), shared by tests/test_sample_cases_cpu.py (no GPU), tests/test_hip_sample_kernels.py and tests/test_hip_sample.py.
A plain helper.

Reference.  float64 on the CPU from the fp32 logits the kernel sees, per row (l = the row, m = max l):
  1. logprob(tok) = l[tok] - (m + log sum exp(l - m)), at temperature 1;
  2. temperature == 0: the lowest index with l == m;
  3. w = exp((l - m) / T), -inf -> 0 (T and top_p are the fp32 values the C ABI receives, widened exactly);
  4. survivors: the k first in (logit descending, index ascending) (a stable descending sort), or all;
  5. top_p < 1: tau = the largest value among the survivors with mass(l >= tau) >= top_p W; nucleus = survivors with l >= tau;
  6. u = decode_cases.ds_uniform(seed, position, row), replayed in Python integers; the pick = the first nucleus element whose
     running mass exceeds u M, in the sorted order (k >= 1) or by ascending index (k = 0); else the last nucleus element.

Edge distances.  Each decision reports how far the reference is from deciding otherwise:
  nucleus: |mass(l >= v) - top_p W| / W for v = tau, the value above tau and the value below it (inf when top_p == 1);
  draw   : min_i |u M - cum_i| / M over the running sums but the last (decode_cases.sample_pick's rule: beyond the last there is
           nothing else to pick).
A case is KEPT only if the reference alone shows every distance above DRAW_MARGIN = 1e-3, the margin decode_cases.py uses for
pm_dec_sample_topk's draws; build() scans seeds for one.  The kernel's fp32 masses are within ~1e-5 of the float64 ones (bound
below), so a kept case has one right token and the GPU tests assert EQUALITY.  Families whose boundaries are denser than the
margin are not built: a row of V equal logits has its boundaries 1 / V apart, so "equal" exists for V <= 257 only, and the
Gaussian family for V <= 1000, B <= 3; at V = 50257 the mass sits on a handful of planted tokens (the tail's share is ~1e-6).

Log-prob bound (u = 2^-24; nothing measured on a kernel enters it).  The kernel forms S = sum exp(l - max) online: a lane adds
n = ceil(ceil(V / 16) / 64) terms, four per rescale; then 6 shuffle merges and 15 wave merges.  With R = min(finite range, 104)
(an argument below -104 gives 0 either way):
  one term       : the difference rounds once (R u), expf within 2 ulp (4 u)                          (R + 4) u
  a lane's adds  : n u
  its rescales   : G = ceil(n / 4) factors, each (|d_k| + 4) u and a product rounding; sum |d_k| <= R   R u + 5 G u
  21 merges      : each side one factor ((R + 4) u), a product (u), an addition (u)                    21 (R + 6) u
  eps_S = (23 R + n + 5 G + 130) u, absolute on log S; then lse = m + logf(S) and logprob = l[tok] - lse: 4 ulp = 8 u at the
  magnitude |m| + |lse| + |l[tok]|.  The GPU suite asserts MARGIN = 1.5 x the bound, as the score kernel's tests do.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from decode_cases import ds_uniform

U32 = 2.0 ** -24
MARGIN = 1.5
DRAW_MARGIN = 1e-3
TOPKS = (0, 1, 2, 50, 64)
TEMPS = (0.0, 1e-3, 0.7, 1.0, 100.0)
TOP_PS = (1.0, 0.9, 0.5, 1e-6)
SEED0 = 4000
SEED_SCAN = 400


def f32(x: float) -> float:
    """the fp32 value the C ABI receives, as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ reference
@dataclass
class RowRef:
    """what does not depend on the draw: one row's statistics, its nucleus in running order with the running masses"""
    m: float
    lse: float
    argmax: int
    order: torch.Tensor   # int64: nucleus token ids in running order (empty at temperature 0)
    cum: torch.Tensor     # float64 running masses of ``order``
    tau: float            # -inf when nothing is cut
    nucleus_edge: float   # distance of the nucleus decision to its nearest edge (inf: no decision)
    lp_bound_S: float     # eps_S of the module docstring


def lowest_argmax(l: torch.Tensor) -> int:
    return int((l == l.max()).nonzero()[0])


def eps_S(l64: torch.Tensor) -> float:
    V = l64.numel()
    fin = l64[torch.isfinite(l64)]
    R = min(float(fin.max() - fin.min()), 104.0) if fin.numel() else 0.0
    n = -(-(-(-V // 16)) // 64)
    G = -(-n // 4)
    return (23.0 * R + n + 5.0 * G + 130.0) * U32


def row_reference(l: torch.Tensor, topk: int, temperature: float, top_p: float) -> RowRef:
    assert l.dtype == torch.float32 and l.dim() == 1
    V = l.numel()
    l64 = l.double()
    m = float(l64.max())
    lse = m + math.log(float(torch.exp(l64 - m).sum())) if m > -math.inf else -math.inf
    am = lowest_argmax(l64)
    T, p = f32(temperature), f32(top_p)
    empty = torch.empty(0, dtype=torch.int64)
    if T == 0.0:
        return RowRef(m, lse, am, empty, empty.double(), -math.inf, math.inf, eps_S(l64))
    w = torch.where(l64 == -math.inf, torch.zeros_like(l64), torch.exp((l64 - m) / T))
    desc = torch.sort(l64, descending=True, stable=True).indices  # (logit descending, index ascending)
    surv = desc[: min(topk, V)] if topk >= 1 else desc
    tau, edge = -math.inf, math.inf
    if p < 1.0:
        vals, ws = l64[surv], w[surv]
        W = float(ws.sum())
        cum = torch.cumsum(ws, 0)
        last = torch.ones_like(vals, dtype=torch.bool)  # the last position of every tie group: mass(l >= its value) = cum there
        last[:-1] = vals[:-1] != vals[1:]
        gv, gm = vals[last], cum[last]
        ok = (gm >= p * W).nonzero()
        g = int(ok[0]) if len(ok) else len(gv) - 1
        tau = float(gv[g])
        near = [abs(float(gm[j]) - p * W) / W for j in (g - 1, g, g + 1) if 0 <= j < len(gv)] if W > 0 else [0.0]
        edge = min(near)
        surv = surv[vals >= tau]
    order = surv if topk >= 1 else torch.sort(surv).values  # the sorted order, or ascending token index
    return RowRef(m, lse, am, order, torch.cumsum(w[order], 0), tau, edge, eps_S(l64))


def draw(rr: RowRef, seed: int, t: int, b: int) -> tuple[int, float]:
    """(the reference's token, the distance of the draw to its nearest edge)"""
    if rr.order.numel() == 0:
        return rr.argmax, math.inf
    M = float(rr.cum[-1])
    target = ds_uniform(seed, t, b)[1] * M
    hit = (rr.cum > target).nonzero()
    pick = int(hit[0]) if len(hit) else rr.order.numel() - 1
    edge = float((rr.cum[:-1] - target).abs().min()) / M if rr.order.numel() > 1 and M > 0 else math.inf
    return int(rr.order[pick]), edge


def logprob(l: torch.Tensor, rr: RowRef, tok: int) -> tuple[float, float]:
    """(float64 log-probability of ``tok``, its bound for the kernel)"""
    x = float(l[tok])
    lp = x - rr.lse
    few = 8 * U32 * (abs(rr.m) + abs(rr.lse) + (abs(x) if math.isfinite(x) else 0.0))
    return lp, rr.lp_bound_S + few


def brute_nucleus(l: torch.Tensor, topk: int, temperature: float, top_p: float) -> set[int]:
    """the nucleus by torch.sort and cumsum in float64, written independently of row_reference: the smallest prefix of the sorted
    survivors whose mass reaches top_p W, extended over the ties of its last value"""
    l64 = l.double()
    T, p = f32(temperature), f32(top_p)
    vals, idx = torch.sort(l64, descending=True, stable=True)
    if topk >= 1:
        vals, idx = vals[:topk], idx[:topk]
    w = torch.where(vals == -math.inf, torch.zeros_like(vals), torch.exp((vals - vals[0]) / T))
    if p >= 1.0:
        return set(idx.tolist())
    cum = torch.cumsum(w, 0)
    need = p * float(w.sum())
    keep = 0
    while True:  # whole tie groups, one at a time
        e = keep
        while e + 1 < len(vals) and vals[e + 1] == vals[keep]:
            e += 1
        if float(cum[e]) >= need or e + 1 == len(vals):
            return set(idx[: e + 1].tolist())
        keep = e + 1


# ----------------------------------------------------------------------------------------------------------------- case table
@dataclass(frozen=True)
class Case:
    family: str
    B: int
    V: int
    topk: int
    temperature: float
    top_p: float
    pos: int = 3       # the cache position t of the launch; the token chosen sits at t + 1
    P: int = 2         # prompt width: t + 1 >= P draws, t + 1 < P forces
    Ttot: int = 8
    d: int = 32
    ragged: bool = False
    n_seeds: int = 1   # how many clear seeds the case runs

    @property
    def id(self) -> str:
        return (f"{self.family}-B{self.B}-V{self.V}-k{self.topk}-T{self.temperature:g}-p{self.top_p:g}"
                + ("-forced" if self.pos + 1 < self.P else "") + ("-ragged" if self.ragged else ""))


SETTINGS = [(k, T, p) for k in TOPKS for T in TEMPS for p in TOP_PS]
HEAVY = [(64, 257), (1, 50257), (3, 50257), (64, 1000), (1, 1000)]


def cases() -> list[Case]:
    out = []
    for i, (k, T, p) in enumerate(SETTINGS):  # every setting at the small sizes; the others take turns (each meets every topk, T, p)
        out.append(Case("planted", 3, 257, k, T, p))
        out.append(Case("planted", 3, 5, k, T, p))
        B, V = HEAVY[i % len(HEAVY)]
        out.append(Case("planted", B, V, k, T, p))
    # the real vocabulary at the full batch: the whole-vocabulary paths, one top-k, the arg-max
    for k, T, p in ((0, 0.7, 0.9), (0, 1.0, 1.0), (0, 1e-3, 0.5), (0, 100.0, 1e-6), (50, 0.7, 0.9), (64, 1.0, 0.5), (0, 0.0, 1.0)):
        out.append(Case("planted", 64, 50257, k, T, p))
    for k, T, p in ((0, 0.7, 0.9), (0, 1.0, 1.0), (0, 1.0, 0.5), (50, 0.7, 0.9), (64, 1.0, 1.0), (2, 100.0, 0.9)):  # many tokens matter
        out.append(Case("gauss", 3, 1000, k, T, p))
        out.append(Case("gauss", 1, 257, k, T, p))
    for V in (5, 257):  # all equal: every token survives any top_p, the draw is uniform
        for k, T, p in ((0, 0.7, 0.5), (0, 100.0, 1e-6), (0, 1.0, 1.0), (64, 1.0, 0.9), (2, 0.7, 0.5)):
            out.append(Case("equal", 3, V, k, T, p, n_seeds=3))
    for V in (5, 1000, 50257):  # one dominant logit: that token for every seed
        for k, T, p in ((0, 1.0, 1.0), (0, 0.7, 0.9), (50, 1.0, 0.5), (0, 100.0, 1.0)):
            out.append(Case("dominant", 3, V, k, T, p, n_seeds=4))
    for V in (5, 257, 50257):  # -inf columns, down to a single finite one: never drawn
        for k, T, p in ((0, 1.0, 1.0), (0, 0.7, 0.5), (64, 1.0, 1.0), (2, 100.0, 0.9), (0, 0.0, 1.0)):
            out.append(Case("neginf", 3, V, k, T, p, n_seeds=2))
    for V in (5, 1000):  # magnitudes up to 3e38 at temperature 1e-3: no NaN
        for k, T, p in ((0, 1e-3, 1.0), (0, 1e-3, 0.5), (64, 1e-3, 0.9), (0, 100.0, 1.0), (0, 0.0, 1.0)):
            out.append(Case("huge", 3, V, k, T, p))
    for k, T, p in ((0, 0.7, 0.9), (50, 1.0, 1.0), (0, 0.0, 1.0)):  # a forced prompt position: the draw is ignored, the tail advances
        out.append(Case("planted", 3, 257, k, T, p, pos=1, P=4))
    for k, T, p in ((0, 0.7, 0.9), (50, 0.7, 0.5)):  # the ragged form: the same picks, the embedding row of ragged_pos
        out.append(Case("planted", 3, 1000, k, T, p, ragged=True))
    out.append(Case("planted", 3, 257, 0, 0.7, 0.9, pos=6))  # t + 1 == Ttot - 1: the last column is written
    return out


SALTS = 8  # how many input draws build() may try until the nucleus decisions of all rows are clear


def _gen(c: Case, salt: int = 0) -> torch.Generator:
    return torch.Generator().manual_seed(7919 * c.B + c.V + 31 * len(c.family) + 104729 * salt)


def logits_of(c: Case, salt: int = 0) -> torch.Tensor:
    """(B, V) f32 of the family; the same for every setting of one (family, B, V, salt)"""
    g = _gen(c, salt)
    B, V = c.B, c.V
    if c.family == "equal":
        return torch.full((B, V), 1.25)
    if c.family == "gauss":
        return torch.randn(B, V, generator=g) * 3.0
    if c.family == "dominant":
        lg = torch.randn(B, V, generator=g)
        lg[torch.arange(B), torch.randint(0, V, (B,), generator=g)] += 6000.0  # weight of the rest: exp(-6000 / 100) = e^-60
        return lg
    if c.family == "neginf":
        lg = torch.full((B, V), -math.inf)
        for b in range(B):  # row 0: a single finite column; the others two and three
            cols = torch.randperm(V, generator=g)[: min(b + 1, V)]
            lg[b, cols] = torch.randn(len(cols), generator=g)
        return lg
    if c.family == "huge":
        vals = torch.tensor([3e38, -3e38, 1e38, 2.5e38, -1e30, 0.0, 3.0e38, -math.inf])
        lg = vals[torch.randint(0, len(vals), (B, V), generator=g)]
        lg[:, V // 2] = 3.4e38  # the maximum, alone
        return lg
    assert c.family == "planted"
    lg = torch.randn(B, V, generator=g) * 2.0
    lg[:, 1::5] = -math.inf
    n = min(7, V)
    for b in range(B):  # a handful of tokens 30 above the rest, anywhere in the row; two of them tie
        cols = torch.randperm(V, generator=g)[:n]
        lift = 30.0 + torch.randn(n, generator=g) * 1.5
        lg[b, cols] = lift
        if n >= 4:
            lg[b, cols[3]] = lg[b, cols[2]]
    return lg


@functools.lru_cache(maxsize=None)
def build(c: Case) -> dict:
    """inputs of the launch and the reference of every kept seed: logits, prompt, emb, postab, key_start, rows (RowRef per row),
    seeds (the first ``n_seeds`` of the scan whose decisions are all clear), picks[seed] (B,), nucleus_edge, draw_edge[seed]"""
    g = _gen(c)
    for salt in range(SALTS):  # inputs whose nucleus decisions are clear in every row, by the reference alone
        lg = logits_of(c, salt)
        rows = [row_reference(lg[b], c.topk, c.temperature, c.top_p) for b in range(c.B)]
        if min(r.nucleus_edge for r in rows) > DRAW_MARGIN:
            break
    B, V = lg.shape
    inp = dict(logits=lg, prompt=torch.randint(0, V, (B, c.P), generator=g),
               emb=torch.randn(V, c.d, generator=g).to(torch.bfloat16), postab=torch.randn(c.Ttot + 1, c.d, generator=g),
               key_start=torch.tensor([0, 2, 1, 0][:B] + [0] * max(0, B - 4), dtype=torch.int32)[:B])
    inp["rows"] = rows
    inp["nucleus_edge"] = min(r.nucleus_edge for r in rows)
    inp["seeds"], inp["picks"], inp["draw_edge"] = [], {}, {}
    if inp["nucleus_edge"] <= DRAW_MARGIN:
        return inp  # the nucleus itself is too close to call: no seed can keep the case
    for seed in range(SEED0, SEED0 + SEED_SCAN):
        picks, edge = [], math.inf
        for b, r in enumerate(rows):
            tok, e = draw(r, seed, c.pos, b)
            picks.append(tok)
            edge = min(edge, e)
            if edge <= DRAW_MARGIN:
                break
        if edge > DRAW_MARGIN:
            inp["seeds"].append(seed)
            inp["picks"][seed] = torch.tensor(picks)
            inp["draw_edge"][seed] = edge
            if len(inp["seeds"]) == c.n_seeds:
                break
    return inp


@functools.lru_cache(maxsize=None)
def kept() -> tuple:
    """the candidates of cases() for which the reference alone finds its clear seeds: the table the GPU tests run.  A candidate whose
    boundaries are denser than the margin (temperature 100 over a whole vocabulary, say) drops out here, by the reference alone;
    tests/test_sample_cases_cpu.py asserts what the kept table still covers."""
    return tuple(c for c in cases() if len(build(c)["seeds"]) == c.n_seeds)


def expected(c: Case, inp: dict, seed: int) -> dict:
    """every output of the launch: next ids, the log-probability column with its bound, the next row, position and ticket"""
    B, V, t1 = c.B, c.V, c.pos + 1
    forced = t1 < c.P
    nxt = inp["prompt"][:, t1].clone() if forced else inp["picks"][seed].clone()
    lps = [logprob(inp["logits"][b], inp["rows"][b], int(nxt[b])) for b in range(B)]
    tp = [(max(0, t1 - int(inp["key_start"][b])) if c.ragged else t1) for b in range(B)]
    x = inp["emb"].float()[nxt.clamp(0, V - 1)] + inp["postab"][torch.tensor(tp)]
    return dict(next=nxt, logprob=torch.tensor([a for a, _ in lps], dtype=torch.float64),
                bound=torch.tensor([b for _, b in lps], dtype=torch.float64), x=x, pos=t1)


# ------------------------------------------------------------------------------------- model level (tests/test_hip_sample.py)
# The sampled runs: GPT2(2, 128) and Whisper tiny with the weights of the ragged / prefill tests (ragged_cases.py), the final
# LayerNorm's gain multiplied by PEAK so that a few tokens of the 50k carry the mass - with the plain synthetic weights the
# boundaries of the running masses lie ~1e-5 apart and no draw is clear of them by DRAW_MARGIN.  Seeds are chosen HERE, on the
# CPU: tests/test_sample_cases_cpu.py replays the run with the oracle alone and asserts the share of unclear positions.
PEAK = 8.0
GPT2_RUN = dict(topk=0, temperature=0.7, top_p=0.9, seed=11, n_new=8)
WHISPER_RUN = dict(topk=0, temperature=0.4, top_p=1.0, seed=5, n_new=8)
EDGE_CAP = 0.10


def position_reference(l: torch.Tensor, run: dict, t: int, b: int):
    """(RowRef, the reference's token, the smallest edge distance of the position) for the fp32 logits row that decides position t + 1"""
    rr = row_reference(l.float(), run["topk"], run["temperature"], run["top_p"])
    tok, e = draw(rr, run["seed"], t, b)
    return rr, tok, min(e, rr.nucleus_edge)


def oracle_sampled_run(last_logits, prompt: torch.Tensor, run: dict, t_shift: int = 0, rows=None):
    """the reference decoding by itself: ``last_logits(tokens (B, L)) -> (B, V)`` fp32 rows (rules applied) that decide position L;
    the draw of new position L is keyed by cache position L - 1 + t_shift and row rows[b] (a ragged batch keeps its rows
    right-aligned: every row's first new token sits at the longest prompt's length).  Returns (tokens (B, P + n_new), edges (B, n_new))"""
    toks = prompt.clone()
    edges = []
    for _ in range(run["n_new"]):
        lg = last_logits(toks)
        t = toks.shape[1] - 1 + t_shift
        picks = [position_reference(lg[b], run, t, b if rows is None else rows[b])[1:] for b in range(toks.shape[0])]
        edges.append([e for _, e in picks])
        toks = torch.cat([toks, torch.tensor([[k] for k, _ in picks])], 1)
    return toks, torch.tensor(edges).T


RAGGED_LENGTHS = (23, 9, 1)  # of gpt2_setup()'s prompt, for the ragged sampled run


def kv_round(name, t):
    """the storage point of the decode step: the caches hold bf16 k / v"""
    return t.to(torch.bfloat16).float() if name == "kv" else t


@functools.lru_cache(maxsize=None)
def gpt2_setup():
    """(module (fp32 holder of bf16 values), state dict, prompt (3, 23)) of the peaked GPT2(2, 128)"""
    import ragged_cases as RC
    from pytorch_models.text import GPT2
    from synthweights import bf16_round_, fill_module

    m = GPT2(2, 128).eval()
    fill_module(m, RC.GPT2_SEED)
    m.norm.weight.data *= PEAK
    bf16_round_(m)
    return m, {k: v.clone() for k, v in m.state_dict().items()}, RC.gpt2_prompt()[:, :23].contiguous()


def gpt2_last_logits(sd):
    from oracle import ref_text as RX

    return lambda toks: RX.gpt2(sd, toks, rp=kv_round)[:, -1]


WHISPER_RULES = dict(eot=50257, timestamp_begin=50364, no_timestamps=50363, max_initial_timestamp=50, suppress=(1, 2, 7, 50258, 50259),
                     blank=(220, 50257))


@functools.lru_cache(maxsize=None)
def whisper_setup():
    """(module, state dict, bf16-valued memory (2, 96, 384) f32, prompt (2, 4)) of the peaked Whisper tiny"""
    import ragged_cases as RC
    from pytorch_models.audio2text import Whisper
    from synthweights import bf16_round_, fill_module, synth_input

    w = Whisper.from_openai("tiny").eval()
    fill_module(w, 55)
    w.decoder.norm.weight.data *= PEAK
    bf16_round_(w)
    memory = synth_input("prefill_memory", (2, 96, 384), 55).to(torch.bfloat16).float()
    return w, {k: v.clone() for k, v in w.state_dict().items()}, memory, RC.whisper_prompt()


def whisper_logits(sd, memory, toks: torch.Tensor, P: int, rules: bool) -> torch.Tensor:
    """(B, L, V) oracle logits of every position of ``toks`` (K/V rounded where the step rounds), after the oracle's rules"""
    from oracle import ref_whisper as RW
    from oracle import ref_whisper_rules as RR

    lg = RW.decoder(sd, "decoder.", toks, memory, rp=kv_round)
    if not rules:
        return lg
    orules = RR.Rules(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in WHISPER_RULES.items()})
    out = lg.clone()
    for b in range(toks.shape[0]):
        for t in range(P - 1, toks.shape[1]):
            out[b, t] = RR.apply(orules, lg[b, t], toks[b, P : t + 1].tolist())
    return out


def whisper_last_logits(sd, memory, P: int, rules: bool):
    return lambda toks: whisper_logits(sd, memory, toks, P, rules)[:, -1]


# --------------------------------------------------------------------------------------------- the wrapper's operand layouts
def wrapper_rows() -> dict:
    """rows for tests/wrapper_cases.check_row on pytorch_models._hip.sampling.dec_sample (the wrapper lives outside ops.py, so its rows
    live here and are not registered in wrapper_cases.ROWS): the plain form, the ragged form, and a top-k one"""
    import wrapper_cases as WC

    def build(form):
        def make(dev):
            g = WC.Gen(dev, WC.SEED + 4000)
            kw = dict(logits=g.f(2, 11), pos=g.t([3], WC.I32), prompt=g.i(11, 2, 2), tok_cur=g.i(11, 2), tokens=g.i(11, 2, 8), emb=g.b(11, 32),
                      pos_tab=g.f(9, 32), ticket=g.t([0], WC.I32), logprobs=g.z(2, 8), topk=0, temperature=0.7, top_p=0.9, seed=5)
            if form == "ragged":
                kw["key_start"] = g.t([0, 1], WC.I32)
            if form == "topk":
                kw.update(topk=3, temperature=1.0)
            return kw
        return make

    inplace = ("pos", "tok_cur", "tokens", "ticket", "logprobs")
    return {form: WC.Row(f"dec_sample:{form}", "dec_sample", build(form), inplace) for form in ("plain", "ragged", "topk")}
