"""Reference, error bounds, adversarial input families, case list and a CPU stand-in shared by the sequence-scoring parity tests
(tests/test_score_cases_cpu.py without a GPU, tests/test_hip_score_kernel.py and tests/test_hip_score.py on one).  A plain helper.

In scope: pytorch_models._hip.ops.lm_score (pm_lm_score_bf16, csrc/lm_score.hip).  Contract: DESIGN.md, "20. Sequence scoring".

Reference.  float64 on the CPU from exactly the bf16 operands the kernel sees (widened exactly): x = h w^T, lse = logsumexp(x),
logprob = x[m, t] - lse (0 where the target is -1), the LOWEST arg-max index, and A[m, v] = sum_k |h w|.

Bounds.  u = 2^-24; every term is derived from the kernel's summation shape, NO number measured on a kernel enters an assertion.
  * accumulation (tests/linear_cases.py): delta[m, v] = (K + 2) u A[m, v]; where A = 0 the logit is exact.
  * lse moves by the softmax-weighted mean of the logit errors, d lse = sum_v p_v dx_v: sum_v p_v delta[m, v].
  * the sum S = sum_v exp(x_v - max) is formed with exp(d) = v_exp_f32(d * log2 e).  With R the row's logit range (fp64 max - min,
    + 2 max delta for the device's own logits) every exponent argument has |d| <= R:
      - one term: d rounds once (u |d|), log2 e is a rounded constant (u |d|), the product rounds once (u |d|), v_exp_f32 is 1 ulp,
        counted as 2 ulp = 4 u: relative (3 R + 4) u;
      - a lane adds the 16 terms of each of the <= NC / 128 tiles of a chunk: <= 16 NC / 128 = 256 additions, 256 u;
      - a lane rescales s by exp(m_old - m_new) once per tile: each factor carries (3 |d_k| + 4) u and one product rounding; the
        maxima only grow, so sum |d_k| <= R: 3 R u + 5 u (NC / 128);
      - 3 pairwise merges per chunk (lane ^ 16, lane ^ 32, the two waves of a row): each side is scaled by one factor
        ((3 R + 4) u), multiplied (u) and added (u): 3 (3 R + 6) u;
      - the chunk merge, C = ceil(V / NC) steps in chunk order: the running side telescopes as the lane's does (3 R u + 6 u C), each
        incoming chunk is scaled once ((3 R + 6) u);
    together eps_S = (21 R + 6 C + 364) u relative on S (NC = 2048), i.e. absolute on log S.  Results of v_exp_f32 below 2^-126
    are flushed: their share of S >= 1 is below 2^-126 V and is not counted.
  * lse = m + logf(S): logf within 2 ulp of |log S| <= |lse| + |m|, the sum rounds once; logprob = x_t - lse rounds once more:
    "a few ulp" = 4 ulp = 8 u at the magnitude |m| + |lse| + |x_t| (m the row maximum).
  * logprob adds delta[m, t] for the target's own logit.  An ignored row has bound 0: it must be exactly 0.
The GPU suite asserts MARGIN = 1.5 x the bound (second-order terms); the CPU stand-in (fp32 torch in the kernel's chunked order:
per-lane online sums over the tiles of a chunk, the three pairwise merges, the chunk merge) stays inside 1.0 x.

Arg-max rule.  margin[m] = 2 max_v delta[m, v].  Where the fp64 top-2 gap of a row exceeds the margin the device index must EQUAL
the reference's; elsewhere the device's pick must be a column whose fp64 logit is within the margin of the maximum.  The cap: in
the Gaussian families at least 90 % of the rows fall under the exact rule (asserted on the CPU for the seeds used; at K = 64 the
gap is ~1e-1 against a margin of ~1e-4).  flat and ties assert their indices exactly on top of the rule.

Families (shapes: the smallest that reach each edge - M 1 / 127 / 129 / 300 around the 128-row block, K 8 / 64 / 72 / 200 / 768 =
one short K step, one whole, the zero-page tail twice, 12 steps; V 1 / 127 / 128 / 129 around a tile, NC - 1 / NC / NC + 1 around a
chunk, 2 NC + 37 = three chunks with a ragged last tile; V = 50257 once for the real tail):
  gauss   unit-variance h, w scaled so that the logits have standard deviation ~4; targets uniform.
  edges   gauss operands; targets at column 0, V - 1, the first and last column of a tile and of a chunk; a quarter of the rows -1.
  peaked  per row one column lifted ~80 above the rest (h += 80 w_v / |w_v|^2 before rounding, as attn_cases plants its peaks), in a
          chunk other than the target's: the first chunk, the last chunk, the last valid column.  logprob ~ -80.
  offset  all logits of a row near +200 or -200 (a shared component: h[:, 0] = +-16, w[:, 0] = 12.5).
  flat    h = 0: every logit exactly 0; lse = log V within the bound, logprob = -lse, argmax 0 exactly.
  ties    rows of w duplicated bit for bit across a tile boundary (127 | 128) and a chunk boundary (NC - 1 | NC); the duplicated
          logit is planted as the row maximum; argmax must be the lower index exactly.
  poison  (GPU) gauss operands as the middle slice of larger buffers with ldh > K, ldw > K; weight rows at and beyond V and hidden
          rows at and beyond M filled with 3e38, the K padding too; outputs and workspace sentinel-guarded.
  perm    (GPU) gauss operands on a fixed permutation of the rows and the first 37 rows alone: bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

U32 = 2.0 ** -24
MARGIN = 1.5
NC = 2048        # columns per vocabulary chunk (csrc/lm_score.hip; the CPU test checks it against pm_lm_score_ws_bytes)
TILE = 128
LOG2E32 = torch.tensor(1.4426950408889634, dtype=torch.float32)
FLT_MAX = 3.4028234663852886e38
SENTINEL = 0x4B4B4B4B
POISON = 3e38
MUTANTS = ("tail_unmasked", "merge_norescale", "tie_high", "last_chunk", "target_tile_off", "ignore_not_zeroed", "exp2_natural")
GAUSS_FAMILIES = ("gauss", "edges")


def nchunks(V: int) -> int:
    return (V + NC - 1) // NC


# ------------------------------------------------------------------------------------------------------------------ reference
@dataclass
class Ref:
    x: torch.Tensor        # (M, V) f64
    lse: torch.Tensor      # (M,)
    logprob: torch.Tensor  # (M,), 0 where ignored
    argmax: torch.Tensor   # (M,) int64, lowest index of the maximum
    A: torch.Tensor        # (M, V) sum_k |h w|
    delta: torch.Tensor    # (M, V) accumulation term
    gap: torch.Tensor      # (M,) fp64 top-2 gap (inf for V = 1)
    margin: torch.Tensor   # (M,) 2 max_v delta
    lse_bound: torch.Tensor
    lp_bound: torch.Tensor


def lowest_argmax(x: torch.Tensor) -> torch.Tensor:
    V = x.shape[-1]
    idx = torch.arange(V, dtype=torch.int64).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def sum_term(R: torch.Tensor, V: int) -> torch.Tensor:
    """eps_S of the module docstring: relative error of the chunked, rescaled sum (absolute on its logarithm)."""
    per_lane_adds = 16 * (NC // TILE)
    const = per_lane_adds + 4 + 5 * (NC // TILE) + 3 * 6 + 6
    return (21.0 * R + 6.0 * nchunks(V) + const) * U32


def reference(h: torch.Tensor, w: torch.Tensor, targets: torch.Tensor) -> Ref:
    assert h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    M, K = h.shape
    V = w.shape[0]
    hd, wd = h.double(), w.double()
    x = hd @ wd.T
    A = hd.abs() @ wd.abs().T
    delta = (K + 2) * U32 * A
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[:, None])
    am = lowest_argmax(x)
    live = targets >= 0
    tcl = targets.clamp(min=0)
    xt = x.gather(1, tcl[:, None])[:, 0]
    logprob = torch.where(live, xt - lse, torch.zeros_like(lse))
    top = x.topk(min(2, V), -1).values
    gap = top[:, 0] - top[:, 1] if V > 1 else torch.full((M,), math.inf, dtype=torch.float64)
    margin = 2 * delta.max(-1).values
    mx = x.max(-1).values
    R = mx - x.min(-1).values + margin
    few = 8 * U32 * (mx.abs() + lse.abs() + torch.where(live, xt.abs(), torch.zeros_like(xt)))
    lse_bound = (p * delta).sum(-1) + sum_term(R, V) + few
    lp_bound = torch.where(live, lse_bound + delta.gather(1, tcl[:, None])[:, 0], torch.zeros_like(lse_bound))
    return Ref(x, lse, logprob, am, A, delta, gap, margin, lse_bound, lp_bound)


def ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound; an element whose bound is 0 must be exact, a non-finite output is an infinite ratio."""
    if got.shape != want.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - want.double()).abs()
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def exact_rows(ref: Ref) -> torch.Tensor:
    return ref.gap > ref.margin


def argmax_ok(ref: Ref, got: torch.Tensor) -> bool:
    """The arg-max rule: equal where the fp64 gap exceeds the margin, else a column within the margin of the maximum."""
    got = got.to(torch.int64).cpu()
    V = ref.x.shape[1]
    if got.shape != ref.argmax.shape or bool(((got < 0) | (got >= V)).any()):
        return False
    ex = exact_rows(ref)
    if not torch.equal(got[ex], ref.argmax[ex]):
        return False
    picked = ref.x.gather(1, got[:, None])[:, 0]
    return bool((ref.x.max(-1).values - picked <= ref.margin)[~ex].all())


@dataclass
class Verdict:
    r_lp: float
    r_lse: float
    am_ok: bool
    exact_ok: bool

    def passed(self, factor: float) -> bool:
        return self.r_lp <= factor and self.r_lse <= factor and self.am_ok and self.exact_ok


def judge(case: "Case", ref: Ref, logprob: torch.Tensor, lse: torch.Tensor, argmax: torch.Tensor) -> Verdict:
    logprob, lse, argmax = logprob.cpu(), lse.cpu(), argmax.cpu().to(torch.int64)
    exact_ok = True
    if case.want_argmax is not None:
        exact_ok = torch.equal(argmax, case.want_argmax)
    return Verdict(ratio(logprob, ref.logprob, ref.lp_bound), ratio(lse, ref.lse, ref.lse_bound), argmax_ok(ref, argmax), exact_ok)


# --------------------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    family: str
    M: int
    V: int
    K: int
    seed: int = 0
    want_argmax: torch.Tensor | None = field(default=None, repr=False)

    @property
    def id(self) -> str:
        return f"{self.family}-M{self.M}-V{self.V}-K{self.K}"


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(1000 + seed)


def _gauss(M, V, K, g):
    h = torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) * (4.0 / math.sqrt(K))
    return h, w


def _edge_columns(V: int) -> list[int]:
    cols = [0, V - 1, TILE - 1, TILE, 2 * TILE - 1, NC - 1, NC, NC + TILE - 1, NC + TILE, 2 * NC - 1, 2 * NC,
            (V - 1) // TILE * TILE, (V - 1) // NC * NC]
    return sorted({c for c in cols if 0 <= c < V})


def _plant(h: torch.Tensor, w: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, lift: float) -> None:
    """h[rows] += lift w[cols] / |w[cols]|^2 (against the bf16 weights the kernel will see): logit (row, col) rises by ~lift."""
    wv = w.to(torch.bfloat16).float()[cols]
    h[rows] += lift * wv / (wv * wv).sum(-1, keepdim=True)


def build(case: Case):
    """(h bf16 (M, K), w bf16 (V, K), targets int64 (M)); fills case.want_argmax for the families that assert it exactly."""
    M, V, K, fam = case.M, case.V, case.K, case.family
    g = _gen(case.seed + 7 * M + 13 * V + 17 * K)
    h, w = _gauss(M, V, K, g)
    targets = torch.randint(0, V, (M,), generator=g)
    rows = torch.arange(M)
    if fam in ("gauss", "poison", "perm"):
        pass
    elif fam == "edges":
        cols = _edge_columns(V)
        targets = torch.tensor([cols[m % len(cols)] for m in range(M)], dtype=torch.int64)
        targets[rows % 4 == 3] = -1
    elif fam == "peaked":
        assert V > NC
        last0 = (V - 1) // NC * NC
        peaks = [0, NC - 1, last0, V - 1]  # first chunk (both ends), last chunk (first column), the last valid column
        pc = torch.tensor([peaks[m % 4] for m in range(M)], dtype=torch.int64)
        # the target in another chunk than the peak: peaks of the first chunk aim at the last chunk and the other way round
        lo = torch.randint(0, NC, (M,), generator=g)
        hi = last0 + torch.randint(0, V - last0, (M,), generator=g)
        targets = torch.where(pc < NC, hi, lo)
        _plant(h, w, rows, pc, 80.0)
    elif fam == "offset":
        h[:, 0] = torch.where(rows % 2 == 0, 16.0, -16.0)
        w[:, 0] = 12.5
        w[:, 1:] *= 0.5
    elif fam == "flat":
        h.zero_()
        case.want_argmax = torch.zeros(M, dtype=torch.int64)
    elif fam == "ties":
        assert V > NC
        w = w.to(torch.bfloat16).float()
        w[TILE] = w[TILE - 1]
        w[NC] = w[NC - 1]
        pc = torch.where(rows % 2 == 0, TILE - 1, NC - 1)
        _plant(h, w, rows, pc, 40.0)
        case.want_argmax = pc.clone()
    else:
        raise ValueError(fam)
    return h.to(torch.bfloat16), w.to(torch.bfloat16), targets


SHAPES = [  # (M, V, K): every M, K and V of the docstring at least once, the chunk edges at more than one M and K
    (1, 1, 8), (127, 127, 64), (129, 128, 72), (300, 129, 200), (1, NC - 1, 64), (127, NC, 8), (129, NC + 1, 64),
    (300, 2 * NC + 37, 72), (129, 2 * NC + 37, 768), (127, NC + 1, 200), (1, 2 * NC + 37, 64), (300, NC - 1, 768),
]
REAL_TAIL = (64, 50257, 64)


def cases() -> list[Case]:
    out = []
    for fam in ("gauss", "edges", "offset", "flat"):
        shapes = list(SHAPES)
        if fam == "gauss":
            shapes.append(REAL_TAIL)
        if fam == "flat":
            shapes = [s for s in SHAPES if s[2] <= 72] + [(64, 50257, 8)]
        out += [Case(fam, *s) for s in shapes]
    multi = [s for s in SHAPES if s[1] > NC]
    out += [Case("peaked", *s) for s in multi if s[2] >= 64] + [Case("peaked", *REAL_TAIL)]
    out += [Case("ties", *s) for s in multi if s[2] >= 64]
    return out


def gpu_only_cases() -> list[Case]:
    shapes = [(1, 1, 8), (127, 129, 72), (129, NC + 1, 64), (300, 2 * NC + 37, 200)]
    return [Case(f, *s) for f in ("poison", "perm") for s in shapes]


# ------------------------------------------------------------------------------------------------------------- CPU stand-in
def _E(d: torch.Tensor, natural: bool) -> torch.Tensor:
    return torch.exp2(d if natural else d * LOG2E32)


def _merge(a, b, natural: bool, rescale: bool = True):
    (ma, sa), (mb, sb) = a, b
    mn = torch.maximum(ma, mb)
    if not rescale:
        return mn, sa + sb
    return mn, sa * _E(ma - mn, natural) + sb * _E(mb - mn, natural)


def standin(h: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, mutant: str | None = None):
    """fp32 torch in the kernel's chunked order -> (logprob f32, lse f32, argmax int64).  `mutant`: one of MUTANTS, a deliberately
    wrong kernel that at least one case must catch."""
    assert mutant is None or mutant in MUTANTS
    M, K = h.shape
    V = w.shape[0]
    x = h.float() @ w.float().T
    nat = mutant == "exp2_natural"
    C = nchunks(V)
    run = None
    best_v = torch.full((M,), -math.inf)
    best_i = torch.full((M,), 2 ** 31 - 1, dtype=torch.int64)
    tg = torch.full((M,), -math.inf)
    t_look = targets + TILE if mutant == "target_tile_off" else targets
    for c in range(C - 1 if (mutant == "last_chunk" and C > 1) else C):
        c0 = c * NC
        cols = min(NC, V - c0)
        nt = (cols + TILE - 1) // TILE
        xc = torch.full((M, nt * TILE), 0.0 if mutant == "tail_unmasked" else -math.inf)
        xc[:, :cols] = x[:, c0:c0 + cols]
        # column in tile = 64 wn + 16 j + 4 fq + r -> lanes (wn, fq) own 16 columns (j, r) per tile
        xt = xc.view(M, nt, 2, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, 2, 4, nt, 16)
        m = torch.full((M, 2, 4), -FLT_MAX)
        s = torch.zeros(M, 2, 4)
        for t in range(nt):
            v = xt[:, :, :, t]
            mn = torch.maximum(m, v.max(-1).values)
            s = s * _E(m - mn, nat) + _E(v - mn[..., None], nat).sum(-1)
            m = mn
        a = _merge((m[:, :, 0], s[:, :, 0]), (m[:, :, 1], s[:, :, 1]), nat)  # lane ^ 16
        b = _merge((m[:, :, 2], s[:, :, 2]), (m[:, :, 3], s[:, :, 3]), nat)
        mw, sw = _merge(a, b, nat)                                           # lane ^ 32
        part = _merge((mw[:, 0], sw[:, 0]), (mw[:, 1], sw[:, 1]), nat)       # the two waves of a row
        run = part if run is None else _merge(run, part, nat, rescale=mutant != "merge_norescale")
        xv = x[:, c0:c0 + cols]
        cv = xv.max(-1).values
        idx = torch.arange(cols, dtype=torch.int64).expand(M, cols)
        hit = xv == cv[:, None]
        ci = (torch.where(hit, idx, torch.full_like(idx, -1)).max(-1).values if mutant == "tie_high"
              else torch.where(hit, idx, torch.full_like(idx, cols)).min(-1).values) + c0
        take = (cv >= best_v) if mutant == "tie_high" else (cv > best_v)
        best_v = torch.where(take, cv, best_v)
        best_i = torch.where(take, ci, best_i)
        inside = (t_look >= c0) & (t_look < c0 + cols)
        tv = x.gather(1, t_look.clamp(0, V - 1)[:, None])[:, 0]
        tg = torch.where(inside, tv, tg)
    mr, sr = run
    lse = mr + torch.log(sr)
    live = (targets >= 0) & (targets < V)
    if mutant == "ignore_not_zeroed":
        logprob = torch.where(live, tg, x[:, 0]) - lse
    else:
        logprob = torch.where(live, tg - lse, torch.zeros_like(lse))
    return logprob, lse, best_i


# ------------------------------------------------------------------------------------------------------------- tiny models
def small_gpt2(seed: int = 5, vocab: int = 1000, d: int = 128, layers: int = 2):
    from pytorch_models.text import GPT2
    from synthweights import bf16_round_, fill_module

    cls = type("GPT2Small", (GPT2,), {"vocab_size": vocab})
    m = cls(layers, d).eval()
    fill_module(m, seed)
    bf16_round_(m)
    return m


def small_gpt(seed: int = 6, vocab: int = 1003, d: int = 128, layers: int = 2):
    from pytorch_models.text import GPT
    from synthweights import bf16_round_, fill_module

    cls = type("GPTSmall", (GPT,), {"vocab_size": vocab})
    m = cls(layers, d).eval()
    fill_module(m, seed)
    bf16_round_(m)
    return m


def small_whisper(seed: int = 7, vocab: int = 1000, d: int = 128, layers: int = 2):
    from pytorch_models.audio2text import Whisper
    from synthweights import bf16_round_, fill_module

    m = Whisper(vocab, layers, d).eval()
    fill_module(m, seed)
    bf16_round_(m)
    return m


def small_t5(seed: int = 8, vocab: int = 1001, d: int = 128, layers: int = 2):
    from pytorch_models.text import T5Model
    from synthweights import bf16_round_, fill_module

    m = T5Model(vocab, d, 2, layers, 256).eval()
    fill_module(m, seed)
    bf16_round_(m)
    return m


def model_reference(logits: torch.Tensor, hidden: torch.Tensor, W: torch.Tensor, tokens: torch.Tensor, lengths):
    """Model level: score against fp64 log_softmax(forward) + gather from the SAME model.  forward's stored logits carry their
    own accumulation error delta (and one f32 store), the kernel's logits theirs: the tolerance is the kernel bound evaluated on
    the shared hidden rows plus forward's delta - 2 delta + the lse terms.  Returns (want (B, L - 1) f64, bound, Ref, targets)."""
    B, L = tokens.shape
    tgt = tokens[:, 1:].clone()
    if lengths is not None:
        keep = torch.arange(1, L)[None, :] < torch.as_tensor(lengths)[:, None]
        tgt[~keep] = -1
    tgt = tgt.reshape(-1)
    rows = hidden[:, :-1].reshape(B * (L - 1), -1).cpu()
    ref = reference(rows, W.cpu(), tgt)
    lg = logits[:, :-1].reshape(B * (L - 1), -1).double().cpu()
    want = torch.log_softmax(lg, -1).gather(1, tgt.clamp(min=0)[:, None])[:, 0]
    want = torch.where(tgt >= 0, want, torch.zeros_like(want))
    p = torch.softmax(lg, -1)
    fwd = (p * (ref.delta + U32 * lg.abs())).sum(-1) + (ref.delta + U32 * lg.abs()).gather(1, tgt.clamp(min=0)[:, None])[:, 0]
    bound = torch.where(tgt >= 0, ref.lp_bound + fwd, torch.zeros_like(fwd))
    return want.view(B, L - 1), bound.view(B, L - 1), ref, tgt
