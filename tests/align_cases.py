"""Reference, derived error bounds and case tables shared by the token-timestamp tests (tests/test_align_cases_cpu.py without a
GPU, tests/test_hip_align_kernels.py and tests/test_hip_align.py on one).  A plain helper, importable without a GPU.

In scope: ops.align_lse / align_matrix / align_dtw (csrc/align.hip) and WhisperDecoder.align.  Contract: DESIGN.md, "21. Token
timestamps".  OpenAI's package is not a dependency of this project: the reference below RESTATES the published algorithm
(cross-attention alignment + dynamic time warping) and parity is against this restatement, nothing is pinned to their code.

Reference (float64, from exactly the bf16 operands the kernels see, widened exactly).  Per clip b with len token rows and F frames
and per selected head:
    x[t, f] = q_t . k_f / 8,  lse[t] = log sum_{f < F} exp x,  p = exp(x - lse)                       t < len, f < F
    n = (p - mean_t p) / std_t p   biased std over t < len; a column whose rows are all equal has std exactly 0 and gives 0
                                   (the published code yields NaN there)
    med = median of 7 along f, reflect padding: index -i reads i, F - 1 + i reads F - 1 - i
    m = mean over the heads of med; entries with t >= len or f >= F are exactly 0.
    DTW on x = -m[skip_first : len - skip_last, : F] (N rows, M columns), literally the published loop (dtw_path): cost[0][0] = 0,
    other border cells +inf, the diagonal if it is strictly below both others, else the cell above if strictly below both others,
    else the cell to the left; back from (N, M) recording (i - 1, j - 1) while i > 0 and j > 0.  start[t] = the lowest frame of
    token row t on the path, -1 outside the window.  The kernels' DTW is compared with the float32 run of this loop, exactly.

Bounds (u = 2^-24; every term follows from the kernels' arithmetic, NO number measured on a kernel enters an assertion; the GPU
tests assert MARGIN = 1.5 x them for second-order terms, as tests/score_cases.py does):
  * logits: 64 products accumulated in fp32 on the MFMA: delta[t, f] = (64 + 2) u sum_k |q k| / 8 (tests/linear_cases.py).
  * lse: moves by the softmax-weighted logit error sum_f p delta; the running sum S is formed with exp(d) = v_exp_f32(d log2 e),
    relative (3 |d| + 4) u per term (tests/score_cases.py), |d| <= R = the row's logit range (+ 2 max delta); a lane adds 4 terms
    per 16-frame tile and rescales once per tile (3 R u in all, 5 u per tile), two pairwise merges (3 R + 6) u each:
    eps_S = (12 R + 9 ceil(F / 16) + 16) u; lse = m + logf(S): 8 u (|max| + |lse|).
  * p = exp(x - lse): relative rp = delta + lse_bound + (3 |x - lse| + 4) u  (THE RELATIVE ERROR OF THE DEVICE EXP), dp = p rp.
  * column mean over len rows, 8 partial sums of ceil(len / 8) terms, 3 tree steps, one division:
    dmean = mean_t dp + (ceil(len / 8) + 4) u mean.
  * deviations d = p - mean: dd = dp + dmean + u |d| (their power-of-two scaling is exact).
  * std = ||d|| / sqrt(len): |std' - std| <= ||dd|| / sqrt(len) (triangle inequality) + (ceil(len / 8) / 2 + 4) u std = dstd.
  * n = d / std: dn = dd / std + |d| dstd / (std (std - dstd)) + u |n|: THE 1 / std AMPLIFICATION of each column; infinite where
    std <= dstd.  cond = max dstd / std over the columns with std > 0 must stay below COND_MAX = 1e-2 in every case (asserted on
    the CPU on the reference alone): beyond it the bound stops saying anything about the kernel.
  * the median is 1-Lipschitz in the maximum norm: dmed = the window maximum of dn (same reflect rule).
  * head mean: dm = mean_a dmed + (A + 2) u mean_a |med| (A - 1 additions, the rounded factor 1 / A, its product, one addition per
    later launch).
Where the reference std is exactly 0 (len = 1, identical rows) the bound is 0: the kernel's value must be exactly 0.

Operand scale: q ~ N(0, 1), k ~ N(0, sigma^2) with sigma in [0.3, 1], so the logits' standard deviation over the tokens is
|k_f| sigma / 8 ~ sigma: the range synthetic Whisper weights show on the CPU, and the range in which the normalisation is well
conditioned.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass

import numpy as np
import torch

U32 = 2.0 ** -24
MARGIN = 1.5
COND_MAX = 1e-2
TILE = 26          # output frames per workgroup of pm_align_matrix_bf16 (csrc/align.hip, MT_W)
MAX_ROWS = 448
SENTINEL = 0x4B4B4B4B
POISON = 3e38
HD = 64


# ------------------------------------------------------------------------------------------------------------------ reference
def reflect_index(F: int) -> torch.Tensor:
    """(F, 7) int64: the frames the median window of each frame reads."""
    idx = torch.arange(F)[:, None] + torch.arange(-3, 4)[None, :]
    idx = idx.abs()
    return torch.where(idx > F - 1, 2 * (F - 1) - idx, idx)


def median7(n: torch.Tensor) -> torch.Tensor:
    """median of 7 along the last dim with reflect padding; F >= 4."""
    return n[..., reflect_index(n.shape[-1])].sort(-1).values[..., 3]


def window_max(e: torch.Tensor) -> torch.Tensor:
    return e[..., reflect_index(e.shape[-1])].max(-1).values


@dataclass
class Head:
    lse: torch.Tensor        # (len,)
    lse_bound: torch.Tensor  # (len,)
    med: torch.Tensor        # (len, F) filtered normalised probabilities
    dmed: torch.Tensor       # (len, F) their bound
    std: torch.Tensor        # (F,) 0 where the rows are all equal
    cond: float              # max dstd / std over the columns with std > 0 (0 if none)


def head_reference(q: torch.Tensor, k: torch.Tensor) -> Head:
    """one clip, one head: q (len, 64), k (F, 64), bf16."""
    assert q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and q.shape[1] == HD and k.shape[1] == HD
    ln, F = q.shape[0], k.shape[0]
    qd, kd = q.double(), k.double()
    x = qd @ kd.T / 8
    delta = (HD + 2) * U32 * (qd.abs() @ kd.abs().T) / 8
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[:, None])
    mx = x.max(-1).values
    R = mx - x.min(-1).values + 2 * delta.max(-1).values
    eps_s = (12.0 * R + 9.0 * math.ceil(F / 16) + 16.0) * U32
    lse_bound = (p * delta).sum(-1) + eps_s + 8 * U32 * (mx.abs() + lse.abs())
    rp = delta + lse_bound[:, None] + (3.0 * (x - lse[:, None]).abs() + 4.0) * U32
    dp = p * rp
    cl = math.ceil(ln / 8)
    mean = p.mean(0)
    dmean = dp.mean(0) + (cl + 4) * U32 * mean
    d = p - mean
    flat = p.max(0).values == p.min(0).values
    d = torch.where(flat, torch.zeros_like(d), d)
    dd = dp + dmean + U32 * d.abs()
    std = d.square().mean(0).sqrt()
    dstd = dd.square().mean(0).sqrt() + (cl / 2 + 4) * U32 * std
    live = std > 0
    s1 = torch.where(live, std, torch.ones_like(std))
    n = torch.where(live, d / s1, torch.zeros_like(d))
    room = s1 - dstd
    dn = dd / s1 + d.abs() * dstd / (s1 * room.clamp(min=1e-300)) + U32 * n.abs()
    dn = torch.where(room > 0, dn, torch.full_like(dn, math.inf))
    dn = torch.where(live, dn, torch.zeros_like(dn))
    cond = float((dstd / s1)[live].max()) if bool(live.any()) else 0.0
    return Head(lse, lse_bound, median7(n), window_max(dn), torch.where(live, std, torch.zeros_like(std)), cond)


@dataclass
class Ref:
    lse: list          # per group: (B, n, L) f64, NaN where t >= len
    lse_bound: list
    m: torch.Tensor        # (B, L, S) f64
    m_bound: torch.Tensor  # (B, L, S); 0 where the value must be exact
    cond: float
    zero_std: torch.Tensor  # (B, S) bool: every head's column std is exactly 0 there (f < F)


def reference(groups, lens, frs) -> Ref:
    """groups: [(q (B, L, H 64) bf16, k (B, S, H 64) bf16, heads), ...] - one entry per aligned layer, in launch order."""
    B, L = groups[0][0].shape[:2]
    S = groups[0][1].shape[1]
    A = sum(len(g[2]) for g in groups)
    m = torch.zeros((B, L, S), dtype=torch.float64)
    dm = torch.zeros_like(m)
    am = torch.zeros_like(m)
    zero = torch.ones((B, S), dtype=torch.bool)
    lses, lbs, cond = [], [], 0.0
    for q, k, heads in groups:
        lse = torch.full((B, len(heads), L), math.nan, dtype=torch.float64)
        lb = torch.full_like(lse, math.nan)
        for b in range(B):
            ln, F = lens[b], frs[b]
            zero[b, F:] = False
            for a, h in enumerate(heads):
                r = head_reference(q[b, :ln, HD * h : HD * h + HD], k[b, :F, HD * h : HD * h + HD])
                lse[b, a, :ln], lb[b, a, :ln] = r.lse, r.lse_bound
                m[b, :ln, :F] += r.med
                dm[b, :ln, :F] += r.dmed
                am[b, :ln, :F] += r.med.abs()
                zero[b, :F] &= r.std == 0
                cond = max(cond, r.cond)
        lses.append(lse)
        lbs.append(lb)
    return Ref(lses, lbs, m / A, dm / A + (A + 2) * U32 * am / A, cond, zero)


def dtw_path(x: np.ndarray):
    """The published loop, in the dtype of x -> (path [(i - 1, j - 1), ...] from the end to the start, cost[N][M])."""
    N, M = x.shape
    dt = x.dtype.type
    cost = np.full((N + 1, M + 1), np.inf, dtype=x.dtype)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = dt(x[i - 1, j - 1] + c)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, path = N, M, []
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return path, cost[N, M]


def dtw_start(m: torch.Tensor, lens, frs, skip_first: int, skip_last: int, dtype=np.float32) -> torch.Tensor:
    """m (B, L, S) -> start (B, L) int32 by the loop above on -m[b, skip_first : len - skip_last, : F] in ``dtype``."""
    B, L, _ = m.shape
    start = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        N = lens[b] - skip_first - skip_last
        if N <= 0:
            continue
        with np.errstate(all="ignore"):
            path, _ = dtw_path((-m[b, skip_first : skip_first + N, : frs[b]]).numpy().astype(dtype))
        for i, j in path:  # j falls along a row: the last entry of a row is its first frame
            start[b, skip_first + i] = j
    return start


def brute_force_cost(x: np.ndarray) -> float:
    """min over every monotone path from cell (0, 0) to (N - 1, M - 1) with steps (1, 1), (1, 0), (0, 1), float64."""
    N, M = x.shape
    best = [math.inf]

    def go(i, j, acc):
        acc += float(x[i, j])
        if i == N - 1 and j == M - 1:
            best[0] = min(best[0], acc)
            return
        if i + 1 < N and j + 1 < M:
            go(i + 1, j + 1, acc)
        if i + 1 < N:
            go(i + 1, j, acc)
        if j + 1 < M:
            go(i, j + 1, acc)

    go(0, 0, 0.0)
    return best[0]


def ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound over the entries where want is not NaN; an entry whose bound is 0 must be exact, a non-finite
    output is an infinite ratio."""
    keep = ~torch.isnan(want)
    g, w, b = got.double()[keep], want[keep], bound[keep]
    if not torch.isfinite(g).all():
        return math.inf
    err = (g - w).abs()
    if bool(((b == 0) & (err > 0)).any()):
        return math.inf
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if bool(nz.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------- kernel cases
@dataclass(frozen=True)
class Case:
    family: str
    B: int
    L: int
    S: int
    H: int                 # heads of the layer (inner = 64 H)
    groups: tuple          # one tuple of head indices per aligned layer
    lens: tuple
    frs: tuple
    sigma: float = 0.6
    seed: int = 0

    @property
    def id(self) -> str:
        return f"{self.family}-B{self.B}-L{self.L}-S{self.S}-h{'+'.join(str(len(g)) for g in self.groups)}"


def cases() -> list:
    T = TILE
    return [
        Case("smallest", 1, 1, 4, 1, ((0,),), (1,), (4,)),
        Case("odd", 1, 17, 67, 4, ((0, 1, 3),), (17,), (67,), seed=1),
        Case("full_width", 1, 5, 1500, 2, ((0, 1),), (5,), (1500,), seed=2),
        Case("max_rows", 1, MAX_ROWS, 70, 1, ((0,),), (MAX_ROWS,), (70,), seed=3),
        Case("ragged", 4, 21, 61, 2, ((1, 0),), (21, 1, 16, 7), (61, 4, 33, 52), seed=4),
        Case("dominant", 1, 9, 16, 2, ((0, 1),), (9,), (16,), sigma=0.3, seed=5),
        Case("flat", 2, 17, 67, 1, ((0,),), (17, 6), (67, 30), seed=6),
        Case("halo", 5, 6, T + 6, 1, ((0,),), (6, 5, 6, 4, 6), (T - 1, T, T + 1, T + 3, T + 4), seed=7),
        Case("layers", 2, 13, 40, 4, ((0, 2), (1, 2, 3)), (13, 9), (40, 31), seed=8),
    ]


def build(case: Case) -> list:
    """-> [(q (B, L, 64 H) bf16, k (B, S, 64 H) bf16, heads), ...] per aligned layer; deterministic in the case."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    out = []
    for heads in case.groups:
        q = torch.randn((case.B, case.L, HD * case.H), generator=g)
        k = torch.randn((case.B, case.S, HD * case.H), generator=g) * case.sigma
        if case.family == "flat":  # every logit exactly 0: all rows equal, every column std exactly 0
            q.zero_()
        if case.family == "dominant":  # token t: one frame 80 above the rest (q += 640 k / |k|^2 along that frame's key)
            for b in range(case.B):
                for h in heads:
                    sl = slice(HD * h, HD * h + HD)
                    for t in range(case.lens[b]):
                        kf = k[b, (3 * t + 1) % case.frs[b], sl].bfloat16().float()
                        q[b, t, sl] += 640.0 * kf / kf.square().sum()
        out.append((q.bfloat16(), k.bfloat16(), tuple(heads)))
    return out


# ------------------------------------------------------------------------------------------------------------------ DTW cases
def planted():
    """12 tokens, 3 heads: token t owns the frames [bounds[t], bounds[t + 1]) (multiples of 8); q_t and the keys of its frames share
    a one-hot direction of amplitude 6, plus N(0, 0.1^2) noise -> (q (1, 12, 192) bf16, k (1, F, 192) bf16, bounds)."""
    g = torch.Generator().manual_seed(77)
    widths = [8, 16, 8, 24, 8, 8, 16, 8, 8, 16, 8, 8]
    bounds = [0] + list(itertools.accumulate(widths))
    F = bounds[-1]
    owner = torch.repeat_interleave(torch.arange(12), torch.tensor(widths))
    q = 0.1 * torch.randn((1, 12, 3 * HD), generator=g)
    k = 0.1 * torch.randn((1, F, 3 * HD), generator=g)
    for h in range(3):
        for t in range(12):
            q[0, t, HD * h + (5 * t + h) % HD] += 6.0
        for f in range(F):
            k[0, f, HD * h + (5 * int(owner[f]) + h) % HD] += 6.0
    return q.bfloat16(), k.bfloat16(), bounds


def dtw_cases() -> list:
    """[(id, m (B, L, S) f32, lens, frs, skip_first, skip_last), ...]"""
    g = torch.Generator().manual_seed(99)

    def rnd(B, L, S):
        return torch.randn((B, L, S), generator=g)

    q, k, _ = planted()
    pm = reference([(q, k, (0, 1, 2))], (12,), (k.shape[1],)).m.float()
    ints = torch.randint(-2, 3, (3, 23, 41), generator=g).float()
    huge = torch.where(torch.rand((1, 11, 29), generator=g) < 0.5, -1e30, 1e30).float()
    return [
        ("n1", rnd(1, 1, 9), (1,), (9,), 0, 0),
        ("m4", rnd(2, 3, 4), (3, 2), (4, 4), 0, 0),
        ("n_gt_m", rnd(1, 40, 13), (40,), (13,), 0, 0),
        ("tall", rnd(1, MAX_ROWS, 64), (MAX_ROWS,), (64,), 0, 0),
        ("wide", rnd(1, 3, 1500), (3,), (1500,), 0, 0),
        ("ints", ints, (23, 23, 17), (41, 33, 41), 0, 0),
        ("const", torch.full((1, 9, 17), 0.5), (9,), (17,), 0, 0),
        ("huge", huge, (11,), (29,), 0, 0),
        ("planted", pm, (12,), (pm.shape[2],), 0, 0),
        ("ragged", rnd(5, 12, 37), (12, 5, 2, 3, 9), (37, 4, 20, 9, 36), 2, 1),
    ]


# ---------------------------------------------------------------------------------------------------------------- model level
def small_whisper(n_layers: int = 2, d: int = 128, seed: int = 58):
    """Whisper(1000, n_layers, d) with synthetic bf16-representable weights, fp32 parameters on the CPU, and its state dict."""
    from pytorch_models.audio2text import Whisper
    from synthweights import bf16_round_, fill_module

    w = Whisper(1000, n_layers, d).eval()
    fill_module(w, seed)
    bf16_round_(w)
    return w, {k: v.clone() for k, v in w.state_dict().items()}


MODEL_CASES = (("w2x128", 2, 128, 500), ("w4x256", 4, 256, 440))  # (name, layers, d_model, mel frames)
MODEL_SEED = 58
# End-to-end bound on m, bf16 model against the fp32 oracle, rel-L2: 2 x the worst figure tools/align_tolerance.py prints for the
# geometry (the oracle re-run with bf16 rounding at the HIP path's storage points, 6 seeds; DESIGN.md section 21 quotes its output)
E2E_WORST = {"w2x128": 3.7368e-02, "w4x256": 5.5586e-02}
E2E_BOUND = {k: 2 * v for k, v in E2E_WORST.items()}


def model_inputs(name: str, seed: int = MODEL_SEED):
    """-> (fp32 CPU model, state dict, mel (3, 80, T), tokens (3, 20), lens, frs) of a model-level case; ragged on both axes."""
    from synthweights import synth_input, synth_tokens

    _, n_layers, d, T = next(c for c in MODEL_CASES if c[0] == name)
    w, sd = small_whisper(n_layers, d, seed)
    S = T // 2
    return (w, sd, synth_input(f"align_mel_{name}", (3, 80, T), seed), synth_tokens(f"align_tok_{name}", (3, 20), 1000, seed),
            (20, 13, 7), (S, S - 37, S // 2 + 1))


def round_bf16(name: str, t: torch.Tensor) -> torch.Tensor:
    """rp hook: bf16 rounding at every storage point of the HIP path (each is a bf16 tensor there)."""
    return t.to(torch.bfloat16).float()


def oracle_qk(sd: dict, tokens: torch.Tensor, memory: torch.Tensor, rp=None):
    """The fp32 oracle's cross-attention projections of a teacher-forced pass: ([q_l (B, L, inner)], [k_l (B, S, inner)]) per
    decoder layer, captured at the "q" / "k" rounding points of oracle/ref_transformer.mha (each layer calls them for its self-
    attention first, its cross-attention second).  ``rp`` (name, tensor) -> tensor: further rounding, applied as the oracle does."""
    from oracle import ref_whisper

    seen = {"q": [], "k": []}

    def hook(name, t):
        t = t if rp is None else rp(name, t)
        if name in seen:
            seen[name].append(t)
        return t

    ref_whisper.decoder(sd, "decoder.", tokens, memory, rp=hook)
    return seen["q"][1::2], seen["k"][1::2]


def oracle_matrix(sd: dict, tokens, memory, heads, lens, frs, rp=None) -> torch.Tensor:
    """m (B, L, S) f64 of the reference above on the oracle's (fp32) q / k, bounds unused: the model-level tests compare in rel-L2."""
    qs, ks = oracle_qk(sd, tokens, memory, rp)
    B, L = tokens.shape
    S = memory.shape[1]
    m = torch.zeros((B, L, S), dtype=torch.float64)
    for b in range(B):
        ln, F = lens[b], frs[b]
        for l, h in heads:
            x = qs[l][b, :ln, HD * h : HD * h + HD].double() @ ks[l][b, :F, HD * h : HD * h + HD].double().T / 8
            p = torch.softmax(x, -1)
            d = p - p.mean(0)
            d = torch.where(p.max(0).values == p.min(0).values, torch.zeros_like(d), d)
            std = d.square().mean(0).sqrt()
            n = torch.where(std > 0, d / torch.where(std > 0, std, torch.ones_like(std)), torch.zeros_like(d))
            m[b, :ln, :F] += median7(n)
    return m / len(heads)


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).norm() / want.double().norm())
