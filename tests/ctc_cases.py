"""References, derived bounds and case tables shared by the CTC tests (tests/test_ctc_cases_cpu.py without a GPU,
tests/test_hip_ctc_kernels.py and tests/test_hip_ctc.py on one).  A plain helper, importable without a GPU.

In scope: ops.ctc_head / ctc_greedy / ctc_forward / ctc_viterbi (csrc/ctc.hip) and audio.Wav2Vec2CTC.  Contract: DESIGN.md,
"CTC heads".  u = 2^-24; NO number measured on a kernel enters an assertion; the GPU suite asserts MARGIN = 1.5 x a bound
(second-order terms).

Head (float64 from exactly the bf16 operands, widened): x = h w^T + bias, lse = logsumexp(x), logp = x - lse, the LOWEST arg-max.
  * logits (tests/linear_cases.py): K products summed in fp32 on the MFMA, (K + 2) u A with A[m, v] = sum_k |h w|; the bias add
    rounds once more, u (A + |bias|): delta[m, v] = (K + 3) u (A + |bias|).  Where that is 0 the logit is exact.
  * lse moves by the softmax-weighted mean of the logit errors: sum_v p_v delta[m, v] (tests/score_cases.py).
  * S = sum_v exp(x_v - max), exp(d) = v_exp_f32(d * log2 e): d rounds once (u |d|), log2 e is a rounded constant (u |d|), the
    product rounds once (u |d|), v_exp_f32 is 1 ulp, counted as 2 ulp = 4 u: term v is relative (3 |d_v| + 4) u, so S is relative
    sum_v p_v (3 |d_v| + 4) u with |d_v| <= max - x_v + 2 max delta; a lane adds its <= 64 terms and two exchanges follow:
    66 additions, 66 u.  Relative on S = absolute on log S.  Terms below 2^-126 are flushed: not counted.
  * lse = max + logf(S): logf within 2 ulp and the sum rounds once: 4 u (|max| + |lse|); logp = x - lse rounds once: 2 u |logp|.
  logp_bound[m, v] = delta[m, v] + lse_bound[m] + 2 u |logp[m, v]|.
  Arg-max: exact wherever the float64 top-two gap exceeds margin[m] = 2 max_v delta[m, v]; at most 5 % of a case's rows may be
  excluded that way (asserted on the reference alone by the CPU test).  The exact family (small-integer h, w, bias: every partial
  sum an integer below 2^24) has delta = 0 in effect: best must be exact on every row, ties to the lowest index.

Greedy: the three-line numpy collapse below.  path_logp: thread i adds ceil(T / 256) terms, the butterfly 6, the wave sums 3:
  |error| <= (ceil(T / 256) + 9) u sum_t |best_logp[t]|.

Forward (float64 alpha recursion on the KERNEL's fp32 logp, widened - the stage is judged alone).  One step of one state is
  a' = m + log(S) + e, S = exp(a - m) + exp(b - m) + exp(c - m), m the maximum (its term is exp(0) = 1 exactly, S in [1, 3]).
  * each other term: relative (3 |d| + 4) u on exp(-|d|), i.e. absolute (3 |d| + 4) exp(-|d|) u <= 4 u; two of them: 8 u; two
    additions of sums <= 3: 6 u.  S >= 1, so log S moves by <= 14 u.
  * log(S) = v_log_f32(S) * ln 2: 1 ulp counted as 2 ulp of log2 S <= 1.585 is 4 u, times ln 2: 2.8 u; the rounded constant and
    the product rounding, 2 u log 3 = 2.2 u: 5 u.
  * m + log S rounds once, u (A_{t-1} + 1.1), and + e once more, u A_t, with A_t = max_s |alpha_t(s)| over the finite states.
  logsumexp is monotone and moves by at most the largest move of its arguments, so the errors of a step ADD to the largest error
  of the step before: bound(T) = sum_{t = 1}^{T - 1} (19 u + u (A_{t-1} + 1.1) + u A_t) + 19 u + u (|loglik| + 1.1) for the
  final merge of the last two states.  Frame 0 copies logp: exact.  A state that is -inf in the reference is -inf on the device
  (its predecessors are): an infeasible pair must give exactly -inf, the one-hot families exactly 0.0 or -inf.

Viterbi: no bound.  start, stop and score must EQUAL the float32 loop below (one max, one add per state and frame, the tie rule:
  stay if not below the others, else s - 1 if not below s - 2, else s - 2; at the end the final blank unless the last label state
  is strictly above it).  Its score can never exceed the log-likelihood of the same logp (a sum contains its largest term).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

U32 = 2.0 ** -24
MARGIN = 1.5
MAX_U = 511
WORD_FRAMES = 16    # back-pointer codes per 32-bit word (csrc/ctc.hip CT_FB)
THREAD_STATES = 4   # extended states per thread of the recursion kernels
EXCLUDED_CAP = 0.05


# ------------------------------------------------------------------------------------------------------------------------ head
HEAD_M = (1, 15, 16, 17, 63, 65, 130)
HEAD_V = (2, 16, 17, 29, 32, 33, 256)
HEAD_K = (8, 64, 72, 136, 768)
HEAD_FAMILIES = ("scale1", "scale30", "lead", "exact")


@dataclass
class HeadCase:
    family: str
    M: int
    V: int
    K: int
    bias: bool

    @property
    def id(self) -> str:
        return f"{self.family}-M{self.M}-V{self.V}-K{self.K}-{'bias' if self.bias else 'nobias'}"


def head_cases() -> list[HeadCase]:
    """every M x three V, every V x three M, every K, both bias settings - per family"""
    out = []
    for fam in HEAD_FAMILIES:
        for s in range(3):
            for i, M in enumerate(HEAD_M):
                out.append(HeadCase(fam, M, HEAD_V[(i + 2 * s + 1) % 7], HEAD_K[(i + 2 * s) % 5], bool((i + s) % 2)))
    return out


def head_build(c: HeadCase):
    """(h bf16 (M, K), w bf16 (V, K), bias f32 (V) | None)"""
    g = torch.Generator().manual_seed(4000 + 7 * c.M + 13 * c.V + 17 * c.K + HEAD_FAMILIES.index(c.family))
    M, V, K = c.M, c.V, c.K
    if c.family == "exact":
        h = torch.randint(-3, 4, (M, K), generator=g).float()
        w = torch.randint(-3, 4, (V, K), generator=g).float()
        if V >= 4:
            w[V - 1] = w[1]  # a duplicated column: ties between 1 and V - 1 wherever it wins
        b = torch.randint(-4, 5, (V,), generator=g).float()
        if V >= 4:
            b[V - 1] = b[1]
        return h.to(torch.bfloat16), w.to(torch.bfloat16), b if c.bias else None
    scale = 30.0 if c.family == "scale30" else 1.0
    h = torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) * (scale / math.sqrt(K))
    b = torch.randn(V, generator=g) * scale if c.bias else None
    if c.family == "lead":  # column 0 (even rows) or V - 1 (odd rows) leads by 14 * 10 = 140 through two features of their own
        rows = torch.arange(M)
        w[:, :2] = 0.0
        w[0, 0] = w[V - 1, 1] = 10.0
        h[:, 0] = torch.where(rows % 2 == 0, 14.0, 0.0)
        h[:, 1] = torch.where(rows % 2 == 0, 0.0, 14.0)
    return h.to(torch.bfloat16), w.to(torch.bfloat16), b


@dataclass
class HeadRef:
    x: torch.Tensor
    logp: torch.Tensor
    best: torch.Tensor
    gap: torch.Tensor
    margin: torch.Tensor
    logp_bound: torch.Tensor


def lowest_argmax(x: torch.Tensor) -> torch.Tensor:
    V = x.shape[-1]
    idx = torch.arange(V, dtype=torch.int64).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def head_reference(h: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None) -> HeadRef:
    assert h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    K = h.shape[1]
    hd, wd = h.double(), w.double()
    bd = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    x = hd @ wd.T + bd
    delta = (K + 3) * U32 * (hd.abs() @ wd.abs().T + bd.abs())
    lse = torch.logsumexp(x, -1)
    logp = x - lse[:, None]
    p = logp.exp()
    mx = x.max(-1).values
    margin = 2 * delta.max(-1).values
    d = (mx[:, None] - x) + margin[:, None]
    eps_s = (p * (3 * d + 4)).sum(-1) * U32 + 66 * U32
    lse_bound = (p * delta).sum(-1) + eps_s + 4 * U32 * (mx.abs() + lse.abs())
    top = x.topk(2, -1).values
    return HeadRef(x, logp, lowest_argmax(x), top[:, 0] - top[:, 1], margin, delta + lse_bound[:, None] + 2 * U32 * logp.abs())


def ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound; an element whose bound is 0 must be exact, a non-finite output is an infinite ratio."""
    if got.shape != want.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - want.double()).abs()
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------- greedy
def collapse(a: np.ndarray, blank: int):
    """(ids, first frames) of one clip's arg-max sequence: repeats merged, blanks removed"""
    keep = (a != blank) & np.r_[True, a[1:] != a[:-1]][: len(a)]
    f = np.nonzero(keep)[0]
    return a[f], f


GREEDY_T = (0, 1, 64, 65, 300)


def greedy_batches(blank: int = 0, V: int = 7):
    """name -> list of per-clip int32 arg-max sequences (packed by the caller)"""
    g = np.random.default_rng(77)
    rnd = [g.integers(0, V, T).astype(np.int32) for T in GREEDY_T]
    wave = np.full(130, blank, dtype=np.int32)
    wave[60:70] = 3  # one token across the wave boundary 63 | 64
    wave[127:130] = 5
    tail = np.full(65, 4, dtype=np.int32)  # ends on label 4 ..
    head = np.full(64, 4, dtype=np.int32)  # .. and the next clip starts on it: two tokens, one per clip
    return {
        "random": rnd,
        "all_blank": [np.full(T, blank, dtype=np.int32) for T in GREEDY_T],
        "one_label": [np.full(T, 2, dtype=np.int32) for T in GREEDY_T],
        "alternating": [np.where(np.arange(T) % 2 == 0, 5, blank).astype(np.int32) for T in GREEDY_T],
        "boundaries": [wave, tail, head, np.zeros(0, dtype=np.int32), head[:1]],
    }


def path_bound(blp: np.ndarray) -> float:
    return (math.ceil(max(len(blp), 1) / 256) + 9) * U32 * float(np.abs(blp.astype(np.float64)).sum())


# ------------------------------------------------------------------------------------------------------------------- recursion
def extended(target, blank: int) -> np.ndarray:
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = target
    return ext


def _skip(ext: np.ndarray, blank: int) -> np.ndarray:
    skip = np.zeros(len(ext), dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return skip


def alpha_reference(logp: np.ndarray, target, blank: int):
    """(log-likelihood, bound) in float64: the literal alpha recursion over the extended labels and the bound of the docstring"""
    lp = np.asarray(logp, dtype=np.float64)
    T = lp.shape[0]
    ext = extended(target, blank)
    S = len(ext)
    skip = _skip(ext, blank)
    a = np.full(S, -np.inf)
    a[:2] = lp[0, ext[:2]]
    bound = 0.0

    def amax(v):
        f = v[np.isfinite(v)]
        return float(np.abs(f).max()) if f.size else 0.0

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(1, T):
            prev = amax(a)
            p1 = np.r_[-np.inf, a[:-1]]
            p2 = np.where(skip, np.r_[-np.inf, -np.inf, a[:-2]][:S], -np.inf)
            m = np.maximum(a, np.maximum(p1, p2))
            fin = np.isfinite(m)
            mm = np.where(fin, m, 0.0)
            a = np.where(fin, mm + np.log(np.exp(a - mm) + np.exp(p1 - mm) + np.exp(p2 - mm)), -np.inf) + lp[t, ext]
            bound += (19 + prev + 1.1 + amax(a)) * U32
        ll = np.logaddexp(a[-1], a[-2]) if S > 1 else a[-1]
    if np.isfinite(ll):
        bound += (19 + abs(ll) + 1.1) * U32
    return float(ll), bound


def viterbi_reference(logp: np.ndarray, target, blank: int):
    """(start (U), stop (U), score) of the float32 loop with the documented tie rule; -1 / -inf for an infeasible pair"""
    lp = np.asarray(logp, dtype=np.float32)
    T = lp.shape[0]
    ext = extended(target, blank)
    S, U = len(ext), len(target)
    skip = _skip(ext, blank)
    ninf = np.float32(-np.inf)
    v = np.full(S, ninf, dtype=np.float32)
    v[:2] = lp[0, ext[:2]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        p1 = np.r_[ninf, v[:-1]].astype(np.float32)
        p2 = np.where(skip, np.r_[ninf, ninf, v[:-2]][:S], ninf).astype(np.float32)
        stay = (v >= p1) & (v >= p2)
        one = ~stay & (p1 >= p2)
        bp[t] = np.where(stay, 0, np.where(one, 1, 2))
        v = (np.where(stay, v, np.where(one, p1, p2)).astype(np.float32) + lp[t, ext]).astype(np.float32)
    start, stop = np.full(U, -1, dtype=np.int32), np.full(U, -1, dtype=np.int32)
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    if not v[s] > ninf:
        return start, stop, ninf
    score = v[s]
    for t in range(T - 1, -1, -1):
        if s & 1:
            if stop[s >> 1] < 0:
                stop[s >> 1] = t + 1
            start[s >> 1] = t
        if t:
            s -= int(bp[t, s])
    return start, stop, score


REC_V = 9
REC_BLANK = 0
REC_U = (0, 1, 2, 31, 32, 33, 127, 128, 129, 511)


@dataclass
class RecCase:
    kind: str      # "random" targets (with repeats) or "repeat": one repeated label
    U: int
    T: int

    @property
    def id(self) -> str:
        return f"{self.kind}-U{self.U}-T{self.T}"


def repeats(target) -> int:
    t = np.asarray(target)
    return int((t[1:] == t[:-1]).sum()) if len(t) > 1 else 0


def rec_target(kind: str, U: int) -> np.ndarray:
    if kind == "repeat":
        return np.full(U, 3, dtype=np.int64)
    g = np.random.default_rng(500 + U)
    t = g.integers(1, REC_V, U)
    if U >= 2:
        t[U // 2] = t[U // 2 - 1]  # at least one repeat
    return t.astype(np.int64)


def rec_cases() -> list[RecCase]:
    """U x T in {1, U, U + repeats (just feasible), U + repeats - 1 (infeasible), 100, 1000}, random and one-label targets"""
    out, seen = [], set()
    for kind in ("random", "repeat"):
        for U in REC_U:
            need = U + repeats(rec_target(kind, U))
            for T in (1, U, need, need - 1, 100, 1000):
                if T >= 1 and (kind, U, T) not in seen and (kind == "random" or U >= 2):
                    seen.add((kind, U, T))
                    out.append(RecCase(kind, U, T))
    return out


def rec_logp(c: RecCase, scale: float = 2.0) -> np.ndarray:
    """f32 (T, V) log-probabilities (a log_softmax of Gaussians: what the head would hand on)"""
    g = torch.Generator().manual_seed(9000 + 31 * c.U + c.T + (0 if c.kind == "random" else 5))
    return torch.log_softmax(torch.randn(c.T, REC_V, generator=g) * scale, -1).numpy()


def feasible(target, T: int) -> bool:
    return T >= len(target) + repeats(target)


def one_hot_logp(frames, V: int = REC_V) -> np.ndarray:
    """0 for the given label of each frame, -inf elsewhere"""
    lp = np.full((len(frames), V), -np.inf, dtype=np.float32)
    lp[np.arange(len(frames)), frames] = 0.0
    return lp


ONE_HOT = [  # (frame labels, target, is the target the collapse of the frames)
    ([3, 3, 0, 3, 5], [3, 3, 5], True),      # a repeated label with the blank between
    ([3, 3, 3, 5, 5], [3, 5], True),         # .. and without: one token
    ([3, 3, 3, 5, 5], [3, 3, 5], False),
    ([0, 0, 4, 4, 2], [4, 2], True),         # a leading blank
    ([4, 2, 2, 0, 0], [4, 2], True),         # a trailing blank
    ([0, 4, 0, 2, 0], [4, 2], True),
    ([4, 0, 2], [2, 4], False),
    ([0, 0, 0], [], True),
    ([0, 1, 0], [], False),
]


# ------------------------------------------------------------------------------------------------------------------------ model
MODEL_LENGTHS = [9600, 6400, 4000, 400]
MODEL_V = 32
HEAD_GAIN = 8.0  # the synthetic lm_head is scaled up so that the log-probabilities are not a constant (see model_ctc)


def model_ctc(seed: int = 82):
    """Wav2Vec2CTC(Wav2Vec2(2, 128), 32) on synthweights, bf16-rounded, and its fp32 state dict.  synthweights fills a Linear with
    O(1 / sqrt(d)) weights: logits of scale ~0.1 would make every log-probability ~ -log 32, and a rel-L2 against the oracle would
    pass whatever the hidden rows were.  The head's weights are scaled by HEAD_GAIN instead (the tolerance stays 2e-2); the CPU test
    checks that a 2e-2 perturbation of the hidden rows then moves the log-probabilities by a comparable amount."""
    from pytorch_models.audio import Wav2Vec2, Wav2Vec2CTC
    from synthweights import bf16_round_, fill_module

    m = Wav2Vec2CTC(Wav2Vec2(2, 128), MODEL_V).eval()
    fill_module(m, seed)
    with torch.no_grad():
        m.lm_head.weight.mul_(HEAD_GAIN)
        m.lm_head.bias.mul_(HEAD_GAIN)
    bf16_round_(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m, sd


def model_targets():
    """(targets int64 (4, 6), target_lengths) for the clips of 29, 19, 12, 1 frames: feasible rows, one of length 0"""
    t = torch.tensor([[5, 5, 9, 1, 30, 2], [7, 8, 8, 3, 0, 0], [4, 31, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    return t, [6, 4, 2, 0]
