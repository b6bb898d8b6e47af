"""References, error bounds, adversarial input families, case lists and a CPU stand-in kernel shared by the GEMM / LayerNorm-fold
parity tests (tests/test_linear_cases_cpu.py without a GPU, tests/test_hip_linear_adversarial.py and its child script
tests/linear_child.py on one).  A plain helper module.

In scope (through pytorch_models._hip.ops): linear - every dispatch target of pm_linear_bf16 that ships (1 = 128 x 128, 2 = persistent
256 x 128, 3 = 256 x 256, 6 / 7 = (64 MI) x 256 tiles of 256 / 320 rows), out_dtype bf16 / f32, residual bf16 / f32, resid_period,
the window form (linear_strided), ln_stats / ln_s (the fold's consumer), want_row_stats (its producer) -, ln_stats_finalize,
linear_f32 (plain and window form), layernorm (with GELU and a residual), row_stats.
Out of scope: the stream-K / hybrid experiments (ids 4, 5: experiments build only, they keep tests/test_hip_kernels.py's check),
pm_dec_linear* (tests/test_hip_decode.py), rmsnorm, geglu, the mixer token-mix kernel.

Contract ("2d. GEMM and LayerNorm-fold numerics contract").

Reference.  float64 on the CPU from exactly the operands the kernel sees (bf16 operands are bf16 tensors, widened exactly), in the
order read off the kernels: z = x w^T + bias, y = act(z) + resid, ONE rounding at the store.  The fold's consumer is
z = rstd (x W'^T - mean s) + c from the f32 stats, s and c it is given (c travels in the bias argument).  erf-GELU is
0.5 z erfc(-z / sqrt 2) (no cancellation for z << 0).  Row partials are the sum and the sum of squares of the ROUNDED outputs per
64-feature block: they are checked against the float64 sums of the y the kernel itself stored.  Beside `want` the reference returns
A = sum |x w| + |bias| (consumer: |rstd| (sum |x W'| + |mean s|) + |c|), z, and the bound.

Bounds.  u = 2^-24; every term is derived, NO number measured on a kernel enters an assertion (and no term is measured against the
reference either: the non-PRECISE SiLU branch follows from the 1-ulp v_exp_f32, see below):
  * fp32 accumulation of K terms in any order: delta = (K + 2) u A.  The consumer's A carries the cancellation of
    acc - mean s and its amplification by |rstd|: the product mean s, the subtraction and the fma round once each, inside the + 2;
    where sum |x w| = 0 the accumulation and 0 + bias are exact: delta = 0 (the actsweep family's pre-activations are exact);
  * store: half a bf16 ulp of want, 2^(floor(log2 |want|) - 8), or u |want| to f32 (2c); a residual add rounds once more: + u |want|;
  * none / ReLU: 1-Lipschitz, delta passes through;
  * GELU-tanh 1.13 delta + u (4 |z| + 2 |g|), PRECISE SiLU 1.10 delta + 4 u |s| (2c);
  * erf-GELU with erff (f32 outputs, layernorm): 1.13 delta + u (6 |z| + 2 |g|).  The argument z / sqrt 2 carries 2 u relative and
    |a erf'(a)| <= 0.49: 1 u on erf; erff <= 4 ulp of a value <= 1 (HIP's documented figure): 8 u; 1 + erf rounds once: 2 u; together
    11 u on the factor, times |z| / 2, rounded up; absolute in z because 1 + erf cancels for z << 0; two outer products: 2 u |g|;
  * gelu_poly / gelu_poly2 (bf16 outputs): 1.13 delta + 3.7e-5, the absolute error csrc/common.h states for all finite x;
  * non-PRECISE SiLU z / (1 + __expf(-z)) (bf16 outputs): __expf(a) = v_exp_f32(a log2 e): the product and the constant carry 2 u |a|
    into the exponent, the instruction 1 ulp = 2 u: e is off by 2 u (|z| + 1) relative; ds/de e = s e / (1 + e) = s sigma(-z); the add
    and the IEEE division round once each: 1.10 delta + u |s| (2 sigma(-z) (|z| + 1) + 2);
  * both SiLU forms: exp(-z) overflows fp32 for z < -88.7 and the result is -0: + |s| there (< 2.6e-37);
  * every activation but none / ReLU: + 2^-126 (results below the smallest normal may be flushed);
  * row partials: 64 terms, (64 + 2) u sum |y| and (64 + 2) u sum y^2;
  * ln_stats_finalize, the one-pass design: with S1, S2 the np = N / 64 partials summed in fp32, d_mean = (np + 2) u sum |p1| / N,
    d_var = (np + 2) u sum p2 / N + 2 |mean| d_mean + u (mean^2 + |var|), d_rstd = rstd (d_var / (2 (var + eps)) + 3 u) (rsqrtf 1 ulp,
    the add): the bound carries the conditioning (mean^2 + var) / (var + eps) - rows at |mean| / sigma = 256 keep 4 digits of rstd;
  * layernorm / row_stats, two passes (2c): e = d u mean |x|, |d_mean| <= e, d_rstd <= rstd (e / sigma + 3 u),
    |d_y| <= |gamma| / sigma (2 + |yhat|) e + 3 u |y|, then GELU (erff), the residual add and the store as above.
The GPU suite asserts MARGIN = 1.5 x the bound (second-order terms); an element whose bound is 0 must be exact; a non-finite
output is an infinite ratio (ratio()).  The CPU stand-in (fp32 torch in its own summation order) stays inside 1.0 x.

Guarantees beside the bound.  Single rounding: the exact family's residual cases make act(z) + resid round ONCE.  Permutation: a row's
result does not depend on where the row sits in the batch - running on x[p] (resid[p], stats[p]) gives y[p] bit for bit.

Families.
  exact    x, w integers in [-a, a] (x half zeros, a from K so that sigma(z) ~ 250), bias / resid integers in [-64, 64]; the consumer
           gets an integer mean, a power-of-two rstd (1/2, 1, 2) and integer s, c.  Every partial sum stays below 2^24: the output must EQUAL
           want.to(out dtype) and the row partials the exact sums.  >= 10 % of a case's pre-residual values exceed 256 in magnitude
           (asserted on the CPU): a rounding before the residual add is then a bit difference.  w differs along n and k.
  cancel   real operands, zero-sum weight rows on x = 1 + small noise: |want| << A.  By the bound.
  offset   consumer: rows at |mean| / sigma = 1, 16, 256 (row m takes ratio m % 3), stats from float64; finalize: the same ratios;
           layernorm / row_stats: |mean| / sigma = 4096, d <= 192 (the factor d makes the family toothless beyond, as in 2c).
  poison   Gaussian operands; every operand (x, w, bias, resid, stats, s and y itself) the middle slice of a larger 16-byte-aligned
           buffer with ldx > K, ldw > K, ldr > N, ldy > N; inputs surrounded by NaN (the window form: also every element between
           batches that no window row covers), y by a sentinel bit pattern.  Finite, bit-identical
           to the run on plain copies, inside the bound.  (EVERY run of every family writes into a sentinel-guarded y: all of
           columns N .. ldy and the rows before and after must be unchanged.)
  perm     Gaussian operands, a fixed random permutation of the rows: y[p] bit for bit.  Ids 1, 2, 3, 6, 7 and linear_f32.
  actsweep x = 0, w = 0, bias = sweep(): the pre-activation is any fp32 value exactly.  A grid of step 1/16 on [-12, 12], the 17
           neighbours of +-4.5, +-0, +-2^-126, +-20, +-100, +-1000, +-65000 and -90 (SiLU's overflow).  All five activations, bf16
           and f32 outputs, each by its bound; every row equals row 0; the GELU rows of ids 2, 3, 6, 7 equal id 1's bit for bit
           (gelu_poly2 claims bit-identity with gelu_poly).

Path -> case (the smallest shapes that reach each path; paths() derives the tags from the shape with the launchers' own arithmetic,
the CPU test asserts REQUIRED_PATHS and, with the library built, that pm_linear_bf16_plan sends every case to its kernel):
  id 1   M = 1, 127, 128, 129; K = 8, 64 (nk = 1), 72, 200 (zero-page tail), 128; N = 8 / 12 / 9 / 130 (16-byte, 8-byte, scalar
         stores, two tile columns); <ACT, YF32> corners; window x with a batch boundary inside a tile; resid_period 5
  id 2   M = 4096, 4104, 4097; N = 8, 136; K = 64 (nk = 1), 128; staged (bf16 out, bf16 resid) / direct (f32 out, f32 resid) epilogue;
         consumer + residual; row partials N = 64, 320; 258 tiles on 256 workgroups (M = 65800)
  id 3   M = 4097 and window x (the default dispatcher's reasons to take it: M = 4097 / window at N = 2048); N = 8, 264; K = 64, 128;
         plain / GELU / residual / consumer
  id 6/7 M = 4096, N = 8, K = 64 (16 / 13 tiles: most workgroups idle, nk = 1); M = 4616, N = 264 (tiles_m % 4 != 0, two tile
         columns); N = 520; M = 82248, N = 8, K = 128 (322 / 258 tiles: two per workgroup); the three epilogue modes; row partials
         N = 64, 320 with and without residual; consumer with and without GELU
  finalize    N / 64 = 1, 2, 3, 4, 6, 16 (odd loop, np % 4 == 2, whole trips); M = 1, 255, 256, 257
  linear_f32  M = 1, 127, 128, 129; N = 1, 5, 128, 130; K = 1, 3, 16, 17, 35; window form; resid_period; every activation
  layernorm / row_stats  d = 8, 64, 192, 768, 1280, 4096; M = 1, 3, 4, 5; bf16 / f32 in and out; GELU + residual; strided rows
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

U32 = 2.0 ** -24
BF16_BITS = 8
GELU_LIP = 1.13
SILU_LIP = 1.10
GELU_POLY_ABS = 3.7e-5  # csrc/common.h: |gelu_poly(x) - x Phi(x)| for all finite x
TINY = 2.0 ** -126
MARGIN = 1.5
EPS = 1e-5
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
ACTS = ("none", "gelu", "approximate_gelu", "relu", "silu")
FORCED_IDS = (2, 3, 6, 7)
SENTINEL = {"bf16": 0x4B4B, "f32": 0x4B4B4B4B}
MUTANTS = ("ktail", "biaslane", "residrow", "padstore", "trunc", "round_first", "resid_first", "lns_shift", "meanrstd",
           "rows_unrounded", "rows_block", "onepass", "fin_drop", "kswap", "tileswap", "gelu_tail")


# --------------------------------------------------------------------------------------------------------------- small helpers
def store_term(want: torch.Tensor, dt: str) -> torch.Tensor:
    """The error of one correctly rounded store of `want`: half a bf16 ulp, 2^(floor(log2 |want|) - 8), or 2^-24 |want| to f32."""
    a = want.double().abs().nan_to_num(0.0)
    if dt != "bf16":
        return U32 * a
    _, ex = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), ex - 1 - BF16_BITS), torch.zeros_like(a))


def store(v: torch.Tensor, dt: str, trunc: bool = False) -> torch.Tensor:
    """The value a correct kernel stores: round to nearest even.  trunc: the deliberately wrong bf16 conversion."""
    v32 = v.float()
    if dt == "bf16" and trunc:
        return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return v32.to(DT[dt])


def ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound; an element whose bound is 0 must be exact, a non-finite output is an infinite ratio."""
    if got.shape != want.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - want.double()).abs()
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit patterns of a bf16 / f32 tensor as integers (NaN-safe comparisons)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sweep() -> torch.Tensor:
    """The actsweep pre-activations, f32 (432 values: a multiple of 8, so the 256-wide kernels take it as N)."""
    grid = torch.arange(-192, 193, dtype=torch.float64) / 16.0
    k = torch.arange(-8, 9, dtype=torch.float64)
    near = 4.5 * (1.0 + k * 2.0 ** -23)  # the 17 fp32 neighbours of 4.5 (4.5 itself at k = 0)
    special = torch.tensor([0.0, -0.0, TINY, -TINY, 20.0, -20.0, 100.0, -100.0, 1000.0, -1000.0, 65000.0, -65000.0, -90.0], dtype=torch.float64)
    s = torch.cat([grid, near, -near, special]).float()
    assert s.numel() == 432
    return s


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    """One problem.  op: linear | linear_f32 | finalize | layernorm | row_stats.  kid: the pm_linear_bf16 kernel the case is aimed at
    (0 for the other ops); forced: it needs PM_GEMM_KERNEL=kid (a child process), else the default dispatcher must pick kid."""
    op: str
    family: str
    M: int
    N: int
    K: int = 0                  # layernorm / row_stats / finalize: unused (N is d)
    kid: int = 0
    forced: bool = False
    act: str = "none"
    ydt: str = "bf16"
    xdt: str = "bf16"           # layernorm / row_stats input
    bias: bool = True
    resid: str | None = None    # "bf16" | "f32"
    period: int = 0
    window: int = 0             # rows per batch of the window form (0: plain rows)
    consumer: bool = False
    rows: bool = False          # want_row_stats
    strided: bool = False       # layernorm / row_stats: ldx > d
    far: str = ""               # far family: "<x | w | resid | residp | y | win>:<2G | 4G | 8G>" - the operand placed far, the distance

    @property
    def id(self) -> str:
        s = f"{self.op}{self.kid or ''}-{self.family}-{self.M}x{self.N}" + (f"x{self.K}" if self.K else "")
        s += f"-{self.xdt}-{self.ydt}" if self.op in ("layernorm", "row_stats") else f"-{self.ydt}"
        s += ("" if self.bias else "-nob") + (f"-r{self.resid}" if self.resid else "") + (f"-p{self.period}" if self.period else "")
        s += (f"-win{self.window}" if self.window else "") + ("-lnc" if self.consumer else "") + ("-rows" if self.rows else "")
        s += ("-ld" if self.strided else "") + (f"-{self.act}" if self.act != "none" else "")
        return s + (f"-{self.far.replace(':', '')}" if self.far else "")

    @property
    def fast_act(self) -> bool:
        """bf16 outputs of pm_linear_bf16 take the non-PRECISE activation forms (gelu_poly, __expf)."""
        return self.op == "linear" and self.ydt == "bf16"


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def window_geometry(case: Case) -> tuple[int, int, int]:
    """(row_stride, batch_stride, buffer elements) of a window-form case: overlapping rows (stride 16 < K where K > 16), batches a
    ragged distance apart.  Both strides are multiples of 8 (bf16) and of 4 (f32)."""
    R = case.window
    rs = 16 if case.K > 16 else 24
    bs = (R - 1) * rs + case.K + 40
    bs += -bs % 8
    nb = case.M // R
    return rs, bs, (nb - 1) * bs + (R - 1) * rs + case.K


def window_index(case: Case) -> torch.Tensor:
    """(M, K) element indices of the window form's rows in the flat buffer."""
    rs, bs, _ = window_geometry(case)
    m = torch.arange(case.M)
    base = (m // case.window) * bs + (m % case.window) * rs
    return base[:, None] + torch.arange(case.K)[None, :]


def tile_rows(kid: int) -> int:
    return {1: 128, 2: 256, 3: 256, 6: 256, 7: 320}[kid]


def tile_cols(kid: int) -> int:
    return 128 if kid in (1, 2) else 256


def paths(case: Case) -> set[str]:
    """The kernel paths a case reaches, derived from its shape with the launchers' own arithmetic."""
    t: set[str] = set()
    M, N, K = case.M, case.N, case.K
    if case.op == "linear":
        k = f"id{case.kid}"
        tm, tn = -(-M // tile_rows(case.kid)), -(-N // tile_cols(case.kid))
        t.add(k)
        t.add(f"{k}-{case.family}")
        if M in (1, 127, 128, 129, 4096, 4097, 4104):
            t.add(f"{k}-M{M}")
        t.add(f"{k}-nk1" if -(-K // 64) == 1 else f"{k}-nk>1")
        if K % 64:
            t.add(f"{k}-ktail")
        vec = N % 4 == 0
        t.add(f"{k}-st16" if N % 8 == 0 else f"{k}-st8" if vec else f"{k}-st1")
        if tn > 1:
            t.add(f"{k}-tiles_n>1")
        if N % tile_cols(case.kid):
            t.add(f"{k}-ragged-N")
        t.add(f"{k}-inst-{'act' if case.act != 'none' else 'none'}-{case.ydt}")
        if case.act != "none":
            t.add(f"{k}-{case.act}")
        if case.window:
            t.add(f"{k}-window")
            if tile_rows(case.kid) % case.window or case.window < tile_rows(case.kid):
                t.add(f"{k}-window-boundary-in-tile")
        if case.period:
            t.add(f"{k}-period")
            if tile_rows(case.kid) % case.period:
                t.add(f"{k}-period-not-dividing-tile")
        if case.resid:
            t.add(f"{k}-resid-{case.resid}")
        if case.kid == 2:
            staged = vec and case.ydt == "bf16" and case.resid != "f32"
            t.add("id2-staged" if staged else "id2-direct")
            if tm * tn > 256:
                t.add("id2-tiles>workgroups")
        if case.kid in (3, 6, 7):
            t.add(f"{k}-epi-{'lnc' if case.consumer else 'res' if case.resid else 'plain'}")
        if case.kid in (6, 7):
            if tm * tn < 256:
                t.add(f"{k}-idle-workgroups")
            if tm * tn > 256:
                t.add(f"{k}-two-tiles-per-workgroup")
            if tm % 4 and tn > 1:
                t.add(f"{k}-tiles_m%4-tiles_n>1")
            if N > 512:
                t.add(f"{k}-N>512")
        if case.consumer:
            t.add(f"{k}-consumer" + ("+resid" if case.resid else "") + ("+gelu" if case.act == "gelu" else ""))
        if case.rows:
            t.add(f"{k}-rows-N{N}" + ("+resid" if case.resid else ""))
    elif case.op == "linear_f32":
        t |= {f"f32-M{M}" if M in (1, 127, 128, 129) else "f32-M", f"f32-N{N}" if N in (1, 5, 128, 130) else "f32-N",
              f"f32-K{K}" if K in (1, 3, 16, 17, 35) else "f32-K", f"f32-{case.act}", f"f32-{case.family}"}
        t.add("f32-vec" if N % 4 == 0 else "f32-scalar")
        if case.window:
            t.add("f32-window")
        if case.period:
            t.add("f32-period")
    elif case.op == "finalize":
        np_ = N // 64
        t |= {f"fin-np{np_}", f"fin-M{M}" if M in (1, 255, 256, 257) else "fin-M"}
        t.add("fin-odd" if np_ % 2 else "fin-np%4==2" if np_ % 4 == 2 else "fin-whole-trips")
    else:
        o = "ln" if case.op == "layernorm" else "rs"
        t |= {f"{o}-d{N}", f"{o}-M{M}", f"{o}-{case.xdt}-{case.ydt}" if o == "ln" else f"{o}-{case.xdt}", f"{o}-{case.family}"}
        if o == "ln":
            t.add(f"ln-NCH{min(-(-(N // 8) // 64), 5)}")
        if case.act == "gelu" and case.resid:
            t.add("ln-gelu+resid")
        if case.strided:
            t.add(f"{o}-strided")
    return t


def _lin(kid, family, M, N, K, **kw) -> Case:
    return Case("linear", family, M, N, K, kid=kid, forced=kw.pop("forced", kid != 1), **kw)


def _id1_cases() -> list[Case]:
    c = []
    for M in (1, 127, 128, 129):  # one tile and its edges
        c.append(_lin(1, "exact", M, 130, 72, resid="bf16"))
    for K in (8, 64, 128, 200):
        c.append(_lin(1, "exact", 129, 12, K, resid="bf16", act="relu"))
    for N, ydt, res in ((8, "bf16", "bf16"), (12, "f32", "f32"), (9, "bf16", "f32"), (9, "f32", "bf16"), (130, "f32", None)):
        c.append(_lin(1, "exact", 127, N, 72, ydt=ydt, resid=res))
    c.append(_lin(1, "exact", 144, 136, 64, window=48, resid="bf16", period=5))  # batch boundary inside a tile, period 5
    c.append(_lin(1, "exact", 130, 8, 72, bias=False))
    for act, ydt in (("gelu", "bf16"), ("gelu", "f32"), ("silu", "bf16"), ("approximate_gelu", "f32")):
        c.append(_lin(1, "cancel", 129, 130, 200, act=act, ydt=ydt, resid="bf16"))
    c.append(_lin(1, "cancel", 127, 12, 128, ydt="f32"))
    c.append(_lin(1, "poison", 129, 130, 72, resid="bf16"))
    c.append(_lin(1, "poison", 127, 12, 200, ydt="f32", resid="f32", act="silu"))
    c.append(_lin(1, "poison", 130, 9, 8, resid="bf16", act="gelu"))
    c.append(_lin(1, "poison", 144, 136, 64, window=48, resid="bf16", period=5))
    c.append(_lin(1, "perm", 257, 130, 200, resid="bf16", act="gelu"))
    c.append(_lin(1, "perm", 129, 12, 72, ydt="f32", resid="f32"))
    for act in ACTS:
        for ydt in ("bf16", "f32"):
            c.append(_lin(1, "actsweep", 2, 432, 8, act=act, ydt=ydt))
    return c


def _id2_cases() -> list[Case]:
    c = [
        _lin(2, "exact", 4096, 8, 64, resid="bf16"),                       # staged, nk = 1
        _lin(2, "exact", 4104, 136, 128, ydt="f32", resid="f32", act="relu"),  # direct
        _lin(2, "exact", 4097, 136, 64, resid="bf16", period=7),
        _lin(2, "exact", 4097, 8, 128, ydt="f32"),
        _lin(2, "exact", 4096, 136, 64, consumer=True, resid="bf16"),     # consumer + residual: kept off the tile kernels
        _lin(2, "exact", 4104, 64, 64, rows=True, resid="bf16"),
        _lin(2, "exact", 4097, 320, 64, rows=True),
        _lin(2, "exact", 65800, 8, 64, resid="bf16"),                      # 258 tiles on 256 workgroups
        _lin(2, "cancel", 4096, 136, 128, ydt="f32", resid="f32"),
        _lin(2, "cancel", 4104, 136, 128, act="approximate_gelu"),
        _lin(2, "offset", 4097, 136, 128, consumer=True),
        _lin(2, "offset", 4096, 136, 64, consumer=True, resid="bf16", act="gelu"),
        _lin(2, "poison", 4104, 136, 64, resid="bf16"),
        _lin(2, "poison", 4097, 136, 128, ydt="f32", resid="f32", act="silu"),
        _lin(2, "poison", 4096, 136, 64, consumer=True, resid="bf16"),
        _lin(2, "poison", 4104, 320, 64, rows=True, resid="bf16"),
        _lin(2, "perm", 4097, 136, 128, resid="bf16", act="gelu"),
        _lin(2, "perm", 4096, 136, 64, consumer=True, resid="bf16"),
    ]
    for act in ACTS:
        for ydt in ("bf16", "f32"):
            c.append(_lin(2, "actsweep", 4096, 432, 64, act=act, ydt=ydt))
    return c


def _id3_cases() -> list[Case]:
    return [
        _lin(3, "exact", 4097, 2048, 64, forced=False),                    # the default dispatcher's own picks
        _lin(3, "exact", 4104, 2048, 64, forced=False, window=1026, resid="bf16"),
        _lin(3, "exact", 4097, 8, 64),
        _lin(3, "exact", 4097, 264, 128, resid="bf16"),
        _lin(3, "exact", 4104, 264, 64, window=1026, resid="bf16", period=9),
        _lin(3, "exact", 4097, 264, 64, consumer=True),
        _lin(3, "exact", 4097, 264, 128, consumer=True, resid="bf16"),
        _lin(3, "cancel", 4097, 264, 128, act="gelu"),
        _lin(3, "offset", 4097, 264, 128, consumer=True, act="gelu"),
        _lin(3, "offset", 4097, 8, 64, consumer=True),
        _lin(3, "poison", 4097, 264, 64, resid="bf16", act="gelu"),
        _lin(3, "poison", 4104, 264, 128, window=1026),
        _lin(3, "poison", 4097, 264, 64, consumer=True),
        _lin(3, "perm", 4097, 264, 128, resid="bf16"),
        _lin(3, "perm", 4097, 264, 64, consumer=True, act="gelu"),
        _lin(3, "actsweep", 4097, 432, 64),
        _lin(3, "actsweep", 4097, 432, 64, act="gelu"),
    ]


def _tile_cases(kid: int) -> list[Case]:
    return [
        _lin(kid, "exact", 4096, 8, 64),                                   # 16 / 13 tiles, nk = 1
        _lin(kid, "exact", 4616, 264, 64, resid="bf16"),                   # tiles_m % 4 != 0, two tile columns
        _lin(kid, "exact", 4616, 264, 128, consumer=True),
        _lin(kid, "exact", 4096, 520, 64, resid="bf16", period=11),
        _lin(kid, "exact", 82248, 8, 128, resid="bf16"),                   # 322 / 258 tiles: two per workgroup
        _lin(kid, "exact", 4616, 64, 64, rows=True),
        _lin(kid, "exact", 4616, 64, 64, rows=True, resid="bf16"),
        _lin(kid, "exact", 4616, 320, 64, rows=True, resid="bf16"),
        _lin(kid, "exact", 4104, 320, 128, rows=True),
        _lin(kid, "cancel", 4616, 264, 128, act="gelu"),
        _lin(kid, "cancel", 4096, 520, 128, resid="bf16", act="gelu"),
        _lin(kid, "offset", 4616, 264, 128, consumer=True),
        _lin(kid, "offset", 4096, 520, 64, consumer=True, act="gelu"),
        _lin(kid, "poison", 4616, 264, 64, resid="bf16"),
        _lin(kid, "poison", 4616, 264, 128, consumer=True, act="gelu"),
        _lin(kid, "poison", 4104, 8, 64, act="gelu"),
        _lin(kid, "poison", 4616, 320, 64, rows=True, resid="bf16"),
        _lin(kid, "perm", 4616, 264, 128, resid="bf16", act="gelu"),
        _lin(kid, "perm", 4616, 264, 64, consumer=True),
        _lin(kid, "perm", 4616, 320, 64, rows=True),
        _lin(kid, "actsweep", 4096, 432, 64),
        _lin(kid, "actsweep", 4096, 432, 64, act="gelu"),
    ]


def _f32_cases() -> list[Case]:
    F = lambda fam, M, N, K, **kw: Case("linear_f32", fam, M, N, K, ydt="f32", **kw)  # noqa: E731
    c = [F("exact", M, N, K, resid="f32") for M, N, K in ((1, 130, 35), (127, 5, 17), (128, 128, 16), (129, 1, 3), (129, 130, 1))]
    c.append(F("exact", 144, 128, 35 + 1, window=48, resid="f32", period=5))
    c.append(F("exact", 144, 5, 17, window=48))
    c += [F("cancel", 129, 130, 35, act=a, resid="f32") for a in ACTS]
    c.append(F("poison", 127, 130, 35, resid="f32", act="gelu"))
    c.append(F("poison", 129, 5, 17, resid="f32", period=5))
    c.append(F("poison", 144, 128, 36, window=48, resid="f32"))
    c.append(F("perm", 257, 130, 35, resid="f32", act="silu"))
    return c


def _fin_cases() -> list[Case]:
    return [Case("finalize", "offset", M, 64 * np_, ydt="f32") for np_, M in ((1, 257), (2, 255), (3, 256), (4, 1), (6, 257), (16, 255), (2, 1), (6, 256))]


def _ln_cases() -> list[Case]:
    c = []
    for d, M, xdt, ydt in ((8, 1, "bf16", "bf16"), (64, 3, "f32", "f32"), (192, 4, "bf16", "f32"), (64, 5, "f32", "bf16")):
        c.append(Case("layernorm", "offset", M, d, xdt=xdt, ydt=ydt))
        c.append(Case("row_stats", "offset", M, d, xdt=xdt, ydt="f32"))
    for d, M, xdt, ydt in ((768, 5, "bf16", "bf16"), (1280, 3, "f32", "bf16"), (4096, 4, "bf16", "f32"), (1280, 1, "f32", "f32"), (4096, 5, "f32", "bf16")):
        c.append(Case("layernorm", "poison", M, d, xdt=xdt, ydt=ydt, strided=True))
        c.append(Case("row_stats", "poison", M, d, xdt=xdt, ydt="f32", strided=True))
    c.append(Case("layernorm", "poison", 5, 768, xdt="bf16", ydt="bf16", act="gelu", resid="bf16", strided=True))
    c.append(Case("layernorm", "poison", 3, 192, xdt="f32", ydt="f32", act="gelu", resid="f32"))
    c.append(Case("layernorm", "offset", 4, 64, xdt="bf16", ydt="bf16", act="gelu", resid="f32"))
    return c


CASES: list[Case] = _id1_cases() + _id2_cases() + _id3_cases() + _tile_cases(6) + _tile_cases(7) + _f32_cases() + _fin_cases() + _ln_cases()
DEFAULT_CASES = [c for c in CASES if not c.forced]
FORCED_CASES = {k: [c for c in CASES if c.forced and c.kid == k] for k in FORCED_IDS}
assert len({c.id for c in CASES}) == len(CASES)

REQUIRED_PATHS = (
    {f"id1-M{m}" for m in (1, 127, 128, 129)} | {"id1-nk1", "id1-nk>1", "id1-ktail", "id1-st16", "id1-st8", "id1-st1", "id1-tiles_n>1"}
    | {f"id1-inst-{a}-{y}" for a in ("act", "none") for y in ("bf16", "f32")}
    | {"id1-window-boundary-in-tile", "id1-period-not-dividing-tile", "id1-resid-bf16", "id1-resid-f32"}
    | {f"id2-M{m}" for m in (4096, 4104, 4097)} | {"id2-nk1", "id2-nk>1", "id2-staged", "id2-direct", "id2-consumer+resid",
                                                  "id2-rows-N64+resid", "id2-rows-N320", "id2-tiles>workgroups", "id2-tiles_n>1"}
    | {"id3-M4097", "id3-window", "id3-nk1", "id3-nk>1", "id3-tiles_n>1", "id3-epi-plain", "id3-epi-res", "id3-epi-lnc", "id3-gelu"}
    | {f"id{k}-{p}" for k in (6, 7) for p in ("nk1", "nk>1", "idle-workgroups", "two-tiles-per-workgroup", "tiles_m%4-tiles_n>1", "N>512",
                                              "epi-plain", "epi-res", "epi-lnc", "rows-N64", "rows-N64+resid", "rows-N320+resid", "rows-N320", "consumer",
                                              "consumer+gelu", "gelu")}
    | {f"id{k}-{f}" for k in (1, 2, 3, 6, 7) for f in ("exact", "cancel", "poison", "perm", "actsweep")}
    | {f"id{k}-offset" for k in (2, 3, 6, 7)}
    | {f"fin-np{n}" for n in (1, 2, 3, 4, 6, 16)} | {f"fin-M{m}" for m in (1, 255, 256, 257)} | {"fin-odd", "fin-np%4==2", "fin-whole-trips"}
    | {f"f32-M{m}" for m in (1, 127, 128, 129)} | {f"f32-N{n}" for n in (1, 5, 128, 130)} | {f"f32-K{k}" for k in (1, 3, 16, 17, 35)}
    | {f"f32-{a}" for a in ACTS} | {"f32-window", "f32-period", "f32-perm", "f32-vec", "f32-scalar"}
    | {f"{o}-d{d}" for o in ("ln", "rs") for d in (8, 64, 192, 768, 1280, 4096)} | {f"{o}-M{m}" for o in ("ln", "rs") for m in (1, 3, 4, 5)}
    | {f"ln-{x}-{y}" for x in ("bf16", "f32") for y in ("bf16", "f32")} | {"rs-bf16", "rs-f32", "ln-gelu+resid", "ln-strided", "rs-strided"}
)


# --------------------------------------------------------------------------------------------------------------- inputs
def _exact_amp(K: int) -> int:
    """a with sigma(sum_k x w) ~ 250 for x (half zeros), w uniform integers in [-a, a]: the variance of one term is (a (a + 1) / 3)^2 / 2."""
    return max(2, min(19, round(math.sqrt(750.0 / math.sqrt(0.5 * K)))))


def _ints(g, shape, a):
    return torch.randint(-a, a + 1, shape, generator=g).float()


def build(case: Case) -> dict:
    """The operands of a case as CPU tensors in the kernel's dtypes.  x is (M, K) - for the window form the flat buffer `xbuf`
    holds it and x is the gather -, w (N, K), bias (N) f32 (the consumer's c), resid (M | period, N), stats (M, 2), s (N)."""
    g = torch.Generator().manual_seed(_seed(case))
    M, N, K, fam = case.M, case.N, case.K, case.family
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp: dict = {}
    if case.op in ("linear", "linear_f32"):
        xdt = torch.bfloat16 if case.op == "linear" else torch.float32
        nx = window_geometry(case)[2] if case.window else M * K
        if fam in ("exact", "far"):
            a = _exact_amp(K)
            xf = _ints(g, (nx,), a) * (torch.rand(nx, generator=g) < 0.5)
            w = _ints(g, (N, K), a)
            w[:, 0] = (torch.arange(N) % (2 * a + 1)).float() - a  # w differs along n whatever the draw
            bias, res = _ints(g, (N,), 64), _ints(g, (case.period or M, N), 64)
        elif fam == "actsweep":
            xf, w, bias, res = torch.zeros(nx), torch.zeros(N, K), sweep(), None
        elif fam == "cancel":
            xf = 1.0 + 0.01 * rn(nx)
            w = rn(N, K)
            w = w - w.mean(1, keepdim=True)
            bias, res = 0.01 * rn(N), 0.01 * rn(case.period or M, N)
        elif fam == "offset":  # consumer: row m at |mean| / sigma = 1, 16, 256
            r = torch.tensor([1.0, 16.0, 256.0])[torch.arange(M) % 3][:, None]
            xf = ((0.25 * r * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]) + 0.25 * rn(M, K)).reshape(-1)
            w, bias, res = rn(N, K), rn(N), rn(case.period or M, N)
        else:
            xf, w, bias, res = rn(nx), rn(N, K) / math.sqrt(K), rn(N), rn(case.period or M, N)
        xf, w = xf.to(xdt), w.to(xdt)
        inp["xbuf" if case.window else "x"] = xf if case.window else xf.view(M, K)
        if case.window:
            inp["x"] = xf[window_index(case)]
        inp["w"] = w
        inp["bias"] = bias.float() if case.bias else None
        inp["resid"] = res.to(DT[case.resid]) if case.resid else None
        if case.consumer:
            if fam in ("exact", "far"):
                mean = _ints(g, (M,), 4)
                rstd = torch.ldexp(torch.ones(M), torch.randint(-1, 2, (M,), generator=g))
                inp["s"] = _ints(g, (N,), 32)
            else:
                x64 = inp["x"].double()
                mean = x64.mean(1)
                rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + EPS)
                inp["s"] = inp["w"].double().sum(1).float()
            inp["stats"] = torch.stack([mean.float(), rstd.float()], 1).contiguous()
    elif case.op == "finalize":
        r = torch.tensor([1.0, 16.0, 256.0])[torch.arange(M) % 3][:, None]
        y = (r * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None] + rn(M, N)).to(torch.bfloat16).double().view(M, N // 64, 64)
        inp["part"] = torch.stack([y.sum(-1), (y * y).sum(-1)], -1).float().contiguous()
    else:
        off = 4096.0 if fam == "offset" else 0.5
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
        inp["x"] = (off * sign + rn(M, N)).to(DT[case.xdt])
        if case.op == "layernorm":
            inp["gamma"], inp["beta"] = 1.0 + 0.5 * rn(N), 0.5 * rn(N)
            inp["resid"] = rn(M, N).to(DT[case.resid]) if case.resid else None
    return inp


# --------------------------------------------------------------------------------------------------------------- reference
def _act64(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "gelu":
        return 0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))
    if act == "approximate_gelu":
        return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
    if act == "relu":
        return z.clamp_min(0.0)
    if act == "silu":
        return z * torch.sigmoid(z)
    return z


def act_bound(z: torch.Tensor, g: torch.Tensor, delta: torch.Tensor, act: str, fast: bool) -> torch.Tensor:
    """The error of act(z) computed in fp32 from a z that is off by delta (module docstring)."""
    az, ag = z.abs(), g.abs()
    if act in ("none", "relu"):
        return delta
    if act == "gelu":
        return GELU_LIP * delta + (GELU_POLY_ABS if fast else U32 * (6 * az + 2 * ag)) + TINY
    if act == "approximate_gelu":
        return GELU_LIP * delta + U32 * (4 * az + 2 * ag) + TINY
    over = torch.where(z < -88.7, ag, torch.zeros_like(ag))
    if fast:
        return SILU_LIP * delta + U32 * ag * (2 * torch.sigmoid(-z) * (az + 1) + 2) + over + TINY
    return SILU_LIP * delta + 4 * U32 * ag + over + TINY


def _resid_rows(case: Case, resid: torch.Tensor) -> torch.Tensor:
    return resid[torch.arange(case.M) % case.period] if case.period else resid


def reference(case: Case, inp: dict) -> dict:
    """float64 `want` and its bound (module docstring); the intermediates the bounds need ride along."""
    M, N = case.M, case.N
    if case.op in ("linear", "linear_f32"):
        x, w = inp["x"].double(), inp["w"].double()
        acc, A = x @ w.T, x.abs() @ w.abs().T
        live = A > 0  # an accumulation of zeros is exact, and so is 0 + bias: delta = 0 there (the actsweep family)
        bias = inp["bias"].double() if inp["bias"] is not None else torch.zeros(N, dtype=torch.float64)
        if case.consumer:
            mean, rstd = inp["stats"][:, :1].double(), inp["stats"][:, 1:].double()
            ms = mean * inp["s"].double()
            z, A = rstd * (acc - ms) + bias, rstd.abs() * (A + ms.abs()) + bias.abs()
        else:
            z, A = acc + bias, A + bias.abs()
        delta = torch.where(live, (case.K + 2) * U32 * A, torch.zeros_like(A))
        g = _act64(z, case.act)
        want, bound = g, act_bound(z, g, delta, case.act, case.fast_act)
        if case.resid:
            want = g + _resid_rows(case, inp["resid"]).double()
            bound = bound + U32 * want.abs()
        return dict(want=want, bound=bound + store_term(want, case.ydt), z=z, pre=g, A=A)
    if case.op == "finalize":
        p = inp["part"].double()
        np_ = N // 64
        s1, s2 = p[..., 0].sum(1), p[..., 1].sum(1)
        mean = s1 / N
        var = (s2 / N - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + EPS)
        d_mean = (np_ + 2) * U32 * p[..., 0].abs().sum(1) / N
        d_var = (np_ + 2) * U32 * s2 / N + 2 * mean.abs() * d_mean + U32 * (mean * mean + var)
        d_rstd = rstd * (d_var / (2 * (var + EPS)) + 3 * U32)
        return dict(want=torch.stack([mean, rstd], 1), bound=torch.stack([d_mean + U32 * mean.abs(), d_rstd], 1),
                    cond=(mean * mean + var) / (var + EPS))
    x = inp["x"].double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    sigma = torch.sqrt(var + EPS)
    e = N * U32 * x.abs().mean(1, keepdim=True)
    if case.op == "row_stats":
        rstd = 1.0 / sigma
        return dict(want=torch.cat([mean, rstd], 1), bound=torch.cat([e + U32 * mean.abs(), rstd * (e / sigma + 3 * U32)], 1))
    yhat = (x - mean) / sigma
    gam, bet = inp["gamma"].double(), inp["beta"].double()
    t = yhat * gam + bet
    delta = gam.abs() / sigma * (2 + yhat.abs()) * e + 3 * U32 * t.abs()
    g = _act64(t, case.act)
    want, bound = g, act_bound(t, g, delta, case.act, False)
    if case.resid:
        want = g + inp["resid"].double()
        bound = bound + U32 * want.abs()
    return dict(want=want, bound=bound + store_term(want, case.ydt), z=t, pre=g)


def exact_preconditions(case: Case, inp: dict, ref: dict) -> dict:
    """What makes the exact family exact, measured on the case: every partial sum an integer below 2^24 (A bounds them all), every
    output and - for the producer - every block's sum of squares of the rounded outputs below 2^24; share of |pre-residual| > 256."""
    y = store(ref["want"], case.ydt).double()
    lim = float(ref["A"].max() + (64 if case.resid else 0))
    sq = float((y * y).view(case.M, -1, 64).sum(-1).max()) if case.rows else 0.0
    frac = ref["want"] * 2  # the consumer's power-of-two rstd (1/2, 1, 2) leaves at most one fractional bit
    return dict(limit=max(lim, sq), integral=bool((frac == frac.round()).all()), share=float((ref["pre"].abs() > 256).double().mean()))


# --------------------------------------------------------------------------------------------------------------- placement
def _embed(t: torch.Tensor, ld: int, fill, dev) -> tuple[torch.Tensor, torch.Tensor]:
    """t (rows, cols) as the middle slice of a flat 16-byte-aligned buffer of `fill`, leading dimension ld >= cols, one guard
    stretch of >= ld elements (a multiple of 16) in front and behind.  Returns (buffer, view)."""
    rows, cols = (t.shape[0], t.shape[1]) if t.dim() == 2 else (1, t.shape[0])
    start = ld + (-ld % 16) + 16
    buf = torch.empty(2 * start + rows * ld, dtype=t.dtype)
    if isinstance(fill, int):
        bits(buf).fill_(fill if fill < 2 ** 15 or t.dtype == torch.float32 else fill - 2 ** 16)
    else:
        buf.fill_(fill)
    view = buf[start:start + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t.view(rows, cols))
    buf = buf.to(dev)
    view = buf[start:start + rows * ld].view(rows, ld)[:, :cols]
    assert view.data_ptr() % 16 == 0
    return buf, (view if t.dim() == 2 else view[0])


def out_shape(case: Case) -> tuple[int, int]:
    return (case.M, 2) if case.op in ("finalize", "row_stats") else (case.M, case.N)


def place(case: Case, inp: dict, dev="cpu", poison: bool = False, perm: torch.Tensor | None = None) -> dict:
    """The operands on `dev`.  y is ALWAYS a slice of a sentinel-filled buffer (guard rows before and after; ldy = N + 8 when
    poisoned, so guard columns too).  poison: every input is the middle slice of a NaN-filled buffer with ld = width + 8 (stats,
    whose rows are dense by contract: NaN before and after).  perm: rows of x, resid and stats permuted (not with a period)."""
    pad = 8 if poison else 0
    nan = float("nan")
    P: dict = {"poison": poison}

    def put(name, t, ld_pad=pad, mult=1):
        if t is None:
            P[name] = None
            return
        ld = t.shape[-1] + (ld_pad if t.dim() == 2 else 0)
        ld += -ld % mult  # pm_linear_f32 wants ldx, ldw multiples of 4 whatever K is: the pad columns hold NaN
        if poison or ld != t.shape[-1]:
            P[name + "_buf"], P[name] = _embed(t, ld, nan, dev)
        else:
            P[name] = t.contiguous().to(dev)

    rowp = (lambda t: t if (perm is None or t is None) else t[perm])  # noqa: E731
    if case.op in ("linear", "linear_f32"):
        if case.window:
            if poison:
                buf = torch.full((inp["xbuf"].numel() + 64,), nan, dtype=inp["xbuf"].dtype)
                covered = torch.zeros(inp["xbuf"].numel(), dtype=torch.bool)
                covered[window_index(case).reshape(-1)] = True  # the gaps between batches that no window row covers hold NaN too
                buf[32:32 + inp["xbuf"].numel()] = torch.where(covered, inp["xbuf"], torch.full_like(inp["xbuf"], nan))
                P["xbuf_buf"] = buf.to(dev)
                P["xbuf"] = P["xbuf_buf"][32:32 + inp["xbuf"].numel()]
            else:
                P["xbuf"] = inp["xbuf"].to(dev)
        else:
            put("x", rowp(inp["x"]), mult=4 if case.op == "linear_f32" else 1)
        put("w", inp["w"], mult=4 if case.op == "linear_f32" else 1)
        put("bias", inp["bias"])
        put("resid", inp["resid"] if case.period else rowp(inp["resid"]))
        if case.consumer:
            put("stats", rowp(inp["stats"]), 0)
            put("s", inp["s"])
    elif case.op == "finalize":
        put("part", inp["part"].view(case.M, -1), 0)
    else:
        put("x", inp["x"], 8 if (poison or case.strided) else 0)
        if case.op == "layernorm":
            put("gamma", inp["gamma"])
            put("beta", inp["beta"])
            put("resid", inp["resid"])
    if case.op not in ("finalize", "row_stats"):
        M, N = out_shape(case)
        P["y_buf"], P["y"] = _embed(torch.zeros(M, N, dtype=DT[case.ydt]), N + pad, SENTINEL[case.ydt], dev)
        P["y_geom"] = (N + pad + (-(N + pad) % 16) + 16, N + pad, M, N)
    return P


def sentinels_intact(case: Case, P: dict) -> bool:
    """Every element of the y buffer outside the (M, N) result still holds the sentinel: columns N .. ldy of every row, the rows
    before and after."""
    if "y_buf" not in P:
        return True
    start, ld, M, N = P["y_geom"]
    b = bits(P["y_buf"].cpu()).clone()
    want = SENTINEL[case.ydt] if (case.ydt == "f32" or SENTINEL[case.ydt] < 2 ** 15) else SENTINEL[case.ydt] - 2 ** 16
    b[start:start + M * ld].view(M, ld)[:, :N] = want
    return bool((b == want).all())


def abi_refusal(case: Case, P: dict) -> str | None:
    """The argument checks of the C entry points (csrc/linear_bf16.hip, linear_f32.hip, layernorm.hip) on the placed operands: a case
    that one of them would refuse is an error of the suite, found without a GPU."""
    al = lambda t, n=16: t is None or t.data_ptr() % n == 0  # noqa: E731
    ld = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    if case.op in ("linear", "linear_f32"):
        e = 8 if case.op == "linear" else 4
        x = P["xbuf"] if case.window else P["x"]
        rs, bs, _ = window_geometry(case) if case.window else (ld(x), 0, 0)
        if (case.op == "linear" and case.K % 8) or rs % e or bs % e or ld(P["w"]) % e or not (al(x) and al(P["w"])):
            return "x / w: 16-byte chunks"
        if case.window and case.M % case.window:
            return "window form: whole batches"
        if case.consumer or case.rows:
            if case.rows and case.N % 64:
                return "row partials: N % 64"
            vec = case.N % 4 == 0 and ld(P["y"]) % 4 == 0 and ld(P["resid"]) % 4 == 0 and al(P["y"], 8) and al(P["bias"]) and al(P["resid"], 8)
            if not (case.M >= 4096 and case.K % 64 == 0 and case.ydt == "bf16" and vec and case.resid != "f32" and ld(P["y"]) % 8 == 0 and case.N % 8 == 0):
                return "the fold needs a staged persistent epilogue"
    elif case.op == "layernorm":
        if case.N % 8 or case.N > 4096 or ld(P["x"]) % 8 or ld(P["y"]) % 8 or ld(P["resid"]) % 8 or case.act not in ("none", "gelu"):
            return "layernorm: d % 8, d <= 4096, rows 16-byte aligned"
        if not all(al(P[k]) for k in ("x", "y", "gamma", "beta", "resid")):
            return "layernorm: 16-byte aligned operands"
    elif case.op == "finalize" and case.N % 64:
        return "finalize: N % 64"
    return None


# --------------------------------------------------------------------------------------------------------------- running the ops
def run(ops, case: Case, P: dict) -> dict:
    """The case through pytorch_models._hip.ops on the placed operands; y lands in P["y"]."""
    if case.op == "linear":
        if case.window:
            rs, bs = P.get("window") or window_geometry(case)[:2]
            ops.linear_strided(P["xbuf"], M=case.M, K=case.K, row_stride=rs, rows_per_batch=case.window, batch_stride=bs, w=P["w"],
                               bias=P["bias"], act=case.act, resid=P["resid"], resid_period=case.period, out=P["y"])
            return dict(y=P["y"])
        out = ops.linear(P["x"], P["w"], P["bias"], act=case.act, resid=P["resid"], out=P["y"], ln_stats=P.get("stats"),
                         ln_s=P.get("s"), want_row_stats=case.rows, resid_period=case.period)
        return dict(y=P["y"], rows=out[1]) if case.rows else dict(y=P["y"])
    if case.op == "linear_f32":
        if case.window:
            rs, bs, _ = window_geometry(case)
            ops.linear_f32(P["xbuf"], P["w"], P["bias"], act=case.act, resid=P["resid"], resid_period=case.period, out=P["y"], M=case.M,
                           K=case.K, row_stride=rs, rows_per_batch=case.window, batch_stride=bs)
        else:
            ops.linear_f32(P["x"], P["w"], P["bias"], act=case.act, resid=P["resid"], resid_period=case.period, out=P["y"])
        return dict(y=P["y"])
    if case.op == "finalize":
        return dict(y=ops.ln_stats_finalize(P["part"].view(case.M, case.N // 64, 2), case.N, EPS))
    if case.op == "row_stats":
        return dict(y=ops.row_stats(P["x"], EPS))
    ops.layernorm(P["x"], P["gamma"], P["beta"], EPS, act=case.act, resid=P["resid"], out=P["y"])
    return dict(y=P["y"])


def plan(ops, case: Case, P: dict) -> int:
    """pm_linear_bf16_plan for the call run() would make."""
    if case.window:
        rs, bs = P.get("window") or window_geometry(case)[:2]
        return ops.linear_strided_plan(P["xbuf"], M=case.M, K=case.K, row_stride=rs, rows_per_batch=case.window, batch_stride=bs,
                                       w=P["w"], bias=P["bias"], act=case.act, resid=P["resid"], resid_period=case.period, out=P["y"])
    return ops.linear_plan(P["x"], P["w"], P["bias"], act=case.act, resid=P["resid"], out=P["y"], ln_stats=P.get("stats"),
                           ln_s=P.get("s"), want_row_stats=case.rows, resid_period=case.period)


# --------------------------------------------------------------------------------------------------------------- the CPU stand-in
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gelu_poly32(x: torch.Tensor, tail: bool = False) -> torch.Tensor:
    """csrc/common.h's gelu_poly in fp32 (the fma through float64: exact product, one rounding up to rare double-rounding ties).
    tail: the form before the factor was kept in [0, 1] (the unclamped outer x)."""
    x = x.float()
    xc = x.clamp(-4.5, 4.5)
    t = _fma32(xc * xc, torch.tensor(2.0 / 20.25).float(), torch.tensor(-1.0))
    q = torch.full_like(x, 3.353692146e-03)
    for c in (-9.328538250e-03, 1.220852128e-02, -1.674404426e-02, 2.762940359e-02, -4.055576763e-02, 5.481856801e-02,
              -7.717196008e-02, 1.569021127e-01):
        q = _fma32(q, t, torch.tensor(c).float())
    f = _fma32(xc, q, torch.tensor(0.5))
    return x * (f if tail else f.clamp(0.0, 1.0))


def _act32(z: torch.Tensor, act: str, fast: bool, tail: bool = False) -> torch.Tensor:
    if act == "gelu":
        return gelu_poly32(z, tail) if fast else 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))
    if act == "approximate_gelu":
        return 0.5 * z * (1.0 + torch.tanh(0.7978845608028654 * (0.044715 * z * z * z + z)))
    if act == "relu":
        return z.clamp_min(0.0)
    if act == "silu":
        return z / (1.0 + torch.exp(-z))
    return z


def emulate(case: Case, P: dict, mutant: str | None = None) -> dict:
    """A correct kernel on the CPU - fp32 matmul in torch's summation order, the epilogue in fp32, one store - writing through the
    placed operands as run() does; `mutant` plants one defect of MUTANTS."""
    M, N, K = case.M, case.N, case.K
    mu = mutant
    if case.op in ("linear", "linear_f32"):
        x = (P["xbuf"][window_index(case)] if case.window else P["x"]).float()
        w = P["w"].float()
        if mu == "kswap" and K >= 16:
            odd = ((torch.arange(M) >> 1) & 1) == 1
            x = x.clone()
            x[odd, 0:8], x[odd, 8:16] = x[odd, 8:16].clone(), x[odd, 0:8].clone()
        z = x @ w.T
        if mu == "ktail" and K % 64:
            t = min(8, 64 - K % 64, K)  # the chunk behind K is whatever lies there: the next row's first elements
            z = z + x.roll(-1, 0)[:, :t] @ w.roll(-1, 0)[:, :t].T
        bias = P["bias"].float() if P["bias"] is not None else torch.zeros(N)
        if mu == "biaslane":
            bias = bias.roll(1)
        if case.consumer:
            mean, rstd = P["stats"][:, :1], P["stats"][:, 1:]
            if mu == "meanrstd":
                mean, rstd = rstd, mean
            s = P["s"].float()
            if mu == "lns_shift" and N > 64:
                s = s.clone()
                n0 = 64 * ((N - 1) // 64)
                s[n0:] = P["s"][n0 - 64:N - 64]
            z = rstd * (z - mean * s) + bias
        else:
            z = z + bias
        if mu == "tileswap" and case.kid in (6, 7) and -(-M // tile_rows(case.kid)) % 4 and N > 256:
            r0 = (-(-M // tile_rows(case.kid)) - 1) * tile_rows(case.kid)
            z = z.clone()
            z[r0:, 0:8], z[r0:, 256:264] = z[r0:, 256:264].clone(), z[r0:, 0:8].clone()
        r = None
        if case.resid:
            r = P["resid"].float()
            if case.period:
                r = r[torch.arange(M).clamp_max(case.period - 1)] if mu == "residrow" else r[torch.arange(M) % case.period]
            elif mu == "residrow":
                r = r.roll(-1, 0)
        fast = case.fast_act
        if r is not None and mu == "resid_first":
            v = _act32(z + r, case.act, fast)
        else:
            v = _act32(z, case.act, fast, tail=mu == "gelu_tail")
            if r is not None:
                v = (store(v, case.ydt).float() if mu == "round_first" else v) + r
        y = store(v, case.ydt, trunc=mu == "trunc")
        P["y"].copy_(y)
        if mu == "padstore":
            start, ld, _, _ = P["y_geom"]
            P["y_buf"][start + M * ld] = 1.0  # a row >= M
            if ld > N:
                P["y_buf"][start + N] = 1.0   # a pad column
        out = dict(y=P["y"])
        if case.rows:
            f = (v if mu == "rows_unrounded" else y.float()).view(M, N // 64, 64)
            rows = torch.stack([f.sum(-1), (f * f).sum(-1)], -1)
            out["rows"] = rows.roll(1, 1) if mu == "rows_block" else rows
        return out
    if case.op == "finalize":
        p = P["part"].view(M, N // 64, 2).float()
        np_ = N // 64
        if mu == "fin_drop" and np_ % 4 == 2:
            p = p[:, :np_ - 2]
        s1, s2 = torch.zeros(M), torch.zeros(M)
        for i in range(p.shape[1]):
            s1, s2 = s1 + p[:, i, 0], s2 + p[:, i, 1]
        inv = torch.tensor(1.0 / N).float()
        mean = s1 * inv
        var = (s2 * inv - mean * mean).clamp_min(0.0)
        return dict(y=torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], 1))
    x = P["x"].float()
    mean = x.sum(1, keepdim=True) / N
    if mu == "onepass":
        var = ((x * x).sum(1, keepdim=True) / N - mean * mean).clamp_min(0.0)
    else:
        var = ((x - mean) ** 2).sum(1, keepdim=True) / N
    rstd = 1.0 / torch.sqrt(var + EPS)
    if case.op == "row_stats":
        return dict(y=torch.cat([mean, rstd], 1))
    v = (x - mean) * rstd * P["gamma"] + P["beta"]
    v = _act32(v, case.act, False)
    if case.resid:
        v = (store(v, case.ydt).float() if mu == "round_first" else v) + P["resid"].float()
    P["y"].copy_(store(v, case.ydt, trunc=mu == "trunc"))
    if mu == "padstore":
        start, ld, _, _ = P["y_geom"]
        P["y_buf"][start + M * ld] = 1.0
    return dict(y=P["y"])


# --------------------------------------------------------------------------------------------------------------- the verdict
def compare(case: Case, out: dict, ref: dict) -> tuple[float, int]:
    """(max |err| / bound, number of outputs that differ from the exact result - exact family only).  The row partials enter the
    ratio against the float64 sums of the y that was stored."""
    y = out["y"].cpu()
    if tuple(y.shape) != out_shape(case) or y.dtype != DT[case.ydt]:
        return float("inf"), -1
    r = ratio(y, ref["want"], ref["bound"])
    bad = 0
    if case.family in ("exact", "far"):
        bad = int((bits(y) != bits(store(ref["want"], case.ydt))).sum())
        r = float("inf") if bad else 0.0
    if case.rows:
        rows = out["rows"].cpu()
        f = y.double().view(case.M, case.N // 64, 64)
        want = torch.stack([f.sum(-1), (f * f).sum(-1)], -1)
        if rows.shape != want.shape or rows.dtype != torch.float32:
            return float("inf"), -1
        if case.family == "exact":
            nb = int((rows.double() != want).sum())
            bad, r = bad + nb, (float("inf") if nb else r)
        else:
            r = max(r, ratio(rows, want, 66 * U32 * torch.stack([f.abs().sum(-1), (f * f).sum(-1)], -1)))
    return r, bad


def fixed_perm(case: Case) -> torch.Tensor:
    return torch.randperm(case.M, generator=torch.Generator().manual_seed(_seed(case) + 1))


def judge(case: Case, inp: dict, ref: dict, runner, dev="cpu", margin: float = MARGIN, on_place=None) -> dict:
    """Every assertion the GPU suite makes on one case, as a record: runner(case, placed operands) -> {y[, rows]} is ops (run) on the
    GPU and the stand-in (emulate) on the CPU.  ok = all of: ratio <= margin (exact: bit-equal), sentinels intact, poison run finite and
    bit-identical with its sentinels intact, permuted run equal to y[p], actsweep rows all equal to row 0.  on_place(P) sees every
    placement - plain, poisoned, permuted - before it runs (the GPU child asks pm_linear_bf16_plan there)."""
    seen = on_place or (lambda P: None)
    P = place(case, inp, dev)
    seen(P)
    out = runner(case, P)
    r, bad = compare(case, out, ref)
    rec = dict(id=case.id, op=case.op, kid=case.kid, family=case.family, ratio=r, mismatches=bad, sentinel=sentinels_intact(case, P))
    y = out["y"].cpu().clone()
    rows = out["rows"].cpu().clone() if case.rows else None
    if case.family == "poison":
        Q = place(case, inp, dev, poison=True)
        seen(Q)
        again = runner(case, Q)
        ya = again["y"].cpu()
        rec["poison_finite"] = bool(torch.isfinite(ya).all()) and (rows is None or bool(torch.isfinite(again["rows"]).all()))
        rec["poison_same"] = bool(torch.equal(bits(ya), bits(y))) and (rows is None or bool(torch.equal(again["rows"].cpu(), rows)))
        rec["poison_sentinel"] = sentinels_intact(case, Q)
    if case.family == "perm":
        p = fixed_perm(case)
        Q = place(case, inp, dev, perm=p)
        seen(Q)
        again = runner(case, Q)
        rec["perm_same"] = bool(torch.equal(bits(again["y"].cpu()), bits(y[p]))) and (rows is None or bool(torch.equal(again["rows"].cpu(), rows[p])))
    if case.family == "actsweep":
        rec["rows_equal"] = bool((bits(y) == bits(y[:1])).all())
        if case.act == "gelu" and case.ydt == "bf16":
            rec["gelu_bits"] = bits(y[0]).tolist()
    flags = [v for k, v in rec.items() if k in ("sentinel", "poison_finite", "poison_same", "poison_sentinel", "perm_same", "rows_equal")]
    rec["ok"] = bool(r <= margin and all(flags))
    return rec


def explain(rec: dict) -> str:
    if rec.get("why"):
        return f"{rec['id']}: {rec['why']}"
    what = f"{rec['mismatches']} outputs differ from the exact result" if rec["family"] in ("exact", "far") else f"{rec['ratio']:.3f} x the bound (allowed {MARGIN})"
    return f"{rec['id']}: {what}; " + ", ".join(f"{k}={v}" for k, v in rec.items() if isinstance(v, bool))


def figure(rec: dict) -> str:
    return f"FIGURE {rec['op']}{rec['kid'] or ''} {rec['family']} {rec['id']} ratio {rec['ratio']:.3f}"


# --------------------------------------------------------------------------------------------------------------- far operands
# DESIGN.md section 30.  The 256-wide GEMMs keep 32-bit offsets per operand and rely on linear_decide to keep every operand inside
# them.  REACH states, per kernel id and operand, the largest quantity the kernel forms in 32 bits, read off the sources; a kernel
# serves a call only while each stays below 2^32.  tests/test_linear_cases_cpu.py asks pm_linear_bf16_plan (host arithmetic on
# made-up pointers) that no kernel id is returned for arguments beyond its reach - that covers bounds no allocation can reach -, and
# the `far` family runs every bound that fits the arena on the GPU: exact-family operands, one of them a view into the poisoned
# arena of tests/wrapper_cases.py with its last row (last batch, last period row) just past 2^31, 2^32 bytes - or, where a kernel's
# reach lies there, 2^33 bytes = 2^32 bf16 elements.  A refusal is a pass; whatever runs must EQUAL want.to(out dtype) whichever
# kernel took it (the dispatcher may move a case it cannot address: `planned` goes into the record, it is not asserted), leave every
# sentinel of the y buffer alone and leave the arena outside the view all poison.
#
#   ids 1, 2 (linear_bf16.hip)   every offset is int64 ((int64_t)gm * ldx + ..., (int64_t)m * ldy + n, ...): no 32-bit reach
#   id 3 (linear_bf16_wide.hip)  xoff / woff are uint32 ELEMENT offsets of 16-byte chunks: (M - 1) ldx + K - 8 - the window form:
#                                (M / R - 1) batch_stride + (R - 1) ldx + K - 8 -, (N - 1) ldw + K - 8; resid and y are int64
#   ids 6, 7 (linear_bf16_tile.hip)  uniform 64-bit row bases plus uint32 BYTE lane offsets: a piece is 8 rows, so x and w reach
#                                7 * 2 ld + (K / 64 - 1) * 128 + 127; the residual block is 16 rows off a 64-bit base,
#                                15 * 2 ldr + 2 (N - 8) + 15, and a periodic residual is addressed off the operand's base,
#                                (min(P, M) - 1) * 2 ldr + 2 (N - 8) + 15; y: 7 * 2 ldy + 7 * 16 + 15
LIMIT32 = 1 << 32
FAR_DIST = {"2G": 1 << 31, "4G": 1 << 32, "8G": 1 << 33}


def reach(kid: int, M: int, N: int, K: int, ldx: int, ldw: int, ldr: int = 0, ldy: int = 0, period: int = 0, window: int = 0,
          batch_stride: int = 0) -> dict:
    """operand -> the largest quantity kernel `kid` forms in 32 bits for it (module comment above); {} for ids 1 and 2"""
    if kid == 3:
        x = (M // window - 1) * batch_stride + (window - 1) * ldx + K - 8 if window else (M - 1) * ldx + K - 8
        return dict(x=x, w=(N - 1) * ldw + K - 8)
    if kid in (6, 7):
        r = dict(x=14 * ldx + (K // 64 - 1) * 128 + 127, w=14 * ldw + (K // 64 - 1) * 128 + 127, y=14 * ldy + 127)
        if ldr:
            r["resid"] = ((min(period, M) - 1) if period else 15) * 2 * ldr + 2 * (N - 8) + 15
        return r
    return {}


FAR_SHAPE = {1: (136, 136, 64), 2: (4096, 8, 64), 3: (4104, 8, 64), 6: (4096, 8, 64), 7: (4096, 8, 64)}  # the smallest each id lists
FAR_WINDOW = {1: (144, 48), 2: (4104, 1026), 3: (4104, 1026), 6: (4104, 1026), 7: (4104, 1026)}     # (M, rows per batch)


def _far_cases() -> list[Case]:
    c = []
    for kid in (1,) + FORCED_IDS:
        M, N, K = FAR_SHAPE[kid]
        for which in ("x", "w", "resid", "y"):
            for d in ("2G", "4G") + (("8G",) if kid == 3 and which in ("x", "w") else ()):  # id 3's reach: 2^32 elements
                c.append(_lin(kid, "far", M, N, K, resid="bf16", far=f"{which}:{d}"))
        for d in ("4G",) + (("8G",) if kid == 3 else ()):
            c.append(_lin(kid, "far", FAR_WINDOW[kid][0], N, K, window=FAR_WINDOW[kid][1], resid="bf16", far=f"win:{d}"))
        for per in (2, 3):  # ids 6 / 7: the periodic row offset (mm % P) * (ldr * 2) was formed in 32 bits
            c.append(_lin(kid, "far", M, N, K, resid="bf16", period=per, far="residp:4G"))
    return c


FAR_CASES = _far_cases()
FAR_DEFAULT = [c for c in FAR_CASES if not c.forced]
FAR_FORCED = {k: [c for c in FAR_CASES if c.forced and c.kid == k] for k in FORCED_IDS}
assert len({c.id for c in FAR_CASES}) == len(FAR_CASES)


def far_geometry(case: Case) -> tuple[str, tuple, tuple]:
    """(operand, shape, strides in elements) of the far view of a case"""
    import wrapper_cases as WC
    which, d = case.far.split(":")
    if which == "win":
        rs, _, _ = window_geometry(case)
        nb, seg = case.M // case.window, (case.window - 1) * rs + case.K
        return "xbuf", (nb, seg), (WC.far_stride(nb, 2, FAR_DIST[d]), 1)
    rows, cols = {"x": (case.M, case.K), "w": (case.N, case.K), "resid": (case.M, case.N), "residp": (case.period, case.N),
                  "y": (case.M, case.N)}[which]
    return which.replace("residp", "resid"), (rows, cols), (WC.far_stride(rows, 2, FAR_DIST[d]), 1)


def far_lds(case: Case) -> dict:
    """the strides the far call passes, for reach(): the far one from far_geometry, the others packed"""
    name, shape, st = far_geometry(case)
    g = dict(M=case.M, N=case.N, K=case.K, ldx=case.K, ldw=case.K, ldr=case.N, ldy=case.N, period=case.period, window=case.window)
    if case.window:
        g["ldx"], g["batch_stride"] = window_geometry(case)[:2]
    g[{"x": "ldx", "w": "ldw", "resid": "ldr", "y": "ldy", "xbuf": "batch_stride"}[name]] = st[0]
    return g


def place_far(case: Case, inp: dict, arena, dev="cpu", touch: bool = True) -> dict:
    """place() with the one far operand a view into `arena`; touch=False builds the views without writing them (the CPU stage
    checks the arithmetic and maps nothing)."""
    import wrapper_cases as WC
    P = place(case, inp, dev)
    name, shape, st = far_geometry(case)
    view = arena.view(shape, st, torch.bfloat16)
    if name == "xbuf":
        rs, bs0, _ = window_geometry(case)
        src = torch.stack([inp["xbuf"][b * bs0:b * bs0 + shape[1]] for b in range(shape[0])])
        P["xbuf"] = arena.view(((shape[0] - 1) * st[0] + shape[1],), (1,), torch.bfloat16)
        P["window"] = (rs, st[0])
    else:
        src = torch.zeros(shape, dtype=torch.bfloat16) if name == "y" else inp[name]
        P[name] = view
        if name == "y":
            del P["y_buf"], P["y_geom"]
    assert tuple(src.shape) == tuple(shape) and src.dtype == torch.bfloat16
    P["far_view"] = view
    P["far_case"] = WC.FarCase("far:" + case.far.split(":")[1], 0, view, tuple(st), 2, src.numel(), 32)
    if touch:
        view.copy_(src.to(dev))
    return P


def judge_far(case: Case, inp: dict, ref: dict, ops, arena, dev="cuda") -> dict:
    """One far case as a record: refused (a pass: y and the arena untouched, and the plan says so too) or run - then y equals
    want.to(out dtype) bit for bit, the sentinels of the y buffer and the arena outside the view are as they were."""
    import wrapper_cases as WC
    P = place_far(case, inp, arena, dev)
    rec = dict(id=case.id, op=case.op, kid=case.kid, family=case.family, far=case.far, ratio=0.0, mismatches=0)
    gate = arena.holds(P["far_case"])
    if gate:  # never run what the arena cannot contain
        arena.erase(P["far_view"])
        return dict(rec, ok=False, why="; ".join(gate))
    rec["planned"] = plan(ops, case, P)
    try:
        out, rec["refused"] = run(ops, case, P), False
        rec["ratio"], rec["mismatches"] = compare(case, out, ref)
    except (ValueError, RuntimeError) as e:
        if WC.is_fault(e):
            raise
        rec["refused"], rec["refusal"] = True, str(e)[:200]
        rec["y_untouched"] = bool((P["y"].cpu().float() == 0).all())
    rec["sentinel"] = sentinels_intact(case, P)
    arena.erase(P["far_view"])
    at = arena.dirty()
    rec["arena_clean"] = at is None
    if at is not None:
        rec["arena_first"] = at - arena.base
        arena.words.fill_(WC.POISON32)
    rec["plan_agrees"] = (rec["planned"] < 0) == rec["refused"]
    rec["ok"] = bool(rec["mismatches"] == 0 and all(v for k, v in rec.items() if k in ("sentinel", "arena_clean", "plan_agrees", "y_untouched")))
    rec["ratio"] = 0.0 if rec["mismatches"] == 0 else 1e300
    return rec


# ---- the reach table against the dispatcher: pm_linear_bf16_plan on made-up aligned pointers (it never dereferences)
def plan_args(M, N, K, ldx, ldw, ldr=0, ldy=0, period=0, window=0, batch_stride=0) -> tuple:
    """the arguments of pm_linear_bf16_plan for a bf16 call with a bias and - where ldr is given - a bf16 residual"""
    p = lambda i: (1 << 40) + (i << 36)  # noqa: E731
    return (p(0), ldx, window, batch_stride, p(1), ldw, p(2), p(3) if ldr else None, ldr, 0, period if ldr else 0, p(4), ldy or N, 0,
            M, N, K, 0, None, None, None, None, 0)


def reach_probes(kid: int) -> dict:
    """name -> (geometry just beyond kernel `kid`'s reach in one operand, that operand).  The far stride is the smallest multiple
    of 8 at which reach() passes 2^32; every other stride is packed.  "base" is the same call with every stride packed."""
    M, N, K = FAR_SHAPE[kid]
    Mw, R = FAR_WINDOW[kid]
    base = dict(M=M, N=N, K=K, ldx=K, ldw=K, ldr=N, ldy=N)
    forms = {"x": (base, "ldx", "x"), "w": (base, "ldw", "w"), "resid": (base, "ldr", "resid"), "y": (base, "ldy", "y"),
             "residp2": (dict(base, period=2), "ldr", "resid"), "residp3": (dict(base, period=3), "ldr", "resid"),
             "win": (dict(base, M=Mw, window=R, ldx=16, batch_stride=(R - 1) * 16 + K + 40), "batch_stride", "x")}
    out = {"base": (base, None)}
    for name, (g, key, operand) in forms.items():
        if operand not in reach(kid, **g) or (name == "win" and kid != 3):
            continue
        lo, hi = g[key], 1 << 40
        while hi - lo > 8:  # reach() grows with the stride: bisect over multiples of 8
            mid = (lo + hi) // 16 * 8
            lo, hi = (lo, mid) if reach(kid, **dict(g, **{key: mid}))[operand] >= LIMIT32 else (mid, hi)
        out[name] = (dict(g, **{key: hi}), operand)
    return out


def reach_fits_arena(g: dict, operand: str, after: int) -> bool:
    """the operand of a probe, as far as the kernel reads it, ends within `after` bytes of its base"""
    rows = {"x": g["M"], "w": g["N"], "y": g["M"], "resid": g.get("period") or g["M"]}[operand]
    if g.get("window"):
        return ((g["M"] // g["window"] - 1) * g["batch_stride"] + g["window"] * 16 + g["K"]) * 2 <= after
    return ((rows - 1) * g[{"x": "ldx", "w": "ldw", "y": "ldy", "resid": "ldr"}[operand]] + max(g["N"], g["K"])) * 2 <= after
