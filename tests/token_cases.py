"""References, error bounds, adversarial input families and case lists shared by the token-path kernel parity tests
(tests/test_token_cases_cpu.py without a GPU, tests/test_hip_token_adversarial.py on one).  A plain helper module.

In scope: pm_mixer_token_mix_bf16, pm_ln_mean, pm_transpose_add_f32 (csrc/mixer.hip); pm_cls_head_gemm, pm_cls_attend
(csrc/cls_tail.hip); pm_vit_tokens, pm_vit_tokens_generic (csrc/vit_tokens.hip); the row reductions pm_mean_ln,
pm_ln_space_to_depth (csrc/convnext.hip), pm_se_gate (csrc/maxvit.hip), pm_mean_rows_bf16 (csrc/conv2d.hip), pm_rmsnorm, pm_geglu
(csrc/layernorm.hip).  Every run on the device goes through lib(), the C ABI, into a sentinel-guarded output; the poison family's
second launch additionally cuts every operand out of a NaN-filled buffer.

Contract ("2h. Token-path numerics contract").  u = 2^-24; half a bf16 ulp of v is 2^(floor(log2 |v|) - 8); no number measured
on a kernel enters a bound; an element whose bound is 0 must be exact; a non-finite output is an infinite ratio; no element is
excluded.  The GPU suite asserts MARGIN = 1.5 x the bound, the CPU stand-in 1.0 x.

Reference: float64 on the CPU from exactly the operands the kernel sees (bf16 x and weights widened, the f32 stats / gamma / beta /
biases it is given).  Bounds per op: see the *_reference functions, each of which states its counts next to the kernel line they
come from; the derivations are collected in DESIGN.md 2h.

Families.
  exact    every intermediate is an integer that the formats hold exactly, so the output (and token mixing's row partials) must
           EQUAL the reference bit for bit; the per-case preconditions are checked by exact_preconditions() on the CPU.
           token_mix: stats (0, 1), gamma 1, beta 0, integer x, W1 / W2 in {-1, 0, 1}, b1 = +-64 alternating so that |z| >= 4.5 and
           gelu_poly returns z or -0.  cls_head_gemm / vit_tokens: integer operands, sums exact in fp32, ONE rounding to bf16, with
           bf16 halfway points of both parities (257 -> 256, 259 -> 260) planted through the bias / pe.
  needle   token_mix: all of W1 on the last real token T - 1 (next to the padding), all of W2 on the last hidden row, b2 distinct per
           token.  cls_attend: one key scores 30 above the rest.
  locate   vit_tokens: one-hot weight rows on an image of distinct codes 0.75 ulp above a bf16 value (round-to-nearest takes the next
           code, truncation the one below): every output NAMES the pixel it was read from.  locpe: a zero image, pe = code(p, f).
           ln_space_to_depth: gamma 1, beta 0 on distinct pixels of a 6 x 10 image, held to the bound: the quadrant order k = 2 dh + dw.
  offset   cls_attend at |mean| / sigma = 4, 64, 4096 (4096: rows of +-2^k with one element one bf16 ulp higher, d = 1024 - a Gaussian
           row cannot carry that ratio in bf16); rmsnorm at 64 (the mean is not removed).
  const    cls_attend on constant rows (variance 0) with in-kernel statistics.
  poison   Gaussian operands; on the GPU a second launch with every operand the 16-byte aligned middle of a NaN-filled buffer:
           finite, bit-identical to the plain run, every sentinel intact.
  perm     Gaussian operands, N = 3: a permutation of the images permutes the outputs bit for bit, each image alone equals its
           slice of the batch, and (token_mix) out = x gives the same bits.
  move     transpose_add_f32: the result is a copy or ONE fp32 addition, bit-equal.

Path -> case (paths() derives the tags; for token mixing from pm_mixer_token_mix_plan's own report, mirrored in tm_plan()):
  token_mix  NB 4 / NB 2 by C % 128 / NB 2 by LDS             C 128 / C 64 (one slab), C 192 (three) / T 16, Dt 640, C 128
             last served / first refused Dt at T 16           992 / 1024 (REFUSED_TOKEN_MIX)
             region_a = scratch / = slab                      T <= 112 / T 128 at NB 4
             nd < 8, = 8, = 9 (W1 -> W1 -> W2)                Dt 32, 256, 288
             nk2 2, 8, 10, 18 (ring depth 8)                  Dt 32, 128, 160, 288
             nk1 1, < 8, = 8, 9 - 15, 17                      T 1 / 16, 49, 128, 196, 257
             nt 1, 8, 9                                       T <= 32, 256, 257 (a second W2 strip with one live row)
             T odd / even / = Tp                              1, 15, 17, 31, 33 / 2, 30 / 16, 32
  ln_mean    T 1, 7; C 1, 255, 256, 257; the four dtype pairs
  transpose  R, Cc in {1, 31, 32, 33}; ldy = R and ldy > R; with and without resid
  cls_head   K 32 (three idle waves), 128, 160 (uneven); M 1, 15, 16, 17, 33; N 64, 128; G 1, 3; no bias; ldx > G K; group stride != K
  cls_attend L 1, 31, 32, 33, 64, 65; d 64 (waves 2, 3 idle in phase A), 128, 192, 384 / 448 (either side of the 64 KiB raise), 1024;
             H 1, 3, 16; stats given / in-kernel; N 1 / 3; x a strided view
  vit        32 x 48 and 48 x 16 images; N 5 at L 4; Mtot 1, 127, 128, 129; d 4, 64, 132, 192, 260; cls / none;
             generic P 4 (K 48), 8 (K 192), 14 (K 588, ragged last step), 32; ldw = Kpad and > Kpad
  rows       mean_ln C 1, 37, 255, 256, 257, HW 1, 9, ldx > C; s2d 2 x 2, 6 x 10, C 1, 37, 96; se_gate ntiles 1, 3, C 5, 64, 300,
             R 1, 5, 64; mean_rows R 1, 7, C 1, 9; rmsnorm d 8, 512, 520, 4096; geglu F 8, 136, ldh > 2 F
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from linear_cases import GELU_LIP, GELU_POLY_ABS, MARGIN, TINY, U32, act_bound, gelu_poly32, ratio, store_term  # noqa: F401

EPS = 1e-6
SENT32, SENT16 = 0x4B4B4B4B, 0x4B4B
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
PM_DT = {torch.bfloat16: 0, torch.float32: 1}
MX_SCR_BYTES, MX_LDS_MAX = 8 * 32 * 33 * 4, 160 * 1024   # csrc/mixer.hip
CODE0 = 0x3000            # the first pixel code's bf16 bit pattern (2^-31); 16384 codes stay finite

OPS = ("token_mix", "ln_mean", "transpose", "cls_head_gemm", "cls_attend", "vit_tokens", "mean_ln", "s2d", "se_gate", "mean_rows",
       "rmsnorm", "geglu")
MUTANT_OF = {  # mutant -> (op, the family aimed at it)
    "pad_token_live": ("token_mix", "needle"), "pad_hidden_live": ("token_mix", "poison"), "stats_image0": ("token_mix", "poison"),
    "b2_by_channel": ("token_mix", "needle"), "gelu_before_bias": ("token_mix", "exact"), "row_sums_unrounded": ("token_mix", "poison"),
    "slab_offset": ("token_mix", "poison"), "resid_dropped": ("token_mix", "exact"),
    "mean_dropped": ("cls_attend", "offset"), "cm_unrounded": ("cls_attend", "offset"), "tail_rows_live": ("cls_attend", "poison"),
    "no_rescale": ("cls_attend", "needle"), "rstd_once": ("cls_attend", "poison"), "head_pad_leak": ("cls_attend", "poison"),
    "group_stride": ("cls_head_gemm", "poison"), "bias_group0": ("cls_head_gemm", "exact"), "wave3_lost": ("cls_head_gemm", "exact"),
    "trunc_store": ("cls_head_gemm", "exact"),
    "gy_gx_swapped": ("vit_tokens", "locate"), "pe_shifted_by_cls": ("vit_tokens", "locpe"), "cls_every_row": ("vit_tokens", "locpe"),
    "pixel_trunc": ("vit_tokens", "locate"), "generic_tail_live": ("vit_tokens", "locate"), "channel_stride": ("vit_tokens", "locate"),
    "ln_of_mean_for_mean_of_ln": ("mean_ln", "poison"), "s2d_quadrants": ("s2d", "locate"), "se_div_ntiles": ("se_gate", "poison"),
    "rms_centred": ("rmsnorm", "offset"), "geglu_halves_swapped": ("geglu", "poison"), "transpose_ldy": ("transpose", "move"),
}
MUTANTS = tuple(MUTANT_OF)


def bf16r(t: torch.Tensor) -> torch.Tensor:
    """Nearest bf16 value (ties to even), kept in the input's wider storage."""
    return t.to(torch.bfloat16).to(t.dtype if t.dtype != torch.bfloat16 else torch.float32)


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def rounded_store(want: torch.Tensor, pre: torch.Tensor, dt: str) -> torch.Tensor:
    """pre + one correctly rounded store of a value within `pre` of `want`."""
    return pre + store_term(want.abs() + pre, dt)


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    op: str
    family: str
    dims: tuple  # ((name, value), ...): the shape and the switches of the problem

    @property
    def d(self) -> dict:
        return dict(self.dims)

    def get(self, k, default=0):
        return self.d.get(k, default)

    @property
    def id(self) -> str:
        parts = []
        for k, v in self.dims:
            if isinstance(v, bool):
                if v:
                    parts.append(k)
            else:
                parts.append(f"{k}{v}")
        return f"{self.op}-{self.family}-" + "-".join(parts)


def mk(op: str, family: str, **dims) -> Case:
    return Case(op, family, tuple(dims.items()))


def _gen(case: Case) -> torch.Generator:
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003)


def tm_plan(T: int, Dt: int, C: int) -> dict | None:
    """csrc/mixer.hip's mx_pick_nb / mx_region_a / mx_lds_bytes, mirrored: what pm_mixer_token_mix_plan must report (the CPU test holds
    the two together for every case); None = refused."""
    if T < 1 or T > 4096 or Dt < 32 or Dt > 4096 or Dt % 32 or C < 64 or C % 64:
        return None
    Tp = (T + 15) // 16 * 16

    def region_a(nb):
        return (max(32 * nb * (Tp + 8) * 2, MX_SCR_BYTES) + 15) // 16 * 16

    def lds(nb):
        return region_a(nb) + 32 * nb * (Dt + 8) * 2

    nb = 4 if C % 128 == 0 and lds(4) <= MX_LDS_MAX else 2 if lds(2) <= MX_LDS_MAX else 0
    if not nb:
        return None
    return dict(NB=nb, lds=lds(nb), region_a=region_a(nb), nk1=Tp // 16, nk2=Dt // 16, nd=Dt // 32, nt=(T + 31) // 32,
                scratch=32 * nb * (Tp + 8) * 2 <= MX_SCR_BYTES)


def paths(case: Case, plan: dict | None = None) -> set[str]:
    """The kernel paths a case reaches.  token_mix: from `plan`, pm_mixer_token_mix_plan's report (default: its mirror tm_plan)."""
    d, t = case.d, set()
    if case.op == "token_mix":
        T, Dt, C = d["T"], d["Dt"], d["C"]
        p = plan or tm_plan(T, Dt, C)
        t |= {f"NB{p['NB']}", "scratch" if p["scratch"] else "slab", f"nd{p['nd']}", f"nk2={p['nk2']}", f"nt{p['nt']}", f"N{d['N']}",
              "rows" if d.get("rows") else "norows", f"slabs{C // (32 * p['NB'])}"}
        if p["NB"] == 2:
            t.add("NB2-by-C" if C % 128 else "NB2-by-lds")
        nk1 = p["nk1"]
        t.add("nk1=1" if nk1 == 1 else "nk1<8" if nk1 < 8 else "nk1=8" if nk1 == 8 else "nk1=9..15" if nk1 < 16 else f"nk1={nk1}")
        t.add("T=Tp" if T % 16 == 0 else "T-odd" if T % 2 else "T-even")
        if T in (1, 15, 17, 31, 33, 2, 30, 16, 32, 257):
            t.add(f"T{T}")
        if Dt == 992:
            t.add("Dt-last-served")
    elif case.op == "ln_mean":
        t |= {f"T{d['T']}", f"C{d['C']}", f"{d['xdt']}>{d['ydt']}", f"N{d['N']}"}
    elif case.op == "transpose":
        t |= {f"R{d['R']}", f"Cc{d['Cc']}", "ldy>R" if d["pad"] else "ldy=R", "resid" if d.get("resid") else "noresid", f"N{d['N']}"}
    elif case.op == "cls_head_gemm":
        t |= {f"K{d['K']}", f"M{d['M']}", f"N{d['N']}", f"G{d['G']}", "bias" if d.get("bias") else "nobias"}
        if d.get("ldpad"):
            t.add("ldx>GK")
        if d.get("gpad"):
            t.add("xg!=K")
        if d["N"] > 64 and d["G"] > 1:
            t.add("N>64&G>1")
    elif case.op == "cls_attend":
        L, dd = d["L"], d["d"]
        t |= {f"L{L}", f"d{dd}", f"H{d['H']}", "stats" if d.get("stats") else "in-kernel", f"N{d['N']}"}
        t.add("lds>64K" if 2 * 64 * dd + CT_SIDE_BYTES > 65536 else "lds<=64K")
        if L <= 32:
            t.add("one-block")
        if L % 32:
            t.add("ragged-block")
    elif case.op == "vit_tokens":
        P, H, W, N, dd = d["P"], d["H"], d["W"], d["N"], d["d"]
        K = 3 * P * P
        generic = P != 16 or d.get("ldpad", 0) > 0 or d.get("generic", False)
        t |= {"generic" if generic else "p16", f"d{dd}", "cls" if d.get("cls") else "nocls", f"Mtot{N * (H // P) * (W // P)}"}
        if H != W:
            t.add(f"{H}x{W}")
        if generic:
            t |= {f"P{P}", "ldw>Kpad" if d.get("ldpad") else "ldw=Kpad", "K-tail" if K % 64 else "K-full"}
        if (H // P) * (W // P) * 2 < 128 and N * (H // P) * (W // P) > 2 * (H // P) * (W // P):
            t.add("tile>2imgs")
    else:
        for k, v in case.dims:
            t.add(k if isinstance(v, bool) and v else f"{k}{v}")
        if d.get("ldpad"):
            t.add("ldpad")
        if case.op in ("ln_mean", "mean_ln", "s2d", "rmsnorm"):
            t.add(f"{d['xdt']}>{d['ydt']}")
    return t


CT_SIDE_BYTES = 4 * 16 * 32 * 4 + 16 * 32 * 2 + 32 * 2 * 4 + 16 * 4 + 4 * 16 * 4 + 16 * 2 * 4  # csrc/cls_tail.hip
_PAIRS = {"bf16>bf16", "bf16>f32", "f32>bf16", "f32>f32"}
REQUIRED_PATHS = {
    "token_mix": {"NB4", "NB2-by-C", "NB2-by-lds", "slabs1", "slabs3", "Dt-last-served", "scratch", "slab", "nd1", "nd8", "nd9",
                  "nk2=2", "nk2=8", "nk2=10", "nk2=18", "nk1=1", "nk1<8", "nk1=8", "nk1=9..15", "nk1=17", "nt1", "nt8", "nt9",
                  "T1", "T15", "T17", "T31", "T33", "T2", "T30", "T16", "T32", "T257", "T-odd", "T-even", "T=Tp", "N1", "N3", "rows", "norows"},
    "ln_mean": {"T1", "T7", "C1", "C255", "C256", "C257", "N1", "N3"} | _PAIRS,
    "transpose": {f"{a}{v}" for a in ("R", "Cc") for v in (1, 31, 32, 33)} | {"ldy>R", "ldy=R", "resid", "noresid", "N1", "N3"},
    "cls_head_gemm": {"K32", "K128", "K160", "M1", "M15", "M16", "M17", "M33", "N64", "N128", "G1", "G3", "bias", "nobias", "ldx>GK",
                      "xg!=K", "N>64&G>1"},
    "cls_attend": {"L1", "L31", "L32", "L33", "L64", "L65", "d64", "d128", "d192", "d384", "d448", "d1024", "H1", "H3", "H16", "stats",
                   "in-kernel", "N1", "N3", "one-block", "ragged-block", "lds>64K", "lds<=64K"},
    "vit_tokens": {"p16", "generic", "32x48", "48x16", "tile>2imgs", "Mtot1", "Mtot127", "Mtot128", "Mtot129", "d4", "d64", "d132",
                   "d192", "d260", "cls", "nocls", "P4", "P8", "P14", "P32", "ldw>Kpad", "ldw=Kpad", "K-tail", "K-full"},
    "mean_ln": {"C1", "C37", "C255", "C256", "C257", "HW1", "HW9", "ldpad"} | _PAIRS,
    "s2d": {"H2", "H6", "W2", "W10", "C1", "C37", "C96", "ldpad"} | _PAIRS,
    "se_gate": {"ntiles1", "ntiles3", "C5", "C64", "C300", "R1", "R5", "R64"},
    "mean_rows": {"R1", "R7", "C1", "C9"},
    "rmsnorm": {"d8", "d512", "d520", "d4096"} | _PAIRS,
    "geglu": {"F8", "F136", "ldpad"},
}
REFUSED_TOKEN_MIX = ((16, 1024, 128), (16, 1024, 64), (16, 48, 64), (16, 32, 96), (0, 32, 64))  # the first: the first refused Dt at T 16


def _cases() -> list[Case]:
    L: list[Case] = []
    # ---- token mixing: T, Dt, C, N, rows
    for (T, Dt, C, N, rows) in (
        (1, 32, 64, 1, True),       # one token: nk1 1, nd 1 (seven waves prime the ring for W2 without a W1 strip), nk2 2, NB 2 by C
        (2, 32, 64, 3, False),      # even, one pair; row_out null
        (15, 288, 192, 1, True),    # three slabs of NB 2; nd 9: wave 0 walks W1 -> W1 -> W2; nk2 18 = 2 x 8 + 2
        (16, 256, 128, 3, True),    # T = Tp: no padding at all; NB 4; nd 8: every wave one strip; nk2 16
        (17, 160, 64, 1, True),     # odd T one past a K step; nk2 10: a partial ring round
        (30, 128, 128, 1, False),   # even below Tp; nk2 8 = the ring depth
        (31, 32, 64, 1, True),
        (32, 32, 128, 1, True),     # T = Tp = one full W2 strip
        (33, 32, 64, 3, True),      # a second W2 strip with one live row in wave 1
        (49, 128, 128, 3, True),    # nk1 4
        (16, 640, 128, 1, True),    # NB 2 because NB 4 would need 195 KiB of LDS
        (16, 992, 128, 1, True),    # the largest served Dt at T 16
        (128, 32, 128, 1, True),    # nk1 8; region_a is the slab (34816 B > the scratch's 33792)
        (196, 32, 64, 1, False),    # nk1 13
        (256, 32, 64, 1, True),     # nt 8: every wave one W2 strip
        (257, 32, 128, 1, True),    # nk1 17; nt 9: wave 0's second W2 strip has one live row
    ):
        for f in ("exact", "needle", "poison") + (("perm",) if N == 3 else ()):
            L.append(mk("token_mix", f, T=T, Dt=Dt, C=C, N=N, rows=rows))
    # ---- ln_mean
    for (T, C, N, xdt, ydt) in ((1, 1, 1, "f32", "f32"), (1, 255, 3, "bf16", "bf16"), (1, 256, 1, "f32", "bf16"), (1, 257, 3, "bf16", "f32"),
                                (7, 257, 3, "f32", "f32"), (7, 1, 1, "bf16", "bf16")):
        for f in ("exact", "poison"):
            L.append(mk("ln_mean", f, T=T, C=C, N=N, xdt=xdt, ydt=ydt))
    # ---- transpose_add_f32
    for (R, Cc, N, pad, resid) in ((1, 1, 1, 0, False), (31, 33, 3, 5, True), (32, 32, 1, 0, True), (33, 31, 1, 3, False),
                                   (1, 33, 3, 7, True), (33, 1, 1, 0, False), (32, 31, 3, 4, False), (31, 32, 1, 1, True)):
        L.append(mk("transpose", "move", R=R, Cc=Cc, N=N, pad=pad, resid=resid))
    # ---- cls_head_gemm
    for (M, K, N, G, bias, ldpad, gpad) in ((1, 32, 64, 1, True, 0, 0), (15, 128, 128, 3, True, 16, 0), (16, 160, 64, 3, False, 0, 8),
                                            (17, 32, 128, 3, True, 24, 8), (33, 160, 128, 1, True, 0, 0)):
        for f in ("exact", "poison"):
            L.append(mk("cls_head_gemm", f, M=M, K=K, N=N, G=G, bias=bias, ldpad=ldpad, gpad=gpad))
    # ---- cls_attend: L, d, H, stats given, N (, |mean| / sigma)
    A = lambda f, L_, d_, H_, st, N_, **kw: L.append(mk("cls_attend", f, L=L_, d=d_, H=H_, stats=st, N=N_, **kw))  # noqa: E731
    A("exact", 1, 64, 1, True, 1), A("exact", 32, 128, 3, True, 1), A("exact", 64, 192, 16, True, 3)
    A("needle", 31, 64, 1, True, 1), A("needle", 33, 128, 3, False, 1), A("needle", 65, 384, 16, True, 1), A("needle", 64, 448, 3, False, 3)
    A("offset", 33, 128, 3, True, 1, ratio=4), A("offset", 65, 64, 1, False, 1, ratio=4), A("offset", 32, 192, 3, True, 1, ratio=64)
    A("offset", 33, 1024, 3, False, 1, ratio=4096), A("offset", 65, 1024, 16, True, 3, ratio=4096)
    A("const", 33, 64, 3, False, 1), A("const", 1, 128, 1, False, 1)
    A("poison", 1, 64, 1, False, 1), A("poison", 31, 128, 3, True, 3), A("poison", 32, 384, 1, False, 1), A("poison", 33, 448, 16, True, 1)
    A("poison", 64, 1024, 3, False, 1), A("poison", 65, 192, 16, False, 3)
    A("perm", 33, 128, 3, True, 3), A("perm", 65, 64, 16, False, 3)
    # ---- ViT token assembly: P, H, W, N, d, cls, ldpad (weight columns beyond Kpad), generic (patch 16 through the generic kernel)
    for (P, H, W, N, dd, cls, ldpad, generic) in (
        (16, 32, 48, 1, 64, True, 0, False),     # gh 2, gw 3
        (16, 48, 16, 43, 4, False, 0, False),    # gh 3, gw 1; Mtot 129: a second row tile with one live row; d 4
        (16, 32, 32, 5, 132, True, 0, False),    # rows of five images in one tile; d % 128 = 4
        (16, 16, 16, 1, 192, False, 0, False),   # Mtot 1
        (16, 16, 16, 127, 260, True, 0, False),  # Mtot 127; three feature tiles, the last 4 wide
        (16, 32, 32, 32, 64, False, 0, False),   # Mtot 128: one full tile
        (4, 8, 12, 3, 64, True, 0, True),        # K 48 < one step
        (8, 16, 24, 1, 132, False, 8, True),     # K 192 = 3 steps; ldw > Kpad
        (14, 28, 42, 2, 4, True, 0, True),       # K 588: the last step holds 12 live columns
        (14, 42, 14, 1, 260, False, 16, True),
        (32, 32, 64, 3, 64, True, 0, True),      # K 3072
        (16, 32, 48, 1, 64, True, 8, True),      # patch 16 through the generic kernel (ldw > K)
    ):
        for f in ("exact", "locate", "locpe", "poison"):
            L.append(mk("vit_tokens", f, P=P, H=H, W=W, N=N, d=dd, cls=cls, ldpad=ldpad, generic=generic))
    # ---- row reductions
    for (C, HW, N, ldpad, xdt, ydt) in ((1, 1, 1, 0, "f32", "f32"), (37, 9, 3, 3, "bf16", "bf16"), (255, 9, 1, 0, "f32", "bf16"),
                                        (256, 1, 3, 8, "bf16", "f32"), (257, 9, 1, 0, "f32", "f32")):
        L.append(mk("mean_ln", "poison", C=C, HW=HW, N=N, ldpad=ldpad, xdt=xdt, ydt=ydt))
    for (H, W, C, N, ldpad, xdt, ydt) in ((2, 2, 1, 1, 0, "f32", "f32"), (6, 10, 37, 2, 3, "bf16", "bf16"), (2, 2, 96, 3, 0, "f32", "bf16"),
                                          (6, 10, 96, 1, 32, "bf16", "f32")):
        for f in ("locate", "poison"):
            L.append(mk("s2d", f, H=H, W=W, C=C, N=N, ldpad=ldpad, xdt=xdt, ydt=ydt))
    for (ntiles, hw, C, R, N) in ((1, 7, 5, 1, 1), (3, 49, 64, 5, 3), (3, 12, 300, 64, 2)):
        L.append(mk("se_gate", "poison", ntiles=ntiles, hw=hw, C=C, R=R, N=N))
    for (R, C, N) in ((1, 1, 1), (7, 9, 3), (1, 9, 2), (7, 1, 1)):
        L.append(mk("mean_rows", "poison", R=R, C=C, N=N))
    for (dd, M, xdt, ydt) in ((8, 1, "f32", "f32"), (512, 5, "bf16", "bf16"), (520, 3, "f32", "bf16"), (4096, 2, "bf16", "f32")):
        for f in ("offset", "poison"):
            L.append(mk("rmsnorm", f, d=dd, M=M, xdt=xdt, ydt=ydt))
    for (F, M, ldpad) in ((8, 1, 0), (136, 5, 8)):
        L.append(mk("geglu", "poison", F=F, M=M, ldpad=ldpad))
    return L


# --------------------------------------------------------------------------------------------------------------- token mixing
def build_token_mix(case: Case) -> dict:
    d, g = case.d, _gen(case)
    N, T, Dt, C = d["N"], d["T"], d["Dt"], d["C"]
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)  # noqa: E731
    if case.family == "exact":
        x = ri(-8, 9, N, T, C).float()
        stats = torch.stack([torch.zeros(N * T), torch.ones(N * T)], -1)
        gamma, beta = torch.ones(C), torch.zeros(C)
        nnz = min(4, T)
        w1 = torch.zeros(Dt, T).scatter_(1, torch.rand(Dt, T, generator=g).argsort(1)[:, :nnz], (ri(0, 2, Dt, nnz) * 2 - 1).float())
        w1[::3, T - 1] = 1.0                                    # the token next to the padding is always in play
        b1 = 64.0 * (1 - 2 * (torch.arange(Dt) % 2)).float()    # even hidden rows +64 (h = z), odd ones -64 (h = -0)
        half = Dt // 2
        a = ri(0, half, T)
        a[::2] = half - 1                                       # the last positive hidden row, Dt - 2
        b = (a + 1 + ri(0, half - 1, T)) % half
        w2 = torch.zeros(T, Dt)
        w2[torch.arange(T), 2 * a] = 1.0
        w2[torch.arange(T), 2 * b] = -1.0
        w2[torch.arange(T), 2 * ri(0, half, T) + 1] = 1.0       # a saturated row: contributes -0
        w2[:, Dt - 1] = -1.0                                    # and the very last hidden row
        b2 = ri(-16, 17, T).float()
    else:
        x = bf16r(rn(N, T, C))
        v, m = torch.var_mean(x, -1, unbiased=False)
        stats = torch.stack([m, torch.rsqrt(v + EPS)], -1).reshape(-1, 2).contiguous()
        gamma, beta = rn(C) * 0.5 + 1, rn(C) * 0.5
        b1 = rn(Dt) * 0.1
        if case.family == "needle":
            w1, w2 = torch.zeros(Dt, T), torch.zeros(T, Dt)
            c1, c2 = rn(Dt), rn(T)
            w1[:, T - 1] = bf16r(c1 + 0.25 * torch.sign(c1))
            w2[:, Dt - 1] = bf16r(c2 + 0.25 * torch.sign(c2))
            b2 = 0.5 + 0.125 * torch.arange(T).float()
        else:
            w1, w2 = bf16r(rn(Dt, T) * T ** -0.5), bf16r(rn(T, Dt) * Dt ** -0.5)
            b2 = rn(T) * 0.1
    return dict(x=x.to(torch.bfloat16), stats=stats, gamma=gamma, beta=beta, w1=w1.to(torch.bfloat16), b1=b1, w2=w2.to(torch.bfloat16), b2=b2)


def tm_reference(case: Case, inp: dict) -> dict:
    """float64, no rounding anywhere, and the bound that a kernel with the three bf16 stores of csrc/mixer.hip must keep:
    dxn   = hulp(|xn| + f) + f, f = u (2 |t g| + |xn|): (x - mean), (..) * rstd and the fma of phase 0 round once each; hulp(v) is
            half a bf16 ulp IN v's BINADE, 2^(floor(log2 v) - 8) (store_term): between 2^-9 v and 2^-8 v.  The flat 2^-9 |xn| is
            too small just above a power of two (the CPU stand-in exceeds it in the needle family, where one product carries all)
    dz1   = sum_t |w1| dxn + (Tp + 2) u A1, A1 = sum_t |w1| (|xn| + dxn) + |b1|: Tp exact products summed in fp32 in any order (the
            padding adds exact zeros but is counted), + 1 for `acc + bb`, + 1 for the first sum of a 16-wide MFMA step
    dh    = da + hulp(|h| + da), da = 1.13 dz1 + 3.7e-5 (gelu_poly, linear_cases.act_bound); the store to hs
    dy    = sum_d |w2| dh + (Dt + 2) u A2 + half a bf16 ulp, A2 = sum_d |w2| (|h| + dh) + |b2| + |x|: Dt products, and the epilogue's
            `sp + bias2` and `+ x`."""
    N, T, Dt, C = (case.d[k] for k in ("N", "T", "Dt", "C"))
    Tp = (T + 15) // 16 * 16
    x = inp["x"].double()
    mean, rstd = inp["stats"][:, 0].double().view(N, T, 1), inp["stats"][:, 1].double().view(N, T, 1)
    g, e = inp["gamma"].double(), inp["beta"].double()
    w1, w2, b1, b2 = inp["w1"].double(), inp["w2"].double(), inp["b1"].double(), inp["b2"].double()
    tg = (x - mean) * rstd * g
    xn = tg + e
    f = U32 * (2 * tg.abs() + xn.abs())
    dxn = store_term(xn.abs() + f, "bf16") + f
    z = torch.einsum("dt,ntc->ndc", w1, xn) + b1[None, :, None]
    A1 = torch.einsum("dt,ntc->ndc", w1.abs(), xn.abs() + dxn) + b1.abs()[None, :, None]
    dz = torch.einsum("dt,ntc->ndc", w1.abs(), dxn) + (Tp + 2) * U32 * A1
    if case.family == "exact":  # common.h: z >= 4.5 gives z, z <= -4.5 gives -0 (exact_preconditions holds |z| >= 4.5)
        h = torch.where(z >= 4.5, z, torch.zeros_like(z))
    else:
        h = 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))
    da = act_bound(z, h, dz, "gelu", True)
    dh = da + store_term(h.abs() + da, "bf16")
    acc = torch.einsum("td,ndc->ntc", w2, h)
    A2 = torch.einsum("td,ndc->ntc", w2.abs(), h.abs() + dh) + b2.abs()[None, :, None] + x.abs()
    pre = torch.einsum("td,ndc->ntc", w2.abs(), dh) + (Dt + 2) * U32 * A2
    want = x + acc + b2[None, :, None]
    bound = torch.zeros_like(want) if case.family == "exact" else rounded_store(want, pre, "bf16")
    return {"want": want, "bound": bound, "z": z, "h": h}


def tm_emulate(case: Case, inp: dict, mutant: str | None = None, images=None, perm=None) -> dict:
    """The kernel in fp32 torch with its three bf16 stores, in torch's summation order; `mutant`: with the named defect."""
    N, T, Dt, C = (case.d[k] for k in ("N", "T", "Dt", "C"))
    x = inp["x"].float()
    st = inp["stats"].view(N, T, 2)
    if images is not None:
        x, st = x[images], st[images]
    if perm is not None:
        x, st = x[perm], st[perm]
    mean, rstd = st[..., 0:1], st[..., 1:2]
    if mutant == "stats_image0":
        mean, rstd = mean[0:1].expand_as(mean), rstd[0:1].expand_as(rstd)
    g, e = inp["gamma"], inp["beta"]
    if mutant == "slab_offset":  # every slab reads slab 0's gamma / beta
        cs = 32 * tm_plan(T, Dt, C)["NB"]
        g, e = g[torch.arange(C) % cs], e[torch.arange(C) % cs]
    xn = bf16r(((x - mean) * rstd) * g + e)
    w1, w2 = inp["w1"].float(), inp["w2"].float()
    if mutant == "pad_token_live" and T % 16:  # the pair's padding slot holds the clamped row T - 1 and W1's padding its weight
        xn, w1 = torch.cat([xn, xn[:, T - 1:T]], 1), torch.cat([w1, w1[:, T - 1:T]], 1)
    z = torch.einsum("dt,ntc->ndc", w1, xn)
    b1 = inp["b1"][None, :, None]
    h = bf16r(gelu_poly32(z) + b1 if mutant == "gelu_before_bias" else gelu_poly32(z + b1))
    acc = torch.einsum("td,ndc->ntc", w2, h)
    if mutant == "pad_hidden_live":  # one K step too many: the 8 pad elements of hs run into the next channel's row
        acc = acc + torch.einsum("td,ndc->ntc", w2[:, :8], h.roll(-1, 2)[:, :8])
    b2 = inp["b2"][torch.arange(C) % T][None, None, :] if mutant == "b2_by_channel" else inp["b2"][None, :, None]
    y32 = acc + b2 + (0.0 if mutant == "resid_dropped" else x)
    y = y32.to(torch.bfloat16)
    src = (y32 if mutant == "row_sums_unrounded" else y.float()).reshape(-1, C // 64, 64)
    rows = torch.stack([src.sum(-1), (src * src).sum(-1)], -1) if case.get("rows") else None
    return {"y": y, "rows": rows, "guard_ok": True}


# --------------------------------------------------------------------------------------------------------------- ln_mean, transpose
def build_ln_mean(case: Case) -> dict:
    d, g = case.d, _gen(case)
    N, T, C = d["N"], d["T"], d["C"]
    if case.family == "exact":  # multiples of T: the fp32 sum is exact and acc / T is an integer that bf16 holds
        x = (torch.randint(-4, 5, (N, T, C), generator=g) * T).float()
        stats = torch.stack([torch.zeros(N * T), torch.ones(N * T)], -1)
        gamma, beta = torch.ones(C), torch.zeros(C)
    else:
        x = torch.randn(N, T, C, generator=g) * 1.5 + 0.3
        x = bf16r(x) if d["xdt"] == "bf16" else x
        v, m = torch.var_mean(x, -1, unbiased=False)
        stats = torch.stack([m, torch.rsqrt(v + EPS)], -1).reshape(-1, 2).contiguous()
        gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g)
    return dict(x=x.to(DT[d["xdt"]]), stats=stats, gamma=gamma, beta=beta)


def ln_mean_reference(case: Case, inp: dict) -> dict:
    """acc += (x - mean) * rstd over t (two roundings per term, T - 1 additions: (T + 1) u S, S = sum |t|), acc / T (u), the fma (u)."""
    d = case.d
    N, T, C = d["N"], d["T"], d["C"]
    x = inp["x"].double()
    st = inp["stats"].double().view(N, T, 2)
    t = (x - st[..., 0:1]) * st[..., 1:2]
    S = t.abs().sum(1)
    m = t.sum(1) / T
    g, e = inp["gamma"].double(), inp["beta"].double()
    want = m * g + e
    pre = g.abs() * ((T + 1) * U32 * S / T + U32 * m.abs()) + U32 * want.abs()
    bound = torch.zeros_like(want) if case.family == "exact" else rounded_store(want, pre, d["ydt"])
    return {"want": want, "bound": bound}


def ln_mean_emulate(case, inp, mutant=None):
    d = case.d
    st = inp["stats"].view(d["N"], d["T"], 2)
    t = (inp["x"].float() - st[..., 0:1]) * st[..., 1:2]
    return {"y": ((t.sum(1) / d["T"]) * inp["gamma"] + inp["beta"]).to(DT[d["ydt"]]), "guard_ok": True}


def build_transpose(case: Case) -> dict:
    d, g = case.d, _gen(case)
    x = torch.randn(d["N"], d["R"], d["Cc"], generator=g)
    return dict(x=x, resid=torch.randn(d["N"], d["Cc"], d["R"], generator=g) if d["resid"] else None)


def transpose_reference(case, inp):
    want = inp["x"].transpose(1, 2) + inp["resid"] if inp["resid"] is not None else inp["x"].transpose(1, 2)  # ONE fp32 addition
    return {"want": want.contiguous().double(), "bound": torch.zeros(want.shape, dtype=torch.float64)}


def transpose_emulate(case, inp, mutant=None):
    d = case.d
    N, R, Cc, ldy = d["N"], d["R"], d["Cc"], d["R"] + d["pad"]
    buf = torch.full((N * Cc * ldy,), SENT32, dtype=torch.int32).view(torch.float32)
    val = inp["x"].transpose(1, 2) + inp["resid"] if inp["resid"] is not None else inp["x"].transpose(1, 2)
    ld = R if mutant == "transpose_ldy" else ldy
    o = (torch.arange(N)[:, None, None] * Cc + torch.arange(Cc)[None, :, None]) * ld + torch.arange(R)[None, None, :]
    buf[o.reshape(-1)] = val.reshape(-1)
    full = buf.view(N, Cc, ldy)
    return {"y": full[:, :, :R].contiguous(), "guard_ok": bool((full[:, :, R:].contiguous().view(torch.int32) == SENT32).all())}


# --------------------------------------------------------------------------------------------------------------- cls_head_gemm
def build_cls_head_gemm(case: Case) -> dict:
    d, g = case.d, _gen(case)
    M, K, N, G = d["M"], d["K"], d["N"], d["G"]
    xg = K + d["gpad"]
    ldx = (G - 1) * xg + K + d["ldpad"]
    if case.family == "exact":
        x = torch.randint(-4, 5, (M, ldx), generator=g).float()
        w = torch.randint(-2, 3, (G, N, K), generator=g).float()
        bias = torch.randint(-8, 9, (G, N), generator=g).float() if d["bias"] else None
        if bias is not None:  # row 0's features 0 and 1 of every group: the bf16 ties 257 (-> 256, even) and 259 (-> 260)
            for gi in range(G):
                dot = x[0, gi * xg:gi * xg + K] @ w[gi, :2].T
                bias[gi, 0], bias[gi, 1] = 257.0 - dot[0], 259.0 - dot[1]
    else:
        x = bf16r(torch.randn(M, ldx, generator=g))
        w = bf16r(torch.randn(G, N, K, generator=g) * K ** -0.5)
        bias = torch.randn(G, N, generator=g) if d["bias"] else None
    return dict(x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), bias=bias, xg=xg, ldx=ldx)


def cls_head_gemm_forward(case, inp, dtype, mutant=None):
    d = case.d
    M, K, N, G, xg = d["M"], d["K"], d["N"], d["G"], inp["xg"]
    outs, As = [], []
    for gi in range(G):
        off = gi * (K if mutant == "group_stride" else xg)
        xs, wg = inp["x"][:, off:off + K].to(dtype), inp["w"][gi].to(dtype)
        if mutant == "wave3_lost":
            xs = xs * ((torch.arange(K) // 32) % 4 != 3).to(dtype)
        b = 0.0 if inp["bias"] is None else inp["bias"][0 if mutant == "bias_group0" else gi].to(dtype)
        outs.append(xs @ wg.T + b)
        As.append(xs.abs() @ wg.abs().T + (0.0 if inp["bias"] is None else inp["bias"][gi].abs().to(dtype)))
    return torch.stack(outs, 1), torch.stack(As, 1)


def cls_head_gemm_reference(case, inp):
    """K exact products in fp32: each wave's chain, the three additions of the four wave partials and the bias: (K + 4) u A."""
    want, A = cls_head_gemm_forward(case, inp, torch.float64)
    if case.family == "exact":  # every sum is exact in fp32: the ONE rounding is the store
        return {"want": want.float().to(torch.bfloat16).double(), "bound": torch.zeros_like(want), "sum": want}
    return {"want": want, "bound": rounded_store(want, (case.d["K"] + 4) * U32 * A, "bf16")}


def cls_head_gemm_emulate(case, inp, mutant=None):
    y32 = cls_head_gemm_forward(case, inp, torch.float32, mutant)[0]
    return {"y": bf16_trunc(y32).to(torch.bfloat16) if mutant == "trunc_store" else y32.to(torch.bfloat16), "guard_ok": True}


# --------------------------------------------------------------------------------------------------------------- cls_attend
ATT_SCALE = 0.125
EXP_REL = 2.0 ** -22  # __expf(a) within 2^-22 (|a| + 1) relative (2b)
NEEDLE_GAP = 30.0


def needle_rows(L: int, H: int) -> list[int]:
    """The needle's row per head: the last real row (of a ragged last block where L % 32), then 0, 31, 32 where they exist."""
    return [min((L - 1, 0, 31, 32)[h % 4], L - 1) for h in range(H)]


def _att_stats(x: torch.Tensor, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    x = x.to(dtype)
    m = x.mean(-1)
    return m, torch.rsqrt(((x - m[..., None]) ** 2).mean(-1) + EPS)


def build_cls_attend(case: Case) -> dict:
    d, g = case.d, _gen(case)
    N, L, dd, H = d["N"], d["L"], d["d"], d["H"]
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if case.family == "exact":  # every weight is 1, 1 / l is exact (L a power of two), the mean of L multiples of L is an integer
        x = (torch.randint(-3, 4, (N, L, dd), generator=g) * L).float()
        u = torch.zeros(N, H, dd)
        stats = torch.stack([torch.zeros(N * L), torch.ones(N * L)], -1)
        return dict(x=x.to(torch.bfloat16), u=u.to(torch.bfloat16), stats=stats)
    if case.family == "const":
        x = torch.randint(-4, 5, (N, L, 1), generator=g).float().expand(N, L, dd).contiguous()
    else:
        sigma = 0.25 + 1.5 * torch.rand(N, L, 1, generator=g)
        mean = rn(N, L, 1) * 0.5
        if case.family == "offset":
            mean = sigma * d["ratio"] * torch.sign(mean)
        x = bf16r(mean + sigma * rn(N, L, dd))
        if case.family == "offset" and d["ratio"] >= 1024:
            # bf16 cannot hold a Gaussian row at this ratio (its spacing at M is M / 128): a row is M = +-2^k with ONE element one
            # ulp higher, sigma = (M / 128) sqrt(1 / d - 1 / d^2) = M / 4096 at d = 1024
            M = torch.sign(mean) * 2.0 ** torch.randint(2, 6, (N, L, 1), generator=g).float()
            x = M.expand(N, L, dd).clone()
            x.scatter_(2, torch.randint(0, dd, (N, L, 1), generator=g), M * (1 + 2.0 ** -7))
    u = rn(N, H, dd) * (16.0 / dd ** 0.5)
    if case.family == "offset":  # the fp32 error of a score grows with |mean| sum |u|: a u that shrinks with the ratio keeps the bound telling
        u = u * min(1.0, 4.0 / d["ratio"])
    if case.family == "needle":  # u along the needle's normalised row: its score is d a, every other one a (xhat* . xhat_j)
        m, r = _att_stats(x, torch.float64)
        xh = (x.double() - m[..., None]) * r[..., None]
        for h, j in enumerate(needle_rows(L, H)):
            dots = torch.einsum("nc,nlc->nl", xh[:, j], xh)
            others = dots.clone()
            others[:, j] = -float("inf")
            top = others.amax(1) if L > 1 else torch.zeros(N, dtype=torch.float64)
            a = NEEDLE_GAP / (ATT_SCALE * (dots[:, j] - top))
            u[:, h] = (a[:, None] * xh[:, j]).float()
    stats = None
    if d["stats"]:
        m, r = _att_stats(x, torch.float32)
        stats = torch.stack([m, r], -1).reshape(-1, 2).contiguous()
    return dict(x=x.to(torch.bfloat16), u=bf16r(u).to(torch.bfloat16), stats=stats)


def cls_attend_reference(case: Case, inp: dict) -> dict:
    """float64 from the bf16 x and u and the f32 stats given (none: fp64 stats of the bf16 rows).  With pi the softmax weights,
    r = rstd, m = mean, B_c = sum_j pi_j r_j |x_jc - m_j|, k = 8 ceil(d / 512) + 6 (a lane's chain and the wave tree of the in-kernel
    statistics), nb = the blocks of 32 rows, na = 34 nb + 4 (a block's 32 MFMA terms, its rescale and its fma; sum16):
      ds_j  = scale r_j ((d + 4) u sum_c |u_c x_jc| + (d + 6) u |m_j| sum_c |u_c|) + 3 u |s_j|      [S in four wave partials, su, the
              product and the difference, then the two factors]  (+ scale r_j dm_j |sum u| + drel_j |s_j| with in-kernel statistics)
      de_j  = ds_j + 2^-22 (3 |s_j - max| + nb)                    [__expf of s - m_block and of every later block's rescale]
      E     = sum_j pi_j r_j |x_jc - m_j| (de_j + sum_i pi_i de_i)   [the normalised weights]
            + 2^-8 B_c                                             [w = bf16(p r): a relative half ulp is at most 2^-8; BOTH sums use
                                                                    the same w and l the unrounded p: the dominant term]
            + na u (1 + 2^-8) sum_j pi_j r_j (|x_jc| + |m_j|) + (na + 3) u |ctx|     [acc, cm, l, acc - cm, 1 / l, the product]
            + sum_j pi_j r_j (dm_j + drel_j |x_jc - m_j|)            [in-kernel statistics only]
      + half a bf16 ulp of the result."""
    d = case.d
    N, L, dd, H = d["N"], d["L"], d["d"], d["H"]
    x, u = inp["x"].double(), inp["u"].double()
    if inp["stats"] is not None:
        st = inp["stats"].double().view(N, L, 2)
        m, r = st[..., 0], st[..., 1]
        dm = drel = torch.zeros(N, L, dtype=torch.float64)
    else:
        m, r = _att_stats(x, torch.float64)
        k = 8 * -(-dd // 512) + 6
        var = ((x - m[..., None]) ** 2).mean(-1)
        dm = (k + 2) * U32 * x.abs().mean(-1)
        drel = 0.5 * ((k + 3) * U32 + dm * dm / (var + EPS)) + 2 * U32
    S, su = torch.einsum("nhc,nlc->nhl", u, x), u.sum(-1)
    s = ATT_SCALE * r[:, None] * (S - m[:, None] * su[..., None])
    pi = torch.softmax(s, -1)
    xc = x - m[..., None]
    want = torch.einsum("nhl,nlc->nhc", pi * r[:, None], xc)
    if case.family == "exact":
        return {"want": want, "bound": torch.zeros_like(want), "s": s, "pi": pi}
    nb = -(-L // 32)
    na = 34 * nb + 4
    ds = ATT_SCALE * r[:, None] * ((dd + 4) * U32 * torch.einsum("nhc,nlc->nhl", u.abs(), x.abs())
                                   + (dd + 6) * U32 * m.abs()[:, None] * u.abs().sum(-1)[..., None]) + 3 * U32 * s.abs()
    ds = ds + ATT_SCALE * r[:, None] * dm[:, None] * su.abs()[..., None] + drel[:, None] * s.abs()
    de = ds + EXP_REL * (3 * (s - s.amax(-1, keepdim=True)).abs() + nb)
    de = de + (pi * de).sum(-1, keepdim=True)
    pr = pi * r[:, None]
    B = torch.einsum("nhl,nlc->nhc", pr, xc.abs())
    pre = torch.einsum("nhl,nlc->nhc", pr * de, xc.abs()) + 2.0 ** -8 * B
    pre = pre + na * U32 * (1 + 2.0 ** -8) * (torch.einsum("nhl,nlc->nhc", pr, x.abs()) + (pr * m.abs()[:, None]).sum(-1, keepdim=True))
    pre = pre + (na + 3) * U32 * want.abs()
    pre = pre + (pr * dm[:, None]).sum(-1, keepdim=True) + torch.einsum("nhl,nlc->nhc", pr * drel[:, None], xc.abs())
    return {"want": want, "bound": rounded_store(want, pre, "bf16"), "s": s, "pi": pi, "m": m, "r": r}


def cls_attend_emulate(case: Case, inp: dict, mutant: str | None = None, images=None, perm=None) -> dict:
    """The kernel's blocks of 32 rows in fp32 torch: online softmax, w = bf16(p rstd) in BOTH sums, l over the unrounded p."""
    x, u, st = inp["x"].float(), inp["u"].float(), inp["stats"]
    N, L, dd = x.shape
    H = u.shape[1]
    st = None if st is None else st.view(N, L, 2)
    sel = images if images is not None else perm
    if sel is not None:
        x, u, st = x[sel], u[sel], None if st is None else st[sel]
        N = len(sel)
    mean, rstd = _att_stats(x, torch.float32) if st is None else (st[..., 0], st[..., 1])
    su = u.sum(-1)
    if mutant == "head_pad_leak":  # the sum of u comes from the next head's lanes
        su = su[:, (torch.arange(H) + 1).clamp(max=H - 1)]
    s = ATT_SCALE * rstd[:, None] * (torch.einsum("nhc,nlc->nhl", u, x) - mean[:, None] * su[..., None])
    m_run = torch.full((N, H), -float("inf"))
    l, cm, acc = torch.zeros(N, H), torch.zeros(N, H), torch.zeros(N, H, dd)
    for j0 in range(0, L, 32):
        idx = torch.arange(j0, min(L, j0 + 32))
        if mutant == "tail_rows_live" and idx.numel() < 32:  # the clamped tail rows keep row L - 1's score
            idx = torch.cat([idx, torch.full((32 - idx.numel(),), L - 1)])
        sb, xb, rb, mb = s[..., idx], x[:, idx], rstd[:, None, idx], mean[:, None, idx]
        m_new = torch.maximum(m_run, sb.amax(-1))
        alpha = torch.ones_like(m_new) if mutant == "no_rescale" else torch.exp(m_run - m_new)
        p = torch.exp(sb - m_new[..., None])
        w = bf16r(p if mutant == "rstd_once" else p * rb)
        l = l * alpha + p.sum(-1)
        cm = cm * alpha + ((p * rb if mutant == "cm_unrounded" else w) * mb).sum(-1)
        acc = acc * alpha[..., None] + torch.einsum("nhj,njc->nhc", w, xb)
        m_run = m_new
    if mutant == "mean_dropped":
        cm = torch.zeros_like(cm)
    return {"y": ((acc - cm[..., None]) / l[..., None]).to(torch.bfloat16), "guard_ok": True}



# --------------------------------------------------------------------------------------------------------------- ViT tokens
def vit_geometry(case: Case) -> dict:
    d = case.d
    P, H, W = d["P"], d["H"], d["W"]
    K = 3 * P * P
    generic = P != 16 or d["ldpad"] > 0 or d["generic"]
    Kpad = -(-K // 64) * 64
    return dict(K=K, Kpad=Kpad, ldw=(Kpad + d["ldpad"]) if generic else K, generic=generic, gh=H // P, gw=W // P, L=(H // P) * (W // P))


def vit_index(case: Case, mutant: str | None = None) -> torch.Tensor:
    """(N, L, K) flat indices into imgs (N, 3, H, W): patch p = gy gw + gx, k = (c P + ph) P + pw."""
    d, geo = case.d, vit_geometry(case)
    P, H, W, N = d["P"], d["H"], d["W"], d["N"]
    p = torch.arange(geo["L"])
    gy, gx = (p % geo["gh"], p // geo["gh"]) if mutant == "gy_gx_swapped" else (p // geo["gw"], p % geo["gw"])
    k = torch.arange(geo["K"])
    c, ph, pw = k // (P * P), (k % (P * P)) // P, k % P
    cs = W * W if mutant == "channel_stride" else H * W
    idx = (c * cs)[None, :] + (gy[:, None] * P + ph[None, :]) * W + gx[:, None] * P + pw[None, :]
    return (torch.arange(N)[:, None, None] * 3 * H * W + idx[None]).clamp(max=N * 3 * H * W - 1)


def build_vit_tokens(case: Case) -> dict:
    d, g, geo = case.d, _gen(case), vit_geometry(case)
    N, H, W, dd, K, L = d["N"], d["H"], d["W"], d["d"], geo["K"], geo["L"]
    npx = N * 3 * H * W
    w = torch.zeros(dd, geo["ldw"])
    if case.family == "exact":
        imgs = torch.randint(-4, 5, (N, 3, H, W), generator=g).float()
        imgs[0, 0, 0, 0], imgs[0, 0, 0, 1] = 259.0, 257.0  # pixels on bf16 ties of both parities (-> 260, 256)
        w[:, :K] = torch.randint(-2, 3, (dd, K), generator=g).float()
        w[:, :2] = 1.0
        bias, pe = torch.randint(-8, 9, (dd,), generator=g).float(), torch.randint(-8, 9, (L, dd), generator=g).float()
        cls = torch.randint(-300, 301, (dd,), generator=g).float() + 0.5
        pix = bf16r(imgs.flatten()[vit_index(case)[0, 0]])
        dot = pix @ w[:2, :K].T + bias[:2]
        pe[0, 0], pe[0, 1] = 257.0 - dot[0], 259.0 - dot[1]  # image 0, patch 0: output ties of both parities
    elif case.family in ("locate", "locpe"):
        code = lambda n, base: ((base + torch.arange(n) % 16384).to(torch.int32) << 16).view(torch.float32)  # noqa: E731
        w[torch.arange(dd), (torch.arange(dd) * 37 + 11) % K] = 1.0
        bias = torch.zeros(dd)
        if case.family == "locate":  # 0.75 ulp above a code: round-to-nearest gives the NEXT code, truncation this one
            imgs = (((CODE0 + torch.arange(npx) % 16384).to(torch.int32) << 16) | 0xC000).view(torch.float32).view(N, 3, H, W)
            pe, cls = torch.zeros(L, dd), code(dd, CODE0 + 14000)
        else:
            imgs, pe, cls = torch.zeros(N, 3, H, W), code(L * dd, CODE0).view(L, dd), code(dd, CODE0 + 14000)
    else:
        imgs = torch.randn(N, 3, H, W, generator=g)
        w[:, :K] = bf16r(torch.randn(dd, K, generator=g) * K ** -0.5)
        bias, pe, cls = torch.randn(dd, generator=g), torch.randn(L, dd, generator=g), torch.randn(dd, generator=g)
    return dict(imgs=imgs, w=w.to(torch.bfloat16), bias=bias, pe=pe, cls=cls if d["cls"] else None)


def vit_forward(case, inp, dtype, mutant=None):
    d, geo = case.d, vit_geometry(case)
    K, L, N = geo["K"], geo["L"], d["N"]
    raw = inp["imgs"].flatten()[vit_index(case, mutant)]
    pix = (bf16_trunc(raw) if mutant == "pixel_trunc" else bf16r(raw)).to(dtype)
    w = inp["w"].to(dtype)
    acc, A = pix @ w[:, :K].T, pix.abs() @ w[:, :K].abs().T
    if mutant == "generic_tail_live" and geo["generic"] and geo["Kpad"] > K:  # the tail of the last K step wraps to the patch's start
        acc = acc + pix[..., :geo["Kpad"] - K] @ w[:, :geo["Kpad"] - K].T
    pe = inp["pe"].to(dtype)
    if mutant == "pe_shifted_by_cls" and inp["cls"] is not None:
        pe = pe.roll(-1, 0)
    v = acc + inp["bias"].to(dtype) + pe
    A = A + inp["bias"].abs().to(dtype) + pe.abs()
    if inp["cls"] is None:
        return v, A
    c = inp["cls"].to(dtype)
    if mutant == "cls_every_row":
        v = v + c
    return torch.cat([c.expand(N, 1, -1), v], 1), torch.cat([torch.zeros(N, 1, d["d"], dtype=dtype), A], 1)


def vit_reference(case, inp):
    """K exact products of bf16-rounded pixels in fp32, `acc + bias + pe`: (K + 3) u A + half a bf16 ulp; the cls row is ONE rounding."""
    want, A = vit_forward(case, inp, torch.float64)
    if case.family in ("exact", "locate", "locpe"):
        return {"want": want.float().to(torch.bfloat16).double(), "bound": torch.zeros_like(want), "sum": want}
    bound = rounded_store(want, (vit_geometry(case)["K"] + 3) * U32 * A, "bf16")
    if inp["cls"] is not None:
        want[:, 0], bound[:, 0] = bf16r(inp["cls"]).double(), 0.0
    return {"want": want, "bound": bound}


def vit_emulate(case, inp, mutant=None):
    return {"y": vit_forward(case, inp, torch.float32, mutant)[0].to(torch.bfloat16), "guard_ok": True}


# --------------------------------------------------------------------------------------------------------------- row reductions
def ln_two_pass(s: torch.Tensor, gamma, beta, k: int, eps: float, ds=None):
    """LayerNorm over the last dim of s (float64) and the bound of the kernels' two-pass fp32 form, whose sums are chains / trees of
    depth k: dm = (k + 2) u mean |s| (the sum and `* inv_c`); the centred values carry dm + u |s - m|; the variance of the centred
    values (k + 3) u relative + dm^2, rsqrtf 2 u: dr / r = ((k + 3) u + dm^2 / (var + eps)) / 2 + 2 u; y = fma((s - m) r, g, b):
    |g| r (dm + u |s - m|) + |g yhat| (dr / r + 2 u) + u |y|.  ds: an error the INPUT already carries (mean_ln's column means):
    + |g| r (ds + mean ds + |yhat| max ds)."""
    m = s.mean(-1, keepdim=True)
    var = ((s - m) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    yhat = (s - m) * r
    want = yhat * gamma + beta
    dm = (k + 2) * U32 * s.abs().mean(-1, keepdim=True)
    drel = 0.5 * ((k + 3) * U32 + dm * dm / (var + eps)) + 2 * U32
    pre = gamma.abs() * r * (dm + U32 * (s - m).abs()) + (gamma * yhat).abs() * (drel + 2 * U32) + U32 * want.abs()
    if ds is not None:
        pre = pre + gamma.abs() * r * (ds + ds.mean(-1, keepdim=True) + yhat.abs() * ds.amax(-1, keepdim=True))
    return want, pre


def _xin(g, shape, dt, scale=1.5, shift=0.3):
    x = torch.randn(*shape, generator=g) * scale + shift
    return (bf16r(x) if dt == "bf16" else x).to(DT[dt])


def build_rows(case: Case) -> dict:
    d, g = case.d, _gen(case)
    op = case.op
    if op == "mean_ln":
        x = _xin(g, (d["N"], d["HW"], d["C"] + d["ldpad"]), d["xdt"])
        return dict(x=x, gamma=torch.randn(d["C"], generator=g) * 0.5 + 1, beta=torch.randn(d["C"], generator=g))
    if op == "s2d":
        x = _xin(g, (d["N"], d["H"], d["W"], d["C"] + d["ldpad"]), d["xdt"])
        gamma, beta = torch.randn(d["C"], generator=g) * 0.5 + 1, torch.randn(d["C"], generator=g)
        if case.family == "locate":
            gamma, beta = torch.ones(d["C"]), torch.zeros(d["C"])
        return dict(x=x, gamma=gamma, beta=beta)
    if op == "se_gate":
        C, R = d["C"], d["R"]
        return dict(psum=torch.randn(d["N"], d["ntiles"], C, generator=g) * d["hw"] / d["ntiles"], w1=torch.randn(R, C, generator=g) * C ** -0.5,
                    b1=torch.randn(R, generator=g), w2=torch.randn(C, R, generator=g), b2=torch.randn(C, generator=g))
    if op == "mean_rows":
        return dict(x=_xin(g, (d["N"], d["R"], d["C"]), "bf16"))
    if op == "rmsnorm":
        x = _xin(g, (d["M"], d["d"]), d["xdt"], *((3.0 / 64, 3.0) if case.family == "offset" else (1.5, 0.0)))
        return dict(x=x, gamma=torch.randn(d["d"], generator=g) * 0.5 + 1)
    return dict(h=_xin(g, (d["M"], 2 * d["F"] + d["ldpad"]), "bf16", 1.5, 0.0))


def rows_forward(case: Case, inp: dict, dtype, mutant=None) -> tuple[torch.Tensor, torch.Tensor | None]:
    """(result, bound before the store | None): dtype float64 is the reference, float32 the stand-in (torch's summation order)."""
    d, op = case.d, case.op
    ref = dtype == torch.float64
    if op == "mean_ln":  # a thread's chain over HW rows, `* inv_hw`; LN over C: chain ceil(C / 256), wave tree 6, 4 partials
        C, HW = d["C"], d["HW"]
        x = inp["x"][..., :C].to(dtype)
        g, b = inp["gamma"].to(dtype), inp["beta"].to(dtype)
        if mutant == "ln_of_mean_for_mean_of_ln":
            return ln_two_pass(x, g, b, 0, EPS)[0].mean(1), None
        s = x.mean(1)
        want, pre = ln_two_pass(s, g, b, -(-C // 256) + 10, EPS, (HW + 1) * U32 * x.abs().mean(1) if ref else None)
        return want, pre
    if op == "s2d":  # per pixel: chain ceil(C / 64), wave tree 6; the quadrants k = 2 dh + dw side by side, zeros behind
        C, N, H, W = d["C"], d["N"], d["H"], d["W"]
        x = inp["x"][..., :C].to(dtype)
        want, pre = ln_two_pass(x, inp["gamma"].to(dtype), inp["beta"].to(dtype), -(-C // 64) + 6, EPS)
        order = ((0, 0), (1, 0), (0, 1), (1, 1)) if mutant == "s2d_quadrants" else ((0, 0), (0, 1), (1, 0), (1, 1))
        ldy = -(-4 * C // 64) * 64 if d["ldpad"] == 0 else 4 * C + d["ldpad"]
        cat = lambda t: torch.cat([t[:, a::2, b::2] for a, b in order] + [torch.zeros(N, H // 2, W // 2, ldy - 4 * C, dtype=dtype)], -1)  # noqa: E731
        return cat(want).reshape(-1, ldy), cat(pre).reshape(-1, ldy)
    if op == "se_gate":
        ps = inp["psum"].to(dtype)
        m = ps.sum(1) / (d["ntiles"] if mutant == "se_div_ntiles" else d["hw"])
        w1, b1, w2, b2 = (inp[k].to(dtype) for k in ("w1", "b1", "w2", "b2"))
        z1 = m @ w1.T + b1
        hid = z1 * torch.sigmoid(z1)
        z2 = hid @ w2.T + b2
        want = torch.sigmoid(z2)
        if not ref:
            return want, None
        # the tile chain and `* inv_hw` (1.0f / hw is itself rounded): (ntiles + 2) u; FC1: chain ceil(C / 64), tree 6, bias; FC2: R fmas
        dm = (d["ntiles"] + 2) * U32 * ps.abs().sum(1) / d["hw"]
        dz1 = dm @ w1.abs().T + (-(-d["C"] // 64) + 8) * U32 * (m.abs() @ w1.abs().T + b1.abs())
        dh = act_bound(z1, hid, dz1, "silu", False)
        dz2 = dh @ w2.abs().T + (d["R"] + 2) * U32 * (hid.abs() @ w2.abs().T + b2.abs())
        return want, 0.25 * dz2 + 4 * U32 * want + TINY
    if op == "mean_rows":
        x = inp["x"].to(dtype)
        return x.mean(1), (d["R"] + 1) * U32 * x.abs().mean(1)
    if op == "rmsnorm":  # a lane's chain of 8 ceil(d / 512) squares, wave tree 6; no centring
        x, g = inp["x"].to(dtype), inp["gamma"].to(dtype)
        xc = x - x.mean(-1, keepdim=True) if mutant == "rms_centred" else x
        want = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS) * g
        k = 8 * -(-d["d"] // 512) + 6
        return want, want.abs() * (0.5 * (k + 3) * U32 + 2 * U32 + 2 * U32)
    F = d["F"]  # geglu: gelu_tanh in fp32 with tanhf (2d's approximate_gelu term), one product
    a, b = inp["h"][:, :F].to(dtype), inp["h"][:, F:2 * F].to(dtype)
    if mutant == "geglu_halves_swapped":
        a, b = b, a
    gl = 0.5 * a * (1.0 + torch.tanh(0.7978845608028654 * (0.044715 * a * a * a + a)))
    want = gl * b
    return want, act_bound(a, gl, torch.zeros_like(a), "approximate_gelu", False) * b.abs() + U32 * want.abs()


def rows_out_dt(case: Case) -> str:
    return case.get("ydt", "f32" if case.op == "se_gate" else "bf16")


def rows_reference(case: Case, inp: dict) -> dict:
    want, pre = rows_forward(case, inp, torch.float64)
    return {"want": want, "bound": rounded_store(want, pre, rows_out_dt(case))}  # s2d's pad columns: want 0, bound 0


def tm_rows_reference(y: torch.Tensor, exact: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """The row partials of the kernel's OWN rounded output, and the bound of an fp32 sum of 64 terms in any order (the argument of
    tests/test_hip_mixer.py; squares of bf16 values are exact in fp32)."""
    blk = y.double().reshape(-1, y.shape[-1] // 64, 64)
    want = torch.stack([blk.sum(-1), (blk * blk).sum(-1)], -1)
    bound = 64 * U32 * torch.stack([blk.abs().sum(-1), (blk * blk).sum(-1)], -1)
    return want, torch.zeros_like(bound) if exact else bound


def rows_emulate(case, inp, mutant=None):
    return {"y": rows_forward(case, inp, torch.float32, mutant)[0].to(DT[rows_out_dt(case)]), "guard_ok": True}


# --------------------------------------------------------------------------------------------------------------- the verdict
ROW_OPS = ("mean_ln", "s2d", "se_gate", "mean_rows", "rmsnorm", "geglu")
_BUILD = {"token_mix": build_token_mix, "ln_mean": build_ln_mean, "transpose": build_transpose, "cls_head_gemm": build_cls_head_gemm,
          "vit_tokens": build_vit_tokens, "cls_attend": build_cls_attend, **dict.fromkeys(ROW_OPS, build_rows)}
_REFERENCE = {"token_mix": tm_reference, "ln_mean": ln_mean_reference, "transpose": transpose_reference,
              "cls_head_gemm": cls_head_gemm_reference, "vit_tokens": vit_reference, "cls_attend": cls_attend_reference, **dict.fromkeys(ROW_OPS, rows_reference)}
_EMULATE = {"token_mix": tm_emulate, "ln_mean": ln_mean_emulate, "transpose": transpose_emulate, "cls_head_gemm": cls_head_gemm_emulate,
            "vit_tokens": vit_emulate, "cls_attend": cls_attend_emulate, **dict.fromkeys(ROW_OPS, rows_emulate)}


def build(case: Case) -> dict:
    return _BUILD[case.op](case)


def reference(case: Case, inp: dict) -> dict:
    return _REFERENCE[case.op](case, inp)


class StandIn:
    """The ops on the CPU in fp32 with the kernels' rounding points and torch's summation order: a correct kernel's stand-in, or,
    with `mutant`, what a kernel with the named defect returns (a mutant only changes the op it is planted in)."""

    def __init__(self, mutant: str | None = None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def run(self, case: Case, inp: dict, poison: bool = False, **kw) -> dict:
        m = self.mutant if self.mutant and MUTANT_OF[self.mutant][0] == case.op else None
        if case.op in ("token_mix", "cls_attend"):
            kw.pop("inplace", None)
            return _EMULATE[case.op](case, inp, m, **kw)
        return _EMULATE[case.op](case, inp, m)


def exact_preconditions(case: Case, inp: dict, ref: dict) -> list[str]:
    """What makes the exact / needle / locate / offset families mean what they say; every entry of the result is a broken precondition."""
    bad, d = [], case.d
    isint = lambda t: bool((t == t.round()).all())  # noqa: E731
    if case.op == "token_mix" and case.family == "exact":
        z, want = ref["z"], ref["want"]
        if not (isint(z) and float(z.abs().min()) >= 4.5):
            bad.append("a pre-activation is no integer with |z| >= 4.5")
        gp = gelu_poly32(z.float())
        if not torch.equal(gp, torch.where(z >= 4.5, z, torch.zeros_like(z)).float()) or bool((gp[z < 0] != 0).any()):
            bad.append("gelu_poly does not return z / -0 on these pre-activations")
        if not (isint(ref["h"]) and float(ref["h"].abs().max()) <= 256):
            bad.append("a hidden activation is no bf16-exact integer")
        if not (isint(want) and float(want.abs().max()) <= 256 and torch.equal(bf16r(want), want)):
            bad.append("an output is no bf16-exact integer")
        if not float((want * want).reshape(-1, d["C"] // 64, 64).sum(-1).max()) < 2 ** 24:
            bad.append("a row block's sum of squares reaches 2^24")
        w1 = inp["w1"].float()
        if not (bool((w1[:, d["T"] - 1] != 0).any()) and int((w1 != 0).sum(1).max()) <= 5):
            bad.append("W1: the last token unused, or more than five non-zeros in a row")
    if case.op == "token_mix" and case.family == "needle":
        w1, w2, T, Dt = inp["w1"].float(), inp["w2"].float(), d["T"], d["Dt"]
        if bool((w1[:, :T - 1] != 0).any()) or bool((w1[:, T - 1] == 0).any()) or bool((w2[:, :Dt - 1] != 0).any()) or bool((w2[:, Dt - 1] == 0).any()):
            bad.append("the needles are not alone")
        if inp["b2"].unique().numel() != T:
            bad.append("b2 is not distinct per token")
    if case.op in ("cls_head_gemm", "vit_tokens") and case.family == "exact":
        s = ref["sum"]
        body = s if case.op == "cls_head_gemm" or not d.get("cls") else s[:, 1:]
        if not (isint(body) and float(body.abs().max()) < 2 ** 23):
            bad.append("a sum is not exact in fp32")
        first = s[0, :, :2] if case.op == "cls_head_gemm" else s[0, 1 if d.get("cls") else 0, :2]
        planted = case.op == "vit_tokens" or d["bias"]
        if planted and not (bool((first.reshape(-1, 2)[:, 0] == 257).all()) and bool((first.reshape(-1, 2)[:, 1] == 259).all())):
            bad.append("the planted ties 257 / 259 are not there")
        t = torch.tensor([257.0, 259.0])
        if not (torch.equal(t.to(torch.bfloat16).float(), torch.tensor([256.0, 260.0])) and torch.equal(bf16_trunc(t), torch.tensor([256.0, 258.0]))):
            bad.append("257 / 259 are no bf16 ties of both parities")
    if case.op == "vit_tokens" and case.family == "locate":
        px = inp["imgs"].flatten()
        n = min(px.numel(), 16384)
        if px[:n].unique().numel() != n or not torch.equal(bits(px.to(torch.bfloat16))[:n].int(), CODE0 + 1 + torch.arange(n, dtype=torch.int32)):
            bad.append("the pixel codes are not distinct, or do not round up to the next code")
        if not torch.equal(bits(bf16_trunc(px).to(torch.bfloat16))[:n].int(), CODE0 + torch.arange(n, dtype=torch.int32)):
            bad.append("truncation does not give the code below")
    if case.op == "vit_tokens" and case.family == "locpe" and inp["pe"].unique().numel() != inp["pe"].numel():
        bad.append("the pe codes are not distinct")
    if case.op == "rmsnorm" and case.family == "offset":
        x = inp["x"].double()
        rt = x.mean(-1).abs() / x.std(-1, unbiased=False).clamp_min(1e-30)
        if d["d"] >= 512 and not bool(((rt > 48) & (rt < 85)).all()):
            bad.append("|mean| / sigma is not 64")
    if case.op == "cls_attend":
        L, H = d["L"], d["H"]
        if case.family == "exact" and not (bool((ref["pi"] == 1.0 / L).all()) and isint(ref["want"]) and float(ref["want"].abs().max()) <= 256):
            bad.append("the weights are not 1 / L, or a mean of the rows is no bf16-exact integer")
        if case.family == "needle" and L > 1:
            for h, j in enumerate(needle_rows(L, H)):
                rest = ref["s"][:, h].clone()
                rest[:, j] = -float("inf")
                gap = ref["s"][:, h, j] - rest.amax(-1)
                if not bool(((gap > 25) & (gap < 35)).all()):
                    bad.append(f"head {h}: the needle at row {j} is {gap.tolist()} above the rest, not 30")
        if case.family == "offset":
            x = inp["x"].double()
            rt = x.mean(-1).abs() / x.std(-1, unbiased=False)
            if not bool(((rt > d["ratio"] / 2) & (rt < d["ratio"] * 2)).all()):
                bad.append(f"|mean| / sigma of the bf16 rows is not {d['ratio']}: {float(rt.min()):.1f} .. {float(rt.max()):.1f}")
        if case.family == "const" and not bool((inp["x"].float().std(-1, unbiased=False) == 0).all()):
            bad.append("a row is not constant")
    if case.op == "ln_mean" and case.family == "exact" and not (isint(ref["want"]) and float(ref["want"].abs().max()) <= 256):
        bad.append("a mean is no bf16-exact integer")
    return bad


def _cmp(y, ref, margin, what="") -> tuple[bool, float, str]:
    want, bound = ref["want"], ref["bound"]
    if tuple(y.shape) != tuple(want.shape):
        return False, float("inf"), f"{what}shape {tuple(y.shape)} for {tuple(want.shape)}"
    r = ratio(y.float() if y.dtype == torch.bfloat16 else y, want, bound)
    if r == float("inf"):
        bad = int(((y.double() - want).abs() > bound).sum()) if torch.isfinite(y.float()).all() else -1
        return False, r, f"{what}{bad} of {y.numel()} outputs differ where the bound is 0 (or are not finite)"
    return r <= margin, r, f"{what}{r:.3f} x the bound (allowed {margin})"


def verify(case: Case, inp: dict, ref: dict, be, margin: float = MARGIN) -> tuple[bool, float, str]:
    """Every assertion the GPU suite makes on a case but the poison family's second launch: (ok, worst ratio, message)."""
    out = be.run(case, inp)
    y = out["y"]
    want_dt = DT[rows_out_dt(case)] if case.op in ROW_OPS else DT[case.get("ydt", "f32")] if case.op in ("ln_mean", "transpose") else torch.bfloat16
    if y.dtype != want_dt:
        return False, float("inf"), f"dtype {y.dtype}"
    if not out["guard_ok"]:
        return False, float("inf"), "wrote outside its output"
    ok, r, msg = _cmp(y, ref, margin)
    if not ok:
        return ok, r, msg
    if case.op == "token_mix":
        if case.get("rows"):
            rw, rb = tm_rows_reference(y, case.family == "exact")
            ok, r2, msg = _cmp(out["rows"], {"want": rw, "bound": rb}, margin, "row partials: ")
            r = max(r, r2)
            if not ok:
                return ok, r, msg
        elif out["rows"] is not None:
            return False, float("inf"), "row partials without row_out"
    if case.op in ("token_mix", "cls_attend") and case.family == "perm":
        N = case.d["N"]
        perm = [(i + 1) % N for i in range(N)]
        outs = [("permuted images", be.run(case, inp, perm=perm), perm)] + [(f"image {i} alone", be.run(case, inp, images=[i]), [i]) for i in range(N)]
        if case.op == "token_mix":
            outs.append(("in place", be.run(case, inp, inplace=True), None))
        for what, o, sel in outs:
            wy = y if sel is None else y[sel]
            if not (o["guard_ok"] and torch.equal(bits(o["y"]), bits(wy))):
                return False, float("inf"), f"{what}: the output differs from the batch's bits"
            if case.get("rows"):
                wr = out["rows"] if sel is None else out["rows"].view(N, case.d["T"], -1, 2)[sel].reshape(-1, out["rows"].shape[1], 2)
                if not torch.equal(bits(o["rows"]), bits(wr)):
                    return False, float("inf"), f"{what}: the row partials differ from the batch's bits"
    if case.op == "cls_head_gemm" and case.family == "poison" and case.d["M"] > 1:  # a row alone equals its row in the batch
        for m in sorted({0, case.d["M"] - 1}):
            one = dict(inp, x=inp["x"][m:m + 1])
            alone = be.run(Case(case.op, case.family, tuple((k, 1 if k == "M" else v) for k, v in case.dims)), one)["y"]
            if not torch.equal(bits(alone[0]), bits(y[m])):
                return False, float("inf"), f"row {m} alone differs from its row in the batch"
    return True, r, ""


# --------------------------------------------------------------------------------------------------------------- on the device
def embedded(t: torch.Tensor, dev, sentinel: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """t as the 16-byte aligned middle of a flat buffer of its dtype (bf16 / f32) filled with NaN or, sentinel, the guard pattern;
    a guard of >= 64 elements (a multiple of 64) in front and behind.  Returns (buffer, dense view)."""
    n = t.numel()
    guard = 64
    if sentinel:
        pat = SENT32 if t.dtype == torch.float32 else SENT16
        buf = torch.full((2 * guard + n,), pat, dtype=torch.int32 if t.dtype == torch.float32 else torch.int16).view(t.dtype)
    else:
        buf = torch.full((2 * guard + n,), float("nan"), dtype=t.dtype)
    buf = buf.to(dev)
    view = buf[guard:guard + n].view(t.shape)
    if not sentinel:
        view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def sentinels_intact(buf: torch.Tensor, view: torch.Tensor) -> bool:
    """Every element of the flat buffer outside the (dense) `view` still holds the guard pattern."""
    b = bits(buf.cpu().clone())
    pat = SENT32 if buf.dtype == torch.float32 else SENT16
    guard = (b.numel() - view.numel()) // 2
    b[guard:guard + view.numel()] = pat
    return bool((b == pat).all())


class Device:
    """The kernels behind StandIn's interface, through lib(): CPU tensors in, CPU tensors out, every output sentinel-guarded.
    poison: every operand cut out of a NaN-filled buffer."""

    def __init__(self, ops, dev="cuda"):
        self.ops, self.dev = ops, dev

    def run(self, case: Case, inp: dict, poison: bool = False, inplace: bool = False, images=None, perm=None) -> dict:
        L, st, d, dev = self.ops.lib(), self.ops._stream(), case.d, self.dev
        keep = []

        def P(t):
            if t is None:
                return None
            if not poison:
                v = t.contiguous().to(dev)
                keep.append(v)  # alive until the call returns: a temporary's memory would go to the next operand
                return v
            buf, v = embedded(t.contiguous(), dev)
            keep.append(buf)
            return v

        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        guards = []

        def out(shape, dt):
            buf, v = embedded(torch.empty(shape, dtype=dt), dev, sentinel=True)
            guards.append((buf, v))
            return v

        extra_ok, res = True, {}
        if case.op == "token_mix":
            N, T, Dt, C = d["N"], d["T"], d["Dt"], d["C"]
            x, stats = inp["x"], inp["stats"].view(N, T, 2)
            sel = images if images is not None else perm
            if sel is not None:
                x, stats, N = x[sel], stats[sel], len(sel)
            x, stats = P(x), P(stats.reshape(-1, 2))
            w1f, w2f = P(self.ops.mixer_pack_weight(inp["w1"]).cpu()), P(self.ops.mixer_pack_weight(inp["w2"]).cpu())
            y = out((N, T, C), torch.bfloat16)
            if inplace:
                y.copy_(x)
                x = y
            rows = out((N * T, C // 64, 2), torch.float32) if d["rows"] else None
            rc = L.pm_mixer_token_mix_bf16(ptr(x), ptr(stats), ptr(P(inp["gamma"])), ptr(P(inp["beta"])), ptr(w1f), ptr(P(inp["b1"])), ptr(w2f),
                                           ptr(P(inp["b2"])), ptr(y), ptr(rows), N, T, Dt, C, st)
            res["rows"] = None if rows is None else rows.cpu().clone()
        elif case.op == "ln_mean":
            y = out((d["N"], d["C"]), DT[d["ydt"]])
            rc = L.pm_ln_mean(ptr(P(inp["x"])), PM_DT[inp["x"].dtype], ptr(P(inp["stats"])), ptr(P(inp["gamma"])), ptr(P(inp["beta"])), ptr(y),
                              PM_DT[y.dtype], d["N"], d["T"], d["C"], st)
        elif case.op == "transpose":
            N, R, Cc, ldy = d["N"], d["R"], d["Cc"], d["R"] + d["pad"]
            full = out((N, Cc, ldy), torch.float32)
            resid = None
            if inp["resid"] is not None:
                resid = P(torch.nn.functional.pad(inp["resid"], (0, d["pad"]), value=float("nan")))
            rc = L.pm_transpose_add_f32(ptr(P(inp["x"])), ptr(resid), ptr(full), ldy, N, R, Cc, st)
            y = full[:, :, :R]
            extra_ok = bool((full[:, :, R:].cpu().contiguous().view(torch.int32) == SENT32).all())
        elif case.op == "cls_head_gemm":
            M, K, N, G = inp["x"].shape[0], d["K"], d["N"], d["G"]
            y = out((M, G, N), torch.bfloat16)
            bias = None if inp["bias"] is None else P(inp["bias"].reshape(-1))
            rc = L.pm_cls_head_gemm(ptr(P(inp["x"])), inp["ldx"], inp["xg"], ptr(P(inp["w"])), ptr(bias), ptr(y), G * N, N, M, N, K, G, st)
        elif case.op == "cls_attend":
            N, Lr, dd, H = d["N"], d["L"], d["d"], d["H"]
            x, u, stats = inp["x"], inp["u"], None if inp["stats"] is None else inp["stats"].view(N, Lr, 2)
            sel = images if images is not None else perm
            if sel is not None:
                x, u, stats, N = x[sel], u[sel], None if stats is None else stats[sel], len(sel)
            rs, bs = (dd + 8, Lr * (dd + 8) + 16) if poison else (dd, Lr * dd)  # poison: NaN between the rows and between the images
            xbuf = torch.full((128 + N * bs,), float("nan"), dtype=torch.bfloat16, device=dev)
            xv = xbuf[64:].as_strided((N, Lr, dd), (bs, rs, 1))
            xv.copy_(x)
            keep.append(xbuf)
            y = out((N, H, dd), torch.bfloat16)
            rc = L.pm_cls_attend(ptr(xv), rs, bs, ptr(P(None if stats is None else stats.reshape(-1, 2))), ptr(P(u)), ptr(y), N, Lr, dd, H,
                                 ATT_SCALE, EPS, st)
        elif case.op == "vit_tokens":
            geo = vit_geometry(case)
            y = out((d["N"], geo["L"] + (inp["cls"] is not None), d["d"]), torch.bfloat16)
            w = inp["w"]
            if poison and geo["generic"] and geo["ldw"] > geo["Kpad"]:  # K .. Kpad zero as the contract requires, NaN beyond
                w = w.clone()
                w[:, geo["Kpad"]:] = float("nan")
            args = (ptr(P(inp["bias"])), ptr(P(inp["pe"])), ptr(P(inp["cls"])), ptr(y), d["N"], d["H"], d["W"], d["P"], d["d"], st)
            if geo["generic"]:
                rc = L.pm_vit_tokens_generic(ptr(P(inp["imgs"])), ptr(P(w)), geo["ldw"], *args)
            else:
                rc = L.pm_vit_tokens(ptr(P(inp["imgs"])), ptr(P(w)), *args)
        elif case.op == "mean_ln":
            y = out((d["N"], d["C"]), DT[d["ydt"]])
            rc = L.pm_mean_ln(ptr(P(inp["x"])), d["C"] + d["ldpad"], PM_DT[inp["x"].dtype], ptr(P(inp["gamma"])), ptr(P(inp["beta"])), EPS,
                              ptr(y), PM_DT[y.dtype], d["N"], d["HW"], d["C"], st)
        elif case.op == "s2d":
            C, N, H, W = d["C"], d["N"], d["H"], d["W"]
            ldy = -(-4 * C // 64) * 64 if d["ldpad"] == 0 else 4 * C + d["ldpad"]
            y = out((N * (H // 2) * (W // 2), ldy), DT[d["ydt"]])
            rc = L.pm_ln_space_to_depth(ptr(P(inp["x"])), C + d["ldpad"], PM_DT[inp["x"].dtype], ptr(P(inp["gamma"])), ptr(P(inp["beta"])), EPS,
                                        ptr(y), ldy, PM_DT[y.dtype], N, H, W, C, st)
        elif case.op == "se_gate":
            y = out((d["N"], d["C"]), torch.float32)
            rc = L.pm_se_gate(ptr(P(inp["psum"])), d["ntiles"], d["hw"], ptr(P(inp["w1"])), ptr(P(inp["b1"])), ptr(P(inp["w2"])), ptr(P(inp["b2"])),
                              ptr(y), d["N"], d["C"], d["R"], st)
        elif case.op == "mean_rows":
            y = out((d["N"], d["C"]), torch.bfloat16)
            rc = L.pm_mean_rows_bf16(ptr(P(inp["x"])), ptr(y), d["N"], d["R"], d["C"], st)
        elif case.op == "rmsnorm":
            y = out((d["M"], d["d"]), DT[d["ydt"]])
            rc = L.pm_rmsnorm(ptr(P(inp["x"])), d["d"], PM_DT[inp["x"].dtype], ptr(P(inp["gamma"])), EPS, ptr(y), d["d"], PM_DT[y.dtype], d["M"],
                              d["d"], st)
        else:
            y = out((d["M"], d["F"]), torch.bfloat16)
            rc = L.pm_geglu(ptr(P(inp["h"])), 2 * d["F"] + d["ldpad"], ptr(y), d["F"], d["M"], d["F"], st)
        assert rc == 0, (case.id, rc)
        res["y"] = y.cpu().contiguous()
        res["guard_ok"] = extra_ok and all(sentinels_intact(b, v) for b, v in guards)
        return res


def run_abi(ops, case: Case, inp: dict, dev="cuda") -> dict:
    """The poison family's second launch: every operand the 16-byte aligned middle of a NaN-filled buffer."""
    return Device(ops, dev).run(case, inp, poison=True)


CASES = _cases()
