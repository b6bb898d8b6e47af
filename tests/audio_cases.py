"""References, error bounds, adversarial input families and case lists shared by the audio front-end parity tests
(tests/test_audio_cases_cpu.py without a GPU, tests/test_hip_audio_adversarial.py on one).  A plain helper module.

In scope (through pytorch_models._hip.ops, the poison family through the C ABI): w2v_stem0 (norm none / layer / instance),
whisper_stem1, grouped_conv (act none / gelu, bias, resid), group_windows, avgpool_time2, and - in the second half of the file, with
their own case type - stft_mel in its three modes (pm_stft_mel, pm_stft_mel_folded, pm_logmel_finalize).
Out of scope: rmsnorm / geglu / embed_tokens (the T5 and ragged suites), EnCodec's kernels (tests/encodec_cases.py), the strided-window GEMM layers of the
feature encoder (tests/linear_cases.py).

Contract ("2e. Audio front-end numerics contract").

Reference.  Float64 on the CPU from exactly the operands the kernel sees.  Beside `want` every op returns A (the sum of absolute
products per output, |bias| and |resid| included) and the element-wise bound.
  w2v_stem0      v = bias + sum_j w[c, j] x[b, t stride + j]; none: GELU(v); layer: LayerNorm over the C0 channels of a step (biased
                 variance, eps inside the root), gamma, beta, GELU; instance: the same over the T0 steps of a clip and channel.
  whisper_stem1  x rounded to bf16 FIRST (the kernel's A operand is bf16: that is the contract); k 3 / pad 1 conv over the packed
                 (d, 3 Cpad) weight + bias, erf-GELU; rows 0 and T + 1 of the (B, T + 2, d) output are +0 bit patterns.
  grouped_conv   act(conv + bias) + resid in the order read off the kernel, one rounding at the store; the contraction runs over
                 all Kp positions of the packed weight (tap, channel < cgp), rows past the slab are zeros.
  group_windows  a copy (f32 -> bf16: one rounding), pad rows and channels cg .. cgp are +0.
  avgpool_time2  one fp32 mean of two bf16 values, rounded to nearest even once more at the store.

Bounds.  u = 2^-24; no term is measured on a kernel.  From DESIGN.md 2c / 2d: delta = (K + 2) u A for fp32 accumulation of K terms
in any order (K = 10; 3 C; k cgp); the half-ulp bf16 store term; gelu_poly: 1.13 delta + 3.7e-5; a residual add + u |want|; the
two-pass LayerNorm term |gamma| / sigma (2 + |yhat|) e with e = max_c delta_c + C u mean_c |v_c|.  MARGIN = 1.5 on the GPU, 1.0 x for
the CPU stand-in; a zero bound means exact.  Added here:
  * the affine step of both norms, yhat g + beta evaluated as fma(v rstd, g, beta) or v (rstd g) + (beta - mean rstd g):
    4 u (|g| (|v| + |mean|) / sigma + |beta|) - rsqrtf 1 ulp, two products, the fma; for LayerNorm |v - mean| replaces |v| + |mean|
    (the kernel centres first);
  * w2v_stem0 instance statistics, for a method that NORMALISES THE COMPUTED fp32 CONV OUTPUT (first order in A / sigma), with the
    T0 terms summed no worse than per-chunk fp32 (nc = min(T0, 1024) terms) and an fp64 fold:
        e_t = 12 u A_t,  d_mean = mean_t e_t + nc u mean_t |v_t|,  d_c = e_t + d_mean + u |c_t|  (c = v - mean),
        d_var = mean_t (2 |c_t| d_c) + (nc + 2) u var,  d_rstd / rstd = d_var / (2 (var + eps)) + 3 u  (eps in the conditioning, as
        2d does for ln_stats_finalize),  d_y = |g| rstd d_c + |g| |c| rstd (d_rstd / rstd) + the affine term.
    There is NO (A / sigma)^2 term: the contract is the reference's behaviour, not the kernel's design.  A variance taken from
    fp32 autocorrelation sums, w^T (R / T - s s^T) w, errs by about u (A / sigma)^2 and is outside this bound once A / sigma > 1e3;
  * avgpool_time2: u |want| for the fp32 add (exact when the exponents are within 16 bits) + the store term.

Families.
  exact    grouped_conv with act none: integers in [-3, 3] (x sparse), bias / resid in [-8, 8], every partial sum below 2^24, >= 90 %
           of a case's outputs exact in bf16 (asserted on the CPU): the output must EQUAL want.to(bf16).  group_windows and
           avgpool_time2 on integers, including means that are bf16 ties (256 and 258 -> 257 -> 256).  A wrong tap, group, chunk
           swizzle, K-padding tap or tile edge is a bit difference.
  onehot   the ops that always apply GELU (both stems, grouped_conv with GELU): one-hot +-1 weights, integer x in [-3, 3],
           half-integer bias (none: x without zeros): the pre-activation is exact (delta = 0), the output is held by the GELU and store terms alone.
  cancel   grouped_conv / whisper_stem1: zero-sum filters on an offset + noise, |want| << A.  w2v_stem0 instance: first-, second-
           and third-difference filters on 2000 cos(2 pi t / 50000 + 0.3 b) + N(0, 1): var >> eps, A / sigma in 1e3 .. 1e4.
  offset   w2v_stem0 LayerNorm mode, |mean| / sigma = 4096 over C0 <= 96 channels (gamma ~ 0.5, beta ~ 1.5 keep |want| above the bound).
  poison   Gaussian operands; through lib(), the C ABI, every operand is the middle slice of a NaN-filled 16-byte-aligned buffer,
           the output the middle of a sentinel-filled one (grouped_conv: ldy > d, ldr > d): finite, bit-identical to the run on plain
           copies, inside the bound, every sentinel untouched; whisper_stem1's rows 0 and T + 1 and group_windows' pad rows and
           channels +0.
  batch    Gaussian operands, B > 1: clip b of the batch run is bit-identical to the single-clip run (log-mel: the per-clip peak too).
  STFT     exact: integer-valued tables in the kernels' layout (plain and folded) and integer samples, power and mel sums below 2^24;
           cancel: pure tones under a real window, the far bins by the bound; loudness (log-mel): amplitude 100 (peak > 0), amplitude
           1e-3 (every value < 0), a half-silent clip (reaches its floor), an all-zero clip (-inf, exactly).

Path -> case (paths() derives the tags from the shape with the launchers' own arithmetic; REQUIRED_PATHS is what must be reached):
  w2v_stem0      C0 8 / 64 / 504 / 512 (idle lanes at 8, 64, 504); T0 1 .. 5 (fewer steps than the four waves), 255 / 256 / 257
                 (conv chunk), 1023 / 1024 / 1025 (autocorrelation chunk); stride 1 / 5 / 11; a waveform tail no step reads;
                 bias or none; none / layer / instance; B 1 / 3
  whisper_stem1  C / Cpad 3 / 64, 64 / 64, 80 / 128, 128 / 128; T 1, 2, 127, 128, 129, 300; d 4, 64, 128, 132 (ragged last N tile),
                 384; B 1 / 3
  grouped_conv   (cg, cgp) (4, 8) (8, 8) (12, 16) (16, 16) (28, 32) (32, 32) (44, 48) (48, 48) (60, 64) (64, 64): all five (CPT, NJ),
                 duplicate weight rows where cg % 16 != 0; k 1, 2, 3, 19, 31, 128: nk = 1, 2, 3, > 4 (prologue and vmcnt ladder), K
                 padding 0 and > 0; stride 1 (swizzled rows where CPT >= 2) / 2 / 3 (padded rows); To 1, 15, 16, 17, 64, 65, 128 (last
                 MI = 1), 129 (first MI = 4), 257; G B tiles % 8 != 0 (xcd_remap); bias or none; none / gelu; resid, ldr > d
                 refusals: cg 20, cg 6, a span above 160 KiB (k 500, stride 3, To 257)
  stft_mel       (n_fft, hop) (400, 160) production, (16, 4) nblk = 1, (128, 64) a block holding a single bin, (8, 2) the smallest hop,
                 (16, 32) hop > n_fft, (402, 6) n_fft / 2 odd, (512, 128) in modes 1 and 2 (52 KiB of LDS), (1024, 256) mode 0 served and
                 mode 1 refused, (2048, 512) refused; symmetric window -> folded tables, asymmetric -> plain, both on integer tables;
                 T = n_fft / 2 + 1, T % hop != 0; n_frames 1, 31, 32, 33, 65 and T // hop; n_mels 1, 5, 80, 128, an empty mel row; 1, 3, 4
                 clips and leading dims; mode 2 with n_mels n_frames % 4 != 0 refused (STFT_CASES, stft_paths(), STFT_REQUIRED)
  group_windows  scalar path cg 4 / 12 / 44, vector path cg 8 / 48; f32 and bf16; ldx > d; pad 0; T 1; cgp - cg = 16 on the vector path
                 (whole pad chunks: the kernel copied the next group's channels into them until this suite)
  avgpool_time2  T 2, 3, 301; d 8, 72
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import torch

from conv_cases import BF16_BITS, GELU_LIP, MARGIN, U32, bf16r, ratio, store, store_term  # noqa: F401  (one definition of each)

GELU_POLY_ABS = 3.7e-5  # csrc/common.h: |gelu_poly(x) - x Phi(x)| for all finite x
EPS = 1e-5
OFFSET_RATIO = 4096.0
SENTINEL = 0x4B4B       # bf16 bit pattern of every output guard
TAIL = 1.0e30           # the value of waveform samples no step reads
TCH, ACH = 256, 1024    # csrc/wav2vec2.hip: steps per workgroup of the conv / autocorrelation pass
OPS = ("w2v_stem0", "whisper_stem1", "grouped_conv", "group_windows", "avgpool_time2")
GELU_OPS = ("w2v_stem0", "whisper_stem1")
MUTANTS = ("tap_edge", "padrow", "trunc", "x_unrounded", "var_unbiased", "var_second_order", "chunk_edge", "group_swap", "kpad_tap",
           "row_dup", "tile_edge", "act_after_resid", "onepass", "padchan")
# the family each mutant is aimed at: it must be rejected by at least one case of it (tests/test_audio_cases_cpu.py)
MUTANT_FAMILY = {"tap_edge": "onehot", "padrow": "poison", "trunc": "poison", "x_unrounded": "poison", "var_unbiased": "poison",
                 "var_second_order": "cancel", "chunk_edge": "onehot", "group_swap": "exact", "kpad_tap": "exact", "row_dup": "poison",
                 "tile_edge": "exact", "act_after_resid": "onehot", "onepass": "offset", "padchan": "exact"}


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    """One problem.  T: output steps (w2v_stem0 T0, grouped_conv To) or input steps (the others).  C: input channels (whisper_stem1
    n_mels, w2v_stem0 C0).  d: output width (whisper_stem1) or row width (group_windows, avgpool_time2)."""
    op: str
    family: str
    B: int
    T: int
    C: int = 0
    d: int = 0
    k: int = 0
    stride: int = 1
    G: int = 1
    cg: int = 0
    cgp: int = 0
    bias: bool = True
    norm: str = "none"
    act: str = "none"
    resid: bool = False
    ld_extra: int = 0   # grouped_conv: ldr - d through ops;  group_windows: ldx - d
    tail: int = 0       # w2v_stem0: samples behind the last window
    xdt: str = "bf16"   # group_windows input
    pads: tuple = (0, 0)

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.family}-b{self.B}-t{self.T}"
        if self.op == "w2v_stem0":
            s += f"-c{self.C}-s{self.stride}-{self.norm}" + ("-b" if self.bias else "") + (f"-tail{self.tail}" if self.tail else "")
        elif self.op == "whisper_stem1":
            s += f"-c{self.C}-d{self.d}"
        elif self.op == "grouped_conv":
            s += f"-g{self.G}x{self.cg}p{self.cgp}-k{self.k}s{self.stride}" + ("-b" if self.bias else "") + ("-r" if self.resid else "")
            s += (f"-ld{self.ld_extra}" if self.ld_extra else "") + (f"-{self.act}" if self.act != "none" else "")
        elif self.op == "group_windows":
            s += f"-g{self.G}x{self.cg}p{self.cgp}-{self.xdt}-pad{self.pads[0]}+{self.pads[1]}" + (f"-ld{self.ld_extra}" if self.ld_extra else "")
        else:
            s += f"-d{self.d}"
        return s

    @property
    def data(self) -> str:
        return self.family if self.family in ("exact", "onehot", "cancel", "offset") else "gauss"


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def cpad(case: Case) -> int:
    return -(-case.C // 64) * 64


def kp(case: Case) -> int:
    return -(-case.k * case.cgp // 64) * 64


def wave_len(case: Case) -> int:
    assert case.tail < case.stride, "a longer tail is another step"
    return (case.T - 1) * case.stride + 10 + case.tail


def tp(case: Case) -> int:
    """grouped_conv: slab rows for To = case.T output steps (one spare row at stride > 1: (Tp - k) % stride != 0)."""
    return (case.T - 1) * case.stride + case.k + (1 if case.stride > 1 else 0)


def gc_launch(case: Case) -> dict:
    """pm_grouped_conv_bf16's own arithmetic (csrc/grouped_conv.hip)."""
    To, s = case.T, case.stride
    mi = 4 if To > 128 else 1
    bm = 64 * mi
    cpt, nj = case.cgp // 8, -(-case.cg // 16)
    taps_p = -(-(kp(case) // 8) // cpt)
    span = (bm - 1) * s + taps_p
    swz = s == 1 and cpt >= 2
    lds = 4 * nj * 16 * 128 + span * (128 if swz else cpt * 16 + 16)
    return dict(mi=mi, cpt=cpt, nj=nj, swz=swz, lds=lds, tiles=-(-To // bm), nk=kp(case) // 64)


def abi_refusal(case: Case) -> str | None:
    """The limits the C entry points answer PM_EUNSUPPORTED / PM_EINVAL / PM_EALIGN to."""
    if case.op == "w2v_stem0" and (case.C % 8 or case.C > 512 or case.T < 1):
        return "w2v_stem0: C0 % 8 == 0, C0 <= 512"
    if case.op == "whisper_stem1" and (case.d % 4 or case.T < 1):
        return "whisper_stem1: d % 4 == 0"
    if case.op == "grouped_conv":
        if case.cg <= 0 or case.cg % 4 or case.cgp not in (8, 16, 32, 48, 64) or not 0 <= case.cgp - case.cg < 8:
            return "grouped_conv: cg % 4 == 0, cgp in (8, 16, 32, 48, 64), cgp - cg < 8"
        if gc_launch(case)["lds"] > 160 * 1024:
            return "grouped_conv: the span exceeds 160 KiB of LDS"
        if (case.G * case.cg + case.ld_extra) % 4:
            return "grouped_conv: ldr % 4 == 0"
    if case.op == "group_windows" and (case.cgp % 8 or case.cgp < case.cg or (case.cg % 8 == 0 and (case.G * case.cg + case.ld_extra) % 8)):
        return "group_windows: cgp % 8 == 0, 16-byte rows on the vector path"
    if case.op == "avgpool_time2" and (case.d % 8 or case.T < 2):
        return "avgpool_time2: d % 8 == 0, T >= 2"
    return None


def paths(case: Case) -> set[str]:
    """The kernel paths a case reaches, derived from its shape with the launchers' own arithmetic."""
    t = set()
    if case.op == "w2v_stem0":
        t |= {f"norm-{case.norm}", f"stride{case.stride}", "bias" if case.bias else "nobias", f"C{case.C}"}
        if case.C < 512:
            t.add("idle-lanes")
        if case.T < 4:
            t.add("steps<waves")
        for edge, name in ((TCH, "conv-chunk"), (ACH, "acorr-chunk")):
            for dlt in (-1, 0, 1):
                if case.T == edge + dlt and (edge == TCH or case.norm == "instance"):
                    t.add(f"{name}{dlt:+d}")
        if case.tail:
            t.add("tail")
    elif case.op == "whisper_stem1":
        t |= {f"C{case.C}/{cpad(case)}", f"nkt{3 * cpad(case) // 64}"}
        if case.d % 128:
            t.add("ragged-n-tile" if case.d > 128 else "clamped-w-rows")
        if case.d > 128:
            t.add("n-tiles>1")
        if case.T % 128:
            t.add("ragged-t-tile")
        if case.T > 128:
            t.add("t-tiles>1")
        if case.T == 1:
            t.add("both-pad-rows-one-step")
    elif case.op == "grouped_conv":
        L = gc_launch(case)
        t |= {f"inst{L['cpt']}-{L['nj']}", f"MI{L['mi']}", "swz" if L["swz"] else "padrows", f"act-{case.act}", f"stride{case.stride}"}
        t.add(f"nk{L['nk']}" if L["nk"] <= 4 else "nk>4")
        t.add("kpad>0" if kp(case) > case.k * case.cgp else "kpad0")
        if case.cg % 16:
            t.add("dup-w-rows")
        if (case.G * case.B * L["tiles"]) % 8:
            t.add("xcd-ragged")
        if L["tiles"] > 1:
            t.add("t-tiles>1")
        if case.T % (64 * L["mi"]):
            t.add("ragged-t-tile")
        t.add("bias" if case.bias else "nobias")
        if case.resid:
            t.add("resid")
        if case.ld_extra:
            t.add("ldr>d")
    elif case.op == "group_windows":
        t |= {"vec" if case.cg % 8 == 0 else "scalar", case.xdt}
        if case.ld_extra:
            t.add("ldx>d")
        if case.pads == (0, 0):
            t.add("pad0")
        if case.T == 1:
            t.add("T1")
        if case.cgp > case.cg:
            t.add("pad-channels")
        if case.cg % 8 == 0 and case.cgp - case.cg >= 8:
            t.add("vec-pad-chunks")
    elif case.op == "avgpool_time2":
        t.add("odd-T" if case.T % 2 else "even-T")
    return t


REQUIRED_PATHS = {
    "w2v_stem0": {"norm-none", "norm-layer", "norm-instance", "stride1", "stride5", "stride11", "bias", "nobias", "C8", "C64", "C504", "C512",
                  "idle-lanes", "steps<waves", "tail"} | {f"conv-chunk{d:+d}" for d in (-1, 0, 1)} | {f"acorr-chunk{d:+d}" for d in (-1, 0, 1)},
    "whisper_stem1": {"C3/64", "C64/64", "C80/128", "C128/128", "nkt3", "nkt6", "ragged-n-tile", "clamped-w-rows", "n-tiles>1", "ragged-t-tile",
                      "t-tiles>1", "both-pad-rows-one-step"},
    "grouped_conv": {"inst1-1", "inst2-1", "inst4-2", "inst6-3", "inst8-4", "MI1", "MI4", "swz", "padrows", "act-none", "act-gelu", "stride1",
                     "stride2", "stride3", "nk1", "nk2", "nk3", "nk>4", "kpad0", "kpad>0", "dup-w-rows", "xcd-ragged", "t-tiles>1",
                     "ragged-t-tile", "bias", "nobias", "resid", "ldr>d"},
    "group_windows": {"vec", "scalar", "f32", "bf16", "ldx>d", "pad0", "T1", "pad-channels", "vec-pad-chunks"},
    "avgpool_time2": {"odd-T", "even-T"},
}


def _cases() -> list[Case]:
    L: list[Case] = []

    def add(fams, op, B, T, **kw):
        for f in fams:
            if f == "batch" and B == 1:
                continue
            L.append(Case(op, f, B, T, **kw))

    # ---- w2v_stem0: C0, T0, stride, norm, bias, B, tail
    for (C0, T0, s, norm, b, B, tail) in (
        (8, 1, 5, "none", True, 1, 0), (8, 2, 5, "layer", False, 3, 3), (64, 3, 1, "instance", True, 3, 0), (8, 4, 11, "instance", False, 1, 7),
        (504, 5, 5, "layer", True, 3, 0), (512, 255, 5, "none", False, 1, 0), (64, 256, 11, "layer", True, 1, 0), (8, 257, 1, "none", True, 3, 0),
        (8, 255, 1, "instance", True, 1, 0), (64, 257, 5, "instance", True, 3, 4), (8, 1023, 1, "instance", False, 1, 0),
        (64, 1024, 5, "instance", True, 1, 0), (512, 1025, 5, "instance", True, 3, 0), (504, 256, 1, "instance", True, 1, 0),
    ):
        add(("onehot", "poison", "batch"), "w2v_stem0", B, T0, C=C0, stride=s, norm=norm, bias=b, tail=tail)
    for (C0, T0, s, B) in ((8, 1025, 5, 3), (64, 257, 1, 1), (512, 1023, 11, 3)):
        add(("cancel",), "w2v_stem0", B, T0, C=C0, stride=s, norm="instance", bias=True)
    for (C0, T0, s) in ((8, 5, 5), (64, 257, 1), (96, 3, 11)):
        add(("offset",), "w2v_stem0", 3, T0, C=C0, stride=s, norm="layer", bias=True)
    # ---- whisper_stem1: C, T, d, B
    for (C, T, d, B) in ((3, 1, 4, 1), (3, 2, 132, 3), (64, 127, 64, 1), (64, 128, 128, 3), (80, 129, 132, 1), (80, 300, 384, 3),
                         (128, 2, 64, 3), (128, 300, 4, 1), (80, 1, 384, 3)):
        add(("onehot", "cancel", "poison", "batch"), "whisper_stem1", B, T, C=C, d=d)
    # ---- grouped_conv: cg, cgp, k, stride, To, G, B, bias, resid, ld_extra
    for (cg, cgp, k, s, To, G, B, b, r, ld) in (
        (4, 8, 1, 1, 1, 3, 1, True, False, 0),        # nk = 1, one step, CPT 1 (padded rows)
        (8, 8, 19, 2, 15, 2, 3, False, True, 4),      # nk = 3, K padding 40
        (12, 16, 2, 1, 16, 3, 1, True, True, 0),      # nk = 1 with padding 32, swizzled rows
        (16, 16, 31, 3, 17, 2, 3, True, False, 0),    # nk = 8
        (28, 32, 3, 2, 64, 3, 1, False, False, 0),    # nk = 2, padding 32
        (32, 32, 128, 1, 65, 1, 3, True, True, 8),    # nk = 64: wav2vec2's kernel length
        (44, 48, 2, 1, 128, 3, 1, True, True, 0),     # nk = 2 (96 -> 128), last MI = 1
        (48, 48, 19, 1, 129, 2, 1, True, True, 4),    # first MI = 4, data2vec's k
        (60, 64, 3, 3, 257, 1, 3, True, False, 0),    # nk = 3, two MI = 4 tiles
        (64, 64, 1, 1, 129, 3, 1, False, True, 0),    # nk = 1 at MI = 4
        (64, 64, 2, 2, 17, 3, 3, True, True, 0),      # nk = 2, padding 0
        (48, 48, 31, 2, 257, 1, 1, True, True, 0),    # SEW: stride 2 at MI = 4
    ):
        kw = dict(k=k, stride=s, G=G, cg=cg, cgp=cgp, bias=b, resid=r, ld_extra=ld)
        add(("exact", "cancel", "poison", "batch"), "grouped_conv", B, To, act="none", **kw)
        add(("onehot", "poison"), "grouped_conv", B, To, act="gelu", **kw)
    # ---- group_windows: cg, cgp, G, T, B, xdt, pads, ld_extra
    for (cg, cgp, G, T, B, xdt, pads, ld) in ((4, 8, 3, 1, 3, "f32", (2, 1), 0), (12, 16, 2, 5, 1, "bf16", (0, 0), 4), (44, 48, 3, 7, 3, "f32", (64, 63), 4),
                                             (8, 8, 2, 3, 3, "bf16", (1, 0), 8), (48, 48, 16, 33, 3, "f32", (64, 63), 0), (48, 64, 2, 4, 1, "bf16", (0, 3), 0)):
        add(("exact", "poison", "batch"), "group_windows", B, T, G=G, cg=cg, cgp=cgp, d=G * cg, xdt=xdt, pads=pads, ld_extra=ld)
    # ---- avgpool_time2
    for (T, d, B) in ((2, 8, 1), (3, 8, 3), (301, 72, 3)):
        add(("exact", "poison", "batch"), "avgpool_time2", B, T, d=d)
    return L


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
REFUSED = (Case("grouped_conv", "exact", 1, 16, k=3, G=2, cg=20, cgp=24), Case("grouped_conv", "exact", 1, 16, k=3, G=2, cg=6, cgp=8),
           Case("grouped_conv", "exact", 1, 257, k=500, stride=3, G=1, cg=64, cgp=64))


# --------------------------------------------------------------------------------------------------------------- inputs
def build(case: Case) -> dict:
    """CPU fp32 tensors holding exactly the values the kernel sees (bf16 operands are bf16-rounded values in fp32 storage)."""
    g = torch.Generator().manual_seed(_seed(case))
    randn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    sign = lambda *s: ints(0, 1, *s) * 2 - 1  # noqa: E731
    half = lambda *s: ints(-2, 1, *s) + 0.5  # noqa: E731  (-1.5, -0.5, 0.5, 1.5)
    B, T = case.B, case.T
    out: dict = {}
    if case.op == "w2v_stem0":
        C0, L = case.C, wave_len(case)
        n = L - case.tail
        if case.data == "onehot":
            x = ints(-3, 3, B, n)
            x = x if case.bias else torch.where(x == 0, torch.full_like(x, 2.0), x)  # no bias: keep the pre-activation off 0
            w = torch.zeros(C0, 10)
            w[torch.arange(C0), torch.randint(0, 10, (C0,), generator=g)] = sign(C0)
            out.update(w=w, bias=half(C0) if case.bias else None)
        elif case.data == "cancel":
            t = torch.arange(n, dtype=torch.float64)
            x = torch.stack([2000.0 * torch.cos(2 * torch.pi * t / 50000.0 + 0.3 * b) for b in range(B)]).float() + randn(B, n)
            w = torch.zeros(C0, 10)
            for c in range(C0):  # (1, -1), (1, -2, 1), (1, -3, 3, -1) at a tap offset that moves with the channel
                coef = ((1.0, -1.0), (1.0, -2.0, 1.0), (1.0, -3.0, 3.0, -1.0))[c % 3]
                o = (c // 3) % (11 - len(coef))
                w[c, o:o + len(coef)] = torch.tensor(coef)
            w = w * (0.5 + torch.rand(C0, 1, generator=g))
            out.update(w=w.float(), bias=0.1 * randn(C0))
        else:
            x = randn(B, n)
            w = randn(C0, 10) * 10 ** -0.5 * (0.05 if case.data == "offset" else 1.0)
            b = 0.5 * randn(C0)
            if case.data == "offset":
                b = (b - b.mean()) / b.std(unbiased=False) + OFFSET_RATIO
            out.update(w=w, bias=b.float() if case.bias else None)
        out["x"] = torch.cat([x, torch.full((B, case.tail), TAIL)], 1).contiguous()
        if case.norm != "none":
            off = case.data == "offset"
            out["gamma"] = (0.5 + 0.05 * randn(C0)) if off else 1.0 + 0.3 * randn(C0)
            out["beta"] = (1.5 + 0.1 * randn(C0)) if off else 0.5 * randn(C0)
        return out
    if case.op == "whisper_stem1":
        C, Cp, d = case.C, cpad(case), case.d
        w = torch.zeros(d, 3, Cp)
        if case.data == "onehot":
            out["x"] = ints(-3, 3, B, C, T)
            w[torch.arange(d), torch.arange(d) % 3, torch.randint(0, C, (d,), generator=g)] = sign(d)
            out["bias"] = half(d)
        elif case.data == "cancel":
            out["x"] = 4.0 + randn(B, C, T) / 16  # rounded to bf16 by the contract, not here
            wr = randn(d, 3, C)
            w[:, :, :C] = bf16r((wr - wr.mean((1, 2), keepdim=True)) * (3 * C) ** -0.5 * 2)
            out["bias"] = 0.1 * randn(d)
        else:
            out["x"] = randn(B, C, T)
            w[:, :, :C] = bf16r(randn(d, 3, C) * (3 * C) ** -0.5)
            out["bias"] = 0.5 * randn(d)
        out["w"] = w.reshape(d, 3 * Cp)
        return out
    if case.op == "grouped_conv":
        G, cg, cgp, k, Tp, Kp, d = case.G, case.cg, case.cgp, case.k, tp(case), kp(case), case.G * case.cg
        K = k * cg
        x = torch.zeros(B, G, Tp, cgp)
        w = torch.zeros(G, cg, Kp)
        wv = w[:, :, :k * cgp].view(G, cg, k, cgp)
        if case.data == "exact":
            x[..., :cg] = ints(-3, 3, B, G, Tp, cg) * (torch.rand(B, G, Tp, cg, generator=g) < min(0.5, 600.0 / K))
            wv[..., :cg] = ints(-3, 3, G, cg, k, cg)
            bias, resid = ints(-8, 8, d), ints(-8, 8, B * T, d)
        elif case.data == "onehot":
            xi = ints(-3, 3, B, G, Tp, cg)
            x[..., :cg] = xi if case.bias else torch.where(xi == 0, torch.full_like(xi, 2.0), xi)  # no bias: keep the pre-activation off 0
            gi, ni = torch.meshgrid(torch.arange(G), torch.arange(cg), indexing="ij")
            wv[gi, ni, torch.randint(0, k, (G, cg), generator=g), torch.randint(0, cg, (G, cg), generator=g)] = sign(G, cg)
            bias, resid = half(d), ints(-8, 8, B * T, d)
        elif case.data == "cancel":
            x[..., :cg] = bf16r(4.0 + randn(B, G, Tp, cg) / 16)
            wr = randn(G, cg, k, cg)
            wv[..., :cg] = bf16r((wr - wr.mean((2, 3), keepdim=True)) * K ** -0.5 * 2)
            bias, resid = 0.1 * randn(d), bf16r(0.1 * randn(B * T, d))
        else:
            x[..., :cg] = bf16r(randn(B, G, Tp, cg))
            wv[..., :cg] = bf16r(randn(G, cg, k, cg) * K ** -0.5)
            bias, resid = 0.5 * randn(d), bf16r(randn(B * T, d))
        out.update(x=x, w=w, bias=bias if case.bias else None, resid=resid if case.resid else None)
        return out
    if case.op == "group_windows":
        if case.data == "exact":
            out["x"] = ints(-128, 128, B, T, case.d)
        else:
            out["x"] = randn(B, T, case.d) if case.xdt == "f32" else bf16r(randn(B, T, case.d))
        return out
    if case.op == "avgpool_time2":
        if case.data == "exact":  # even integers around 256: pairs (256, 258), (258, 260) ... have means that are bf16 ties
            x = 2 * ints(-3, 3, B, T, case.d) + 256 * sign(B, T, case.d)
            x[:, 0::2][..., 0] = 256.0
            x[:, 1::2][..., 0] = 258.0
            out["x"] = x
        else:
            out["x"] = bf16r(randn(B, T, case.d))
        return out
    raise ValueError(case.op)


# --------------------------------------------------------------------------------------------------------------- the reference
def gelu_erf(z: torch.Tensor) -> torch.Tensor:
    return 0.5 * z * torch.erfc(-z * 0.7071067811865476)


def _gelu(z: torch.Tensor, dtype) -> torch.Tensor:
    if dtype == torch.float64:
        return gelu_erf(z)
    from linear_cases import gelu_poly32  # the stand-in evaluates the kernels' own polynomial in fp32

    return gelu_poly32(z)


def _taps_sum(terms, dtype, reverse):
    """sum of `terms` (a list of (a, b) factor pairs, already broadcast) in `dtype`, in list order or reversed.  Returns (z, A)."""
    z = A = None
    for a, b in (reversed(terms) if reverse else terms):
        p = a.to(dtype) * b.to(dtype)
        z = p if z is None else z + p
        A = p.double().abs() if A is None else A + p.double().abs()
    return z, A


def autocorr32(x: torch.Tensor, T0: int, stride: int) -> torch.Tensor:
    """The 10 + 55 per-clip sums (S, R) of csrc/wav2vec2.hip's FIRST design, in its own arithmetic: fp32 thread-private fma chains
    over steps t, t + 256, .., a 6-level tree over the 64 lanes, ((w0 + w1) + w2) + w3, the chunks folded in fp64.  (B, 65) f64."""
    cols = x.unfold(1, 10, stride)[:, :T0].double()  # (B, T0, 10)
    iu = torch.triu_indices(10, 10)
    terms = torch.cat([cols, cols[..., iu[0]] * cols[..., iu[1]]], -1)  # products of two fp32 values: exact in fp64
    B = x.shape[0]
    nch = -(-T0 // ACH)
    terms = torch.cat([terms, terms.new_zeros(B, nch * ACH - T0, 65)], 1).view(B, nch, 4, 256, 65)
    acc = torch.zeros(B, nch, 256, 65, dtype=torch.float32)
    for i in range(4):
        acc = (acc.double() + terms[:, :, i]).float()  # fmaf: one rounding per step
    acc = acc.view(B, nch, 4, 64, 65)
    for _ in range(6):
        acc = acc[:, :, :, 0::2] + acc[:, :, :, 1::2]
    acc = acc[:, :, :, 0]
    part = ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]
    return part.double().sum(1)


def _stats_second_order(x, w, bias, T0, stride):
    """(mean, var) per (clip, channel) the way the finalize kernel forms them from the fp32 sums: var = w^T (R / T - s s^T) w in fp64."""
    tot = autocorr32(x, T0, stride) / T0
    s, R = tot[:, :10], torch.zeros(x.shape[0], 10, 10, dtype=torch.float64)
    iu = torch.triu_indices(10, 10)
    R[:, iu[0], iu[1]] = tot[:, 10:]
    R = R + R.triu(1).transpose(1, 2)
    cov = R - s[:, :, None] * s[:, None, :]
    wd = w.double()
    mean = s @ wd.t() + (bias.double() if bias is not None else 0.0)
    var = torch.einsum("cj,bjk,ck->bc", wd, cov, wd).clamp_min(0.0)
    return mean[:, None, :], var[:, None, :]


def _chunked_mean(v: torch.Tensor, dtype) -> torch.Tensor:
    """mean over dim 1; in fp32: per-1024-step chunk sums in fp32, folded in fp64 (what the bound allows a correct method)."""
    if dtype == torch.float64:
        return v.mean(1, keepdim=True)
    tot = sum(ch.sum(1, keepdim=True).double() for ch in v.split(ACH, 1))
    return (tot / v.shape[1]).to(dtype)


def _w2v(case, inp, dtype, reverse, mutant):
    u, K = U32, 10
    x, w, T0 = inp["x"], inp["w"], case.T
    cols = x.unfold(1, 10, case.stride)[:, :T0]  # (B, T0, 10): the tail never enters
    v, A = _taps_sum([(cols[:, :, j, None], w[None, None, :, j]) for j in range(10)], dtype, reverse)
    if inp["bias"] is not None:
        v, A = v + inp["bias"].to(dtype), A + inp["bias"].double().abs()
    if mutant == "chunk_edge" and T0 > TCH:  # the first step of every later 256-step chunk takes the previous step's window
        v = v.clone()
        v[:, TCH::TCH] = v[:, TCH - 1:-1:TCH]
    e = torch.zeros_like(A) if case.family == "onehot" else (K + 2) * u * A
    r = {"v": v, "A": A}
    vd = v.double()
    if case.norm == "none":
        y, dy = v, e
    else:
        g, bt = inp["gamma"].to(dtype), inp["beta"].to(dtype)
        gd, bd = inp["gamma"].double().abs(), inp["beta"].double().abs()
        if case.norm == "layer":
            C = case.C
            if mutant == "onepass":
                v32 = v.float()
                mean = v32.mean(-1, keepdim=True)
                var = ((v32 * v32).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
                mean, var = mean.to(dtype), var.to(dtype)
            else:
                mean = v.mean(-1, keepdim=True)
                var = (v - mean).square().mean(-1, keepdim=True)
            sigma = torch.sqrt(var + EPS)
            yhat = (v - mean) / sigma
            y = yhat * g + bt
            ee = e.max(-1, keepdim=True).values + C * u * vd.abs().mean(-1, keepdim=True)
            dy = gd / sigma.double() * (2 + yhat.double().abs()) * ee + 4 * u * (gd * yhat.double().abs() + bd)
        else:  # instance: over the T0 steps of a clip and channel
            if mutant == "var_second_order":
                mean, var = _stats_second_order(x, w, inp["bias"], T0, case.stride)
                mean, var = mean.to(dtype), var.to(dtype)
            else:
                mean = _chunked_mean(v, dtype)
                var = _chunked_mean((v - mean).square(), dtype)
                if mutant == "var_unbiased" and T0 > 1:
                    var = var * (T0 / (T0 - 1))
            rstd = 1.0 / torch.sqrt(var + EPS)
            c = v - mean
            y = c * rstd * g + bt
            nc = min(T0, ACH)
            cd, rd, var_d = c.double().abs(), rstd.double(), var.double()
            em = e.mean(1, keepdim=True) + nc * u * vd.abs().mean(1, keepdim=True)
            dc = e + em + u * cd
            dvar = (2 * cd * dc).mean(1, keepdim=True) + (nc + 2) * u * var_d
            rel = dvar / (2 * (var_d + EPS)) + 3 * u
            dy = gd * rd * dc + gd * cd * rd * rel + 4 * u * (gd * rd * (vd.abs() + mean.double().abs()) + bd)
            r.update(var=var, sigma=torch.sqrt(var_d + EPS))
        r["mean"] = mean
    want = _gelu(y, dtype)
    r.update(want=want, bound=GELU_LIP * dy + GELU_POLY_ABS + store_term(want, "bf16"))
    return r


def _stem1(case, inp, dtype, reverse, mutant):
    u = U32
    B, C, T, d, Cp = case.B, case.C, case.T, case.d, cpad(case)
    x = inp["x"] if mutant == "x_unrounded" else bf16r(inp["x"])
    w = inp["w"].view(d, 3, Cp)
    xp = torch.zeros(B, C, T + 2)
    xp[:, :, 1:T + 1] = x
    if mutant == "tap_edge":  # no zero at t = -1 / t = T: the neighbouring values of the channel-major buffer
        flat = torch.cat([torch.ones(1), x.reshape(-1), torch.ones(1)])
        idx = (torch.arange(B)[:, None] * C + torch.arange(C)[None, :]) * T + 1
        xp[:, :, 0], xp[:, :, T + 1] = flat[idx - 1], flat[idx + T]
    terms = [(xp[:, c, tap:tap + T, None], w[None, None, :, tap, c]) for tap in range(3) for c in range(C)]
    v, A = _taps_sum(terms, dtype, reverse)
    v, A = v + inp["bias"].to(dtype), A + inp["bias"].double().abs()
    e = torch.zeros_like(A) if case.family == "onehot" else (3 * C + 2) * u * A
    g = _gelu(v, dtype)
    zrow = torch.zeros(B, 1, d, dtype=g.dtype)
    zb = torch.zeros(B, 1, d, dtype=torch.float64)
    last = torch.full_like(zrow, float(torch.tensor([SENTINEL], dtype=torch.int16).view(torch.bfloat16))) if mutant == "padrow" else zrow
    return {"v": v, "want": torch.cat([zrow, g, last], 1), "A": torch.cat([zb, A, zb], 1),
            "bound": torch.cat([zb, GELU_LIP * e + GELU_POLY_ABS + store_term(g, "bf16"), zb], 1)}


def _gconv(case, inp, dtype, reverse, mutant):
    u = U32
    B, G, cg, cgp, k, s, To, Kp = case.B, case.G, case.cg, case.cgp, case.k, case.stride, case.T, kp(case)
    x, w = inp["x"], inp["w"]
    if mutant == "group_swap":
        x = x.flip(1)
    taps = -(-Kp // cgp)
    xz = torch.cat([x, x.new_zeros(B, G, (To - 1) * s + taps - x.shape[2] + 1, cgp)], 2)  # rows past the slab: zeros
    wz = torch.cat([w, w.new_zeros(G, cg, taps * cgp - Kp)], 2).view(G, cg, taps, cgp)
    if mutant == "kpad_tap" and Kp > k * cgp:
        wz = wz.clone()
        wz[:, :, k, 0] = 1.0
    z = torch.zeros(B, To, G, cg, dtype=dtype)
    A = torch.zeros(B, To, G, cg, dtype=torch.float64)
    for tap in (reversed(range(taps)) if reverse else range(taps)):
        xs = xz[:, :, tap:tap + (To - 1) * s + 1:s, :]  # (B, G, To, cgp)
        wt = wz[:, :, tap, :]
        if not wt.any():
            continue
        z += torch.einsum("bgtc,gnc->btgn", xs.to(dtype), wt.to(dtype))
        A += torch.einsum("bgtc,gnc->btgn", xs.double().abs(), wt.double().abs())
    z, A = z.reshape(B * To, G * cg), A.reshape(B * To, G * cg)
    live = A > 0
    if inp["bias"] is not None:
        z, A = z + inp["bias"].to(dtype), A + inp["bias"].double().abs()
    if mutant == "tile_edge" and To > 1:  # step 16 i of every subtile takes the accumulator of the step behind it
        zt = z.view(B, To, -1).clone()
        idx = torch.arange(0, To, 16)
        zt[:, idx] = zt[:, (idx + 1).clamp_max(To - 1)]
        z = zt.view(B * To, -1)
    e = torch.where(live, (k * cgp + 2) * u * A, torch.zeros_like(A))
    if case.family == "onehot":
        e = torch.zeros_like(A)
    res = inp["resid"]
    if mutant == "act_after_resid" and res is not None:
        z, res = z + res.to(dtype), None
    if case.act == "gelu":
        z = _gelu(z, dtype)
        e = GELU_LIP * e + GELU_POLY_ABS
    want = z
    if res is not None:
        want = z + res.to(dtype)
        e = e + u * want.double().abs()
    if inp["resid"] is not None:
        A = A + inp["resid"].double().abs()
    return {"want": want, "A": A, "bound": e + store_term(want, "bf16"), "guard_bad": mutant == "row_dup"}


def _windows(case, inp, dtype, mutant):
    B, T, G, cg, cgp = case.B, case.T, case.G, case.cg, case.cgp
    pl, pr = case.pads
    x = inp["x"].to(dtype).view(B, T, G, cg).permute(0, 2, 1, 3)
    fill = float(torch.tensor([SENTINEL], dtype=torch.int16).view(torch.bfloat16)) if mutant == "padrow" else 0.0
    out = torch.full((B, G, pl + T + pr, cgp), fill, dtype=dtype)
    out[:, :, pl:pl + T, cg:] = 0.0
    out[:, :, pl:pl + T, :cg] = x
    if mutant == "padchan":  # the vector path copying whole chunks up to cgp: the next group's channels (here: the own ones again)
        out[:, :, pl:pl + T, cg:] = x[..., :cgp - cg]
    bound = torch.zeros(out.shape, dtype=torch.float64)
    if case.xdt == "f32":
        bound = store_term(out, "bf16")
    return {"want": out, "A": out.double().abs(), "bound": bound}


def _pool(case, inp, dtype, reverse):
    x = inp["x"].to(dtype)
    To = case.T // 2
    a, c = x[:, 0:2 * To:2], x[:, 1:2 * To:2]
    want = 0.5 * ((c + a) if reverse else (a + c))
    return {"want": want, "A": 0.5 * (a.double().abs() + c.double().abs()), "bound": U32 * want.double().abs() + store_term(want, "bf16")}


def forward(case: Case, inp: dict, dtype=torch.float64, reverse=False, mutant=None) -> dict:
    """The op in `dtype` arithmetic: float64 = the reference; float32 with reverse=True = the stand-in for a correct kernel."""
    assert mutant is None or mutant in MUTANTS
    if case.op == "w2v_stem0":
        return _w2v(case, inp, dtype, reverse, mutant)
    if case.op == "whisper_stem1":
        return _stem1(case, inp, dtype, reverse, mutant)
    if case.op == "grouped_conv":
        return _gconv(case, inp, dtype, reverse, mutant)
    if case.op == "group_windows":
        return _windows(case, inp, dtype, mutant)
    if case.op == "avgpool_time2":
        return _pool(case, inp, dtype, reverse)
    raise ValueError(case.op)


def reference(case: Case, inp: dict) -> dict:
    return forward(case, inp)


def emulate(case: Case, inp: dict) -> dict:
    """A correct kernel's stand-in: fp32 arithmetic, taps and channels in the opposite order, gelu_poly, a bf16 store."""
    r = forward(case, inp, torch.float32, reverse=True)
    return {"y": store(r["want"], "bf16"), "guard_bad": False}


def mutant_output(case: Case, inp: dict, mutant: str) -> dict:
    """What a kernel with the named defect would return (float64 arithmetic otherwise, rounded to bf16)."""
    r = forward(case, inp, mutant=mutant)
    return {"y": store(r["want"], "bf16", trunc=mutant == "trunc"), "guard_bad": bool(r.get("guard_bad", False))}


def mutant_applies(case: Case, mutant: str) -> bool:
    """Whether the defect changes anything a case of this shape could see."""
    op = case.op
    return {
        "tap_edge": op == "whisper_stem1",
        "padrow": op == "whisper_stem1" or (op == "group_windows" and sum(case.pads) > 0),
        "trunc": op != "group_windows" or case.xdt == "f32",
        "x_unrounded": op == "whisper_stem1",
        "var_unbiased": op == "w2v_stem0" and case.norm == "instance" and 1 < case.T <= 257,
        "var_second_order": op == "w2v_stem0" and case.norm == "instance",
        "chunk_edge": op == "w2v_stem0" and case.T > TCH,
        "group_swap": op == "grouped_conv" and case.G > 1,
        "kpad_tap": op == "grouped_conv" and kp(case) > case.k * case.cgp and case.T > 1,
        "row_dup": op == "grouped_conv" and case.cg % 16 != 0,
        "tile_edge": op == "grouped_conv" and case.T > 1,
        "act_after_resid": op == "grouped_conv" and case.act == "gelu" and case.resid,
        "onepass": op == "w2v_stem0" and case.norm == "layer",
        "padchan": op == "group_windows" and case.cg % 8 == 0 and case.cgp - case.cg >= 8,
    }[mutant]


def accepts(case: Case, got: dict, ref: dict) -> tuple[bool, float]:
    """The GPU suite's verdict: bf16 output; the exact family EQUALS want.to(bf16), every other stays within MARGIN x the bound
    (a zero bound means exact); a touched sentinel (guard_bad) is a rejection."""
    y = got["y"]
    if y.dtype != torch.bfloat16 or got.get("guard_bad"):
        return False, float("inf")
    if case.family == "exact":
        ok = y.shape == ref["want"].shape and torch.equal(y, store(ref["want"], "bf16"))
        return ok, 0.0 if ok else float("inf")
    rt = ratio(y, ref["want"], ref["bound"])
    return rt <= MARGIN, rt


def uninformative_fraction(ref: dict) -> float:
    """Share of a case's elements whose bound exceeds half of |want| (a comparison that says little); exact zeros do not count."""
    w, b = ref["want"].double().abs(), ref["bound"]
    return float(((b > 0.5 * w) & (b > 0)).double().mean())


# --------------------------------------------------------------------------------------------------------------- running a case
def out_shape(case: Case) -> tuple[int, ...]:
    if case.op == "w2v_stem0":
        return case.B, case.T, case.C
    if case.op == "whisper_stem1":
        return case.B, case.T + 2, case.d
    if case.op == "grouped_conv":
        return case.B * case.T, case.G * case.cg
    if case.op == "group_windows":
        return case.B, case.G, sum(case.pads) + case.T, case.cgp
    return case.B, case.T // 2, case.d


def _typed(case: Case, inp: dict) -> dict:
    """The operands in each kernel's own dtype (CPU, contiguous)."""
    t = {k: v for k, v in inp.items() if v is not None}
    if case.op == "whisper_stem1":
        t["w"] = t["w"].bfloat16()
    elif case.op == "grouped_conv":
        t["x"], t["w"] = t["x"].bfloat16(), t["w"].bfloat16()
        if "resid" in t:
            t["resid"] = t["resid"].bfloat16()
    elif case.op == "avgpool_time2" or (case.op == "group_windows" and case.xdt == "bf16"):
        t["x"] = t["x"].bfloat16()
    return {k: v.contiguous() for k, v in t.items()}


def _wide(t: torch.Tensor, extra: int, fill: float, dev) -> torch.Tensor:
    """t (..., cols) as the leading columns of rows `extra` elements wider, the rest `fill`."""
    if not extra:
        return t.to(dev).clone()
    buf = torch.full((*t.shape[:-1], t.shape[-1] + extra), fill, dtype=t.dtype, device=dev)
    buf[..., :t.shape[-1]] = t.to(dev)
    return buf[..., :t.shape[-1]]


def to_device(case: Case, inp: dict, dev) -> dict:
    """Plain copies for the ops wrappers; the row strides ldr / ldx > d come from a wider tensor's leading columns."""
    t = {k: v.to(dev).clone() for k, v in _typed(case, inp).items()}
    if case.op == "grouped_conv" and "resid" in t:
        t["resid"] = _wide(t["resid"], case.ld_extra, float("nan"), dev)
    if case.op == "group_windows":
        t["x"] = _wide(t["x"], case.ld_extra, float("nan"), dev)
    return t


def run(ops, case: Case, t: dict) -> dict:
    """One launch through pytorch_models._hip.ops."""
    if case.op == "w2v_stem0":
        return {"y": ops.w2v_stem0(t["x"], t["w"], t.get("bias"), case.norm, t.get("gamma"), t.get("beta"), EPS, case.stride)}
    if case.op == "whisper_stem1":
        return {"y": ops.whisper_stem1(t["x"], t["w"], t["bias"])}
    if case.op == "grouped_conv":
        return {"y": ops.grouped_conv(t["x"], t["w"], t.get("bias"), case.k, case.stride, case.cg, case.act, t.get("resid"))}
    if case.op == "group_windows":
        return {"y": ops.group_windows(t["x"], case.G, case.cgp, *case.pads)}
    if case.op == "avgpool_time2":
        return {"y": ops.avgpool_time2(t["x"])}
    raise ValueError(case.op)


def _ibits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def embedded(t: torch.Tensor, dev, ld: int = 0, sentinel: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """t as the middle slice of a flat buffer filled with NaN (sentinel: the bf16 guard pattern), rows `ld` wide (0: dense), a guard of
    >= one row and a multiple of 64 elements in front and behind, so the slice keeps the buffer's 16-byte alignment.
    Returns (buffer, view)."""
    cols = t.shape[-1]
    ld = ld or cols
    rows = t.numel() // cols
    guard = -(-max(ld, 64) // 64) * 64
    buf = torch.full((2 * guard + rows * ld,), float("nan"), dtype=t.dtype)
    if sentinel:
        _ibits(buf).fill_(SENTINEL)
    buf = buf.to(dev)
    view = buf[guard:guard + rows * ld].view(rows, ld)[:, :cols]
    if not sentinel:
        view.copy_(t.reshape(rows, cols))
    assert view.data_ptr() % 16 == 0
    return buf, view


def sentinels_intact(buf: torch.Tensor, view: torch.Tensor) -> bool:
    """Every element of the flat bf16 buffer outside `view` still holds the guard pattern."""
    b = _ibits(buf.cpu()).clone()
    rows, cols = view.shape
    ld = view.stride(0)
    guard = (buf.numel() - rows * ld) // 2
    mid = b[guard:guard + rows * ld].view(rows, ld)
    mid[:, :cols] = SENTINEL
    return bool((b == SENTINEL).all())


def run_abi(ops, case: Case, inp: dict, dev) -> dict:
    """The poison family's launch through lib(): NaN-surrounded operands, a sentinel-surrounded output (grouped_conv: ldy = d + 8,
    ldr = d + 4 + ld_extra).  Returns y (dense copy) and guard_bad."""
    L, st = ops.lib(), ops._stream()
    t = _typed(case, inp)
    ld_in = {"resid": case.G * case.cg + 4 + case.ld_extra} if case.op == "grouped_conv" else {}
    if case.op == "group_windows":
        ld_in["x"] = case.d + case.ld_extra
    P = {k: embedded(v, dev, ld_in.get(k, 0))[1] for k, v in t.items()}
    ptr = lambda k: P[k].data_ptr() if k in P else None  # noqa: E731
    shape = out_shape(case)
    ldy = shape[-1] + (8 if case.op == "grouped_conv" else 0)
    obuf, oview = embedded(torch.empty(shape, dtype=torch.bfloat16), dev, ldy, sentinel=True)
    if case.op == "w2v_stem0":
        part = stats = None
        if case.norm == "instance":
            n = int(L.pm_w2v_stem0_scratch_floats(case.B, case.T))
            part = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            stats = torch.full((case.B, case.C, 2), float("nan"), dtype=torch.float32, device=dev)
        rc = L.pm_w2v_stem0(ptr("x"), ptr("w"), ptr("bias"), {"none": 0, "layer": 1, "instance": 2}[case.norm], ptr("gamma"), ptr("beta"), EPS,
                            part.data_ptr() if part is not None else None, stats.data_ptr() if stats is not None else None,
                            oview.data_ptr(), case.B, wave_len(case), case.C, 10, case.stride, st)
    elif case.op == "whisper_stem1":
        rc = L.pm_whisper_stem1(ptr("x"), ptr("w"), ptr("bias"), oview.data_ptr(), case.B, case.C, cpad(case), case.T, case.d, st)
    elif case.op == "grouped_conv":
        rc = L.pm_grouped_conv_bf16(ptr("x"), ptr("w"), ptr("bias"), ptr("resid"), ld_in["resid"] if "resid" in P else 0, oview.data_ptr(), ldy,
                                    case.B, case.G, tp(case), case.cg, case.cgp, case.k, case.stride, kp(case), ops.ACT[case.act], st)
    elif case.op == "group_windows":
        rc = L.pm_group_windows(ptr("x"), ld_in["x"], ops._dt(P["x"]), oview.data_ptr(), case.B, case.T, case.G, case.cg, case.cgp, *case.pads, st)
    else:
        rc = L.pm_avgpool_time2(ptr("x"), oview.data_ptr(), case.B, case.T, case.d, st)
    assert rc == 0, (case.id, rc)
    return {"y": oview.cpu().contiguous().view(shape), "guard_bad": not sentinels_intact(obuf, oview)}


def clip(case: Case, inp: dict, b: int) -> tuple[Case, dict]:
    """The single-clip problem of clip b (batch family)."""
    To = case.T
    one = {}
    for k, v in inp.items():
        if v is None or k not in ("x", "resid"):
            one[k] = v
        elif k == "resid":
            one[k] = v[b * To:(b + 1) * To].clone()
        else:
            one[k] = v[b:b + 1].clone()
    return replace(case, B=1), one


def rows_of_clip(case: Case, y: torch.Tensor, b: int) -> torch.Tensor:
    return y.reshape(case.B, -1)[b]


# =============================================================================================================== STFT / mel / log-mel
# pm_stft_mel / pm_stft_mel_folded / pm_logmel_finalize through ops.stft_mel.  The twiddle tables are OPERANDS (ops.stft_mel takes
# them as arguments), so the reference is the float64 contraction of exactly those tables with the reflect-padded frames; for real
# windows tests/test_audio_cases_cpu.py also holds that contraction against torch.stft in float64 (table rounding u A and the
# window symmetrisation, computed from the window, are what separates the two).
# Bounds: delta_re, delta_im = (n + 2) u A over the n-term chain (n = n_fft plain; n_fft / 2 + 2 folded: the a +- m add is one more
# rounding of each term); power p = re^2 + im^2: 2 |re| delta_re + 2 |im| delta_im + delta_re^2 + delta_im^2 + 3 u p; mel row of ne
# entries (fma chain): sum val delta_p + (ne + 1) u acc; log10: delta_acc / (acc ln 10) + 4 u |log10 acc| (log10f: 2 ulp); the peak is a
# maximum, 1-Lipschitz: delta_peak = the largest delta among the elements that can be the maximum; floor and affine map:
# max(delta_v, delta_peak) / 4 + 2 u |out| (delta_v only where the element can stay above the floor).  want = -inf (an all-silent clip) and
# want = 0 with bound 0 (an empty mel row in mode 1, integer tables) must be met exactly.
STFT_MUTANTS = ("reflect_edge", "frame_shift", "mirror_n0", "half_nyq", "bin_rows", "mel_tail", "peak_global", "floor_first")
STFT_MUTANT_FAMILY = {"reflect_edge": "exact", "frame_shift": "exact", "mirror_n0": "exact", "half_nyq": "exact", "bin_rows": "exact",
                      "mel_tail": "exact", "peak_global": "loudness", "floor_first": "loudness"}
FT = 32  # csrc/logmel.hip: frames per workgroup


@dataclass(frozen=True)
class StftCase:
    family: str
    n_fft: int
    hop: int
    T: int
    mode: int = 0
    n_mels: int = 0
    win: str = "hann"          # hann (symmetric: folded tables) | asym (plain) | int (integer plain tables) | intfold (integer folded)
    B: int = 1
    n_frames: int = 0          # 0: 1 + T // hop
    lead: tuple = ()           # leading dims in place of B
    empty_row: bool = False

    @property
    def id(self) -> str:
        s = f"stft-{self.family}-n{self.n_fft}h{self.hop}-t{self.T}-f{self.frames}-m{self.mode}"
        s += (f"x{self.n_mels}" if self.mode else "") + ("e" if self.empty_row else "") + f"-{self.win}-b{'x'.join(map(str, self.lead)) or self.B}"
        return s

    @property
    def frames(self) -> int:
        return self.n_frames or 1 + self.T // self.hop

    @property
    def clips(self) -> int:
        return int(torch.Size(self.lead).numel()) if self.lead else self.B

    @property
    def folded(self) -> bool:
        return self.win in ("hann", "intfold")

    @property
    def nk(self) -> int:
        return 2 * ((self.n_fft // 2 + 2) // 2) if self.folded else self.n_fft


def stft_lds_bytes(c: StftCase, mode: int | None = None) -> int:
    mode = c.mode if mode is None else mode
    nsamp = c.hop * (FT - 1) + c.n_fft
    skewed = ((nsamp + nsamp // c.hop + 1) + 3) & ~3
    return 4 * (skewed + ((c.n_fft // 2 + 1) * FT if mode else 0) + (4 * ((c.n_fft // 2 + 2) // 2) if c.folded else 0))


def stft_refusal(c: StftCase) -> str | None:
    if c.n_fft % 2 or c.hop % 2 or c.hop < 2 or c.n_fft > 2048 or c.T <= c.n_fft // 2 or c.frames > 1 + c.T // c.hop:
        return "stft_mel: even n_fft <= 2048, even hop, T > n_fft / 2, n_frames <= 1 + T / hop"
    if stft_lds_bytes(c) > 64 * 1024:
        return "stft_mel: more than 64 KiB of LDS"
    if c.mode == 2 and (c.n_mels * c.frames) % 4:
        return "logmel_finalize: per_clip % 4 == 0"
    return None


def stft_paths(c: StftCase) -> set[str]:
    nbins = c.n_fft // 2 + 1
    nblk = -(-nbins // 32)
    t = {f"n{c.n_fft}h{c.hop}", "folded" if c.folded else "plain", f"mode{c.mode}"}
    if nblk < 4:
        t.add("idle-waves")
    if nblk == 1:
        t.add("nblk1")
    if nbins % 32 == 1:
        t.add("single-bin-block")
    if c.hop > c.n_fft:
        t.add("hop>n_fft")
    if (c.n_fft // 2) % 2:
        t.add("odd-half")
    if c.T == c.n_fft // 2 + 1:
        t.add("shortest-T")
    if c.T % c.hop:
        t.add("T%hop")
    if c.frames == c.T // c.hop:
        t.add("dropped-last-frame")
    if c.frames in (1, 31, 32, 33, 65):
        t.add(f"frames{c.frames}")
    if c.mode and c.n_mels % 8:
        t.add("n_mels%8")
    if c.mode:
        t.add(f"n_mels{c.n_mels}")
    if c.empty_row:
        t.add("empty-row")
    if c.clips > 1:
        t.add("clips>1")
    if c.lead:
        t.add("leading-dims")
    if stft_lds_bytes(c) > 48 * 1024:
        t.add("lds>48k")
    return t


STFT_REQUIRED = {"n400h160", "n16h4", "n128h64", "n8h2", "n16h32", "n402h6", "n512h128", "n1024h256", "folded", "plain", "mode0", "mode1", "mode2",
                 "idle-waves", "nblk1", "single-bin-block", "hop>n_fft", "odd-half", "shortest-T", "T%hop", "dropped-last-frame", "frames1",
                 "frames31", "frames32", "frames33", "frames65", "n_mels%8", "n_mels1", "n_mels5", "n_mels80", "n_mels128", "empty-row", "clips>1",
                 "leading-dims", "lds>48k"}

S = StftCase
STFT_CASES = [
    # exact: integer tables in the kernel's layout, integer samples
    S("exact", 16, 4, 9, win="int"), S("exact", 16, 4, 9, win="intfold", B=3), S("exact", 8, 2, 61, 1, 5, "intfold", 3, n_frames=31),
    S("exact", 8, 2, 64, 1, 5, "int", n_frames=32, empty_row=True), S("exact", 128, 64, 2100, win="intfold", n_frames=33),
    S("exact", 128, 64, 2100, win="int", B=3, n_frames=33),
    S("exact", 400, 160, 5333, 1, 80, "intfold", n_frames=33), S("exact", 400, 160, 5333, win="int", n_frames=33), S("exact", 16, 32, 300, win="int", B=3),
    S("exact", 16, 32, 300, 1, 1, "intfold"), S("exact", 402, 6, 400, win="intfold", n_frames=65), S("exact", 402, 6, 202, 1, 1, "int", n_frames=31),
    S("exact", 512, 128, 4096, 1, 128, "intfold", n_frames=32), S("exact", 1024, 256, 2000, win="int", n_frames=1),
    S("exact", 1024, 256, 2000, win="intfold", B=3),
    # cancel: pure tones, far bins by the bound
    S("cancel", 400, 160, 4800), S("cancel", 400, 160, 4800, win="asym"), S("cancel", 128, 64, 2000), S("cancel", 16, 4, 50, win="asym"),
    S("cancel", 1024, 256, 3000), S("cancel", 402, 6, 300, win="asym"),
    # poison: Gaussian, all three modes
    S("poison", 400, 160, 5280, 2, 80, n_frames=33), S("poison", 512, 128, 4096, 2, 128), S("poison", 512, 128, 4096, 1, 128, win="asym"),
    S("poison", 8, 2, 40, 1, 5, "asym", empty_row=True), S("poison", 16, 32, 300, 0), S("poison", 402, 6, 202, 2, 8, n_frames=32),
    S("poison", 128, 64, 65, 0, win="asym"),
    # batch: clip b of the batch run is the single-clip run, the per-clip peak included
    S("batch", 400, 160, 3200, 2, 80, B=3, n_frames=20), S("batch", 16, 4, 70, 0, lead=(2, 2)), S("batch", 8, 2, 33, 1, 5, "asym", 3),
    # loudness: amplitude 100, amplitude 1e-3, a half-silent clip, an all-zero clip
    S("loudness", 400, 160, 3200, 2, 80, B=4, n_frames=20), S("loudness", 16, 4, 64, 2, 8, "asym", 4, n_frames=16, empty_row=True),
]
STFT_REFUSED = (S("poison", 1024, 256, 3000, 1, 8), S("poison", 2048, 512, 5000), S("poison", 16, 4, 40, 2, 5, n_frames=3))
assert len({c.id for c in STFT_CASES}) == len(STFT_CASES)


def _pack_table(m: torch.Tensor, nblk: int) -> torch.Tensor:
    """(nk, nblk * 32) -> the kernels' [nblk][nk / 2][2][32] layout."""
    nk = m.shape[0]
    return m.float().view(nk // 2, 2, nblk, 32).permute(2, 0, 1, 3).contiguous().view(-1)


def _unpack_table(t: torch.Tensor, nk: int, nblk: int) -> torch.Tensor:
    return t.view(nblk, nk // 2, 2, 32).permute(1, 2, 0, 3).reshape(nk, nblk * 32)


def stft_window(c: StftCase) -> torch.Tensor | None:
    if c.win.startswith("int"):
        return None
    w = torch.hann_window(c.n_fft, periodic=True, dtype=torch.float64)
    return (w if c.win == "hann" else w * torch.linspace(0.7, 1.3, c.n_fft, dtype=torch.float64) + 0.01).float()


def stft_build(c: StftCase, stft_tables) -> dict:
    """x (clips, T) f32, the two tables, the filterbank (dense f32 and CSR).  stft_tables: ops.stft_tables (host code)."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % 100003)
    N, nbins = c.n_fft, c.n_fft // 2 + 1
    nblk, nk, B, T = -(-nbins // 32), c.nk, c.clips, c.T
    out: dict = {}
    if c.win.startswith("int"):
        live = N // 2 + 1 if c.folded else N
        dens = min(1.0, 150.0 / live)
        tabs = []
        for _ in range(2):
            m = torch.zeros(nk, nblk * 32)
            m[:live, :nbins] = torch.randint(-1, 2, (live, nbins), generator=g).float() * (torch.rand(live, nbins, generator=g) < dens)
            tabs.append(_pack_table(m, nblk))
        out["tables"] = (tabs[0], tabs[1], c.folded)
        out["x"] = torch.randint(-2, 3, (B, T), generator=g).float()
    else:
        tc, ts, folded = stft_tables(stft_window(c), N)
        assert folded == c.folded
        out["tables"] = (tc, ts, folded)
        t = torch.arange(T, dtype=torch.float64)
        if c.family == "cancel":
            out["x"] = torch.stack([torch.sin(2 * torch.pi * (0.11 + 0.07 * b) * t + b) for b in range(B)]).float()
        elif c.family == "loudness":
            tone = torch.sin(2 * torch.pi * 0.05 * t) + 0.1 * torch.randn(T, generator=g).double()
            half = tone * 0.1 * (t < T // 2)
            out["x"] = torch.stack([100.0 * tone, 1e-3 * tone, half, torch.zeros(T, dtype=torch.float64)]).float()
        else:
            out["x"] = torch.randn(B, T, generator=g)
    if c.mode:
        F_ = torch.zeros(c.n_mels, nbins)
        width = max(2, -(-nbins // c.n_mels) + 1)
        for m in range(c.n_mels):
            lo = min(m * nbins // c.n_mels, nbins - 1)
            hi = min(lo + width, nbins)
            F_[m, lo:hi] = (torch.randint(1, 3, (hi - lo,), generator=g).float() if c.win.startswith("int")
                            else (0.2 + torch.rand(hi - lo, generator=g)) / width)
        if c.empty_row:
            F_[c.n_mels // 2] = 0.0
        out["filters"] = F_
    return out


def _stft_frames(c: StftCase, x: torch.Tensor, mutant) -> torch.Tensor:
    """(clips, frames, n_fft + 1): torch.stft's center = True / reflect framing, plus the sample behind each frame (mirror_n0)."""
    N, T = c.n_fft, c.T
    s = torch.arange(c.frames)[:, None] * c.hop + torch.arange(N + 1)[None, :] - N // 2 + (c.hop if mutant == "frame_shift" else 0)
    edge = 1 if mutant == "reflect_edge" else 0
    s = torch.where(s < 0, -s - edge, s)
    s = torch.where(s >= T, 2 * (T - 1) - s + edge, s).clamp(0, T - 1)
    return x[:, s]


def stft_forward(c: StftCase, inp: dict, dtype=torch.float64, mutant=None) -> dict:
    assert mutant is None or mutant in STFT_MUTANTS
    u, N, nbins = U32, c.n_fft, c.n_fft // 2 + 1
    nblk = -(-nbins // 32)
    f = _stft_frames(c, inp["x"], mutant).to(dtype)
    C = _unpack_table(inp["tables"][0], c.nk, nblk).to(dtype)
    Sn = _unpack_table(inp["tables"][1], c.nk, nblk).to(dtype)
    if c.folded:
        h = N // 2
        a, m = f[..., :h + 1], f[..., :N + 1].flip(-1)[..., :h + 1].clone()  # m[n] = f[N - n]
        if mutant != "mirror_n0":
            m[..., 0] = 0
        re, im = (a + m) @ C[:h + 1], (a - m) @ Sn[:h + 1]
        if mutant == "half_nyq":
            re = re + 2 * f[..., h, None] * C[h]
        Aa = a.double().abs() + m.double().abs()
        Are, Aim, n = Aa @ C[:h + 1].double().abs(), Aa @ Sn[:h + 1].double().abs(), h + 2
    else:
        re, im = f[..., :N] @ C, f[..., :N] @ Sn
        Are, Aim, n = f[..., :N].double().abs() @ C.double().abs(), f[..., :N].double().abs() @ Sn.double().abs(), N
    if mutant == "bin_rows":  # rows 0 .. 3 and 4 .. 7 of every group of 8 swapped
        perm = torch.arange(nblk * 32) ^ 4
        re, im = re[..., perm], im[..., perm]
    dre, dim_ = (n + 2) * u * Are, (n + 2) * u * Aim
    p = re * re + im * im
    red, imd = re.double().abs(), im.double().abs()
    dp = 2 * red * dre + 2 * imd * dim_ + dre * dre + dim_ * dim_ + 3 * u * p.double()
    p, dp, Ap = p[..., :nbins].transpose(-1, -2), dp[..., :nbins].transpose(-1, -2), (Are * Are + Aim * Aim)[..., :nbins].transpose(-1, -2)
    r = {"re": re[..., :nbins], "im": im[..., :nbins], "A": Ap}
    if c.mode == 0:
        r.update(want=p, bound=dp)
    else:
        Fm = inp["filters"].clone()
        if mutant == "mel_tail":
            for row in Fm:
                nz = row.nonzero()
                if len(nz):
                    row[nz[-1]] = 0
        acc = Fm.to(dtype) @ p
        ne = (inp["filters"] != 0).sum(1).double()[:, None]
        dacc = inp["filters"].double() @ dp + (ne + 1) * u * acc.double()
        r["A"] = inp["filters"].double() @ Ap
        if c.mode == 1:
            r.update(want=acc, bound=dacc)
        else:
            accf = acc.clamp_min(1e-10) if mutant == "floor_first" else acc
            v = torch.log10(accf)
            vd = v.double()
            slope = dacc / (acc.double().clamp_min(1e-300) * 2.302585092994046)
            dv = torch.where(acc.double() > 0, slope + 4 * u * vd.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0), torch.zeros_like(dacc)).clamp_max(1e30)
            flat, dflat = vd.flatten(1), dv.flatten(1)
            peak = flat.max(1).values
            if mutant == "peak_global":
                peak = peak.max().expand_as(peak)
            lower = (flat - dflat).max(1, keepdim=True).values
            dpk = torch.where(flat + dflat >= lower, dflat, torch.zeros_like(dflat)).max(1).values
            pk, dpk = peak[:, None, None], dpk[:, None, None]
            o = (torch.maximum(v, pk.to(dtype) - 8) + 4) / 4
            live = vd + dv > pk - 8 - dpk
            bound = torch.maximum(torch.where(live, dv, torch.zeros_like(dv)), dpk.expand_as(dv)) / 4 + 2 * u * o.double().abs().nan_to_num(0.0, neginf=0.0)
            bound = torch.where(torch.isinf(o.double()), torch.zeros_like(bound), bound)
            r.update(want=o, bound=bound, peak=peak)
    rows = nbins if c.mode == 0 else c.n_mels
    shape = (*(c.lead or (c.B,)), rows, c.frames)
    r["want"], r["bound"] = r["want"].reshape(shape), r["bound"].reshape(shape)
    return r


def stft_ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """ratio() with want = -inf allowed: such an element must be -inf in the output too; every other element finite."""
    if got.shape != want.shape:
        return float("inf")
    inf = torch.isinf(want)
    if not torch.equal(got.double()[inf], want.double()[inf]):
        return float("inf")
    keep = ~inf
    return ratio(got[keep], want[keep], bound[keep])


def stft_accepts(c: StftCase, y: torch.Tensor, ref: dict) -> tuple[bool, float]:
    if y.dtype != torch.float32:
        return False, float("inf")
    if c.family == "exact":
        ok = y.shape == ref["want"].shape and torch.equal(y.double(), ref["want"])
        return ok, 0.0 if ok else float("inf")
    r = stft_ratio(y, ref["want"], ref["bound"])
    return r <= MARGIN, r


def stft_emulate(c: StftCase, inp: dict) -> torch.Tensor:
    return stft_forward(c, inp, torch.float32)["want"].float()


def stft_mutant_output(c: StftCase, inp: dict, mutant: str) -> torch.Tensor:
    return stft_forward(c, inp, mutant=mutant)["want"].float()


def stft_mutant_applies(c: StftCase, mutant: str) -> bool:
    return {"reflect_edge": True, "frame_shift": True, "mirror_n0": c.folded, "half_nyq": c.folded, "bin_rows": c.n_fft >= 16,
            "mel_tail": c.mode >= 1, "peak_global": c.mode == 2 and c.clips > 1, "floor_first": c.mode == 2}[mutant]


def stft_csr(filters: torch.Tensor, dev):
    nz = filters != 0
    ptr = torch.zeros(filters.shape[0] + 1, dtype=torch.int32)
    ptr[1:] = nz.sum(1).cumsum(0)
    rows, cols = nz.nonzero(as_tuple=True)
    return ptr.to(dev), cols.to(torch.int32).to(dev), filters[rows, cols].contiguous().to(dev)


def stft_run(ops, c: StftCase, inp: dict, dev, x=None) -> torch.Tensor:
    """One call of ops.stft_mel on plain copies (x: another clip set of the same case, for the batch family)."""
    x = inp["x"] if x is None else x
    x = x.view(*c.lead, c.T) if c.lead and x.shape[0] == c.clips else x
    tabs = (inp["tables"][0].to(dev), inp["tables"][1].to(dev), inp["tables"][2])
    csr = stft_csr(inp["filters"], dev) if c.mode else None
    return ops.stft_mel(x.to(dev).clone(), tabs, c.n_fft, c.hop, c.frames, c.mode, csr, c.n_mels)


def stft_run_abi(ops, c: StftCase, inp: dict, dev) -> dict:
    """The poison family's launch through lib(): every operand inside NaN (the int32 CSR arrays: inside -1), the output inside sentinels."""
    L, st = ops.lib(), ops._stream()
    B, rows = c.clips, (c.n_fft // 2 + 1 if c.mode == 0 else c.n_mels)
    x = embedded(inp["x"], dev)[1]
    tc, ts = embedded(inp["tables"][0], dev)[1], embedded(inp["tables"][1], dev)[1]
    ptr = col = val = None
    if c.mode:
        p_, c_, v_ = stft_csr(inp["filters"], "cpu")
        guard = torch.full((64,), -1, dtype=torch.int32)
        pbuf, cbuf = torch.cat([guard, p_, guard]).to(dev), torch.cat([guard, c_, guard]).to(dev)
        ptr, col, val = pbuf[64:64 + p_.numel()], cbuf[64:64 + c_.numel()], embedded(v_.view(1, -1), dev)[1]
    obuf, oview = embedded(torch.empty(B * rows, c.frames, dtype=torch.float32), dev, sentinel=True)
    peak = torch.zeros(B, dtype=torch.int32, device=dev) if c.mode == 2 else None
    fn = L.pm_stft_mel_folded if c.folded else L.pm_stft_mel
    dp = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = fn(x.data_ptr(), x.stride(0), B, c.T, tc.data_ptr(), ts.data_ptr(), c.n_fft, c.hop, c.frames, c.mode, dp(ptr), dp(col), dp(val), c.n_mels,
            oview.data_ptr(), dp(peak), st)
    assert rc == 0, (c.id, rc)
    if c.mode == 2:
        rc = L.pm_logmel_finalize(oview.data_ptr(), peak.data_ptr(), B, rows * c.frames, st)
        assert rc == 0, (c.id, rc)
    shape = (*(c.lead or (c.B,)), rows, c.frames)
    return {"y": oview.cpu().contiguous().view(shape), "guard_bad": not sentinels_intact(obuf, oview)}
