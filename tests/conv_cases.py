"""References, error bounds, adversarial input families and case lists shared by the 2-D convolution parity tests
(tests/test_conv_cases_cpu.py without a GPU, tests/test_hip_conv_adversarial.py on one).  A plain helper module.

In scope (through pytorch_models._hip.ops): conv_bf16, resnet_stem, dwconv7_ln, convnext_stem, dwconv3_bn_act (y, psum, gate,
write_y=False), maxvit_stem, im2col3x3, avgpool2x2, conv2d_nhwc (dense, grouped, depthwise; act none / relu / silu; resid).
Out of scope: EnCodec's conv1d_f32 and its transposed form (the same treatment in tests/encodec_cases.py); the 1-D
grouped_conv and the wav2vec2 and Whisper stems have the same treatment in tests/audio_cases.py.

Contract ("2c. Convolution numerics contract").

Reference.  Every op is evaluated in float64 on the CPU from exactly the operands the kernel sees (bf16 operands are bf16-rounded
values kept in fp32 storage, bf16r()), as a plain loop over the filter taps (conv_taps()): the MaxViT right / bottom zero pad at
stride 2, ReLU after the residual add (conv_bf16), the activation before it (conv2d_nhwc), GELU-tanh, LayerNorm with the biased
variance, zero pad columns up to ldy.  Beside `want` it returns A = sum |x w| + |bias| (+ |resid|) per output and, for the
LayerNorm kernels, the pre-LN row z, its mean and its sigma = sqrt(var + eps).

Bounds.  u = 2^-24 (fp32 unit roundoff), no number measured on a kernel enters one:
  * convolution with fp32 accumulation of K terms in ANY order (an MFMA tree, an fma chain): delta = (K + 2) u A - K - 1 additions
    and, for fma chains, no product rounding (bf16 x bf16 products are exact in fp32 anyway), + 2 for the bias and residual adds;
  * store: half a bf16 ulp of want, 2^(floor(log2 |want|) - 8), for a round-to-nearest bf16 store; u |want| to f32.  bf16 has 8
    significand bits, so half an ulp lies between 2^-9 |want| (just below a power of two) and 2^-8 |want| (at one).  The
    flat 2^-9 |want| is NOT satisfiable: a correctly rounded store of 1.00390625 is off by 2^-8.  The half ulp is the tightest
    form a correct kernel meets, and it still separates truncation, whose error reaches a whole ulp = 2 x the term;
  * ReLU and max-pool are 1-Lipschitz: delta passes through (the pool takes the window's largest bound);
  * folded BatchNorm t = fma(z, scale, shift): delta_t = |scale| delta + u |t|;
  * GELU-tanh g = 0.5 t (1 + tanh(c (t + 0.044715 t^3))): delta_g = 1.13 delta_t + u (4 |t| + 2 |g|).  1.13 >= sup |g'| = 1.129.
    The device term: the argument carries <= 4 u relative (three products, one fma) and |a| sech^2 a <= 0.45, tanhf <= 2 ulp of
    a value <= 1, 1 + tanh rounds once more (<= 2 u absolute): together <= 5.8 u on the factor (1 + tanh), times 0.5 |t| gives
    < 3 u |t|, rounded up to 4 u |t| (it is ABSOLUTE in t: for t << 0 the factor cancels and g itself is tiny); the two outer
    products add 2 u |g|;
  * SiLU s = z / (1 + exp(-z)): delta_s = 1.10 delta + 4 u |s| (sup |s'| = 1.0998; expf <= 2 ulp, the add and the division one
    rounding each, and e / (1 + e) <= 1);
  * gate y = g gate: delta_y = |gate| delta_g + u |y|;  row sums psum = sum_w g, Wo terms in sequence:
    delta_ps = sum_w delta_g + (Wo - 1) u sum_w |g|;
  * LayerNorm over C channels after a convolution with per-channel delta_c: with e = max_c delta_c + C u mean_c |z_c| (the second
    term covers the fp32 mean and the centred squares), |dy_c| <= |gamma_c| / sigma (2 + |yhat_c|) e: the mean moves by <= e, a
    centred value by <= 2 e, sigma by <= e relative to sigma times |yhat|; then the store term.
  * avgpool2x2: K = 4, A = mean |x|;  im2col3x3 copies: only the store term (zero unless f32 -> bf16).
The GPU suite asserts MARGIN = 1.5 x the bound (second-order terms, as the attention contract does); an element whose bound is 0
must be exact; a non-finite output is an infinite ratio (ratio()).

Families.
  exact   x, w small integers in [-3, 3] (x sparse), bias / resid integers in [-8, 8]: every product and partial sum is an integer
          below 2^24, so fp32 arithmetic is exact in any order and the output must EQUAL want.to(out dtype).  At least 90 % of a
          case's outputs satisfy |want| <= 256 (exact in bf16; asserted on the CPU).  conv_bf16, conv2d_nhwc (none / relu),
          resnet_stem, im2col3x3, avgpool2x2.  A wrong tap, chunk, swizzle, image index, edge guard or bias lane is a bit difference.
  cancel  real operands, every filter's taps sum to about 0, x = a large smooth offset + small noise: |want| << A.  By the bound.
  offset  (LayerNorm kernels, C <= 96) the bias puts the pre-LN row at |mean| / sigma ~ 4096: an fp32 two-pass LayerNorm sits
          at a few hundredths of the bound, a one-pass E[z^2] - mean^2 variance is orders of magnitude outside.  The bound's
          factor C makes the family toothless at C >= 768 (one-pass is only 2.4 x over at 768 / 1024): not used there.
  poison  Gaussian operands; on the GPU every operand is the middle slice of a NaN-filled buffer (16-byte aligned, checked):
          finite output, bit-identical to the run on plain copies, and the plain run inside the bound.
  batch   Gaussian operands, N > 1: image n of the batch run is bit-identical to the single-image run; batch run by the bound.

Path -> case (the smallest shapes that reach each path; paths() derives the tags from the shape, the CPU test asserts them all):
  conv_bf16   BN = 64 with clamped weight rows (Cout 8, 24, 40)      conv_bf16-*-1x1x127x64-o8..., -1x8x16x128-o24, -2x3x2x64-o40
              nk = 1 (no prefetch) / nk = 2                            -1x1x1x64-o64-k1s1 / -1x8x16x128-o24-k1s1
              M = 1, 127, 128, 129                                      -1x1x1x64 / -1x1x127x64 / -1x8x16x128 / -1x3x43x64
              a 128-row tile over three images at stride 2 (pix0)       -3x10x19x64-o68-k3s2 (Ho Wo = 50)
              8-byte stores (Cout % 8 = 4) / scalar stores               -o68, -o132 / -o65, -o130
              H or W of 1 or 2 at stride 2                              -1x2x2x192-o128, -1x3x1x64-o130, -2x1x3x64-o132
              all four <RES, RELU> instantiations at both BN            asserted by the CPU test from the case list
  dwconv7_ln  SW = 4 (C > 2048)                                         dwconv7_ln-*-1x2x9x2052, -3x5x17x4096, -1x1x1x4096
              sblk = 1 / 64 KiB of dynamic LDS                          -1x3x3x1028, -3x1x8x2048, -3x5x17x4096
              many strips per workgroup across rows and images (C = 4)  -3x5x17x4, -3x2x9x4
              W < 4 / W = 1 / W = 8 / H = 1                             -3x3x3x40 / -1x1x1x8 / -1x1x8x40 / -3x1x8x2048
  maxvit_stem NCH = 2 / 4, ragged last channel block, ldy > d           maxvit_stem-*-d65, -d96, -d128 / -d200, -d256 / -d200-ld256
  dwconv3     C = 4, W = 1, H = 1 at stride 1                           dwconv3-*-2x7x7x4-s1, -2x5x1x40-s1, -2x1x5x40-s1
              2 x 2 and 3 x 2 at stride 2 (one output pixel / row)      -2x2x2x4-s2, -2x3x2x40-s2
  resnet_stem window larger than the image, 1 x 1 and 1 x k conv maps   resnet_stem-*-2x1x1, -2x2x3, -2x5x5
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
BF16_BITS = 8  # significand bits of bf16 (7 stored): half an ulp of w is 2^(floor(log2 |w|) - 8), between 2^-9 |w| and 2^-8 |w|
GELU_LIP = 1.13
SILU_LIP = 1.10
MARGIN = 1.5
EPS = 1e-6
OFFSET_RATIO = 4096.0
MUTANTS = ("replicate", "origin", "transpose", "chunkswap", "tileimg", "relu_first", "trunc", "onepass", "biastail", "padcols")
LN_OPS = ("dwconv7_ln", "convnext_stem")
EXACT_OPS = ("conv_bf16", "conv2d_nhwc", "resnet_stem", "im2col3x3", "avgpool2x2")
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """Nearest bf16 value, kept in fp32 storage: both paths see exactly these numbers."""
    return x.to(torch.bfloat16).float()


def store_term(want: torch.Tensor, dt: str) -> torch.Tensor:
    """The error of one correctly rounded store of `want`: half a bf16 ulp, 2^(floor(log2 |want|) - 8), or 2^-24 |want| to f32."""
    a = want.double().abs().nan_to_num(0.0)
    if dt != "bf16":
        return U32 * a
    _, ex = torch.frexp(a)  # a = m 2^ex with m in [0.5, 1)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), ex - 1 - BF16_BITS), torch.zeros_like(a))


def store(want: torch.Tensor, dt: str, trunc: bool = False) -> torch.Tensor:
    """The value a correct kernel stores: round to nearest even.  trunc: the deliberately wrong bf16 conversion."""
    w32 = want.float()
    if dt == "bf16" and trunc:
        return (w32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return w32.to(DT[dt])


def ratio(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want| / bound; an element whose bound is 0 must be exact, a non-finite output is an infinite ratio."""
    if got.shape != want.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - want.double()).abs()
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    """One problem.  C = input channels (3 for the stems), Cout = output channels / the stems' width d (0: same as C)."""
    op: str
    family: str
    N: int
    H: int
    W: int
    C: int
    Cout: int = 0
    k: int = 3
    stride: int = 1
    pad: int = 0
    groups: int = 1
    bias: bool = True
    resid: bool = False
    act: str = "none"
    xdt: str = "bf16"
    ydt: str = "bf16"
    ldy: int | None = None
    gate: bool = False

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.family}-{self.N}x{self.H}x{self.W}x{self.C}"
        if self.op in ("conv_bf16", "conv2d_nhwc"):
            s += f"-o{self.Cout}-k{self.k}s{self.stride}" + (f"g{self.groups}" if self.groups > 1 else "")
            s += ("-b" if self.bias else "") + ("-r" if self.resid else "") + (f"-{self.act}" if self.act != "none" else "")
        elif self.op in ("convnext_stem", "maxvit_stem"):
            s += f"-d{self.Cout}"
        elif self.op == "dwconv3":
            s += f"-s{self.stride}" + ("-gate" if self.gate else "")
        if self.op not in ("conv_bf16", "conv2d_nhwc", "resnet_stem"):
            s += f"-{self.xdt}-{self.ydt}" + (f"-ld{self.ldy}" if self.ldy else "")
        return s

    @property
    def data(self) -> str:
        return self.family if self.family in ("exact", "cancel", "offset") else "gauss"


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def out_hw(case: Case) -> tuple[int, int]:
    H, W, s = case.H, case.W, case.stride
    if case.op == "conv_bf16":
        p = 1 if case.k == 3 else 0
        return (H + 2 * p - case.k) // s + 1, (W + 2 * p - case.k) // s + 1
    if case.op == "conv2d_nhwc":
        return (H + 2 * case.pad - case.k) // s + 1, (W + 2 * case.pad - case.k) // s + 1
    if case.op == "resnet_stem":
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    if case.op == "convnext_stem":
        return H // 4, W // 4
    if case.op == "maxvit_stem" or (case.op == "dwconv3" and s == 2):
        return (H - 2) // 2 + 1, (W - 2) // 2 + 1
    if case.op == "avgpool2x2":
        return H // 2, W // 2
    return H, W


def default_ldy(case: Case) -> int | None:
    if case.op == "dwconv7_ln":
        return case.ldy or -(-case.C // 64) * 64
    if case.op == "im2col3x3":
        return case.ldy or -(-9 * case.C // 64) * 64
    if case.op == "maxvit_stem":
        return case.ldy or case.Cout
    return None


def abi_refusal(case: Case) -> str | None:
    """The limits the C entry points answer PM_EUNSUPPORTED / PM_EINVAL to (csrc/resnet.hip, convnext.hip, maxvit.hip, conv2d.hip)."""
    H, W, C, d = case.H, case.W, case.C, case.Cout
    Ho, Wo = out_hw(case)
    if min(Ho, Wo) <= 0:
        return "empty output"
    if case.op == "conv_bf16" and (C % 64 or case.k not in (1, 3) or case.stride not in (1, 2)):
        return "conv_bf16: Cin % 64, k in (1, 3), stride in (1, 2)"
    if case.op == "dwconv7_ln" and (C % 4 or default_ldy(case) % 4 or C > 4096):
        return "dwconv7_ln: C % 4 == 0, C <= 4096"
    if case.op == "convnext_stem" and (H < 4 or W < 4 or d > 384):
        return "convnext_stem: sides >= 4, d <= 384"
    if case.op == "dwconv3" and (C % 4 or (case.stride == 2 and min(H, W) < 2)):
        return "dwconv3: C % 4 == 0, sides >= 2 at stride 2"
    if case.op == "maxvit_stem" and (min(H, W) < 2 or d > 256):
        return "maxvit_stem: sides >= 2, d <= 256"
    if case.op == "im2col3x3" and (C % 4 or default_ldy(case) % 4):
        return "im2col3x3: C % 4 == 0"
    if case.op == "avgpool2x2" and (H % 2 or W % 2 or C % 4):
        return "avgpool2x2: even sides, C % 4 == 0"
    return None


def paths(case: Case) -> set[str]:
    """The kernel paths a case reaches, derived from its shape with the launchers' own arithmetic."""
    H, W, C, N = case.H, case.W, case.C, case.N
    Ho, Wo = out_hw(case)
    t = set()
    if case.op == "conv_bf16":
        BN = 64 if case.Cout <= 64 else 128
        nk, M = case.k * case.k * C // 64, N * Ho * Wo
        t |= {f"BN{BN}", f"inst{BN}-{int(case.resid)}{int(case.act == 'relu')}", f"k{case.k}s{case.stride}"}
        t.add(f"nk{nk}" if nk <= 2 else "nk>2")
        if case.Cout % BN:
            t.add(f"clamp{BN}")
        if M in (1, 127, 128, 129):
            t.add(f"M{M}")
        t.add("st16" if case.Cout % 8 == 0 else "st8" if case.Cout % 4 == 0 else "st2")
        if case.stride == 2 and case.k == 3 and Ho * Wo < 64 and N >= 3:
            t.add("tile-spans-3-images-s2")
        if case.stride == 2 and min(H, W) <= 2:
            t.add("hw<=2-s2")
    elif case.op == "dwconv7_ln":
        SW = 8 if C <= 2048 else 4
        spr = -(-W // SW)
        sblk = max(1, min(-(-256 // (C // 4)), 8192 // (SW * C)))
        t.add(f"SW{SW}")
        if sblk == 1:
            t.add("sblk1")
        if sblk * SW * C * 4 == 65536:
            t.add("lds64k")
        if sblk > spr * H and N > 1:
            t.add("strips-cross-images")
        for cond, tag in ((W < 4, "W<4"), (W == 1, "W1"), (W == 8, "W8"), (H == 1, "H1")):
            if cond:
                t.add(tag)
    elif case.op in ("maxvit_stem", "convnext_stem"):
        t.add(f"NCH{-(-case.Cout // 64)}")
        if case.Cout % 64 and case.Cout > 64:
            t.add("ragged-multi-block")
        if case.ldy and case.ldy > case.Cout:
            t.add("ldy>d")
    elif case.op == "dwconv3":
        t.add(f"s{case.stride}")
        for cond, tag in ((C == 4, "C4"), (W == 1, "W1"), (H == 1, "H1"), (Ho * Wo == 1, "one-pixel"), (Ho == 1, "one-row")):
            if cond:
                t.add(f"{tag}-s{case.stride}")
    elif case.op == "resnet_stem":
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if H < 7 or W < 7:
            t.add("window>image")
        if Hc == 1 and Wc == 1:
            t.add("pool-1x1-map")
        elif Hc == 1 or Wc == 1:
            t.add("pool-1xk-map")
    elif case.op == "conv2d_nhwc":
        cg = C // case.groups
        t.add("vec" if cg % 8 == 0 and C % 8 == 0 else "scalar")
        t.add("depthwise" if case.groups == C else f"groups{case.groups}")
        t |= {f"act-{case.act}", f"k{case.k}s{case.stride}"}
        if case.resid:
            t.add("resid")
    return t


REQUIRED_PATHS = {
    "conv_bf16": {"BN64", "BN128", "clamp64", "clamp128", "nk1", "nk2", "nk>2", "M1", "M127", "M128", "M129", "st16", "st8", "st2",
                  "tile-spans-3-images-s2", "hw<=2-s2", "k1s1", "k1s2", "k3s1", "k3s2"}
    | {f"inst{bn}-{r}{a}" for bn in (64, 128) for r in (0, 1) for a in (0, 1)},
    "dwconv7_ln": {"SW4", "SW8", "sblk1", "lds64k", "strips-cross-images", "W<4", "W1", "W8", "H1"},
    "maxvit_stem": {"NCH1", "NCH2", "NCH4", "ragged-multi-block", "ldy>d"},
    "convnext_stem": {"NCH1", "NCH2", "NCH6", "ragged-multi-block"},
    "dwconv3": {"s1", "s2", "C4-s1", "W1-s1", "H1-s1", "one-pixel-s1", "one-pixel-s2", "one-row-s2"},
    "resnet_stem": {"window>image", "pool-1x1-map", "pool-1xk-map"},
    "conv2d_nhwc": {"scalar", "vec", "depthwise", "groups2", "groups1", "act-none", "act-relu", "act-silu", "resid", "k3s1", "k3s2"},
}


def _cases() -> list[Case]:
    L: list[Case] = []

    def add(fams, op, N, H, W, C, **kw):
        for f in fams:
            if f == "batch" and N == 1:
                continue
            if f == "exact" and kw.get("act") == "silu":
                continue
            if f == "offset" and (kw.get("Cout") or C) > 96:
                continue
            L.append(Case(op, f, N, H, W, C, **kw))

    dense = ("exact", "cancel", "poison", "batch")
    # ---- conv_bf16: N, H, W, Cin, Cout, k, stride, bias, resid, relu
    for (N, H, W, Cin, Cout, k, s, b, r, relu) in (
        (1, 1, 1, 64, 64, 1, 1, True, False, False),     # M = 1, nk = 1, BN 64 <0, 0>
        (1, 1, 127, 64, 8, 1, 1, True, True, True),      # M = 127, Cout 8: clamped rows at BN 64 <1, 1>
        (1, 8, 16, 128, 24, 1, 1, True, True, False),    # M = 128, nk = 2, Cout 24 <1, 0>
        (2, 3, 2, 64, 40, 3, 2, True, False, True),      # Cout 40 at BN 64 <0, 1>, 3 x 2 at stride 2
        (1, 3, 43, 64, 65, 3, 1, True, False, True),     # M = 129, Cout 65: scalar stores, BN 128 <0, 1>
        (3, 10, 19, 64, 68, 3, 2, True, True, True),     # Ho Wo = 50: tile 0 spans three images; 8-byte stores <1, 1>
        (2, 5, 4, 128, 72, 1, 2, False, True, False),    # 1 x 1 stride 2 (the shortcut), no bias, Cout % 16 = 8 <1, 0>
        (1, 2, 2, 192, 128, 3, 2, True, False, False),   # 2 x 2 at stride 2: one output pixel; Cout = BN <0, 0>
        (1, 3, 1, 64, 130, 3, 2, True, True, True),      # W = 1 at stride 2; scalar stores with a residual, two column tiles
        (2, 1, 3, 64, 132, 3, 2, True, False, True),     # H = 1 at stride 2; 8-byte stores in the second column tile
        (1, 2, 3, 128, 136, 3, 1, True, True, False),    # even / odd sides at stride 1
        (1, 7, 6, 192, 200, 3, 1, True, True, True),     # nk = 27, Cout 200
        (2, 8, 8, 64, 72, 3, 1, True, False, False),     # M = 128 at BN 128, a tile over two images
    ):
        add(dense, "conv_bf16", N, H, W, Cin, Cout=Cout, k=k, stride=s, bias=b, resid=r, act="relu" if relu else "none")
    # ---- conv2d_nhwc: N, H, W, Cin, Cout, stride, groups, act, resid
    for (N, H, W, Cin, Cout, s, g, act, r) in (
        (2, 9, 8, 3, 16, 2, 1, "silu", False),           # Cin = 3: the scalar path, MobileViT's stem
        (2, 5, 6, 3, 10, 1, 1, "relu", True),
        (1, 7, 5, 16, 16, 1, 16, "relu", True),          # depthwise
        (2, 6, 7, 16, 24, 2, 2, "none", True),           # groups = 2, cin_g = 8: 16-byte loads
        (1, 5, 5, 8, 12, 1, 1, "silu", True),
        (2, 4, 3, 24, 24, 2, 24, "silu", False),         # depthwise, stride 2
        (3, 2, 2, 8, 20, 2, 1, "none", False),           # 2 x 2 at stride 2
    ):
        add(dense, "conv2d_nhwc", N, H, W, Cin, Cout=Cout, k=3, stride=s, pad=1, groups=g, act=act, resid=r)
    # ---- resnet_stem
    for (H, W) in ((1, 1), (2, 3), (5, 5), (8, 9), (33, 18)):
        add(dense, "resnet_stem", 2, H, W, 3, Cout=64, k=7, stride=2, xdt="f32")
    # ---- dwconv7_ln: the four dtype pairs spread over the cases
    ln = ("cancel", "offset", "poison", "batch")
    for (C, H, W, N, xdt, ydt) in (
        (4, 5, 17, 3, "f32", "f32"), (4, 2, 9, 3, "bf16", "bf16"), (8, 1, 1, 1, "f32", "bf16"), (8, 7, 7, 3, "bf16", "f32"),
        (40, 3, 3, 3, "f32", "f32"), (40, 1, 8, 1, "bf16", "bf16"), (96, 2, 9, 3, "bf16", "f32"), (96, 7, 7, 1, "f32", "bf16"),
        (1028, 3, 3, 1, "f32", "f32"), (2048, 1, 8, 3, "bf16", "bf16"), (2052, 2, 9, 1, "f32", "bf16"),
        (4096, 5, 17, 3, "bf16", "f32"), (4096, 1, 1, 1, "f32", "f32"),
    ):
        add(ln, "dwconv7_ln", N, H, W, C, k=7, groups=C, xdt=xdt, ydt=ydt)
    # ---- convnext_stem
    for (d, H, W, ydt) in ((1, 4, 4, "f32"), (45, 8, 36, "f32"), (64, 4, 4, "bf16"), (65, 8, 36, "bf16"), (352, 4, 4, "f32"),
                           (352, 8, 36, "bf16")):
        add(ln, "convnext_stem", 2, H, W, 3, Cout=d, k=4, stride=4, xdt="f32", ydt=ydt)
    # ---- dwconv3_bn_act
    act3 = ("cancel", "poison", "batch")
    for (C, H, W, s, xdt, gate) in (
        (4, 1, 1, 1, "f32", False), (4, 7, 7, 1, "bf16", True), (40, 1, 5, 1, "bf16", False), (40, 5, 1, 1, "f32", True),
        (256, 7, 7, 1, "f32", False), (256, 1, 1, 1, "bf16", True),
        (4, 2, 2, 2, "bf16", True), (40, 3, 2, 2, "f32", False), (256, 9, 13, 2, "bf16", False), (40, 14, 15, 2, "f32", True),
    ):
        add(act3, "dwconv3", 2, H, W, C, k=3, stride=s, groups=C, xdt=xdt, ydt=xdt, gate=gate)
    # ---- maxvit_stem
    for (d, H, W, ydt, ldy) in ((1, 2, 2, "f32", None), (32, 3, 5, "f32", 64), (65, 30, 17, "f32", None), (96, 2, 2, "bf16", None),
                                (128, 3, 5, "f32", None), (200, 30, 17, "bf16", 256), (256, 3, 5, "f32", None),
                                (256, 30, 17, "bf16", None)):
        add(act3, "maxvit_stem", 2, H, W, 3, Cout=d, k=3, stride=2, xdt="f32", ydt=ydt, ldy=ldy)
    # ---- im2col3x3 / avgpool2x2
    copy = ("exact", "poison", "batch")
    for (N, H, W, C, xdt, ydt, ldy) in ((2, 3, 5, 4, "f32", "f32", None), (1, 1, 1, 8, "bf16", "bf16", None),
                                        (2, 4, 3, 12, "f32", "bf16", 128), (2, 2, 1, 16, "bf16", "f32", None)):
        add(copy, "im2col3x3", N, H, W, C, xdt=xdt, ydt=ydt, ldy=ldy)
    for (N, H, W, C, xdt, ydt) in ((2, 2, 2, 4, "f32", "f32"), (2, 6, 4, 12, "f32", "bf16"), (3, 4, 10, 72, "bf16", "bf16")):
        add(copy, "avgpool2x2", N, H, W, C, k=2, stride=2, xdt=xdt, ydt=ydt)
    return L


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


# --------------------------------------------------------------------------------------------------------------- inputs
def _round(t: torch.Tensor, dt: str) -> torch.Tensor:
    return bf16r(t) if dt == "bf16" else t.float()


def _filter_shape(case: Case) -> tuple[int, int, int, int]:
    """(Cout, kh, kw, Cin / groups) of the generic form."""
    if case.op in ("dwconv7_ln", "dwconv3"):
        return case.C, case.k, case.k, 1
    if case.op in ("conv_bf16", "conv2d_nhwc"):
        return case.Cout, case.k, case.k, case.C // case.groups
    return case.Cout, case.k, case.k, 3


def build(case: Case) -> dict:
    """CPU fp32 tensors holding exactly the values the kernel sees.  x is NHWC (the stems' images too: to_device() lays them out
    as NCHW), w the generic (Cout, kh, kw, Cin / groups) filter (to_device() derives each kernel's own layout)."""
    g = torch.Generator().manual_seed(_seed(case))
    N, H, W, C = case.N, case.H, case.W, case.C
    Ho, Wo = out_hw(case)
    wdt = "bf16" if case.op in ("conv_bf16", "conv2d_nhwc") else "f32"
    randn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    out = {}
    if case.op in ("im2col3x3", "avgpool2x2"):
        out["x"] = ints(-3, 3, N, H, W, C) if case.data == "exact" else _round(randn(N, H, W, C), case.xdt)
        return out
    fs = _filter_shape(case)
    Cout, K = fs[0], fs[1] * fs[2] * fs[3]
    if case.data == "exact":
        density = min(0.5, 600.0 / K)  # sum of K terms of variance 16 density: sigma <= 98, so |want| <= 256 on > 98 % of the outputs
        out["x"] = ints(-3, 3, N, H, W, C) * (torch.rand(N, H, W, C, generator=g) < density)
        out["w"] = ints(-3, 3, *fs)
        out["bias"] = ints(-8, 8, Cout) if case.bias else None
        out["resid"] = ints(-8, 8, N, Ho, Wo, Cout) if case.resid else None
        return out
    if case.data == "cancel":
        # x = offset + a slow ramp + noise of 1 / 64 of it; zero-sum filters: interior outputs see only the ramp and the noise
        ramp = torch.linspace(0, 0.25, max(W, 2))[:W].view(1, 1, W, 1) + torch.linspace(0, 0.25, max(H, 2))[:H].view(1, H, 1, 1)
        out["x"] = _round(4.0 + ramp + randn(N, H, W, C) / 16, case.xdt)
        w = randn(*fs)
        w = (w - w.mean((1, 2, 3), keepdim=True)) * K ** -0.5 * 2
        out["w"] = _round(w, wdt)
    else:
        out["x"] = _round(randn(N, H, W, C), case.xdt)
        out["w"] = _round(randn(*fs) * K ** -0.5 * (0.05 if case.data == "offset" else 1.0), wdt)
    if case.op in ("conv_bf16", "conv2d_nhwc"):
        out["bias"] = randn(Cout) * 0.5 if case.bias else None
        out["resid"] = bf16r(randn(N, Ho, Wo, Cout)) if case.resid else None
    elif case.op in LN_OPS:
        b = randn(Cout)
        if case.data == "offset":  # unit spread around 4096: the convolution adds ~ 0.05 to it
            b = (b - b.mean()) / b.std(unbiased=False).clamp_min(1e-3) + OFFSET_RATIO if Cout > 1 else b + OFFSET_RATIO
        out["bias"] = b.float()
        out["gamma"] = 1.0 + 0.5 * randn(Cout)
        out["beta"] = randn(Cout)
    elif case.op == "dwconv3":
        out["scale"] = 1.0 + 0.2 * randn(Cout)
        out["shift"] = 0.1 * randn(Cout)
        out["gate"] = torch.sigmoid(randn(N, Cout)) if case.gate else None
    else:  # resnet_stem, maxvit_stem
        out["bias"] = 0.1 * randn(Cout)
    return out


# --------------------------------------------------------------------------------------------------------------- the reference
def conv_taps(x, w, stride, pads, groups=1, dtype=torch.float64, reverse=False, replicate=False):
    """Convolution as a plain loop over the taps.  x (N, H, W, Cin), w (Cout, kh, kw, Cin / groups), pads (top, left, bottom,
    right) zeros (replicate: edge values, a mutant).  Returns (z, A): sum x w and sum |x w|, (N, Ho, Wo, Cout), no bias.
    reverse: taps and channels in the opposite order (for the fp32 evaluation of the CPU test)."""
    x, w = x.to(dtype), w.to(dtype)
    N, H, W, Cin = x.shape
    Cout, kh, kw, cg = w.shape
    pt, pl, pb, pr = pads
    Ho, Wo = (H + pt + pb - kh) // stride + 1, (W + pl + pr - kw) // stride + 1
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), mode="replicate" if replicate else "constant").permute(0, 2, 3, 1)
    if reverse:
        xp, w = xp.flip(-1), w.flip(-1).reshape(groups, Cout // groups, kh, kw, cg).flip(0).reshape(Cout, kh, kw, cg)
    z = torch.zeros(N, Ho, Wo, Cout, dtype=dtype)
    A = torch.zeros_like(z)
    taps = [(i, j) for i in range(kh) for j in range(kw)]
    for (i, j) in (reversed(taps) if reverse else taps):
        xs = xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride, :].reshape(N, Ho, Wo, groups, cg)
        wt = w[:, i, j, :].reshape(groups, Cout // groups, cg)
        if cg == 1 and groups == Cout:  # depthwise
            prod = xs[..., 0] * wt[:, 0, 0]
            z += prod
            A += prod.abs()
        else:
            z += torch.einsum("nhwgc,goc->nhwgo", xs, wt).reshape(N, Ho, Wo, Cout)
            A += torch.einsum("nhwgc,goc->nhwgo", xs.abs(), wt.abs()).reshape(N, Ho, Wo, Cout)
    if reverse and groups > 1:
        z = z.reshape(N, Ho, Wo, groups, -1).flip(3).reshape(N, Ho, Wo, Cout)
        A = A.reshape(N, Ho, Wo, groups, -1).flip(3).reshape(N, Ho, Wo, Cout)
    return z, A


def geometry(case: Case) -> tuple[int, tuple[int, int, int, int], int]:
    """(stride, pads (top, left, bottom, right), groups) of the op's convolution."""
    if case.op == "conv_bf16":
        p = 1 if case.k == 3 else 0
        return case.stride, (p, p, p, p), 1
    if case.op == "conv2d_nhwc":
        return case.stride, (case.pad,) * 4, case.groups
    if case.op == "resnet_stem":
        return 2, (3, 3, 3, 3), 1
    if case.op == "dwconv7_ln":
        return 1, (3, 3, 3, 3), case.C
    if case.op == "convnext_stem":
        return 4, (0, 0, 0, 0), 1
    if case.op == "dwconv3":
        return (1, (1, 1, 1, 1), case.C) if case.stride == 1 else (2, (0, 0, 1, 1), case.C)
    if case.op == "maxvit_stem":
        return 2, (0, 0, 1, 1), 1
    raise ValueError(case.op)


def gelu_tanh(t: torch.Tensor) -> torch.Tensor:
    return 0.5 * t * (1.0 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t * t * t)))


def _tile_image(z: torch.Tensor) -> torch.Tensor:
    """Mutant: the image index of output row m is taken from row 128 (m // 128), the first row of its tile."""
    N, Ho, Wo, C = z.shape
    m = torch.arange(N * Ho * Wo)
    n_tile = (m // 128 * 128) // (Ho * Wo)
    return z.reshape(N, Ho * Wo, C)[n_tile, m % (Ho * Wo)].reshape(N, Ho, Wo, C)


def _conv(case, inp, mutant, dtype, reverse):
    stride, pads, groups = geometry(case)
    x, w = inp["x"], inp["w"]
    if mutant == "transpose":
        w = w.transpose(1, 2)
    if mutant == "chunkswap":  # chunks 0 and 1 of every 64-channel K step of the pixel operand
        idx = torch.arange(x.shape[-1]).view(-1, 8, 8)
        idx[:, [0, 1]] = idx[:, [1, 0]]
        x = x[..., idx.reshape(-1)]
    if mutant == "origin":  # symmetric pad <-> right / bottom pad: the window origin moves by the pad
        pt, pl, pb, pr = pads
        pads = (0, 0, pt + pb, pl + pr) if pt else (pb, pr, 0, 0)
    z, A = conv_taps(x, w, stride, pads, groups, dtype, reverse, replicate=mutant == "replicate")
    if mutant == "tileimg":
        z = _tile_image(z)
    return z, A


def _layer_norm(z, gamma, beta, onepass=False):
    """LayerNorm over the last dim, biased variance.  Returns (y, mean, sigma, yhat).  onepass: E[z^2] - mean^2 in fp32 (mutant)."""
    if onepass:
        z = z.float()
        mean = z.mean(-1, keepdim=True)
        var = (z * z).mean(-1, keepdim=True) - mean * mean
    else:
        mean = z.mean(-1, keepdim=True)
        var = (z - mean).square().mean(-1, keepdim=True)
    sigma = torch.sqrt(var + EPS)
    yhat = (z - mean) / sigma
    return yhat * gamma.to(z.dtype) + beta.to(z.dtype), mean, sigma, yhat


def _pad_cols(t: torch.Tensor, ldy: int | None, mutant) -> torch.Tensor:
    """(rows..., C) -> (rows..., ldy) with zeros behind (mutant padcols: never written, i.e. the NaNs that were there)."""
    if ldy is None or ldy == t.shape[-1]:
        return t
    fill = float("nan") if mutant == "padcols" else 0.0
    return torch.cat([t, torch.full((*t.shape[:-1], ldy - t.shape[-1]), fill, dtype=t.dtype)], -1)


def forward(case: Case, inp: dict, dtype=torch.float64, reverse=False, mutant=None) -> dict:
    """The op in `dtype` arithmetic: float64 = the reference; float32 with reverse=True = the CPU test's stand-in for a correct
    kernel.  Returns want (in the output's layout, pad columns included), the bound's ingredients, and for dwconv3 psum."""
    assert mutant is None or mutant in MUTANTS
    u = U32
    ldy = default_ldy(case)
    r = {}
    if case.op == "im2col3x3":
        x = inp["x"].to(dtype)
        N, H, W, C = x.shape
        xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if mutant == "replicate" else "constant").permute(0, 2, 3, 1)
        cols = torch.cat([xp[:, i:i + H, j:j + W, :] for i in range(3) for j in range(3)], -1).reshape(N * H * W, 9 * C)
        r["want"] = _pad_cols(cols, ldy, mutant)
        r["A"] = r["want"].abs()
        r["bound"] = store_term(r["want"], case.ydt) if (case.xdt, case.ydt) == ("f32", "bf16") else torch.zeros_like(r["A"].double())
        return r
    if case.op == "avgpool2x2":
        x = inp["x"].to(dtype)
        a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
        r["want"] = ((d + c) + (b + a)) * 0.25 if reverse else ((a + b) + (c + d)) * 0.25
        r["A"] = (a.abs() + b.abs() + c.abs() + d.abs()) * 0.25
        r["bound"] = 6 * u * r["A"].double() + store_term(r["want"], case.ydt)
        return r
    fs = _filter_shape(case)
    K = fs[1] * fs[2] * fs[3]
    z, A = _conv(case, inp, mutant, dtype, reverse)
    bias = inp.get("bias")
    if bias is not None:
        b = bias.to(dtype).clone()
        if mutant == "biastail" and case.Cout % 8:
            b[-(case.Cout % 8):] = 0
        z, A = z + b, A + bias.to(dtype).abs()
    if case.op == "conv_bf16":
        res = inp["resid"]
        if res is not None:
            z = F.relu(z) + res.to(dtype) if mutant == "relu_first" else z + res.to(dtype)
            A = A + res.to(dtype).abs()
        want = F.relu(z) if case.act == "relu" and not (mutant == "relu_first" and res is not None) else z
        delta = (K + 2) * u * A.double()
    elif case.op == "conv2d_nhwc":
        delta = (K + 2) * u * A.double()
        if case.act == "relu":
            z = F.relu(z)
        elif case.act == "silu":
            z = z * torch.sigmoid(z)
            delta = SILU_LIP * delta + 4 * u * z.double().abs()
        want = z
        if inp["resid"] is not None:
            want = z + inp["resid"].to(dtype)
            A = A + inp["resid"].to(dtype).abs()
            delta = delta + u * (inp["resid"].double().abs() + want.double().abs())
    elif case.op == "resnet_stem":
        conv = F.relu(z)  # the bf16 conv map; rounding is monotonic, so the pool commutes with it
        dmap = (K + 2) * u * A.double() + store_term(conv, "bf16")
        pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)  # noqa: E731
        r.update(want=pool(conv), A=pool(A), bound=pool(dmap))  # the largest bound of the window, store term included
        return r
    elif case.op in LN_OPS:
        C = z.shape[-1]
        y, mean, sigma, yhat = _layer_norm(z, inp["gamma"], inp["beta"], onepass=mutant == "onepass")
        dc = (K + 2) * u * A.double()
        e = dc.max(-1, keepdim=True).values + C * u * z.double().abs().mean(-1, keepdim=True)
        delta = inp["gamma"].double().abs() / sigma.double() * (2 + yhat.double().abs()) * e
        want = y
        r.update(z=z, mean=mean, sigma=sigma)
    elif case.op == "dwconv3":
        sc, sh = inp["scale"].to(dtype), inp["shift"].to(dtype)
        t = z * sc + sh
        dt_ = sc.double().abs() * (K + 2) * u * A.double() + u * t.double().abs()
        gl = gelu_tanh(t) if dtype == torch.float64 else F.gelu(t, approximate="tanh")
        dg = GELU_LIP * dt_ + u * (4 * t.double().abs() + 2 * gl.double().abs())
        Wo = gl.shape[2]
        r["psum"] = gl.sum(2)
        r["psum_bound"] = dg.sum(2) + (Wo - 1) * u * gl.double().abs().sum(2)
        want, delta = gl, dg
        if inp["gate"] is not None:
            gt = inp["gate"].to(dtype)[:, None, None, :]
            want = gl * gt
            delta = gt.double().abs() * dg + u * want.double().abs()
    elif case.op == "maxvit_stem":
        want = gelu_tanh(z) if dtype == torch.float64 else F.gelu(z, approximate="tanh")
        delta = GELU_LIP * (K + 2) * u * A.double() + u * (4 * z.double().abs() + 2 * want.double().abs())
    else:
        raise ValueError(case.op)
    bound = delta + store_term(want, case.ydt)
    if case.op == "dwconv7_ln":  # (N*H*W, ldy) rows
        want, bound, A = (t.reshape(-1, t.shape[-1]) for t in (want, bound, A))
    if ldy is not None:
        want, bound, A = _pad_cols(want, ldy, mutant), _pad_cols(bound, ldy, None), _pad_cols(A, ldy, None)
    r.update(want=want, A=A, bound=bound)
    return r


def reference(case: Case, inp: dict) -> dict:
    return forward(case, inp)


def emulate(case: Case, inp: dict) -> dict:
    """A correct kernel's stand-in: fp32 arithmetic, taps and channels in the opposite order, the output rounded to its dtype."""
    r = forward(case, inp, torch.float32, reverse=True)
    out = {"y": store(r["want"], case.ydt)}
    if "psum" in r:
        out["psum"] = r["psum"].float()
    return out


def mutant_output(case: Case, inp: dict, mutant: str) -> dict:
    """What a kernel with the named defect would return (float64 arithmetic otherwise, rounded to the output dtype)."""
    r = forward(case, inp, mutant=mutant)
    out = {"y": store(r["want"], case.ydt, trunc=mutant == "trunc")}
    if "psum" in r:
        out["psum"] = r["psum"].float()
    return out


def mutant_applies(case: Case, mutant: str) -> bool:
    """Whether the defect changes anything a case of this shape could see."""
    stride, pads, _ = geometry(case) if case.op not in ("im2col3x3", "avgpool2x2") else (1, (0, 0, 0, 0), 1)
    if mutant == "replicate":
        return max(pads) > 0 or case.op == "im2col3x3"
    if mutant == "origin":
        return stride == 2 and max(pads) > 0
    if mutant == "transpose":
        return case.op not in ("im2col3x3", "avgpool2x2") and case.k > 1
    if mutant == "chunkswap":
        return case.op == "conv_bf16"
    if mutant == "tileimg":
        Ho, Wo = out_hw(case)
        return case.op == "conv_bf16" and case.N > 1 and (Ho * Wo) % 128 != 0
    if mutant == "relu_first":
        return case.op == "conv_bf16" and case.resid and case.act == "relu"
    if mutant == "trunc":
        return case.ydt == "bf16" and case.family in ("poison", "batch")
    if mutant == "onepass":
        return case.op in LN_OPS and case.family == "offset"
    if mutant == "biastail":
        return case.op in ("conv_bf16", "conv2d_nhwc") and case.bias and case.Cout % 8 != 0
    if mutant == "padcols":
        ldy = default_ldy(case)
        return ldy is not None and ldy > (9 * case.C if case.op == "im2col3x3" else case.Cout or case.C)
    return False


# the family each mutant is aimed at: it must be rejected by at least one case of it (tests/test_conv_cases_cpu.py)
MUTANT_FAMILY = {"replicate": "exact", "origin": "exact", "transpose": "exact", "chunkswap": "exact", "tileimg": "exact",
                 "relu_first": "exact", "biastail": "exact", "trunc": "poison", "onepass": "offset", "padcols": "cancel"}


def accepts(case: Case, got: dict, ref: dict) -> tuple[bool, float]:
    """The GPU suite's verdict on an output: exact family -> equality with want.to(out dtype), else ratio <= MARGIN (y and psum)."""
    if case.family == "exact":
        ok = got["y"].dtype == DT[case.ydt] and torch.equal(got["y"], store(ref["want"], case.ydt))
        return ok, 0.0 if ok else float("inf")
    rt = ratio(got["y"], ref["want"], ref["bound"])
    if "psum" in got and got["psum"] is not None:
        rt = max(rt, ratio(got["psum"], ref["psum"], ref["psum_bound"]))
    return rt <= MARGIN, rt


def exact_fraction(case: Case, ref: dict) -> float:
    """Fraction of a case's outputs with |want| <= 256 (integers exact in bf16)."""
    return float((ref["want"].abs() <= 256).double().mean())


# --------------------------------------------------------------------------------------------------------------- running a case
STEMS = ("resnet_stem", "convnext_stem", "maxvit_stem")


def poisoned(t: torch.Tensor, dev) -> torch.Tensor:
    """t as the middle slice of a NaN-filled contiguous buffer with (at least) one extra image on each side; the guard is a
    multiple of 16 elements, so the slice keeps the buffer's 16-byte alignment."""
    guard = -(-max(t.numel() // max(t.shape[0], 1), 1) // 16) * 16
    buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device=dev)
    out = buf[guard:guard + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all())
    return out


def to_device(case: Case, inp: dict, dev, poison: bool = False) -> dict:
    """The operands in each kernel's own dtype and layout on `dev`: NCHW f32 images and (taps, d) weights for the stems, (k, k, C)
    f32 filters for the depthwise kernels, bf16 NHWC / (Cout, k, k, Cin / g) for the dense ones."""
    place = (lambda v: poisoned(v, dev)) if poison else (lambda v: v.to(dev).clone())
    t = {}
    if case.op in STEMS:
        t["x"] = place(inp["x"].permute(0, 3, 1, 2).contiguous())
        t["w"] = place(inp["w"].permute(0, 3, 1, 2).reshape(case.Cout, -1).t().contiguous())
    elif case.op in ("dwconv7_ln", "dwconv3"):
        t["x"] = place(inp["x"].to(DT[case.xdt]))
        t["w"] = place(inp["w"][..., 0].permute(1, 2, 0).contiguous())
    elif case.op in ("conv_bf16", "conv2d_nhwc"):
        t["x"], t["w"] = place(inp["x"].bfloat16()), place(inp["w"].bfloat16())
    else:
        t["x"] = place(inp["x"].to(DT[case.xdt]))
    for k in ("bias", "resid", "gamma", "beta", "scale", "shift", "gate"):
        if inp.get(k) is not None:
            t[k] = place(inp[k].bfloat16() if k == "resid" else inp[k].float().contiguous())
    return t


def run(ops, case: Case, t: dict) -> dict:
    """One launch through pytorch_models._hip.ops.  Returns {"y": ..., "psum": ..., "psum_only": ...} (the last two: dwconv3)."""
    ydt = DT[case.ydt]
    if case.op == "conv_bf16":
        return {"y": ops.conv_bf16(t["x"], t["w"], t.get("bias"), case.stride, relu=case.act == "relu", resid=t.get("resid"))}
    if case.op == "conv2d_nhwc":
        return {"y": ops.conv2d_nhwc(t["x"], t["w"], t.get("bias"), case.stride, case.pad, case.groups, case.act, t.get("resid"))}
    if case.op == "resnet_stem":
        return {"y": ops.resnet_stem(t["x"], t["w"], t["bias"])}
    if case.op == "dwconv7_ln":
        return {"y": ops.dwconv7_ln(t["x"], t["w"], t["bias"], t["gamma"], t["beta"], EPS, ydt, ldy=case.ldy)}
    if case.op == "convnext_stem":
        return {"y": ops.convnext_stem(t["x"], t["w"], t["bias"], t["gamma"], t["beta"], EPS, ydt)}
    if case.op == "dwconv3":
        y, ps = ops.dwconv3_bn_act(t["x"], t["w"], t["scale"], t["shift"], case.stride, gate=t.get("gate"), out_dtype=ydt, want_psum=True)
        only = ops.dwconv3_bn_act(t["x"], t["w"], t["scale"], t["shift"], case.stride, want_psum=True, write_y=False)
        return {"y": y, "psum": ps, "psum_only": only}
    if case.op == "maxvit_stem":
        return {"y": ops.maxvit_stem(t["x"], t["w"], t["bias"], ydt, ldy=case.ldy)}
    if case.op == "im2col3x3":
        return {"y": ops.im2col3x3(t["x"], ydt, ldy=case.ldy)}
    if case.op == "avgpool2x2":
        return {"y": ops.avgpool2x2(t["x"], ydt)}
    raise ValueError(case.op)


def out_shape(case: Case) -> tuple[int, ...]:
    Ho, Wo = out_hw(case)
    if case.op in ("dwconv7_ln", "im2col3x3"):
        return case.N * case.H * case.W, default_ldy(case)
    if case.op == "maxvit_stem":
        return case.N, Ho, Wo, default_ldy(case)
    return case.N, Ho, Wo, case.Cout or case.C


def image(case: Case, inp: dict, n: int) -> tuple[Case, dict]:
    """The single-image problem of image n (batch family)."""
    one = {k: (v[n:n + 1].clone() if k in ("x", "resid", "gate") and v is not None else v) for k, v in inp.items()}
    return Case(**{**case.__dict__, "N": 1}), one


def rows_of_image(case: Case, y: torch.Tensor, n: int) -> torch.Tensor:
    return y.reshape(case.N, -1)[n]
