"""References, error bounds, adversarial input families and case lists shared by the EnCodec kernel parity tests
(tests/test_encodec_cases_cpu.py without a GPU, tests/test_hip_encodec_adversarial.py on one).  A plain helper module.

In scope (through pytorch_models._hip.ops, the poison family through the C ABI): conv1d_f32 in its plain and its transposed form,
lstm_f32 (one, two - wavefront and plain - and three layers, residual), rvq_encode, rvq_decode, groupnorm1_, encodec_scale,
scale_clips.  The model-level tests (fixtures of the reference's own outputs) stay in tests/test_hip_encodec.py.

Contract ("2f. EnCodec numerics contract").

Reference.  Float64 on the CPU from exactly the fp32 operands the kernel sees, in the order read off csrc/encodec.hip.
  conv        source frame of row m, tap j: f = m stride - left + j, mirrored ONCE by index arithmetic (f < 0 -> -f, f >= Tin ->
              2 (Tin - 1) - f) or, zero_pad, dropped: left / right up to Tin - 1 and the transposed form are one code path
              (conv_forward).  ELU on the operand, then the taps, bias, residual.  Column n of the (Mr, up Cout) product is channel
              n % Cout of output frame m up + n / Cout - trim.  The transposed form's matrix is written from the header's formula,
              w[r Cout + co][j Cin + ci] = weight[ci][co][r + (1 - j) s] (convt_matrix), and checked on the CPU against
              F.conv_transpose1d + trim in float64.
  lstm        TEACHER-FORCED per step, so that no bound grows with |W_hh|^T: step t of a layer takes the KERNEL'S OWN h_(t-1) (fp32,
              widened) and the layer's input row and keeps its own float64 c; it returns h_t and a propagated bound (below).  The
              last layer of a call is checked against that; its input rows come from single-layer calls of the layers below, each
              checked the same way (lstm_verify): two layers - wavefront and plain held to the SAME reference - feed layer 1 the
              single-layer run's h0 and the call's own y_(t-1); three layers are the composition.  residual: y must EQUAL
              x + (the same call without it), one fp32 addition.
  rvq_encode  d = norms - 2 r.e in float64 from the fp32 norms the kernel is given; code = the LOWEST index of the minimum, found
              explicitly (no reliance on argmin's tie rule); r -= e in fp32, as the kernel does.
  rvq_decode  sequential fp32 additions in stage order, indices clamped into the codebook: bit-equal.
  groupnorm   mean and biased variance over the whole clip, eps inside the root, per-channel affine (channel = index % C), + resid.
  scale       sqrt(mean_t(mean_c(x)^2)) + 1e-8;  scale_clips: x / s or x s with the fp32 s the kernel is given.

Bounds.  u = 2^-24, no number measured on a kernel enters one.  expm1f, expf and tanhf are taken to be within 2 ulp (4 u relative),
the convention of 2c; TINY = 2^-126 is added wherever a result may fall below fp32's normal range (sigmoid(-100) is 3.7e-44 in
float64 and 0 after expf overflowed).
  * fp32 accumulation of K terms in any order: (K + 2) u A, A = sum |x w| + |bias| + |resid| (2c); the f32 store u |want|.
  * conv: K = k Cin.  ELU on load gives each product a relative 3 u more: + 3 u sum |elu(x) w|.
  * sigmoid s(z) = 1 / (1 + exp(-z)): delta_s = 0.25 delta_z + 4 u s + TINY (sup s' = 1 / 4; expf, the add, the division: as 2c
    writes SiLU);  tanh: delta = delta_z + 4 u |tanh z| + TINY.
  * lstm pre-activation: K = 2 H terms (input and recurrent part, whichever kernel sums them), delta_z = (2 H + 4) u A; in the
    onehot and saturate families every pre-activation is ONE exact product and delta_z = 0.  Cell: local(t) = |c_(t-1)| delta_f +
    |g| delta_i + i delta_g + 2 u |c_t| + TINY, e_c(t) = f e_c(t-1) + local(t);  e_h(t) = o (e_c(t) + 4 u |tanh c| + TINY) +
    |tanh c| delta_o + u |h| + TINY (the products may underflow too).
  * rvq_encode: delta_j = (128 + 2) u (|norm_j| + 2 sum |r e_j|).  A decision is DECIDED when min over j != best of (d_j - m delta_j)
    exceeds d_best + m delta_best (m = MARGIN on the GPU): a correct kernel cannot choose otherwise.  In every row the first stage at
    which the codes differ from the reference must be an undecided one; later stages of that row are exempt (the rule of
    tests/test_hip_encodec.py with e = 0 and this threshold).  The exact family has delta = 0: every code must EQUAL.
  * groupnorm: the two-pass form of 2c's LayerNorm term.  e = u |mean| + (64 + 2) u sqrt(var): the fp32 mu the apply pass subtracts,
    and per-thread fp32 sums of at most 64 CENTRED values (everything above them in fp64).  |dy| <= |gamma| / sigma (2 + |yhat|) e +
    3 u |gamma yhat| + u |y| (+ u (|resid| + |want|)) + the store.  No (mean / sigma)^2 term: a kernel that needs one fails.
  * scale: delta = sum_t 2 |m_t| (C + 1) u mean_c |x| / (2 T s) + 3 u s + u |want|;  scale_clips: u |want| (one rounding).
The GPU suite asserts MARGIN = 1.5 x the bound, the CPU stand-in 1.0 x; an element whose bound is 0 must be exact (ratio()).

Families.
  exact     conv: integer operands, every partial sum below 2^24, the output must EQUAL want; with elu=True x >= 0, where ELU is the
            identity (an ELU applied to the wrong thing still shows).  Sub-family ramp: x[b, t, c] = (b Tin + t) Cin + c and one-hot
            weight rows, so that every output NAMES the clip, frame and channel it was read from (mirror and tap indexing).
            rvq_encode: integer codebooks in [-3, 3], integer latents, planted duplicates: exact integer distances, ties at every
            stage, codes EQUAL.  rvq_decode: bit-equal, also from a non-contiguous (B, n_q, T) view and with indices -1, 1024, 2^40.
            groupnorm: a constant integer clip gives beta (+ resid) exactly.  scale: an all-zero clip gives float32(1e-8), x / s = 0.
  onehot    lstm: W_ih, W_hh signed permutations with disjoint rows, bias 0: the output is held by the gate terms alone, a wrong k,
            wave range or batch row is a gross error.
  saturate  lstm: the same with x = +-1 and weights of +-100 (layer 0's W_ih) and +-128 (all others: 100 h would not be an exact
            product, and exp turns an absolute error of the argument into a relative one): pre-activations of +-100 and beyond, where
            expf overflows; the output must be finite and inside the bound.
  cancel    conv: zero-sum weight rows on an offset of 4 plus noise.
  offset    groupnorm at |mean| / sigma = 4096.
  small     groupnorm with sigma = 0.01 (var = 10 eps: where eps sits matters).
  gaussian  rvq_encode by the decided rule, with planted pairs whose float64 margin is 4 x the threshold (must match) and 0.25 x
            (exempt), at a norm difference that only the fp32 norms carry.
  poison    Gaussian operands; on the GPU a second launch through lib() with every operand the middle of a NaN-filled 16-byte
            aligned buffer (conv: a NaN gap between clips, x_batch_stride > Tin Cin), the output the middle of a sentinel-filled
            buffer, the LSTM / GroupNorm workspace NaN-filled: finite, bit-identical to the plain run, every sentinel intact.
  batch     Gaussian operands, B > 1: row / clip b of the batch run is bit-identical to its run alone.

Path -> case (the smallest shapes that reach each path; paths() derives the tags with the launchers' own arithmetic):
  conv   NT 1 / 2 / 4 / 8 (N <= 16, 32, 64, more)                  conv-*-b1-t128-12x16 / -t7-2x32 / -t386-20x64 / -t257-16x132
         two N tiles, ragged last: 16-byte / scalar stores          -t257-16x132 / -b3-t33-64x130
         element-wise gather (Cin 1, 2, 3)                          -t4-1x2-k7 (K 7), -t7-2x32, -t40-3x3-k7 (K 21)
         vector gather, a tap changing inside a K step (4, 12, 20)  -t253-4x20, -t128-12x16 and -t5-12x4, -t386-20x64
         K % 16 = 4 / 8 / 12, nk 1 / 2 / > 2                        -12x16-k3 / -12x4-k2 / -4x20-k7;  -16x132-k1 / -4x20-k7 / -64x130
         Mr 1, 2, 127, 128, 129, 257                                -t1-1x1, -t3-4x8, -t253-4x20, -t128-12x16, -t386-20x64, -t257
         stride 2, 3, 5, 8 with -T % stride != 0                    -t253-4x20-k7s2, -t386-..s3, -b3-t33-..s5, -t21-8x12-k16s8
         left = Tin - 1 / right = Tin - 1 / mirrored on both sides  -t7-2x32-k7 (6 + 0) / -t5-12x4-k2 (0 + 4) / -t4-1x2-k7 (3 + 3)
  convT  (s, Cout) = (2, 4), (8, 20), (5, 3)                        convT-*-t5-4x4-s2, -t7-16x20-s8 and -t130-16x20-s8, -t9-8x3-s5
         trim 0 / > 0, Tout short, the untrimmed (T + 1) s form     -t7-16x20-s8 (untrimmed) / the others; -t5-4x4-s2-o10 is short
  lstm   kq = H / 4 = 16, 32, 48 (partial group), 128, 144          lstm-*-h64, -h128, -h192, -h512, -h576
         one layer, wavefront, plain, three layers (hbuf[l & 1])    -l1, -l2, -l2-plain, -l3
         B 1, 15, 16, 17, 33 (one, a ragged and three batch tiles)  -b1, -b15, -b16, -b17, -b33
  rvq    M 1, 15, 16, 17, 33; n_q 1, 2, 32                          rvq_encode-*-m1-q1 ... -m33-q32
         duplicates inside a lane's four entries, across fq, tiles, waves: every stage of every exact case holds pairs of all four
         kinds (rvq_twin); stage 0 has the sets 0 / 1 / 4 / 16 / 767 / 1023 (row 0, every M) and 255 / 256 (row 2: the last entry
         of wave 0 against the first of wave 1); a stage > 0: row 4 of the n_q > 1 cases
  gn     256 % C != 0 (C 3, 48, 96, 320), n = C, n around a chunk, > 256 chunks   groupnorm-*-c3-t1, -c32-t511/512/513, -c32-t131200
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

from conv_cases import MARGIN, U32, ratio, store_term  # noqa: F401  (one definition of each)

TINY = 2.0 ** -126
EPS = 1e-5
OFFSET_RATIO = 4096.0
GN_CHUNK, GN_PER = 16384, 64     # csrc/encodec.hip: floats per workgroup, per thread
CBM, CBK = 128, 16               # csrc/encodec.hip: rows of a convolution tile, its K step
RVQ_D, RVQ_N = 128, 1024
SENTINEL = 0x4B4B4B4B            # int32 pattern of every f32 output guard (1.33e7: finite, so a read of it would not show as NaN;
SENTINEL64 = 0x4B4B4B4B4B4B4B4B  # the bit comparison with the plain run shows it)

OPS = ("conv", "convT", "lstm", "rvq_encode", "rvq_decode", "groupnorm", "scale")
MUTANTS = ("mirror_edge", "replicate", "extra_pad_zero", "elu_after", "tap_carry", "clip_cross", "up_phase_swap", "trim_shift",
           "bias_lane", "gate_order", "stale_acc", "c_not_reset", "row_clamp", "tie_highest", "wave_tie", "no_norm", "resid_stale",
           "onepass", "var_unbiased", "chan_step", "eps_outside", "square_first")
# the op group and the family each mutant is aimed at: it must be rejected by at least one case of them
MUTANT_OP = {**dict.fromkeys(("mirror_edge", "replicate", "extra_pad_zero", "elu_after", "tap_carry", "clip_cross", "bias_lane"), "conv"),
             "up_phase_swap": "convT", "trim_shift": "convT",
             **dict.fromkeys(("gate_order", "stale_acc", "c_not_reset", "row_clamp"), "lstm"),
             **dict.fromkeys(("tie_highest", "wave_tie", "no_norm", "resid_stale"), "rvq_encode"),
             **dict.fromkeys(("onepass", "var_unbiased", "chan_step", "eps_outside"), "groupnorm"), "square_first": "scale"}
MUTANT_FAMILY = {"mirror_edge": "exact", "replicate": "exact", "extra_pad_zero": "exact", "elu_after": "exact", "tap_carry": "exact",
                 "clip_cross": "exact", "up_phase_swap": "exact", "trim_shift": "exact", "bias_lane": "exact",
                 "gate_order": "onehot", "stale_acc": "poison", "c_not_reset": "onehot", "row_clamp": "onehot",
                 "tie_highest": "exact", "wave_tie": "exact", "no_norm": "gaussian", "resid_stale": "exact",
                 "onepass": "offset", "var_unbiased": "poison", "chan_step": "poison", "eps_outside": "small", "square_first": "poison"}


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    """One problem.  T: input frames (conv, convT, lstm, groupnorm), rows M (rvq_encode), frames (rvq_decode), samples (scale).
    C: input channels (conv), hidden size (lstm), channels (groupnorm, scale).  stride: the transposed form's s = up."""
    op: str
    family: str
    B: int
    T: int
    C: int = 0
    Cout: int = 0
    k: int = 1
    stride: int = 1
    left: int = 0
    right: int = 0
    elu: bool = False
    bias: bool = True
    resid: bool = False
    trim: int = 0
    t_out: int = 0       # convT: output frames (0: Mr up - trim)
    layers: int = 1
    plain: bool = False
    nq: int = 1
    sub: str = ""        # "ramp" (conv exact), "view" (rvq_decode: a non-contiguous codes view)

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.family}{'-' + self.sub if self.sub else ''}-b{self.B}-t{self.T}"
        if self.op == "conv":
            s += f"-{self.C}x{self.Cout}-k{self.k}s{self.stride}-p{self.left}+{self.right}"
        elif self.op == "convT":
            s += f"-{self.C}x{self.Cout}-s{self.stride}-trim{self.trim}" + (f"-o{self.t_out}" if self.t_out else "")
        elif self.op == "lstm":
            return f"lstm-{self.family}-b{self.B}-t{self.T}-h{self.C}-l{self.layers}" + ("-plain" if self.plain else "") + ("-r" if self.resid else "")
        elif self.op in ("rvq_encode", "rvq_decode"):
            return f"{self.op}-{self.family}{'-' + self.sub if self.sub else ''}-" + (f"m{self.T}" if self.op == "rvq_encode" else f"b{self.B}-t{self.T}") + f"-q{self.nq}"
        else:
            return s + f"-c{self.C}" + ("-r" if self.resid else "")
        return s + ("-elu" if self.elu else "") + ("" if self.bias else "-nobias") + ("-r" if self.resid else "")

    @property
    def up(self) -> int:
        return self.stride if self.op == "convT" else 1


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def conv_geometry(case: Case) -> dict:
    """The arguments pm_conv1d_f32 gets: the transposed form is k = 2, stride = 1, one zero frame on each side, up = s."""
    if case.op == "convT":
        k, stride, left, right, zero = 2, 1, 1, 1, True
    else:
        k, stride, left, right, zero = case.k, case.stride, case.left, case.right, False
    Mr = (case.T + left + right - k) // stride + 1
    Tout = case.t_out or Mr * case.up - case.trim
    return dict(k=k, stride=stride, left=left, right=right, zero_pad=zero, up=case.up, trim=case.trim, Mr=Mr, Tout=Tout,
                N=case.up * case.Cout, K=k * case.C)


def conv_nt(N: int) -> int:
    return 1 if N <= 16 else 2 if N <= 32 else 4 if N <= 64 else 8


def abi_refusal(case: Case) -> str | None:
    """The limits the C entry points answer PM_EINVAL / PM_EUNSUPPORTED to (csrc/encodec.hip)."""
    if case.op in ("conv", "convT"):
        g = conv_geometry(case)
        if case.T + g["left"] + g["right"] < g["k"]:
            return "conv: the padded clip is shorter than the kernel"
        if not g["zero_pad"] and (g["left"] >= case.T or g["right"] >= case.T):
            return "conv: one reflection only"
        if g["trim"] + g["Tout"] > g["Mr"] * g["up"] or g["Tout"] < 1:
            return "conv: every frame of y must be written"
        if case.resid and (g["up"] != 1 or g["trim"]):
            return "conv: residual with the plain form only"
    if case.op == "lstm" and (case.C < 64 or case.C % 64):
        return "lstm: H % 64 == 0"
    return None


def paths(case: Case) -> set[str]:
    """The kernel paths a case reaches, derived from its shape with the launchers' own arithmetic."""
    t = set()
    if case.op in ("conv", "convT"):
        g = conv_geometry(case)
        N, K, Mr, Cin, Cout = g["N"], g["K"], g["Mr"], case.C, case.Cout
        nt = conv_nt(N)
        nk = -(-K // CBK)
        t |= {f"NT{nt}", "st4" if Cout % 4 == 0 else "st1", "vec" if Cin % 4 == 0 else "elem", f"nk{nk}" if nk <= 2 else "nk>2",
              f"B{case.B}", f"Cin{Cin}"}
        if -(-N // (16 * nt)) > 1 and N % (16 * nt):
            t.add("ragged-N-tile-" + ("st4" if Cout % 4 == 0 else "st1"))
        if Cin % 4 == 0 and Cin % CBK:
            t.add("tap-in-kstep")
        if K % CBK:
            t.add(f"Kmod{K % CBK}")
        if K in (7, 21):
            t.add(f"K{K}")
        if Mr in (1, 2, 127, 128, 129, 257):
            t.add(f"Mr{Mr}")
        if -(-Mr // CBM) > 1:
            t.add("M-tiles>1")
        if case.op == "conv":
            t.add(f"s{case.stride}" + ("-extra" if case.stride > 1 and -case.T % case.stride else ""))
            if case.left == case.T - 1 and case.T > 1:
                t.add("left-max")
            if case.right == case.T - 1 and case.T > 1:
                t.add("right-max")
            if any(m * case.stride - case.left < 0 and m * case.stride - case.left + case.k - 1 >= case.T for m in range(Mr)):
                t.add("mirror-both")
            t |= {x for c, x in ((case.elu, "elu"), (not case.bias, "nobias"), (case.resid, "resid")) if c}
        else:
            t.add(f"up{case.stride}x{Cout}")
            if Cout % 4 == 0 and CBK % Cout:
                t.add("frame-in-tile")
            if Cout % 4:
                t.add("frame-in-group")
            t.add("trim0" if case.trim == 0 else "trim>0")
            if g["Tout"] < Mr * g["up"] - case.trim:
                t.add("tout-short")
            if case.trim == 0 and g["Tout"] == Mr * g["up"]:
                t.add("untrimmed")
    elif case.op == "lstm":
        kq = case.C // 4
        t |= {f"H{case.C}", f"kq{kq}", f"T{case.T}", f"B{case.B}", "resid" if case.resid else "noresid",
              "wavefront" if case.layers == 2 and not case.plain else f"plain{case.layers}"}
        if kq % 128:
            t.add("partial-k-group")
        if kq > 128:
            t.add("k-groups>1")
        if case.B % 16:
            t.add("ragged-batch-tile")
        if case.B > 16:
            t.add("batch-tiles>1")
    elif case.op == "rvq_encode":
        t |= {f"M{case.T}", f"q{case.nq}"}
    elif case.op == "rvq_decode":
        t |= {f"q{case.nq}", "view" if case.sub == "view" else "contiguous"}
    elif case.op == "groupnorm":
        n, C = case.T * case.C, case.C
        t |= {f"C{C}", f"B{case.B}"}
        for cond, tag in ((256 % C != 0, "cstep"), (n == C, "n=C"), (n == GN_CHUNK, "n=chunk"), (n == GN_CHUNK - C, "n=chunk-C"),
                          (n == GN_CHUNK + C, "n=chunk+C"), (-(-n // GN_CHUNK) > 256, "chunks>256"), (case.resid, "resid"),
                          (n % GN_CHUNK != 0 and n > GN_CHUNK, "ragged-chunk")):
            if cond:
                t.add(tag)
    elif case.op == "scale":
        t |= {f"C{case.C}", f"T{case.T}", f"B{case.B}"}
    return t


REQUIRED_PATHS = {
    "conv": {"NT1", "NT2", "NT4", "NT8", "ragged-N-tile-st4", "ragged-N-tile-st1", "st4", "st1", "vec", "elem", "tap-in-kstep",
             "Cin1", "Cin2", "Cin3", "Cin4", "Cin12", "Cin20", "Cin16", "Cin64", "K7", "K21", "Kmod4", "Kmod8", "Kmod12", "nk1", "nk2",
             "nk>2", "Mr1", "Mr2", "Mr127", "Mr128", "Mr129", "Mr257", "M-tiles>1", "s1", "s2-extra", "s3-extra", "s5-extra", "s8-extra",
             "left-max", "right-max", "mirror-both", "B1", "B3", "elu", "nobias", "resid"},
    "convT": {"up2x4", "up8x20", "up5x3", "frame-in-tile", "frame-in-group", "trim0", "trim>0", "tout-short", "untrimmed", "B1", "B3",
              "M-tiles>1", "NT1", "NT8"},
    "lstm": {"H64", "H128", "H192", "H512", "H576", "kq16", "kq32", "kq48", "kq128", "kq144", "partial-k-group", "k-groups>1",
             "T1", "T2", "T3", "T17", "B1", "B15", "B16", "B17", "B33", "ragged-batch-tile", "batch-tiles>1", "plain1", "wavefront",
             "plain2", "plain3", "resid"},
    "rvq_encode": {"M1", "M15", "M16", "M17", "M33", "q1", "q2", "q32"},
    "rvq_decode": {"view", "contiguous", "q1", "q32"},
    "groupnorm": {"C1", "C3", "C32", "C48", "C96", "C320", "C512", "cstep", "n=C", "n=chunk", "n=chunk-C", "n=chunk+C", "chunks>256",
                  "ragged-chunk", "B1", "B3", "resid"},
    "scale": {"C1", "C2", "T1", "T1023", "T1024", "T1025", "B1", "B3"},
}


def _cases() -> list[Case]:
    L: list[Case] = []

    def add(fams, op, B, T, sub="", **kw):
        for f in fams:
            if f == "batch" and (T if op == "rvq_encode" else B) == 1:
                continue
            L.append(Case(op, "exact", B, T, sub="ramp", **kw) if f == "ramp" else Case(op, f, B, T, sub=sub, **kw))

    # ---- conv: B, Tin, Cin, Cout, k, stride, left, right, elu, bias, resid, cancel too
    for (B, T, Cin, Cout, k, s, l, r, elu, bias, resid, more) in (
        (1, 1, 1, 1, 1, 1, 0, 0, False, True, False, False),       # Mr = 1, K = 1
        (1, 4, 1, 2, 7, 1, 3, 3, False, True, False, False),       # K = 7; every window mirrored on both sides
        (1, 7, 2, 32, 7, 1, 6, 0, True, True, False, False),       # left = Tin - 1; NT 2
        (3, 40, 3, 3, 7, 1, 3, 3, False, False, True, True),       # K = 21, scalar stores, no bias, residual
        (1, 3, 4, 8, 4, 2, 2, 1, False, True, False, False),       # Mr = 2
        (1, 253, 4, 20, 7, 2, 5, 1, True, True, True, True),       # Mr = 127; Cin 4: the tap changes 4 times in a K step; K % 16 = 12
        (1, 128, 12, 16, 3, 1, 1, 1, False, True, False, False),   # Mr = 128 (one full tile); Cin 12, K % 16 = 4, nk 3; NT 1
        (1, 5, 12, 4, 2, 1, 0, 4, True, True, False, False),       # right = Tin - 1; K % 16 = 8, nk 2
        (1, 386, 20, 64, 5, 3, 2, 1, False, True, True, False),    # Mr = 129; Cin 20; stride 3; NT 4
        (1, 257, 16, 132, 1, 1, 0, 0, True, True, True, False),    # Mr = 257: three M tiles; two N tiles, 16-byte stores; nk 1
        (3, 33, 64, 130, 10, 5, 5, 2, True, True, True, True),     # two N tiles, scalar stores; stride 5; nk 40
        (3, 21, 8, 12, 16, 8, 8, 3, True, True, False, False),     # stride 8
    ):
        fams = ("exact", "ramp", "poison", "batch") + (("cancel",) if more else ())
        add(fams, "conv", B, T, C=Cin, Cout=Cout, k=k, stride=s, left=l, right=r, elu=elu, bias=bias, resid=resid)
    # ---- convT: B, Tin, Cin, Cout, s, trim, t_out (0: everything behind the trim)
    for (B, T, Cin, Cout, s, trim, t_out, elu) in (
        (1, 5, 4, 4, 2, 1, 10, True),        # N = 8; Tout = T s is one short of Mr up - trim
        (3, 7, 16, 20, 8, 0, 0, True),       # N = 160: two N tiles, the frame index changes inside a 16-column tile; untrimmed
        (3, 9, 8, 3, 5, 3, 45, False),       # N = 15: scalar stores, the frame index changes inside a 4-group
        (1, 130, 16, 20, 8, 8, 1040, True),  # Mr = 131: two M tiles
    ):
        add(("exact", "ramp", "poison", "batch"), "convT", B, T, C=Cin, Cout=Cout, stride=s, trim=trim, t_out=t_out, elu=elu)
    # ---- lstm: B, T, H, layers, plain, residual
    for (B, T, H, layers, plain, resid) in (
        (1, 1, 64, 1, False, False), (17, 2, 64, 2, False, False), (33, 17, 64, 3, False, False), (15, 3, 128, 1, False, False),
        (16, 2, 128, 3, False, True), (1, 17, 192, 2, False, False), (33, 2, 192, 2, True, False), (1, 2, 512, 1, False, False),
        (17, 3, 512, 2, False, True), (16, 2, 576, 1, False, False), (3, 3, 576, 3, False, False), (15, 2, 576, 2, True, True),
    ):
        add(("onehot", "saturate", "poison", "batch"), "lstm", B, T, C=H, layers=layers, plain=plain, resid=resid)
    # ---- rvq_encode: M, n_q
    for (M, nq) in ((1, 1), (15, 2), (16, 32), (17, 2), (33, 32)):
        add(("exact", "gaussian", "poison", "batch"), "rvq_encode", 1, M, nq=nq)
    # ---- rvq_decode
    for (B, T, nq, sub) in ((1, 1, 1, ""), (3, 9, 32, ""), (3, 9, 32, "view"), (2, 65, 2, "view")):
        add(("exact", "poison", "batch"), "rvq_decode", B, T, nq=nq, sub=sub)
    # ---- groupnorm: B, T, C, resid
    for (B, T, C, resid) in ((1, 5, 1, False), (3, 1, 3, True), (1, 511, 32, False), (3, 512, 32, False), (1, 513, 32, True),
                             (3, 342, 48, True), (1, 1, 96, False), (3, 200, 96, False), (3, 60, 320, True), (1, 32, 512, False),
                             (1, 33, 512, True)):
        add(("exact", "offset", "small", "poison", "batch"), "groupnorm", B, T, C=C, resid=resid)
    add(("offset", "poison"), "groupnorm", 1, 131200, C=32)  # 257 chunks: the apply pass's loop over the chunks runs twice
    # ---- scale
    for (B, T, C) in ((1, 1, 1), (3, 1023, 2), (1, 1024, 1), (3, 1025, 1), (3, 1024, 2)):
        add(("exact", "poison", "batch"), "scale", B, T, C=C)
    return L


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)

# refused by the launcher's argument checks before any launch (tests/test_hip_encodec_adversarial.py::test_refusals)
REFUSED = (Case("conv", "exact", 1, 4, C=4, Cout=4, k=7, left=4, right=2),       # left >= Tin
           Case("conv", "exact", 1, 4, C=4, Cout=4, k=9, left=2, right=2, t_out=1),  # Tin + left + right < k (Tout = 0 is PM_EINVAL)
           Case("convT", "exact", 1, 4, C=4, Cout=4, stride=2, resid=True),      # residual with up != 1
           Case("convT", "exact", 1, 4, C=4, Cout=4, stride=2, trim=3, t_out=8),  # trim + Tout > Mr up
           Case("lstm", "onehot", 1, 2, C=96))
REFUSED_RC = (2, 2, 1, 1, 2)  # what the C entry point answers to each: PM_EINVAL 1, PM_EUNSUPPORTED 2


# --------------------------------------------------------------------------------------------------------------- inputs
def convt_matrix(weight: torch.Tensor) -> torch.Tensor:
    """ConvTranspose1d's (Cin, Cout, 2 s) weight as the (s Cout, 2 Cin) matrix of include/pm_mi355x.h:
    w[r Cout + co][j Cin + ci] = weight[ci][co][r + (1 - j) s]."""
    Cin, Cout, k2 = weight.shape
    s = k2 // 2
    w = torch.empty(s * Cout, 2 * Cin, dtype=weight.dtype)
    for r in range(s):
        for j in range(2):
            w[r * Cout:(r + 1) * Cout, j * Cin:(j + 1) * Cin] = weight[:, :, r + (1 - j) * s].t()
    return w


def rvq_twin(j, q: int):
    """The exact RVQ family's twin of entry j at stage q.  rvq_encode_kernel reads entry j as 256 wave + 16 tile + 4 fq + rr, so
    j ^ 1 lies inside the same lane's four entries, j ^ 4 across fq, j ^ 16 across tiles, j ^ 256 across waves.  Which of the four
    it is turns with bits 5 and 6 of j (which no twin changes) and with the stage: every stage holds all four kinds."""
    kind = ((j >> 5) + q) & 3
    return j ^ (1 << (kind * 2 + (kind == 3) * 2))  # 1, 4, 16, 256


# stage 0 of the exact family, each set closed under rvq_twin(., 0) and a copy of its lowest entry: the first ties inside a lane
# (0 / 1), across fq (0 / 4), tiles (0 / 16) and waves (0 / 767, 0 / 1023) at once; the second is the last entry of wave 0 against
# the first of wave 1 (255 / 256).  RVQ_EXACT_ROWS: latent row -> the entry of stage 0 it equals; rows 0 and 2 meet the two sets,
# rows 1, 3, 5, 6 one pair of each kind (8 / 9, 584 / 600, 40 / 44, 100 / 356).
RVQ_TIE_SETS = ((0, 1, 4, 5, 16, 17, 767, 1023), (255, 256, 257, 511))
RVQ_EXACT_ROWS = {0: 1023, 1: 9, 2: 256, 3: 600, 5: 44, 6: 356}


def _perm_weights(g, H: int, scale: float):
    """Signed permutations with disjoint rows: row i of W_ih holds one +-scale when i is even, row i of W_hh when i is odd."""
    out = []
    for part in range(2):
        w = torch.zeros(4 * H, H)
        for gate in range(4):
            p = torch.randperm(H, generator=g)
            sg = torch.randint(0, 2, (H,), generator=g).float() * 2 - 1
            rows = torch.arange(H)
            live = rows % 2 == part
            w[gate * H + rows[live], p[live]] = sg[live] * scale
        out.append(w)
    return out


def build(case: Case) -> dict:
    """CPU fp32 tensors holding exactly the values the kernel sees."""
    g = torch.Generator().manual_seed(_seed(case))
    randn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    B, T, C = case.B, case.T, case.C
    fam = case.family
    if case.op in ("conv", "convT"):
        geo = conv_geometry(case)
        N, K, Cout = geo["N"], geo["K"], case.Cout
        out = {}
        if fam == "exact" and case.sub == "ramp":
            out["x"] = torch.arange(float(B * T * C)).view(B, T, C)
            w = torch.zeros(N, K)
            w[torch.arange(N), (torch.arange(N) * 7 + 3) % K] = 1.0
            out["w"] = w
        elif fam == "exact":
            out["x"] = ints(0 if case.elu else -3, 3, B, T, C) * (torch.rand(B, T, C, generator=g) < 0.6)
            out["w"] = ints(-3, 3, N, K)
        elif fam == "cancel":
            out["x"] = 4.0 + randn(B, T, C) / 16
            w = randn(N, K)
            out["w"] = (w - w.mean(1, keepdim=True)) * K ** -0.5 * 2
        else:
            out["x"] = randn(B, T, C)
            out["w"] = randn(N, K) * K ** -0.5
        integer = fam == "exact"
        out["bias"] = (ints(-8, 8, Cout) if integer else randn(Cout) * 0.5) if case.bias else None
        out["resid"] = (ints(-8, 8, B, geo["Tout"], Cout) if integer else randn(B, geo["Tout"], Cout)) if case.resid else None
        return out
    if case.op == "lstm":
        H = C
        out = {"w_ih": [], "w_hh": [], "bias": []}
        for l in range(case.layers):
            if fam in ("onehot", "saturate"):  # saturate: x = +-1 times 100 in layer 0; every other product is by 128 and so exact
                wi, wh = _perm_weights(g, H, 128.0 if fam == "saturate" else 2.0)
                wi = wi * (100.0 / 128.0) if fam == "saturate" and l == 0 else wi
                b = torch.zeros(4 * H)
            else:
                wi, wh, b = randn(4 * H, H) * H ** -0.5, randn(4 * H, H) * H ** -0.5, randn(4 * H) * 0.3
            out["w_ih"].append(wi), out["w_hh"].append(wh), out["bias"].append(b)
        out["x"] = (torch.randint(0, 2, (B, T, H), generator=g).float() * 2 - 1) if fam == "saturate" else randn(B, T, H)
        return out
    if case.op in ("rvq_encode", "rvq_decode"):
        nq = case.nq
        if case.op == "rvq_decode":
            E = randn(nq, RVQ_N, RVQ_D)
            codes = torch.randint(0, RVQ_N, (B, nq, T), generator=g)
            if fam == "exact":  # indices outside the codebook are clamped into it
                flat = codes.view(-1)
                flat[0], flat[flat.numel() // 2], flat[-1] = -1, RVQ_N, 2 ** 40
            return {"E": E, "codes": codes}
        M = T
        if fam == "exact":
            # every entry has a twin (rvq_twin), so every decision of every stage is a tie, and every stage holds all four kinds of
            # pair; stage 0 also holds the two sets of RVQ_TIE_SETS, each a copy of its lowest entry
            E = ints(-3, 3, nq, RVQ_N, RVQ_D)
            j = torch.arange(RVQ_N)
            for q in range(nq):
                E[q] = E[q, torch.minimum(j, rvq_twin(j, q))]
            for tied in RVQ_TIE_SETS:
                E[0, list(tied)] = E[0, tied[0]].clone()
            z = ints(-4, 4, M, RVQ_D)
            for i, a_ in RVQ_EXACT_ROWS.items():  # stage 0: the latent IS an entry (and its twins)
                if i < M:
                    z[i] = E[0, a_]
            if nq > 1 and M > 4:  # a stage > 0: the residual IS an entry of stage 1
                z[4] = E[0, 700] + E[1, 261]
            return {"z": z, "E": E, "norms": E.square().sum(-1)}
        E = randn(nq, RVQ_N, RVQ_D)
        z = randn(M, RVQ_D) * (1.5 if nq > 1 else 1.0)
        norms = E.square().sum(-1)
        planted = []
        if fam == "gaussian":
            # planted pairs: entry b repeats entry a (a > b, so that a tie would go to b), the latent is that entry, and the fp32 norm
            # of b is raised by 4 x (must be decided for a) or 0.25 x (exempt) the threshold delta_a + delta_b
            for i, (a, b, f) in enumerate(((900, 17, 4.0), (300, 299, 0.25), (513, 5, 4.0), (77, 76, 0.25))):
                if i >= M:
                    break
                E[0, b] = E[0, a]
                z[i] = E[0, a]
                thr = 2 * (RVQ_D + 2) * U32 * 3 * float(E[0, a].double().square().sum())
                norms[0, b] = norms[0, a] + f * thr * MARGIN
                planted.append((i, a, b, f))
        return {"z": z, "E": E, "norms": norms, "planted": planted}
    if case.op == "groupnorm":
        if fam == "exact":
            x = torch.full((B, T, C), 1.0) * ints(-9, 9, B, 1, 1)
        else:
            x = randn(B, T, C)
            if fam == "offset":
                x = x + OFFSET_RATIO * (torch.arange(B).view(B, 1, 1) % 2 * 2 - 1)  # clips at -4096, +4096, -4096
            elif fam == "small":
                x = x * 0.01
        integer = fam == "exact"
        return {"x": x, "gamma": ints(-3, 3, C) if integer else 1.0 + 0.5 * randn(C), "beta": ints(-8, 8, C) if integer else randn(C),
                "resid": (ints(-8, 8, B, T, C) if integer else randn(B, T, C)) if case.resid else None}
    if case.op == "scale":
        x = randn(B, C, T)
        if fam == "exact":
            x[0] = 0.0
        return {"x": x}
    raise ValueError(case.op)


# --------------------------------------------------------------------------------------------------------------- convolution
def conv_forward(case: Case, inp: dict, dtype=torch.float64, reverse=False, mutant=None) -> dict:
    """pm_conv1d_f32 in `dtype` arithmetic (float64: the reference; float32 with reverse=True: a correct kernel's stand-in, the K
    terms in the opposite order).  Returns want (B, Tout, Cout) and, in float64, the bound."""
    geo = conv_geometry(case)
    k, s, left, right, up, trim, Mr, Tout, N, K = (geo[n] for n in ("k", "stride", "left", "right", "up", "trim", "Mr", "Tout", "N", "K"))
    x, w = inp["x"].to(dtype), inp["w"].to(dtype)
    B, Tin, Cin = x.shape
    Cout = case.Cout
    elu_on_load = case.elu and mutant != "elu_after"
    xe = torch.stack([F.elu(x[b_]) for b_ in range(B)]) if elu_on_load else x  # clip by clip: the stand-in must not depend on the batch

    def mirror(f):
        if geo["zero_pad"]:
            return f.clamp(0, Tin - 1), (f >= 0) & (f < Tin)
        ok = torch.ones_like(f, dtype=torch.bool)
        if mutant == "replicate":
            return f.clamp(0, Tin - 1), ok
        src = f.abs()
        src = torch.where(src >= Tin, (2 * Tin - 1 if mutant == "mirror_edge" else 2 * (Tin - 1)) - src, src)
        if mutant == "extra_pad_zero" and s > 1 and -Tin % s:
            ok = f < Tin + right - (-Tin % s)
        return src, ok

    m = torch.arange(Mr)[:, None]
    if mutant == "tap_carry" and Cin % 4 == 0:  # the chunk's tap is that of the K step's first column; ci runs on past Cin
        kk = torch.arange(K)[None, :]
        tap = (kk // CBK * CBK) // Cin
        src, ok = mirror(m * s - left + tap)
        flat = (src * Cin + kk - tap * Cin).clamp(0, Tin * Cin - 1)
        gK = xe.reshape(B, Tin * Cin)[:, flat] * ok[None]
    else:
        f = m * s - left + torch.arange(k)[None, :]
        src, ok = mirror(f)
        if mutant == "clip_cross":  # the batch as one long sequence: a window at a clip's edge reads the neighbour
            absf = torch.arange(B)[:, None, None] * Tin + f[None]
            inside = (absf >= 0) & (absf < B * Tin)
            absf = torch.where(inside, absf, torch.arange(B)[:, None, None] * Tin + src[None])
            g = xe.reshape(B * Tin, Cin)[absf]
        else:
            g = xe[:, src]
        g = g * ok[None, :, :, None]
        if mutant == "up_phase_swap":
            g = g.flip(2)
        gK = g.reshape(B, Mr, K)
    if reverse:  # clip by clip: the stand-in's rows must not depend on the batch either
        P = torch.stack([gK[b_].flip(-1) @ w.flip(-1).t() for b_ in range(B)])
    else:
        P = gK @ w.t()
    if mutant == "elu_after" and case.elu:
        P = F.elu(P)
    r = {}
    if dtype == torch.float64:
        A = gK.abs() @ w.abs().t()
        extra = 3 * U32 * A if case.elu else 0.0
    if inp["bias"] is not None:
        c = torch.arange(N) % Cout
        if mutant == "bias_lane":
            c = c // 4 * 4
        P = P + inp["bias"].to(dtype)[c]
        if dtype == torch.float64:
            A = A + inp["bias"].double().abs()[torch.arange(N) % Cout]
    place = lambda t: F.pad(t.reshape(B, Mr * up, Cout), (0, 0, 0, 1))[:, trim + (mutant == "trim_shift"):][:, :Tout]  # noqa: E731
    want = place(P)
    if inp["resid"] is not None:
        want = want + inp["resid"].to(dtype)
    r["want"] = want
    if dtype == torch.float64:
        A = place(A)
        delta = (K + 2) * U32 * A + (place(extra) if case.elu else 0.0)
        if inp["resid"] is not None:
            delta = delta + (K + 2) * U32 * inp["resid"].double().abs()
        r["bound"] = delta + store_term(want, "f32")
    return r


# --------------------------------------------------------------------------------------------------------------- LSTM
def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def lstm_step_reference(w_ih, w_hh, bias, xin, hkernel, exact_pre: bool):
    """One layer, teacher-forced: xin (B, T, H) the layer's input rows, hkernel (B, T, H) the kernel's own h.  Returns (want, bound):
    h_t computed in float64 from the kernel's h_(t-1), and the propagated bound e_h(t)."""
    xin, hk = xin.double(), hkernel.double()
    B, T, H = xin.shape
    wi, wh, b = w_ih.double(), w_hh.double(), bias.double()
    hprev = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64), hk[:, :-1]], 1)
    z = xin @ wi.t() + hprev @ wh.t() + b
    A = xin.abs() @ wi.abs().t() + hprev.abs() @ wh.abs().t() + b.abs()
    dz = torch.zeros_like(A) if exact_pre else (2 * H + 4) * U32 * A
    zi, zf, zg, zo = z.split(H, -1)
    di, df, dg, do = dz.split(H, -1)
    i, f, g, o = _sig(zi), _sig(zf), torch.tanh(zg), _sig(zo)
    di, df, do = (0.25 * d + 4 * U32 * v + TINY for d, v in ((di, i), (df, f), (do, o)))
    dg = dg + 4 * U32 * g.abs() + TINY
    c = torch.zeros(B, H, dtype=torch.float64)
    ec = torch.zeros(B, H, dtype=torch.float64)
    want, bound = [], []
    for t in range(T):
        cn = f[:, t] * c + i[:, t] * g[:, t] if t else i[:, t] * g[:, t]
        local = (c.abs() * df[:, t] if t else 0.0) + g[:, t].abs() * di[:, t] + i[:, t] * dg[:, t] + 2 * U32 * cn.abs() + TINY
        ec = (f[:, t] * ec if t else 0.0) + local
        c = cn
        th = torch.tanh(c)
        h = o[:, t] * th
        want.append(h)
        bound.append(o[:, t] * (ec + 4 * U32 * th.abs() + TINY) + th.abs() * do[:, t] + U32 * h.abs() + TINY)
    return torch.stack(want, 1), torch.stack(bound, 1)


def lstm_emulate(x, w_ih, w_hh, bias, residual=False, plain=False, dtype=torch.float32, mutant=None):
    """The stacked LSTM run sequentially in `dtype`: float32 = a correct kernel's stand-in, float64 + mutant = a defective one."""
    B, T, H = x.shape
    inp = x.to(dtype)
    c = torch.zeros(B, H, dtype=dtype)
    rows = torch.arange(B).clamp(max=15) if mutant == "row_clamp" else torch.arange(B)  # clamped to the tile, not to B - 1
    for l, (wi, wh, b) in enumerate(zip(w_ih, w_hh, bias)):
        wi, wh, b = wi.to(dtype), wh.to(dtype), b.to(dtype)
        if mutant == "stale_acc":  # the store takes the accumulator without the last four k of each wave's quarter (recurrent part)
            wh = wh.clone()
            kq = H // 4
            for wv in range(4):
                wh[:, (wv + 1) * kq - 4:(wv + 1) * kq] = 0
        h = torch.zeros(B, H, dtype=dtype)
        if mutant != "c_not_reset" or l == 0:  # (mutant: a layer starts from the cell state the layer below left in cbuf[0])
            c = torch.ones(B, H, dtype=dtype) if mutant == "c_not_reset" else torch.zeros(B, H, dtype=dtype)
        ys = []
        mm = (lambda a, w_: torch.stack([r_ @ w_.t() for r_ in a])) if dtype == torch.float32 else (lambda a, w_: a @ w_.t())  # row by row
        for t in range(T):
            z = mm(inp[rows, t], wi) + (mm(h[rows], wh) if t else 0.0) + b
            zi, zf, zg, zo = z.split(H, -1)
            if mutant == "gate_order":
                zg, zo = zo, zg
            i, f, g, o = _sig(zi), _sig(zf), torch.tanh(zg), _sig(zo)
            c = f * c + i * g if (t or mutant == "c_not_reset") else i * g
            h = o * torch.tanh(c)
            ys.append(h)
        inp = torch.stack(ys, 1)
    y = inp.float()
    return x + y if residual else y


def lstm_verify(case: Case, inp: dict, run) -> tuple[bool, float, str]:
    """run(x, w_ih, w_hh, bias, residual, plain) -> y (CPU f32) is the implementation under test.  Every layer below the last runs
    as a single-layer call and is checked step by step; the whole call's output is checked as the last layer fed with those rows."""
    exact_pre = case.family in ("onehot", "saturate")
    wi, wh, b = inp["w_ih"], inp["w_hh"], inp["bias"]
    rows, worst = inp["x"], 0.0
    for l in range(case.layers - 1):
        y = run(rows, wi[l:l + 1], wh[l:l + 1], b[l:l + 1], False, False)
        worst = max(worst, ratio(y, *lstm_step_reference(wi[l], wh[l], b[l], rows, y, exact_pre)))
        rows = y
    forms = [case.plain] if case.layers != 2 else [case.plain, not case.plain]  # two layers: the other form too, the same reference
    for plain in forms:
        y = run(inp["x"], wi, wh, b, False, plain)
        if y.shape != inp["x"].shape:
            return False, float("inf"), "shape"
        worst = max(worst, ratio(y, *lstm_step_reference(wi[-1], wh[-1], b[-1], rows, y, exact_pre)))
        if case.resid and plain == case.plain:
            yr = run(inp["x"], wi, wh, b, True, plain)
            if not torch.equal(yr, inp["x"] + y):
                return False, float("inf"), "the residual form is not x + y"
    return True, worst, ""


# --------------------------------------------------------------------------------------------------------------- RVQ
def rvq_reference(z, E, norms, nq, margin=MARGIN, mutant=None) -> dict:
    """codes (nq, M): lowest index of the float64 minimum of norms - 2 r.e, r -= e in fp32; decided (nq, M); ties (nq, M)."""
    r = z.float().clone()
    ar = torch.arange(RVQ_N)[None, :]
    codes, decided, ties = [], [], []
    for q in range(nq):
        Eq = E[q].double()
        dot = r.double() @ Eq.t()
        nrm = torch.zeros_like(dot) if mutant == "no_norm" else norms[q].double()[None, :]
        d = nrm - 2 * dot
        delta = (RVQ_D + 2) * U32 * (norms[q].double().abs()[None, :] + 2 * r.double().abs() @ Eq.abs().t())
        dmin = d.min(1, keepdim=True).values
        hit = d == dmin
        if mutant == "tie_highest":
            code = torch.where(hit, ar, -1).max(1).values
        elif mutant == "wave_tie":  # lowest inside a wave of 256 entries, "<=" across the waves: the highest tied wave wins
            wave = torch.where(hit, ar // 256, -1).max(1, keepdim=True).values
            code = torch.where(hit & (ar // 256 == wave), ar, RVQ_N).min(1).values
        else:
            code = torch.where(hit, ar, RVQ_N).min(1).values
        best = code[:, None]
        lo = (d - margin * delta).scatter(1, best, float("inf")).min(1).values
        decided.append(lo > (d + margin * delta).gather(1, best)[:, 0])
        ties.append(hit.sum(1) > 1)
        codes.append(code)
        if mutant != "resid_stale":
            r = r - E[q][code]
    return {"codes": torch.stack(codes), "decided": torch.stack(decided), "ties": torch.stack(ties)}


def rvq_emulate(z, E, norms, nq) -> torch.Tensor:
    """A correct kernel's stand-in: fp32 distances (fma(-2, r.e, norm)), first minimum, r -= e."""
    r = z.float().clone()
    ar = torch.arange(RVQ_N)[None, :]
    codes = []
    for q in range(nq):
        d = torch.addcmul(norms[q][None, :], r.flip(-1) @ E[q].flip(-1).t(), torch.tensor(-2.0))
        code = torch.where(d == d.min(1, keepdim=True).values, ar, RVQ_N).min(1).values
        codes.append(code)
        r = r - E[q][code]
    return torch.stack(codes)


def rvq_codes_accept(got: torch.Tensor, ref: dict, exact: bool) -> tuple[bool, float, str]:
    """The decided rule.  Returns (ok, share of differing (stage, row) pairs, message)."""
    want = ref["codes"]
    if got.shape != want.shape or got.dtype != torch.int64:
        return False, float("inf"), "shape / dtype"
    differ = got != want
    if exact:
        return not bool(differ.any()), float(differ.float().mean()), f"{int(differ.sum())} codes differ from the exact result"
    M = want.shape[1]
    first = torch.where(differ.any(0), differ.int().argmax(0), torch.full((M,), -1))
    bad = [(int(m), int(first[m])) for m in (first >= 0).nonzero()[:, 0] if bool(ref["decided"][first[m], m])]
    return not bad, float(differ.float().mean()), f"(row, stage) differs at a decided decision: {bad[:8]}"


def rvq_decode_reference(codes: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    B, nq, T = codes.shape
    idx = codes.clamp(0, RVQ_N - 1)
    out = E[0][idx[:, 0]]
    for q in range(1, nq):
        out = out + E[q][idx[:, q]]
    return out


# --------------------------------------------------------------------------------------------------------------- GroupNorm, scale
def gn_forward(case: Case, inp: dict, dtype=torch.float64, mutant=None) -> dict:
    x = inp["x"]
    B, T, C = x.shape
    n = T * C
    xf = x.reshape(B, n)
    ch = torch.arange(n) % C
    if mutant == "chan_step":  # the channel of element i taken from its thread alone: (i % 256) % C
        ch = torch.arange(n) % 256 % C
    if mutant == "onepass":  # fp32 sums of 64 values per thread, E[x^2] - mean^2
        pad = F.pad(xf, (0, -n % GN_CHUNK)).view(B, -1, GN_PER, 256)
        s, ss = torch.zeros(B, pad.shape[1], 256), torch.zeros(B, pad.shape[1], 256)
        for j in range(GN_PER):
            s, ss = s + pad[:, :, j], ss + pad[:, :, j] * pad[:, :, j]
        mean = s.double().sum((1, 2)) / n
        var = (ss.double().sum((1, 2)) / n - mean * mean).clamp_min(0)
    else:
        mean = xf.double().mean(1)
        var = (xf.double() - mean[:, None]).square().sum(1) / (n - 1 if mutant == "var_unbiased" and n > 1 else n)
    rstd = 1.0 / (var.sqrt() + EPS) if mutant == "eps_outside" else 1.0 / torch.sqrt(var + EPS)
    if dtype == torch.float32:  # the stand-in: the kernel's own roundings
        mu, rs = mean.float()[:, None], rstd.float()[:, None]
        y = torch.addcmul(inp["beta"][ch], (xf - mu) * rs, inp["gamma"][ch])
        if inp["resid"] is not None:
            y = y + inp["resid"].reshape(B, n)
        return {"want": y.view(B, T, C)}
    yhat = (xf.double() - mean[:, None]) * rstd[:, None]
    gam = inp["gamma"].double()[ch]
    y = yhat * gam + inp["beta"].double()[ch]
    e = (U32 * mean.abs() + (GN_PER + 2) * U32 * var.sqrt())[:, None]
    delta = gam.abs() * rstd[:, None] * (2 + yhat.abs()) * e + 3 * U32 * (gam * yhat).abs() + U32 * y.abs()
    want = y
    if inp["resid"] is not None:
        want = y + inp["resid"].double().reshape(B, n)
        delta = delta + U32 * (inp["resid"].double().reshape(B, n).abs() + want.abs())
    return {"want": want.view(B, T, C), "bound": (delta + store_term(want, "f32")).view(B, T, C), "mean": mean, "var": var}


def scale_forward(inp: dict, dtype=torch.float64, mutant=None) -> dict:
    x = inp["x"]
    B, C, T = x.shape
    if dtype == torch.float32:
        m = x.flip(1).sum(1) / C
        return {"want": (m.double().square().mean(1).float().sqrt() + torch.tensor(1e-8)).view(B, 1, 1)}
    xd = x.double()
    m2 = xd.square().mean(1) if mutant == "square_first" else xd.mean(1).square()
    s = m2.mean(1).sqrt()
    want = s + 1e-8
    dm = (C + 1) * U32 * xd.abs().mean(1)
    delta = (2 * xd.mean(1).abs() * dm).sum(1) / (2 * T * s.clamp_min(1e-300)) + 3 * U32 * s + U32 * want
    return {"want": want.view(B, 1, 1), "bound": delta.view(B, 1, 1)}


# --------------------------------------------------------------------------------------------------------------- the verdict
class StandIn:
    """The ops on the CPU: dtype float32 = a correct kernel's stand-in (fp32 arithmetic, another summation order);
    float64 with a mutant = what a kernel with the named defect returns."""

    def __init__(self, dtype=torch.float32, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.dtype, self.mutant = dtype, mutant

    def conv(self, case, inp):
        return conv_forward(case, inp, self.dtype, reverse=self.dtype == torch.float32, mutant=self.mutant)["want"].float()

    def lstm(self, x, w_ih, w_hh, bias, residual, plain):
        return lstm_emulate(x, w_ih, w_hh, bias, residual, plain, self.dtype, self.mutant)

    def rvq_encode(self, z, E, norms, nq):
        if self.mutant:
            return rvq_reference(z, E, norms, nq, mutant=self.mutant)["codes"]
        return rvq_emulate(z, E, norms, nq)

    def rvq_decode(self, codes, E):
        return rvq_decode_reference(codes, E)

    def groupnorm(self, case, inp):
        return gn_forward(case, inp, self.dtype, self.mutant)["want"].float()

    def scale(self, inp):
        return scale_forward(inp, self.dtype, self.mutant)["want"].float()

    def scale_clips(self, x, s, divide):
        return x / s if divide else x * s


def clip(case: Case, inp: dict, b: int) -> tuple[Case, dict]:
    """The single-clip (row) problem of clip b (batch family)."""
    per_clip = {"conv": ("x", "resid"), "convT": ("x", "resid"), "lstm": ("x",), "groupnorm": ("x", "resid"), "scale": ("x",),
                "rvq_decode": ("codes",), "rvq_encode": ("z",)}[case.op]
    one = {k: (v[b:b + 1] if k in per_clip and v is not None else v) for k, v in inp.items()}
    return (replace(case, T=1) if case.op == "rvq_encode" else replace(case, B=1)), one


def reference(case: Case, inp: dict) -> dict:
    if case.op in ("conv", "convT"):
        return conv_forward(case, inp)
    if case.op == "rvq_encode":
        return rvq_reference(inp["z"], inp["E"], inp["norms"], case.nq)
    if case.op == "rvq_decode":
        return {"want": rvq_decode_reference(inp["codes"], inp["E"])}
    if case.op == "groupnorm":
        return gn_forward(case, inp)
    if case.op == "scale":
        return scale_forward(inp)
    return {}  # lstm: the reference needs the kernel's own h (lstm_verify)


def run_plain(be, case: Case, inp: dict) -> torch.Tensor:
    """The case's main output through backend `be` (a StandIn, or the GPU suite's wrapper of pytorch_models._hip.ops)."""
    if case.op in ("conv", "convT"):
        return be.conv(case, inp)
    if case.op == "lstm":
        return be.lstm(inp["x"], inp["w_ih"], inp["w_hh"], inp["bias"], case.resid, case.plain)
    if case.op == "rvq_encode":
        return be.rvq_encode(inp["z"], inp["E"], inp["norms"], case.nq)
    if case.op == "rvq_decode":
        return be.rvq_decode(inp["codes"].transpose(1, 2).contiguous().transpose(1, 2) if case.sub == "view" else inp["codes"], inp["E"])
    if case.op == "groupnorm":
        return be.groupnorm(case, inp)
    return be.scale(inp)


def verify(case: Case, inp: dict, ref: dict, be, margin: float = MARGIN) -> tuple[bool, float, str]:
    """Every assertion the GPU suite makes on a case but the poison family's second launch: (ok, ratio, message)."""
    y = None
    if case.op == "lstm":
        ok, r, msg = lstm_verify(case, inp, be.lstm)
        if ok and not r <= margin:
            ok, msg = False, f"{r:.3f} x the bound (allowed {margin})"
    elif case.op == "rvq_encode":
        y = run_plain(be, case, inp)
        rf = ref if margin == MARGIN else rvq_reference(inp["z"], inp["E"], inp["norms"], case.nq, margin)
        ok, r, msg = rvq_codes_accept(y, rf, case.family == "exact")
    else:
        y = run_plain(be, case, inp)
        want = ref["want"]
        if tuple(y.shape) != tuple(want.shape) or y.dtype != torch.float32:
            return False, float("inf"), "shape / dtype"
        if case.op == "rvq_decode" or (case.family == "exact" and case.op != "scale"):
            ok = torch.equal(y, want.float())
            r, msg = (0.0 if ok else float("inf")), f"{int((y.double() != want.float().double()).sum())} of {y.numel()} outputs differ from the exact result"
        else:
            r = ratio(y, want, ref["bound"])
            ok, msg = r <= margin, f"{r:.3f} x the bound (allowed {margin})"
        if ok and case.op == "scale":
            if case.family == "exact" and not bool(y[0, 0, 0] == torch.tensor(1e-8, dtype=torch.float32)):
                return False, float("inf"), "an all-zero clip must give float32(1e-8)"
            for divide in (True, False):  # by the kernel's own fp32 scale: one rounding each, 0 / 1e-8 = 0
                got = be.scale_clips(inp["x"], y, divide)
                if case.family == "batch":
                    for b_ in sorted({0, case.B // 2, case.B - 1}):
                        if not torch.equal(be.scale_clips(inp["x"][b_:b_ + 1], y[b_:b_ + 1], divide), got[b_:b_ + 1]):
                            return False, float("inf"), f"scale_clips(divide={divide}): clip {b_} of the batch differs from its run alone"
                w2 = inp["x"].double() / y.double() if divide else inp["x"].double() * y.double()
                r2 = ratio(got, w2, U32 * w2.abs())
                if not r2 <= margin:
                    return False, r2, f"scale_clips(divide={divide}): {r2:.3f} x the bound"
                r = max(r, r2)
    if not ok:
        return False, r, msg
    if case.family == "batch":
        nb = case.T if case.op == "rvq_encode" else case.B
        full = run_plain(be, case, inp) if y is None else y
        for b_ in sorted({0, nb // 2, nb - 1}):
            c1, one = clip(case, inp, b_)
            alone = run_plain(be, c1, one)
            part = full[:, b_] if case.op == "rvq_encode" else full[b_]
            if not torch.equal(alone.reshape(-1), part.reshape(-1)):
                return False, float("inf"), f"clip / row {b_} of the batch differs from its run alone"
    return True, r, ""


# --------------------------------------------------------------------------------------------------------------- on the device
def embedded(t: torch.Tensor, dev, gap: int = 0, sentinel: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """t (B, ...) as the middle of a flat buffer filled with NaN (f32) or the guard pattern (sentinel, and every int64 buffer), clip b
    at b * (numel per clip + gap), a guard of >= 64 elements in front and behind: the view keeps 16-byte alignment.
    Returns (buffer, view)."""
    B = t.shape[0]
    per = t.numel() // B
    guard = -(-max(per, 64) // 64) * 64
    total = 2 * guard + B * (per + gap)
    if t.dtype == torch.int64:
        buf = torch.full((total,), SENTINEL64, dtype=torch.int64)
    elif sentinel:
        buf = torch.full((total,), SENTINEL, dtype=torch.int32).view(torch.float32)
    else:
        buf = torch.full((total,), float("nan"), dtype=torch.float32)
    buf = buf.to(dev)
    view = buf[guard:guard + B * (per + gap)].view(B, per + gap)[:, :per].unflatten(1, tuple(t.shape[1:]))
    if not sentinel:
        view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def sentinels_intact(buf: torch.Tensor, view: torch.Tensor) -> bool:
    """Every element of the flat buffer outside the (dense) `view` still holds the guard pattern."""
    b = buf.cpu().clone()
    pat = SENTINEL64 if b.dtype == torch.int64 else SENTINEL
    bits = b if b.dtype == torch.int64 else b.view(torch.int32)
    guard = (b.numel() - view.numel()) // 2
    bits[guard:guard + view.numel()] = pat
    return bool((bits == pat).all())


class Device:
    """pytorch_models._hip.ops behind StandIn's interface: CPU tensors in, CPU tensors out."""

    def __init__(self, ops, dev="cuda"):
        self.ops, self.dev = ops, dev

    def _d(self, t):
        return None if t is None else t.to(self.dev)

    def conv(self, case, inp):
        g = conv_geometry(case)
        return self.ops.conv1d_f32(self._d(inp["x"]), self._d(inp["w"]), self._d(inp["bias"]), k=g["k"], stride=g["stride"], left=g["left"],
                                   right=g["right"], elu=case.elu, resid=self._d(inp["resid"]), zero_pad=g["zero_pad"], up=g["up"],
                                   trim=g["trim"], t_out=g["Tout"]).cpu()

    def lstm(self, x, w_ih, w_hh, bias, residual, plain):
        d = lambda ts: [self._d(t) for t in ts]  # noqa: E731
        return self.ops.lstm_f32(self._d(x).contiguous(), d(w_ih), d(w_hh), d(bias), residual=residual, plain=plain).cpu()

    def rvq_encode(self, z, E, norms, nq):
        return self.ops.rvq_encode(self._d(z).contiguous(), self._d(E), self._d(norms), nq).cpu()

    def rvq_decode(self, codes, E):
        return self.ops.rvq_decode(self._d(codes), self._d(E)).cpu()

    def groupnorm(self, case, inp):
        return self.ops.groupnorm1_(self._d(inp["x"]).clone(), self._d(inp["gamma"]), self._d(inp["beta"]), EPS, self._d(inp["resid"])).cpu()

    def scale(self, inp):
        return self.ops.encodec_scale(self._d(inp["x"]).contiguous()).cpu()

    def scale_clips(self, x, s, divide):
        return self.ops.scale_clips(self._d(x).contiguous(), self._d(s), divide).cpu()


def run_abi(ops, case: Case, inp: dict, dev) -> dict:
    """The poison family's launch through lib(): NaN-surrounded operands (conv: a NaN gap of 8 floats between the clips), a
    sentinel-surrounded output, a NaN-filled workspace.  Returns y (dense CPU copy) and guard_bad."""
    import ctypes

    L, st = ops.lib(), ops._stream()
    P = lambda t, gap=0: None if t is None else embedded(t.contiguous(), dev, gap)[1]  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    nan = lambda n, dt=torch.float32: torch.full((max(int(n), 4),), float("nan"), dtype=dt, device=dev)  # noqa: E731
    B, T, C = case.B, case.T, case.C
    if case.op in ("conv", "convT"):
        g = conv_geometry(case)
        x = P(inp["x"], 8)
        w, bias, resid = P(inp["w"][None])[0], P(None if inp["bias"] is None else inp["bias"][None]), P(inp["resid"])
        obuf, y = embedded(torch.empty(B, g["Tout"], case.Cout), dev, sentinel=True)
        rc = L.pm_conv1d_f32(ptr(x), T * C + 8, ptr(w), ptr(bias), ptr(resid), ptr(y), B, T, C, case.Cout, g["k"], g["stride"], g["left"],
                             g["right"], int(g["zero_pad"]), int(case.elu), g["up"], g["trim"], g["Tout"], st)
    elif case.op == "lstm":
        n = case.layers
        x = P(inp["x"])
        ws = {k: [P(t[None])[0] for t in inp[k]] for k in ("w_ih", "w_hh", "bias")}
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        work = nan(L.pm_lstm_workspace_floats(B, T, C))
        obuf, y = embedded(torch.empty(B, T, C), dev, sentinel=True)
        rc = L.pm_lstm_f32(ptr(x), arr(ws["w_ih"]), arr(ws["w_hh"]), arr(ws["bias"]), n, ptr(work), ptr(y),
                           int(case.resid) | (2 if case.plain else 0), B, T, C, st)
    elif case.op == "rvq_encode":
        z, E, norms = P(inp["z"][None])[0], P(inp["E"][None])[0], P(inp["norms"][None])[0]
        obuf, y = embedded(torch.empty(1, case.nq, T, dtype=torch.int64), dev, sentinel=True)
        rc = L.pm_rvq_encode_f32(ptr(z), ptr(E), ptr(norms), ptr(y), T, case.nq, RVQ_D, RVQ_N, st)
        y = y[0]
    elif case.op == "rvq_decode":
        codes = inp["codes"].transpose(1, 2).contiguous().transpose(1, 2) if case.sub == "view" else inp["codes"]
        cbuf = torch.full((codes.numel() + 128,), SENTINEL64, dtype=torch.int64, device=dev)
        cv = cbuf[64:64 + codes.numel()].as_strided(codes.shape, codes.stride())
        cv.copy_(codes)
        E = P(inp["E"][None])[0]
        obuf, y = embedded(torch.empty(B, T, RVQ_D), dev, sentinel=True)
        rc = L.pm_rvq_decode_f32(ptr(cv), cv.stride(0), cv.stride(1), cv.stride(2), ptr(E), ptr(y), B, T, case.nq, RVQ_D, RVQ_N, st)
    elif case.op == "groupnorm":
        n = T * C
        gamma, beta, resid = P(inp["gamma"][None])[0], P(inp["beta"][None])[0], P(inp["resid"])
        work = nan(L.pm_groupnorm1_workspace_doubles(B, n), torch.float64)
        obuf, y = embedded(torch.empty(B, T, C), dev, sentinel=True)  # in place: the operand sits inside the sentinels
        y.copy_(inp["x"])
        rc = L.pm_groupnorm1_f32(ptr(y), ptr(gamma), ptr(beta), ptr(resid), ptr(work), B, n, C, float(EPS), st)
    else:
        x = P(inp["x"])
        obuf, y = embedded(torch.empty(B, 1, 1), dev, sentinel=True)
        rc = L.pm_encodec_scale_f32(ptr(x), ptr(y), B, C, T, st)
        if rc == 0:
            out = {}
            for divide in (1, 0):
                o2, y2 = embedded(torch.empty(B, C, T), dev, sentinel=True)
                rc = rc or L.pm_scale_clips_f32(ptr(x), ptr(y), ptr(y2), B, C * T, divide, st)
                out[divide] = (y2.cpu().contiguous(), not sentinels_intact(o2, y2))
            assert rc == 0, (case.id, rc)
            return {"y": y.cpu().contiguous(), "guard_bad": not sentinels_intact(obuf, y) or out[1][1] or out[0][1], "div": out[1][0], "mul": out[0][0]}
    assert rc == 0, (case.id, rc)
    return {"y": y.cpu().contiguous(), "guard_bad": not sentinels_intact(obuf, y)}
