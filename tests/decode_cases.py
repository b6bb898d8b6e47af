"""Float64 references, derived bounds, input families, case lists and a CPU stand-in for the decode-step kernels of csrc/decode.hip.
Shared by tests/test_decode_cases_cpu.py (no GPU: the stand-in passes every assertion, every named defect fails one, the case lists
reach every path) and tests/test_hip_decode_adversarial.py (the same judge() on the kernels).  DESIGN.md "2g. Decode-step numerics
contract" holds the derivations; this docstring states the contract and maps every launcher path to the cases that reach it.

CONTRACT (u = 2^-24; no number measured on a kernel enters an assertion; the GPU suite asserts MARGIN = 1.5 x the bound, the CPU stand-in
1.0 x; an element whose bound is 0 must be exact; a non-finite output is an infinite ratio)

  three-term split   split3(x) = (hi, mid, lo), three bf16 values with hi + mid + lo = x exactly for |x| in [2^-90, 2^100] (below, lo
                     falls into bf16 subnormals).  bf16 x bf16 products are exact in fp32, so pm_dec_linear without LayerNorm is an fp32
                     sum of 3 K exact products in some order plus c further additions:
                         delta_z = (3 K + c) u A',   A' = sum_k (|hi| + |mid| + |lo|) |w| + |bias|,
                         c = 3 (the four waves' partial tiles) + k_split (the parts, K split only) + 1 (the bias)
  K parts            part p of pm_dec_linear_kparts: (3 K_p + 3) u A'_p over its own K steps [ksteps p / k_split, ksteps (p + 1) / k_split)
  activation         apply_act<ACT, true>: erf-GELU 1.13 delta_z + u (6 |z| + 2 |g|), GELU-tanh 1.13 delta_z + u (4 |z| + 2 |g|)
                     (linear_cases.act_bound, the bounds of 2d and 2c); the residual adds u |want|, the f32 store u |want|
  fused LayerNorm    two passes from registers: e = K u mean |x|, |dxn_k| <= |gamma_k| / sigma (2 + |xhat_k|) e + 3 u |xn_k| (2d), then
                         delta_z = sum_k |w_nk| dxn_k + (3 K + c) u A'(xn)
  DL_QKV             q as above; k and v are rounded once, to nearest even, to bf16: delta_z + half a bf16 ulp of (|want| + delta_z)
  discrete outputs   arg-max indices, tickets, every cache row but the written one, every byte outside an output: exact

INPUT FAMILIES
  exact   x integers: half zeros, the rest up to 12 significant bits, three per row with 19 - 20 (mid and lo carry information);
          w integers in [-2, 2] that differ along n and k; bias, resid integers; A' < 2^24, so every partial sum in any order is an
          exact integer and the output EQUALS the reference.  DL_QKV: bias plants exact bf16 ties (258, 262, ... x 2^s) in row 0.
  cancel  zero-sum weight rows (w[:, K/2:] = -w[:, :K/2]) on x = 1 + 2^-6 noise: |z| << A'
  offset  LayerNorm, K <= 192: x = 4096 + noise (|mean| / sigma = 4096): a one-pass variance is orders of magnitude out
  scale   no LayerNorm, activation, bias: out(2^k x) == 2^k out(x) bit for bit, k = +-40
  poison  every operand the 16-byte aligned middle of a NaN-filled buffer with ldx > K, ldw > K, ldr > N
  perm    y(x[p]) == y(x)[p] bit for bit (rows are independent; M > 16 moves rows between row tiles / gridDim.z workgroups)
  tie     arg-max: x rows = one direction + 5 % noise; every arg-max tile has one planted winner row (alpha_t x the direction, alpha_t
          distinct) and every other logit sits >= 4 x the bound below it; duplicated weight rows (identical arithmetic, equal logits)
          in one 16-feature tile on different kq lanes, in adjacent feature tiles, in the first and the last arg-max tile, in the ragged
          last tile, and (persistent kernel) in two tiles walked by one workgroup: the lowest index must win
  EVERY run of every family writes into sentinel-guarded outputs with ldo > N; only what the entry point documents may change.

PATH -> CASES (paths(case) computes the tags from pm_dec_linear_plan's report; REQUIRED_PATHS lists them; the CPU test asserts both)
  dec_linear_kernel   MT 1 / 2 / 4, gridDim.z 1 / 2 / 3 / 4, NSTEP 4 / 8 (+ several trips) without LayerNorm, NSTEP 4 / 8 / 10 with it
                      (gamma / beta in registers at 4, through LDS at 8 and 10), K = 32 (three waves idle), N 1 / 15 / 16 / 17 / 130
                      (clamped weight rows, ragged tile), MT 2 / 4 under the default dispatch (nwg * mt > 512: N = 4112 / 2752, K = 32),
                      the LayerNorm refusal (mt > 2 and more than 4 K steps per wave)
  DL_QKV              H 1 / 3, Tmax 4 / 40, pos 0 / 1 / Tmax - 1, M 1 / 17
  DL_ARGMAX           FT 4 (K 32, 512), FT 2 with LayerNorm (K 544, 1280), M 1 / 17 / 33 (MT 4), bias through PRE_B and in-loop; persistent
                      <1, 8, 4> and <2, 8, 4> (N = 4040, M 1 / 16 / 17 / 32), a second tile per workgroup (N = 64 (CUs + 1) + 5, K = 32)
  K split             k_split 2 / 3 / 8, uneven parts (5 K steps over 3), K / 32 == k_split, both sides of nwg * mt * k_split <= 1024,
                      ld_parts > N, part_stride > M ld_parts, tickets zero afterwards, a second launch gives the same bits
  children            PM_DEC_ROWSPLIT=0 (MT 2 / 4 at small N), PM_DEC_LOGITS_PERSIST=0, PM_DEC_LOGITS_WAVES=4 (tests/decode_child.py)
  pm_dec_embed        B 1 / 4 / 5, d 8 / 512 / 520, token ids -1 and V (clamped), bit for bit
  argmax_reduce /     planted (ws_val, ws_idx): tiles 1 / 255 / 256 / 257 / 1024 / 1025, B 1 / 3 / 300 (many workgroups on one ticket: the
  next_token          position advances by one, the ticket returns to 0), prompt forcing on both sides of t + 1 = P, t + 1 = Ttot (no token, no
                      margin written), margin == top1 - best other tile winner as an fp32 subtraction, d 8 / 2048 / 2056 (the c != tid
                      re-load), forced ids outside [0, V)
  pm_dec_sample_topk  the splitmix64 draw in Python integers, top-k with ties to the lowest index, cumulative softmax in float64: the
                      sampled token EQUALS the reference's; seeds chosen so that the reference alone shows no draw within 1e-4 of a
                      boundary; k 1 / 2 / 64, V = k / 257 / 1000, -inf below the top k, ldl > V
  fused self block    pm_dec_attention_fused / _kv32 / _chain: pos 0 (only the LDS key) / 1 / 255 / 256 / 257 / 512, d 64 / 512 / 576 /
                      1024 / 1088 / 1280 (NCH 8 / 12 / 16 / 20 with nch < NCH, one projection at a time beyond 1024), H and B 1 / 3,
                      chain IN 0 / 1 / 8 / 9 / 17 / 64 parts with and without x_bias, OUT at d 512 (W_o early) and 1280 (at the tail);
                      needle: the decisive key is the newest (from LDS), key 0, key Lc - 1, 255, 256, or the only one

FUSED SELF BLOCK (bounds): the row x + x_bias + parts is formed in fp32 in the kernel's order and compared bit for bit;
q, k, v = LayerNorm -> an fp32 FMA chain: delta_q = sum |w| dxn + (d + 2) u (sum |w xn| + |b|); the stored k / v row: + half a bf16 ulp
(kv32: + u |want|), exactly row pos of each (b, h); the reference attends over the STORED row; |ds| <= sum |dq| |k| / 8 + 66 u sum |q k| / 8;
delta_att = 2 E A + (2 Lk + 4) u A with E = max |ds| + u max |s - m| + 2 u, A = sum_j p_j |v_j|; chain OUT: the heads summed in order
against att W_o^T by sum |datt| |w| + (64 + H + 2) u sum |att w|.
"""
from __future__ import annotations

import hashlib
import math
from dataclasses import dataclass

import torch

from attn_cases import bf16r
from linear_cases import MARGIN, _act64, act_bound, bits, ratio, store_term

U = 2.0 ** -24
EPS = 1e-5
PAD = 64  # sentinel elements in front of and behind every guarded view
SENT = {torch.float32: (torch.int32, 0x4B4B4B4B), torch.bfloat16: (torch.int16, 0x4B4B), torch.int32: (torch.int32, 0x4B4B4B4B),
        torch.int64: (torch.int64, 0x4B4B4B4B4B4B4B4B)}
NAN = {torch.float32: (torch.int32, 0x7FC00000), torch.bfloat16: (torch.int16, 0x7FC0)}
ACT_ID = {"none": 0, "gelu": 1, "approximate_gelu": 2}
MODE = {"linear": 0, "qkv": 1, "argmax": 2, "ksplit": 0, "kparts": 3}
ENVS = {"": {}, "rowsplit0": {"PM_DEC_ROWSPLIT": "0"}, "persist0": {"PM_DEC_LOGITS_PERSIST": "0"}, "waves4": {"PM_DEC_LOGITS_WAVES": "4"}}
MUTANTS = ("drop_lo", "drop_mid", "trunc_cache", "kv_row_off", "onepass", "act_after_resid", "bias_shift", "parts_missing", "tie_high",
           "embed_pos_row", "tail_pos_row", "no_forcing", "margin_top2", "newest_dropped")
TOK_OPS = ("reduce", "next", "sample")
NEXT_V = 1031  # vocabulary of the planted arg-max tails: more ids than tiles, so every tile winner is another embedding row
DEFAULT_CUS = 256  # what pm_dec_linear_plan assumes without a device; the GPU suite passes the device's count


# --------------------------------------------------------------------------------------------------------------- small helpers
def split3(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """csrc/decode.hip split3 on an fp32 tensor: three bf16 values (kept in fp32 storage), round to nearest even."""
    x = x.float()
    hi = bf16r(x)
    r1 = x - hi
    mid = bf16r(r1)
    lo = bf16r(r1 - mid)
    return hi, mid, lo


def trunc_bf16(v: torch.Tensor) -> torch.Tensor:
    """The deliberately wrong bf16 conversion: drop the low 16 bits."""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def digest(*ts: torch.Tensor) -> str:
    h = hashlib.sha1()
    for t in ts:
        h.update(bits(t.cpu()).numpy().tobytes())
    return h.hexdigest()


class Guarded:
    """A strided view in the middle of a buffer filled with a sentinel (outputs) or NaN (poisoned operands); the view starts 16-byte
    aligned.  intact(): every element outside the view still holds the fill."""

    def __init__(self, shape, strides, dtype, dev, table=SENT, init: torch.Tensor | None = None):
        idt, self.fill = table[dtype]
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        self.raw = torch.full((span + 2 * PAD,), self.fill, dtype=idt, device=dev)
        self.shape, self.strides = tuple(shape), tuple(strides)
        self.view = self.raw.view(dtype).as_strided(self.shape, self.strides, PAD)
        assert self.view.data_ptr() % 16 == 0
        if init is not None:
            self.view.copy_(init.to(dev))

    def intact(self) -> bool:
        r = self.raw.clone()
        r.as_strided(self.shape, self.strides, PAD).fill_(self.fill)
        return bool((r == self.fill).all())

    def reset(self):
        self.raw.fill_(self.fill)


def _ld(n: int, mult: int = 4) -> int:
    """A leading dimension > n, a multiple of `mult`."""
    return (n // mult + 2) * mult


# --------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    op: str  # linear | qkv | argmax | ksplit | kparts | embed
    family: str
    M: int
    N: int
    K: int
    ln: bool = False
    act: str = "none"
    bias: bool = False
    resid: bool = False
    k_split: int = 0
    H: int = 0
    Tmax: int = 0
    pos: int = 0
    env: str = ""  # the child process the case runs in ("" = the default dispatch)
    expect: tuple = ()  # (field, value) pairs of pm_dec_linear_plan's report the case is listed for
    refused: int = 0  # the error code the launcher must return instead of launching
    P: int = 0  # token tails (reduce / next / sample; there M = B, N = arg-max tiles or V, K = d): prompt length
    Ttot: int = 0
    topk: int = 0
    wild: bool = False  # the forced prompt token lies outside [0, V)
    kv32: bool = False  # fused self block (fself; M = B, N = 64 H, K = d, Tmax = cache length): float caches
    n_parts: int = -1  # -1: pm_dec_attention_fused[_kv32]; >= 0: pm_dec_attention_chain with that many parts on its IN side
    xbias: bool = False
    emit: bool = False  # chain OUT side: per-head partial sums of the output projection instead of att
    needle: int = -1  # needle family: the index of the decisive key (== pos: the newest, taken from LDS)

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.family}-M{self.M}-N{self.N}-K{self.K}"
        s += "-ln" if self.ln else ""
        s += f"-{self.act}" if self.act != "none" else ""
        s += "-b" if self.bias else ""
        s += "-r" if self.resid else ""
        s += f"-ks{self.k_split}" if self.k_split else ""
        s += f"-H{self.H}-T{self.Tmax}-p{self.pos}" if self.op == "qkv" else ""
        s += f"-t{self.pos}-P{self.P}-T{self.Ttot}" if self.op in TOK_OPS else ""
        s += f"-H{self.H}-T{self.Tmax}-p{self.pos}" if self.op == "fself" else ""
        s += "-kv32" if self.kv32 else ""
        s += f"-in{self.n_parts}" if self.n_parts >= 0 else ""
        s += "-xb" if self.xbias else ""
        s += "-emit" if self.emit else ""
        s += f"-key{self.needle}" if self.needle >= 0 else ""
        s += f"-k{self.topk}" if self.topk else ""
        s += "-wild" if self.wild else ""
        s += f"-{self.env}" if self.env else ""
        return s

    @property
    def tile(self) -> int:
        """features per arg-max tile (pm_dec_argmax_tile)"""
        return 32 if (self.K // 32 + 3) // 4 > 4 else 64

    @property
    def ntiles(self) -> int:
        return (self.N + self.tile - 1) // self.tile


def _seed(c: Case) -> int:
    return int(hashlib.sha1(f"{c.op}{c.family}{c.M}{c.N}{c.K}{c.ln}{c.act}{c.k_split}{c.H}{c.Tmax}{c.pos}{c.P}{c.Ttot}{c.topk}{c.kv32}{c.n_parts}{c.needle}".encode()).hexdigest()[:8], 16) & 0x7FFFFFFF


def persist2_N(cus: int, waves: int = 8) -> int:
    """The smallest N that gives one workgroup of the persistent kernel a second arg-max tile, ragged by 5 features."""
    return 64 * ((cus if waves == 8 else 2 * cus) + 1) + 5


def _c(op, fam, M, N, K, **kw) -> Case:
    return Case(op, fam, M, N, K, **kw)


def cases(cus: int = DEFAULT_CUS) -> list[Case]:
    L: list[Case] = []
    lin = lambda *a, **k: L.append(_c("linear", *a, **k))  # noqa: E731
    # ---- plain mode, no LayerNorm: row-tile edges x feature edges x K paths
    lin("exact", 1, 1, 32, expect=(("MT", 1), ("gz", 1), ("NSTEP", 4)))
    lin("exact", 15, 15, 32, bias=True)
    lin("exact", 16, 16, 128, resid=True)
    lin("exact", 17, 17, 160, bias=True, resid=True, expect=(("MT", 1), ("gz", 2)))
    lin("exact", 32, 130, 512, bias=True, expect=(("gz", 2), ("NSTEP", 4)))
    lin("exact", 33, 130, 544, resid=True, expect=(("gz", 3), ("NSTEP", 8)))
    lin("exact", 48, 16, 1024, bias=True, resid=True, expect=(("gz", 3), ("NSTEP", 8)))
    lin("exact", 49, 17, 2080, bias=True, expect=(("gz", 4), ("NSTEP", 8)))
    lin("exact", 64, 130, 2080, bias=True, resid=True, expect=(("gz", 4), ("NSTEP", 8)))
    lin("exact", 17, 4112, 32, bias=True, resid=True, expect=(("MT", 2), ("gz", 1)))
    lin("exact", 49, 2752, 32, bias=True, resid=True, expect=(("MT", 4), ("gz", 1)))
    lin("cancel", 17, 130, 160, act="gelu", bias=True, resid=True)
    lin("cancel", 33, 130, 1056, act="approximate_gelu", bias=True)
    lin("cancel", 64, 17, 2080, act="gelu", resid=True)
    lin("cancel", 1, 15, 1280, act="approximate_gelu", resid=True)
    lin("cancel", 49, 2752, 32, act="gelu", bias=True, resid=True, expect=(("MT", 4),))
    lin("scale", 17, 130, 160)
    lin("scale", 33, 17, 2080)
    lin("scale", 64, 130, 32)
    lin("poison", 17, 130, 160, act="gelu", bias=True, resid=True)
    lin("poison", 1, 15, 32, bias=True)
    lin("poison", 64, 130, 2080, resid=True)
    lin("perm", 33, 130, 160, bias=True, resid=True)
    lin("perm", 64, 130, 2080, act="gelu", resid=True)
    lin("perm", 17, 4112, 32, bias=True, expect=(("MT", 2),))
    # ---- fused LayerNorm: NSTEP 4 (gamma / beta in registers), 8 and 10 (through LDS)
    lin("cancel", 1, 130, 32, ln=True, bias=True, expect=(("NSTEP", 4), ("LN", 1)))
    lin("cancel", 16, 17, 128, ln=True, act="gelu", bias=True, resid=True)
    lin("cancel", 17, 130, 512, ln=True, act="approximate_gelu", bias=True, expect=(("NSTEP", 4), ("gz", 2)))
    lin("cancel", 32, 130, 544, ln=True, act="gelu", bias=True, expect=(("NSTEP", 8), ("gz", 2)))
    lin("cancel", 33, 16, 1024, ln=True, resid=True, expect=(("NSTEP", 8), ("gz", 3)))
    lin("cancel", 17, 130, 1056, ln=True, act="gelu", bias=True, resid=True, expect=(("NSTEP", 10),))
    lin("cancel", 32, 17, 1280, ln=True, bias=True, expect=(("NSTEP", 10),))
    lin("cancel", 64, 130, 1280, ln=True, act="approximate_gelu", expect=(("NSTEP", 10), ("gz", 4)))
    lin("cancel", 49, 130, 512, ln=True, bias=True, expect=(("gz", 4),))
    lin("cancel", 17, 4112, 32, ln=True, bias=True, expect=(("MT", 2), ("LN", 1)))
    lin("cancel", 49, 2752, 128, ln=True, bias=True, expect=(("MT", 4), ("LN", 1)))
    lin("offset", 17, 130, 160, ln=True, bias=True)
    lin("offset", 33, 17, 128, ln=True, act="gelu")
    lin("offset", 1, 17, 32, ln=True, resid=True)
    lin("offset", 64, 130, 192, ln=True, bias=True)
    lin("poison", 33, 17, 544, ln=True, act="gelu", bias=True, resid=True)
    lin("poison", 17, 130, 1280, ln=True, bias=True)
    lin("perm", 49, 17, 544, ln=True, bias=True)
    lin("perm", 33, 130, 128, ln=True, act="gelu", resid=True)
    lin("cancel", 49, 2752, 544, ln=True, refused=2)  # mt > 2 and 5 K steps per wave: PM_EUNSUPPORTED
    # ---- children: PM_DEC_ROWSPLIT=0 reaches MT 2 / 4 at small N
    lin("exact", 17, 130, 160, bias=True, resid=True, env="rowsplit0", expect=(("MT", 2), ("gz", 1)))
    lin("exact", 49, 17, 2080, bias=True, env="rowsplit0", expect=(("MT", 4), ("gz", 1), ("NSTEP", 4)))
    lin("cancel", 32, 130, 1280, ln=True, act="gelu", bias=True, env="rowsplit0", expect=(("MT", 2), ("NSTEP", 10)))
    lin("cancel", 33, 16, 128, ln=True, bias=True, resid=True, env="rowsplit0", expect=(("MT", 4), ("NSTEP", 4)))
    lin("perm", 64, 130, 544, act="gelu", resid=True, env="rowsplit0", expect=(("MT", 4),))
    lin("poison", 17, 17, 544, ln=True, bias=True, env="rowsplit0", expect=(("MT", 2), ("NSTEP", 8)))
    # ---- DL_QKV
    q = lambda fam, M, K, H, T, p, **k: L.append(_c("qkv", fam, M, 3 * 64 * H, K, H=H, Tmax=T, pos=p, **k))  # noqa: E731
    q("exact", 1, 128, 1, 4, 0, bias=True)
    q("exact", 17, 160, 3, 40, 1, bias=True)
    q("exact", 17, 32, 1, 4, 3, bias=True)
    q("cancel", 1, 512, 3, 40, 39, ln=True, bias=True)
    q("cancel", 17, 128, 1, 40, 0, ln=True, bias=True)
    q("cancel", 17, 1280, 3, 4, 1, ln=True)
    q("poison", 17, 160, 3, 4, 3, ln=True, bias=True)
    q("poison", 1, 544, 1, 40, 1, bias=True)
    q("perm", 17, 512, 3, 40, 39, ln=True, bias=True)
    # ---- DL_ARGMAX
    am = lambda M, N, K, **k: L.append(_c("argmax", "tie", M, N, K, **k))  # noqa: E731
    am(1, 300, 32, expect=(("kernel", "linear"), ("FT", 4)))
    am(17, 300, 512, bias=True, expect=(("kernel", "linear"), ("FT", 4), ("MT", 2)))
    am(33, 300, 32, bias=True, expect=(("FT", 4), ("MT", 4)))
    am(17, 300, 512, ln=True, bias=True, expect=(("kernel", "linear"), ("FT", 4), ("LN", 1)))
    am(33, 4040, 512, ln=True, bias=True, expect=(("kernel", "linear"), ("FT", 4), ("MT", 4)))
    am(1, 300, 544, ln=True, expect=(("FT", 2), ("NSTEP", 10)))
    am(17, 300, 1280, ln=True, bias=True, expect=(("FT", 2), ("MT", 2), ("NSTEP", 10)))
    pers = ((1, 512), (16, 128), (17, 128), (32, 512))
    for M, K in pers + ((17, 512),):
        am(M, 4040, K, ln=True, bias=M == 17, expect=(("kernel", "logits"), ("MT", 1 if M <= 16 else 2), ("waves", 8)))
    am(17, persist2_N(cus), 32, ln=True, expect=(("kernel", "logits"), ("gx", cus), ("tiles", cus + 2)))
    for M, K in pers:
        am(M, 4040, K, ln=True, bias=M == 17, env="persist0", expect=(("kernel", "linear"), ("FT", 4)))
        am(M, 4040, K, ln=True, bias=M == 17, env="waves4", expect=(("kernel", "logits"), ("waves", 4), ("FT", 2)))
    am(17, persist2_N(cus, 4), 32, ln=True, env="waves4", expect=(("kernel", "logits"), ("gx", 2 * cus), ("tiles", 2 * cus + 2)))
    am(17, persist2_N(cus, 4), 32, ln=True, env="persist0", expect=(("kernel", "linear"),))
    am(17, persist2_N(cus), 32, ln=True, env="persist0", expect=(("kernel", "linear"),))
    # ---- K split
    def ks(fam, M, N, K, split, expect=(), **kw):
        L.append(_c("ksplit", fam, M, N, K, k_split=split, expect=expect, **kw))
        L.append(_c("kparts", fam, M, N, K, k_split=split, expect=expect))  # the parts as they stand: no bias, activation, residual

    ks("exact", 1, 16, 64, 2, bias=True, resid=True, expect=(("gy", 2), ("gz", 1)))
    ks("exact", 17, 130, 160, 3, bias=True, resid=True, expect=(("gy", 3), ("gz", 2)))
    ks("exact", 33, 64, 256, 8, bias=True, expect=(("gy", 8), ("gz", 3)))
    ks("exact", 33, 2720, 96, 2, resid=True, expect=(("gz", 3), ("MT", 1)))
    ks("exact", 33, 2736, 96, 2, bias=True, resid=True, expect=(("gz", 1), ("MT", 4)))
    ks("cancel", 64, 130, 2080, 3, act="gelu", bias=True, resid=True, expect=(("gz", 4), ("NSTEP", 8)))
    ks("cancel", 17, 17, 2048, 8, act="approximate_gelu", bias=True, expect=(("gy", 8),))
    ks("poison", 17, 130, 160, 3, act="gelu", bias=True, resid=True)
    ks("perm", 33, 130, 544, 2, bias=True, resid=True)
    # ---- pm_dec_embed (M = B, N = V, K = d)
    for B, d in ((1, 8), (4, 512), (5, 520)):
        L.append(_c("embed", "exact", B, 37, d, pos=3))
        L.append(_c("embed", "poison", B, 37, d, pos=0))
    # ---- pm_dec_argmax_reduce / pm_dec_next_token on planted (ws_val, ws_idx): M = B, N = n_tiles, K = d
    tk = lambda op, fam, B, nt, d, t, P, T, **k: L.append(_c(op, fam, B, nt, d, pos=t, P=P, Ttot=T, **k))  # noqa: E731
    tk("next", "exact", 1, 1, 8, 0, 1, 4)  # one tile: no runner-up, the margin is +inf
    tk("next", "exact", 3, 255, 2048, 2, 4, 8)  # t + 1 < P: the prompt is forced
    tk("next", "exact", 3, 256, 2056, 3, 4, 8)  # t + 1 == P: the first free choice; d > 2048 re-loads the positional row
    tk("next", "exact", 300, 257, 8, 5, 4, 8)  # many workgroups on one ticket
    tk("next", "exact", 3, 1024, 8, 7, 4, 8)  # t + 1 == Ttot: no token, no margin written
    tk("next", "exact", 300, 1025, 2048, 1, 4, 8, wild=True)  # forced ids outside [0, V): stored as they are, embedded clamped
    tk("next", "poison", 3, 257, 2056, 4, 4, 8)
    tk("reduce", "exact", 1, 1, 0, 0, 1, 4)
    tk("reduce", "exact", 3, 256, 0, 1, 4, 8)
    tk("reduce", "exact", 300, 1025, 0, 5, 4, 8)
    tk("reduce", "exact", 3, 257, 0, 7, 4, 8)
    tk("reduce", "poison", 3, 1024, 0, 3, 4, 8)
    # ---- pm_dec_sample_topk: M = B, N = V, K = d
    for B, V, k, t in ((1, 1, 1, 0), (4, 2, 2, 3), (5, 64, 64, 5), (4, 257, 1, 4), (5, 257, 2, 3), (4, 257, 64, 6), (5, 1000, 64, 4), (1, 1000, 2, 9),
                       (4, 1000, 64, 1)):
        tk("sample", "exact" if V != 257 else "poison", B, V, 520 if V == 1000 else 8, t, 4, 12, topk=k)
    # ---- fused attention block, self form: M = B, N = 64 H, K = d
    fs = lambda fam, B, H, d, p, **k: L.append(_c("fself", fam, B, 64 * H, d, H=H, Tmax=p + 1 + (p % 3), pos=p, ln=True, bias=True, **k))  # noqa: E731
    for i, p in enumerate((0, 1, 255, 256, 257, 512)):  # only the LDS key; the 256-key group boundary; three groups
        d = (64, 512, 576, 1024, 1088, 1280)[i]  # NCH 8 / 8 / 12 / 16 / 20 (nch < NCH at 64, 576, 1088), one projection at a time beyond 1024
        fs("cancel", 3 if i % 2 else 1, 1 if i % 2 else 3, d, p)
        fs("cancel", 1 if i % 2 else 3, 3 if i % 2 else 1, (512, 1280, 64, 1088, 1024, 576)[i], p, kv32=i % 2 == 0, n_parts=(0, 1, 8, 9, 17, 64)[i],
           xbias=i % 2 == 1)
    fs("cancel", 3, 3, 512, 257, n_parts=8, xbias=True, emit=True)  # OUT side, W_o requested early
    fs("cancel", 1, 3, 1280, 256, n_parts=0, emit=True)  # OUT side, W_o requested at the tail
    fs("cancel", 3, 1, 1280, 1, n_parts=17, emit=True, kv32=True)
    fs("poison", 3, 3, 576, 257, n_parts=9, xbias=True)
    fs("poison", 1, 3, 1088, 0)
    fs("poison", 3, 1, 512, 256, n_parts=1, emit=True)
    for p, key in ((300, 300), (300, 0), (300, 299), (300, 255), (300, 256), (0, 0), (256, 255), (256, 256)):
        fs("needle", 3, 3, 512 if key % 2 else 1088, p, needle=key, kv32=key == 299)
    return L


CASES = cases()
REQUIRED_PATHS = frozenset(
    [f"linear:MT{m}" for m in (1, 2, 4)] + [f"linear:gz{z}" for z in (1, 2, 3, 4)] + ["linear:NSTEP4", "linear:NSTEP8", "linear:trips"]
    + [f"linear:LN{n}" for n in (4, 8, 10)] + ["linear:LN:MT2", "linear:LN:MT4", "linear:K32", "linear:refusal", "linear:default:MT2",
                                               "linear:default:MT4"]
    + [f"linear:N{n}" for n in (1, 15, 16, 17, 130)] + [f"linear:M{m}" for m in (1, 15, 16, 17, 32, 33, 48, 49, 64)]
    + [f"linear:act:{a}" for a in ACT_ID] + ["linear:bias", "linear:resid"]
    + ["qkv:H1", "qkv:H3", "qkv:T4", "qkv:T40", "qkv:pos0", "qkv:pos1", "qkv:poslast", "qkv:M1", "qkv:M17"]
    + ["argmax:FT4", "argmax:FT2", "argmax:MT4", "argmax:inloop_bias", "argmax:persist:MT1", "argmax:persist:MT2", "argmax:persist:tile2",
       "argmax:persist0", "argmax:waves4", "argmax:waves4:tile2"]
    + [f"ksplit:ks{s}" for s in (2, 3, 8)] + ["ksplit:uneven", "ksplit:ksteps==ks", "ksplit:rowsplit", "ksplit:norowsplit", "kparts:ks3"]
    + ["embed:B1", "embed:B4", "embed:B5", "embed:d8", "embed:d512", "embed:d520"]
    + [f"next:tiles{n}" for n in (1, 255, 256, 257, 1024, 1025)] + [f"next:B{b}" for b in (1, 3, 300)] + [f"next:d{d}" for d in (8, 2048, 2056)]
    + ["next:forced", "next:first_free", "next:free", "next:end", "next:wild", "reduce:tiles1", "reduce:tiles1025", "reduce:B300", "reduce:end"]
    + [f"fself:pos{p}" for p in (0, 1, 255, 256, 257, 512)] + [f"fself:d{d}" for d in (64, 512, 576, 1024, 1088, 1280)]
    + ["fself:H1", "fself:H3", "fself:B1", "fself:B3", "fself:kv32", "fself:fused", "fself:chain", "fself:xbias", "fself:emit:early", "fself:emit:tail"]
    + [f"fself:in{n}" for n in (0, 1, 8, 9, 17, 64)] + ["fself:needle:newest", "fself:needle:first", "fself:needle:last", "fself:needle:255",
                                                        "fself:needle:256", "fself:needle:only"]
    + [f"sample:k{k}" for k in (1, 2, 64)] + [f"sample:V{v}" for v in ("k", 257, 1000)] + ["sample:forced", "sample:free"])


def plan_args(c: Case) -> dict:
    return dict(M=c.M, N=c.N, K=c.K, ln=c.ln, mode=MODE[c.op], k_split=c.k_split)


def paths(c: Case, rep: dict) -> set[str]:
    """The path tags a case reaches, from pm_dec_linear_plan's report `rep` (ops.dec_linear_plan) of its launch."""
    if c.op == "embed":
        return {f"embed:B{c.M}", f"embed:d{c.K}"}
    if c.op in ("next", "reduce"):
        t1 = c.pos + 1
        when = "end" if t1 == c.Ttot else "forced" if t1 < c.P else "first_free" if t1 == c.P else "free"
        return {f"{c.op}:tiles{c.N}", f"{c.op}:B{c.M}", f"{c.op}:d{c.K}", f"{c.op}:{when}"} | ({f"{c.op}:wild"} if c.wild else set())
    if c.op == "fself":
        t = {f"fself:pos{c.pos}", f"fself:d{c.K}", f"fself:H{c.H}", f"fself:B{c.M}", "fself:chain" if c.n_parts >= 0 else "fself:fused"}
        t |= {"fself:kv32"} if c.kv32 else set()
        t |= {f"fself:in{c.n_parts}"} if c.n_parts >= 0 else set()
        t |= {"fself:xbias"} if c.xbias else set()
        t |= {"fself:emit:early" if c.K <= 512 else "fself:emit:tail"} if c.emit else set()
        if c.needle >= 0:
            t.add("fself:needle:" + ("only" if c.pos == 0 else "newest" if c.needle == c.pos else "first" if c.needle == 0 else
                                     "last" if c.needle == c.pos - 1 else str(c.needle)))
        return t
    if c.op == "sample":
        return {f"sample:k{c.topk}", f"sample:V{'k' if c.N == c.topk else c.N}", "sample:forced" if c.pos + 1 < c.P else "sample:free"}
    if c.refused:
        return {"linear:refusal"} if rep.get("refused") == c.refused else set()
    t = set()
    per_wave = (c.K // 32 + 3) // 4
    if c.op == "linear":
        t |= {f"linear:MT{rep['MT']}", f"linear:gz{rep['gz']}", f"linear:N{c.N}", f"linear:M{c.M}", f"linear:act:{c.act}"}
        t |= {"linear:bias"} if c.bias else set()
        t |= {"linear:resid"} if c.resid else set()
        t |= {"linear:K32"} if c.K == 32 else set()
        if rep["LN"]:
            t |= {f"linear:LN{rep['NSTEP']}"} | ({f"linear:LN:MT{rep['MT']}"} if rep["MT"] > 1 else set())
        else:
            t |= {f"linear:NSTEP{rep['NSTEP']}"} | ({"linear:trips"} if per_wave > rep["NSTEP"] else set())
        if not c.env and rep["MT"] > 1:
            t.add(f"linear:default:MT{rep['MT']}")
    elif c.op == "qkv":
        t |= {f"qkv:H{c.H}", f"qkv:T{c.Tmax}", f"qkv:M{c.M}", "qkv:poslast" if c.pos == c.Tmax - 1 else f"qkv:pos{c.pos}"}
    elif c.op == "argmax":
        if rep["kernel"] == "logits":
            tag = "argmax:persist" if rep["waves"] == 8 else "argmax:waves4"
            t |= {f"{tag}:MT{rep['MT']}"} if rep["waves"] == 8 else {tag}
            t |= {f"{tag}:tile2"} if rep["tiles"] > rep["gx"] else set()
        else:
            t |= {f"argmax:FT{rep['FT']}"} | ({"argmax:MT4"} if rep["MT"] == 4 else set()) | ({"argmax:persist0"} if c.env == "persist0" else set())
            t |= {"argmax:inloop_bias"} if c.bias and rep["FT"] * rep["MT"] > 8 else set()
    else:
        ksteps = c.K // 32
        t |= {f"{c.op}:ks{c.k_split}"}
        if c.op == "ksplit":
            t |= {"ksplit:uneven"} if ksteps % c.k_split else set()
            t |= {"ksplit:ksteps==ks"} if ksteps == c.k_split else set()
            t |= {"ksplit:rowsplit"} if rep["gz"] > 1 else ({"ksplit:norowsplit"} if c.M > 16 else set())
    return t


# --------------------------------------------------------------------------------------------------------------- inputs
def _exact_x(g, M, K):
    amp = int(min(4095, 2 ** 22 // K))
    x = torch.randint(-amp, amp + 1, (M, K), generator=g).double()
    x = x * (torch.rand(M, K, generator=g) < 0.5)
    big = torch.randint(2 ** 18, 2 ** 20, (64 * M + 64,), generator=g) | 1
    big = big[split3(big.float())[2] != 0].tolist()  # 19 - 20 significant bits whose lo term is not zero
    for m in range(M):  # three such entries per row, at positions that differ from row to row
        for k in torch.randperm(K, generator=g)[:3].tolist():
            x[m, k] = float(big.pop() * (1 if (m + k) % 2 else -1))
    return x.float()


def _exact_w(N, K):
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return (((n * 7 + k * 3 + (n * k) % 5) % 5) - 2).to(torch.bfloat16)


def tie_layout(c: Case, cus: int = DEFAULT_CUS) -> tuple[dict[int, tuple[int, float]], list[tuple[int, int]]]:
    """({tile: (planted winner row, alpha)}, [(source, copy)]) of the tie family.  Every copy is a bit-identical weight row at a HIGHER
    index that must lose: tile 0's winner again in the same 16-feature tile on another kq lane (1 -> 9); tile 1's in the adjacent
    16-feature tile (T + 5 -> T + 21); the winner over ALL tiles (the top alpha: tile 2, or tile 1 where the persistent kernel's
    workgroup 1 also walks the last tile) twice in the ragged last tile (+1, +3).  The alphas are distinct otherwise."""
    T, nt, N = c.tile, c.ntiles, c.N
    last0 = (nt - 1) * T
    top = 1 if N in (persist2_N(cus), persist2_N(cus, 4)) else 2
    win = {}
    for t in range(nt):
        width = min(T, N - t * T)
        win[t] = (t * T + (7 * t + 1) % width, 1.0 + ((t * 37) % nt) / nt)
    win[0] = (1, win[0][1])
    win[1] = (T + 5, win[1][1])
    win[2] = (2 * T + 3, win[2][1])
    win[top] = (win[top][0], 2.5)
    plants = [(1, 9), (T + 5, T + 21), (win[top][0], last0 + 1)]
    if N - last0 >= 4:
        plants.append((win[top][0], last0 + 3))
    assert nt >= 4 and all(b_ < N for _, b_ in plants)
    return win, plants


def build(c: Case, cus: int = DEFAULT_CUS) -> dict:
    g = torch.Generator().manual_seed(_seed(c))
    M, N, K = c.M, c.N, c.K
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp: dict = {}
    if c.op in TOK_OPS:
        return _tok_build(c, g)
    if c.op == "fself":
        return _fs_build(c, g)
    if c.op == "embed":
        B, V, d = M, N, K
        inp["emb"] = bf16r(rn(V, d)).to(torch.bfloat16)
        inp["postab"] = rn(c.pos + 2, d)
        tok = torch.randint(0, V, (B,), generator=g)
        tok[0] = -1 if B > 1 else V  # clamped to 0 / V - 1
        if B > 1:
            tok[-1] = V
        inp["tok"] = tok.long()
        return inp
    if c.family == "exact":
        x, w = _exact_x(g, M, K), _exact_w(N, K)
        bias = torch.randint(-1000, 1001, (N,), generator=g).float() if c.bias else None
        resid = torch.randint(-1000, 1001, (M, N), generator=g).float() if c.resid else None
        if c.op == "qkv":  # plant exact bf16 ties in row 0 of every fifth k / v column through the bias
            z0 = x[0].double() @ w.double().T
            inner = 64 * c.H
            ties = (258.0, 262.0, 774.0, 1028.0, 1036.0, 3080.0, 65792.0)  # halfway between two bf16 values, both parities
            for j, col in enumerate(range(inner, 3 * inner, 5)):
                bias[col] = float(ties[j % len(ties)] * (1 if j % 2 else -1) - z0[col])
    else:
        w = bf16r(rn(N, K) * K ** -0.5)
        if c.family == "cancel":
            w[:, K // 2:] = -w[:, : K // 2]
            x = 1.0 + 2.0 ** -6 * rn(M, K)
        elif c.family == "offset":
            x = 4096.0 + rn(M, K)
        elif c.family == "scale":
            x = rn(M, K)
            w = bf16r(torch.sign(rn(N, K)) * torch.exp2(torch.rand(N, K, generator=g) * 5 - 4))
        elif c.family == "tie":
            x0 = rn(K) + 0.25  # (a mean and a spread: LayerNorm changes the direction)
            x = x0[None] + 0.05 * rn(M, K) * x0.abs().mean()
            w = bf16r(rn(N, K) * 0.02 * K ** -0.5)
        else:
            x = rn(M, K) * 2
        w = w.to(torch.bfloat16)
        bias = 0.1 * rn(N) if c.bias else None
        resid = rn(M, N) if c.resid else None
    inp.update(x=x.float().contiguous(), w=w.contiguous(), bias=bias, resid=resid)
    if c.ln:
        inp["gamma"], inp["beta"] = 1.0 + 0.1 * rn(K), 0.1 * rn(K)
    if c.family == "tie":
        xn = (_ln64(x.double(), inp["gamma"].double(), inp["beta"].double())[0] if c.ln else x.double())[0]
        dirn = xn / xn.norm()
        w = inp["w"].float()
        win, plants = tie_layout(c, cus)
        for col, alpha in win.values():
            w[col] = bf16r((alpha * 0.5 * dirn).float())
        for a, b in plants:
            w[b] = w[a]
            if bias is not None:
                bias[b] = bias[a]
        inp["plants"] = plants
        inp["w"] = w.to(torch.bfloat16)
    if c.op == "qkv":
        inp["kc0"] = bf16r(rn(M, c.H, c.Tmax, 64)).to(torch.bfloat16)
        inp["vc0"] = bf16r(rn(M, c.H, c.Tmax, 64)).to(torch.bfloat16)
    return inp


# --------------------------------------------------------------------------------------------------------------- reference
def _ln64(x, g, b):
    mu = x.mean(-1, keepdim=True)
    sig = (((x - mu) ** 2).mean(-1, keepdim=True) + EPS).sqrt()
    xh = (x - mu) / sig
    return xh * g + b, xh, sig


def kpart_ranges(K: int, ks: int) -> list[tuple[int, int]]:
    n = K // 32
    return [(32 * (n * p // ks), 32 * (n * (p + 1) // ks)) for p in range(ks)]


def _aprime(xn: torch.Tensor, w64: torch.Tensor, k0: int = 0, k1: int | None = None) -> torch.Tensor:
    hi, mid, lo = split3(xn.float())
    s = (hi.double().abs() + mid.double().abs() + lo.double().abs())[:, k0:k1]
    return s @ w64.abs()[:, k0:k1].T


def reference(c: Case, inp: dict) -> dict:
    """name -> (want float64, bound float64) per float output; 'int:' names -> exact integer tensors."""
    if c.op in TOK_OPS:
        return _tok_reference(c, inp)
    if c.op == "fself":
        return _fs_reference(c, inp)
    if c.op == "embed":
        tok = inp["tok"].clamp(0, c.N - 1)
        want = (inp["emb"].float()[tok] + inp["postab"][c.pos]).double()  # one fp32 addition: the reference does it in fp32 too
        return {"x": (want, torch.zeros_like(want))}
    M, N, K = c.M, c.N, c.K
    x, w = inp["x"].double(), inp["w"].double()
    b = inp["bias"].double() if inp["bias"] is not None else torch.zeros(N, dtype=torch.float64)
    cc = 3 + 1 + c.k_split
    if c.ln:
        xn, xh, sig = _ln64(x, inp["gamma"].double(), inp["beta"].double())
        e = K * U * x.abs().mean(-1, keepdim=True)
        dxn = inp["gamma"].double().abs() / sig * (2 + xh.abs()) * e + 3 * U * xn.abs()
        lnterm = dxn @ w.abs().T
    else:
        xn, lnterm = x, 0.0
    z = xn @ w.T + b
    for a_, b_ in inp.get("plants", ()):  # identical rows: identical logits, whatever the float64 product's blocking does at its edges
        assert torch.equal(w[a_], w[b_]) and b[a_] == b[b_]
        z[:, b_] = z[:, a_]
    A = _aprime(xn, w) + b.abs()
    dz = lnterm + (3 * K + cc) * U * A
    out: dict = {"z": (z, dz)}
    if c.op == "kparts":
        zs, bs = [], []
        for k0, k1 in kpart_ranges(K, c.k_split):
            zs.append(xn[:, k0:k1] @ w[:, k0:k1].T)
            bs.append((3 * (k1 - k0) + 3) * U * _aprime(xn, w, k0, k1) + U * zs[-1].abs())
        out["parts"] = (torch.stack(zs), torch.stack(bs))
        return out
    if c.op in ("linear", "ksplit"):
        gact = _act64(z, c.act)
        y = gact + (inp["resid"].double() if c.resid else 0.0)
        bd = act_bound(z, gact, dz, c.act, False) + (U * y.abs() if c.resid else 0.0) + U * y.abs()
        out["out"] = (y, bd)
    elif c.op == "qkv":
        inner = 64 * c.H
        out["out"] = (z[:, :inner], dz[:, :inner] + U * z[:, :inner].abs())
        for name, lo_ in (("k", inner), ("v", 2 * inner)):
            zz, dd = z[:, lo_: lo_ + inner].reshape(M, c.H, 64), dz[:, lo_: lo_ + inner].reshape(M, c.H, 64)
            out[name] = (zz, dd + store_term(zz.abs() + dd, "bf16"))
    elif c.op == "argmax":
        T, nt = c.tile, c.ntiles
        zp = torch.full((M, nt * T), -math.inf, dtype=torch.float64)
        zp[:, :N] = z
        dp = torch.zeros(M, nt * T, dtype=torch.float64)
        dp[:, :N] = dz + U * z.abs()
        zt, dt = zp.view(M, nt, T), dp.view(M, nt, T)
        best = zt.max(-1)
        out["ws_val"] = (best.values, dt.max(-1).values)
        out["int:ws_idx"] = (best.indices + torch.arange(nt)[None] * T).int()  # max() returns the FIRST maximal index: the lowest
        out["tiles"] = (zt, dt)
    return out


def tie_preconditions(c: Case, ref: dict) -> dict:
    """Every arg-max tile: the logits equal to the winner are the planted copies only, every other one sits >= 4 x the bound below."""
    zt, dt = ref["tiles"]
    best = zt.max(-1, keepdim=True).values
    tied = zt == best
    others = torch.where(tied, torch.full_like(zt, -math.inf), zt)
    gap = best.squeeze(-1) - others.max(-1).values
    need = 4 * dt.max(-1).values
    plants = tie_layout(c)[1]
    n_tied_tiles = int((tied.sum(-1) > 1).all(0).sum())
    glob = ref["ws_val"][0]
    gbest = glob.max(-1, keepdim=True).values
    ggap = gbest.squeeze(-1) - torch.where(glob == gbest, torch.full_like(glob, -math.inf), glob).max(-1).values
    return dict(decisive=bool((gap >= need).all()), min_gap_over_need=float((gap / need).min()), plants=len(plants), tied_tiles=n_tied_tiles,
                global_decisive=bool((ggap >= 4 * ref["ws_val"][1].max(-1).values).all()), global_tied=int((glob == gbest).sum(-1).min()))


def exact_preconditions(c: Case, inp: dict, ref: dict) -> dict:
    x, w = inp["x"].double(), inp["w"].double()
    A = _aprime(inp["x"], w) + (inp["bias"].double().abs() if inp["bias"] is not None else 0.0) + (inp["resid"].double().abs() if c.resid else 0.0)
    _, mid, lo = split3(inp["x"])
    pre = dict(limit=float(A.max()), integral=bool((x == x.round()).all()), mid_share=float((mid != 0).double().mean()),
               lo_rows=bool((lo != 0).any(-1).all()), zeros=float((x == 0).double().mean()),
               w_varies=bool((w[1:] != w[:-1]).any(1).all() if c.N > 1 else True) and bool((w[:, 1:] != w[:, :-1]).any()))
    if c.op == "qkv":
        inner = 64 * c.H
        kv = ref["z"][0][:, inner:]
        _, ex = torch.frexp(kv.abs())
        q = torch.ldexp(torch.ones_like(kv), ex - 8)  # the bf16 spacing at each value
        pre["wide_share"] = float(((kv / q) != (kv / q).round()).double().mean())  # more than 8 significant bits
        frac = (kv / q) - (kv / q).floor()
        pre["ties"] = int((frac == 0.5).sum())
        half_up = ((kv / q).floor() + 1) * q
        pre["ties_even_down"] = int(((frac == 0.5) & (bf16r(kv.float()).double() != half_up)).sum())  # where round-half-up is wrong
    return pre


def scale_preconditions(c: Case, inp: dict) -> dict:
    lo_, hi_ = math.inf, 0.0
    wabs = inp["w"].double().abs()
    for k in (-40, 0, 40):
        for t in split3(inp["x"] * 2.0 ** k):
            nz = t.double().abs()[t != 0]
            lo_, hi_ = min(lo_, float(nz.min()) * float(wabs[wabs > 0].min())), max(hi_, float(nz.max()) * float(wabs.max()) * c.K * 3)
            lo_ = min(lo_, float(nz.min()))
    return dict(lo=lo_, hi=hi_, ok=lo_ >= 2.0 ** -90 and hi_ <= 2.0 ** 100)


# --------------------------------------------------------------------------------------------------------------- placement
def _operand(t: torch.Tensor | None, dev, poison: bool, ld: int | None = None):
    """The tensor on `dev`: as it is, or (poison) as the 16-byte aligned middle of a NaN-filled buffer with row stride ld."""
    if t is None:
        return None
    if not poison:
        return t.to(dev).contiguous()
    strides = (1,) if t.dim() == 1 else (ld, 1)
    return Guarded(t.shape, strides, t.dtype, dev, table=NAN, init=t).view


def place(c: Case, inp: dict, dev="cpu", poison: bool = False, perm: torch.Tensor | None = None, scale: float = 1.0) -> dict:
    M, N, K = c.M, c.N, c.K
    P: dict = {"poison": poison, "g": {}, "dev": dev}
    G = P["g"]
    if c.op in TOK_OPS:
        return _tok_place(c, inp, P, dev, poison)
    if c.op == "fself":
        return _fs_place(c, inp, P, dev, poison)
    if c.op == "embed":
        P["emb"], P["postab"] = _operand(inp["emb"], dev, poison, K), _operand(inp["postab"], dev, poison, K)
        P["tok"] = inp["tok"].to(dev)
        P["posv"] = torch.tensor([c.pos], dtype=torch.int32, device=dev)
        G["x"] = Guarded((M, K), (K, 1), torch.float32, dev)  # (x rows are d apart: the entry point has no leading dimension)
        return P
    x = inp["x"] * scale
    resid = inp["resid"]
    if perm is not None:
        x, resid = x[perm], (resid[perm] if resid is not None else None)
    P["x"] = _operand(x, dev, poison, K + 8)
    P["w"] = _operand(inp["w"], dev, poison, K + 16)
    P["bias"] = _operand(inp["bias"], dev, poison)
    P["resid"] = _operand(resid, dev, poison, N + 3)
    P["gamma"], P["beta"] = (_operand(inp["gamma"], dev, poison), _operand(inp["beta"], dev, poison)) if c.ln else (None, None)
    if c.op in ("linear", "ksplit"):
        G["out"] = Guarded((M, N), (_ld(N), 1), torch.float32, dev)
    if c.op == "ksplit":
        nt, mt = (N + 15) // 16, (M + 15) // 16
        mt = 1 if mt <= 1 else 2 if mt == 2 else 4
        P["ws"] = torch.empty(nt * c.k_split * mt * 256, dtype=torch.float32, device=dev)
        G["tickets"] = Guarded((nt * 4,), (1,), torch.int32, dev, init=torch.zeros(nt * 4, dtype=torch.int32))
    if c.op == "kparts":
        ldp = _ld(N)
        G["parts"] = Guarded((c.k_split, M, N), (M * ldp + 8, ldp, 1), torch.float32, dev)
    if c.op == "qkv":
        inner = 64 * c.H
        G["out"] = Guarded((M, inner), (_ld(inner), 1), torch.float32, dev)
        kc0, vc0 = (inp["kc0"][perm], inp["vc0"][perm]) if perm is not None else (inp["kc0"], inp["vc0"])
        st = (c.H * c.Tmax * 64, c.Tmax * 64, 64, 1)
        G["kc"] = Guarded(kc0.shape, st, torch.bfloat16, dev, init=kc0)
        G["vc"] = Guarded(vc0.shape, st, torch.bfloat16, dev, init=vc0)
        P["posv"] = torch.tensor([c.pos], dtype=torch.int32, device=dev)
    if c.op == "argmax":
        nt = c.ntiles
        G["ws_val"] = Guarded((M, nt), (nt, 1), torch.float32, dev)
        G["ws_idx"] = Guarded((M, nt), (nt, 1), torch.int32, dev)
    return P


def _p(t):
    return None if t is None else t.data_ptr()


def run(L, c: Case, P: dict) -> int:
    """The C entry point on the placement; returns its status."""
    G = P["g"]
    if c.op in TOK_OPS:
        return _tok_run(L, c, P)
    if c.op == "fself":
        return _fs_run(L, c, P)
    if c.op == "embed":
        return L.pm_dec_embed(_p(P["tok"]), _p(P["emb"]), _p(P["postab"]), _p(P["posv"]), _p(G["x"].view), c.M, c.K, c.N, None)
    x, w, r = P["x"], P["w"], P["resid"]
    ldr = r.stride(0) if r is not None else 0
    if c.op == "ksplit":
        o = G["out"].view
        return L.pm_dec_linear_ksplit(_p(x), x.stride(0), _p(w), w.stride(0), _p(P["bias"]), _p(r), ldr, _p(o), o.stride(0), c.M, c.N, c.K,
                                      ACT_ID[c.act], c.k_split, _p(P["ws"]), _p(G["tickets"].view), None)
    if c.op == "kparts":
        o = G["parts"].view
        return L.pm_dec_linear_kparts(_p(x), x.stride(0), _p(w), w.stride(0), _p(o), o.stride(1), o.stride(0), c.M, c.N, c.K, c.k_split, None)
    o = G["out"].view if "out" in G else None
    kc, vc = (G["kc"].view, G["vc"].view) if c.op == "qkv" else (None, None)
    wv, wi = (G["ws_val"].view, G["ws_idx"].view) if c.op == "argmax" else (None, None)
    return L.pm_dec_linear(_p(x), x.stride(0), _p(P["gamma"]), _p(P["beta"]), EPS, _p(w), w.stride(0), _p(P["bias"]), _p(r), ldr, _p(o),
                           o.stride(0) if o is not None else 0, c.M, c.N, c.K, ACT_ID[c.act], MODE[c.op], _p(kc), _p(vc), 64 * c.H, c.H, c.Tmax,
                           _p(P.get("posv")), _p(wv), _p(wi), None)


def abi_refusal(c: Case, P: dict) -> str | None:
    """Why the entry point would refuse this placement before launching (None: it launches) - the launchers' own checks."""
    if c.op == "embed" or c.op in TOK_OPS:
        return "d % 8" if c.K % 8 else None
    if c.op == "fself":
        return "d % 64, d > 1280 or the cache is too short" if c.K % 64 or c.K > 1280 or c.pos >= c.Tmax or c.Tmax > 4096 else None
    x, w = P["x"], P["w"]
    if c.M > 64 or c.K % 32:
        return "M > 64 or K % 32"
    if x.stride(0) < c.K or w.stride(0) < c.K or x.stride(0) % 4 or w.stride(0) % 8 or (x.data_ptr() | w.data_ptr()) & 15:
        return "x / w strides or alignment"
    if c.ln and ((P["gamma"].data_ptr() | P["beta"].data_ptr()) & 15 or c.K > 1280):
        return "gamma / beta alignment or K > 1280"
    if c.k_split and (c.k_split < 2 or c.k_split > 8 or c.K // 32 < c.k_split):
        return "k_split"
    if c.op == "kparts":
        o = P["g"]["parts"].view
        if o.data_ptr() & 15 or o.stride(1) % 4 or o.stride(0) % 4 or o.stride(0) < c.M * o.stride(1):
            return "parts layout"
    return None


# --------------------------------------------------------------------------------------------------------------- the CPU stand-in
def _act32(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "gelu":
        return torch.nn.functional.gelu(z)
    if act == "approximate_gelu":
        return torch.nn.functional.gelu(z, approximate="tanh")
    return z


def emulate(c: Case, P: dict, mutant: str | None = None) -> int:
    """A correct kernel in fp32 torch with its own summation order (three fp32 matmuls over the explicit split3 terms, then the
    epilogue in the kernel's order), writing where the kernel writes; `mutant` plants one of MUTANTS."""
    G = P["g"]
    if c.op in TOK_OPS:
        return _tok_emulate(c, P, mutant)
    if c.op == "fself":
        return _fs_emulate(c, P, mutant)
    if c.op == "embed":
        tok = P["tok"].clamp(0, c.N - 1)
        row = c.pos - 1 if mutant == "embed_pos_row" and c.pos > 0 else c.pos
        G["x"].view.copy_(P["emb"].float()[tok] + P["postab"][row])
        return 0
    x = P["x"].float()
    w = P["w"].float()
    if c.ln:
        mu = x.mean(-1, keepdim=True)
        var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp_min(0) if mutant == "onepass" else ((x - mu) ** 2).mean(-1, keepdim=True)
        x = (x - mu) * torch.rsqrt(var + EPS) * P["gamma"] + P["beta"]
    hi, mid, lo = split3(x)
    terms = [hi] + ([mid] if mutant != "drop_mid" else []) + ([lo] if mutant != "drop_lo" else [])

    def prod(k0=0, k1=None):
        acc = torch.zeros(c.M, c.N)
        for t in terms:
            if c.family == "perm":  # row by row: a blocked matrix product need not give a row the same bits at another place
                acc = acc + torch.stack([w[:, k0:k1] @ t[m, k0:k1] for m in range(c.M)])
            else:
                acc = acc + t[:, k0:k1] @ w[:, k0:k1].T
        return acc

    if c.op == "kparts":
        for p, (k0, k1) in enumerate(kpart_ranges(c.K, c.k_split)):
            G["parts"].view[p].copy_(prod(k0, k1))
        return 0
    if c.k_split:
        z = torch.zeros(c.M, c.N)
        rng = kpart_ranges(c.K, c.k_split)
        for k0, k1 in (rng[:-1] if mutant == "parts_missing" else rng):
            z = z + prod(k0, k1)
    else:
        z = prod()
    if P["bias"] is not None:
        z = z + (P["bias"].roll(1) if mutant == "bias_shift" else P["bias"])
    if c.op in ("linear", "ksplit"):
        r = P["resid"]
        if mutant == "act_after_resid" and r is not None:
            y = _act32(z + r, c.act)
        else:
            y = _act32(z, c.act) + (r if r is not None else 0.0)
        G["out"].view.copy_(y)
    elif c.op == "qkv":
        inner = 64 * c.H
        G["out"].view.copy_(z[:, :inner])
        row = c.pos if mutant != "kv_row_off" else (c.pos + 1 if c.pos + 1 < c.Tmax else c.pos - 1)
        for name, lo_ in (("kc", inner), ("vc", 2 * inner)):
            v = z[:, lo_: lo_ + inner].reshape(c.M, c.H, 64)
            G[name].view[:, :, row] = trunc_bf16(v) if mutant == "trunc_cache" else v.to(torch.bfloat16)
    elif c.op == "argmax":
        T, nt = c.tile, c.ntiles
        zp = torch.full((c.M, nt * T), -math.inf)
        zp[:, : c.N] = z
        zt = zp.view(c.M, nt, T)
        if mutant == "tie_high":
            idx = T - 1 - zt.flip(-1).max(-1).indices
            val = zt.max(-1).values
        else:
            val, idx = zt.max(-1)
        G["ws_val"].view.copy_(val)
        G["ws_idx"].view.copy_((idx + torch.arange(nt)[None] * T).int())
    return 0


# --------------------------------------------------------------------------------------------------------------- the token tails
def ds_uniform(seed: int, t: int, b: int) -> tuple[int, float]:
    """pm_dec_sample_topk's draw in Python integers: (the 24-bit integer, u = it / 2^24 in [0, 1), exact)."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (t + 1) + 0xBF58476D1CE4E5B9 * (b + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z >> 40, (z >> 40) / 16777216.0


def _tok_V(c: Case) -> int:
    return c.N if c.op == "sample" else NEXT_V


def _topk_order(row: torch.Tensor, k: int) -> list[int]:
    """The k largest in the order (value descending, index ascending), by an explicit sort key."""
    return sorted(range(row.numel()), key=lambda i: (-float(row[i]), i))[:k]


def sample_pick(c: Case, logits: torch.Tensor, seed: int) -> tuple[list[int], float]:
    """(the reference's token per sequence, the smallest |u - boundary| / 1 over all draws): top-k in float64, cumulative softmax in float64."""
    toks, near = [], math.inf
    for b in range(c.M):
        order = _topk_order(logits[b], c.topk)
        v = logits[b][order].double()
        cum = torch.cumsum(torch.exp(v - v[0]), 0)
        u = ds_uniform(seed, c.pos, b)[1]
        edges = cum / cum[-1]
        near = min(near, float((edges[:-1] - u).abs().min()) if c.topk > 1 else math.inf)
        pick = int((u * float(cum[-1]) < cum).nonzero()[0]) if bool((u * float(cum[-1]) < cum).any()) else c.topk - 1
        toks.append(order[pick])
    return toks, near


def _tok_build(c: Case, g) -> dict:
    B, d, V = c.M, c.K, _tok_V(c)
    inp: dict = {}
    prompt = torch.randint(0, V, (B, c.P), generator=g)
    if c.wild:
        prompt[::2] = -5
        prompt[1::2] = V + 10
    inp["prompt"] = prompt.long()
    if c.op != "reduce":
        inp["emb"] = bf16r(torch.randn(V, d, generator=g)).to(torch.bfloat16)
        inp["postab"] = torch.randn(c.Ttot + 1, d, generator=g)
    if c.op == "sample":
        lg = torch.randn(B, V, generator=g) * 2
        if V >= 257:
            lg[:, 5::7] = -math.inf  # entries far below the top k (at least k stay finite)
            lg[:, 11] = lg[:, 200]  # an exact tie, usually inside the top 64: the lower index goes first
            lg[:, 3] = lg[:, 250] = lg.max() + 1.0  # and one at the very top
        inp["logits"] = lg
        for seed in range(1000, 1400):  # the first seed whose draws all stay clear of a cumulative boundary (the reference alone decides)
            if sample_pick(c, lg, seed)[1] > 1e-3:
                break
        inp["seed"] = seed
        return inp
    nt = c.N
    inp["ws_val"] = torch.randint(0, 24, (B, nt), generator=g).float() / 8 - 1  # few distinct values: ties between tiles in most rows
    if nt > 4:
        inp["ws_val"][:, 3] = -math.inf
        inp["ws_val"][0, nt // 2:] = inp["ws_val"][0].max()  # half the tiles tie at the top: the margin is 0
    inp["ws_idx"] = torch.stack([torch.randperm(NEXT_V, generator=g)[:nt] for _ in range(B)]).int()
    return inp


def _tok_reference(c: Case, inp: dict) -> dict:
    """Every output of the launch as the tensor it must hold afterwards (compared as integers): tok_cur, tokens_out, margin_out, x, pos,
    ticket.  tokens_out starts at -7, margin_out at 123: only column t + 1 may change, and nothing when t + 1 == Ttot."""
    B, V, t1 = c.M, _tok_V(c), c.pos + 1
    if c.op == "sample":
        pick = sample_pick(c, inp["logits"], inp["seed"])[0]
        margin = None
    else:
        pick, margin = [], []
        for b in range(B):
            v, ix = inp["ws_val"][b].tolist(), inp["ws_idx"][b].tolist()
            best = max(v)
            win = min(i for val, i in zip(v, ix) if val == best)
            others = [val for val, i in zip(v, ix) if i != win]
            pick.append(win)
            margin.append(best - max(others) if others else math.inf)  # fp32 values: the float64 difference rounds once, as the fp32 one
    nxt = torch.tensor([int(inp["prompt"][b, t1]) if t1 < c.P else pick[b] for b in range(B)], dtype=torch.int64)
    out = {"tok_cur": nxt}
    tokens = torch.full((B, c.Ttot), -7, dtype=torch.int64)
    if t1 < c.Ttot:
        tokens[:, t1] = nxt
    out["tokens_out"] = tokens
    if margin is not None:
        m = torch.full((B, c.Ttot), 123.0)
        if t1 < c.Ttot:
            m[:, t1] = torch.tensor(margin, dtype=torch.float64).float()
        out["margin_out"] = m
    if c.op != "reduce":
        out["x"] = inp["emb"].float()[nxt.clamp(0, V - 1)] + inp["postab"][t1]
        out["pos"] = torch.tensor([t1], dtype=torch.int32)
        out["ticket"] = torch.zeros(1, dtype=torch.int32)
    else:
        out["pos"] = torch.tensor([c.pos], dtype=torch.int32)  # pm_dec_argmax_reduce leaves the position to pm_dec_advance
    return out


def _tok_place(c: Case, inp: dict, P: dict, dev, poison: bool) -> dict:
    B, d, G = c.M, c.K, P["g"]
    P["prompt"] = inp["prompt"].to(dev)
    for name in ("emb", "postab"):
        P[name] = _operand(inp.get(name), dev, poison, d)
    if c.op == "sample":
        P["logits"] = Guarded((B, c.N), (_ld(c.N), 1), torch.float32, dev, table=NAN, init=inp["logits"]).view  # ldl > V in every family
    else:
        P["ws_val"], P["ws_idx"] = _operand(inp["ws_val"], dev, poison, c.N), inp["ws_idx"].to(dev)
    G["tok_cur"] = Guarded((B,), (1,), torch.int64, dev)
    G["tokens_out"] = Guarded((B, c.Ttot), (c.Ttot, 1), torch.int64, dev, init=torch.full((B, c.Ttot), -7, dtype=torch.int64))
    if c.op != "sample":
        G["margin_out"] = Guarded((B, c.Ttot), (c.Ttot, 1), torch.float32, dev, init=torch.full((B, c.Ttot), 123.0))
    if c.op != "reduce":
        G["x"] = Guarded((B, d), (d, 1), torch.float32, dev)
        G["ticket"] = Guarded((1,), (1,), torch.int32, dev, init=torch.zeros(1, dtype=torch.int32))
    G["pos"] = Guarded((1,), (1,), torch.int32, dev, init=torch.tensor([c.pos], dtype=torch.int32))
    return P


def _tok_run(L, c: Case, P: dict) -> int:
    G = P["g"]
    v = lambda n: _p(G[n].view)  # noqa: E731
    if c.op == "reduce":
        return L.pm_dec_argmax_reduce(_p(P["ws_val"]), _p(P["ws_idx"]), c.N, v("pos"), _p(P["prompt"]), c.P, v("tok_cur"), v("tokens_out"), c.Ttot,
                                      v("margin_out"), c.M, None)
    if c.op == "next":
        return L.pm_dec_next_token(_p(P["ws_val"]), _p(P["ws_idx"]), c.N, v("pos"), _p(P["prompt"]), c.P, v("tok_cur"), v("tokens_out"), c.Ttot,
                                   v("margin_out"), _p(P["emb"]), _p(P["postab"]), v("x"), c.K, NEXT_V, v("ticket"), c.M, None)
    lg = P["logits"]
    return L.pm_dec_sample_topk(_p(lg), lg.stride(0), c.N, c.topk, P["seed"], v("pos"), _p(P["prompt"]), c.P, v("tok_cur"), v("tokens_out"),
                                c.Ttot, _p(P["emb"]), _p(P["postab"]), v("x"), c.K, v("ticket"), c.M, None)


def _tok_emulate(c: Case, P: dict, mutant: str | None) -> int:
    """The tails in torch: a stable descending sort for the order, fp32 for the softmax."""
    G, B, V, t1 = P["g"], c.M, _tok_V(c), c.pos + 1
    if c.op == "sample":
        lg = P["logits"]
        srt = torch.sort(lg, dim=-1, descending=True, stable=True)
        v, ix = srt.values[:, : c.topk], srt.indices[:, : c.topk]
        cum = torch.cumsum(torch.exp(v - v[:, :1]), -1)
        u = torch.tensor([ds_uniform(P["seed"], c.pos, b)[1] for b in range(B)], dtype=torch.float32)[:, None] * cum[:, -1:]
        pick = (u < cum).float().argmax(-1)
        win = ix.gather(1, pick[:, None])[:, 0]
    else:
        wv, wi = P["ws_val"], P["ws_idx"].long()
        best = wv.max(-1, keepdim=True).values
        cand = torch.where(wv == best, wi, torch.full_like(wi, -1 if mutant == "tie_high" else 2 ** 31))
        win = cand.max(-1).values if mutant == "tie_high" else cand.min(-1).values
        rest = torch.where(wi == win[:, None], torch.full_like(wv, -math.inf), wv)
        second = rest.max(-1).values
        if mutant == "margin_top2":  # the runner-up among DIFFERENT values instead of among the other tiles
            second = torch.where(wv == best, torch.full_like(wv, -math.inf), wv).max(-1).values
        if t1 < c.Ttot:
            G["margin_out"].view[:, t1] = best[:, 0] - second
    nxt = P["prompt"][:, t1] if (t1 < c.P and mutant != "no_forcing") else win
    G["tok_cur"].view.copy_(nxt)
    if t1 < c.Ttot:
        G["tokens_out"].view[:, t1] = nxt
    if c.op != "reduce":
        row = c.pos if mutant == "tail_pos_row" else t1
        G["x"].view.copy_(P["emb"].float()[nxt.clamp(0, V - 1)] + P["postab"][row])
        G["pos"].view.fill_(t1)
    return 0


# --------------------------------------------------------------------------------------------------------------- fused self block
def _fs_build(c: Case, g) -> dict:
    B, H, d, T, inner = c.M, c.H, c.K, c.Tmax, c.N
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    kdt = torch.float32 if c.kv32 else torch.bfloat16
    inp = dict(x=rn(B, d), gamma=1.0 + 0.1 * rn(d), beta=0.1 * rn(d), w=bf16r(rn(3 * inner, d) * d ** -0.5), bias=0.1 * rn(3 * inner))
    kc0, vc0 = rn(B, H, T, 64), rn(B, H, T, 64)
    if not c.kv32:
        kc0, vc0 = bf16r(kc0), bf16r(vc0)
    if c.family == "needle":  # q = its bias exactly (zero weights); one key per (b, h) scores 30, every other ~ N(0, 1)
        inp["w"][: 2 * inner] = 0
        q = bf16r(rn(inner))
        inp["bias"][:inner] = q
        qh = q.view(H, 64)
        key = bf16r(30.0 * 8.0 * qh / qh.square().sum(-1, keepdim=True))
        if c.needle == c.pos:
            inp["bias"][inner: 2 * inner] = key.reshape(-1)  # the newest key: k = its bias, exactly (bf16 values)
        else:
            inp["bias"][inner: 2 * inner] = bf16r(rn(inner))
            kc0[:, :, c.needle] = key[None]
    inp["w"] = inp["w"].to(torch.bfloat16)
    inp["kc0"], inp["vc0"] = kc0.to(kdt), vc0.to(kdt)
    if c.n_parts > 0:
        inp["parts"] = rn(c.n_parts, B, d)
        inp["xb"] = 0.1 * rn(d) if c.xbias else None
    if c.emit:
        inp["wo"] = bf16r(rn(d, inner) * inner ** -0.5).to(torch.bfloat16)
    return inp


def _fs_row(c: Case, inp: dict) -> torch.Tensor:
    """The block's input row in fp32, in the kernel's order: parts in part order, then the bias, then the stream."""
    x = inp["x"]
    if c.n_parts <= 0:
        return x
    sp = torch.zeros_like(x)
    for p in range(c.n_parts):
        sp = sp + inp["parts"][p]
    return (sp + (inp["xb"] if inp["xb"] is not None else 0.0)) + x


def _fs_reference(c: Case, inp: dict) -> dict:
    d, w = c.K, inp["w"].double()
    xin = _fs_row(c, inp)
    xn, xh, sig = _ln64(xin.double(), inp["gamma"].double(), inp["beta"].double())
    e = d * U * xin.double().abs().mean(-1, keepdim=True)
    dxn = inp["gamma"].double().abs() / sig * (2 + xh.abs()) * e + 3 * U * xn.abs()
    b = inp["bias"].double()
    z = xn @ w.T + b
    dz = dxn @ w.abs().T + (d + 2) * U * (xn.abs() @ w.abs().T + b.abs())  # an fp32 FMA chain of d terms, the 8-lane sum, the bias
    return {"xin": xin, "z": (z, dz)}


def _fs_attention(c: Case, inp: dict, ref: dict, krow: torch.Tensor, vrow: torch.Tensor, drop_newest: bool = False):
    """(want, bound) of att (B, 64 H) over the old cache rows and the STORED newest row (B, H, 64): the kernel attends over what it stored."""
    B, H, inner, pos = c.M, c.H, c.N, c.pos
    q, dq = (t[:, :inner].reshape(B, H, 64) for t in ref["z"])
    K = torch.cat([inp["kc0"][:, :, :pos].double(), krow.double()[:, :, None]], 2)
    V = torch.cat([inp["vc0"][:, :, :pos].double(), vrow.double()[:, :, None]], 2)
    if drop_newest and pos > 0:
        K, V = K[:, :, :-1], V[:, :, :-1]
    Lk = K.shape[2]
    s = torch.einsum("bhd,bhkd->bhk", q, K) / 8
    ds = torch.einsum("bhd,bhkd->bhk", dq, K.abs()) / 8 + (64 + 2) * U * torch.einsum("bhd,bhkd->bhk", q.abs(), K.abs()) / 8
    m = s.max(-1, keepdim=True).values
    p = torch.softmax(s, -1)
    A = torch.einsum("bhk,bhkd->bhd", p, V.abs())
    want = torch.einsum("bhk,bhkd->bhd", p, V)
    E = ds.max(-1).values + U * (s - m).abs().max(-1).values + 2 * U
    bound = 2 * E[..., None] * A + (2 * Lk + 4) * U * A
    return want.reshape(B, inner), bound.reshape(B, inner)


def _fs_place(c: Case, inp: dict, P: dict, dev, poison: bool) -> dict:
    B, H, d, T, inner, G = c.M, c.H, c.K, c.Tmax, c.N, P["g"]
    kdt = torch.float32 if c.kv32 else torch.bfloat16
    for name in ("x", "w"):
        P[name] = _operand(inp[name], dev, poison, d)  # (rows d apart: the entry point has no leading dimensions)
    for name in ("gamma", "beta", "bias"):
        P[name] = _operand(inp[name], dev, poison)
    P["xb"] = _operand(inp.get("xb"), dev, poison)
    P["wo"] = _operand(inp.get("wo"), dev, poison, inner)
    if c.n_parts > 0:
        P["parts"] = Guarded(inp["parts"].shape, (B * d, d, 1), torch.float32, dev, table=NAN, init=inp["parts"]).view if poison else inp["parts"].to(dev)
    st = (H * T * 64, T * 64, 64, 1)
    for name in ("kc", "vc"):
        init = inp[name + "0"].clone()
        if poison:
            init[:, :, c.pos:] = math.nan  # rows from pos on hold no key yet: a kernel that reads one of them spreads the NaN
        G[name] = Guarded(init.shape, st, kdt, dev, init=init)
        P["init_" + name] = init
    P["posv"] = torch.tensor([c.pos], dtype=torch.int32, device=dev)
    if c.n_parts > 0:
        G["xout"] = Guarded((B, d), (d, 1), torch.float32, dev)
    if c.emit:
        G["hp"] = Guarded((B, H, d), (H * d, d, 1), torch.float32, dev)
    else:
        G["att"] = Guarded((B, inner), (inner, 1), torch.float32, dev)
    return P


def _fs_run(L, c: Case, P: dict) -> int:
    G, B, H, d, T = P["g"], c.M, c.H, c.K, c.Tmax
    kc, vc = G["kc"].view, G["vc"].view
    if c.n_parts < 0:
        fn = L.pm_dec_attention_fused_kv32 if c.kv32 else L.pm_dec_attention_fused
        return fn(_p(P["x"]), d, _p(P["gamma"]), _p(P["beta"]), EPS, _p(P["w"]), _p(P["bias"]), _p(kc), _p(vc), H * T * 64, T * 64, 64, _p(P["posv"]),
                  0, T, _p(G["att"].view), B, H, 1, None)
    np_ = c.n_parts
    return L.pm_dec_attention_chain(_p(P["x"]), d, _p(P["gamma"]), _p(P["beta"]), EPS, _p(P["w"]), _p(P["bias"]), _p(kc), _p(vc), H * T * 64, T * 64, 64,
                                    _p(P["posv"]), 0, T, B, H, 1, int(c.kv32), _p(P["parts"]) if np_ else None, np_, B * d, d,
                                    _p(P["xb"]) if np_ else None, _p(G["xout"].view) if np_ else None, _p(P["wo"]) if c.emit else None,
                                    _p(G["hp"].view) if c.emit else None, None if c.emit else _p(G["att"].view), None)


def _fs_emulate(c: Case, P: dict, mutant: str | None) -> int:
    """The block in fp32 torch: row, LayerNorm, one matmul for q / k / v, the cache append, softmax attention, the per-head products."""
    G, B, H, d, inner, pos = P["g"], c.M, c.H, c.K, c.N, c.pos
    inp = dict(x=P["x"], parts=P.get("parts"), xb=P["xb"])
    xin = _fs_row(c, inp)
    if c.n_parts > 0:
        G["xout"].view.copy_(xin)
    mu = xin.mean(-1, keepdim=True)
    xn = (xin - mu) * torch.rsqrt(((xin - mu) ** 2).mean(-1, keepdim=True) + EPS) * P["gamma"] + P["beta"]
    z = xn @ P["w"].float().T + P["bias"]
    q = z[:, :inner].reshape(B, H, 64)
    row = pos if mutant != "kv_row_off" else (pos + 1 if pos + 1 < c.Tmax else pos - 1)
    new = []
    for name, lo_ in (("kc", inner), ("vc", 2 * inner)):
        v = z[:, lo_: lo_ + inner].reshape(B, H, 64)
        st = trunc_bf16(v) if (mutant == "trunc_cache" and not c.kv32) else v.to(G[name].view.dtype)
        old = G[name].view[:, :, :pos].float()
        G[name].view[:, :, row] = st
        new.append(torch.cat([old, st.float()[:, :, None]], 2))
    K, V = new
    lost = pos if mutant == "newest_dropped" else c.needle if mutant == "needle_dropped" else -1  # a kernel that loses one key
    if lost >= 0:
        keep = torch.arange(pos + 1) != lost
        K, V = K[:, :, keep], V[:, :, keep]
    p = torch.softmax(torch.einsum("bhd,bhkd->bhk", q, K) / 8, -1)
    att = torch.einsum("bhk,bhkd->bhd", p, V)  # (no key left: zeros)
    if c.emit:
        G["hp"].view.copy_(torch.einsum("bhj,nhj->bhn", att, P["wo"].float().view(d, H, 64)))
    else:
        G["att"].view.copy_(att.reshape(B, inner))
    return 0


def _fs_check(c: Case, P: dict, ref: dict, notes: list[str]) -> float:
    G, B, H, inner, pos = P["g"], c.M, c.H, c.N, c.pos
    worst = 0.0
    if c.n_parts > 0 and not torch.equal(bits(G["xout"].view.cpu()), bits(ref["xin"])):
        notes.append("x_out: not the row x + bias + parts (in part order) bit for bit")
    z, dz = ref["z"]
    rows = torch.ones(c.Tmax, dtype=torch.bool)
    rows[pos] = False
    stored = {}
    for name, lo_ in (("kc", inner), ("vc", 2 * inner)):
        got = G[name].view.cpu()
        if not torch.equal(bits(got[:, :, rows]), bits(P["init_" + name][:, :, rows])):
            notes.append(f"{name}: a cache row other than pos = {pos} changed")
        zz, dd = z[:, lo_: lo_ + inner].reshape(B, H, 64), dz[:, lo_: lo_ + inner].reshape(B, H, 64)
        bd = dd + (U * zz.abs() if c.kv32 else store_term(zz.abs() + dd, "bf16"))
        stored[name] = got[:, :, pos].float()
        worst = max(worst, ratio(stored[name], zz, bd))
    if not (torch.isfinite(stored["kc"]).all() and torch.isfinite(stored["vc"]).all()):
        return math.inf
    want, bound = _fs_attention(c, P["inp"], ref, stored["kc"], stored["vc"])
    if c.emit:
        wo = P["inp"]["wo"].double()
        hp = G["hp"].view.cpu().double().sum(1)  # the heads in order (float64: the consumer's H additions are in the bound)
        worst = max(worst, ratio(hp.float(), want @ wo.T, bound @ wo.abs().T + (64 + H + 2) * U * (want.abs() @ wo.abs().T)))
    else:
        worst = max(worst, ratio(G["att"].view.cpu(), want, bound))
    return worst


# --------------------------------------------------------------------------------------------------------------- judging
def fixed_perm(c: Case) -> torch.Tensor:
    g = torch.Generator().manual_seed(_seed(c) ^ 0x5EED)
    p = torch.randperm(c.M, generator=g)
    return p if c.M < 2 or not torch.equal(p, torch.arange(c.M)) else p.roll(1)


def _check_outputs(c: Case, P: dict, ref: dict, exact: bool, notes: list[str], perm=None) -> float:
    """Sentinels, the integer outputs, and max |err| / bound over the float outputs of one finished launch."""
    G = P["g"]
    worst = 0.0
    for name, g in G.items():
        if not g.intact():
            notes.append(f"{name}: a byte outside the output changed")
    sel = (lambda t: t[perm]) if perm is not None else (lambda t: t)

    def cmp(name, got, want, bound):
        nonlocal worst
        want, bound = sel(want), sel(bound)
        got = got.cpu()
        if exact:
            if not torch.equal(bits(got), bits(want.to(got.dtype))):
                notes.append(f"{name}: {int((bits(got) != bits(want.to(got.dtype))).sum())} elements differ from the exact result")
            return
        r = ratio(got.float(), want, bound)
        worst = max(worst, r)

    if c.op in TOK_OPS:
        for name in G:  # every output is discrete or a bit-exact fp32 result: compared as integers
            if not torch.equal(bits(G[name].view.cpu()), bits(ref[name])):
                notes.append(f"{name}: {int((bits(G[name].view.cpu()) != bits(ref[name])).sum())} elements differ")
    if c.op == "fself":
        worst = max(worst, _fs_check(c, P, ref, notes))
    if c.op == "embed":
        cmp("x", G["x"].view, *ref["x"])
    if c.op in ("linear", "ksplit"):
        cmp("out", G["out"].view, *ref["out"])
    if c.op == "ksplit" and int(G["tickets"].view.abs().sum()) != 0:
        notes.append("a K-split ticket is not back at zero")
    if c.op == "kparts":
        got = G["parts"].view.cpu()
        want, bound = ref["parts"]
        if perm is not None:
            want, bound = want[:, perm], bound[:, perm]
        if exact:
            if not torch.equal(bits(got), bits(want.float())):
                notes.append("parts: differ from the exact result")
        else:
            worst = max(worst, ratio(got, want, bound))
    if c.op == "qkv":
        cmp("out", G["out"].view, *ref["out"])
        for name, key in (("kc", "k"), ("vc", "v")):
            got = G[name].view.cpu()
            init = sel(P["init_" + name])
            rows = torch.ones(c.Tmax, dtype=torch.bool)
            rows[c.pos] = False
            if not torch.equal(bits(got[:, :, rows]), bits(init[:, :, rows])):
                notes.append(f"{name}: a cache row other than pos = {c.pos} changed")
            cmp(name, got[:, :, c.pos], *ref[key])
    if c.op == "argmax":
        cmp("ws_val", G["ws_val"].view, *ref["ws_val"])
        wi = G["ws_idx"].view.cpu()
        want = sel(ref["int:ws_idx"])
        if not torch.equal(wi, want):
            bad = (wi != want).nonzero()[0].tolist()
            notes.append(f"ws_idx: {int((wi != want).sum())} tile winners differ, first at (row, tile) {bad}: {int(wi[bad[0], bad[1]])} for {int(want[bad[0], bad[1]])}")
        # the winner over all tiles, as pm_dec_argmax_reduce forms it: highest value, lowest index among equals
        wv = G["ws_val"].view.cpu()
        best = wv.max(-1, keepdim=True).values
        tok = torch.where(wv == best, wi, torch.full_like(wi, 2 ** 31 - 1)).min(-1).values
        zt = sel(ref["tiles"][0])
        want_tok = zt.reshape(c.M, -1).max(-1).indices.int()
        if not torch.equal(tok, want_tok):
            notes.append(f"the winner over all tiles differs in {int((tok != want_tok).sum())} rows")
    return worst


def judge(c: Case, inp: dict, ref: dict, runner, dev="cpu", margin: float = MARGIN) -> dict:
    """Everything the suite asserts about one case; runner(case, P) launches on the placement P and returns the status."""
    notes: list[str] = []
    exact = c.family == "exact"
    rec = dict(id=c.id, op=c.op, family=c.family, env=c.env, ratio=0.0)

    def launch(**kw):
        P = place(c, inp, dev, poison=c.family == "poison", **kw)
        if c.op == "qkv":
            P["init_kc"], P["init_vc"] = inp["kc0"], inp["vc0"]
        if c.op == "sample":
            P["seed"] = inp["seed"]
        P["inp"] = inp
        rc = runner(c, P)
        if rc != 0:
            notes.append(f"the entry point returned {rc}")
        return P

    if c.refused:
        P = place(c, inp, dev)
        rc = runner(c, P)
        ok = rc == c.refused and all(bool((g.raw == g.fill).all()) for g in P["g"].values())  # refused before anything is written
        return dict(rec, ok=ok, notes=[] if ok else [f"expected refusal {c.refused}, got {rc}"], ratio=0.0)
    if c.op == "sample":
        rec["seed"] = inp["seed"]
    P = launch()
    worst = _check_outputs(c, P, ref, exact, notes)
    first = {n: bits(g.view.cpu()).clone() for n, g in P["g"].items()}
    exact = exact or c.op in TOK_OPS
    rec["digest"] = digest(*(g.view for _, g in sorted(P["g"].items())))
    if c.op == "ksplit" and not notes:  # a second launch on the same workspace and tickets: the same bits
        G = P["g"]
        G["out"].reset()
        rc = runner(c, P)
        if rc != 0 or not torch.equal(bits(G["out"].view.cpu()), first["out"]) or int(G["tickets"].view.abs().sum()) != 0:
            notes.append("a second launch differs or leaves a ticket")
    if c.family == "perm" and not notes:
        p = fixed_perm(c)
        Q = launch(perm=p)
        worst = max(worst, _check_outputs(c, Q, ref, exact, notes, perm=p))
        for n, g in Q["g"].items():
            if n == "tickets":
                continue
            want_bits = first[n][:, p] if n == "parts" else first[n][p]  # (parts: the rows are the second dimension)
            if not torch.equal(bits(g.view.cpu()), want_bits):
                notes.append(f"{n}: permuted rows give other bits")
    if c.family == "scale" and not notes:
        base = P["g"]["out"].view.cpu()
        for k in (40, -40):
            Q = launch(scale=2.0 ** k)
            if not Q["g"]["out"].intact():
                notes.append("scale: a byte outside the output changed")
            if not torch.equal(bits(Q["g"]["out"].view.cpu()), bits(base * 2.0 ** k)):
                notes.append(f"scale: out(2^{k} x) != 2^{k} out(x)")
    rec.update(ratio=worst, ok=not notes and worst <= margin, notes=notes)
    return rec


def figure(rec: dict) -> str:
    return f"RATIO {rec['op']} {rec['family']} {rec['id']} {rec['ratio']:.3f}"


def explain(rec: dict) -> str:
    return f"{rec['id']}: ratio {rec['ratio']:.3f}; " + "; ".join(rec.get("notes", []))
