"""Cases and float64 references shared by the kernel-level tests of csrc/decode_t5.hip (tests/test_t5_decode_cases_cpu.py without a
GPU, tests/test_hip_t5_decode.py on one).  A plain helper module.

Contract:
  * references are plain torch, written from the definition of each stage (oracle/ref_t5.py semantics), and dtype-generic: the GPU
    file evaluates them in float64, the CPU file also in float32 to prove that the tolerance is satisfiable;
  * storage points: weights, caches and the packed cross K/V hold bf16 VALUES before either path sees them; the key / value pair a
    step appends is rounded once, by the kernel, so the attention reference takes row t from the kernel's own cache and that row
    is checked on its own against the unrounded projection (`row_ok`: one bf16 rounding, 2^-8 |want| + 1e-6);
  * tolerance: rtol = atol = TOL = 1e-5, the project's rule for kernels whose sums are fp32, at outputs of rms ~ 1 (values are
    scaled by a power of two so that they are);
  * the position-bias table is NOT the model's (which is constant from distance 127 on): every (head, distance) holds its own
    random value of deviation 2, so an index error at any distance moves the output by O(0.1);
  * random keys hide a lost key (2048 keys share the mass), so every attention geometry also has NEEDLE rows: one key j* is made
    c q / |q| with c chosen so that it takes 0.9 of the softmax mass, its value row is made distinct.  The own key (j* = t) of the
    self-attention kernels comes out of the projection and cannot be planted: there the table entry of distance 0 is raised instead.

The reference functions take keyword MUTATIONS (an index shift, a dropped key, dropped columns, ...): MUTANTS names each with the
case built to expose it, and the CPU file requires that it misses the tolerance by 10 x there.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from synthweights import synth_input, synth_tokens

TOL = 1e-5
EPS = 1e-6  # with the tiny-row cases (a row of x scaled by 1e-3: mean(x^2) ~ 1e-6) the eps term decides tens of percent
U_BF16 = 2.0 ** -8
NEEDLE_MASS = 0.9
NEG_INF = float("-inf")


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """Nearest bf16 value in fp32 storage: both paths see exactly these numbers."""
    return x.to(torch.bfloat16).float()


def used(got: torch.Tensor, want: torch.Tensor, tol: float = TOL) -> float:
    """Largest |got - want| / (tol + tol |want|): the used fraction of the allowance (nan if anything is not finite)."""
    got, want = got.double(), want.double()
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("nan")
    return float(((got - want).abs() / (tol + tol * want.abs())).max())


def row_ok(got: torch.Tensor, want: torch.Tensor) -> float:
    """Used fraction of one bf16 rounding of the (unrounded) projection: |got - want| <= 2^-8 |want| + 1e-6."""
    got, want = got.double(), want.double()
    if not torch.isfinite(got).all():
        return float("nan")
    return float(((got - want).abs() / (U_BF16 * want.abs() + 1e-6)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the operations, from their definitions


def rms_norm(x, gamma, eps, count=None):
    """x * rsqrt(mean(x^2) + eps) * gamma; ``count`` (mutation): the mean taken over another number of columns"""
    n = x.shape[-1] if count is None else count
    return x * torch.rsqrt((x * x).sum(-1, keepdim=True) / n + eps) * gamma


def gelu_tanh(a):
    return 0.5 * a * (1 + torch.tanh(math.sqrt(2 / math.pi) * (a + 0.044715 * a * a * a)))


def gelu_erf(a):
    return 0.5 * a * (1 + torch.erf(a / math.sqrt(2)))


def _normed(x, g, dtype, no_eps, count, drop_cols):
    xn = rms_norm(x.to(dtype), g.to(dtype), 0.0 if no_eps else EPS, count)
    if drop_cols is not None:  # mutation: the projections never see columns >= drop_cols
        xn = xn.clone()
        xn[:, drop_cols:] = 0
    return xn


def argmax_lowest(vals: torch.Tensor, idx: torch.Tensor) -> int:
    """the index paired with the largest value, the lowest such index on ties (also when every value is -inf)"""
    return int(idx[vals == vals.max()].min())


# ---------------------------------------------------------------------------------------------------------------------------------
# self-attention step: RMS norm -> [q|k|v] -> append at t -> one query over t + 1 keys with score / 8 + lut[h, t - j]


@dataclass(frozen=True)
class SelfCase:
    id: str
    B: int
    d: int
    H: int
    Tmax: int
    t: int
    needles: tuple = ()   # per row: the planted key (B == len(needles))
    own: bool = False     # the own key t carries the mass (lut[h, 0] raised); B == 1
    tiny_row: int | None = None

    @property
    def inner(self):
        return self.H * 64

    @property
    def n(self):
        return self.t + 1


SELF_CASES = [
    # d: 40 / 384 = ragged first column group, 512 = one full group, 520 = one chunk in the second group, 1024 = both full.
    # H with d = 512: inner = 384 < d and 768 > d.  B = 9: a second row group of one row in t5_rms_proj_kernel; 64: the ABI's limit.
    SelfCase("d40_h1_b1_t0", 1, 40, 1, 64, 0),
    SelfCase("d384_h6_t1", 2, 384, 6, 64, 1),
    SelfCase("d512_h12_b9_t31", 9, 512, 12, 64, 31),
    SelfCase("d520_h6_b9_t32", 9, 520, 6, 64, 32),
    SelfCase("d512_h6_b8_t63_last", 8, 512, 6, 64, 63),
    SelfCase("d512_h6_t255", 2, 512, 6, 300, 255),
    SelfCase("d1024_h1_t256", 2, 1024, 1, 300, 256),
    SelfCase("d512_h12_t257", 2, 512, 12, 300, 257),
    SelfCase("d520_h2_t299_last", 2, 520, 2, 300, 299),
    SelfCase("d1024_h2_t2047_last", 2, 1024, 2, 2048, 2047),
    SelfCase("d520_h2_b64_t40", 64, 520, 2, 64, 40),
    SelfCase("tiny_row", 2, 512, 1, 64, 5, tiny_row=1),
    # needles: 0 / 31 / 32 = the 32-key value groups, 255 / 256 / 257 = the 256-thread stride, n - 2, and (own) n - 1 = t, 2047
    SelfCase("needle_n33", 3, 512, 2, 64, 32, needles=(0, 30, 31)),
    SelfCase("needle_n258", 5, 512, 2, 300, 257, needles=(0, 31, 32, 255, 256)),
    SelfCase("needle_n2048", 7, 512, 2, 2048, 2047, needles=(0, 31, 32, 255, 256, 257, 2046)),
    SelfCase("own_n33", 1, 512, 2, 64, 32, own=True),
    SelfCase("own_n258", 1, 512, 2, 300, 257, own=True),
    SelfCase("own_n2048", 1, 520, 2, 2048, 2047, own=True),
]


def ref_self(c: SelfCase, inp: dict, dtype=torch.float64, own=None, *, lut_shift=0, drop_key=None, drop_cols=None, no_eps=False,
             count=None, scale=0.125) -> dict:
    """q (B, inner), the unrounded k / v of this step (B, H, 64), att (B, inner) and the softmax p (B, H, n).  ``own`` = the
    (k, v) rows at t as cached (B, H, 64); None: this evaluation's own projection rounded to bf16."""
    B, H, t, n, inner = c.B, c.H, c.t, c.n, c.inner
    xn = _normed(inp["x"], inp["g"], dtype, no_eps, count, drop_cols)
    qkv = xn @ inp["w"].to(dtype).T
    q, kn, vn = (qkv[:, i * inner:(i + 1) * inner].reshape(B, H, 64) for i in range(3))
    k, v = inp["kc"][:, :, :n].to(dtype).clone(), inp["vc"][:, :, :n].to(dtype).clone()
    kt, vt = (bf16r(kn), bf16r(vn)) if own is None else own
    k[:, :, t], v[:, :, t] = kt.to(dtype), vt.to(dtype)
    dist = (t - torch.arange(n) + lut_shift).clamp(0, c.Tmax - 1)  # lut_shift (mutation): lut[h, t - j +- 1]
    s = torch.einsum("bhe,bhne->bhn", q, k) * scale + inp["lut"].to(dtype)[:, dist]
    if drop_key is not None:  # mutation: row b never sees key drop_key[b]
        for b, j in enumerate(drop_key):
            s[b, :, j] = NEG_INF
    p = torch.softmax(s, -1)
    att = torch.einsum("bhn,bhne->bhe", p, v).reshape(B, inner)
    return dict(q=q.reshape(B, inner), k_new=kn, v_new=vn, att=att, p=p)


def _pow2_to_unit(rms: float) -> float:
    return 2.0 ** round(-math.log2(max(rms, 1e-30)))


@functools.lru_cache(maxsize=None)
def build_self(c: SelfCase) -> dict:
    """x (B, d) f32; g (d,) f32; w (3 inner, d) bf16 values; kc / vc (B, H, Tmax, 64) bf16 values (rows >= t are never to be read:
    the GPU file overwrites them with NaN); lut (H, Tmax) f32.  Treat as read-only."""
    assert not c.needles or len(c.needles) == c.B
    assert not c.own or c.B == 1
    B, H, inner, t = c.B, c.H, c.inner, c.t
    x = synth_input(f"t5d_x_{c.id}", (B, c.d), 1)
    if c.tiny_row is not None:
        x[c.tiny_row] *= 1e-3
    inp = dict(
        x=x,
        g=1 + 0.1 * synth_input("t5d_g", (c.d,), 2),
        w=bf16r(synth_input(f"t5d_w_{c.id}", (3 * inner, c.d), 3, scale=c.d ** -0.5)),
        kc=bf16r(synth_input(f"t5d_k_{c.id}", (B, H, c.Tmax, 64), 4)),
        vc=bf16r(synth_input(f"t5d_v_{c.id}", (B, H, c.Tmax, 64), 5)),
        lut=2 * synth_input(f"t5d_lut_{c.id}", (H, c.Tmax), 6),
    )
    r = ref_self(c, inp)
    q = r["q"].view(B, H, 64)
    dist = t - torch.arange(c.n)
    if c.needles:
        for b, js in enumerate(c.needles):
            assert 0 <= js < t
            for h in range(H):
                s = (inp["kc"][b, h, :c.n].double() @ q[b, h]) * 0.125 + inp["lut"][h, dist].double()
                s[t] = (bf16r(r["k_new"][b, h]).double() @ q[b, h]) * 0.125 + inp["lut"][h, 0].double()
                s[js] = NEG_INF
                target = torch.logsumexp(s, 0) + math.log(NEEDLE_MASS / (1 - NEEDLE_MASS))
                qn = q[b, h].norm()
                inp["kc"][b, h, js] = bf16r(((target - inp["lut"][h, t - js].double()) * 8 / qn * q[b, h] / qn).float())
            inp["vc"][b, :, js] = bf16r(1.5 * synth_input(f"t5d_needle_v_{c.id}", (H, 64), 7 + b))
    elif c.own:
        for h in range(H):
            s = (r["p"][0, h].log())  # scores up to a constant
            rest = torch.logsumexp(s[:t], 0)
            inp["lut"][h, 0] += float(rest + math.log(NEEDLE_MASS / (1 - NEEDLE_MASS)) - s[t])
        vs = _pow2_to_unit(float(r["v_new"].square().mean().sqrt()))
        inp["w"][2 * inner:] *= vs
    else:  # many keys share the mass and the output shrinks: values (cache and weight rows) scaled back by a power of two
        vs = _pow2_to_unit(float(r["att"].square().mean().sqrt()))
        inp["vc"] *= vs
        inp["w"][2 * inner:] *= vs
    return inp


# ---------------------------------------------------------------------------------------------------------------------------------
# cross-attention step: RMS norm -> q -> one query over the first src_len[b] keys of the packed (B, S, [k | v]) projection


@dataclass(frozen=True)
class CrossCase:
    id: str
    B: int
    d: int
    H: int
    S: int
    src_len: tuple        # per row, as given to the kernel: <= 0 -> zeros, > S -> S
    needles: tuple = ()   # per row: the planted key or None
    tiny_row: int | None = None

    @property
    def inner(self):
        return self.H * 64

    def keys(self, b: int) -> int:
        return max(0, min(self.src_len[b], self.S))


CROSS_CASES = [
    CrossCase("s16_d40_h1", 4, 40, 1, 16, (-3, 1, 16, 21)),
    CrossCase("s16_d512_h1_b1", 1, 512, 1, 16, (16,)),
    CrossCase("s300_d512_h6", 8, 512, 6, 300, (0, 1, 255, 256, 257, 300, 305, -3)),
    CrossCase("s2048_d1024_h2", 6, 1024, 2, 2048, (2048, 2053, 257, 256, 0, 2047)),
    CrossCase("s300_d520_h12_b9", 9, 520, 12, 300, (300, 299, 33, 32, 31, 2, 305, 0, 64)),
    CrossCase("s16_d384_h1_b64", 64, 384, 1, 16, tuple((0, 1, 15, 16, 21, -3, 7, 9)[b % 8] for b in range(64))),
    CrossCase("tiny_row", 2, 512, 1, 16, (16, 16), tiny_row=1),
    CrossCase("needle_s2048", 10, 512, 2, 2048, (2048,) * 8 + (258, 258), needles=(0, 31, 32, 255, 256, 257, 2046, 2047, 256, 257)),
    CrossCase("needle_s300", 4, 520, 2, 300, (33, 33, 305, 300), needles=(31, 32, 298, 299)),
]


def ref_cross(c: CrossCase, inp: dict, dtype=torch.float64, *, drop_key=None, drop_cols=None, no_eps=False, count=None,
              scale=0.125) -> dict:
    B, H, inner = c.B, c.H, c.inner
    xn = _normed(inp["x"], inp["g"], dtype, no_eps, count, drop_cols)
    q = (xn @ inp["w"].to(dtype).T).view(B, H, 64)
    att = torch.zeros(B, inner, dtype=dtype)
    ps = []
    for b in range(B):
        n = c.keys(b)
        if n == 0:  # nothing to attend to: zeros
            ps.append(None)
            continue
        kv = inp["kv"][b, :n].to(dtype)
        k, v = kv[:, :inner].reshape(n, H, 64), kv[:, inner:].reshape(n, H, 64)
        s = torch.einsum("he,nhe->hn", q[b], k) * scale
        if drop_key is not None and drop_key[b] is not None:
            s[:, drop_key[b]] = NEG_INF
        p = torch.softmax(s, -1)
        ps.append(p)
        att[b] = torch.einsum("hn,nhe->he", p, v).reshape(inner)
    return dict(q=q.reshape(B, inner), att=att, p=ps)


@functools.lru_cache(maxsize=None)
def build_cross(c: CrossCase) -> dict:
    """x, g as build_self; w (inner, d) bf16 values; kv (B, S, 2 inner) bf16 values (rows >= src_len[b] are never to be read)."""
    assert len(c.src_len) == c.B and (not c.needles or len(c.needles) == c.B)
    B, H, inner = c.B, c.H, c.inner
    x = synth_input(f"t5c_x_{c.id}", (B, c.d), 11)
    if c.tiny_row is not None:
        x[c.tiny_row] *= 1e-3
    inp = dict(
        x=x,
        g=1 + 0.1 * synth_input("t5c_g", (c.d,), 12),
        w=bf16r(synth_input(f"t5c_w_{c.id}", (inner, c.d), 13, scale=c.d ** -0.5)),
        kv=bf16r(synth_input(f"t5c_kv_{c.id}", (B, c.S, 2 * inner), 14)),
    )
    r = ref_cross(c, inp)
    q = r["q"].view(B, H, 64)
    for b in range(B):
        n = c.keys(b)
        if n == 0:
            continue
        js = c.needles[b] if c.needles else None
        if js is None:
            inp["kv"][b, :, inner:] *= _pow2_to_unit(float(r["att"][b].square().mean().sqrt()))
            continue
        assert 0 <= js < n
        for h in range(H):
            s = (inp["kv"][b, :n, h * 64:(h + 1) * 64].double() @ q[b, h]) * 0.125
            s[js] = NEG_INF
            target = (torch.logsumexp(s, 0) if n > 1 else torch.tensor(0.0)) + math.log(NEEDLE_MASS / (1 - NEEDLE_MASS))
            qn = q[b, h].norm()
            inp["kv"][b, js, h * 64:(h + 1) * 64] = bf16r((target * 8 / qn * q[b, h] / qn).float())
        inp["kv"][b, js, inner:] = bf16r(1.5 * synth_input(f"t5c_needle_v_{c.id}", (inner,), 17 + b))
    return inp


# ---------------------------------------------------------------------------------------------------------------------------------
# GEGLU step: RMS norm -> gelu_tanh(w_f xn) * (v_f xn)


@dataclass(frozen=True)
class GegluCase:
    id: str
    B: int
    d: int
    F: int
    ldh: int
    tiny_row: int | None = None


GEGLU_CASES = [
    GegluCase("f8_d40_b1", 1, 40, 8, 8),
    GegluCase("f24_d520_b9_pad", 9, 520, 24, 28),
    GegluCase("f1024_d512_b8", 8, 512, 1024, 1024),
    GegluCase("f1032_d1024_b64_pad", 64, 1024, 1032, 1036),
    GegluCase("f24_d384_pad", 2, 384, 24, 28),
    GegluCase("tiny_row", 2, 512, 24, 24, tiny_row=1),
]


def ref_geglu(c: GegluCase, inp: dict, dtype=torch.float64, *, swap=False, erf=False, drop_cols=None, no_eps=False, count=None):
    xn = _normed(inp["x"], inp["g"], dtype, no_eps, count, drop_cols)
    a, b = xn @ inp["w"].to(dtype).T, xn @ inp["v"].to(dtype).T
    if swap:  # mutation: the gate and the value rows exchanged
        a, b = b, a
    return (gelu_erf if erf else gelu_tanh)(a) * b


@functools.lru_cache(maxsize=None)
def build_geglu(c: GegluCase) -> dict:
    """w (gate) and v (value) (F, d) bf16 values; the value rows at 1.5 d^-1/2 so that the output's rms is ~ 1"""
    x = synth_input(f"t5g_x_{c.id}", (c.B, c.d), 21)
    if c.tiny_row is not None:
        x[c.tiny_row] *= 1e-3
    return dict(
        x=x,
        g=1 + 0.1 * synth_input("t5g_g", (c.d,), 22),
        w=bf16r(synth_input(f"t5g_w_{c.id}", (c.F, c.d), 23, scale=c.d ** -0.5)),
        v=bf16r(synth_input(f"t5g_v_{c.id}", (c.F, c.d), 24, scale=1.5 * c.d ** -0.5)),
    )


def interleave(w: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """rows [w_0; v_0; w_1; v_1; ...], written out row by row (the layout pm_t5_dec_geglu reads)"""
    out = torch.empty(2 * w.shape[0], w.shape[1], dtype=w.dtype)
    for f in range(w.shape[0]):
        out[2 * f], out[2 * f + 1] = w[f], v[f]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# next token: the winner over the classifier's tile winners, prompt forcing, eos / pad bookkeeping


@dataclass(frozen=True)
class NextCase:
    id: str
    B: int
    nt: int      # tile winners per row (the vocabulary is 64 nt)
    d: int
    eos: bool

    @property
    def V(self):
        return 64 * self.nt


NEXT_P, NEXT_TTOT = 2, 4  # position 1 is forced, 2 and 3 are generated, the step at t = 3 has no token left to write
NEXT_CASES = [
    NextCase("nt1_b1", 1, 1, 8, True),
    NextCase("nt4_b64", 64, 4, 40, True),
    NextCase("nt125_b9", 9, 125, 520, True),
    NextCase("nt300_b64", 64, 300, 1024, True),   # more than 256 tiles: the strided second trip
    NextCase("nt300_b64_no_eos", 64, 300, 512, False),
    NextCase("nt300_b1", 1, 300, 512, True),
]
PAD_ID = 3


@functools.lru_cache(maxsize=None)
def build_next(c: NextCase) -> dict:
    """Per step t (0 .. Ttot - 1) the tile winners ws_val (B, nt) f32 and ws_idx (B, nt) i32 (an arbitrary index of the tile's 64,
    as the classifier reports), prompt (B, P), E (V, d) bf16 values, eos_id.  Planted in EVERY step where the row exists: row 0 an
    exact tie in two lanes of one wave, row 1 in two waves, row 2 between the first and the second stride (nt > 256), row 3 all
    -inf; in each tie the LATER tile carries the LOWER index, so a winner chosen by tile position is wrong."""
    B, nt, V = c.B, c.nt, c.V
    steps = []
    for t in range(NEXT_TTOT):
        val = synth_input(f"t5n_val_{c.id}", (B, nt), 31 + t)
        idx = (torch.arange(nt) * 64)[None] + synth_tokens(f"t5n_idx_{c.id}", (B, nt), 64, 41 + t)
        for row, (a, b) in enumerate(((3, 5), (10, 70), (34, 290))):
            if row < B and b < nt:
                val[row, a] = val[row, b] = 9.0
                idx[row, a], idx[row, b] = idx[row, b].clone(), idx[row, a].clone()  # the later tile has the lower index
        if B > 3:
            val[3] = NEG_INF
        steps.append((val, idx.to(torch.int32)))
    # the eos id: what the last row generates at its first free position, so that at least that row finishes there
    v1, i1 = steps[NEXT_P - 1]
    eos = argmax_lowest(v1[B - 1], i1[B - 1]) if c.eos else -1
    return dict(steps=steps, prompt=synth_tokens(f"t5n_prompt_{c.id}", (B, NEXT_P), V, 51), eos_id=eos,
                E=bf16r(synth_input(f"t5n_E_{c.id}", (V, c.d), 52)))


def ref_next(c: NextCase, inp: dict) -> dict:
    """The bookkeeping, step by step, in plain Python: tokens (B, Ttot), finished (B,), out_len (B,), and per step the ids whose
    embedding rows the next step reads."""
    B = c.B
    tokens = torch.full((B, NEXT_TTOT), PAD_ID, dtype=torch.int64)
    tokens[:, :NEXT_P] = inp["prompt"]
    finished = torch.zeros(B, dtype=torch.int32)
    out_len = torch.full((B,), NEXT_TTOT, dtype=torch.int64)
    nexts = []
    for t in range(NEXT_TTOT):
        val, idx = inp["steps"][t]
        nxt = torch.empty(B, dtype=torch.int64)
        for b in range(B):
            if t + 1 < NEXT_P:
                nxt[b] = inp["prompt"][b, t + 1]
            elif finished[b]:
                nxt[b] = PAD_ID
            else:
                nxt[b] = argmax_lowest(val[b], idx[b])
                if inp["eos_id"] >= 0 and nxt[b] == inp["eos_id"]:
                    finished[b] = 1
                    out_len[b] = t + 2
            if t + 1 < NEXT_TTOT:
                tokens[b, t + 1] = nxt[b]
        nexts.append(nxt)
    return dict(tokens=tokens, finished=finished, out_len=out_len, nexts=nexts)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: (name, family, case id, reference keywords).  Each must miss TOL by 10 x on its case (tests/test_t5_decode_cases_cpu.py).

SELF = {c.id: c for c in SELF_CASES}
CROSS = {c.id: c for c in CROSS_CASES}
GEGLU = {c.id: c for c in GEGLU_CASES}

MUTANTS = [
    ("lut_index_plus_1", "self", "d520_h6_b9_t32", dict(lut_shift=1)),
    ("lut_index_minus_1", "self", "d520_h6_b9_t32", dict(lut_shift=-1)),
    ("lut_index_plus_1", "self", "d512_h12_t257", dict(lut_shift=1)),
    ("lut_index_minus_1", "self", "d512_h12_t257", dict(lut_shift=-1)),
    ("lut_index_plus_1", "self", "d1024_h2_t2047_last", dict(lut_shift=1)),
    ("lut_index_minus_1", "self", "d1024_h2_t2047_last", dict(lut_shift=-1)),
    ("lut_index_minus_1", "self", "own_n2048", dict(lut_shift=-1)),
    ("columns_ge_512_dropped", "self", "d520_h6_b9_t32", dict(drop_cols=512)),
    ("columns_ge_512_dropped", "self", "d1024_h1_t256", dict(drop_cols=512)),
    ("columns_ge_512_dropped", "cross", "s2048_d1024_h2", dict(drop_cols=512)),
    ("columns_ge_512_dropped", "cross", "s300_d520_h12_b9", dict(drop_cols=512)),
    ("columns_ge_512_dropped", "geglu", "f24_d520_b9_pad", dict(drop_cols=512)),
    ("columns_ge_512_dropped", "geglu", "f1032_d1024_b64_pad", dict(drop_cols=512)),
    ("gate_and_value_swapped", "geglu", "f24_d520_b9_pad", dict(swap=True)),
    ("gate_and_value_swapped", "geglu", "f8_d40_b1", dict(swap=True)),
    ("erf_gelu", "geglu", "f1024_d512_b8", dict(erf=True)),
    ("eps_omitted", "self", "tiny_row", dict(no_eps=True)),
    ("eps_omitted", "cross", "tiny_row", dict(no_eps=True)),
    ("eps_omitted", "geglu", "tiny_row", dict(no_eps=True)),
    ("mean_over_512", "self", "d520_h6_b9_t32", dict(count=512)),
    ("mean_over_512", "self", "d40_h1_b1_t0", dict(count=512)),
    ("mean_over_512", "cross", "s16_d40_h1", dict(count=512)),
    ("mean_over_512", "geglu", "f24_d384_pad", dict(count=512)),
    ("mean_over_1024", "geglu", "f24_d520_b9_pad", dict(count=1024)),
    ("scale_rsqrt_inner", "self", "d512_h12_t257", dict(scale=768 ** -0.5)),
    ("scale_rsqrt_d", "self", "d1024_h2_t2047_last", dict(scale=1024 ** -0.5)),
    ("scale_rsqrt_d", "cross", "s300_d512_h6", dict(scale=512 ** -0.5)),
    ("scale_one", "cross", "s2048_d1024_h2", dict(scale=1.0)),
]
