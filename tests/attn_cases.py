"""Reference, error bound and adversarial input families shared by the attention parity tests
(tests/test_attn_cases_cpu.py without a GPU, tests/test_hip_attention_adversarial.py on one).  A plain helper module.

Contract ("attention numerics contract"):
  * reference = float64 masked_fill + softmax + matmul, top-left causal;
  * a query row with no visible key (a DEAD row) returns zeros - what F.scaled_dot_product_attention returns on the CPU and
    pytorch_models/_cpu.py with it (pinned by test_attn_cases_cpu.py, not assumed);
  * kernels that feed a bf16 P to the matrix pipe and store bf16: |got - want| <= u (A + |want|), u = 2^-8, A = softmax @ |v|.
    Rounding each p_j to bf16 (relative error <= u) moves the numerator by at most u sum_j p_j |v_j| = u A l, the row sum l is
    taken over the unrounded fp32 p, the bf16 store rounds once more (<= u |want|, 2^-9 when to nearest).  The GPU suite
    asserts 1.5 x that: the margin covers the fp32 score / exp2 error (<= |s| 2^-22 relative on p, below 0.02 u for the
    |s| <= 200 used here) and the online rescale.  No measured number enters the assertion.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from synthweights import synth_input

U_BF16 = 2.0 ** -8
F32_TOL = 2e-5  # rtol = atol of the f32 kernels (tests/test_hip_fp32_models.py, test_hip_exact.py)
DEC_TOL = 1e-5  # rtol = atol of pm_dec_attention (tests/test_hip_decode.py)
NEG_INF = float("-inf")


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """Nearest bf16 value, kept in fp32 storage: both paths see exactly these numbers."""
    return x.to(torch.bfloat16).float()


def split_heads(x: torch.Tensor, H: int) -> torch.Tensor:
    """(B, L, H*hd) -> (B, H, L, hd)"""
    B, L, D = x.shape
    return x.view(B, L, H, D // H).transpose(1, 2)


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """(B, H, L, hd) -> (B, L, H*hd)"""
    B, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(B, L, H * hd)


def ref_probs(q, k, bias=None, causal=False, scale=None):
    """float64 softmax(q k^T scale + bias [causal]) on (B, H, L, hd) operands, zero on dead rows, and the dead-row mask."""
    q, k = q.double(), k.double()
    Lq, Lk = q.shape[-2], k.shape[-2]
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.double()
    if causal:
        s = s.masked_fill(~torch.ones(Lq, Lk, dtype=torch.bool).tril(), NEG_INF)
    dead = (s == NEG_INF).all(-1)
    return torch.softmax(s.masked_fill(dead[..., None], 0.0), -1).masked_fill(dead[..., None], 0.0), dead


def ref_attention(q, k, v, bias=None, causal=False, scale=None):
    """float64 attention on (B, H, L, hd) operands.  Returns (want, A, dead): want = softmax(q k^T scale + bias) v with zeros on
    dead rows, A = softmax(...) |v| (zeros on dead rows), dead = (B, H, Lq) bool."""
    p, dead = ref_probs(q, k, bias, causal, scale)
    v = v.double()
    return p @ v, p @ v.abs(), dead


def bf16_bound(want: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    return U_BF16 * (A.double() + want.double().abs())


def bound_ratio(got: torch.Tensor, want: torch.Tensor, A: torch.Tensor) -> float:
    """max |got - want| / bf16_bound; an element whose bound is 0 (dead rows, v == 0 under every live key) must be exact, and a
    non-finite output is an infinite ratio."""
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - want.double()).abs()
    bnd = bf16_bound(want, A)
    if (err[bnd == 0] != 0).any():
        return float("inf")
    live = bnd > 0
    return float((err[live] / bnd[live]).max()) if live.any() else 0.0


# Unbiased row sums.  With v == 1 a bf16-P kernel returns bf16(sum_j bf16(p_j) / sum_j p_j).  Round-to-nearest errors are
# zero-mean, at most u p_j each and (at worst) uniform: standard deviation u / sqrt(3) p_j.  Over a row whose effective key count
# n_eff = (sum p)^2 / sum p^2 is at least NEFF_EXACT = 64 the quotient's deviation from 1 has sigma <= u / sqrt(3) / 8 = 2.8e-4, so
# six sigma (1.7e-3) stay below 2^-9, the distance at which bf16 stops rounding to 1.0: such rows are EXACTLY 1.  A P conversion
# by truncation has mean relative error ~ 0.7 u: the quotient sits near 1 - 2.8e-3 and stores as 1 - 2^-8.  Both the per-element
# bound (1.5 u (A + |want|) >= 3 u A for same-sign v) and the 2^-7 row-sum property accept that; this one does not.
NEFF_EXACT = 64.0


def row_neff(case, inp) -> torch.Tensor:
    """(B, H, Lq) effective number of keys of each softmax row (0 on dead rows)."""
    qh, kh = split_heads(inp["q"], case.H), split_heads(inp["k"], case.H)
    p, _ = ref_probs(qh, kh, inp["bias"], case.causal)
    return p.sum(-1).square() / p.square().sum(-1).clamp_min(1e-300)


def emulate_bf16_kernel(q, k, v, bias=None, causal=False, scale=None, truncate=False) -> torch.Tensor:
    """The arithmetic of the bf16 MFMA kernels on the CPU: fp32 scores, exact row max, fp32 p, fp32 row sum over the unrounded p,
    P rounded to bf16 for P.V (fp32 accumulation), one bf16 store; dead rows zero.  (B, H, L, hd) fp32 in, fp32 (bf16 values) out."""
    q, k, v = q.float(), k.float(), v.float()
    Lq, Lk = q.shape[-2], k.shape[-2]
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.float()
    if causal:
        s = s.masked_fill(~torch.ones(Lq, Lk, dtype=torch.bool).tril(), NEG_INF)
    dead = (s == NEG_INF).all(-1, keepdim=True)
    m = s.max(-1, keepdim=True).values.masked_fill(dead, 0.0)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pb = (p.view(torch.int32) & -65536).view(torch.float32) if truncate else bf16r(p)  # truncate: a deliberately wrong conversion
    o = (pb @ v) / l.masked_fill(dead, 1.0)
    return bf16r(o.masked_fill(dead, 0.0))


# --------------------------------------------------------------------------------------------------------------- the cases
LEADS = (1, 63, 64, 65, 130)
MASKS = ("trail",) + tuple(f"lead{p}" for p in LEADS) + ("holes", "checker")
BIAS_FORMS = ("BH", "1H", "B1", "11", "expand", "off4", "padrow")
# The f32 kernels keep the project's 2e-5: fp32 torch SDPA itself stays within it of fp64 at score deviations 1 and 8 and on the
# planted family (scores up to ~60), NOT at 30 (|s| up to ~150: the rounding of the fp32 score alone, |s| 2^-24 per term, is
# already 1e-5 on p).  So the f32 kernels get {1, 8}; test_attn_cases_cpu.py asserts that the reference alone passes on them.
F32_SCALES = (1.0, 8.0)


@dataclass(frozen=True)
class Case:
    """One attention problem.  kernel: head | tiled | tiled_bias | generic_bf16 | generic_f32 | mfma_f32 (which kernel the
    dispatcher picks for it: expected_kernel(), asserted by the CPU test).  family: scale | planted | bias | mask."""
    kernel: str
    B: int
    H: int
    Lq: int
    Lk: int
    hd: int = 64
    family: str = "scale"
    scale: float = 1.0        # standard deviation of the scaled scores q.k / sqrt(hd)
    causal: bool = False
    form: str | None = None   # bias layout (BIAS_FORMS); None = no bias
    mask: str | None = None   # MASKS, or "deadbatch" (last batch element: every key masked)
    noisy: bool = False       # mask families: the -inf entries ride on an N(0, 3^2) bias instead of zeros

    @property
    def id(self) -> str:
        s = f"{self.kernel}-{self.B}x{self.H}x{self.Lq}x{self.Lk}x{self.hd}-{self.family}"
        if self.family != "planted":
            s += f"{self.scale:g}"
        for flag, name in ((self.causal, "causal"), (self.form, self.form), (self.mask, self.mask), (self.noisy, "noisy")):
            if flag:
                s += "-" + str(name)
        return s

    @property
    def f32(self) -> bool:
        return self.kernel in ("generic_f32", "mfma_f32")


def planted_positions(Lk: int) -> list[int]:
    """Keys where a running max must jump: fixed block edges, the last key, first and last key of every 64-key tile."""
    pos = {0, 15, 16, 31, 32, 63, 64, Lk - 1}
    for t in range(0, Lk, 64):
        pos.update((t, min(t + 63, Lk - 1)))
    return sorted(p for p in pos if 0 <= p < Lk)


def _seed(case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def keep_mask(case: Case) -> torch.Tensor | None:
    """(B, 1, Lq, Lk) bool, True = key may be seen; None without a mask."""
    if case.mask is None:
        return None
    B, Lq, Lk = case.B, case.Lq, case.Lk
    keep = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if case.mask == "trail":  # per-batch lengths, at least one key
        for b in range(B):
            keep[b, :, :, 1 + (b * 37 + Lk // 2) % Lk:] = False
    elif case.mask.startswith("lead"):  # left padding of p keys; batch element 0 pads one key less.  Capped so that a key stays
        p = min(int(case.mask[4:]), Lk - 1, Lq - 1 if case.causal else Lk)  # and, under causal, a live query row stays
        for b in range(B):
            keep[b, :, :, : p - (1 if b == 0 and p > 1 else 0)] = False
    elif case.mask == "holes":  # random interior holes (the same for every query), first and last key kept
        g = torch.Generator().manual_seed(_seed(case))
        hole = torch.rand(B, 1, 1, Lk, generator=g) < 0.5
        hole[..., 0] = hole[..., -1] = False
        keep = keep & ~hole
    elif case.mask == "checker":
        i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
        keep = keep & ((i + j) % 2 == 0)
    elif case.mask == "deadbatch":
        keep[B - 1] = False
    else:
        raise ValueError(case.mask)
    return keep


def build(case: Case) -> dict:
    """Inputs of a case, all bf16-rounded fp32 CPU tensors: q (B, Lq, H*hd), k / v (B, Lk, H*hd), bias = the DENSE broadcastable
    f32 bias (b, h, Lq, Lk) or None (place_bias() lays it out as case.form on a device), keep = the bool mask or None."""
    B, H, Lq, Lk, hd = case.B, case.H, case.Lq, case.Lk, case.hd
    sd = _seed(case)
    amp = math.sqrt(case.scale) if case.family != "planted" else 1.0
    q = synth_input("adv_q", (B, Lq, H * hd), sd, scale=amp)
    k = bf16r(synth_input("adv_k", (B, Lk, H * hd), sd + 1, scale=amp))
    v = bf16r(synth_input("adv_v", (B, Lk, H * hd), sd + 2))
    if case.family == "planted":
        # every query row gets ONE dominant key: q_i += 40 k_j / |k_j| lifts the scaled score of key j by 40 |k_j| / sqrt(hd)
        # (about 40) and moves the others by 40 N(0, 1) / sqrt(hd)
        pos = torch.tensor(planted_positions(Lk))
        g = torch.Generator().manual_seed(sd)
        j = pos[torch.randint(len(pos), (B, H, Lq), generator=g)]
        kj = torch.gather(split_heads(k, H), 2, j[..., None].expand(B, H, Lq, hd))
        q = merge_heads(split_heads(q, H) + 40.0 * kj / kj.norm(dim=-1, keepdim=True))
    q = bf16r(q)
    bias, keep = None, keep_mask(case)
    if case.form is not None:
        b0 = 1 if case.form in ("1H", "11", "expand") else B
        h0 = 1 if case.form in ("B1", "11", "expand") else H
        if case.family == "bias" or case.noisy:
            bias = synth_input("adv_bias", (b0, h0, Lq, Lk), sd + 3, scale=3.0)
        else:
            bias = torch.zeros(b0, h0, Lq, Lk)
        if keep is not None:
            assert b0 == B, "masks are per batch element"
            bias = bias.masked_fill(~keep, NEG_INF)
    return {"q": q, "k": k, "v": v, "bias": bias, "keep": keep}


def place_bias(bias: torch.Tensor, case: Case, device) -> torch.Tensor:
    """The dense bias in the memory layout of case.form, shape (b, h, Lq, Lk) as ops.attention takes it."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    bias = bias.to(device)
    if case.form == "expand":  # stride-0 batch and head dims
        out = bias.expand(B, H, Lq, Lk)
        assert out.stride(0) == 0 and out.stride(1) == 0
    elif case.form == "off4":  # a view one float past a 16-byte boundary: 4-byte aligned, legal, scalar loads
        buf = torch.empty(bias.numel() + 1, dtype=torch.float32, device=device)
        out = buf[1:].view(bias.shape)
        out.copy_(bias)
        assert out.data_ptr() % 16 == 4
    elif case.form == "padrow":  # rows padded to a multiple of 4 floats: 16-byte loads even when Lk % 4 != 0 (ragged last group)
        ld = (Lk + 3) // 4 * 4 + 4
        buf = torch.full((*bias.shape[:3], ld), float("nan"), dtype=torch.float32, device=device)
        out = buf[..., :Lk]
        out.copy_(bias)
    else:
        out = bias.contiguous()
    return out


def bias_vector_path(bias: torch.Tensor) -> bool:
    """Whether attn_fwd_hd64's 16-byte bias loads apply (attention_bf16.hip: base and every used stride a multiple of 16 bytes)."""
    sb = 0 if bias.shape[0] == 1 else bias.stride(0)
    sh = 0 if bias.shape[1] == 1 else bias.stride(1)
    return not ((bias.data_ptr() | (sb * 4) | (sh * 4) | (bias.stride(2) * 4)) & 15)


def expected_kernel(case: Case) -> str:
    """The dispatch rule of pytorch_models._hip.ops.attention / attention_f32 + the C ABI, from the shape alone."""
    if case.f32:
        return "mfma_f32" if case.hd == 64 and not case.causal and case.form is None else "generic_f32"
    if case.hd != 64:
        return "generic_bf16"
    if case.form is not None:
        return "tiled_bias"
    return "head" if not case.causal and case.Lq <= 256 and case.Lk <= 256 else "tiled"


def reference(case: Case, inp: dict):
    """(want, A, dead) in the merged layout: (B, Lq, H*hd), (B, Lq, H*hd), (B, H, Lq)."""
    qh, kh, vh = (split_heads(inp[n], case.H) for n in ("q", "k", "v"))
    want, A, dead = ref_attention(qh, kh, vh, inp["bias"], case.causal)
    return merge_heads(want), merge_heads(A), dead.expand(case.B, case.H, case.Lq)


def _cases() -> list[Case]:
    C = []
    # ---- attn_head_hd64: persistent per-head kernel, no mask
    for (Lq, Lk) in ((165, 197), (256, 256), (33, 17), (1, 255)):
        for sc in (1.0, 8.0, 30.0):
            C.append(Case("head", 2, 2, Lq, Lk, scale=sc))
        C.append(Case("head", 2, 2, Lq, Lk, family="planted"))
    C.append(Case("head", 100, 3, 33, 17, scale=8.0))  # 300 heads > CU count: every workgroup walks both LDS buffers
    C.append(Case("head", 90, 3, 165, 197, family="planted"))
    # ---- attn_fwd_hd64 plain / causal
    for (Lq, Lk, causal) in ((130, 577, False), (448, 257, False), (300, 300, True), (6, 9, True)):
        for sc in (1.0, 8.0, 30.0):
            C.append(Case("tiled", 2, 2, Lq, Lk, scale=sc, causal=causal))
        C.append(Case("tiled", 2, 2, Lq, Lk, family="planted", causal=causal))
    C.append(Case("tiled", 1, 2, 1500, 1500, family="planted"))
    C.append(Case("tiled", 1, 1, 1500, 1500, scale=8.0, causal=True))
    # ---- attn_fwd_hd64 _bias: every layout on a 16-byte-load shape (Lk % 4 == 0) and a scalar one, then the other shapes
    for form in BIAS_FORMS:
        C.append(Case("tiled_bias", 2, 3, 128, 256, family="bias", scale=4.0, form=form))
        C.append(Case("tiled_bias", 2, 3, 70, 133, family="bias", scale=4.0, form=form, causal=form in ("1H", "padrow")))
    for (Lq, Lk, causal) in ((197, 200, False), (9, 6, False), (300, 321, True), (300, 321, False), (197, 200, True)):
        C.append(Case("tiled_bias", 2, 2, Lq, Lk, family="bias", scale=8.0, form="BH", causal=causal))
    C.append(Case("tiled_bias", 1, 2, 600, 1500, family="bias", scale=8.0, form="1H"))
    for mask in MASKS:
        for causal in (False, True):
            C.append(Case("tiled_bias", 3, 2, 197, 200, family="mask", scale=4.0, form="BH", mask=mask, causal=causal, noisy=causal))
    for mask in ("trail", "holes"):  # diffuse rows under a mask (the unbiased-row-sum property needs many comparable keys)
        C.append(Case("tiled_bias", 2, 2, 130, 600, family="mask", scale=1.0, form="BH", mask=mask))
    for (Lq, Lk) in ((70, 133), (128, 256), (300, 321), (9, 6)):
        for mask, causal in (("lead65", True), ("holes", False), ("trail", True), ("deadbatch", False), ("deadbatch", True)):
            C.append(Case("tiled_bias", 2, 2, Lq, Lk, family="mask", scale=4.0, form="B1", mask=mask, causal=causal, noisy=Lk == 321))
    # ---- generic kernels: every head dim, shapes in rotation; bias, causal, masks
    shapes = ((49, 256), (257, 257), (6, 9))
    for i, hd in enumerate((16, 20, 32, 36, 60, 80, 128)):
        Lq, Lk = shapes[i % 3]
        Lq2, Lk2 = shapes[(i + 1) % 3]
        C.append(Case("generic_bf16", 2, 2, Lq, Lk, hd, scale=8.0))
        C.append(Case("generic_bf16", 2, 2, Lq2, Lk2, hd, family="planted", causal=True))
        C.append(Case("generic_bf16", 2, 2, Lq, Lk, hd, family="bias", scale=4.0, form=BIAS_FORMS[i]))
        C.append(Case("generic_bf16", 2, 2, Lq2, Lk2, hd, family="mask", scale=4.0, form="BH", mask=MASKS[i], causal=i % 2 == 0))
        C.append(Case("generic_bf16", 2, 2, Lq, Lk, hd, family="mask", scale=4.0, form="B1", mask="lead65", causal=True, noisy=True))
        C.append(Case("generic_bf16", 2, 2, Lq2, Lk2, hd, family="mask", scale=4.0, form="BH", mask="deadbatch"))
    C.append(Case("generic_bf16", 2, 2, 257, 257, 32, family="mask", scale=4.0, form="BH", mask="checker", causal=True))
    for (Lq, Lk) in shapes:
        for sc in F32_SCALES:
            C.append(Case("mfma_f32", 2, 2, Lq, Lk, 64, scale=sc))
        C.append(Case("mfma_f32", 2, 2, Lq, Lk, 64, family="planted"))
        C.append(Case("generic_f32", 2, 2, Lq, Lk, 64, family="bias", scale=4.0, form="BH"))
        C.append(Case("generic_f32", 2, 2, Lq, Lk, 64, family="planted", causal=True))
        C.append(Case("generic_f32", 2, 2, Lq, Lk, 32, family="bias", scale=4.0, form="expand", causal=True))
        for i, mask in enumerate(MASKS + ("deadbatch",)):
            C.append(Case("generic_f32", 2, 2, Lq, Lk, 64, family="mask", scale=4.0, form="BH", mask=mask, causal=i % 2 == 1, noisy=mask == "holes"))
    return C


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
MASKED_CASES = [c for c in CASES if c.mask is not None]
DIFFUSE_CASES = [c for c in CASES if c.kernel in ("head", "tiled", "tiled_bias") and c.scale == 1.0 and c.family in ("scale", "mask")
                 and c.Lk >= 197]


# --------------------------------------------------------------------------------------------------------------- window attention
@dataclass(frozen=True)
class WCase:
    N: int
    Himg: int
    Wimg: int
    heads: int
    ws: int
    mode: str              # block | grid
    scale: float = 1.0
    bias_amp: float = 0.0  # 0 = no bias; else the bias is uniform in +-bias_amp
    dead: bool = False     # head 0: every query misses key 0, query token 1 sees no key at all, token 2 only the LAST key

    @property
    def id(self) -> str:
        return (f"win-{self.N}x{self.Himg}x{self.Wimg}-h{self.heads}-ws{self.ws}-{self.mode}-s{self.scale:g}-b{self.bias_amp:g}"
                + ("-dead" if self.dead else ""))

    @property
    def nwork(self) -> int:
        return self.N * (self.Himg // self.ws) * (self.Wimg // self.ws) * self.heads


WCASES = [
    WCase(2, 14, 14, 3, 7, "block", 1.0, 10.0),
    WCase(2, 14, 14, 3, 7, "grid", 8.0, 10.0),
    WCase(1, 14, 21, 5, 7, "block", 30.0, 0.0),
    WCase(1, 21, 14, 5, 7, "grid", 30.0, 10.0),
    WCase(3, 10, 15, 1, 5, "grid", 8.0, 10.0),
    WCase(3, 10, 5, 1, 5, "block", 30.0, 3.0),
    WCase(1, 16, 24, 16, 8, "block", 8.0, 10.0),
    WCase(1, 8, 16, 16, 8, "grid", 30.0, 0.0),
    WCase(1, 16, 8, 3, 8, "grid", 4.0, 3.0, True),
    WCase(2, 14, 7, 5, 7, "block", 4.0, 3.0, True),
    WCase(1, 15, 10, 3, 5, "block", 4.0, 10.0, True),
]
assert any(c.nwork % 4 for c in WCASES)


def window_partition(x: torch.Tensor, c: WCase) -> torch.Tensor:
    """(N*Himg*Wimg, C) pixel rows -> (windows, ws*ws, C), tokens row-major inside a window; 'block' = contiguous ws x ws blocks,
    'grid' = pixels Himg/ws (Wimg/ws) apart (pytorch_models/image/maxvit.py)."""
    N, Hh, Ww, ws, C = c.N, c.Himg, c.Wimg, c.ws, x.shape[-1]
    nWy, nWx = Hh // ws, Ww // ws
    if c.mode == "block":
        y = x.reshape(N, nWy, ws, nWx, ws, C).permute(0, 1, 3, 2, 4, 5)
    else:
        y = x.reshape(N, ws, nWy, ws, nWx, C).permute(0, 2, 4, 1, 3, 5)
    return y.reshape(N * nWy * nWx, ws * ws, C)


def window_unpartition(y: torch.Tensor, c: WCase) -> torch.Tensor:
    """Inverse of window_partition: (windows, ws*ws, C) -> (N*Himg*Wimg, C) pixel rows."""
    N, Hh, Ww, ws, C = c.N, c.Himg, c.Wimg, c.ws, y.shape[-1]
    nWy, nWx = Hh // ws, Ww // ws
    y = y.reshape(N, nWy, nWx, ws, ws, C)
    y = y.permute(0, 1, 3, 2, 4, 5) if c.mode == "block" else y.permute(0, 3, 1, 4, 2, 5)
    return y.reshape(N * Hh * Ww, C)


def build_window(c: WCase) -> dict:
    """q, k, v (N*Himg*Wimg, 32*heads) bf16-rounded fp32, bias (heads, L, L) f32 or None."""
    M, D, L = c.N * c.Himg * c.Wimg, 32 * c.heads, c.ws * c.ws
    sd = _seed(c)
    amp = math.sqrt(c.scale)
    out = {"q": bf16r(synth_input("adv_wq", (M, D), sd, scale=amp)), "k": bf16r(synth_input("adv_wk", (M, D), sd + 1, scale=amp)),
           "v": bf16r(synth_input("adv_wv", (M, D), sd + 2)), "bias": None}
    if c.bias_amp:
        g = torch.Generator().manual_seed(sd)
        bias = (torch.rand(c.heads, L, L, generator=g) * 2 - 1) * c.bias_amp
        if c.dead:
            bias[0, :, 0] = NEG_INF
            bias[0, 1, :] = NEG_INF
            bias[0, 2, : L - 1] = NEG_INF
        out["bias"] = bias
    return out


def reference_window(c: WCase, inp: dict):
    """(want, A, dead) in window layout: (windows, L, 32*heads) twice, (windows, heads, L)."""
    qh, kh, vh = (split_heads(window_partition(inp[n], c), c.heads) for n in ("q", "k", "v"))
    bias = None if inp["bias"] is None else inp["bias"][None]
    want, A, dead = ref_attention(qh, kh, vh, bias)
    return merge_heads(want), merge_heads(A), dead


# --------------------------------------------------------------------------------------------------------------- decode attention
@dataclass(frozen=True)
class DCase:
    B: int
    H: int
    T: int
    lk: int
    family: str = "scale"  # scale (score deviation 8) | planted (one key with score 30 per (b, h): first, last, tile edges)

    @property
    def id(self) -> str:
        return f"dec-{self.B}x{self.H}-T{self.T}-lk{self.lk}-{self.family}"


DCASES = [DCase(4, 8, max(lk, 16) + (lk % 2) * 8, lk, fam) for lk in (1, 64, 65, 129, 512, 513, 1024, 1025, 1500, 1537) for fam in ("scale", "planted")]


def build_decode(c: DCase, per_batch_q: bool = True) -> dict:
    """q (B, H*64) fp32 (bf16 values), k / v (B, H, T, 64) bf16-rounded fp32.  per_batch_q False: one query per head shared by the
    batch (the fused kernels' query is LayerNorm(x) W^T + bias; with W = 0 it is the bias, exactly)."""
    B, H, T, lk = c.B, c.H, c.T, c.lk
    sd = _seed(c)
    amp = math.sqrt(8.0) if c.family == "scale" else 1.0
    q = bf16r(synth_input("adv_dq", (B if per_batch_q else 1, H * 64), sd, scale=amp).expand(B, H * 64).clone())
    k = bf16r(synth_input("adv_dk", (B, H, T, 64), sd + 1, scale=amp))
    v = bf16r(synth_input("adv_dv", (B, H, T, 64), sd + 2))
    if c.family == "planted":
        pos = [0, lk - 1] + planted_positions(lk)
        for b in range(B):
            for h in range(H):
                qv = q[b, h * 64:(h + 1) * 64]
                k[b, h, pos[(b * H + h) % len(pos)]] = 30.0 * 8.0 * qv / qv.square().sum()  # this key's scaled score: 30
        k = bf16r(k)
    return {"q": q, "k": k, "v": v}


def reference_decode(c: DCase, inp: dict):
    """(want, A): (B, H*64) float64 each."""
    q = inp["q"].view(c.B, c.H, 1, 64)
    want, A, _ = ref_attention(q, inp["k"][:, :, : c.lk], inp["v"][:, :, : c.lk])
    return want.reshape(c.B, c.H * 64), A.reshape(c.B, c.H * 64)
