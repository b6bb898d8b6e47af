"""Reference and cases of pm_prefill_attention_bf16 ("append a chunk to the caches, attend with absolute-position causality"),
shared by tests/test_prefill_cases_cpu.py (no GPU) and tests/test_hip_prefill_kernel.py.  A plain helper module.

The reference is attn_cases.ref_attention (float64) over [old keys | the chunk's keys] with an explicit keep-mask
j <= p0 + i, so ``want`` and ``A`` come from the code every other attention kernel is held to, and the bound is the derived
one of attn_cases.py (1.5 u (A + |want|), u = 2^-8): rows sums over the unrounded fp32 p, P rounded to bf16 for P.V.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from attn_cases import NEG_INF, bf16r, merge_heads, ref_attention, split_heads
from synthweights import synth_input

B, H = 2, 3  # three heads: a head stride that is no power of two
# one query; ragged and exact 32 / 64 tiles; a chunk boundary inside (63, 65) and on (64) a key tile; several tiles of old keys
CHUNKS = ((0, 1), (0, 31), (0, 32), (0, 33), (0, 64), (0, 65), (0, 130), (1, 1), (63, 2), (64, 64), (65, 33), (200, 130))
EXACT_FIT = ((0, 64), (64, 64), (200, 130))  # lk_max == p0 + C; every other case leaves 5 unused cache positions behind the chunk


@dataclass(frozen=True)
class PCase:
    p0: int
    C: int
    family: str = "scale"  # scale | planted
    scale: float = 1.0     # standard deviation of the scaled scores (scale family)

    @property
    def lk_max(self) -> int:
        return self.p0 + self.C + (0 if (self.p0, self.C) in EXACT_FIT else 5)

    @property
    def id(self) -> str:
        return f"p{self.p0}-c{self.C}-{self.family}" + (f"{self.scale:g}" if self.family == "scale" else "")


# scale 30: scores up to |s| ~ 200 (attn_cases' largest); scale 1: diffuse rows, where a lost key costs a visible share of the sum
CASES = [PCase(p0, C, fam, sc) for (p0, C) in CHUNKS for fam, sc in (("scale", 1.0), ("scale", 30.0), ("planted", 1.0))]
assert len({c.id for c in CASES}) == len(CASES)
assert any(c.lk_max == c.p0 + c.C for c in CASES) and sum(c.lk_max > c.p0 + c.C for c in CASES) > len(CASES) // 2


def _seed(case: PCase) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % 100003


def planted_key(case: PCase, i: int) -> int:
    """The absolute position of the key that chunk row i is aimed at.  i % 4 == 1: the FUTURE in-chunk key p0 + i + 1 (masked: a
    leak by one position makes it the whole answer); i % 4 == 3 with old keys: an old key (first / last in turn); otherwise the
    LAST VISIBLE key p0 + i (a mask that is one position too tight loses the whole answer)."""
    if i % 4 == 1 and i + 1 < case.C:
        return case.p0 + i + 1
    if i % 4 == 3 and case.p0 > 0:
        return 0 if i % 8 == 3 else case.p0 - 1
    return case.p0 + i


def build(case: PCase) -> dict:
    """bf16-rounded fp32 CPU tensors: q, k, v (B, C, H*64) of the chunk, k_old, v_old (B, H, p0, 64) of the caches."""
    p0, C = case.p0, case.C
    sd = _seed(case)
    amp = math.sqrt(case.scale) if case.family == "scale" else 1.0
    q = synth_input("pf_q", (B, C, H * 64), sd, scale=amp)
    k = bf16r(synth_input("pf_k", (B, C, H * 64), sd + 1, scale=amp))
    v = bf16r(synth_input("pf_v", (B, C, H * 64), sd + 2))
    k_old = bf16r(synth_input("pf_ko", (B, H, p0, 64), sd + 3, scale=amp))
    v_old = bf16r(synth_input("pf_vo", (B, H, p0, 64), sd + 4))
    if case.family == "planted":
        # every key carries a one-hot mark in V (16 at dim key % 64); every query gets one dominant key: q_i += 40 k_j / |k_j|
        # lifts the scaled score of key j by about 40 and moves the others by 40 N(0, 1) / 8
        kall = torch.cat([k_old, split_heads(k, H)], 2)
        vall = torch.cat([v_old, split_heads(v, H)], 2)
        for j in range(p0 + C):
            vall[:, :, j, j % 64] += 16.0
        vall = bf16r(vall)
        v_old, v = vall[:, :, :p0].contiguous(), merge_heads(vall[:, :, p0:])
        qh = split_heads(q, H).clone()
        for i in range(C):
            kj = kall[:, :, planted_key(case, i)]
            qh[:, :, i] += 40.0 * kj / kj.norm(dim=-1, keepdim=True)
        q = merge_heads(qh)
    return {"q": bf16r(q), "k": k, "v": v, "k_old": k_old, "v_old": v_old}


def keep_mask(p0: int, C: int) -> torch.Tensor:
    """(1, 1, C, p0 + C) bool: query i of the chunk sits at p0 + i and sees keys j <= p0 + i"""
    return torch.arange(p0 + C)[None, :] <= (p0 + torch.arange(C))[:, None]


def ref_prefill(q, k, v, k_old, v_old):
    """One launch in float64.  q, k, v (B, C, H*64), k_old / v_old (B, H, p0, 64) -> (want, A (B, C, H*64), k_all, v_all
    (B, H, p0 + C, 64) = the caches afterwards)."""
    n_heads = k_old.shape[1]
    p0, C = k_old.shape[2], q.shape[1]
    k_all = torch.cat([k_old, split_heads(k, n_heads)], 2)
    v_all = torch.cat([v_old, split_heads(v, n_heads)], 2)
    bias = torch.zeros(1, 1, C, p0 + C, dtype=torch.float64).masked_fill(~keep_mask(p0, C)[None, None], NEG_INF)
    want, A, dead = ref_attention(split_heads(q, n_heads), k_all, v_all, bias)
    assert not dead.any()  # key 0 is visible to every query
    return merge_heads(want), merge_heads(A), k_all, v_all


def reference(case: PCase, inp: dict):
    want, A, _, _ = ref_prefill(inp["q"], inp["k"], inp["v"], inp["k_old"], inp["v_old"])
    return want, A
