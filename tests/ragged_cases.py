"""Reference and cases of the ragged-prompt kernels, shared by tests/test_ragged_cases_cpu.py (no GPU),
tests/test_hip_ragged_kernels.py and tests/test_hip_ragged.py.  A plain helper module in the manner of prefill_cases.py.

Sequences of different prompt lengths are RIGHT-ALIGNED in the caches: row b's first token sits at cache position start_b, the
keys below it are padding.  The two attention kernels are defined by an explicit keep-mask:

    pm_prefill_attention_ragged_bf16 : the query at position p = p0 + i of row b keeps keys lo(p) <= j <= p, lo(p) = min(start_b, p)
                                       (a padded query, p < start_b, sees itself only);
    pm_dec_attention_ragged          : row b keeps keys lo_b <= j < Lk, lo_b = min(start_b, Lk - 1).

The float64 reference is attn_cases.ref_attention under that mask, so ``want`` and ``A`` come from the code every other attention
kernel is held to and the bound is the derived one of attn_cases.py: 1.5 u (A + |want|), u = 2^-8 (bound_ratio <= 1.5).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import prefill_cases as PC
from attn_cases import NEG_INF, bf16r, merge_heads, ref_attention, split_heads
from synthweights import synth_input, synth_tokens

B, H = 3, 3  # three heads: a head stride that is no power of two; three rows: three start classes per case

# (p0, C) -> the rows' starts.  Over the list every class occurs (test_ragged_cases_cpu.py asserts it):
#   0                     : a full-length row
#   inside, off an edge   : p0 < start < p0 + C, start % 64 not in (0, 63) - a wave with padded AND valid queries
#   63 / 64 / 65          : on, before and behind a key-tile edge
#   old, mid-tile         : 0 < start < p0 off a tile edge - the mask cuts through the keys read from the caches
#   beyond                : start >= p0 + C - the row's whole chunk is padding
# (63, 2) with start 64 and (200, 130) with start 260 put queries whose first visible key lies one key tile BEHIND their wave's
# first tile into one wave with queries that start in it: the online softmax meets a fully masked tile first.
STARTS = {
    (0, 1): (0, 5, 0),
    (0, 33): (0, 17, 40),
    (0, 65): (63, 64, 65),
    (0, 130): (65, 97, 0),
    (63, 2): (0, 64, 30),
    (64, 64): (30, 100, 129),
    (200, 130): (100, 260, 331),
}
CHUNKS = tuple(STARTS)
EXACT_FIT = ((64, 64), (200, 130))  # lk_max == p0 + C; every other case leaves 5 unused cache positions behind the chunk


@dataclass(frozen=True)
class RCase:
    p0: int
    C: int
    family: str = "scale"  # scale | planted
    scale: float = 1.0

    @property
    def starts(self) -> tuple:
        return STARTS[(self.p0, self.C)]

    @property
    def lk_max(self) -> int:
        return self.p0 + self.C + (0 if (self.p0, self.C) in EXACT_FIT else 5)

    @property
    def id(self) -> str:
        return f"p{self.p0}-c{self.C}-{self.family}" + (f"{self.scale:g}" if self.family == "scale" else "")


CASES = [RCase(p0, C, fam, sc) for (p0, C) in CHUNKS for fam, sc in (("scale", 1.0), ("scale", 30.0), ("planted", 1.0))]
assert len({c.id for c in CASES}) == len(CASES)


def _seed(case) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("ragged-" + case.id)) % 100003


def planted_key(case: RCase, b: int, i: int) -> int:
    """The absolute position of the key that chunk row i of batch row b is aimed at.  Valid queries (p0 + i >= start_b) with
    i % 8 == 0 aim at start_b - 1 (MASKED: a leak by one position below the start becomes the whole answer), with i % 8 == 4 at
    start_b (the first visible key: a mask one position too tight loses the whole answer); the first valid query of the chunk takes
    both turns' place when it has neither (it aims at start_b - 1).  Everything else keeps prefill_cases.planted_key's targets
    (the future key, an old key, the last visible key)."""
    p, st = case.p0 + i, case.starts[b]
    if p >= st:
        first_valid = i == max(0, st - case.p0)
        if st >= 1 and (i % 8 == 0 or first_valid):
            return st - 1
        if i % 8 == 4:
            return st
    return PC.planted_key(PC.PCase(case.p0, case.C), i)


def build(case: RCase) -> dict:
    """bf16-rounded fp32 CPU tensors: q, k, v (B, C, H*64) of the chunk, k_old, v_old (B, H, p0, 64) of the caches, starts (B,)."""
    p0, C = case.p0, case.C
    sd = _seed(case)
    amp = math.sqrt(case.scale) if case.family == "scale" else 1.0
    q = synth_input("rg_q", (B, C, H * 64), sd, scale=amp)
    k = bf16r(synth_input("rg_k", (B, C, H * 64), sd + 1, scale=amp))
    v = bf16r(synth_input("rg_v", (B, C, H * 64), sd + 2))
    k_old = bf16r(synth_input("rg_ko", (B, H, p0, 64), sd + 3, scale=amp))
    v_old = bf16r(synth_input("rg_vo", (B, H, p0, 64), sd + 4))
    if case.family == "planted":  # prefill_cases.build's marks and dominant keys, the target chosen per batch row
        kall = torch.cat([k_old, split_heads(k, H)], 2)
        vall = torch.cat([v_old, split_heads(v, H)], 2)
        for j in range(p0 + C):
            vall[:, :, j, j % 64] += 16.0
        vall = bf16r(vall)
        v_old, v = vall[:, :, :p0].contiguous(), merge_heads(vall[:, :, p0:])
        qh = split_heads(q, H).clone()
        for b in range(B):
            for i in range(C):
                kj = kall[b, :, planted_key(case, b, i)]
                qh[b, :, i] += 40.0 * kj / kj.norm(dim=-1, keepdim=True)
        q = merge_heads(qh)
    return {"q": bf16r(q), "k": k, "v": v, "k_old": k_old, "v_old": v_old, "starts": torch.tensor(case.starts, dtype=torch.int64)}


def keep_mask(p0: int, C: int, starts) -> torch.Tensor:
    """(B, C, p0 + C) bool: the query at p = p0 + i of row b keeps keys min(start_b, p) <= j <= p"""
    p = (p0 + torch.arange(C))[None, :, None]
    j = torch.arange(p0 + C)[None, None, :]
    lo = torch.minimum(torch.as_tensor(starts, dtype=torch.int64)[:, None, None], p)
    return (j >= lo) & (j <= p)


def valid_rows(p0: int, C: int, starts) -> torch.Tensor:
    """(B, C) bool: the queries that belong to their row's prompt (position >= start_b)"""
    return (p0 + torch.arange(C))[None, :] >= torch.as_tensor(starts, dtype=torch.int64)[:, None]


def ref_prefill(q, k, v, k_old, v_old, starts, shift: int = 0):
    """One launch in float64 -> (want, A (B, C, H*64)).  ``shift`` moves the lower edge of the mask (tests of the tests: -1 leaks
    the key below the start, +1 loses the first visible key; the query's own key always stays)."""
    n_heads = k_old.shape[1]
    p0, C = k_old.shape[2], q.shape[1]
    k_all = torch.cat([k_old, split_heads(k, n_heads)], 2)
    v_all = torch.cat([v_old, split_heads(v, n_heads)], 2)
    bias = _bias(p0, C, starts, shift)
    want, A, dead = ref_attention(split_heads(q, n_heads), k_all, v_all, bias)
    assert not dead.any()  # key p is visible to query p
    return merge_heads(want), merge_heads(A)


def _bias(p0: int, C: int, starts, shift: int = 0) -> torch.Tensor:
    keep = keep_mask(p0, C, starts)
    if shift:
        p = (p0 + torch.arange(C))[None, :, None]
        j = torch.arange(p0 + C)[None, None, :]
        lo = torch.minimum(torch.as_tensor(starts, dtype=torch.int64)[:, None, None] + shift, p).clamp(min=0)
        keep = (j >= lo) & (j <= p)
    return torch.zeros(keep.shape[0], 1, C, p0 + C, dtype=torch.float64).masked_fill(~keep[:, None], NEG_INF)


def reference(case: RCase, inp: dict):
    return ref_prefill(inp["q"], inp["k"], inp["v"], inp["k_old"], inp["v_old"], inp["starts"])


# ---- the step attention: one query per row over the first Lk cache positions ----
@dataclass(frozen=True)
class SCase:
    Lk: int
    family: str = "scale"  # scale | planted

    @property
    def starts(self) -> tuple:
        return (0, 3, self.Lk - 1, self.Lk + 2)  # a full row, a short prefix of padding, one key left, a clamped start (>= Lk)

    @property
    def T(self) -> int:
        return self.Lk + (5 if self.Lk % 2 else 0)  # odd Lk: unused cache positions behind the keys

    @property
    def id(self) -> str:
        return f"lk{self.Lk}-{self.family}"


SB = 4  # rows of a step case: one per start
SCASES = [SCase(lk, fam) for lk in (1, 5, 129, 300) for fam in ("scale", "planted")]


def step_lo(case: SCase) -> list:
    return [max(0, min(s, case.Lk - 1)) for s in case.starts]


def build_step(case: SCase) -> dict:
    """q f32 (SB, H*64), k / v bf16-rounded (SB, H, T, 64); planted: row b is aimed at key lo_b - 1 where there is one (masked; at lo_b
    otherwise) and every key carries prefill_cases' one-hot mark in V"""
    sd = _seed(case)
    q = synth_input("rs_q", (SB, H * 64), sd)
    k = bf16r(synth_input("rs_k", (SB, H, case.T, 64), sd + 1))
    v = bf16r(synth_input("rs_v", (SB, H, case.T, 64), sd + 2))
    if case.family == "planted":
        for j in range(case.T):
            v[:, :, j, j % 64] += 16.0
        v = bf16r(v)
        qh = q.view(SB, H, 64).clone()
        for b, lo in enumerate(step_lo(case)):
            kj = k[b, :, lo - 1 if lo >= 1 else lo]
            qh[b] += 40.0 * kj / kj.norm(dim=-1, keepdim=True)
        q = qh.view(SB, H * 64)
    return {"q": q, "k": k, "v": v, "starts": torch.tensor(case.starts, dtype=torch.int64)}


def reference_step(case: SCase, inp: dict):
    """(want, A) (SB, H*64) float64"""
    lo = torch.tensor(step_lo(case))
    keep = torch.arange(case.Lk)[None, :] >= lo[:, None]
    bias = torch.zeros(SB, 1, 1, case.Lk, dtype=torch.float64).masked_fill(~keep[:, None, None], NEG_INF)
    want, A, dead = ref_attention(inp["q"].view(SB, H, 1, 64), inp["k"][:, :, : case.Lk], inp["v"][:, :, : case.Lk], bias)
    assert not dead.any()
    return want.reshape(SB, H * 64), A.reshape(SB, H * 64)


# ---- the end-to-end runs (tests/test_hip_ragged.py; their seeds are pinned on the CPU by tests/test_ragged_cases_cpu.py) ----
GPT2_SEED, GPT2_P, GPT2_LENGTHS, GPT2_NEW = 72, 40, (40, 23, 1), 12  # GPT2(2, 128), fill_module seed 72: test_hip_prefill.py's


def gpt2_prompt() -> torch.Tensor:
    """(3, 40) int64 ids below 2000; row b's prompt is its first GPT2_LENGTHS[b] ids, the rest is padding the decoders must ignore"""
    # token seed 101: of the seeds 93 .. 109 the one whose per-row oracle runs have the largest smallest top-2 margin (0.046), chosen
    # on the CPU before any device run; test_ragged_cases_cpu.py pins that the all-rounded oracle loop keeps every row's ids
    return synth_tokens("ragged_tok", (len(GPT2_LENGTHS), GPT2_P), 2000, 101)


WHISPER_P, WHISPER_LENGTHS, WHISPER_NEW = 4, (4, 2), 12  # Whisper tiny, seed 55, memory (2, 96, 384): test_hip_prefill.py's


def whisper_prompt() -> torch.Tensor:
    return synth_tokens("ragged_wprompt", (len(WHISPER_LENGTHS), WHISPER_P), 51865, 55)
