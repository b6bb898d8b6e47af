"""Cases, inputs and the float64 reference of the variable-length (packed) attention tests: tests/test_varlen_cases_cpu.py
without a GPU, tests/test_hip_varlen_kernels.py on one.  A plain helper module.

Reference = tests/attn_cases.py's float64 attention, applied to every sequence of the packed batch alone; the bound is that
module's bf16 contract (|got - want| <= u (A + |want|), the GPU test asserts 1.5 x).  The length sets sit on the edges of the
tiled kernel: its 128-query block, the 32 queries of a wave, the 64-key tile and its 32-key half; every set but the last holds a
sequence of length 0 or sequences that start in the middle of another one's block.  q / k / v are column slices of ONE
(T_total + SLACK, 3 * H * 64) buffer, as the models hand them over, with SLACK rows that belong to no sequence behind the data.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

from attn_cases import bf16_bound, bf16r, bound_ratio, emulate_bf16_kernel, planted_positions, ref_attention, split_heads  # noqa: F401
from synthweights import synth_input

LENGTH_SETS = ((1, 33, 64, 0, 129), (31, 32, 65, 127, 128), (191, 193, 63, 0, 0, 2), (257, 1, 300))
HEADS = (2, 3)
SLACK = 5


@dataclass(frozen=True)
class Case:
    lengths: tuple
    H: int
    family: str = "scale"   # scale | planted
    scale: float = 1.0      # standard deviation of the scaled scores q.k / 8 (family "scale")
    causal: bool = False

    @property
    def id(self) -> str:
        s = "-".join(str(n) for n in self.lengths) + f"-H{self.H}-{self.family}"
        if self.family == "scale":
            s += f"{self.scale:g}"
        return s + ("-causal" if self.causal else "")

    @property
    def total(self) -> int:
        return sum(self.lengths)

    @property
    def cu(self) -> list[int]:
        out = [0]
        for n in self.lengths:
            out.append(out[-1] + n)
        return out


CASES = [Case(ls, H, fam, sc, causal) for ls in LENGTH_SETS for H in HEADS
         for fam, sc in (("scale", 1.0), ("scale", 30.0), ("planted", 1.0)) for causal in (False, True)]


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.id)) % 100003


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """(1, H, n, 64) -> (n, H * 64)"""
    return x[0].transpose(0, 1).reshape(x.shape[2], -1)


@lru_cache(maxsize=None)
def build(case: Case) -> torch.Tensor:
    """The (T_total + SLACK, 3 * H * 64) buffer of a case, bf16-rounded fp32 on the CPU: columns [q | k | v].  Shared - do not write."""
    T, D = case.total, case.H * 64
    sd = _seed(case)
    amp = math.sqrt(case.scale) if case.family == "scale" else 1.0
    q = synth_input("vl_q", (T + SLACK, D), sd, scale=amp)
    k = bf16r(synth_input("vl_k", (T + SLACK, D), sd + 1, scale=amp))
    v = bf16r(synth_input("vl_v", (T + SLACK, D), sd + 2))
    if case.family == "planted":  # one dominant key per query row, at the tile edges of ITS OWN sequence (attn_cases.build)
        g = torch.Generator().manual_seed(sd)
        for r0, n in zip(case.cu, case.lengths):
            if n == 0:
                continue
            pos = torch.tensor(planted_positions(n))
            j = pos[torch.randint(len(pos), (case.H, n), generator=g)]
            kh = k[r0 : r0 + n].view(n, case.H, 64).transpose(0, 1)  # (H, n, 64)
            kj = torch.gather(kh, 1, j[..., None].expand(case.H, n, 64))
            qh = q[r0 : r0 + n].view(n, case.H, 64).transpose(0, 1) + 40.0 * kj / kj.norm(dim=-1, keepdim=True)
            q[r0 : r0 + n] = qh.transpose(0, 1).reshape(n, D)
    return torch.cat([bf16r(q), k, v], 1)


def qkv(case: Case, buf: torch.Tensor):
    """The q / k / v views (T_total, H * 64) of a buffer laid out like build()'s: column slices, the slack rows cut off."""
    T, D = case.total, case.H * 64
    return buf[:T, :D], buf[:T, D : 2 * D], buf[:T, 2 * D :]


def sequences(case: Case):
    """(b, first row, length) of every sequence that has rows."""
    return [(b, r0, n) for b, (r0, n) in enumerate(zip(case.cu, case.lengths)) if n]


def _per_sequence(case: Case, fn):
    q, k, v = qkv(case, build(case))
    outs = []
    for _, r0, n in sequences(case):
        outs.append(fn(*(split_heads(t[r0 : r0 + n][None], case.H) for t in (q, k, v))))
    return outs


@lru_cache(maxsize=None)
def reference(case: Case):
    """float64 (want, A), each (T_total, H * 64): every sequence attends to itself alone.  Shared - do not write."""
    outs = _per_sequence(case, lambda q, k, v: ref_attention(q, k, v, None, case.causal)[:2])
    return torch.cat([merge_heads(w) for w, _ in outs], 0), torch.cat([merge_heads(a) for _, a in outs], 0)


def emulate(case: Case) -> torch.Tensor:
    """The bf16 kernels' arithmetic on the CPU (attn_cases.emulate_bf16_kernel), per sequence -> (T_total, H * 64)."""
    return torch.cat([merge_heads(o) for o in _per_sequence(case, lambda q, k, v: emulate_bf16_kernel(q, k, v, None, case.causal))], 0)
