"""Cases, tables and the float64 reference of the packed attention with a relative-position bias read by distance
(pm_attention_varlen_relbias_bf16): tests/test_relbias_cases_cpu.py without a GPU, tests/test_hip_relbias_kernels.py on one.
A plain helper module on top of tests/varlen_cases.py: its LENGTH_SETS, HEADS, SLACK, buffer layout ([q | k | v] column
slices of one buffer with slack rows) and its "scale" / "planted" q-k-v families are reused as they are.

    bias(h, q, k) = lut[h, clamp(k - q, -R, R) + R]        q, k positions inside the sequence

Radii.  R = 0 (one entry: every pair is clamped), R = 5 (the clamp is active inside every 64-key tile), R = 128 (T5's
max_distance; with the lengths 257 / 300 the clamp edge crosses 64-key tile and 128-query block boundaries).
Tables (fp32, (H, 2R + 1)):
    t5        RelativePositionBias.lut(True) of a module whose (H, 32) parameter is synthetic, standard deviation 2; the module's
              max_distance is its radius, so this family exists at R = 128 only
    distinct  every entry a different draw, standard deviation 2, nothing symmetric in the sign of k - q: a swapped sign or an
              index off by one moves probabilities by O(1).  Runs on the "planted" q / k / v as well as on "scale"
    window    as distinct, with -inf for |d| > 3 (at R = 0 there is no such entry: one finite value)
    dead      -inf for d <= 0, run causal: every visible key is masked, every row is dead and must come back exactly zero
Reference: attn_cases.ref_attention in float64 on every sequence alone with the dense (1, H, n, n) bias gathered from the table
on the host; bound: attn_cases.bf16_bound (the GPU test asserts 1.5 x, the CPU emulation stays within 1.0 x)."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import varlen_cases as VC
from attn_cases import bf16_bound, bound_ratio, emulate_bf16_kernel, ref_attention, split_heads  # noqa: F401
from varlen_cases import HEADS, LENGTH_SETS, SLACK, merge_heads  # noqa: F401

RADII = (0, 5, 128)
NEG_INF = float("-inf")


@dataclass(frozen=True)
class Case:
    lengths: tuple
    H: int
    table: str          # t5 | distinct | window | dead
    R: int
    causal: bool = False
    family: str = "scale"  # the q / k / v family of varlen_cases.build: scale (1.0) | planted

    @property
    def id(self) -> str:
        return ("-".join(str(n) for n in self.lengths) + f"-H{self.H}-{self.table}-R{self.R}-{self.family}"
                + ("-causal" if self.causal else ""))

    @property
    def vc(self) -> VC.Case:
        return VC.Case(self.lengths, self.H, self.family, 1.0, self.causal)

    @property
    def total(self) -> int:
        return sum(self.lengths)


def _cases() -> list[Case]:
    out = []
    for i, ls in enumerate(LENGTH_SETS):
        for j, R in enumerate(RADII):
            H = HEADS[(i + j) % 2]
            for causal in (False, True):
                out.append(Case(ls, H, "distinct", R, causal, "scale"))
                out.append(Case(ls, HEADS[(i + j + 1) % 2], "distinct", R, causal, "planted"))
                out.append(Case(ls, H, "window", R, causal))
                if R == 128:
                    out.append(Case(ls, H, "t5", R, causal))
            out.append(Case(ls, H, "dead", R, True))
    return out


CASES = _cases()
LIVE_CASES = [c for c in CASES if c.table != "dead"]
DEAD_CASES = [c for c in CASES if c.table == "dead"]


def _seed(case: Case) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(f"{case.table}-{case.R}-{case.H}-{case.lengths}")) % 100003


@lru_cache(maxsize=None)
def table(case: Case) -> torch.Tensor:
    """The (H, 2R + 1) fp32 table of a case.  Shared - do not write."""
    H, R = case.H, case.R
    g = torch.Generator().manual_seed(_seed(case))
    if case.table == "t5":
        from pytorch_models.text.t5 import RelativePositionBias

        rp = RelativePositionBias(H)
        assert rp.max_distance == R
        with torch.no_grad():
            rp.bias.copy_(2.0 * torch.randn(H, rp.n_buckets, generator=g))
        return rp.lut(True).clone()
    lut = 2.0 * torch.randn(H, 2 * R + 1, generator=g)
    d = torch.arange(-R, R + 1)
    if case.table == "window":
        lut[:, d.abs() > 3] = NEG_INF
    elif case.table == "dead":
        lut[:, d <= 0] = NEG_INF
    return lut


def dense(lut: torch.Tensor, n: int, R: int) -> torch.Tensor:
    """(H, n, n) bias gathered from an (H, >= 2R + 1) table: [h, q, k] = lut[h, clamp(k - q, -R, R) + R]."""
    idx = torch.arange(n, device=lut.device)
    return lut[:, (idx[None, :] - idx[:, None]).clamp(-R, R) + R]


def _per_sequence(case: Case, fn):
    q, k, v = VC.qkv(case.vc, VC.build(case.vc))
    lut = table(case)
    outs = []
    for _, r0, n in VC.sequences(case.vc):
        outs.append(fn(*(split_heads(t[r0 : r0 + n][None], case.H) for t in (q, k, v)), dense(lut, n, case.R)[None]))
    return outs


@lru_cache(maxsize=None)
def reference(case: Case):
    """float64 (want, A), each (T_total, H * 64): every sequence attends to itself alone under the gathered bias.  Shared."""
    outs = _per_sequence(case, lambda q, k, v, b: ref_attention(q, k, v, b, case.causal)[:2])
    return torch.cat([merge_heads(w) for w, _ in outs], 0), torch.cat([merge_heads(a) for _, a in outs], 0)


def emulate(case: Case) -> torch.Tensor:
    """The bf16 kernels' arithmetic on the CPU (attn_cases.emulate_bf16_kernel), per sequence -> (T_total, H * 64)."""
    return torch.cat([merge_heads(o) for o in _per_sequence(case, lambda q, k, v, b: emulate_bf16_kernel(q, k, v, b, case.causal))], 0)
