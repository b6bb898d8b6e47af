"""Shared by tests/test_t5_generate_cpu.py, tests/test_hip_t5_generate.py and tests/golden/make_golden_t5_generate.py: the
geometries, sources and lengths of the T5 generation tests, and the oracle's runs over them (oracle/ref_t5.py on the
bf16-rounded weights, CPU, fp32) - ids, teacher-forced logits and the top-2 margin of every decision.

A case decodes ``n`` decisions per row from the pad id; ``max_new_tokens = n`` corresponds to ``R5.greedy(sd, ids[:len], n + 1)``."""
import functools

import torch

from oracle import ref_t5 as R5
from synthweights import bf16_round_, fill_module, synth_tokens

MARGIN = 0.05  # the project's near-tie rule (test_hip_t5.py, test_hip_exact.py): a decision below it may go either way
LENGTHS8 = (64, 37, 5, 50, 64, 1, 23, 48)

# name -> (vocab, dim, heads, layers, mlp), weight seed, source name, (B, S), source seed, lengths, decisions per row
CASES = {
    "inner_ne_d": ((2000, 512, 6, 2, 1024), 94, "t5_gen_tok", (8, 64), 96, LENGTHS8, 16),   # 6 * 64 = 384 != 512
    "h8_l4": ((2000, 512, 8, 4, 1024), 94, "t5_gen_tok", (8, 64), 96, LENGTHS8, 32),      # the fixture's geometry
    "unfused": ((2000, 512, 8, 2, 1024), 97, "t5_gen_wide", (33, 32), 98, tuple(1 + (7 * b) % 32 for b in range(33)), 8),  # B * H = 264 > 256
    "long": ((2000, 512, 6, 2, 1024), 94, "t5_gen_long", (1, 16), 99, (16,), 159),          # 160 positions: distances beyond 128
}
TEACHER_FORCED = ("inner_ne_d", "h8_l4", "unfused", "long")


def build(case: str, rounded: bool = True):
    """(T5Model on the CPU in fp32, a copy of its state dict); ``rounded``: parameters rounded to bf16 values, as the GPU holds them"""
    from pytorch_models.text import T5Model

    geom, seed = CASES[case][:2]
    m = T5Model(*geom).eval()
    fill_module(m, seed)
    if rounded:
        bf16_round_(m)
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def sources(case: str):
    _, _, name, shape, seed, lengths, n = CASES[case]
    return synth_tokens(name, shape, 1000, seed), list(lengths), n


def run_oracle(sd: dict, tok, lengths, n: int) -> dict:
    ids, logits = [], []
    with torch.no_grad():
        for b, ln in enumerate(lengths):
            out, _ = R5.greedy(sd, tok[b, :ln], n + 1, eos_id=-1)
            ids.append(out)
            logits.append(R5.model(sd, tok[b, :ln], out))  # (n + 1, V): row t decides position t + 1
    ids, logits = torch.stack(ids), torch.stack(logits)
    top2 = logits.topk(2, -1).values
    return dict(ids=ids, logits=logits, margins=top2[..., 0] - top2[..., 1])


@functools.lru_cache(maxsize=None)
def oracle(case: str) -> dict:
    _, sd = build(case)
    tok, lengths, n = sources(case)
    return run_oracle(sd, tok, lengths, n)


def oracle_lengths(ids: torch.Tensor, eos_id: int) -> torch.Tensor:
    """per row: positions up to and including the first eos among the generated ones (1 ..), or all of them"""
    out = []
    for row in ids:
        hit = (row[1:] == eos_id).nonzero()
        out.append(int(hit[0]) + 2 if len(hit) else len(row))
    return torch.tensor(out)
