"""End-to-end bf16 tolerance of the alignment matrix m of Whisper.align, derived on the CPU (no GPU, no kernel): the fp32 oracle
re-run with bf16 rounding at every storage point of the HIP path (the oracle's rp hooks: stem, residual stream, LayerNorm outputs,
q / k / v projections, attention outputs, MLP hidden, memory) against the unrounded oracle on the same bf16-valued weights; the
alignment reference of tests/align_cases.py (float64) runs on each pass's cross-attention q / k.  rel-L2 of m per seed at the two
geometries of tests/test_hip_align.py; the test allows 2 x the worst figure (accumulation order, which the emulation does not
model).  DESIGN.md section 21 quotes the output.  Also prints how many start indices the rounding moves (bf16 can move a path).

    python tools/align_tolerance.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import align_cases as ac  # noqa: E402
from oracle import ref_whisper  # noqa: E402
from pytorch_models.audio2text.align import default_heads  # noqa: E402

torch.set_grad_enabled(False)
SEEDS = (58, 59, 60, 61, 62, 63)

if __name__ == "__main__":
    for name, n_layers, d, T in ac.MODEL_CASES:
        worst = 0.0
        for seed in SEEDS:
            w, sd, mel, tokens, lens, frs = ac.model_inputs(name, seed)
            heads = default_heads(n_layers, d // 64)
            plain = ac.oracle_matrix(sd, tokens, ref_whisper.encoder(sd, "encoder.", mel), heads, lens, frs)
            mem_r = ref_whisper.encoder(sd, "encoder.", mel, rp=ac.round_bf16)
            rounded = ac.oracle_matrix(sd, tokens, mem_r, heads, lens, frs, rp=ac.round_bf16)
            e = ac.rel_l2(rounded, plain)
            s0 = ac.dtw_start(plain.float(), lens, frs, 1, 1)
            s1 = ac.dtw_start(rounded.float(), lens, frs, 1, 1)
            worst = max(worst, e)
            print(f"{name} seed {seed}: rel-L2 of m {e:.4e}  (|m| rms {float(plain.square().mean().sqrt()):.3f}); start moved in "
                  f"{int((s0 != s1).sum())} of {int((s0 >= 0).sum())} aligned rows")
        print(f"{name}: worst rel-L2 {worst:.4e} -> test bound 2 x = {2 * worst:.4e}")
