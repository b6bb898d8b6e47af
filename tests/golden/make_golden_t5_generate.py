"""Generate the T5 generation fixture by IMPORTING THE REFERENCE on CPU (build container only; never runs on the GPU box):

    python tests/golden/make_golden_t5_generate.py

* t5_generate.npz   the reference's T5Model (fp32, synthweights, seed and sources of tests/t5_generate_cases.py case "h8_l4")
      under the reference's own loop on ids (T5Generator.generate, text/t5.py:219-225: encode once, decode the whole prefix,
      arg-max of the last position), 32 decisions per row of a batch of 8 sources cut to mixed lengths, never stopping:
      ``ids`` (8, 33) int16, ``margins`` (8, 32) top-1 minus top-2 logit of every decision, ``logits_s16`` (8, 33, 125) every
      16th logit of the teacher-forced decode of the final ids.
Conventions (save) as make_golden.py; only data is written."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")  # the reference's ``pytorch_models`` wins
sys.path.insert(1, os.path.join(ROOT, "pytorch-models_amd"))  # only for ``synthweights``
sys.path.insert(2, os.path.join(ROOT, "tests"))
sys.path.insert(3, ROOT)

import pytorch_models  # noqa: E402

assert pytorch_models.__file__.startswith("/root/reference"), pytorch_models.__file__
from pytorch_models.text import T5Model  # noqa: E402
from synthweights import fill_module  # noqa: E402

import t5_generate_cases as TC  # noqa: E402
from make_golden import save  # noqa: E402

torch.set_grad_enabled(False)
CASE = "h8_l4"


def main():
    geom, seed = TC.CASES[CASE][:2]
    m = T5Model(*geom).eval()
    fill_module(m, seed)
    tok, lengths, n = TC.sources(CASE)
    ids, margins, logits = [], [], []
    for b, ln in enumerate(lengths):
        memory = m.encode(tok[b, :ln])
        out, marg = [0], []
        while len(out) < n + 1:
            lg = m.decode(torch.tensor(out), memory)[-1]
            top2 = lg.topk(2).values
            marg.append(float(top2[0] - top2[1]))
            out.append(int(lg.argmax()))
        ids.append(out)
        margins.append(marg)
        logits.append(m.decode(torch.tensor(out), memory)[:, ::16])
    save("t5_generate", dict(case=CASE, geometry=list(geom), seed=seed, lengths=lengths, decisions=n),
         ids=torch.tensor(ids, dtype=torch.int16), margins=torch.tensor(margins), logits_s16=torch.stack(logits))


if __name__ == "__main__":
    main()
