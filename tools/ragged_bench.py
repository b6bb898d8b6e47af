"""Ragged prompt batches on MI355X (generate.GreedyDecoder(lengths=...)): wall time of decoding a batch of prompts of different
lengths (a) in ONE ragged run, against (b) one rectangular run of the same rows all padded to the longest length (what the padding
would cost if it were real tokens) and (c) what the parent commit offered for such a batch: one rectangular call per distinct length,
summed.  All three through prefill=True and graph replay, the rectangular ones through lengths=None.  Beside them the ragged prompt
attention kernel alone against the plain one (p0 = 0, C = 512) and Whisper-base against its default (chain) step: the price of
leaving the chain.  Synthetic weights.  Writes profiles/ragged/.  Not a BASELINE metric - a measurement to go with
tests/test_hip_ragged.py.

    python tools/ragged_bench.py [--model gpt2|whisper|all] [--batch 32] [--new 64] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="all", choices=("gpt2", "whisper", "all"))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=19)
args = ap.parse_args()
out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "ragged")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.audio2text.generate import GreedyDecoder  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

assert torch.cuda.is_available(), "ragged_bench measures on a HIP device"
torch.set_grad_enabled(False)
B, N = args.batch, args.new


def run_ms(decoders, reps):
    """wall time of one run() of every decoder in turn (reset, prompt pass, N graph replays), synchronised at both ends"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for st in decoders:
            st.run(True)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def compare(dec, memory, prompt, lens, name):
    """(a) ragged, (b) rectangular at the longest length, (c) one rectangular decoder per distinct length - alternating rounds"""
    P = prompt.shape[1]
    ragged = [GreedyDecoder(dec, memory, prompt, N, prefill=True, lengths=lens)]
    rect = [GreedyDecoder(dec, memory, prompt, N, prefill=True)]
    per_len = []
    for n in sorted(set(lens)):
        rows = [b for b, x in enumerate(lens) if x == n]
        per_len.append(GreedyDecoder(dec, None if memory is None else memory[rows].contiguous(), prompt[rows, :n].contiguous(), N, prefill=True))
    forms = dict(ragged=ragged, rectangular=rect, per_length=per_len)
    for sts in forms.values():  # warm-up + capture
        for st in sts:
            st.run(True)
    times = {k: [] for k in forms}
    for _ in range(2):  # alternating rounds on one box
        for k, sts in forms.items():
            times[k].append(run_ms(sts, args.reps))
    med = {k: statistics.median(x["median"] for x in v) for k, v in times.items()}
    new_tokens = B * N
    res = dict(model=name, batch=B, n_new=N, padded_width=P, lengths=list(lens), distinct_lengths=len(per_len),
               self_block=dict(ragged="unfused", rectangular="chain" if rect[0]._chain else "fused" if rect[0]._fuse_self else "unfused"),
               run_ms=times, run_ms_median=med, ragged_over_rectangular=med["ragged"] / med["rectangular"],
               per_length_over_ragged=med["per_length"] / med["ragged"],
               new_tokens_per_s={k: new_tokens / (v * 1e-3) for k, v in med.items()}, device=torch.cuda.get_device_name(0),
               note="host clock around GreedyDecoder.run(graph=True) (reset, prompt pass, n_new replays), synchronised at both ends; "
                    "per_length = the sum over one rectangular decoder per distinct length (built and captured beforehand)")
    print(json.dumps({k: res[k] for k in ("model", "run_ms_median", "ragged_over_rectangular", "per_length_over_ragged")}), flush=True)
    return res


def kernel_alone(H, C, starts):
    """pm_prefill_attention_ragged_bf16 against pm_prefill_attention_bf16 at p0 = 0 on the same rows, alternating"""
    inner = H * 64
    qkv = synth_input("ragged_bench_qkv", (B * C, 3 * inner), 7).to(torch.bfloat16).cuda()
    kc = torch.empty(B, H, C, 64, dtype=torch.bfloat16, device="cuda")
    vc = torch.empty_like(kc)
    out = torch.empty(B * C, inner, dtype=torch.bfloat16, device="cuda")
    ks = torch.tensor(starts, dtype=torch.int32).clamp(max=C).cuda()
    zero = torch.zeros_like(ks)
    forms = dict(plain=lambda: ops.prefill_attention(qkv, kc, vc, H, 0, out=out),
                 ragged_zero_starts=lambda: ops.prefill_attention_ragged(qkv, kc, vc, H, 0, zero, out=out),
                 ragged=lambda: ops.prefill_attention_ragged(qkv, kc, vc, H, 0, ks, out=out))
    t = {k: [] for k in forms}
    for _ in range(3):
        for k, fn in forms.items():
            t[k].append(time_us(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(C=C, us=med, us_all=t, ragged_over_plain=med["ragged"] / med["plain"], zero_starts_over_plain=med["ragged_zero_starts"] / med["plain"],
                masked_key_share=float(sum(min(s, C) * (2 * C - min(s, C)) for s in starts)) / (len(starts) * C * C))


rng = np.random.Generator(np.random.PCG64(args.seed))
os.makedirs(out_dir, exist_ok=True)
if args.model in ("gpt2", "all"):
    from pytorch_models.text import GPT2

    m = GPT2.from_hf("gpt2").eval()
    fill_module(m, 72)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    lens = [int(x) for x in rng.integers(16, 513, size=B)]
    P = 512
    prompt = synth_tokens("ragged_bench_gpt2", (B, P), 50257, 11).cuda()
    res = compare(m, None, prompt, lens, "gpt2")
    res["prefill_attention_alone"] = kernel_alone(12, P, [max(lens) - n for n in lens])
    print(json.dumps(dict(prefill_attention_alone=res["prefill_attention_alone"]["us"])), flush=True)
    path = os.path.join(out_dir, f"gpt2_b{B}.json")
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path)
    del m
if args.model in ("whisper", "all"):
    from pytorch_models.audio2text import Whisper

    w = Whisper.from_openai("base").eval()
    fill_module(w, 56)
    bf16_round_(w)
    w = w.to(torch.bfloat16).cuda()
    memory = synth_input("ragged_bench_memory", (B, 1500, 512), 56).to(torch.bfloat16).cuda()
    lens = [int(x) for x in rng.integers(4, 65, size=B)]
    prompt = synth_tokens("ragged_bench_whisper", (B, 64), 51865, 11).cuda()
    res = compare(w.decoder, memory, prompt, lens, "whisper-base")
    path = os.path.join(out_dir, f"whisper_base_b{B}.json")
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path)
