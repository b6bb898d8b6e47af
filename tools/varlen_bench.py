"""Variable-length encoder batches on MI355X (BERT.forward / Wav2Vec2.forward with lengths=): the time of one ragged batch
(a) packed (lengths=), against (b) the same rows run as the padded rectangle (what a user who pads pays - and gets wrong results
for) and (c) one rectangular call per distinct length, summed (the only correct form before lengths=).  Beside them
pm_attention_varlen_bf16 alone against pm_attention_bf16 on the padded operands.  The work ratios printed next to the times are
arithmetic on the lengths (rows: sum(len) / (B L); attention: sum(len^2) / (B L^2)), not measurements.  Device events around
`reps` calls, every form warmed up, forms alternated over `rounds` rounds in one process, all rounds reported.  Seeded, synthetic
weights.  Writes profiles/varlen/.  Not a BASELINE metric - a measurement to go with tests/test_hip_varlen.py.

    python tools/varlen_bench.py [--leg bert|w2v|all] [--reps 30] [--rounds 3]
    python tools/varlen_bench.py --leg bert --trace      # a few packed and padded forwards and nothing else (for rocprofv3)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]

ap = argparse.ArgumentParser()
ap.add_argument("--leg", default="all", choices=("bert", "w2v", "all"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seed", type=int, default=23)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "varlen")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

assert torch.cuda.is_available(), "varlen_bench measures on a HIP device"
torch.set_grad_enabled(False)


def call_ms(fn, reps):
    """device time of one call: events around `reps` calls in a row (host gaps between launches included: they are part of a call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(forms, reps, rounds):
    for fn in forms.values():  # every shape a timed window uses, twice
        fn()
        fn()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(call_ms(fn, reps))
    return times


def summary(times):
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v), all=v) for k, v in times.items()}


def work_ratios(lens, L):
    B = len(lens)
    return dict(sum_len=int(sum(lens)), rows=sum(lens) / (B * L), attention=sum(n * n for n in lens) / (B * L * L))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def per_length_calls(lens):
    return [(n, [b for b, x in enumerate(lens) if x == n]) for n in sorted(set(lens))]


def bert_leg():
    from pytorch_models.text import BERT

    B, L = 64, 512
    rng = np.random.Generator(np.random.PCG64(args.seed))
    m = BERT(30522, 12, 768).eval()  # BERT-base geometry
    fill_module(m, 74)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    lens = [int(min(L, 8 + rng.gamma(2.0, 60.0))) for _ in range(B)]  # 8 .. 512, mean near 128, drawn once
    x = synth_tokens("varlen_bench_tok", (B, L), 30522, 11).cuda()
    groups = [(n, x[rows, :n].contiguous()) for n, rows in per_length_calls(lens)]
    forms = dict(packed=lambda: m(x, lengths=lens), padded=lambda: m(x), per_length=lambda: [m(xs) for _, xs in groups])
    if args.trace:
        for _ in range(3):
            forms["packed"]()
            forms["padded"]()
        torch.cuda.synchronize()
        return None
    ratios = work_ratios(lens, L)
    print(json.dumps(dict(leg="bert", lengths_mean=sum(lens) / B, **ratios)), flush=True)
    # results first (faster and different is not faster): the packed rows against the per-length calls' rows
    y = m(x, lengths=lens)
    worst = 0.0
    for (n, rows), (_, xs) in zip(per_length_calls(lens), groups):
        worst = max(worst, rel(y[rows, :n], m(xs)))
    assert worst < 2e-2, worst
    times = summary(alternate(forms, args.reps, args.rounds))
    # the attention alone, on one layer's operands
    H, inner = 12, 768
    seq = ops.seq_lens(lens, L, "cuda")
    qkv_p = synth_input("varlen_bench_qkv", (seq.total, 3 * inner), 7).to(torch.bfloat16).cuda()
    qkv_r = synth_input("varlen_bench_qkv_r", (B, L, 3 * inner), 7).to(torch.bfloat16).cuda()
    out_p, out_r = torch.empty(seq.total, inner, dtype=torch.bfloat16, device="cuda"), torch.empty(B, L, inner, dtype=torch.bfloat16, device="cuda")
    att = dict(varlen=lambda: ops.attention_varlen(qkv_p[:, :inner], qkv_p[:, inner : 2 * inner], qkv_p[:, 2 * inner :], H, seq, out=out_p),
               padded=lambda: ops.attention(qkv_r[..., :inner], qkv_r[..., inner : 2 * inner], qkv_r[..., 2 * inner :], H, out=out_r))
    att_us = {k: [] for k in att}
    for _ in range(args.rounds):
        for k, fn in att.items():
            att_us[k].append(time_us(fn))
    med = {k: v["median"] for k, v in times.items()}
    att_med = {k: statistics.median(v) for k, v in att_us.items()}
    grid = B * H * ((max(lens) + 127) // 128)
    live = H * sum((n + 127) // 128 for n in lens)
    res = dict(model="bert-base (12 x 768, vocab 30522)", batch=B, padded_length=L, lengths=lens, distinct_lengths=len(groups),
               work_ratios_by_construction=ratios, forward_ms=times, forward_ms_median=med,
               packed_over_padded=med["packed"] / med["padded"], per_length_over_packed=med["per_length"] / med["packed"],
               packed_vs_per_length_rel_l2_worst=worst,
               attention_alone_us=dict(all=att_us, median=att_med, varlen_over_padded=att_med["varlen"] / att_med["padded"],
                                       varlen_grid_workgroups=grid, varlen_live_workgroups=live),
               device=torch.cuda.get_device_name(0),
               note="device events around `reps` calls (host gaps included); forms alternated over the rounds in one process; "
                    "padded = the rectangle with every position treated as real (its results differ: not a correct alternative); "
                    "per_length = one rectangular call per distinct length, summed")
    print(json.dumps(dict(leg="bert", forward_ms_median=med, packed_over_padded=res["packed_over_padded"],
                          per_length_over_packed=res["per_length_over_packed"], attention_alone_us=att_med)), flush=True)
    return "bert_base_b64.json", res


def w2v_leg():
    from pytorch_models.audio import Wav2Vec2

    B, rate = 32, 16000
    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    m = Wav2Vec2(24, 1024).eval()  # wav2vec2-large geometry, layer-norm stem, pre-norm encoder
    fill_module(m, 82)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    lens = [int(v) for v in rng.integers(rate, 10 * rate + 1, size=B)]  # 1 .. 10 s, drawn once
    L = max(lens)
    x = synth_input("varlen_bench_wave", (B, L), 81, scale=0.1).cuda()
    clips = [x[b : b + 1, :n].contiguous() for b, n in enumerate(lens)]
    forms = dict(packed=lambda: m(x, lengths=lens), padded=lambda: m(x), per_length=lambda: [m(c) for c in clips])
    if args.trace:
        for _ in range(3):
            forms["packed"]()
            forms["padded"]()
        torch.cuda.synchronize()
        return None
    frames = [m.frame_length(n) for n in lens]
    ratios = work_ratios(frames, m.frame_length(L))
    print(json.dumps(dict(leg="w2v", frames_mean=sum(frames) / B, **ratios)), flush=True)
    y = m(x, lengths=lens)
    worst = max(rel(y[b, :f], m(clips[b])[0]) for b, f in enumerate(frames))
    assert worst < 2e-2, worst
    times = summary(alternate(forms, args.reps, args.rounds))
    med = {k: v["median"] for k, v in times.items()}
    res = dict(model="wav2vec2-large (24 x 1024, layer-norm stem)", batch=B, samples=lens, frames=frames, padded_frames=m.frame_length(L),
               encoder_work_ratios_by_construction=ratios, forward_ms=times, forward_ms_median=med,
               packed_over_padded=med["packed"] / med["padded"], per_length_over_packed=med["per_length"] / med["packed"],
               packed_vs_per_clip_rel_l2_worst=worst, device=torch.cuda.get_device_name(0),
               note="the stem and the positional convolution run on the padded rectangle in both batched forms; only the encoder is packed")
    print(json.dumps(dict(leg="w2v", forward_ms_median=med, packed_over_padded=res["packed_over_padded"],
                          per_length_over_packed=res["per_length_over_packed"])), flush=True)
    return "wav2vec2_large_b32.json", res


for leg, fn in (("bert", bert_leg), ("w2v", w2v_leg)):
    if args.leg in (leg, "all"):
        got = fn()
        if got is not None:
            os.makedirs(out_dir, exist_ok=True)
            path = os.path.join(out_dir, got[0])
            json.dump(got[1], open(path, "w"), indent=1, sort_keys=True)
            print("wrote", path, flush=True)
        torch.cuda.empty_cache()
