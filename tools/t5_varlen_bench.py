"""Ragged source batches through T5's encoder on MI355X (T5Model.encode(x, lengths) / generate(..., packed=True)): the time of
one batch of 32 sources padded to 512
(a) packed: the valid rows only, the relative-position bias read by distance inside pm_attention_varlen_relbias_bf16,
(b) dense: the code T5DecodeState.encode runs for a lengths batch (t5_generate.encode_dense) - the padded rectangle with an
    fp32 (B, H, S, S) table (the relative bias plus -inf on padded key columns) built per call and read by every layer through
    pm_attention_bias_bf16,
(c) per_length: one rectangular encode per distinct length, summed.
Beside them the attention kernel alone: the new entry point on packed operands against pm_attention_bias_bf16 on the padded
operands with the (B, H, S, S) table.  The work ratios and the bias bytes printed next to the times are arithmetic on the shapes
(rows: sum(len) / (B S); attention: sum(len^2) / (B S^2); bias: bytes of the table one layer's attention is handed), not
measurements.  Lengths: the draw of tools/varlen_bench.py's BERT leg (8 + Gamma(2, 60) clipped to S, the same seed) at this
batch.  Device events around `reps` calls, every form warmed up, forms alternated over `rounds` rounds in one process, all rounds
reported.  Seeded, synthetic weights.  Writes profiles/t5_varlen/.  Not a BASELINE metric.

    python tools/t5_varlen_bench.py [--size small|base|all] [--reps 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="all", choices=("small", "base", "all"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seed", type=int, default=23)
args = ap.parse_args()
out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "t5_varlen")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.text import T5Model  # noqa: E402
from pytorch_models.text.t5_generate import encode_dense  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

assert torch.cuda.is_available(), "t5_varlen_bench measures on a HIP device"
torch.set_grad_enabled(False)
B, S = 32, 512


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
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v), all=v) for k, v in times.items()}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def leg(size):
    rng = np.random.Generator(np.random.PCG64(args.seed))
    lens = [int(min(S, 8 + rng.gamma(2.0, 60.0))) for _ in range(B)]
    m = T5Model.from_t5x(f"t5_1_1-{size}").eval()
    fill_module(m, 94)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    enc = m.encoder
    H, R, n_layers = enc.layers[0].sa.n_heads, enc.attn_bias.max_distance, len(enc.layers)
    inner = H * 64
    x = synth_tokens("t5_varlen_bench_tok", (B, S), 32128, 11).cuda()
    len_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    distinct = sorted(set(lens))
    groups = [(n, [b for b, v in enumerate(lens) if v == n]) for n in distinct]
    xs = [x[rows, :n].contiguous() for n, rows in groups]
    forms = dict(packed=lambda: m.encode(x, lens), dense=lambda: encode_dense(m, x, len_t)[0],
                 per_length=lambda: [m.encode(v) for v in xs])
    ratios = dict(sum_len=int(sum(lens)), rows=sum(lens) / (B * S), attention=sum(n * n for n in lens) / (B * S * S))
    bias_bytes = dict(packed=H * (2 * R + 1) * 4, dense=B * H * S * S * 4, per_length=sum(H * n * n * 4 for n in distinct))
    print(json.dumps(dict(size=size, lengths_mean=sum(lens) / B, bias_bytes_per_layer=bias_bytes, **ratios)), flush=True)
    # results first: the packed rows against the per-length calls' rows and against the dense-table form's valid rows
    y, yd = forms["packed"](), forms["dense"]()
    assert encode_dense(m, x, len_t)[1] == bias_bytes["dense"]
    worst = max(rel(y[rows, :n], m.encode(v)) for (n, rows), v in zip(groups, xs))
    worst_dense = max(rel(y[b, :n], yd[b, :n]) for b, n in enumerate(lens))
    assert worst < 2e-2 and worst_dense < 2e-2, (worst, worst_dense)
    times = alternate(forms, args.reps, args.rounds)
    # the attention alone, on one layer's operands
    seq = ops.seq_lens(lens, S, "cuda")
    lut = enc.attn_bias.lut(True)
    qkv_p = synth_input("t5_varlen_bench_qkv", (seq.total, 3 * inner), 7).to(torch.bfloat16).cuda()
    qkv_r = synth_input("t5_varlen_bench_qkv_r", (B, S, 3 * inner), 7).to(torch.bfloat16).cuda()
    dead = torch.arange(S, device="cuda")[None, :] >= len_t[:, None]
    table = (enc.attn_bias(S, True).float()[None]
             + torch.zeros(B, S, device="cuda").masked_fill_(dead, float("-inf"))[:, None, None, :]).contiguous()
    out_p = torch.empty(seq.total, inner, dtype=torch.bfloat16, device="cuda")
    out_r = torch.empty(B, S, inner, dtype=torch.bfloat16, device="cuda")
    att = dict(varlen_relbias=lambda: ops.attention_varlen(qkv_p[:, :inner], qkv_p[:, inner : 2 * inner], qkv_p[:, 2 * inner :], H, seq,
                                                           out=out_p, rel_lut=lut, radius=R),
               dense_table=lambda: ops.attention(qkv_r[..., :inner], qkv_r[..., inner : 2 * inner], qkv_r[..., 2 * inner :], H,
                                                 bias=table, out=out_r))
    att_us = {k: [] for k in att}
    for _ in range(args.rounds):
        for k, fn in att.items():
            att_us[k].append(time_us(fn))
    med = {k: v["median"] for k, v in times.items()}
    att_med = {k: statistics.median(v) for k, v in att_us.items()}
    res = dict(model=f"t5_1_1-{size} encoder ({n_layers} x {enc.norm.dim}, {H} heads)", batch=B, padded_length=S, lengths=lens,
               distinct_lengths=len(distinct), work_ratios_by_construction=ratios, bias_bytes_per_layer_by_construction=bias_bytes,
               encode_ms=times, encode_ms_median=med, dense_over_packed=med["dense"] / med["packed"],
               per_length_over_packed=med["per_length"] / med["packed"], packed_vs_per_length_rel_l2_worst=worst,
               packed_vs_dense_rel_l2_worst=worst_dense,
               attention_alone_us=dict(all=att_us, median=att_med, relbias_over_dense=att_med["varlen_relbias"] / att_med["dense_table"],
                                       grid_workgroups=B * H * ((max(lens) + 127) // 128),
                                       live_workgroups=H * sum((n + 127) // 128 for n in lens)),
               device=torch.cuda.get_device_name(0),
               note="device events around `reps` calls (host gaps included); forms alternated over the rounds in one process; dense = "
                    "t5_generate.encode_dense, T5DecodeState.encode's lengths path (table built per call); per_length = one rectangular encode per distinct length")
    print(json.dumps(dict(size=size, encode_ms_median=med, dense_over_packed=res["dense_over_packed"],
                          per_length_over_packed=res["per_length_over_packed"], attention_alone_us=att_med)), flush=True)
    return f"t5_{size}_b32.json", res


for size in ("small", "base"):
    if args.size in (size, "all"):
        name, res = leg(size)
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, name)
        json.dump(res, open(path, "w"), indent=1, sort_keys=True)
        print("wrote", path, flush=True)
        torch.cuda.empty_cache()
