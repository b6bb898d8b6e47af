"""Prompt prefill on MI355X (generate.GreedyDecoder(prefill=True)): time to the FIRST new token with the prompt consumed one decode
step per token (prefill=False: P graph replays) against the batched prompt pass (prefill=True: the pass + one replay), the
per-layer split of the pass, and pm_prefill_attention_bf16 alone against pm_attention_bf16(causal) at p0 = 0 on the same rows
(the same work except for the cache writes).  Synthetic weights.  Writes profiles/prefill/.  Not a BASELINE metric - a
measurement to go with tests/test_hip_prefill.py, from which a later change can choose the default.

    python tools/prefill_bench.py [--model gpt2|whisper|all] [--batch 32] [--reps 7] [--chunk 512]
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--chunk", type=int, default=512)
ap.add_argument("--gpt2-prompts", type=int, nargs="+", default=[16, 64, 256, 512, 1000])
ap.add_argument("--whisper-prompts", type=int, nargs="+", default=[4, 64, 224])
args = ap.parse_args()
out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "prefill")))

import torch  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.audio2text.generate import GreedyDecoder  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

assert torch.cuda.is_available(), "prefill_bench measures on a HIP device"
torch.set_grad_enabled(False)
B = args.batch


def first_token_ms(st, reps):
    """wall time of a whole run of n_new = 1 (reset, prompt, first new token), synchronised at both ends: median / min / max"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run(True)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def layer_split_us(st, reps):
    """per layer, the device time of its part of the prompt pass (events around each layer of each chunk), median over reps"""
    per = []
    for _ in range(reps):
        st.reset()
        log = []
        st.prefill(log)
        torch.cuda.synchronize()
        acc = {}
        for l, e0, e1 in log:
            acc[l] = acc.get(l, 0.0) + e0.elapsed_time(e1) * 1e3
        per.append(acc)
    return [statistics.median(p[l] for p in per) for l in sorted(per[0])]


def kernel_alone(H, C):
    """pm_prefill_attention_bf16 at p0 = 0 against pm_attention_bf16(causal) on the same (B * C, 3 * H * 64) rows, alternating"""
    inner = H * 64
    qkv = synth_input("prefill_bench_qkv", (B * C, 3 * inner), 7).to(torch.bfloat16).cuda()
    kc = torch.empty(B, H, C, 64, dtype=torch.bfloat16, device="cuda")
    vc = torch.empty_like(kc)
    out = torch.empty(B * C, inner, dtype=torch.bfloat16, device="cuda")
    q3 = qkv.view(B, C, 3 * inner)
    q, k, v = q3[..., :inner], q3[..., inner : 2 * inner], q3[..., 2 * inner :]
    new = lambda: ops.prefill_attention(qkv, kc, vc, H, 0, out=out)  # noqa: E731
    old = lambda: ops.attention(q, k, v, H, causal=True, out=out.view(B, C, inner))  # noqa: E731
    t_new, t_old = [], []
    for _ in range(3):
        t_new.append(time_us(new))
        t_old.append(time_us(old))
    a, b = statistics.median(t_new), statistics.median(t_old)
    return dict(C=C, prefill_attention_us=a, attention_causal_us=b, ratio=a / b, prefill_attention_us_all=t_new, attention_causal_us_all=t_old)


def bench(name, dec, memory_of, vocab, prompts, n_layers, H):
    rows = []
    for P in prompts:
        prompt = synth_tokens(f"prefill_bench_{name}", (B, P), vocab, 11).cuda()
        memory = memory_of()
        plain = GreedyDecoder(dec, memory, prompt, 1)
        pre = GreedyDecoder(dec, memory, prompt, 1, prefill=True, prefill_chunk=args.chunk)
        plain.run(True)  # warm-up + capture
        pre.run(True)
        assert (pre.n_steps, plain.n_steps) == (1, P)
        t_plain, t_pre = [], []
        for _ in range(2):  # alternating rounds on one box
            t_plain.append(first_token_ms(plain, args.reps))
            t_pre.append(first_token_ms(pre, args.reps))
        a = statistics.median(x["median"] for x in t_plain)
        b = statistics.median(x["median"] for x in t_pre)
        row = dict(P=P, chunks=pre._pre_chunks, first_token_ms_prefill_false=t_plain, first_token_ms_prefill_true=t_pre, speedup=a / b,
                   same_first_token=bool(torch.equal(plain.tokens, pre.tokens)))
        if pre._pre_chunks:
            split = layer_split_us(pre, args.reps)
            row.update(prefill_pass_us_per_layer=split, prefill_pass_us=sum(split),
                       attention_alone=kernel_alone(H, min(args.chunk, P - 1)))
        print(json.dumps({k: row[k] for k in row if k not in ("first_token_ms_prefill_false", "first_token_ms_prefill_true")}
                         | dict(ms_prefill_false=a, ms_prefill_true=b)), flush=True)
        rows.append(row)
        del plain, pre
    wins = [r["P"] for r in rows if r["speedup"] > 1.0]
    res = dict(model=name, batch=B, layers=n_layers, heads=H, chunk=args.chunk, reps=args.reps, device=torch.cuda.get_device_name(0),
               prompts=rows, smallest_P_where_prefill_wins=min(wins) if wins else None,
               note="first_token_ms: host clock around GreedyDecoder.run(graph=True) with n_new = 1, synchronised at both ends; "
                    "prefill_pass_us_per_layer: device events around each layer of the pass (the last layer stops after its attention)")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}_b{B}.json")
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path)


if args.model in ("gpt2", "all"):
    from pytorch_models.text import GPT2

    m = GPT2.from_hf("gpt2").eval()
    fill_module(m, 78)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    bench("gpt2_small", m, lambda: None, 50257, args.gpt2_prompts, len(m.layers), m.layers[0].sa.n_heads)
    del m

if args.model in ("whisper", "all"):
    from pytorch_models.audio2text import Whisper

    w = Whisper.from_openai("base").eval()
    fill_module(w, 56)
    bf16_round_(w)
    w = w.to(torch.bfloat16).cuda()
    mem = w.encoder(synth_input("prefill_bench_mel", (B, 80, 3000), 56).cuda())
    bench("whisper_base", w.decoder, lambda: mem, 51865, args.whisper_prompts, len(w.decoder.layers), w.decoder.layers[0].sa.n_heads)
