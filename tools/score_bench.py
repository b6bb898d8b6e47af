"""Sequence scoring on MI355X: the fused vocabulary log-softmax kernel (ops.lm_score, csrc/lm_score.hip) against the materialised
route it replaces, synthetic weights.  Not a BASELINE metric - the measurement behind profiles/score/README.md.
    python tools/score_bench.py [--workload gpt2|whisper|all] [--out profiles/score]
Per workload (GPT-2 small at 32 x 1024, Whisper-base decoder at 32 x 224), in ONE process:
  (a) model.score(...)                                            tokens/s, peak memory above the model
  (b) forward + torch.log_softmax + gather (the only route before) tokens/s, peak memory; if it cannot allocate at that batch the
      batch is halved until it can, and the line says so
  (c) the head alone on the same hidden rows: ops.lm_score against ops.linear(..., f32) + log_softmax + gather: ms, and the fused
      head's fraction of the 2.5 PFLOP/s bf16 peak (2 M V K flop)
Every figure is the median of `--repeats` timed runs after `--warmup` untimed ones (HIP events around each run).  With
--workload all each workload runs as a child process under its own time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]
PEAK_FLOPS = 2.5e15

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="all", choices=("gpt2", "whisper", "all"))
ap.add_argument("--out", default=None, help="directory for <workload>.json")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--limit", type=int, default=240, help="seconds per workload (child processes of --workload all)")
args = ap.parse_args()

if args.workload == "all":
    rc = 0
    for wl in ("gpt2", "whisper"):
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", wl, "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        if args.out:
            cmd += ["--out", args.out]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{wl}: no result within {args.limit} s - stopping", flush=True)
            sys.exit(124)
        if r.returncode != 0:  # a fault or an abort: start nothing more on the device
            print(f"{wl}: exit status {r.returncode} - stopping", flush=True)
            sys.exit(r.returncode)
    sys.exit(rc)

import torch  # noqa: E402

from pytorch_models._hip import ops  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

torch.set_grad_enabled(False)


def timed(fn):
    """(median ms, peak bytes above what was allocated before) of fn over the repeats"""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), torch.cuda.max_memory_allocated() - base


def gather_route(logits, tokens):
    lp = torch.log_softmax(logits[:, :-1], -1)
    return lp.gather(-1, tokens[:, 1:, None])[..., 0]


if args.workload == "gpt2":
    from pytorch_models.text import GPT2

    B, L, V = 32, 1024, 50257
    m = GPT2.from_hf("gpt2")
    fill_module(m, 1)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda().eval()
    tokens = synth_tokens("score_bench", (B, L), V, 2).cuda()
    score = lambda t: m.score(t)  # noqa: E731
    forward = lambda t: m(t)  # noqa: E731
    hidden = lambda t: m.hidden_rows(t)  # noqa: E731
    name = f"GPT-2 small, {B} x {L}, V = {V}"
else:
    from pytorch_models.audio2text import Whisper

    B, L, V = 32, 224, 51865
    m = Whisper.from_openai("base")
    fill_module(m, 1)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda().eval()
    tokens = synth_tokens("score_bench", (B, L), V, 2).cuda()
    memory = m.encoder(synth_input("score_bench_mel", (B, 80, 3000), 2).cuda())
    score = lambda t: m.decoder.score(t, memory[: t.shape[0]])  # noqa: E731
    forward = lambda t: m.decoder(t, memory[: t.shape[0]])  # noqa: E731
    hidden = lambda t: m.decoder.hidden_rows(t, memory[: t.shape[0]])  # noqa: E731
    name = f"Whisper-base decoder, {B} x {L}, V = {V}"

res = {"workload": name, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats}
ms, peak = timed(lambda: score(tokens))
res["score"] = {"ms": ms, "tokens_per_s": B * L / ms * 1e3, "peak_bytes": peak}
print(f"(a) score                         {ms:9.2f} ms  {B * L / ms:9.1f} k tokens/s  peak {peak / 1e6:9.1f} MB", flush=True)

bb = B
while True:
    try:
        tb = tokens[:bb]
        ms, peak = timed(lambda: gather_route(forward(tb), tb))
        break
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        if bb == 1:
            raise
        bb //= 2
res["forward_log_softmax_gather"] = {"batch": bb, "ms": ms, "tokens_per_s": bb * L / ms * 1e3, "peak_bytes": peak,
                                     "fits_at_full_batch": bb == B}
print(f"(b) forward + log_softmax + gather{ms:9.2f} ms  {bb * L / ms:9.1f} k tokens/s  peak {peak / 1e6:9.1f} MB"
      + ("" if bb == B else f"  (batch {bb}: batch {B} cannot allocate)"), flush=True)

h, W = hidden(tokens)
rows = h[:, :-1].reshape(B * (L - 1), -1)
tgt = tokens[:, 1:].reshape(-1).contiguous()
M, K = rows.shape
ops.LM_SCORE_CHECK_IDS = False  # the head alone: no read-back inside the timed region
ms_f, peak_f = timed(lambda: ops.lm_score(rows, W, tgt))
flop = 2.0 * M * V * K
res["head_fused"] = {"M": M, "K": K, "ms": ms_f, "peak_bytes": peak_f, "fraction_of_bf16_peak": flop / (ms_f * 1e-3) / PEAK_FLOPS,
                     "ws_bytes": ops.lm_score_ws_bytes(M, V)}
print(f"(c) head, fused ops.lm_score      {ms_f:9.2f} ms  {flop / ms_f / 1e9:7.1f} TFLOP/s = {100 * flop / (ms_f * 1e-3) / PEAK_FLOPS:.1f} % of "
      f"the bf16 peak  peak {peak_f / 1e6:9.1f} MB", flush=True)
ms_g, peak_g = timed(lambda: ops.linear(rows, W, None, out_dtype=torch.float32))
res["head_gemm_only"] = {"ms": ms_g, "peak_bytes": peak_g}
print(f"(c) head, ops.linear (f32) alone  {ms_g:9.2f} ms  {flop / ms_g / 1e9:7.1f} TFLOP/s", flush=True)
ms_m, peak_m = timed(lambda: torch.log_softmax(ops.linear(rows, W, None, out_dtype=torch.float32), -1).gather(-1, tgt[:, None]))
res["head_materialised"] = {"ms": ms_m, "peak_bytes": peak_m}
print(f"(c) head, linear + log_softmax + gather {ms_m:9.2f} ms  peak {peak_m / 1e6:9.1f} MB", flush=True)
a = ops.lm_score(rows, W, tgt)
b = torch.log_softmax(ops.linear(rows, W, None, out_dtype=torch.float32), -1).gather(-1, tgt[:, None])[:, 0]
res["max_abs_difference_of_the_two_heads"] = float((a - b).abs().max())
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.workload + ".json"), "w") as f:
        json.dump(res, f, indent=1)
