"""Whisper beam search on MI355X (generate.BeamDecoder): us per decode step of `clips` x `beams` rows against the GREEDY step at the
same number of rows (the beams=1 launch list, same box, same run), the share of the step the three beam kernels take, and the
bytes the K / V re-gather moves.  Synthetic weights, no eos: every run is `--new` steps.  Writes profiles/whisper_beam/.
Not a BASELINE metric - a measurement to go with tests/test_hip_beam.py.

    python tools/whisper_beam_bench.py [--tag base] [--clips 8] [--beams 5] [--new 224] [--reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/whisper_beam_bench.py --profile-run --reps 2
    python tools/whisper_beam_bench.py --stats <dir>        # kernel shares + re-gather bytes/s into the JSON of the first command
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="base")
ap.add_argument("--clips", type=int, default=8)
ap.add_argument("--beams", type=int, default=5)
ap.add_argument("--new", type=int, default=224)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--profile-run", action="store_true", help="only `reps` eager beam runs: the body of a rocprofv3 --kernel-trace run")
ap.add_argument("--stats", default=None, help="directory of that rocprofv3 run: adds kernel shares to the JSON of a plain run")
args = ap.parse_args()
B, W, N = args.clips, args.beams, args.new
out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "whisper_beam")))
path = os.path.join(out_dir, f"{args.tag}_b{B}_w{W}_n{N}.json")
BEAM_KERNELS = ("dec_beam_topw_kernel", "dec_beam_select_kernel", "dec_beam_reorder_kernel")

if args.stats:  # ---- post-processing only: no GPU
    files = glob.glob(os.path.join(args.stats, "**", "*kernel_stats.csv"), recursive=True)
    assert len(files) == 1, files
    res = json.load(open(path))
    calls = res["profile_run_steps"]  # launches of every step kernel in the traced run
    rows = [r for r in csv.DictReader(open(files[0])) if int(r["Calls"]) % calls == 0 and "dec_" in r["Name"]]
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    shares = {}
    for k in BEAM_KERNELS:
        ns = sum(int(r["TotalDurationNs"]) for r in rows if k in r["Name"])
        shares[k] = dict(us_per_step=ns / calls / 1e3, share_of_step_kernel_time=ns / total)
    short = lambda n: (re.search(r"dec_\w+?_kernel(<[^>]*>|I[A-Za-z0-9]*E)?", n) or re.search(r"dec_\w+", n)).group(0)  # noqa: E731
    res["rocprofv3"] = dict(step_kernels={short(r["Name"]): dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3) for r in rows},
                            step_kernel_us=total / calls / 1e3, beam_kernels=shares,
                            note="eager launches under rocprofv3 --kernel-trace --stats; shares are of the summed kernel time of a step, not of its wall time")
    reorder_s = shares["dec_beam_reorder_kernel"]["us_per_step"] * 1e-6 * res["steps"]
    res["reorder"]["achieved_bytes_per_s"] = res["reorder"]["bytes_per_run"] / reorder_s
    res["reorder"]["note"] = "bytes read + written by the clips that moved, over the kernel's summed time in the traced run (idle clips and launch included)"
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(beam_kernels=shares, reorder=res["reorder"])))
    sys.exit(0)

import torch  # noqa: E402

from pytorch_models.audio2text import Whisper  # noqa: E402
from pytorch_models.audio2text.generate import BeamDecoder, GreedyDecoder  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

torch.set_grad_enabled(False)
w = Whisper.from_openai(args.tag).eval()
fill_module(w, 56)
bf16_round_(w)
w = w.to(torch.bfloat16).cuda()
mel = synth_input("beam_bench_mel", (B, 80, 3000), 56).cuda()
prompt = synth_tokens("beam_bench_prompt", (B, 4), 51865, 56).cuda()
memory = w.encoder(mel)
beam = BeamDecoder(w.decoder, memory, prompt, N, W)
steps = beam.n_steps

if args.profile_run:
    for _ in range(args.reps):
        beam.run(graph=False)
    torch.cuda.synchronize()
    print(json.dumps(dict(profile_run_steps=steps * args.reps)))
    if os.path.exists(path):
        res = json.load(open(path))
        res["profile_run_steps"] = steps * args.reps
        json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    sys.exit(0)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(median=statistics.median(out) / steps * 1e6, min=min(out) / steps * 1e6, max=max(out) / steps * 1e6)


# the greedy step at the same rows: the beams=1 construction (arg-max tiles + pm_dec_next_token), each clip's memory W times
greedy = GreedyDecoder(w.decoder, memory.repeat_interleave(W, 0), prompt.repeat_interleave(W, 0), N)
beam.run(True)
greedy.run(True)
t_beam, t_greedy = [], []
for _ in range(3):  # alternating rounds on one box
    t_beam.append(timed(lambda: beam.run(True), args.reps))
    t_greedy.append(timed(lambda: greedy.run(True), args.reps))
# what the re-gather moves: parents of every step of one run (eager, read back at the end)
beam.reset()
pars = []
for _ in range(steps):
    beam.step()
    pars.append(beam.parents.clone())
pars = torch.stack(pars).cpu()
H, L = w.decoder.layers[0].sa.n_heads, len(w.decoder.layers)
ident = torch.arange(W)
moved_bytes, moved_steps = 0, 0
for t in range(steps):
    for b in range(B):
        if not torch.equal(pars[t, b], ident):
            rows_w = int((pars[t, b] != ident).sum())
            moved_bytes += (W + rows_w) * H * (t + 1) * 64 * 2 * 2 * L  # W rows read, the moved rows written; K and V of L layers
            moved_steps += 1
res = dict(tag=args.tag, clips=B, beams=W, rows=B * W, new=N, steps=steps, reps=args.reps, device=torch.cuda.get_device_name(0),
           launches_per_step=dict(beam=len(beam.launches), greedy=len(greedy.launches)),
           step_us_beam_replayed=t_beam, step_us_greedy_same_rows_replayed=t_greedy,
           beam_over_greedy=statistics.median(x["median"] for x in t_beam) / statistics.median(x["median"] for x in t_greedy),
           reorder=dict(bytes_per_run=moved_bytes, clip_steps_moved=moved_steps, clip_steps=B * steps,
                        bytes_last_step_if_all_move=2 * B * W * H * (steps) * 64 * 2 * 2 * L),
           best_scores=beam.scores[:, 0].tolist())
print(json.dumps({k: res[k] for k in ("rows", "step_us_beam_replayed", "step_us_greedy_same_rows_replayed", "beam_over_greedy", "reorder")}), flush=True)
os.makedirs(out_dir, exist_ok=True)
json.dump(res, open(path, "w"), indent=1, sort_keys=True)
print("wrote", path)
