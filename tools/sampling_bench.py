"""The sampling tail on MI355X: what temperature / top-p / the whole vocabulary / log-probs cost per decode step, synthetic weights.
Not a BASELINE metric - the measurement behind profiles/sampling/README.md.
    python tools/sampling_bench.py [--out profiles/sampling]
Geometries: GPT-2 small (12 x 768, V 50257) and Whisper-base's decoder (6 x 512, V 51865, memory 1500), batch 32, prompt 4, 60 new
tokens.  In ONE process, for each of
    arg-max            the default tail (pm_dec_linear mode 2 + pm_dec_next_token), as it always was built
    topk 50            the default top-k tail (full logits + pm_dec_sample_topk), as it always was built
    the new tail       full logits + pm_dec_sample at (topk 50, p 0.9, T 0.7), (topk 0, p 1, T 1), (topk 0, p 0.9, T 0.7), (T 0),
                       each with and without the log-prob buffer
  (a) us per step: the median over `--repeats` graph-replayed runs (HIP events around a whole run / its steps);
  (b) the tail kernel ALONE: the run's last launch, 20 times back to back in one HIP graph that first resets the position, 10
      replays after one: us per launch, the kernel boundary included (tools/ctc_bench.py's method).  The logits are those the run
      left behind; with synthetic weights they are nearly flat (standard deviation ~1), the LONG case for the nucleus: the
      threshold search always runs its 8 passes whatever the values.
The share of the step the whole-vocabulary nucleus costs = ((topk 0, p 0.9, T 0.7) - (topk 0, p 1, T 1)) / the former."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="directory for gpt2_small.json / whisper_base.json / sampling.txt")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--new", type=int, default=60)
args = ap.parse_args()

import torch  # noqa: E402

from pytorch_models.audio2text.generate import GreedyDecoder  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

torch.set_grad_enabled(False)
LINES = []
CONFIGS = [("arg-max (default tail)", dict()), ("topk 50 (default tail)", dict(topk=50, seed=1))]
for name, kw in (("topk 50, p 0.9, T 0.7", dict(topk=50, top_p=0.9, temperature=0.7)), ("topk 0, p 1, T 1", dict(topk=0)),
                 ("topk 0, p 0.9, T 0.7", dict(topk=0, top_p=0.9, temperature=0.7)), ("T 0 (arg-max, new tail)", dict(temperature=0.0))):
    for lp in (False, True):
        CONFIGS.append((name + (", log-probs" if lp else ""), dict(kw, seed=1, return_logprobs=lp)))


def say(s):
    print(s, flush=True)
    LINES.append(s)


def step_us(st) -> float:
    st.run()  # warm-up, capture
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 1e3 * statistics.median(ms) / st.n_steps


def kernel_us(st, n=20, replays=10) -> float:
    fn, a = st.launches[-1]
    assert n < st.Ttot
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st.reset()
        fn(*a[:-1], stream.cuda_stream)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=stream):
            st.pos.zero_()  # every launch moves the position: each replay starts over, inside the positional table
            for _ in range(n):
                rc = fn(*a[:-1], torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * n)


def bench(name, dec, memory, prompt):
    say(f"== {name}: batch {prompt.shape[0]}, prompt {prompt.shape[1]}, {args.new} new tokens")
    res = {}
    for label, kw in CONFIGS:
        st = GreedyDecoder(dec, memory, prompt, args.new, **kw)
        step = step_us(st)
        kern = kernel_us(st)
        res[label] = dict(step_us=round(step, 1), tail_kernel_us=round(kern, 2), tail=st.launches[-1][0].__name__)
        say(f"  {label:38s} {step:8.1f} us / step    tail {st.launches[-1][0].__name__:20s} alone {kern:7.2f} us")
        del st
    full, cut = res["topk 0, p 1, T 1"]["step_us"], res["topk 0, p 0.9, T 0.7"]["step_us"]
    res["nucleus_share_of_step"] = round((cut - full) / cut, 4)
    res["new_tail_over_argmax"] = round(full / res["arg-max (default tail)"]["step_us"], 4)
    say(f"  the whole-vocabulary nucleus costs {100 * (cut - full) / cut:.1f} % of its step; the whole-vocabulary draw runs at "
        f"{full / res['arg-max (default tail)']['step_us']:.3f} x the arg-max step")
    return res


def main():
    from pytorch_models.audio2text import Whisper
    from pytorch_models.text import GPT2

    B = args.batch
    m = GPT2.from_hf("gpt2").eval()
    fill_module(m, 1)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    out = {"gpt2_small": bench("GPT-2 small", m, None, synth_tokens("sampling_bench", (B, 4), 50257, 2).cuda())}
    del m
    w = Whisper.from_openai("base").eval()
    fill_module(w, 56)
    bf16_round_(w)
    w = w.to(torch.bfloat16).cuda()
    memory = synth_input("sampling_bench_memory", (B, 1500, 512), 56).to(torch.bfloat16).cuda()
    out["whisper_base"] = bench("Whisper-base decoder", w.decoder, memory, synth_tokens("sampling_bench_w", (B, 4), 51865, 3).cuda())
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k, v in out.items():
            with open(os.path.join(args.out, k + ".json"), "w") as f:
                json.dump(v, f, indent=1)
        with open(os.path.join(args.out, "sampling.txt"), "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
