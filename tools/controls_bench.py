"""Eos stopping and the repetition controls on MI355X: what they cost per decode step and what the early exit saves, synthetic
weights.  Not a BASELINE metric - the measurement behind profiles/controls/README.md and DESIGN.md section 31.
    python tools/controls_bench.py [--out profiles/controls]
Geometries: GPT-2 small (12 x 768, V 50257, 1024 positions) and Whisper-base's decoder (6 x 512, V 51865, memory 1500, 448 positions),
batch 32, prompt 4, decoded to the last position.  In ONE process:
  (a) us per graph-replayed step (HIP events around 32 consecutive replays, median over --repeats runs) at histories near 64 and near
      max_seq_len, for the default tail, eos only (pm_dec_finish behind it), each control alone (which takes the full-logits route:
      pm_dec_linear mode 0 + pm_dec_controls + pm_dec_sample_topk at k = 1), all together, and - the yardstick of that route -
      top-k 1 through the full logits with no control (topk = 2 builds the same launches; its k = 2 selection costs one more pass);
  (b) the two kernels ALONE, 20 launches back to back in one HIP graph, 10 replays (tools/sampling_bench.py's method), with
      pm_dec_whisper_rules timed the same way in the same run as the yardstick of a latency-bound logit filter;
  (c) the wall time of a run whose rows ALL finish after a quarter of n against the same run without eos_token_id.  The rows are made
      to finish together by planting the eos: the final LayerNorm's bias becomes c x the eos's embedding row, so the eos is every
      row's arg-max at every position, and min_new_tokens = n / 4 - 1 holds it back until then."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="directory for gpt2_small.json / whisper_base.json / controls.txt")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--batch", type=int, default=32)
args = ap.parse_args()

import torch  # noqa: E402

from pytorch_models._hip import decode_plan as plan, lib  # noqa: E402
from pytorch_models.audio2text import generate as G  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

torch.set_grad_enabled(False)
LINES = []
EOS = 11
CONFIGS = [("default tail", dict()), ("eos only", dict(eos=EOS)), ("full logits, k = 2, no control", dict(topk=2, seed=1)),
           ("repetition_penalty 1.3", dict(repetition_penalty=1.3)), ("no_repeat_ngram_size 3", dict(no_repeat_ngram_size=3)),
           ("min_new_tokens (+ eos)", dict(eos=EOS, min_new_tokens=8)),
           ("all together", dict(eos=EOS, min_new_tokens=8, repetition_penalty=1.3, no_repeat_ngram_size=3))]
WINDOW = 32


def say(s):
    print(s, flush=True)
    LINES.append(s)


def window_us(st, starts) -> list[float]:
    """us per step over WINDOW replays from each step index of ``starts``, median over the repeats"""
    res = {s: [] for s in starts}
    for _ in range(args.repeats + 1):  # the first run warms up and captures
        one_step = st.begin(True)
        ev = {}
        for i in range(st.n_steps):
            if i in res:
                ev[i] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[i][0].record()
            one_step()
            if i - WINDOW + 1 in ev:
                ev[i - WINDOW + 1][1].record()
        torch.cuda.synchronize()
        for s, (e0, e1) in ev.items():
            res[s].append(1e3 * e0.elapsed_time(e1) / WINDOW)
    return [statistics.median(v[1:]) for v in res.values()]


def alone_us(launch, n=20, replays=10) -> float:
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        launch(stream.cuda_stream)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=stream):
            for _ in range(n):
                launch(torch.cuda.current_stream().cuda_stream)
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * n)


def kernels_alone(V: int, Ttot: int, hists) -> dict:
    """pm_dec_controls (every control on), pm_dec_finish and pm_dec_whisper_rules on (batch, V) logits and random histories"""
    B, L, dev = args.batch, lib(), torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, V, generator=g).to(dev)
    tokens = torch.randint(0, V, (B, Ttot), generator=g).to(dev)
    cur, fin = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    lp = torch.zeros(B, Ttot, device=dev)
    out = {}

    def call(fn, a):
        def launch(stream):
            rc = fn(*a[:-1], stream)
            assert rc == 0, rc
        return launch

    for h in hists:
        pos = torch.tensor([h - 1], dtype=torch.int32, device=dev)
        for label, kw in (("penalty", dict(repetition_penalty=1.3)), ("ngram 3", dict(no_repeat_ngram=3)), ("ngram 8", dict(no_repeat_ngram=8)),
                          ("all", dict(repetition_penalty=1.3, no_repeat_ngram=3, min_new_tokens=Ttot, eos=EOS))):
            out[f"pm_dec_controls {label}, history {h}"] = alone_us(call(L.pm_dec_controls, plan.controls_args(logits, tokens, pos, 4, None, **kw)))
        ts = V - 1500  # Whisper's layout: the last 1501 ids are timestamps
        a = (logits.data_ptr(), logits.stride(0), V, tokens.data_ptr(), Ttot, pos.data_ptr(), 4, ts - 100, ts - 1, ts, 50, None, 0, None, 0, B, None)
        out[f"pm_dec_whisper_rules, history {h}"] = alone_us(call(L.pm_dec_whisper_rules, a))
        logits.normal_()
    pos = torch.tensor([Ttot - 1], dtype=torch.int32, device=dev)
    out["pm_dec_finish"] = alone_us(call(L.pm_dec_finish, plan.finish_args(tokens, cur, lp, fin, pos, 4, EOS, 0)))
    return {k: round(v, 2) for k, v in out.items()}


def early_exit(dec, memory, prompt, n: int) -> dict:
    """(c): every row's arg-max is the eos, held back by min_new_tokens until a quarter of n"""
    E = dec.token_embs.weight
    old = dec.norm.bias.clone()
    # logit[eos] gains 40 |E_eos|; any other id 40 |E_v| cos(E_v, E_eos), a tenth of that at most for random rows of this width
    dec.norm.bias.copy_((40.0 * E[EOS].float() / E[EOS].float().norm()).to(old.dtype))
    q = n // 4

    def wall(**kw):
        st = G.GreedyDecoder(dec, memory, prompt, n, **kw)
        st.run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            st.run()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts), st

    stop_ms, st = wall(eos=EOS, min_new_tokens=q - 1)
    n_new = st.output_lengths().tolist()
    steps = (st.steps_run, st.n_steps)
    poll = G.POLL_EVERY
    G.POLL_EVERY = 1 << 30  # the same launches, never polled: all n steps
    try:
        full_ms, _ = wall(eos=EOS, min_new_tokens=q - 1)
    finally:
        G.POLL_EVERY = poll
    plain_ms, _ = wall()
    dec.norm.bias.copy_(old)
    return dict(n=n, quarter=q, n_new_min=min(n_new), n_new_max=max(n_new), steps_run=steps[0], n_steps=steps[1], stop_ms=round(stop_ms, 2),
                same_launches_all_steps_ms=round(full_ms, 2), default_tail_no_eos_ms=round(plain_ms, 2))


def bench(name, dec, memory, prompt):
    B, P = prompt.shape
    Tmax = dec.pos_embs.shape[0]
    n = Tmax - P
    say(f"== {name}: batch {B}, prompt {P}, {n} new tokens (to position {Tmax})")
    starts = [64 - WINDOW // 2 - 1, n + P - 1 - WINDOW]
    res = {"steps": {}}
    for label, kw in CONFIGS:
        st = G.GreedyDecoder(dec, memory, prompt, n, **kw)
        near64, nearmax = window_us(st, starts)
        res["steps"][label] = dict(history_64_us=round(near64, 1), history_max_us=round(nearmax, 1), launches=len(st.launches))
        say(f"  {label:34s} {near64:8.1f} us / step near history 64   {nearmax:8.1f} near {Tmax}   ({len(st.launches)} launches)")
        del st
    res["kernels_alone_us"] = kernels_alone(dec.token_embs.weight.shape[0], Tmax, (64, Tmax))
    for k, v in res["kernels_alone_us"].items():
        say(f"  {k:44s} {v:7.2f} us")
    res["early_exit"] = ee = early_exit(dec, memory, prompt, n)
    say(f"  early exit: rows finish after {ee['n_new_min']}..{ee['n_new_max']} of {n} new tokens (asked: {ee['quarter']}); {ee['steps_run']} of "
        f"{ee['n_steps']} steps run: {ee['stop_ms']:.1f} ms; the same launches for all steps {ee['same_launches_all_steps_ms']:.1f} ms; "
        f"the default tail without eos_token_id {ee['default_tail_no_eos_ms']:.1f} ms")
    return res


def main():
    from pytorch_models.audio2text import Whisper
    from pytorch_models.text import GPT2

    B = args.batch
    m = GPT2.from_hf("gpt2").eval()
    fill_module(m, 1)
    bf16_round_(m)
    m = m.to(torch.bfloat16).cuda()
    out = {"gpt2_small": bench("GPT-2 small", m, None, synth_tokens("controls_bench", (B, 4), 50257, 2).cuda())}
    del m
    w = Whisper.from_openai("base").eval()
    fill_module(w, 56)
    bf16_round_(w)
    w = w.to(torch.bfloat16).cuda()
    memory = synth_input("controls_bench_memory", (B, 1500, 512), 56).to(torch.bfloat16).cuda()
    out["whisper_base"] = bench("Whisper-base decoder", w.decoder, memory, synth_tokens("controls_bench_w", (B, 4), 51865, 3).cuda())
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k, v in out.items():
            with open(os.path.join(args.out, k + ".json"), "w") as f:
                json.dump(v, f, indent=1)
        with open(os.path.join(args.out, "controls.txt"), "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
