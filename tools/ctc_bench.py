"""CTC heads on MI355X: Wav2Vec2CTC's kernels (csrc/ctc.hip) against the same rows through stock PyTorch-ROCm, synthetic weights.
Not a BASELINE metric - the measurement behind profiles/ctc/README.md.
    python tools/ctc_bench.py [--out profiles/ctc]
Workload: wav2vec2-base geometry (12 x 768, legacy stem, post-norm), V = 32, 32 clips of 10 s (499 frames each), transcripts of
150 labels.  In ONE process, warm (the operands were just touched; nothing is flushed) unless a leg says otherwise:
  (a) the encoder alone, then decode / score / align end to end (encoder included)                                    ms
  (b) each kernel alone on the encoder's rows: ops.ctc_head against its read-h-once bound (bytes of h / time), ops.ctc_greedy,
      ops.ctc_forward and ops.ctc_viterbi for 32 clips and for one clip alone, with the time per frame (the chain is serial in T)
  (c) the yardsticks on the same rows: F.linear + log_softmax + argmax on the device + the collapse on the host; F.ctc_loss on
      the device from the kernels' log-probabilities; a numpy Viterbi on the host (vectorised over the states and the clips)
End-to-end and stock figures are medians of `--repeats` eager runs after `--warmup` untimed ones (HIP events around one run); an
eager launch of these small kernels is bounded by the host (~18 us from Python), so the kernels ALONE are timed as HIP graphs of 20
back-to-back launches, 10 replays after one: time per launch, the kernel boundary included.  Host legs are wall time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="directory for wav2vec2_base.json / wav2vec2_base.txt")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--labels", type=int, default=150)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.audio import Wav2Vec2, Wav2Vec2CTC  # noqa: E402
from pytorch_models.transformer import _f32  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input, synth_tokens  # noqa: E402

torch.set_grad_enabled(False)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, repeats=None):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats or args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def graphed(fn, n=20, replays=10):
    """ms per launch of fn inside a captured graph of n serial launches"""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for i in range(n):
            fn(i)
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (replays * n)


def host_viterbi(lp, targets, blank):
    """numpy float32, every clip at once (all share T and U here), one step per frame -> (start, stop (B, U), score (B))"""
    B, T, _ = lp.shape
    U = targets.shape[1]
    S = 2 * U + 1
    ext = np.full((B, S), blank, dtype=np.int64)
    ext[:, 1::2] = targets
    skip = np.zeros((B, S), dtype=bool)
    skip[:, 2:] = (ext[:, 2:] != blank) & (ext[:, 2:] != ext[:, :-2])
    ninf = np.float32(-np.inf)
    v = np.full((B, S), ninf, dtype=np.float32)
    em = np.take_along_axis(lp, ext[:, None, :].repeat(T, 1), 2)  # (B, T, S)
    v[:, :2] = em[:, 0, :2]
    bp = np.zeros((B, T, S), dtype=np.int8)
    pad1, pad2 = np.full((B, 1), ninf, dtype=np.float32), np.full((B, 2), ninf, dtype=np.float32)
    for t in range(1, T):
        p1 = np.concatenate([pad1, v[:, :-1]], 1)
        p2 = np.where(skip, np.concatenate([pad2, v[:, :-2]], 1), ninf)
        stay = (v >= p1) & (v >= p2)
        one = ~stay & (p1 >= p2)
        bp[:, t] = np.where(stay, 0, np.where(one, 1, 2))
        v = np.where(stay, v, np.where(one, p1, p2)) + em[:, t]
    start, stop = np.full((B, U), -1, dtype=np.int32), np.full((B, U), -1, dtype=np.int32)
    score = np.full(B, ninf, dtype=np.float32)
    for b in range(B):
        s = S - 1 if not v[b, S - 2] > v[b, S - 1] else S - 2
        if not v[b, s] > ninf:
            continue
        score[b] = v[b, s]
        for t in range(T - 1, -1, -1):
            if s & 1:
                if stop[b, s >> 1] < 0:
                    stop[b, s >> 1] = t + 1
                start[b, s >> 1] = t
            if t:
                s -= int(bp[b, t, s])
    return start, stop, score


B, V, U, BLANK = args.batch, 32, args.labels, 0
m = Wav2Vec2CTC(Wav2Vec2(12, 768, stem_bias=False, stem_legacy=True, pre_norm=False), V, BLANK)
fill_module(m, 3)
with torch.no_grad():
    m.lm_head.weight.mul_(8.0)
bf16_round_(m)
m = m.to(torch.bfloat16).cuda().eval()
x = synth_input("ctc_bench_wave", (B, 160000), 4).cuda()
targets = (synth_tokens("ctc_bench_targets", (B, U), V - 1, 5) + 1).to(torch.int32)  # ids 1 .. V - 1: never the blank
tl = [U] * B
h = m.encoder(x)
T, d = h.shape[1], h.shape[2]
rows = h.reshape(B * T, d)
M = rows.shape[0]
w, bias = m.lm_head.weight, _f32(m.lm_head, "b", m.lm_head.bias)
seq = ops.seq_lens([T] * B, T, "cuda")
seq1 = ops.seq_lens([T], T, "cuda")
tg = targets.cuda()
res = {"workload": f"wav2vec2-base geometry, V = {V}, {B} clips x 160000 samples = {T} frames, {U} labels per clip",
       "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats, "state": "warm",
       "h_bytes": 2 * M * d, "logp_bytes": 4 * M * V}

ms_e = timed(lambda: m.encoder(x))
ms_dec = timed(lambda: m.decode(x))
ms_sc = timed(lambda: m.score(x, targets, tl))
ms_al = timed(lambda: m.align(x, targets, tl))
res["end_to_end_ms"] = {"encoder": ms_e, "decode": ms_dec, "score": ms_sc, "align": ms_al}
say(f"(a) encoder alone {ms_e:8.2f} ms; decode {ms_dec:8.2f} ms, score {ms_sc:8.2f} ms, align {ms_al:8.2f} ms end to end (encoder included)")

logp, best, blp = ops.ctc_head(rows, w, bias)
ms_h_eager = timed(lambda: ops.ctc_head(rows, w, bias, out=logp, best_out=best, best_logp_out=blp), repeats=4 * args.repeats)
ms_h = graphed(lambda i=0: ops.ctc_head(rows, w, bias, out=logp, best_out=best, best_logp_out=blp))
NCOPY = 12  # 12 x 24.5 MB = 294 MB of hidden rows, more than the 256 MB Infinity Cache: a copy is read 11 launches after its last use
copies = [rows.clone() for _ in range(NCOPY)]
ms_h_rot = graphed(lambda i=0: ops.ctc_head(copies[i % NCOPY], w, bias, out=logp, best_out=best, best_logp_out=blp), n=2 * NCOPY)
del copies
hb = 2e-6 * M * d
res["head"] = {"ms_eager_launch": ms_h_eager, "ms_warm": ms_h, "ms_rotating": ms_h_rot, "h_read_GBps_warm": hb / ms_h, "h_read_GBps_rotating": hb / ms_h_rot,
               "bound_ms_at_6.3TBps": hb / 6300.0, "bound_ms_at_8TBps": hb / 8000.0}
say(f"(b) ops.ctc_head M={M} K={d} V={V}: {1e3 * ms_h:7.2f} us warm (the same {hb:.1f} MB of h every launch) = {hb / ms_h:6.0f} GB/s, "
    f"{1e3 * ms_h_rot:7.2f} us over {NCOPY} rotating copies of h = {hb / ms_h_rot:6.0f} GB/s; read-h-once bound {1e3 * hb / 6300.0:.2f} us at the 6.3 TB/s "
    f"a copy reaches ({1e3 * hb / 8000.0:.2f} us at the 8 TB/s peak); {4e-6 * M * V:.1f} MB of logp written; one eager launch {1e3 * ms_h_eager:.1f} us (host-bound)")
tl_d = torch.tensor(tl, dtype=torch.int32, device="cuda")
ws = torch.empty(ops.ctc_ws_bytes(B, T, U), dtype=torch.uint8, device="cuda")
logp1 = logp[:T]
ms_g = graphed(lambda i=0: ops.ctc_greedy(best, seq, blp, BLANK))
ms_f = graphed(lambda i=0: ops.ctc_forward(logp, seq, tg, tl_d, BLANK))
ms_f1 = graphed(lambda i=0: ops.ctc_forward(logp1, seq1, tg[:1], tl_d[:1], BLANK))
ms_v = graphed(lambda i=0: ops.ctc_viterbi(logp, seq, tg, tl_d, BLANK, ws=ws))
ms_v1 = graphed(lambda i=0: ops.ctc_viterbi(logp1, seq1, tg[:1], tl_d[:1], BLANK, ws=ws))
res["greedy"] = {"ms": ms_g}
res["forward"] = {"ms": ms_f, "ms_one_clip": ms_f1, "ns_per_frame": 1e6 * ms_f / T, "ns_per_frame_one_clip": 1e6 * ms_f1 / T, "states": 2 * U + 1}
res["viterbi"] = {"ms": ms_v, "ms_one_clip": ms_v1, "ns_per_frame": 1e6 * ms_v / T, "ns_per_frame_one_clip": 1e6 * ms_v1 / T, "ws_bytes": ws.numel()}
say(f"(b) ops.ctc_greedy, {B} clips              {1e3 * ms_g:9.2f} us")
say(f"(b) ops.ctc_forward, {B} clips, {2 * U + 1} states  {1e3 * ms_f:9.2f} us = {1e6 * ms_f / T:6.0f} ns per frame; one clip alone {1e3 * ms_f1:.2f} us = {1e6 * ms_f1 / T:.0f} ns per frame")
say(f"(b) ops.ctc_viterbi, {B} clips             {1e3 * ms_v:9.2f} us = {1e6 * ms_v / T:6.0f} ns per frame (backtrace included); one clip alone {1e3 * ms_v1:.2f} us = "
    f"{1e6 * ms_v1 / T:.0f} ns per frame; back-pointer workspace {ws.numel() / 1e6:.2f} MB")


def stock_head():
    lp = torch.log_softmax(F.linear(rows, w, bias.to(w.dtype)).float(), -1)
    return lp, lp.argmax(-1)


ms_sh = timed(stock_head)
t0 = time.perf_counter()
am = stock_head()[1].view(B, T).cpu().numpy()
texts = []
for b in range(B):
    a = am[b]
    keep = (a != BLANK) & np.r_[True, a[1:] != a[:-1]]
    texts.append(a[keep])
t1 = time.perf_counter()
lp_tbv = logp.view(B, T, V).transpose(0, 1).contiguous()
in_len, tg_len = torch.full((B,), T, dtype=torch.long, device="cuda"), torch.full((B,), U, dtype=torch.long, device="cuda")
tg64 = tg.long()
ms_loss = timed(lambda: F.ctc_loss(lp_tbv, tg64, in_len, tg_len, blank=BLANK, reduction="none"))
loss = F.ctc_loss(lp_tbv, tg64, in_len, tg_len, blank=BLANK, reduction="none")
lp_host = logp.view(B, T, V).cpu().numpy()
t2 = time.perf_counter()
hs0, hs1, hsc = host_viterbi(lp_host, targets.numpy(), BLANK)
t3 = time.perf_counter()
res["stock"] = {"linear_log_softmax_argmax_device_ms": ms_sh, "argmax_copy_and_host_collapse_wall_ms": 1e3 * (t1 - t0),
                "ctc_loss_device_ms": ms_loss, "numpy_viterbi_host_wall_ms": 1e3 * (t3 - t2)}
say(f"(c) stock F.linear + log_softmax + argmax on the device {ms_sh:9.4f} ms; the same plus the copy and the host collapse, wall {1e3 * (t1 - t0):.2f} ms")
say(f"(c) stock F.ctc_loss on the device from the same log-probabilities {ms_loss:9.4f} ms")
say(f"(c) numpy Viterbi on the host from the same log-probabilities, wall {1e3 * (t3 - t2):9.1f} ms")

ids, n, start, path = ops.ctc_greedy(best, seq, blp, BLANK)
ll = ops.ctc_forward(logp, seq, tg, tl, BLANK)
vs0, vs1, vsc = ops.ctc_viterbi(logp, seq, tg, tl, BLANK, ws=ws)
same_text = all(int(n[b]) == len(texts[b]) and np.array_equal(ids[b, : len(texts[b])].cpu().numpy(), texts[b]) for b in range(B))
res["agreement"] = {"decode_equals_the_stock_collapse": bool(same_text),
                    "max_rel_loglik_vs_ctc_loss": float(((ll + loss).abs() / loss.abs()).max()),
                    "viterbi_equals_the_host_loop": bool(np.array_equal(vs0.cpu().numpy(), hs0) and np.array_equal(vs1.cpu().numpy(), hs1)
                                                         and np.array_equal(vsc.cpu().numpy(), hsc))}
say(f"    agreement: decode == stock collapse {same_text} (the stock bf16 logits may flip near-ties); max |loglik + ctc_loss| / |ctc_loss| "
    f"{res['agreement']['max_rel_loglik_vs_ctc_loss']:.3e}; viterbi == the host loop {res['agreement']['viterbi_equals_the_host_loop']}")
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "wav2vec2_base.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "wav2vec2_base.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
