"""Token timestamps on MI355X: Whisper.align's kernels (csrc/align.hip) against the stock-ops route, synthetic weights.  Not a
BASELINE metric - the measurement behind profiles/align/README.md.
    python tools/align_bench.py [--out profiles/align]
Workload: Whisper-base decoder (8 layers, d = 512, 8 heads), 32 clips x 224 tokens x 1500 frames, the default alignment heads
(layers 4-7, 32 heads), skip_first = 4, skip_last = 1.  In ONE process:
  (a) decoder.align(...) end to end                                ms, peak memory above the model and the encoder output
  (b) each kernel alone on one layer's q / k (8 heads): ops.align_lse, ops.align_matrix; ops.align_dtw on the final m, with the
      number of anti-diagonals (= barriers of the sweep) and the time per diagonal
  (c) the kernels from the same q / k of the four layers (4 x (lse + matrix) + dtw) against the stock PyTorch-ROCm yardstick on the
      same q / k: einsum + softmax + std_mean + reflect pad / unfold / sort median on the device, then the copy of m to the host
      and a numpy DTW vectorised over the anti-diagonals and the clips; ms and peak device memory of each
Device figures are medians of `--repeats` runs after `--warmup` untimed ones (HIP events); the host DTW is wall time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="directory for whisper_base.json / whisper_base.txt")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batch", type=int, default=32)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.audio2text import Whisper  # noqa: E402
from pytorch_models.audio2text import align as al  # noqa: E402
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
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(repeats or args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), torch.cuda.max_memory_allocated() - base


def host_dtw(m, skip_first, skip_last):
    """numpy, float32: every clip at once, one step per anti-diagonal -> start (B, L) int32 (all clips share N and M here)."""
    B, L, M = m.shape
    N = L - skip_first - skip_last
    x = -m[:, skip_first:skip_first + N]
    cost = np.full((B, N + 1, M + 1), np.inf, dtype=np.float32)
    cost[:, 0, 0] = 0
    trace = np.full((B, N + 1, M + 1), 2, dtype=np.int8)
    trace[:, :, 0] = 1
    trace[:, 0, :] = 2
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[:, i - 1, j - 1], cost[:, i - 1, j], cost[:, i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        cost[:, i, j] = x[:, i - 1, j - 1] + np.where(t0, c0, np.where(t1, c1, c2))
        trace[:, i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    start = np.full((B, L), -1, dtype=np.int32)
    for b in range(B):
        i, j, tr = N, M, trace[b]
        while i > 0 or j > 0:
            if i > 0 and j > 0:
                start[b, skip_first + i - 1] = j - 1
            t = tr[i, j]
            i, j = (i - 1, j - 1) if t == 0 else ((i - 1, j) if t == 1 else (i, j - 1))
    return start


B, L, S, V = args.batch, 224, 1500, 51865
SKIP = (4, 1)
w = Whisper.from_openai("base")
fill_module(w, 1)
bf16_round_(w)
w = w.to(torch.bfloat16).cuda().eval()
dec = w.decoder
H, n_layers = dec.layers[0].sa.n_heads, len(dec.layers)
inner = 64 * H
tokens = synth_tokens("align_bench", (B, L), V, 2).cuda()
memory = w.encoder(synth_input("align_bench_mel", (B, 80, 2 * S), 2).cuda())
heads = al.default_heads(n_layers, H)
by = al._by_layer(heads)
A = len(heads)
res = {"workload": f"Whisper-base decoder, {B} clips x {L} tokens x {S} frames, {A} heads of layers {sorted(by)}",
       "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
       "materialised_probabilities_bytes": 4 * B * A * L * S, "m_bytes": 4 * B * L * S}

ms, peak = timed(lambda: dec.align(tokens, memory, skip_first=SKIP[0], skip_last=SKIP[1]))
res["align_end_to_end"] = {"ms": ms, "peak_bytes": peak}
say(f"(a) decoder.align end to end         {ms:9.2f} ms   peak {peak / 1e6:9.1f} MB above the model and memory")

# the q / k projections of the aligned layers, as align() makes them
qk = {}


def fold(l, q, ca, mem):
    wkv, bkv = ca._pack("kv")
    qk[l] = (q, ops.linear(mem.reshape(-1, mem.shape[-1]), wkv, bkv).view(B, S, 2 * inner)[..., :inner])


al._walk(dec, ops.embed_tokens(tokens, al._wb(dec.token_embs, "E", dec.token_embs.weight), al._f32(dec, "pos", dec.pos_embs)), memory, by, fold)
lens_d = ops.align_counts(L, B, 1, L, "lengths", tokens.device)
frs_d = ops.align_counts(S, B, 4, S, "frames", tokens.device)
heads_d = {l: torch.tensor(v, dtype=torch.int32).cuda() for l, v in by.items()}
m = torch.empty((B, L, S), dtype=torch.float32, device="cuda")
l0 = min(by)
q0, k0 = qk[l0]
flop = 2.0 * B * len(by[l0]) * L * S * 64
ms_l, pk_l = timed(lambda: ops.align_lse(q0, k0, heads_d[l0], lens_d, frs_d))
lse0 = ops.align_lse(q0, k0, heads_d[l0], lens_d, frs_d)
ms_m, pk_m = timed(lambda: ops.align_matrix(q0, k0, heads_d[l0], lens_d, frs_d, lse0, m, 1.0 / A, True))
res["lse_one_layer"] = {"ms": ms_l, "peak_bytes": pk_l, "tflops": flop / ms_l / 1e9}
res["matrix_one_layer"] = {"ms": ms_m, "peak_bytes": pk_m, "qk_tflops": flop * 32 / 26 / ms_m / 1e9, "m_write_GBps": 4e-6 * B * L * S / ms_m}
say(f"(b) ops.align_lse, one layer ({len(by[l0])} heads) {ms_l:9.3f} ms   {flop / ms_l / 1e9:7.1f} TFLOP/s of QK^T")
say(f"(b) ops.align_matrix, one layer       {ms_m:9.3f} ms   m = {4e-6 * B * L * S:.1f} MB written once; QK^T again at 32 / 26 columns")


def kernels():
    for i, l in enumerate(sorted(by)):
        q, k = qk[l]
        lse = ops.align_lse(q, k, heads_d[l], lens_d, frs_d)
        ops.align_matrix(q, k, heads_d[l], lens_d, frs_d, lse, m, 1.0 / A, i == 0)
    return ops.align_dtw(m, lens_d, frs_d, *SKIP)


start = kernels()
ws = torch.empty(ops.align_ws_bytes(B, L, S), dtype=torch.uint8, device="cuda")
ms_d, pk_d = timed(lambda: ops.align_dtw(m, lens_d, frs_d, *SKIP, ws=ws))
N = L - sum(SKIP)
diag = N + S - 1
ms_d1, _ = timed(lambda: ops.align_dtw(m[:1], lens_d[:1], frs_d[:1], *SKIP, ws=ws))
res["dtw"] = {"ms": ms_d, "ms_one_clip": ms_d1, "anti_diagonals": diag, "ns_per_diagonal": 1e6 * ms_d / diag, "ns_per_diagonal_one_clip": 1e6 * ms_d1 / diag,
              "ws_bytes": ws.numel()}
say(f"(b) ops.align_dtw, {B} clips           {ms_d:9.3f} ms   {diag} anti-diagonals = barriers of the sweep: {1e6 * ms_d / diag:.0f} ns per diagonal "
    f"(backtrace included); one clip alone {ms_d1:.3f} ms = {1e6 * ms_d1 / diag:.0f} ns per diagonal; trace workspace {ws.numel() / 1e6:.1f} MB")
ms_k, pk_k = timed(kernels)
res["kernels_from_qk"] = {"ms": ms_k, "peak_bytes": pk_k}
say(f"(c) kernels from q / k (4 x (lse + matrix) + dtw) {ms_k:9.2f} ms   peak {pk_k / 1e6:9.1f} MB")


def stock_matrix():
    acc = None
    for l in sorted(by):
        q, k = qk[l]
        hs = torch.tensor(by[l], device="cuda")
        qh = q.view(B, L, H, 64).transpose(1, 2)[:, hs].float()
        kh = k.reshape(B, S, H, 64).transpose(1, 2)[:, hs].float()
        p = torch.softmax(torch.einsum("bhld,bhsd->bhls", qh, kh) * 0.125, -1)
        std, mean = torch.std_mean(p, dim=-2, keepdim=True, unbiased=False)
        n = (p - mean) / std
        med = torch.nn.functional.pad(n, (3, 3, 0, 0), mode="reflect").unfold(-1, 7, 1).sort(-1).values[..., 3]
        acc = med.sum(1) if acc is None else acc + med.sum(1)
    return acc / A


ms_s, pk_s = timed(stock_matrix, repeats=3)
t0 = time.perf_counter()
m_host = stock_matrix().cpu().numpy()
t1 = time.perf_counter()
start_host = host_dtw(m_host, *SKIP)
t2 = time.perf_counter()
res["stock"] = {"device_ms": ms_s, "device_peak_bytes": pk_s, "matrix_and_copy_wall_ms": 1e3 * (t1 - t0), "host_dtw_wall_ms": 1e3 * (t2 - t1),
                "total_ms": ms_s + 1e3 * (t2 - t1)}
say(f"(c) stock ops on the same q / k: device part {ms_s:9.2f} ms, peak {pk_s / 1e6:9.1f} MB; numpy DTW on the host {1e3 * (t2 - t1):9.1f} ms "
    f"(matrix + copy to the host, wall: {1e3 * (t1 - t0):.1f} ms)")
mk = m.cpu().numpy()
res["agreement"] = {"max_abs_m_difference": float(np.abs(mk - m_host).max()),
                    "start_equal_to_host_dtw_on_the_kernels_m": bool((host_dtw(mk, *SKIP) == start.cpu().numpy()).all()),
                    "start_rows_equal_to_the_stock_route": int((start_host == start.cpu().numpy()).sum()), "start_rows": int(start_host.size)}
say(f"    agreement: max |m - stock m| {res['agreement']['max_abs_m_difference']:.3e}; start == numpy DTW on the kernels' m: "
    f"{res['agreement']['start_equal_to_host_dtw_on_the_kernels_m']}; rows equal to the stock route's: "
    f"{res['agreement']['start_rows_equal_to_the_stock_route']} of {start_host.size}")
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "whisper_base.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "whisper_base.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
