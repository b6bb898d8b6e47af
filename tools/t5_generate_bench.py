"""T5Model.generate on MI355X: new tokens/s and us per decode step (replayed and eager), the encoder + cross-K/V set-up
apart, against (a) the full-prefix loop generate_ids over the same rows and (b) a plain-torch KV-cached step (F.linear + SDPA on
the same bf16 weights), with the step's byte count over the HBM rates.  Synthetic weights; never stops (eos_id = -1).  Writes
profiles/t5_generate/<size>_b<B>_s<S>_n<N>.json.  Not a BASELINE metric - a measurement to go with tests/test_hip_t5_generate.py.

    python tools/t5_generate_bench.py [--size small] [--batch 32] [--src 512] [--new 128] [--reps 10] [--baseline-rows 2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/t5_generate_bench.py --size small --reps 3 --baseline-rows 0 --no-torch
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_models.text import T5Model  # noqa: E402
from pytorch_models.text.t5_generate import T5DecodeState, distance_lut  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_tokens  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="small")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--src", type=int, default=512)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--baseline-rows", type=int, default=2, help="rows timed through generate_ids (rows are independent: scaled to the batch)")
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
torch.set_grad_enabled(False)
B, S, N = args.batch, args.src, args.new
m = T5Model.from_t5x(f"t5_1_1-{args.size}")
fill_module(m, 1)
bf16_round_(m)
m = m.to(torch.bfloat16).cuda().eval()
src = synth_tokens("t5_gen_bench_src", (B, S), 32128, 2).cuda()
lengths = torch.full((B,), S, dtype=torch.int32, device="cuda")  # full rows through the padded path (its per-row bias is built)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


st = T5DecodeState(m, B, S, 1, N, 0, -1, False)
st.bind(src, lengths, None)
st.run(True)  # warm-up + capture
st.run(False)
setup = timed(lambda: st.bind(src, lengths, None), args.reps)
replay = timed(lambda: st.run(True), args.reps)
eager = timed(lambda: st.run(False), max(3, args.reps // 3))
steps = st.n_steps
res = dict(size=args.size, batch=B, src=S, new=N, steps=steps, launches_per_step=len(st.launches), fused_self=st.fuse_self,
           device=torch.cuda.get_device_name(0), reps=args.reps,
           setup_ms=dict(median=setup[0] * 1e3, min=setup[1] * 1e3, max=setup[2] * 1e3), encoder_bias_bytes=st.encoder_bias_bytes,
           step_us_replayed=dict(median=replay[0] / steps * 1e6, min=replay[1] / steps * 1e6, max=replay[2] / steps * 1e6),
           step_us_eager=dict(median=eager[0] / steps * 1e6, min=eager[1] / steps * 1e6, max=eager[2] / steps * 1e6),
           new_tokens_per_s_decode=B * N / replay[0], new_tokens_per_s_with_setup=B * N / (replay[0] + setup[0]))

# ---- bytes one step must move: decoder weights, classifier, cross K/V (all keys), self caches (mean fill)
dec = m.decoder
H = dec.layers[0].sa.n_heads
w_bytes = sum(p.numel() * 2 for n, p in dec.named_parameters() if not n.startswith("attn_bias")) + m.classifier.weight.numel() * 2
cross_bytes = len(dec.layers) * B * S * 2 * H * 64 * 2
self_bytes = len(dec.layers) * B * H * ((steps + 1) / 2) * 64 * 2 * 2
tot_bytes = w_bytes + cross_bytes + self_bytes
step_s = replay[0] / steps
res["step_bytes"] = dict(weights=w_bytes, cross_kv=cross_bytes, self_cache_mean=self_bytes, total=tot_bytes)
res["roofline"] = dict(fraction_of_8TBs=tot_bytes / 8e12 / step_s, fraction_of_measured_copy_6p29TBs=tot_bytes / 6.29e12 / step_s)
print(json.dumps({k: res[k] for k in ("size", "setup_ms", "step_us_replayed", "step_us_eager", "new_tokens_per_s_decode", "roofline")}), flush=True)

# ---- (a) the full-prefix loop, one row at a time (what generate_ids does; rows are independent, so a few rows scale to the batch)
if args.baseline_rows > 0:
    rows = min(args.baseline_rows, B)
    m.generate_ids(src[0], 4, eos_id=-1)
    t = timed(lambda: [m.generate_ids(src[b], N + 1, eos_id=-1) for b in range(rows)], 1)[0]
    res["generate_ids"] = dict(rows_timed=rows, s_per_row=t / rows, s_for_batch=t / rows * B, new_tokens_per_s=N * rows / t)
    res["speedup_vs_generate_ids"] = (t / rows * B) / (replay[0] + setup[0])
    print(json.dumps(dict(generate_ids=res["generate_ids"], speedup=res["speedup_vs_generate_ids"])), flush=True)


# ---- (b) a plain-torch KV-cached step: F.linear + SDPA, bf16, the same weights, the position known to the host
def torch_decode():
    memory = m.encode(src)
    d, inner = memory.shape[-1], H * 64
    lut = distance_lut(dec.attn_bias, N + 1).to(torch.bfloat16)
    cross, caches = [], []
    for layer in dec.layers:
        k = F.linear(memory, layer.ca.k_proj.weight).view(B, S, H, 64).transpose(1, 2)
        v = F.linear(memory, layer.ca.v_proj.weight).view(B, S, H, 64).transpose(1, 2)
        cross.append((k, v))
        caches.append((torch.empty(B, H, N + 1, 64, dtype=torch.bfloat16, device="cuda"), torch.empty(B, H, N + 1, 64, dtype=torch.bfloat16, device="cuda")))
    wqkv = [torch.cat([layer.sa.q_proj.weight, layer.sa.k_proj.weight, layer.sa.v_proj.weight], 0) for layer in dec.layers]

    def rms(norm, x):
        xf = x.float()
        return (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + norm.eps) * norm.weight.float()).to(torch.bfloat16)

    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    out = [tok]
    for t in range(N):
        x = m.token_embs.weight[tok]
        for layer, (kc, vc), (ck, cv), w in zip(dec.layers, caches, cross, wqkv):
            q, k, v = F.linear(rms(layer.sa_norm, x), w).view(B, 3, H, 64).unbind(1)
            kc[:, :, t], vc[:, :, t] = k, v
            bias = lut[:, : t + 1].flip(1)[None, :, None, :]  # key j at distance t - j
            a = F.scaled_dot_product_attention(q[:, :, None], kc[:, :, : t + 1], vc[:, :, : t + 1], attn_mask=bias.expand(B, H, 1, t + 1))
            x = x + F.linear(a.reshape(B, inner), layer.sa.out_proj.weight)
            q = F.linear(rms(layer.ca_norm, x), layer.ca.q_proj.weight).view(B, H, 1, 64)
            a = F.scaled_dot_product_attention(q, ck, cv)
            x = x + F.linear(a.reshape(B, inner), layer.ca.out_proj.weight)
            h = rms(layer.mlp_norm, x)
            g = F.gelu(F.linear(h, layer.mlp[0].w.weight), approximate="tanh") * F.linear(h, layer.mlp[0].v.weight)
            x = x + F.linear(g, layer.mlp[2].weight)
        tok = F.linear(rms(dec.norm, x), m.classifier.weight).float().argmax(-1)
        out.append(tok)
    return torch.stack(out, 1)


if not args.no_torch:
    torch_decode()
    t = timed(torch_decode, max(3, args.reps // 3))
    res["torch_kv_cached"] = dict(s=t[0], new_tokens_per_s=B * N / t[0], note="encoder (this build's) + cross K/V + eager F.linear / SDPA steps")
    res["speedup_vs_torch_kv_cached"] = t[0] / (replay[0] + setup[0])
    print(json.dumps(dict(torch_kv_cached=res["torch_kv_cached"], speedup=res["speedup_vs_torch_kv_cached"])), flush=True)

out_dir = os.path.join(ROOT, os.environ.get("PM_PROFILE_DIR", os.path.join("profiles", "t5_generate")))
os.makedirs(out_dir, exist_ok=True)
path = os.path.join(out_dir, f"{args.size}_b{B}_s{S}_n{N}.json")
with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
print("wrote", path)
