"""Mixer-B/16 on one MI355X: img/s of the bf16 forward at batch 256, 224 x 224 on synthetic weights, the time of each kernel class
(each launch timed on its own over a warmed window of tens of ms, tools/_timing.py, times its count per step), its algorithmic
FLOPs and bytes and their fraction of the bound, and two same-box yardsticks in the same run:
  (a) the same weights through stock PyTorch-ROCm ops (the reference's arithmetic in bf16);
  (b) the token-mixing half built from the ops that existed before pm_mixer_token_mix_bf16 - LayerNorm, transpose().contiguous()
      into a K-padded buffer, two ops.linear on padded operands, a transposing residual add - against the fused kernel, three
      alternating rounds so the spread is visible.
The yardsticks live in this tool only.  Prints one JSON line.
    python tools/mixer_bench.py [--tag B/16] [--batch 256] [--side 224]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.image import MLPMixer  # noqa: E402
from pytorch_models.transformer import _f32, _fold_ln, derived  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

PEAK_BF16 = 2.5e15  # FLOP/s, dense bf16 MFMA (spec)
HBM_SPEC = 8.0e12  # B/s
L2_SHARED = 17.0e12  # B/s: measured rate of rows every workgroup shares, served by the XCDs' L2 (16.8 - 18.8)

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="B/16")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--side", type=int, default=224)
args = ap.parse_args()
torch.set_grad_enabled(False)

m = MLPMixer.from_google(args.tag, img_size=args.side).eval()
fill_module(m, 161)
bf16_round_(m)
m = m.to(torch.bfloat16).cuda()
B, S = args.batch, args.side
x = synth_input("mixer_bench", (B, 3, S, S), 161).cuda()


def window(fn, ms_per_call):
    """warm-up and timed windows of ~40 ms each"""
    n = max(3, int(40.0 / max(ms_per_call, 1e-3)))
    return time_us(fn, warmup=n, iters=n)


route = m.route(B)
t_probe = time_us(lambda: m(x), warmup=2, iters=3) / 1e3
t_model = window(lambda: m(x), t_probe)

# ---- yardstick (a): stock PyTorch-ROCm ops on the same bf16 weights
x_bf = x.to(torch.bfloat16)


def ref_forward(imgs):
    h = F.conv2d(imgs, m.patch_embed.weight, m.patch_embed.bias, stride=m.patch_embed.stride).flatten(2).transpose(1, 2)
    for l in m.layers:
        tm, cm = l.token_mixing, l.channel_mixing
        n = F.layer_norm(h, h.shape[-1:], l.norm1.weight, l.norm1.bias, l.norm1.eps).transpose(-1, -2)
        h = h + F.linear(F.gelu(F.linear(n, tm.linear1.weight, tm.linear1.bias)), tm.linear2.weight, tm.linear2.bias).transpose(-1, -2)
        n = F.layer_norm(h, h.shape[-1:], l.norm2.weight, l.norm2.bias, l.norm2.eps)
        h = h + F.linear(F.gelu(F.linear(n, cm.linear1.weight, cm.linear1.bias)), cm.linear2.weight, cm.linear2.bias)
    return F.layer_norm(h, h.shape[-1:], m.norm.weight, m.norm.bias, m.norm.eps).mean(1)


t_ref_probe = time_us(lambda: ref_forward(x_bf), warmup=2, iters=3) / 1e3
t_ref = window(lambda: ref_forward(x_bf), t_ref_probe)
y_ref = ref_forward(x_bf).float()
err = float((y_ref - m(x).float()).norm() / y_ref.norm())

# ---- the layer's operands
ck = m.forward_checkpoints(x)
h0 = ck["tokens"]
N, T, C = h0.shape
M = N * T
l = m.layers[0]
tm, cm = l.token_mixing, l.channel_mixing
Dt, hid = tm.linear1.out_features, cm.linear1.out_features
g1, be1, w1f, b1, w2f, b2 = l._token_operands()
stats = ops.row_stats(h0.view(M, C), l.norm1.eps)
Tp = w1f.shape[1] * 16


def fused():
    return ops.mixer_token_mix(h0, stats, g1, be1, w1f, b1, w2f, b2, want_row_stats=True)


# ---- yardstick (b): the token-mixing half from the ops that predate the fused kernel
Kp = -(-T // 64) * 64  # ops.linear wants K % 64 == 0
w1k = torch.zeros((Dt, Kp), dtype=torch.bfloat16, device="cuda")
w1k[:, :T] = tm.linear1.weight
w2k = torch.zeros((Kp, Dt), dtype=torch.bfloat16, device="cuda")  # N padded: the output rows keep the row stride of the input
w2k[:T] = tm.linear2.weight
b2k = torch.zeros(Kp, dtype=torch.float32, device="cuda")
b2k[:T] = b2
xt = torch.zeros((N, C, Kp), dtype=torch.bfloat16, device="cuda")  # pad columns stay zero


def composed():
    n = ops.layernorm(h0.view(M, C), g1, be1, l.norm1.eps).view(N, T, C)
    xt[:, :, :T].copy_(n.transpose(1, 2))  # the transposing copy
    u = ops.linear(xt.view(N * C, Kp), w1k, b1, act="gelu")
    v = ops.linear(u, w2k, b2k).view(N, C, Kp)
    return h0 + v[:, :, :T].transpose(1, 2)  # the transposing residual add


err_b = float((composed().float() - fused()[0].float()).norm() / fused()[0].float().norm())
rounds = []
for _ in range(3):
    tf = window(fused, 0.2)
    tc = window(composed, 1.0)
    rounds.append(dict(fused_us=round(tf, 1), composed_us=round(tc, 1), speedup=round(tc / tf, 3)))

# ---- per kernel class: one launch of each distinct shape, timed alone, times its count per step
classes = {}
L = len(m.layers)


def add(cls, fn, count, flops, nbytes, bound_s, bound_name):
    us = window(fn, 0.05)
    classes[cls] = dict(us=us * count, flops=flops * count, bytes=nbytes * count, launches=count, bound_us=bound_s * 1e6 * count,
                        bound=bound_name)


pw = m.patch_embed.weight
P = pw.shape[2]
add("patch_embed", lambda: m.tokens(x), 1, 2.0 * M * C * 3 * P * P, x.numel() * 4 + M * C * 2,
    max(2.0 * M * C * 3 * P * P / PEAK_BF16, (x.numel() * 4 + M * C * 2) / HBM_SPEC), "max(hbm, mfma)")
add("row_stats", lambda: ops.row_stats(h0.view(M, C), 1e-6), 1 if route == "fold" else L + 1, 0.0, M * C * 2, M * C * 2 / HBM_SPEC, "hbm")


def slab_tiles():
    """32-channel tiles per workgroup, as csrc/mixer.hip picks them: 4 where one image x 128 channels fits the LDS, else 2."""
    lds = lambda nb: max(64 * nb * (Tp + 8), 33792) + 64 * nb * (Dt + 8)  # noqa: E731
    return 4 if C % 128 == 0 and lds(4) <= 160 * 1024 else 2


n_wg = N * C // (32 * slab_tiles())
tm_flops = 4.0 * N * C * Tp * Dt
tm_stream = 2.0 * M * C * 2
tm_l2 = n_wg * 2.0 * (w1f.numel() + w2f.numel())
tm_bounds = dict(stream_hbm=tm_stream / HBM_SPEC, mfma=tm_flops / PEAK_BF16, l2_weights=tm_l2 / L2_SHARED)
tm_bound = max(tm_bounds, key=tm_bounds.get)
add("token_mix", fused, L, tm_flops, tm_stream, tm_bounds[tm_bound], tm_bound)
y1, rows = fused()
y1 = y1.view(M, C)
if route == "fold":
    add("ln_stats_finalize", lambda: ops.ln_stats_finalize(rows, C, 1e-6), 2 * L, 0.0, rows.numel() * 4, rows.numel() * 4 / HBM_SPEC, "hbm")
    st = ops.ln_stats_finalize(rows, C, l.norm2.eps)
    l1, l2 = cm.linear1, cm.linear2
    wl, s, c = derived(cm, "l1_ln", (l1.weight, l1.bias, l.norm2.weight, l.norm2.bias), lambda: _fold_ln(l1.weight, l1.bias, l.norm2))
    fc1 = lambda: ops.linear(y1, wl, c, act="gelu", ln_stats=st, ln_s=s)  # noqa: E731
    hh = fc1()
    fc2 = lambda: ops.linear(hh, l2.weight, _f32(l2, "b", l2.bias), resid=y1, want_row_stats=True)  # noqa: E731
else:
    n2 = l.norm2
    add("layernorm", lambda: ops.layernorm(y1, _f32(n2, "g", n2.weight), _f32(n2, "b", n2.bias), n2.eps), L, 0.0, 2.0 * M * C * 2,
        2.0 * M * C * 2 / HBM_SPEC, "hbm")
    tt = ops.layernorm(y1, _f32(n2, "g", n2.weight), _f32(n2, "b", n2.bias), n2.eps)
    l1, l2 = cm.linear1, cm.linear2
    fc1 = lambda: ops.linear(tt, l1.weight, _f32(l1, "b", l1.bias), act="gelu")  # noqa: E731
    hh = fc1()
    fc2 = lambda: ops.linear(hh, l2.weight, _f32(l2, "b", l2.bias), resid=y1)  # noqa: E731
gf = 2.0 * M * C * hid
add("channel_fc1_gelu", fc1, L, gf, (M * C + C * hid + M * hid) * 2, gf / PEAK_BF16, "mfma")
add("channel_fc2_resid", fc2, L, gf, (M * hid + C * hid + 2 * M * C) * 2, gf / PEAK_BF16, "mfma")
gn, bn = _f32(m.norm, "g", m.norm.weight), _f32(m.norm, "b", m.norm.bias)
add("head_ln_mean", lambda: ops.ln_mean(ck["last"], stats, gn, bn, torch.bfloat16), 1, 0.0, M * C * 2, M * C * 2 / HBM_SPEC, "hbm")

out = {}
for k, c_ in classes.items():
    sec = c_["us"] * 1e-6
    e = dict(us_per_step=round(c_["us"], 1), launches=c_["launches"], gflop=round(c_["flops"] / 1e9, 2), mbytes=round(c_["bytes"] / 1e6, 1),
             tb_per_s=round(c_["bytes"] / sec / 1e12, 3), bound=c_["bound"], bound_us=round(c_["bound_us"], 1),
             frac_of_bound=round(c_["bound_us"] / c_["us"], 3))
    if c_["flops"]:
        e["tflop_per_s"] = round(c_["flops"] / sec / 1e12, 1)
    out[k] = e
res = {
    "tool": "mixer_bench", "model": f"Mixer-{args.tag} bf16 (bf16 residual stream)", "batch": B, "side": S, "tokens": T, "route": route,
    "img_per_s": round(B / (t_model * 1e-6), 1), "ms_per_step": round(t_model / 1e3, 3),
    "yardstick_a_pytorch_bf16": {"img_per_s": round(B / (t_ref * 1e-6), 1), "ms_per_step": round(t_ref / 1e3, 3), "rel_l2_vs_hip": round(err, 5)},
    "speedup_vs_yardstick_a": round(t_ref / t_model, 3),
    "yardstick_b_token_mixing_half": {"rounds": rounds, "rel_l2_composed_vs_fused": round(err_b, 5),
                                      "composed": "layernorm + transposing copy + 2 x linear (K, N padded to %d) + transposing add" % Kp},
    "token_mix_bounds_us": {k: round(v * 1e6, 1) for k, v in tm_bounds.items()}, "token_mix_workgroups": n_wg,
    "sum_of_kernel_classes_ms": round(sum(c_["us"] for c_ in classes.values()) / 1e3, 3), "kernels": out,
    "bounds": {"bf16_mfma_flop_s": PEAK_BF16, "hbm_spec_b_s": HBM_SPEC, "l2_shared_rows_b_s": L2_SHARED},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res), flush=True)
