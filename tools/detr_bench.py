"""DETR-R50 on one MI355X: img/s of the bf16 forward at batch 16, 800 x 1216 (25 x 38 = 950 tokens) on synthetic weights,
alternating in one process with a same-box yardstick - the same weights through stock PyTorch-ROCm (nn.Conv2d / BatchNorm2d
channels_last, F.linear, F.scaled_dot_product_attention, bf16; the reference's arithmetic).  Then the time of each kernel class
over one forward (every launch bracketed by its own HIP events, ops.LAUNCH_LOG) with its algorithmic FLOPs and share of the bound;
pm_conv_bf16 at the four stage shapes against F.conv2d (MIOpen) on the same tensors; pm_attention_hd32_bf16 against
pm_attention_generic_bf16 on the encoder and cross-attention shapes.  The yardstick lives in this tool only.  Prints one JSON line.
    python tools/detr_bench.py [--batch 16] [--height 800] [--width 1216] [--rounds 3]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.image import DETR  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

PEAK_BF16 = 2.5e15  # FLOP/s, dense bf16 MFMA (spec)
PEAK_F32_VALU = 157.3e12  # FLOP/s, fp32 vector fma (spec)
HBM_SPEC = 8.0e12  # B/s
BOUND = dict(linear_bf16="mfma_bf16", conv_bf16="mfma_bf16", attention_hd32="mfma_bf16", resnet_stem="valu_f32")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--height", type=int, default=800)
ap.add_argument("--width", type=int, default=1216)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--profile-only", action="store_true", help="warm up and run three forwards, nothing else (for a kernel trace)")
args = ap.parse_args()
torch.set_grad_enabled(False)

m = DETR.from_facebook("resnet50").eval()
fill_module(m, 131, skip=("window", "filters", "freqs"))
bf16_round_(m)
m = m.to(torch.bfloat16).cuda()
B, Hi, Wi = args.batch, args.height, args.width
x = synth_input("detr_bench", (B, 3, Hi, Wi), 131).cuda()

if args.profile_only:
    for _ in range(5):
        m(x)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "detr_bench", "profile_only": True}))
    sys.exit(0)


def window(fn, ms_per_call, target_ms=400.0):
    n = max(3, int(target_ms / max(ms_per_call, 1e-3)))
    return time_us(fn, warmup=max(2, n // 2), iters=n)


# ---- yardstick: the same bf16 weights through stock PyTorch-ROCm ops
ref = copy.deepcopy(m).to(memory_format=torch.channels_last)
x_cl = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
pos_ref = m.pos_embed.table((Hi + 31) // 32, (Wi + 31) // 32).to(torch.bfloat16)


def ref_mha(sa, q, k, v):
    split = lambda t: t.unflatten(-1, (sa.n_heads, sa.head_dim)).transpose(-2, -3)  # noqa: E731
    o = F.scaled_dot_product_attention(split(F.linear(q, sa.q_proj.weight, sa.q_proj.bias)), split(F.linear(k, sa.k_proj.weight, sa.k_proj.bias)),
                                       split(F.linear(v, sa.v_proj.weight, sa.v_proj.bias)))
    return F.linear(o.transpose(-2, -3).flatten(-2), sa.out_proj.weight, sa.out_proj.bias)


def ref_ln(n, t):
    return F.layer_norm(t, n.normalized_shape, n.weight, n.bias, n.eps)


def ref_mlp(l, t):
    return F.linear(F.relu(F.linear(t, l.mlp.linear1.weight, l.mlp.linear1.bias)), l.mlp.linear2.weight, l.mlp.linear2.bias)


def ref_forward(imgs):
    h = torch.nn.Sequential.forward(ref.backbone.stem, imgs)
    for stage in ref.backbone.stages:
        for b in stage:
            h = F.relu(torch.nn.Sequential.forward(b.shortcut, h) + torch.nn.Sequential.forward(b.residual, h)) \
                if not isinstance(b.shortcut, torch.nn.Identity) else F.relu(h + torch.nn.Sequential.forward(b.residual, h))
    h = F.conv2d(h, ref.input_proj.weight, ref.input_proj.bias)
    t = h.flatten(-2).transpose(-1, -2)
    for l in ref.encoder:
        qk = t + pos_ref
        t = ref_ln(l.sa_norm, t + ref_mha(l.sa, qk, qk, t))
        t = ref_ln(l.mlp_norm, t + ref_mlp(l, t))
    qe = ref.query_embed
    q = torch.zeros_like(qe)
    for l in ref.decoder:
        qk = q + qe
        q = ref_ln(l.sa_norm, q + ref_mha(l.sa, qk, qk, q))
        q = ref_ln(l.ca_norm, q + ref_mha(l.ca, q + qe, t + pos_ref, t))
        q = ref_ln(l.mlp_norm, q + ref_mlp(l, q))
    q = ref_ln(ref.norm, q)
    return F.linear(q, ref.classifier.weight, ref.classifier.bias), torch.nn.Sequential.forward(ref.box_head, q).sigmoid()


t_probe = time_us(lambda: m(x), warmup=2, iters=3) / 1e3
t_ref_probe = time_us(lambda: ref_forward(x_cl), warmup=2, iters=3) / 1e3
hip_ms, ref_ms = [], []
for _ in range(args.rounds):  # alternate: both see the same machine state over the run
    hip_ms.append(window(lambda: m(x), t_probe) / 1e3)
    ref_ms.append(window(lambda: ref_forward(x_cl), t_ref_probe) / 1e3)
yl, yb = ref_forward(x_cl)
gl, gb = m(x)
err = dict(logits=float((yl.float() - gl).norm() / yl.float().norm()), boxes=float((yb.float() - gb).norm() / yb.float().norm()))
t_model, t_ref = min(hip_ms), min(ref_ms)

# ---- per kernel class over one forward (events around every launch)
for _ in range(2):
    m(x)
ops.LAUNCH_LOG = {}
m(x)
torch.cuda.synchronize()
log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None
kernels = {}
for name, recs in log.items():
    us = sum(e0.elapsed_time(e1) for e0, e1, _ in recs) * 1e3
    as_bytes = name in ("layernorm",)
    flops = sum(w[0] if isinstance(w, tuple) else (0.0 if as_bytes else w) for _, _, w in recs)
    nbytes = sum(w[1] if isinstance(w, tuple) else (w if as_bytes else 0.0) for _, _, w in recs)
    e = dict(us_per_step=round(us, 1), launches=len(recs), gflop=round(flops / 1e9, 2), mbytes=round(nbytes / 1e6, 1))
    s = us * 1e-6
    bound = BOUND.get(name, "hbm")
    if bound == "mfma_bf16":
        e["frac_bf16_peak"] = round(flops / s / PEAK_BF16, 4)
    elif bound == "valu_f32":
        e["frac_f32_valu_peak"] = round(flops / s / PEAK_F32_VALU, 4)
    if nbytes:
        e["frac_hbm_spec"] = round(nbytes / s / HBM_SPEC, 4)
    kernels[name] = e
del ref
torch.cuda.empty_cache()

# ---- pm_conv_bf16 at the four stage shapes (the 3 x 3 of a non-first block) against F.conv2d on the same tensors
convs = {}
h0, w0 = ((Hi - 1) // 2 + 1 - 1) // 2 + 1, ((Wi - 1) // 2 + 1 - 1) // 2 + 1
for si in range(4):
    c = 64 << si
    hh, ww = ((h0 - 1) >> si) + 1, ((w0 - 1) >> si) + 1
    xa = synth_input(f"db_conv_x{si}", (B, hh, ww, c), 1).to(torch.bfloat16).cuda()
    wa = synth_input(f"db_conv_w{si}", (c, 3, 3, c), 2, scale=(9 * c) ** -0.5).to(torch.bfloat16).cuda()
    ba = synth_input(f"db_conv_b{si}", (c,), 3).cuda()
    x_nchw = xa.permute(0, 3, 1, 2)  # channels_last view of the same memory
    w_nchw = wa.permute(0, 3, 1, 2)
    bb = ba.to(torch.bfloat16)
    flops = 2.0 * B * hh * ww * c * 9 * c
    us = window(lambda: ops.conv_bf16(xa, wa, ba, 1, relu=True), 1.0, 100.0)
    us_t = window(lambda: F.relu(F.conv2d(x_nchw, w_nchw, bb, 1, 1)), 1.0, 100.0)
    d = float((ops.conv_bf16(xa, wa, ba, 1, relu=True).float() - F.relu(F.conv2d(x_nchw, w_nchw, bb, 1, 1)).permute(0, 2, 3, 1).float()).abs().max())
    convs[f"stage{si}_3x3"] = dict(shape=[B, hh, ww, c], gflop=round(flops / 1e9, 1), us=round(us, 1),
                                    frac_bf16_peak=round(flops / (us * 1e-6) / PEAK_BF16, 4), us_torch_conv2d_relu=round(us_t, 1),
                                    speedup_vs_torch=round(us_t / us, 3), max_abs_diff=round(d, 4))

# ---- pm_attention_hd32_bf16 against pm_attention_generic_bf16
attn = {}
HW = ((Hi + 31) // 32) * ((Wi + 31) // 32)
for Lq, Lk in ((HW, HW), (100, HW)):
    q = synth_input("db_q", (B, Lq, 256), 4).to(torch.bfloat16).cuda()
    kv = synth_input("db_kv", (B, Lk, 512), 5).to(torch.bfloat16).cuda()
    k, v = kv[..., :256], kv[..., 256:]
    flops = 4.0 * B * 8 * Lq * Lk * 32
    us = window(lambda: ops.attention_hd32(q, k, v, 8), 0.3, 100.0)
    us_g = window(lambda: ops.attention(q, k, v, 8), 2.0, 100.0)
    d = float((ops.attention_hd32(q, k, v, 8).float() - ops.attention(q, k, v, 8).float()).abs().max())
    attn[f"{Lq}x{Lk}"] = dict(B=B, heads=8, us=round(us, 1), frac_bf16_peak=round(flops / (us * 1e-6) / PEAK_BF16, 4),
                               us_generic_bf16=round(us_g, 1), speedup_vs_generic=round(us_g / us, 2), max_abs_diff=round(d, 5))

res = {
    "tool": "detr_bench", "model": "DETR-R50 bf16", "batch": B, "image": [Hi, Wi], "tokens": HW,
    "img_per_s": round(B / (t_model * 1e-3), 2), "ms_per_step": round(t_model, 3), "ms_per_step_rounds": [round(t, 3) for t in hip_ms],
    "yardstick_pytorch_channels_last_sdpa": {"img_per_s": round(B / (t_ref * 1e-3), 2), "ms_per_step": round(t_ref, 3),
                                             "ms_per_step_rounds": [round(t, 3) for t in ref_ms],
                                             "rel_l2_vs_hip": {k: round(v, 5) for k, v in err.items()}},
    "speedup_vs_yardstick": round(t_ref / t_model, 3),
    "conv_bf16_vs_torch": convs,
    "attention_hd32_vs_generic": attn,
    "kernels_one_forward_event_timed": kernels,
    "bounds": {"bf16_mfma_flop_s": PEAK_BF16, "hbm_spec_b_s": HBM_SPEC, "f32_valu_flop_s": PEAK_F32_VALU},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res), flush=True)
