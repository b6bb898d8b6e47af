"""MaxViT-T on one MI355X: img/s of the bf16 forward at batch 256, 224 x 224 on synthetic weights; the time of each kernel class
over one forward (every launch bracketed by its own HIP events, ops.LAUNCH_LOG), with its algorithmic FLOPs and bytes and their
fraction of the bound; the window-attention kernel against pm_attention_generic_bf16 on the same windows (the "before": rows
gathered into window order outside the timing); and a same-box yardstick: the same weights through plain PyTorch-ROCm ops (the
reference's arithmetic, bf16, channels_last, SDPA with the relative bias).  The yardstick lives in this tool only.  Prints one
JSON line.
    python tools/maxvit_bench.py [--variant tiny] [--batch 256] [--side 224]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.image import MaxViT  # noqa: E402
from pytorch_models.image.maxvit import _window_bias, block, grid, unblock, ungrid  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

PEAK_BF16 = 2.5e15  # FLOP/s, dense bf16 MFMA (spec)
PEAK_F32_VALU = 157.3e12  # FLOP/s, fp32 vector fma (spec)
HBM_SPEC = 8.0e12  # B/s
BOUND = dict(linear_bf16="mfma_bf16", maxvit_stem="valu_f32")

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="tiny")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--side", type=int, default=224)
args = ap.parse_args()
torch.set_grad_enabled(False)

m = MaxViT.from_google(args.variant).eval()
fill_module(m, 91)
bf16_round_(m)
m = m.to(torch.bfloat16).cuda()
B, S = args.batch, args.side
x = synth_input("mvit_bench", (B, 3, S, S), 91).cuda()


def window(fn, ms_per_call):
    """warm-up and timed windows of ~40 ms each"""
    n = max(3, int(40.0 / max(ms_per_call, 1e-3)))
    return time_us(fn, warmup=n, iters=n)


t_probe = time_us(lambda: m(x), warmup=2, iters=3) / 1e3
t_model = window(lambda: m(x), t_probe)

# ---- yardstick: the same bf16 weights through stock PyTorch-ROCm ops (channels_last), the reference's arithmetic
ref = copy.deepcopy(m).to(memory_format=torch.channels_last)
x_cl = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def ref_layer(layer, t):
    sa, ln1, ln2, mlp = layer.sa, layer.sa_norm, layer.mlp_norm, layer.mlp
    a = F.layer_norm(t, ln1.normalized_shape, ln1.weight, ln1.bias, ln1.eps)
    q, k, v = (F.linear(a, p.weight, p.bias).unflatten(-1, (sa.n_heads, 32)).transpose(-2, -3)
               for p in (sa.q_proj, sa.k_proj, sa.v_proj))
    o = F.scaled_dot_product_attention(q, k, v, _window_bias(sa.attn_bias, sa.bias_index))
    t = t + F.linear(o.transpose(-2, -3).flatten(-2), sa.out_proj.weight, sa.out_proj.bias)
    a = F.layer_norm(t, ln2.normalized_shape, ln2.weight, ln2.bias, ln2.eps)
    return t + F.linear(F.gelu(F.linear(a, mlp.linear1.weight, mlp.linear1.bias), approximate="tanh"), mlp.linear2.weight,
                        mlp.linear2.bias)


def ref_forward(imgs):
    h = nn.Sequential.forward(ref.stem, imgs)
    for stage in ref.stages:
        for blk in stage:
            t = blk.mbconv(h).permute(0, 2, 3, 1)
            t, nH, nW = block(t, 7)
            t = unblock(ref_layer(blk.block_layer, t), nH, nW, 7)
            t, nH, nW = grid(t, 7)
            t = ungrid(ref_layer(blk.grid_layer, t), nH, nW, 7)
            h = t.permute(0, 3, 1, 2)
    return F.layer_norm(F.adaptive_avg_pool2d(h, 1).flatten(1), ref.norm.normalized_shape, ref.norm.weight, ref.norm.bias,
                        ref.norm.eps)


t_ref_probe = time_us(lambda: ref_forward(x_cl), warmup=2, iters=3) / 1e3
t_ref = window(lambda: ref_forward(x_cl), t_ref_probe)
yr = ref_forward(x_cl).float()
err = float((yr - m(x).float()).norm() / yr.norm())
del ref

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
    # work per launch: (flops, bytes), or one number (bytes for the normalisations, flops for the GEMMs)
    as_bytes = name in ("layernorm",)
    flops = sum(w[0] if isinstance(w, tuple) else (0.0 if as_bytes else w) for _, _, w in recs)
    nbytes = sum(w[1] if isinstance(w, tuple) else (w if as_bytes else 0.0) for _, _, w in recs)
    e = dict(us_per_step=round(us, 1), launches=len(recs), gflop=round(flops / 1e9, 2), mbytes=round(nbytes / 1e6, 1))
    s = us * 1e-6
    bound = BOUND.get(name, "hbm")
    if bound == "mfma_bf16":
        e["frac_bf16_peak"] = round(flops / s / PEAK_BF16, 3)
    elif bound == "valu_f32":
        e["frac_f32_valu_peak"] = round(flops / s / PEAK_F32_VALU, 3)
    if nbytes:
        e["frac_hbm_spec"] = round(nbytes / s / HBM_SPEC, 3)
    kernels[name] = e

# ---- window attention vs the generic kernel on the stage shapes (bias from the stage's first block)
attn = {}
H = W = S // 2  # the stem output; each stage halves it
for si, stage in enumerate(m.stages):
    H, W = H // 2, W // 2
    d = stage[0].block_layer.sa.n_heads * 32
    nh = d // 32
    if si > 1:
        break
    bias = stage[0].block_layer.sa.window_bias()
    M = B * H * W
    qkv = synth_input(f"mvb_qkv{si}", (M, 3 * d), 91).to(torch.bfloat16).cuda()
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    nbytes = M * d * 2 * 4.0
    row = {}
    for mode in ("block", "grid"):
        us = window(lambda: ops.window_attention(q, k, v, B, H, W, nh, 7, mode, bias), 0.5)
        row[mode] = dict(us=round(us, 1), tb_per_s=round(nbytes / us / 1e6, 3), frac_hbm_spec=round(nbytes / (us * 1e-6) / HBM_SPEC, 3))
    qw = block(qkv.view(B, H, W, 3 * d), 7)[0].reshape(-1, 49, 3 * d)
    b4 = bias[None]
    us_g = window(lambda: ops.attention(qw[..., :d], qw[..., d:2 * d], qw[..., 2 * d:], nh, False, b4), 2.0)
    row["generic_bf16_window_ordered"] = dict(us=round(us_g, 1), tb_per_s=round(nbytes / us_g / 1e6, 3))
    row["speedup_block_vs_generic"] = round(us_g / row["block"]["us"], 2)
    attn[f"stage{si}"] = dict(shape=[B, H, W, d], heads=nh, algorithmic_mbytes=round(nbytes / 1e6, 1), **row)

res = {
    "tool": "maxvit_bench", "model": f"MaxViT-{args.variant} bf16 (f32 residual stream)", "batch": B, "side": S,
    "img_per_s": round(B / (t_model * 1e-6), 1), "ms_per_step": round(t_model / 1e3, 3),
    "yardstick_pytorch_channels_last": {"img_per_s": round(B / (t_ref * 1e-6), 1), "ms_per_step": round(t_ref / 1e3, 3),
                                        "rel_l2_vs_hip": round(err, 5)},
    "speedup_vs_yardstick": round(t_ref / t_model, 3),
    "window_attention": attn,
    "kernels_one_forward_event_timed": kernels,
    "bounds": {"bf16_mfma_flop_s": PEAK_BF16, "hbm_spec_b_s": HBM_SPEC, "f32_valu_flop_s": PEAK_F32_VALU},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res), flush=True)
