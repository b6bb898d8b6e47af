"""ConvNeXt-T on one MI355X: img/s of the bf16 forward at batch 256, 224 x 224 on synthetic weights, the time of each kernel class
(each launch timed on its own over a warmed window of tens of ms, tools/_timing.py, times its count per step), its algorithmic
FLOPs and bytes and their fraction of the bound, and a same-box yardstick: the same weights through plain PyTorch-ROCm ops
(the reference's nn.Sequential arithmetic, bf16, channels_last).  The yardstick lives in this tool only.  Prints one JSON line.
    python tools/convnext_bench.py [--variant tiny] [--batch 256] [--side 224]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-models_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

from _timing import time_us  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402
from pytorch_models.image import ConvNeXt  # noqa: E402
from pytorch_models.image.convnext import _gemm  # noqa: E402
from pytorch_models.transformer import _f32  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

PEAK_BF16 = 2.5e15  # FLOP/s, dense bf16 MFMA (spec)
PEAK_F32_VALU = 157.3e12  # FLOP/s, fp32 vector fma (spec)
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # B/s: spec, and the measured device-to-device copy rate of this box type

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="tiny")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--side", type=int, default=224)
args = ap.parse_args()
torch.set_grad_enabled(False)

m = ConvNeXt.from_facebook(args.variant).eval()
fill_module(m, 91)
bf16_round_(m)
m = m.to(torch.bfloat16).cuda()
B, S = args.batch, args.side
x = synth_input("cnx_bench", (B, 3, S, S), 91).cuda()


def window(fn, ms_per_call):
    """warm-up and timed windows of ~40 ms each"""
    n = max(3, int(40.0 / max(ms_per_call, 1e-3)))
    return time_us(fn, warmup=n, iters=n)


t_probe = time_us(lambda: m(x), warmup=2, iters=3) / 1e3
t_model = window(lambda: m(x), t_probe)

# yardstick: the same bf16 weights through stock PyTorch-ROCm modules (channels_last), the reference's arithmetic
ref = copy.deepcopy(m).to(memory_format=torch.channels_last)
x_cl = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def ref_forward(imgs):
    h = nn.Sequential.forward(ref.stem, imgs)
    for stage in ref.stages:
        h = stage[0](h)
        for blk in list(stage)[1:]:
            h = h + nn.Sequential.forward(blk, h) * blk.gamma
    return ref.norm(ref.pool(h))


t_ref_probe = time_us(lambda: ref_forward(x_cl), warmup=2, iters=3) / 1e3
t_ref = window(lambda: ref_forward(x_cl), t_ref_probe)
err = float((ref_forward(x_cl).float() - m(x).float()).norm() / ref_forward(x_cl).float().norm())

# per kernel class: one launch of each distinct shape, timed alone, times its count per step
classes = {}


def add(cls, fn, count, flops, nbytes, bound):
    us = window(fn, 0.05)
    c = classes.setdefault(cls, dict(us=0.0, flops=0.0, bytes=0.0, launches=0, bound=bound))
    c["us"] += us * count
    c["flops"] += flops * count
    c["bytes"] += nbytes * count
    c["launches"] += count


ln = m.stem[2]
stem_args = (x, m._stem_w(), _f32(m.stem[0], "b", m.stem[0].bias), _f32(ln, "g", ln.weight), _f32(ln, "b", ln.bias), ln.eps)
h4 = ops.convnext_stem(*stem_args)
N, H, W, C = h4.shape
add("stem", lambda: ops.convnext_stem(*stem_args), 1, 2.0 * 48 * N * H * W * C, x.numel() * 4 + h4.numel() * 4, "valu_f32")
h = h4.view(-1, C)
per_stage = {}
for si, stage in enumerate(m.stages):
    if si > 0:
        ds = stage[0]
        w = m._down_w(ds)
        g0, b0 = _f32(ds[0], "g", ds[0].weight), _f32(ds[0], "b", ds[0].bias)
        hv = h.view(N, H, W, C)
        t = ops.ln_space_to_depth(hv, g0, b0, ds[0].eps, w.dtype)
        bd = _f32(ds[2], "b", ds[2].bias)
        add("downsample_ln_s2d", lambda: ops.ln_space_to_depth(hv, g0, b0, ds[0].eps, w.dtype), 1, 0.0,
            h.numel() * 4 + t.numel() * 2, "hbm")
        h = _gemm(t, w, bd)
        add("downsample_gemm", lambda: _gemm(t, w, bd), 1, 2.0 * t.shape[0] * w.shape[0] * 4 * C,
            t.numel() * 2 + w.numel() * 2 + h.numel() * 4, "mfma_bf16")
        H, W, C = H // 2, W // 2, w.shape[0]
    blocks = list(stage)[1:]
    blk = blocks[0]
    wdw, w1, b1, w2, b2 = blk._packed()
    dw, bl = blk[1], blk[3]
    hv = h.view(N, H, W, C)
    dargs = (hv, wdw, _f32(dw, "b", dw.bias), _f32(bl, "g", bl.weight), _f32(bl, "b", bl.bias), bl.eps, torch.bfloat16)
    t = ops.dwconv7_ln(*dargs)
    M = N * H * W
    add(f"dwconv_ln_stage{si}", lambda: ops.dwconv7_ln(*dargs), len(blocks), 2.0 * 49 * M * C, M * C * 4 + t.numel() * 2, "hbm")
    u = _gemm(t, w1, b1, act="gelu", out_dtype=torch.bfloat16)
    add("fc1_gelu", lambda: _gemm(t, w1, b1, act="gelu", out_dtype=torch.bfloat16), len(blocks), 2.0 * M * 4 * C * C,
        t.numel() * 2 + w1.numel() * 2 + u.numel() * 2, "mfma_bf16")
    add("fc2_resid", lambda: _gemm(u, w2, b2, resid=h), len(blocks), 2.0 * M * C * 4 * C,
        u.numel() * 2 + w2.numel() * 2 + 2 * M * C * 4, "mfma_bf16")
    per_stage[si] = dict(shape=[N, H, W, C], blocks=len(blocks))
    for b_ in blocks:
        h = b_.run(h, N, H, W)
gn, bn = _f32(m.norm, "g", m.norm.weight), _f32(m.norm, "b", m.norm.bias)
hv = h.view(N, H * W, C)
add("head_mean_ln", lambda: ops.mean_ln(hv, gn, bn, m.norm.eps, torch.bfloat16), 1, 0.0, h.numel() * 4 + N * C * 2, "hbm")

out = {}
for k, c in classes.items():
    s = c["us"] * 1e-6
    e = dict(us_per_step=round(c["us"], 1), launches=c["launches"], gflop=round(c["flops"] / 1e9, 2), mbytes=round(c["bytes"] / 1e6, 1))
    e["tb_per_s"] = round(c["bytes"] / s / 1e12, 3)
    if c["bound"] == "hbm":
        e["frac_hbm_spec"] = round(c["bytes"] / s / HBM_SPEC, 3)
        e["frac_hbm_copy"] = round(c["bytes"] / s / HBM_COPY, 3)
    elif c["bound"] == "mfma_bf16":
        e["tflop_per_s"] = round(c["flops"] / s / 1e12, 1)
        e["frac_bf16_peak"] = round(c["flops"] / s / PEAK_BF16, 3)
    else:
        e["tflop_per_s"] = round(c["flops"] / s / 1e12, 2)
        e["frac_f32_valu_peak"] = round(c["flops"] / s / PEAK_F32_VALU, 3)
        e["frac_hbm_spec"] = round(c["bytes"] / s / HBM_SPEC, 3)
    out[k] = e
res = {
    "tool": "convnext_bench", "model": f"ConvNeXt-{args.variant} bf16 (f32 residual stream)", "batch": B, "side": S,
    "img_per_s": round(B / (t_model * 1e-6), 1), "ms_per_step": round(t_model / 1e3, 3),
    "yardstick_pytorch_channels_last": {"img_per_s": round(B / (t_ref * 1e-6), 1), "ms_per_step": round(t_ref / 1e3, 3),
                                        "rel_l2_vs_hip": round(err, 5)},
    "speedup_vs_yardstick": round(t_ref / t_model, 3),
    "sum_of_kernel_classes_ms": round(sum(c["us"] for c in classes.values()) / 1e3, 3),
    "stages": per_stage, "kernels": out,
    "bounds": {"bf16_mfma_flop_s": PEAK_BF16, "hbm_spec_b_s": HBM_SPEC, "hbm_copy_measured_b_s": HBM_COPY, "f32_valu_flop_s": PEAK_F32_VALU},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res), flush=True)
