"""End-to-end bf16 tolerance of DETR's HIP form, derived on the CPU (no GPU, no kernel): the CPU form run with every tensor the
HIP form STORES rounded to bf16 - folded conv weights, every convolution / GEMM / attention / LayerNorm output, P inside the
attention stays fp32 - against the unrounded CPU form on the same bf16-rounded weights, rel-L2 per checkpoint.
tests/test_hip_detr.py allows 2 x these figures (other summation order, bf16 P); DESIGN.md section 12 quotes them.

    python tools/detr_tolerance.py            # small @ 224 x 225 and resnet50 @ 224 x 224, the test's two cases
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-models_amd"))
from pytorch_models.image import DETR  # noqa: E402
from synthweights import bf16_round_, fill_module, synth_input  # noqa: E402

torch.set_grad_enabled(False)
SEED, SKIP = 131, ("window", "filters", "freqs")


def r(t):
    return t.to(torch.bfloat16).float()


def conv_bn(x, conv, bn, relu, resid=None):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    y = F.conv2d(x, r(conv.weight * s[:, None, None, None]), bn.bias - bn.running_mean * s, conv.stride, conv.padding)
    if resid is not None:
        y = y + resid
    return r(F.relu(y) if relu else y)


def bottleneck(b, x):
    q = b.residual
    u = conv_bn(x, q[0], q[1], True)
    t = conv_bn(u, q[3], q[4], True)
    sc = x if isinstance(b.shortcut, torch.nn.Identity) else conv_bn(x, b.shortcut[0], b.shortcut[1], False)
    return conv_bn(t, q[6], q[7], True, resid=sc)


def attend(m, q_in, k_in, v_in, q_emb, k_emb):
    """Projections as the HIP form makes them: x W^T + (W emb + b) in fp32, one rounding."""
    def proj(p, x, emb):
        y = F.linear(x, p.weight) + (F.linear(emb, p.weight, p.bias) if emb is not None else p.bias)
        return r(y).unflatten(-1, (m.n_heads, m.head_dim)).transpose(-2, -3)

    o = F.scaled_dot_product_attention(proj(m.q_proj, q_in, q_emb), proj(m.k_proj, k_in, k_emb), proj(m.v_proj, v_in, None))
    return r(o.transpose(-2, -3).flatten(-2))


def ln(n, x):
    return r(F.layer_norm(x, n.normalized_shape, n.weight, n.bias, n.eps))


def mlp_norm(layer, x):
    u = r(F.relu(F.linear(x, layer.mlp.linear1.weight, layer.mlp.linear1.bias)))
    return ln(layer.mlp_norm, r(F.linear(u, layer.mlp.linear2.weight, layer.mlp.linear2.bias) + x))


def out_res(m, o, x):
    return r(F.linear(o, m.out_proj.weight, m.out_proj.bias) + x)


def rounded_forward(m, x):
    out = {}
    st = m.backbone.stem
    s = st[1].weight / torch.sqrt(st[1].running_var + st[1].eps)
    h = F.relu(F.conv2d(x, st[0].weight * s[:, None, None, None], st[1].bias - st[1].running_mean * s, 2, 3))
    h = F.max_pool2d(r(h), 3, 2, 1)
    out["stem"] = h
    for i, stage in enumerate(m.backbone.stages):
        for b in stage:
            h = bottleneck(b, h)
        out[f"stage{i}"] = h
    h = r(m.input_proj(h))
    pos = m.pos_embed(h.shape[-2], h.shape[-1]).flatten(0, 1)
    t = h.flatten(-2).transpose(-1, -2)
    out["input_proj"] = t
    for l in m.encoder:
        t = ln(l.sa_norm, out_res(l.sa, attend(l.sa, t, t, t, pos, pos), t))
        t = mlp_norm(l, t)
    out["memory"] = t
    qe = m.query_embed
    q = torch.zeros(x.shape[0], *qe.shape)
    for l in m.decoder:
        q = ln(l.sa_norm, out_res(l.sa, attend(l.sa, q, q, q, qe, qe), q))
        q = ln(l.ca_norm, out_res(l.ca, attend(l.ca, q, t, t, qe, pos), q))
        q = mlp_norm(l, q)
    q = ln(m.norm, q)
    out["logits"] = m.classifier(q)
    bh = m.box_head
    out["boxes"] = bh[4](r(F.relu(bh[2](r(F.relu(bh[0](q))))))).sigmoid()
    return out


def plain_forward(m, x):
    out = {}
    h = m.backbone.stem(x)
    out["stem"] = h
    for i, stage in enumerate(m.backbone.stages):
        h = stage(h)
        out[f"stage{i}"] = h
    h = m.input_proj(h)
    pos = m.pos_embed(h.shape[-2], h.shape[-1]).flatten(0, 1)
    t = h.flatten(-2).transpose(-1, -2)
    out["input_proj"] = t
    for l in m.encoder:
        t = l(t, pos)
    out["memory"] = t
    out["logits"], out["boxes"] = m(x)
    return out


def build(name):
    m = (DETR([1, 1, 1, 1]) if name == "small" else DETR.from_facebook("resnet50")).eval()
    fill_module(m, SEED, skip=SKIP)
    bf16_round_(m)
    shape = (2, 3, 224, 225) if name == "small" else (2, 3, 224, 224)
    return m, synth_input(f"detr_{name}_x", shape, SEED)


if __name__ == "__main__":
    for name in ("small", "r50"):
        m, x = build(name)
        want, got = plain_forward(m, x), rounded_forward(m, x)
        for k in want:
            print(f"{name:6s} {k:11s} rel-L2 {float((got[k] - want[k]).norm() / want[k].norm()):.5f}")
