"""Synthetic facebookresearch/detr checkpoint (reference loader: pytorch_models/image/detr.py, load_facebook_state_dict), built
from geometry in the upstream layout - torchvision ResNet names under `backbone.0.body` (conv1 / bn1, layerN.B.convK / bnK,
`downsample.0 / .1` on the first block of a stage), nn.MultiheadAttention's packed `in_proj_weight` / `in_proj_bias`, `norm2`
meaning the MLP norm in the encoder and the cross-attention norm in the decoder, `query_embed.weight` - with values from
synthweights.synth_tensor keyed by the upstream name, so the golden generator (reference loader) and the tests (this package's
loader) read identical inputs.  One key the loader never names rides along, as in a real file."""
import torch

from synthweights import synth_tensor

VARIANTS = dict(resnet50=[3, 4, 6, 3], resnet101=[3, 4, 23, 3])


def facebook_detr(backbone_layers, seed=0, d_model=256, n_classes=91, n_queries=100) -> dict:
    sd = {}

    def put(key, shape):
        v = synth_tensor("ckpt:" + key, shape, seed)
        if key.endswith("running_var"):
            v = v.abs() + 0.5
        sd[key] = v

    def conv(prefix, cout, cin, k):
        put(f"{prefix}.weight", (cout, cin, k, k))

    def bn(prefix, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            put(f"{prefix}.{leaf}", (c,))

    def linear(prefix, cout, cin):
        put(f"{prefix}.weight", (cout, cin))
        put(f"{prefix}.bias", (cout,))

    def norm(prefix, c):
        put(f"{prefix}.weight", (c,))
        put(f"{prefix}.bias", (c,))

    def mha(prefix, d):
        put(f"{prefix}.in_proj_weight", (3 * d, d))
        put(f"{prefix}.in_proj_bias", (3 * d,))
        linear(f"{prefix}.out_proj", d, d)

    body = "backbone.0.body"
    conv(f"{body}.conv1", 64, 3, 7)
    bn(f"{body}.bn1", 64)
    cin = 64
    for si, nb in enumerate(backbone_layers):
        cout = 256 << si
        mid = cout // 4
        for bi in range(nb):
            pre = f"{body}.layer{si + 1}.{bi}"
            conv(f"{pre}.conv1", mid, cin, 1)
            bn(f"{pre}.bn1", mid)
            conv(f"{pre}.conv2", mid, mid, 3)
            bn(f"{pre}.bn2", mid)
            conv(f"{pre}.conv3", cout, mid, 1)
            bn(f"{pre}.bn3", cout)
            if bi == 0:
                conv(f"{pre}.downsample.0", cout, cin, 1)
                bn(f"{pre}.downsample.1", cout)
            cin = cout
    put("input_proj.weight", (d_model, cin, 1, 1))
    put("input_proj.bias", (d_model,))
    put("query_embed.weight", (n_queries, d_model))
    for kind in ("encoder", "decoder"):
        for li in range(6):
            pre = f"transformer.{kind}.layers.{li}"
            mha(f"{pre}.self_attn", d_model)
            norm(f"{pre}.norm1", d_model)
            if kind == "decoder":
                mha(f"{pre}.multihead_attn", d_model)
                norm(f"{pre}.norm3", d_model)
            norm(f"{pre}.norm2", d_model)
            linear(f"{pre}.linear1", 8 * d_model, d_model)
            linear(f"{pre}.linear2", d_model, 8 * d_model)
    norm("transformer.decoder.norm", d_model)
    linear("class_embed", n_classes + 1, d_model)
    linear("bbox_embed.layers.0", d_model, d_model)
    linear("bbox_embed.layers.1", d_model, d_model)
    linear("bbox_embed.layers.2", 4, d_model)
    sd["backbone.0.body.fc.weight"] = torch.zeros(8, 8)  # torchvision's classifier head: present upstream, never loaded
    return sd
