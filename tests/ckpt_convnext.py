"""Synthetic facebookresearch/ConvNeXt checkpoint (the "model" entry of convnext_*_22k_224.pth; reference loader:
pytorch_models/image/convnext.py, load_facebook_state_dict), built from geometry with values from synthweights.synth_tensor keyed by
the upstream key, so the golden generator (reference loader) and the tests (this package's loader) read identical inputs.  It
carries the classifier `head.*` that the loader ignores."""
from synthweights import synth_tensor

VARIANTS = dict(
    atto=(40, (2, 2, 6, 2)),
    femto=(48, (2, 2, 6, 2)),
    pico=(64, (2, 2, 6, 2)),
    nano=(80, (2, 2, 8, 2)),
    tiny=(96, (3, 3, 9, 3)),
    small=(96, (3, 3, 27, 3)),
    base=(128, (3, 3, 27, 3)),
    large=(192, (3, 3, 27, 3)),
    xlarge=(256, (3, 3, 27, 3)),
    huge=(352, (3, 3, 27, 3)),
)


def facebook_convnext(d_model, depths, n_classes=11, seed=0):
    sd = {}

    def put(k, shape):
        sd[k] = synth_tensor("ckpt:" + k, shape, seed)

    def wb(prefix, wshape, n):
        put(f"{prefix}.weight", wshape)
        put(f"{prefix}.bias", (n,))

    wb("downsample_layers.0.0", (d_model, 3, 4, 4), d_model)
    wb("downsample_layers.0.1", (d_model,), d_model)
    d = d_model
    for i, depth in enumerate(depths):
        if i > 0:
            wb(f"downsample_layers.{i}.0", (d,), d)
            wb(f"downsample_layers.{i}.1", (2 * d, d, 2, 2), 2 * d)
            d *= 2
        for j in range(depth):
            p = f"stages.{i}.{j}"
            wb(f"{p}.dwconv", (d, 1, 7, 7), d)
            wb(f"{p}.norm", (d,), d)
            wb(f"{p}.pwconv1", (4 * d, d), 4 * d)
            wb(f"{p}.pwconv2", (d, 4 * d), d)
            put(f"{p}.gamma", (d,))
    wb("norm", (d,), d)
    wb("head", (n_classes, d), n_classes)
    return sd
