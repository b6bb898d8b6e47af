"""Synthetic google-research/maxvit TF checkpoint reader (reference loader: pytorch_models/image/maxvit.py,
load_google_state_dict), built from geometry in the upstream TF layouts - (kh, kw, in, out) kernels, (kh, kw, C, 1) depthwise
kernels, (d, H, 32) q / k / v and (H, 32, d) o weights, (H, 13, 13) relative biases - with values from synthweights.synth_tensor
keyed by the TF variable name, so the golden generator (reference loader) and the tests (this package's loader) read identical
inputs.  Each variable comes with its ExponentialMovingAverage copy (the one the loader reads) and the raw one (ignored), plus an
optimizer slot the loader never names."""
import numpy as np

from synthweights import synth_tensor

VARIANTS = dict(
    tiny=(64, [2, 2, 5, 2], [64, 128, 256, 512]),
    small=(64, [2, 2, 5, 2], [96, 192, 384, 768]),
    base=(64, [2, 6, 14, 2], [96, 192, 384, 768]),
    large=(128, [2, 6, 14, 2], [128, 256, 512, 1024]),
    xlarge=(192, [2, 6, 14, 2], [192, 384, 768, 1536]),
)


class Reader:
    """The two methods of tf.train.load_checkpoint's reader that the loader uses."""

    def __init__(self, tensors: dict):
        self.tensors = tensors

    def get_variable_to_shape_map(self):
        return {k: list(v.shape) for k, v in self.tensors.items()}

    def get_tensor(self, name):
        return self.tensors[name]


def google_maxvit(stem_dim, n_blocks, dims, seed=0, window=7) -> Reader:
    t = {}

    def put(name, shape):
        key = f"maxvit/{name}"
        v = synth_tensor("ckpt:" + key, shape, seed).numpy()
        if name.endswith("moving_variance"):
            v = np.abs(v) + 0.5
        t[key + "/ExponentialMovingAverage"] = v
        t[key] = np.zeros(shape, np.float32)

    def conv(prefix, k, cin, cout, bias=True):
        put(f"{prefix}/kernel", (k, k, cin, cout))
        if bias:
            put(f"{prefix}/bias", (cout,))

    def norm(prefix, c, bn=False):
        put(f"{prefix}/gamma", (c,))
        put(f"{prefix}/beta", (c,))
        if bn:
            put(f"{prefix}/moving_mean", (c,))
            put(f"{prefix}/moving_variance", (c,))

    conv("stem/conv_0", 3, 3, stem_dim)
    norm("stem/norm_0", stem_dim, bn=True)
    conv("stem/conv_1", 3, stem_dim, stem_dim)
    cin = stem_dim
    for si, (nb, d) in enumerate(zip(n_blocks, dims)):
        for bi in range(nb):
            p = f"block_{si:02d}_{bi:02d}"
            hid = 4 * d
            norm(f"{p}/mbconv/pre_norm", cin, bn=True)
            conv(f"{p}/mbconv/expand_conv", 1, cin, hid, bias=False)
            norm(f"{p}/mbconv/expand_norm", hid, bn=True)
            put(f"{p}/mbconv/depthwise_conv/depthwise_kernel", (3, 3, hid, 1))
            norm(f"{p}/mbconv/depthwise_norm", hid, bn=True)
            conv(f"{p}/mbconv/se/reduce_conv2d", 1, hid, hid // 16)
            conv(f"{p}/mbconv/se/expand_conv2d", 1, hid // 16, hid)
            conv(f"{p}/mbconv/shrink_conv", 1, hid, d)
            if cin != d:
                conv(f"{p}/mbconv/shortcut_conv", 1, cin, d)
            H = d // 32
            for sfx in ("", "_1"):
                norm(f"{p}/attn_layer_norm{sfx}", d)
                put(f"{p}/attention{sfx}/relative_bias", (H, 2 * window - 1, 2 * window - 1))
                for n in "qkv":
                    put(f"{p}/attention{sfx}/{n}/weight", (d, H, 32))
                    put(f"{p}/attention{sfx}/{n}/bias", (H, 32))
                put(f"{p}/attention{sfx}/o/weight", (H, 32, d))
                put(f"{p}/attention{sfx}/o/bias", (d,))
                norm(f"{p}/ffn_layer_norm{sfx}", d)
                put(f"{p}/ffn{sfx}/expand_dense/weight", (d, 4 * d))
                put(f"{p}/ffn{sfx}/expand_dense/bias", (4 * d,))
                put(f"{p}/ffn{sfx}/shrink_dense/weight", (4 * d, d))
                put(f"{p}/ffn{sfx}/shrink_dense/bias", (d,))
            cin = d
    norm("final_layer_norm", cin)
    t["global_step"] = np.array(0, np.int64)
    t["maxvit/stem/conv_0/kernel/Momentum"] = np.zeros((3, 3, 3, stem_dim), np.float32)
    return Reader(t)
