"""EnCodec on one MI355X, fp32 on synthetic weights: 24khz at 32 clips x 10 s and 48khz at 16 clips x 10 s.
* encode and decode in audio-seconds per second, eager and replayed as one HIP graph (pytorch_models.graph.GraphedForward);
* the same weights through stock PyTorch-ROCm fp32 operators written here (F.conv1d on a reflect-padded copy, F.conv_transpose1d,
  nn.LSTM, F.group_norm, the distance / argmin loop of the model): the yardstick;
* microseconds per LSTM launch: pm_lstm_f32 on the model's (B, T, 512) minus its input-projection GEMM(s), as the wavefront
  (T + 1 launches, both layers in each) and as plain passes (2 T launches);
* every convolution shape of encoder and decoder alone: TFLOP/s and the fraction of the 157 TFLOP/s f32 matrix peak, and - where
  the window form of pm_linear_f32 can take the shape (a multiple of 4 floats per stride step) - that GEMM on a reflect-padded,
  ELU-applied copy built beforehand (its padding pass is NOT in its time).
`--profile-run` only runs encode + decode a few times: the body of a `rocprofv3 --kernel-trace --stats` run.
Prints one JSON line.    python tools/encodec_bench.py [--variant 24khz] [--batch 32] [--seconds 10]"""
import argparse
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
from pytorch_models.audio import EnCodec  # noqa: E402
from pytorch_models.audio import encodec as E  # noqa: E402
from pytorch_models.graph import GraphedForward  # noqa: E402
from synthweights import fill_module, synth_input  # noqa: E402

PEAK_F32 = 157e12  # FLOP/s, f32 MFMA (spec)
RATE = {"24khz": 24000, "48khz": 48000}

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="24khz", choices=sorted(RATE))
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--profile-run", action="store_true")
args = ap.parse_args()
torch.set_grad_enabled(False)
B = args.batch or {"24khz": 32, "48khz": 16}[args.variant]
samples = int(args.seconds * RATE[args.variant])

m = EnCodec.from_facebook(args.variant).eval()
fill_module(m, 171)
for mod in m.modules():  # weight-norm gains that keep the signal alive: an effective weight of 0.8 v
    if isinstance(mod, (nn.Conv1d, nn.ConvTranspose1d)) and nn.utils.parametrize.is_parametrized(mod, "weight"):
        p = mod.parametrizations.weight
        p.original0.copy_(0.8 * p.original1.flatten(1).norm(dim=1).view(-1, 1, 1))
m = m.cuda()
C = m.encoder[0].conv.in_channels
x = synth_input("encodec_bench", (B, C, samples), 171, scale=0.3).cuda()
codes, scale = m.encode(x)
audio_s = B * args.seconds

if args.profile_run:
    for _ in range(5):
        m.decode(*m.encode(x))
    torch.cuda.synchronize()
    print(json.dumps({"tool": "encodec_bench", "mode": "profile-run", "variant": args.variant, "batch": B, "iterations": 5}))
    sys.exit(0)


def window(fn, ms_per_call):
    n = max(3, int(40.0 / max(ms_per_call, 1e-3)))
    return time_us(fn, warmup=n, iters=n)


def timed(fn):
    return window(fn, time_us(fn, warmup=1, iters=2) / 1e3)


# ---- the model, eager and graphed
class _Enc(nn.Module):
    def forward(self, a):
        return m.encode(a)[0]


class _Dec(nn.Module):
    def forward(self, c):
        return m.decode(c, scale)


t_enc, t_dec = timed(lambda: m.encode(x)), timed(lambda: m.decode(codes, scale))
g_enc, g_dec = GraphedForward(_Enc(), x), GraphedForward(_Dec(), codes)
t_enc_g, t_dec_g = timed(lambda: g_enc(x)), timed(lambda: g_dec(codes))
assert torch.equal(g_enc(x), codes)


# ---- yardstick: the same weights through stock PyTorch-ROCm fp32 operators
def y_conv(c, h):
    extra = -h.shape[2] % c.pad.stride
    h = F.conv1d(F.pad(h, (c.pad.left, c.pad.right + extra), mode="reflect"), c.conv.weight, c.conv.bias, c.conv.stride)
    return F.group_norm(h, 1, c.norm.weight, c.norm.bias, c.norm.eps) if isinstance(c.norm, nn.GroupNorm) else h


def y_convt(c, h):
    h = F.conv_transpose1d(h, c.conv.weight, c.conv.bias, c.conv.stride)
    if isinstance(c.norm, nn.GroupNorm):
        h = F.group_norm(h, 1, c.norm.weight, c.norm.bias, c.norm.eps)
    return h[..., c.unpad.left: -c.unpad.right]


_stock_lstm = {}


def y_lstm(l, h):
    if l not in _stock_lstm:
        s = nn.LSTM(l.input_size, l.hidden_size, l.num_layers).cuda().eval()
        s.load_state_dict(l.state_dict())
        _stock_lstm[l] = s
    return h + _stock_lstm[l](h.permute(2, 0, 1))[0].permute(1, 2, 0)


def y_stack(stack, h):
    for c in stack:
        if isinstance(c, nn.ELU):
            h = F.elu(h)
        elif isinstance(c, E.Conv1d):
            h = y_conv(c, h)
        elif isinstance(c, E.ConvTranspose1d):
            h = y_convt(c, h)
        elif isinstance(c, E.LSTM):
            h = y_lstm(c, h)
        else:
            h = y_conv(c.shortcut, h) + y_conv(c.layers[3], F.elu(y_conv(c.layers[1], F.elu(h))))
    return h


def y_encode(a):
    s = None
    if m.normalize:
        s = a.mean(1, keepdim=True).square().mean(2, keepdim=True).sqrt() + 1e-8
        a = a / s
    r = y_stack(m.encoder, a).transpose(1, 2)
    out = []
    for vq in m.quantizer:
        e = vq.embed
        i = (r.square().sum(-1, keepdim=True) - 2 * r @ e.T + e.square().sum(-1)).argmin(-1)
        r = r - F.embedding(i, e)
        out.append(i)
    return torch.stack(out, 1), s


def y_decode(c, s):
    q = sum(F.embedding(c[:, i], vq.embed) for i, vq in enumerate(m.quantizer))
    y = y_stack(m.decoder, q.transpose(1, 2))
    return y if s is None else y * s


t_yenc, t_ydec = timed(lambda: y_encode(x)), timed(lambda: y_decode(codes, scale))
ycodes, _ = y_encode(x)
ywave, wave = y_decode(codes, scale), m.decode(codes, scale)
agree = dict(codes_equal_fraction=round(float((ycodes == codes).float().mean()), 5),
             wave_max_err_over_max_abs=float((ywave - wave).abs().max() / ywave.abs().max()))

# ---- LSTM: microseconds per step
lstm = m.encoder[13]
T = codes.shape[2]
hx = synth_input("encodec_bench_lstm", (B, T, 512), 171).cuda()
t_lstm = timed(lambda: lstm.run_tm(hx))  # the wavefront: one GEMM, T + 1 launches
lw = [[getattr(lstm, f"{n}_l{l}").detach() for l in range(2)] for n in ("weight_ih", "weight_hh")]
lb = [(getattr(lstm, f"bias_ih_l{l}") + getattr(lstm, f"bias_hh_l{l}")).detach() for l in range(2)]
t_lstm_plain = timed(lambda: ops.lstm_f32(hx, lw[0], lw[1], lb, residual=True, plain=True))  # two GEMMs, 2 T launches
w0 = lstm.weight_ih_l0.detach()
t_gemm = timed(lambda: ops.linear_f32(hx.view(B * T, 512), w0, None))
lstm_res = dict(B=B, T=T, input_gemm_us_each=round(t_gemm, 1), kernel_boundary_us=1.45,
                wavefront=dict(total_us=round(t_lstm, 1), launches=T + 1, us_per_launch=round((t_lstm - t_gemm) / (T + 1), 3)),
                plain_passes=dict(total_us=round(t_lstm_plain, 1), launches=2 * T, us_per_launch=round((t_lstm_plain - 2 * t_gemm) / (2 * T), 3)))

# ---- every convolution shape alone
convs = []


def conv_shapes(stack, t_in):
    t = t_in
    for c in stack:
        if isinstance(c, E.Conv1d):
            yield c, t
            t = -(-t // c.conv.stride[0])
        elif isinstance(c, E.ConvTranspose1d):
            yield c, t
            t = t * c.conv.stride[0]
        elif isinstance(c, E.EnCodecBlock):
            for cc in (c.shortcut, c.layers[1], c.layers[3]):
                yield cc, t


seen = set()
for side, stack, t_in in (("enc", m.encoder, samples), ("dec", m.decoder, T)):
    for c, t in conv_shapes(stack, t_in):
        cv = c.conv
        tr = isinstance(c, E.ConvTranspose1d)
        key = (tr, cv.in_channels, cv.out_channels, cv.kernel_size[0], cv.stride[0], t)
        if key in seen:
            continue
        seen.add(key)
        saved, c.norm = c.norm, nn.Identity()  # the convolution kernel alone
        h = synth_input(f"encodec_bench_{key}", (B, t, cv.in_channels), 171).cuda()
        us = timed(lambda: c.run_tm(h, elu=True))
        c.norm = saved
        if tr:
            flops = 2.0 * B * (t + 1) * cv.stride[0] * cv.out_channels * 2 * cv.in_channels
        else:
            flops = 2.0 * B * -(-t // cv.stride[0]) * cv.out_channels * cv.kernel_size[0] * cv.in_channels
        e = dict(side=side, kind="convT" if tr else "conv", cin=cv.in_channels, cout=cv.out_channels, k=cv.kernel_size[0],
                 stride=cv.stride[0], frames=t, us=round(us, 1), tflop_per_s=round(flops / us / 1e6, 2),
                 frac_of_f32_peak=round(flops / (us * 1e-6) / PEAK_F32, 4))
        if not tr and (cv.stride[0] * cv.in_channels) % 4 == 0:  # pm_linear_f32's window form on a padded copy
            s, k, cin = cv.stride[0], cv.kernel_size[0], cv.in_channels
            extra = -t % s
            hp = F.pad(F.elu(h).transpose(1, 2), (c.pad.left, c.pad.right + extra), mode="reflect").transpose(1, 2).contiguous()
            w2d = cv.weight.detach().permute(0, 2, 1).reshape(cv.out_channels, -1).contiguous()
            tout = -(-t // s)
            us_l = timed(lambda: ops.linear_f32(hp, w2d, cv.bias, M=B * tout, K=k * cin, row_stride=s * cin, rows_per_batch=tout,
                                                batch_stride=hp.shape[1] * cin))
            e["linear_f32_window_us"] = round(us_l, 1)
        convs.append(e)

res = {
    "tool": "encodec_bench", "model": f"EnCodec {args.variant} fp32", "batch": B, "seconds_per_clip": args.seconds, "frames": T,
    "encode": dict(eager_ms=round(t_enc / 1e3, 3), graphed_ms=round(t_enc_g / 1e3, 3), audio_s_per_s_eager=round(audio_s / (t_enc * 1e-6), 1),
                   audio_s_per_s_graphed=round(audio_s / (t_enc_g * 1e-6), 1)),
    "decode": dict(eager_ms=round(t_dec / 1e3, 3), graphed_ms=round(t_dec_g / 1e3, 3), audio_s_per_s_eager=round(audio_s / (t_dec * 1e-6), 1),
                   audio_s_per_s_graphed=round(audio_s / (t_dec_g * 1e-6), 1)),
    "yardstick_pytorch_fp32": dict(encode_ms=round(t_yenc / 1e3, 3), decode_ms=round(t_ydec / 1e3, 3),
                                   encode_speedup=round(t_yenc / t_enc_g, 3), decode_speedup=round(t_ydec / t_dec_g, 3), **agree),
    "lstm": lstm_res, "convs": convs, "bounds": {"f32_mfma_flop_s": PEAK_F32}, "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res), flush=True)
