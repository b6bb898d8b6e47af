"""Derived-state coherence: the families, their entry points and the tensors that provably do not reach an output.

Almost no kernel reads a parameter directly: transformer.derived() builds packed, folded, re-typed or transposed operands and
caches them under a signature of a hand-written tuple of dependencies; GraphedForward and the decoders hold raw pointers into
those operands.  A dependency missing from one tuple is silent - finite, plausible, wrong numbers after a checkpoint is loaded
into a module that has run once.  The tests built on this table change the weights of a WARM module and compare with what
the same module computes once every cache is dropped (transformer.clear_derived), and with a module that never saw the old
weights: tests/test_coherence_cases_cpu.py (no GPU: derived() itself, and that every tensor of every family matters) and
tests/test_hip_coherence.py (the HIP paths).

One row per family (FAMILIES): ``make(seed)`` builds the fp32 CPU module in eval mode with synthweights.fill_module +
bf16_round_; ``inputs()`` the CPU inputs; ``entries`` the entry points, each ``fn(model, inputs) -> tensor or tuple of
tensors`` on whatever device holds both; ``cpu(model, inputs)`` the plain-torch float64 CPU form of the first entry point;
``dtype`` the parameter dtype of the HIP module ("bf16" or "fp32"); ``fp32`` whether the family also has an fp32 HIP path (for
the .float() / .to(bfloat16) round trip); ``expect`` the derived keys that must exist after the warm run (the path the row
is about did engage); ``quiet`` the insensitivity list."""
from __future__ import annotations

import fnmatch
from dataclasses import dataclass, field
from typing import Callable

import torch

from synthweights import bf16_round_, fill_module, synth_input, synth_tensor, synth_tokens

SEED = 211

# Softmax is invariant under a shift that is the same for every key: the key projection's bias adds q . b_k to every score of a
# query, whatever the mask or additive bias, so it never reaches the attention output.  True of every MHA of the shared blocks.
K_BIAS = "q . b_k is one constant per query row: softmax drops it"


@dataclass
class Entry:
    fn: Callable
    # True: the result is a floating tensor that depends on every tensor outside the family's quiet list, so a one-tensor
    # change must move it.  False (token ids, entry points that run a part of the model): only coherence is asserted.
    moves: bool = True


@dataclass
class Family:
    id: str
    make: Callable
    inputs: Callable
    entries: dict
    cpu: Callable
    dtype: str = "bf16"
    fp32: bool = False
    expect: tuple = ()
    quiet: dict = field(default_factory=dict)
    cpu_inputs: Callable | None = None  # a smaller input for the CPU sensitivity run (same code path on the CPU)
    # ``cpu`` may be None: a row whose float64 form cannot separate "reaches the output" from rounding at this geometry; every
    # entry of such a row is ``moves=False`` (coherence, fresh-module and round-trip equality only).
    scope: tuple = ()  # name prefixes of the tensors the one-tensor loop of this row writes (a family split by submodule); () = all
    whole: bool = True  # False: the whole-checkpoint and round-trip tests run on a sibling row of the same module

    def is_quiet(self, key: str) -> bool:
        return any(fnmatch.fnmatchcase(key, pat) for pat in self.quiet)

    def keys(self, module: torch.nn.Module) -> list:
        """the floating tensors this row writes one at a time"""
        return [k for k in float_keys(module) if not self.scope or k.startswith(self.scope)]


# synthweights draws a LayerNorm gain around 1 but has no rule for the gain of a weight-norm parametrization, which it draws
# around 0 with a deviation of 0.1: every EnCodec convolution then attenuates tenfold and nothing behind the first few layers
# reaches the output above rounding.  The table shifts these gains to 1 +- 0.1, in the first fill and in every replacement.
GAIN = "parametrizations.weight.original0"


def filled(module: torch.nn.Module, seed: int) -> torch.nn.Module:
    module = module.eval()
    with torch.no_grad():
        fill_module(module, seed)
        for k, t in named_tensors(module).items():
            if k.endswith(GAIN):
                t.add_(1.0)
        bf16_round_(named_tensors(module))  # the buffers kept out of the state dict too
    return module


def named_tensors(module: torch.nn.Module) -> dict:
    """every parameter and buffer by name: the state dict plus the buffers kept out of it (the STFT window)"""
    named = dict(module.named_parameters())
    named.update(module.named_buffers())
    return named


def float_keys(module: torch.nn.Module) -> list[str]:
    return [k for k, v in named_tensors(module).items() if v.is_floating_point()]


def replacement(key: str, t: torch.Tensor, seed: int = SEED) -> torch.Tensor:
    """The value a test writes over ``t``: the draw of the NEXT seed for the same key (a variance stays positive the way the
    first fill keeps it), rounded to bf16, in the tensor's own dtype and device."""
    v = synth_tensor(key, t.shape, seed + 1)
    return (v + 1.0 if key.endswith(GAIN) else v).to(torch.bfloat16).to(device=t.device, dtype=t.dtype)


@torch.no_grad()
def overwrite(module: torch.nn.Module, key: str, seed: int = SEED) -> None:
    """in place, under no_grad: what a converter's ``copy_`` does (bumps ``_version``)"""
    t = named_tensors(module)[key]
    t.copy_(replacement(key, t, seed))


def second_state(fam: Family) -> dict:
    """the checkpoint of the next seed, fp32 CPU tensors holding bf16 values: every parameter and buffer by name"""
    return {k: v.detach().clone() for k, v in named_tensors(fam.make(SEED + 1)).items()}


@torch.no_grad()
def load_state(module: torch.nn.Module, state: dict, **kw) -> None:
    """``load_state_dict`` of the entries the state dict has, an in-place copy for the buffers kept out of it"""
    own = module.state_dict()
    # (in the module's own dtype and device, so that assign=True swaps in tensors of the kind it held)
    module.load_state_dict({k: state[k].to(device=t.device, dtype=t.dtype) for k, t in own.items()}, **kw)
    for k, t in named_tensors(module).items():
        if k not in own:
            t.copy_(state[k].to(device=t.device, dtype=t.dtype))


def outputs(fam: Family, name: str, model, inp: dict) -> tuple:
    """the entry point's result as a tuple of cloned tensors (a graph's output buffer is overwritten by the next call)"""
    with torch.no_grad():
        out = fam.entries[name].fn(model, inp)
    out = out if isinstance(out, (tuple, list)) else (out,)
    return tuple(o.clone() for o in out if isinstance(o, torch.Tensor))


def same(a: tuple, b: tuple) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def change(a: torch.Tensor, b: torch.Tensor) -> float:
    """relative L2 distance of two float64 results"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / a.norm().clamp_min(1e-300))


# In float64 a tensor that does not reach the output leaves it within rounding: 2^-53 per operation over chains of at most a few
# thousand accumulations, 1e-12 at the outside; QUIET_MAX leaves a factor 100.  A tensor that does reach it is re-drawn as a
# whole (a relative change of order 1 in the tensor); the weakest path of these models is a query / key projection under a
# near-uniform softmax, second order in the (small) scores, and the families kept here stay above LOUD_MIN = 1e-6 by their
# construction (d >= 64, several keys per query, values that differ between keys).  DETR's decoder and MobileViT at their test
# geometry do not: their rows carry no float64 form and assert coherence only (see _detr, _mobile_vit).
QUIET_MAX, LOUD_MIN = 1e-10, 1e-6


# ---------------------------------------------------------------------------------------------------------------- shared blocks
def _blocks(id_, cls, kw, x_shape, mem_shape=None, expect=(), cpu_x_shape=None):
    from pytorch_models import transformer as T

    def make(seed=SEED):
        return filled(getattr(T, cls)(*kw[0], **kw[1]), seed)

    def inputs(shape=x_shape):
        inp = {"x": synth_input(id_ + "_x", shape, SEED)}
        if mem_shape is not None:
            inp["mem"] = synth_input(id_ + "_mem", mem_shape, SEED)
        return inp

    def fwd(m, inp):
        x = inp["x"].to(next(m.parameters()).dtype)
        if mem_shape is None:
            return m(x)
        return m(x, inp["mem"].to(x.dtype))

    return Family(id_, make, inputs, {"forward": Entry(fwd)}, fwd, fp32=True, expect=expect, quiet={"*.k_proj.bias": K_BIAS},
                  cpu_inputs=None if cpu_x_shape is None else (lambda: inputs(cpu_x_shape)))


# ------------------------------------------------------------------------------------------------------------------------ image
def _vit():
    from pytorch_models.image import ViT

    def make(seed=SEED):  # patch 8: the zero-padded patch weight (w2d_pad); class-token pooling: the last layer for row 0 only
        return filled(ViT(2, 128, 2, 8, img_size=32), seed)

    def fwd(m, inp):
        return m(inp["img"])

    return Family("vit", make, lambda: {"img": synth_input("coh_vit", (3, 3, 32, 32), SEED)}, {"forward": Entry(fwd)},
                  lambda m, inp: m(inp["img"].double()), fp32=True, expect=("w2d_pad", "pack_cls"), quiet={"*.k_proj.bias": K_BIAS})


def _mixer(dtype):
    from pytorch_models.image import MLPMixer

    def make(seed=SEED):  # patch 8: w2d_pad on the bf16 path; 16 tokens
        return filled(MLPMixer(2, 64, 8, img_size=32), seed)

    def fwd(m, inp):
        return m(inp["img"])

    return Family("mixer_" + dtype, make, lambda: {"img": synth_input("coh_mixer", (3, 3, 32, 32), SEED)}, {"forward": Entry(fwd)},
                  lambda m, inp: m(inp["img"].double()), dtype=dtype,
                  expect=("mixer_w1f", "mixer_w2f", "w2d_pad") if dtype == "bf16" else ("mixer_w1_f32",),
                  # token mixing's output bias is one value per TOKEN, added to all its channels; it rides the residual stream and
                  # every reader of that stream (norm2, the next block's norm1, the final norm) is a LayerNorm over the channels,
                  # which removes a shift common to them
                  quiet={"layers.*.token_mixing.linear2.bias": "a shift common to a token's channels: every LayerNorm after it removes it"})


def _convnext():
    from pytorch_models.image import ConvNeXt

    def make(seed=SEED):
        return filled(ConvNeXt(32, (1, 1, 1, 1)), seed)

    def fwd(m, inp):
        return m(inp["img"])

    return Family("convnext", make, lambda: {"img": synth_input("coh_convnext", (2, 3, 64, 64), SEED)}, {"forward": Entry(fwd)},
                  lambda m, inp: m(inp["img"].double()), fp32=True, expect=("convnext_block", "stem_t", "s2d"))


def _maxvit():
    from pytorch_models.image import MaxViT

    def make(seed=SEED):  # the geometry of tests/test_hip_maxvit.py (SMALL); the window / grid partition needs 224 x 224
        return filled(MaxViT(32, [1, 1, 2, 1], [32, 64, 96, 128]), seed)

    def fwd(m, inp):
        return m(inp["img"])

    return Family("maxvit", make, lambda: {"img": synth_input("coh_maxvit", (1, 3, 224, 224), SEED)}, {"forward": Entry(fwd)},
                  lambda m, inp: m(inp["img"].double()), fp32=True, expect=("mbconv", "bn_fold", "win_bias", "stem"),
                  quiet={"*.k_proj.bias": K_BIAS})


# ------------------------------------------------------------------------------------------------------------------------- text
def _bert():
    from pytorch_models.text import BERT

    lengths = [9, 5, 1]

    def make(seed=SEED):
        return filled(BERT(300, 2, 128), seed)

    def fwd(m, inp):
        return m(inp["tok"])

    def fwd_len(m, inp):
        return m(inp["tok"], lengths=lengths)

    return Family("bert", make, lambda: {"tok": synth_tokens("coh_bert", (3, 9), 300, SEED)},
                  {"forward": Entry(fwd), "forward_lengths": Entry(fwd_len)},
                  lambda m, inp: m(inp["tok"], lengths=[9, 9, 9]),  # every row whole: forward(), through the CPU form lengths= has
                  fp32=True, quiet={"*.k_proj.bias": K_BIAS})


def _gpt2():
    from oracle import ref_text
    from pytorch_models.text import GPT2

    lengths = [9, 6]

    def make(seed=SEED):
        return filled(GPT2(2, 128), seed)

    def cpu(m, inp):
        return ref_text.gpt2({k: v for k, v in m.state_dict().items()}, inp["tok"])

    return Family("gpt2", make, lambda: {"tok": synth_tokens("coh_gpt2", (2, 9), 50257, SEED)},
                  {"forward": Entry(lambda m, inp: m(inp["tok"])),
                   "generate": Entry(lambda m, inp: m.generate(inp["tok"][:, :4], 5), moves=False),
                   "generate_prefill": Entry(lambda m, inp: m.generate(inp["tok"], 4, prefill=True), moves=False),
                   "generate_beams": Entry(lambda m, inp: m.generate(inp["tok"][:, :4], 4, beams=2, return_beams=True), moves=False),
                   "score": Entry(lambda m, inp: m.score(inp["tok"], lengths))},
                  cpu, fp32=True, quiet={"*.k_proj.bias": K_BIAS})


# ------------------------------------------------------------------------------------------------------------------------ audio
def _whisper():
    from pytorch_models.audio2text import Whisper

    def make(seed=SEED):
        return filled(Whisper(300, 2, 128), seed)

    def inputs():
        return {"mel": synth_input("coh_whisper_mel", (2, 80, 40), SEED), "tok": synth_tokens("coh_whisper", (2, 6), 300, SEED)}

    def mel(m, inp):
        return inp["mel"].to(next(m.parameters()).dtype)

    return Family("whisper", make, inputs,
                  {"forward": Entry(lambda m, inp: m(mel(m, inp), inp["tok"])),
                   "generate": Entry(lambda m, inp: m.generate(mel(m, inp), inp["tok"][:, :2], 5), moves=False),
                   "generate_exact": Entry(lambda m, inp: m.generate(mel(m, inp), inp["tok"][:, :2], 4, exact=True), moves=False),
                   "generate_beams": Entry(lambda m, inp: m.generate(mel(m, inp), inp["tok"][:, :2], 4, beams=2, return_beams=True),
                                           moves=False),
                   "align": Entry(lambda m, inp: m.align(mel(m, inp), inp["tok"], return_matrix=True), moves=False)},
                  lambda m, inp: m(inp["mel"].double(), inp["tok"]), fp32=True, quiet={"*.k_proj.bias": K_BIAS})


def _sd64(m):
    return {k: v.double() for k, v in m.state_dict().items()}


def _gpt():
    from oracle import ref_text
    from pytorch_models.text import GPT
    from pytorch_models.text.generator import DecoderGenerator

    def make(seed=SEED):  # post-norm, no final norm: decodes through the fp32 twin ("exact32") of the bf16 model
        return filled(GPT(2, 128), seed)

    def generate(m, inp):
        ids = DecoderGenerator(m, None).generate_ids(inp["tok"][0, :4].tolist(), max_tokens=4)
        return torch.tensor(ids)

    return Family("gpt", make, lambda: {"tok": synth_tokens("coh_gpt", (2, 9), 1000, SEED)},
                  {"forward": Entry(lambda m, inp: m(inp["tok"])), "generate": Entry(generate, moves=False)},
                  lambda m, inp: ref_text.gpt(_sd64(m), inp["tok"]), fp32=True, quiet={"*.k_proj.bias": K_BIAS})


def _t5():
    from oracle import ref_t5
    from pytorch_models.text import T5Model

    lengths = [9, 6]

    def make(seed=SEED):  # head_dim is 64: two heads at d = 128
        return filled(T5Model(300, 128, 2, 2, 256), seed)

    def inputs():
        return {"src": synth_tokens("coh_t5_src", (2, 9), 300, SEED), "tgt": synth_tokens("coh_t5_tgt", (2, 5), 300, SEED)}

    def generate(packed):  # the same geometry for every call: only the signature can separate the kept decode state
        return lambda m, inp: m.generate(inp["src"], lengths=lengths, max_new_tokens=5, packed=packed)

    return Family("t5", make, inputs,
                  {"forward": Entry(lambda m, inp: m(inp["src"], inp["tgt"])),
                   "encode_lengths": Entry(lambda m, inp: m.encode(inp["src"], lengths=lengths), moves=False),  # the encoder alone
                   "generate": Entry(generate(False), moves=False), "generate_packed": Entry(generate(True), moves=False),
                   "score": Entry(lambda m, inp: m.score(inp["src"], inp["tgt"]))},
                  lambda m, inp: ref_t5.model(_sd64(m), inp["src"], inp["tgt"]))


def _w2v(id_, build, oracle, n=4000):
    lengths = [n, n - 1000]

    def make(seed=SEED):
        return filled(build(), seed)

    entries = {"forward": Entry(lambda m, inp: m(inp["wave"]))}
    if oracle is None:  # the layer-norm stem: the variable-length form exists, and it is the CPU form
        entries["forward_lengths"] = Entry(lambda m, inp: m(inp["wave"], lengths=lengths))
        cpu = lambda m, inp: m(inp["wave"].double(), lengths=[n, n])  # noqa: E731
    else:
        cpu = lambda m, inp: oracle(_sd64(m), inp["wave"].double())  # noqa: E731
    quiet = {"*.k_proj.bias": K_BIAS}
    if id_ == "sew":  # the one biased convolution in front of a GroupNorm (one group per channel, statistics over time)
        quiet["feature_encoder.0.0.bias"] = "a per-channel constant in front of the stem's GroupNorm, which subtracts the channel's mean"
    return Family(id_, make, lambda: {"wave": synth_input("coh_" + id_, (2, n), SEED)}, entries, cpu, quiet=quiet)


def _ctc():
    from pytorch_models.audio import Wav2Vec2, Wav2Vec2CTC

    n, lengths = 4000, [4000, 3000]
    targets, target_lengths = torch.tensor([[3, 5, 5, 9], [7, 2, 0, 0]]), [4, 2]

    def make(seed=SEED):
        return filled(Wav2Vec2CTC(Wav2Vec2(1, 128), 32, blank=31), seed)

    return Family("ctc", make, lambda: {"wave": synth_input("coh_ctc", (2, n), SEED)},
                  {"log_probs": Entry(lambda m, inp: m.log_probs(inp["wave"], lengths=lengths)),
                   "decode": Entry(lambda m, inp: m.decode(inp["wave"], lengths=lengths), moves=False),
                   "score": Entry(lambda m, inp: m.score(inp["wave"], targets, target_lengths, lengths=lengths)),
                   "align": Entry(lambda m, inp: m.align(inp["wave"], targets, target_lengths, lengths=lengths), moves=False)},
                  # (log_probs itself answers in fp32: the encoder's float64 rows through the head by hand)
                  lambda m, inp: torch.log_softmax(torch.nn.functional.linear(m.encoder(inp["wave"].double(), lengths=[n, n]),
                                                                              m.lm_head.weight, m.lm_head.bias), -1),
                  quiet={"*.k_proj.bias": K_BIAS})


def _audio_rows():
    from oracle import ref_audio as RA
    from pytorch_models.audio import SEW, Data2VecAudio, Wav2Vec2

    return [
        _w2v("wav2vec2", lambda: Wav2Vec2(2, 64), None),
        # the HuBERT / wav2vec2-base form: group-norm ("legacy") stem without biases, post-norm encoder
        _w2v("hubert", lambda: Wav2Vec2(2, 128, stem_bias=False, stem_legacy=True, pre_norm=False),
             lambda sd, x: RA.wav2vec2(sd, x, pre_norm=False, legacy=True)),
        _w2v("data2vec_audio", lambda: Data2VecAudio(2, 128), RA.data2vec_audio),
        _w2v("sew", lambda: SEW(2, 128), RA.sew),
        _ctc(),
    ]


def _spectrogram(kind):
    from pytorch_models.audio.spectrogram import MelSpectrogram, Spectrogram

    def make(seed=SEED):  # the analytic window / filterbank at SEED (fill_module leaves them alone), a drawn one at any other seed
        m = (Spectrogram(64, 16) if kind == "power" else MelSpectrogram(64, 16, 10, 16000)).eval()
        if seed != SEED:
            for key in float_keys(m):
                overwrite(m, key, seed - 1)
        return m

    def fwd(m, inp):
        return m(inp["wave"])

    return Family("spectrogram_" + kind, make, lambda: {"wave": synth_input("coh_wave", (2, 400), SEED)}, {"forward": Entry(fwd)},
                  lambda m, inp: m(inp["wave"].double()), dtype="fp32")


def _detr(part, scope, cpu_ok, whole=False, quiet=None):
    from pytorch_models.image import DETR

    def make(seed=SEED):
        return filled(DETR([1, 1, 1, 1]), seed)

    def cpu(m, inp):
        logits, boxes = m(inp["img"].double())
        return torch.cat([logits.flatten(), boxes.flatten()])

    # One module, four rows by top-level submodule (350 tensors).  ``pos_embed.freqs`` is in no row: the HIP path recomputes the
    # analytic frequencies on the host (the buffer is bf16 after .to(bfloat16)) and never reads it.
    # The decoder row has no float64 form: its first layer's self-attention sees tgt = 0, so every value row is the bias and its
    # q / k projections cannot reach the output (float64 change 9e-16); in the later layers they reach it at 5e-8 .. 3e-6, below
    # LOUD_MIN and below what a bf16 activation resolves.  Its entry is moves=False: staleness, fresh-module and round-trip
    # equality are asserted for every tensor of it all the same.
    return Family("detr_" + part, make, lambda: {"img": synth_input("coh_detr", (1, 3, 64, 64), SEED)},
                  {"forward": Entry(lambda m, inp: m(inp["img"]), moves=cpu_ok)}, cpu if cpu_ok else None,
                  expect=("bn_fold", "conv_bn", "stem", "w2d", "embed_qkv_2", "embed_q_1", "embed_kv_1"),
                  quiet=quiet or {}, scope=scope, whole=whole)


def _mobile_vit():
    from pytorch_models.image import MobileViT

    def make(seed=SEED):
        return filled(MobileViT.from_apple("xxs"), seed)

    # No float64 form at this geometry: 64 x 64 ends in one token per patch sequence (q / k of the last stage cannot reach the
    # output, float64 change 0.0) and the q biases of the other stages reach it at 1e-6 .. 5e-6.  moves=False.
    return Family("mobile_vit", make, lambda: {"img": synth_input("coh_mobile_vit", (1, 3, 64, 64), SEED)},
                  {"forward": Entry(lambda m, inp: m(inp["img"]), moves=False)}, None, expect=("folded_nhwc",))


def _encodec(side):
    from pytorch_models.audio import EnCodec

    def make(seed=SEED):  # the 24 kHz form (mono, causal, weight-norm parametrizations on every convolution) with 4 codebooks
        return filled(EnCodec(1, "weight_norm", True, 4, False), seed)

    if side == "encode":  # codes are discrete: coherence only, over the tensors that feed them
        return Family("encodec_encode", make, lambda: {"wave": synth_input("coh_encodec", (2, 1, 3200), SEED)},
                      {"encode": Entry(lambda m, inp: m.encode(inp["wave"])[0], moves=False)}, None, dtype="fp32",
                      expect=("w2d", "books"), scope=("encoder.", "quantizer."))
    codes = synth_tokens("coh_encodec_codes", (2, 4, 10), 1024, SEED)  # decoding from given codes is floating end to end

    def decode(m, inp):
        return m.decode(inp["codes"])

    return Family("encodec_decode", make, lambda: {"codes": codes}, {"decode": Entry(decode)}, decode, dtype="fp32",
                  expect=("w2d",), scope=("quantizer.", "decoder."))


def _families():
    enc = ((2, 64), {})
    rows = [
        _blocks("encoder_pre", "Encoder", enc, (2, 9, 64)),
        _blocks("encoder_post", "Encoder", ((2, 64), {"pre_norm": False}), (2, 9, 64)),
        _blocks("decoder_pre_cross", "Decoder", ((2, 64), {"cross_attn": True}), (2, 9, 64), (2, 5, 64)),
        _blocks("decoder_post_cross", "Decoder", ((2, 64), {"cross_attn": True, "pre_norm": False}), (2, 9, 64), (2, 5, 64)),
        # the one size above tiny: the LayerNorm fold engages (tests/test_hip_fuzz.py's geometry); the CPU form has no such
        # threshold, its sensitivity run takes a small input
        _blocks("encoder_fold", "Encoder", ((2, 128), {"n_heads": 2, "norm_eps": 1e-6}), (190, 700, 128),
                expect=("pack_qkv_ln", "l1_ln"), cpu_x_shape=(2, 9, 128)),
        _vit(), _mixer("bf16"), _mixer("fp32"), _convnext(), _maxvit(),
        _detr("backbone", ("backbone.",), True, whole=True), _detr("encoder", ("encoder.",), True, quiet={"*.k_proj.bias": K_BIAS}),
        _detr("decoder", ("decoder.",), False), _detr("head", ("input_proj.", "query_embed", "norm.", "classifier.", "box_head."), True),
        _mobile_vit(), _encodec("encode"), _encodec("decode"), _bert(), _gpt(), _gpt2(), _t5(),
        _whisper(), *_audio_rows(), _spectrogram("power"), _spectrogram("mel"),
    ]
    return {f.id: f for f in rows}


FAMILIES = _families()
