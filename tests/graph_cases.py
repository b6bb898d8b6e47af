"""Graph replay contract: the protocol that replays a call as a captured graph and compares it bit for bit
with the eager call, and the four tables that say which wrappers and which models go through it.

pytorch_models/graph.py rests on one sentence: every operator is a kernel launch on the current stream with no host
synchronisation.  The parity, layout and coherence suites launch eagerly, once, on the default stream, so they cannot see the
host plumbing fail in the six ways a replay can:

  1. a wrapper reads device memory or uploads on the host;      4. a scalar taken from a tensor's contents becomes a kernel argument;
  2. a launch goes to another stream than the current one;      5. a cached tensor is replaced while a graph holds its pointer;
  3. state a kernel expects reset is reset by the wrapper;      6. a replay allocates.

``check_replay`` is written once over two callables, ``capture(run, static) -> handle`` and ``replay(handle)``:
tests/test_hip_graph_ops.py and tests/test_hip_graph_models.py pass torch.cuda.graph / GraphedForward, tests/test_graph_cases_cpu.py a
recording fake (``FakeGraphs``) and toy ops with each defect planted.  Every comparison is of bits; nothing here has a tolerance.

The tables: CAPTURED (ids of wrapper_cases.ROWS replayed as single ops), HOST_BOUND (ROWS id -> why the wrapper needs the host:
it must raise the capture guard of ops.no_capture instead), MODELS (one entry per model class at the smallest geometry of its
family's tests) and NOT_GRAPHED (entry point -> why it is not replayed).  CAPTURED | HOST_BOUND is every row and MODELS |
NOT_GRAPHED every exported model class and every entry point README.md names: a new wrapper or model has to choose a table."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import torch
from torch import Tensor

import wrapper_cases as WC

SEED_B = 1000  # the seed offset of the second operand set: beyond the per-row offsets of wrapper_cases.ROWS


class CaseProvesNothing(AssertionError):
    """the two operand sets of a case give the same bits somewhere: a failure of the case, not of the op"""


# ---------------------------------------------------------------------------------------------------------------- the protocol
@dataclass
class Handle:
    """what ``capture`` returns: ``result`` - the captured call's result, whose tensors every replay overwrites; ``static`` - the
    operands the captured launches read; ``graph`` - whatever ``replay`` needs"""
    graph: object
    result: object
    static: object = None


def _named_diff(got, want) -> list[str]:
    if [n for n, _ in got] != [n for n, _ in want]:
        return [f"results differ in kind: {[n for n, _ in got]} vs {[n for n, _ in want]}"]
    return [n for (n, x), (_, y) in zip(got, want) if not WC.same_bits(x, y)]


def check_replay(run, set_a, set_b, overwrite, *, capture, replay, clone, snap, inplace: bool = False, warm=None, allocated=None,
                 hook=None, same_ok=()) -> list[str]:
    """``run(operands) -> result`` eagerly on clones of ``set_a`` and ``set_b`` (the wanted bits), then captured on static operands
    and replayed on each; returns the problems found (an empty list: the call replays bit for bit).

    ``clone(operands)``: a deep copy; ``snap(operands, result) -> [(name, tensor clone)]``: outputs and in-place operands;
    ``overwrite(static, src)``: ``copy_`` of every tensor of ``src`` into ``static`` - the new data AND the pre-call content of
    the in-place operands (``set_a`` / ``set_b`` themselves are never run on).  ``inplace``: the call consumes operands, so the
    "replay again" steps restore them first.  ``warm(fn)``: runs fn in front of the capture (a side stream on the GPU);
    ``allocated()``: bytes in use; ``hook()``: eager work between two replays; ``same_ok``: names of results that cannot differ
    between the two sets (a position counter advanced by one)."""
    problems: list[str] = []
    ea, eb = clone(set_a), clone(set_b)
    res_a = run(ea)
    want_a = snap(ea, res_a)
    want_b = snap(eb, run(eb))
    if _named_diff(snap(ea, res_a), want_a):  # (an op that hands out one private buffer per call site)
        problems.append("the result of an eager call changed when the op was called again: it does not own its memory")
    if not want_a:
        raise CaseProvesNothing("the call returns nothing and writes nothing")
    same = [n for (n, x), (_, y) in zip(want_a, want_b) if n not in same_ok and WC.same_bits(x, y)]
    if same:
        raise CaseProvesNothing(f"{same} hold the same bits for both operand sets")
    del ea, eb, res_a

    static = clone(set_a)
    if warm is not None:
        warm(lambda: run(static))
    overwrite(static, set_a)
    handle = capture(run, static)
    static = handle.static if handle.static is not None else static

    def step(src, want, what: str) -> None:
        if src is not None:
            overwrite(static, src)
        replay(handle)
        bad = _named_diff(snap(static, handle.result), want)
        if bad:
            problems.append(f"{what}: {bad} differ from the eager call")

    step(set_a, want_a, "first replay")
    step(set_b, want_b, "replay on new operands")
    step(set_b if inplace else None, want_b, "second replay on the same operands")
    if hook is not None:
        hook()
        step(set_b if inplace else None, want_b, "replay after eager work in between")
    if allocated is not None:
        before = allocated()
        for _ in range(3):
            if inplace:
                overwrite(static, set_b)
            replay(handle)
        after = allocated()
        if after != before:
            problems.append(f"three further replays changed the memory in use from {before} to {after} bytes")
        bad = _named_diff(snap(static, handle.result), want_b)
        if bad:
            problems.append(f"replay after three further ones: {bad} differ from the eager call")
    step(set_a, want_a, "replay on the first operands again")
    return problems


class FakeGraphs:
    """The CPU stand-in for stream capture: an op issues its kernels through ``launch(fn)``.  Outside a capture fn runs at once;
    inside, it is recorded and NOT run - host code of the op runs once, at capture, as under torch.cuda.graph - and ``replay``
    re-runs the recorded closures.  ``bytes`` is the memory the toy ops say they hold."""

    def __init__(self) -> None:
        self.recording, self.bytes = None, 0

    def launch(self, fn) -> None:
        if self.recording is not None:
            self.recording.append(fn)
        else:
            fn()

    def capture(self, run, static) -> Handle:
        self.recording = []
        try:
            result = run(static)
        finally:
            launches, self.recording = self.recording, None
        return Handle(launches, result)

    @staticmethod
    def replay(handle: Handle) -> None:
        for fn in handle.graph:
            fn()

    def allocated(self) -> int:
        return self.bytes


# ------------------------------------------------------------------------------------------------------- operand sets of a row
def clone_kw(kw: dict) -> dict:
    """every tensor of a row's keyword arguments cloned (lists and tuples rebuilt); everything else - ints, SeqLens - shared"""
    out = dict(kw)
    for path, t in WC.operands(kw):
        out = WC.replaced(out, path, t.clone())
    return out


def overwrite_kw(static: dict, src: dict) -> None:
    for path, t in WC.operands(src):
        WC.get(static, path).copy_(t)


# Floating-point operands that are the same in both sets, each with its reason
SHARED = {("stft_mel", "tables"): "the twiddle tables of the analysis window: a function of n_fft and the window, not data"}


def row_sets(r: WC.Row, dev) -> tuple[dict, dict]:
    """The two operand sets of a row: the canonical build and the build SEED_B seeds on.  An operand whose SHAPE depends on the
    drawn values (the CSR form of a random filterbank) is structure, not data: set b takes set a's.  Every floating-point
    operand of the same shape must differ between the sets, or the case proves nothing."""
    a, b = r.build(dev), r.build(dev, SEED_B)
    # (a structure is taken whole: the CSR triple's row pointers always have one shape, and set b's pointers over set a's shorter
    # column and value arrays sent the kernel past their end - results that depended on what lay behind them)
    whole = {path[0] for path, t in WC.operands(a) if WC.get(b, path).shape != t.shape or WC.get(b, path).dtype != t.dtype}
    for path, t in WC.operands(a):
        u = WC.get(b, path)
        if path[0] in whole:
            b = WC.replaced(b, path, t.clone())
        elif t.is_floating_point() and t.numel() and WC.same_bits(t, u) and (r.id, path[0]) not in SHARED and \
                not (path[0] in r.inplace and not bool(t.any())):  # (a zeroed output buffer is not data)
            raise CaseProvesNothing(f"{r.id}: operand {WC.path_name(path)} is the same in both sets")
    return a, b


def host_kw(r: WC.Row, kw: dict) -> dict:
    """the row's call with its ``host_ok`` operands as host ints: the form that uploads"""
    kw = dict(kw)
    for name in r.host_ok:
        kw[name] = [int(v) for v in kw[name].tolist()]
    return kw


# ------------------------------------------------------------------------------------------------------------------ the tables
# Results that are the same for both operand sets by construction: the sets share their positions (integer operands that are
# ids, lengths or positions may stay), and these results are functions of the positions alone.
SAME_OK = {
    "dec_next_token": ("pos", "ticket"), "dec_next_token:plain": ("pos", "ticket"),
    "dec_sample_topk": ("pos", "ticket"), "dec_sample_topk:plain": ("pos", "ticket"),
    "dec_beam_select": ("pos", "ticket"),
}

HOST_BOUND = {
    "dec_linear_ksplit": "the stand-alone op reads its ticket counters back after the launch (the decoders put the kernel into their plan)",
    "dec_whisper_rules": "the stand-alone op uploads the suppress / blank id lists (the decoders upload them once, when they are built)",
    "dec_beam_reorder": "the stand-alone op reads parents and pos on the host, uploads its pointer table and synchronises",
    "align_dtw": "called with host lengths / frames (host_ok): one upload through align_counts",
    "ctc_forward": "called with host target_lengths (host_ok): one upload through align_counts",
    "ctc_viterbi": "called with host target_lengths (host_ok): one upload through align_counts",
}

# Every other row launches without host data (ctc_greedy too: the wrapper takes and returns device tensors; the Python lists of
# the best-path decoding are Wav2Vec2CTC.decode's callers' business).  align_dtw / ctc_forward / ctc_viterbi are in both
# tables: captured with the device counts of their canonical row, refused with host ones.
CAPTURED = (
    "ln_stats_finalize", "linear", "linear:ln_fold", "linear_f32", "attention_f32", "layernorm", "layernorm:plain", "rmsnorm", "geglu",
    "attention", "conv2d_nhwc", "mean_rows", "vit_tokens", "linear_strided", "w2v_stem0", "group_windows", "grouped_conv",
    "avgpool_time2", "stft_mel", "whisper_stem1", "embed_tokens", "embed_tokens:f32_table", "dec_linear", "dec_argmax", "dec_attention",
    "prefill_attention", "dec_attention_ragged", "prefill_attention_ragged", "embed_tokens_ragged", "dec_embed_ragged",
    "dec_next_token", "dec_next_token:plain", "dec_sample_topk", "dec_sample_topk:plain", "dec_beam_topw", "dec_beam_select",
    "dwconv7_ln", "ln_space_to_depth", "convnext_stem", "mean_ln", "window_attention", "dwconv3_bn_act", "se_gate", "maxvit_stem",
    "im2col3x3", "avgpool2x2", "conv_bf16", "resnet_stem", "attention_hd32", "mixer_token_mix", "row_stats", "ln_mean",
    "transpose_add_f32", "conv1d_f32", "lstm_f32", "rvq_encode", "rvq_decode", "groupnorm1_", "encodec_scale", "scale_clips",
    "cls_head_gemm", "cls_attend", "lm_score", "align_lse", "align_matrix", "align_dtw", "attention_varlen", "attention_varlen:plain",
    "embed_tokens_varlen", "rows_pack", "rows_unpack", "rows_zero_tail", "segment_mean", "ctc_head", "ctc_greedy", "ctc_forward",
    "ctc_viterbi",
)


# ------------------------------------------------------------------------------------------------------------------ the models
@dataclass
class Model:
    """``make(k)``: the fp32 CPU module in eval mode, unfilled, for geometry k (only a fixed position table makes it depend on
    k); ``inputs(k, seed)``:
    the CPU inputs of geometry k - 0 the captured one (batch 2), 1 another batch and another sequence length or image size for
    the SAME module, 2 a third geometry for a second instance; ``cast``: the indices of the inputs that take the parameters'
    dtype; ``dtypes``: the parameter dtypes the family's HIP path serves; ``method``: an entry point other than forward;
    ``lengths``: for a forward that also takes device lengths, (k) -> the lengths tensor - it must raise the guard."""
    cls: str
    make: Callable
    inputs: Callable
    cast: tuple = ()
    dtypes: tuple = ("bf16",)
    method: str | None = None
    lengths: Callable | None = None
    warmup: int = 2


def _img(tag, shapes):
    from synthweights import synth_input
    return lambda k, seed: (synth_input(f"graph_{tag}", shapes[k], seed),)


def _tok(tag, shapes, vocab):
    from synthweights import synth_tokens
    return lambda k, seed: (synth_tokens(f"graph_{tag}", shapes[k], vocab, seed),)


def _models() -> dict:
    from synthweights import synth_input, synth_tokens

    from pytorch_models import audio, audio2text, image, text

    both = ("bf16", "fp32")
    sq = ((2, 3, 32, 32), (3, 3, 32, 32), (1, 3, 64, 64))  # a fixed position table: the same module changes its batch only
    waves = ((2, 4000), (3, 5000), (1, 4400))
    mels = ((2, 80, 40), (3, 80, 56), (1, 80, 24))
    toks = ((2, 9), (3, 13), (1, 6))
    rect = ((2, 3, 64, 64), (3, 3, 96, 64), (1, 3, 64, 128))

    def encodec(k=0):
        return audio.EnCodec(1, "weight_norm", True, 4, False)

    def t5(k=0):
        return text.T5Model(300, 128, 2, 2, 256)

    def whisper(k=0):
        return audio2text.Whisper(300, 2, 128)

    def hidden(tag, shapes):  # (B, L, d) activations, then (B, S, d) memory where there is one
        return lambda k, seed: tuple(synth_input(f"graph_{tag}{i}", s, seed) for i, s in enumerate(shapes[k]))

    def whisper_dec(k, seed):
        (B, L), S = toks[k], mels[k][2] // 2
        return synth_tokens("graph_wdec", (B, L), 300, seed), synth_input("graph_wdec_mem", (B, S, 128), seed)

    def whisper_full(k, seed):
        return synth_input("graph_whisper", mels[k], seed), synth_tokens("graph_whisper", toks[k], 300, seed)

    def t5_full(k, seed):
        (B, S) = toks[k]
        return synth_tokens("graph_t5_src", (B, S), 300, seed), synth_tokens("graph_t5_tgt", (B, S - 4), 300, seed)

    def wave_lengths(k):
        return torch.tensor([waves[k][1] - 500 * b for b in range(waves[k][0])])

    def tok_lengths(k):
        return torch.tensor([toks[k][1] - b for b in range(toks[k][0])])

    return {
        # ---- image
        "ViT": Model("ViT", lambda k: image.ViT(2, 128, 2, 8, img_size=sq[k][-1]), _img("vit", sq), dtypes=both),
        "MLPMixer": Model("MLPMixer", lambda k: image.MLPMixer(2, 64, 8, img_size=sq[k][-1]), _img("mixer", sq), dtypes=both),
        # (warmup=1: the mixer kernel raises its dynamic-LDS limit at its first launch, which must fall in front of the capture)
        "MLPMixer:warmup1": Model("MLPMixer", lambda k: image.MLPMixer(2, 64, 8, img_size=sq[k][-1]), _img("mixer1", sq), warmup=1),
        "ConvNeXt": Model("ConvNeXt", lambda k: image.ConvNeXt(32, (1, 1, 1, 1)), _img("convnext", rect), dtypes=both),
        "MaxViT": Model("MaxViT", lambda k: image.MaxViT(32, [1, 1, 2, 1], [32, 64, 96, 128]),
                        _img("maxvit", ((2, 3, 224, 224), (1, 3, 224, 448), (1, 3, 448, 224))), dtypes=both),
        "MobileViT": Model("MobileViT", lambda k: image.MobileViT.from_apple("xxs"), _img("mobile_vit", ((2, 3, 64, 64), (3, 3, 128, 64), (1, 3, 64, 128)))),
        "DETR": Model("DETR", lambda k: image.DETR([1, 1, 1, 1]), _img("detr", rect)),  # a tuple: (logits, boxes)
        # ---- audio
        "Wav2Vec2": Model("Wav2Vec2", lambda k: audio.Wav2Vec2(2, 64), _img("w2v", waves), lengths=wave_lengths),
        "Wav2Vec2:hubert": Model("Wav2Vec2", lambda k: audio.Wav2Vec2(2, 128, stem_bias=False, stem_legacy=True, pre_norm=False), _img("hubert", waves)),
        "Data2VecAudio": Model("Data2VecAudio", lambda k: audio.Data2VecAudio(2, 128), _img("d2v", waves)),
        "SEW": Model("SEW", lambda k: audio.SEW(2, 128), _img("sew", waves)),
        "Wav2Vec2CTC": Model("Wav2Vec2CTC", lambda k: audio.Wav2Vec2CTC(audio.Wav2Vec2(1, 128), 32, blank=31), _img("ctc", waves),
                             lengths=wave_lengths),
        "EnCodecEncoder": Model("EnCodecEncoder", lambda k: encodec().encoder, _img("enc_e", ((2, 1, 3200), (1, 1, 4800), (3, 1, 2560))),
                                dtypes=("fp32",)),
        "EnCodecDecoder": Model("EnCodecDecoder", lambda k: encodec().decoder, _img("enc_d", ((2, 128, 10), (1, 128, 15), (3, 128, 8))),
                                dtypes=("fp32",)),
        "EnCodec.encode": Model("EnCodec", encodec, _img("enc_q", ((2, 1, 3200), (1, 1, 4800), (3, 1, 2560))), dtypes=("fp32",),
                                method="encode"),  # the quantiser: int64 codes (and None for the scale)
        "EnCodec.decode": Model("EnCodec", encodec, _tok("enc_codes", ((2, 4, 10), (1, 4, 15), (3, 4, 8)), 1024), dtypes=("fp32",),
                                method="decode"),
        # ---- audio2text
        "WhisperPreprocessor": Model("WhisperPreprocessor", lambda k: audio2text.WhisperPreprocessor(),
                                     lambda k, s: (synth_input("graph_pre", ((2, 4000), (1, 8000), (3, 1600))[k], s, scale=0.1),), dtypes=("fp32",)),
        "WhisperEncoder": Model("WhisperEncoder", lambda k: whisper().encoder, _img("wenc", mels), cast=(0,), dtypes=both),
        "WhisperDecoder": Model("WhisperDecoder", lambda k: whisper().decoder, whisper_dec, cast=(1,), dtypes=both),
        "Whisper": Model("Whisper", whisper, whisper_full, cast=(0,), dtypes=both),
        # ---- text
        "BERT": Model("BERT", lambda k: text.BERT(300, 2, 128), _tok("bert", toks, 300), dtypes=both, lengths=tok_lengths),
        "GPT": Model("GPT", lambda k: text.GPT(2, 128), _tok("gpt", toks, 1000), dtypes=both),
        "GPT2": Model("GPT2", lambda k: text.GPT2(2, 128), _tok("gpt2", toks, 50257), dtypes=both),
        "T5Encoder": Model("T5Encoder", lambda k: t5().encoder, hidden("t5e", (((2, 9, 128),), ((3, 13, 128),), ((1, 6, 128),))), cast=(0,)),
        "T5Decoder": Model("T5Decoder", lambda k: t5().decoder,
                           hidden("t5d", (((2, 5, 128), (2, 9, 128)), ((3, 7, 128), (3, 13, 128)), ((1, 3, 128), (1, 6, 128)))), cast=(0, 1)),
        "T5Model": Model("T5Model", t5, t5_full, lengths=tok_lengths),
    }


MODELS = _models()

NOT_GRAPHED = {
    "DETRPipeline": "builds Python lists of class names and boxes from the detections on the host (DETR itself is replayed)",
    "DecoderGenerator": "not a module: a tokenizer loop around generate()",
    "DecoderGenerator.generate": "a tokenizer loop around the model's generate(), which owns its graph",
    "GPT2.generate": "KV-cached decoding owns its captured step and its tests (tests/test_hip_decode.py)",
    "WhisperDecoder.generate": "KV-cached decoding owns its captured step and its tests (tests/test_hip_decode.py, test_hip_beam.py)",
    "Whisper.generate": "WhisperDecoder.generate behind the encoder",
    "audio2text.generate": "the module of the decoders: they own their captured step and its tests",
    "T5Model.generate": "owns its captured decode state and its tests (tests/test_hip_t5_generate.py)",
    "GPT.score": "takes lengths=: read on the host to build the ignore mask",
    "GPT2.score": "takes lengths=: read on the host to build the ignore mask",
    "WhisperDecoder.score": "takes lengths=: read on the host to build the ignore mask",
    "Whisper.score": "WhisperDecoder.score behind the encoder",
    "T5Model.score": "takes lengths= / src_lengths=: read on the host",
    "T5Model.encode": "takes lengths=: seq_lens reads them on the host and uploads cu_seqlens (without lengths it is T5Encoder, replayed)",
    "BERT.embed": "takes lengths=: seq_lens reads them on the host and uploads cu_seqlens",
    "WhisperDecoder.align": "uploads its counts and head tables and back-traces the DTW path on the host",
    "Whisper.align": "WhisperDecoder.align behind the encoder",
    # the forwards that ALSO take lengths: replayed without them (MODELS), refused with them
    "BERT.forward(lengths)": "seq_lens reads the lengths on the host and uploads cu_seqlens",
    "Wav2Vec2.forward(lengths)": "seq_lens reads the lengths on the host and uploads cu_seqlens",
    "Wav2Vec2CTC.forward(lengths)": "seq_lens reads the lengths on the host and uploads cu_seqlens",
    "T5Model.forward(lengths)": "src_lengths: seq_lens reads them on the host and uploads cu_seqlens",
}

ENTRY_WORDS = ("forward", "generate", "generate_ids", "generate_batch", "score", "align", "decode", "encode", "embed", "log_probs")


def flat(res) -> list:
    """the tensors of a model's result, named by position (None entries - EnCodec.encode's scale - dropped)"""
    res = res if isinstance(res, (tuple, list)) else (res,)
    return [(f"output {i}", t) for i, t in enumerate(res) if isinstance(t, Tensor)]
