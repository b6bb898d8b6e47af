"""The launch list of a decode step as text, one line per launch: the kernel's name and every argument.

A decode step is nothing but its launch list (pytorch_models/_hip/decode_plan.py), so two builds whose plans print the same text
run the same step.  An argument is printed verbatim unless its slot in _hip.SIGNATURES is a pointer; a pointer is printed as
``s<k>+<byte offset>`` where s<k> is the k-th distinct tensor storage in order of first appearance in the list, found among the
tensors the decoder keeps alive: its attributes, lists and tuples of tensors in them, and ``_keep``.  A pointer into no such
storage would dangle once its tensor is freed: render() raises on it, naming the launch and the argument.  The persistent path's
device table (``table``) is read back and printed record by record the same way.

    python tools/decode_plan.py [--out plan.txt] [case ...]      # every case of CASES by default

With a model given, plan() also resolves pointers into the model's own tensors (marked as not kept) instead of failing, so the
plans of a build that forgot to keep one can still be printed and compared; the command line reports them and exits 1.
tests/test_hip_decode_plan.py asserts that no case has any.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "pytorch-models_amd")) if p not in sys.path]
import torch  # noqa: E402
from torch import Tensor, nn  # noqa: E402

from pytorch_models import _hip  # noqa: E402


def _tensors(obj, depth: int = 0):
    if isinstance(obj, Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)) and depth < 3:
        for o in obj:
            yield from _tensors(o, depth + 1)


def kept_tensors(dec):
    """the tensors reachable from the decoder object: attributes, lists and tuples of tensors in them, ``_keep``"""
    for v in vars(dec).values():
        yield from _tensors(v)


def model_tensors(model: nn.Module):
    """parameters, buffers and the tensors derived from them (transformer.derived) of every submodule"""
    for m in model.modules():
        yield from m.parameters(recurse=False)
        yield from m.buffers(recurse=False)
        for hit in m.__dict__.get("_pm_derived", {}).values():
            yield from _tensors(hit[1])


class _Storages:
    def __init__(self, dec, model) -> None:
        self.spans = {}  # base address -> (bytes, kept)
        for kept, ts in ((True, kept_tensors(dec)), (False, model_tensors(model) if model is not None else ())):
            for t in ts:
                st = t.untyped_storage()
                if st.nbytes() and (st.data_ptr() not in self.spans or st.nbytes() > self.spans[st.data_ptr()][0]):
                    self.spans[st.data_ptr()] = (st.nbytes(), kept or self.spans.get(st.data_ptr(), (0, False))[1])
        self.names = {}
        self.dangling = []

    def name(self, p: int | None, where: str) -> str:
        if p is None or p == 0:
            return "null"
        for base, (size, kept) in self.spans.items():
            if base <= p < base + size:
                if not kept:
                    self.dangling.append(where)
                return f"s{self.names.setdefault(base, len(self.names))}+{p - base}"
        raise LookupError(f"{where}: pointer {p:#x} lies in no tensor the decoder keeps alive")


def plan(dec, model: nn.Module | None = None) -> tuple[list[str], list[str]]:
    """(lines, dangling): the plan's text, and the (launch, argument) places whose pointer resolves only into ``model``'s tensors"""
    st = _Storages(dec, model)
    sigs = {**_hip.SIGNATURES, **_hip.EXPERIMENT_SIGNATURES}
    lines = []
    for i, (fn, args) in enumerate(dec.launches):
        name = fn.__name__
        argtypes = sigs[name][0]
        assert len(argtypes) == len(args), f"launch {i} {name}: {len(args)} arguments for {len(argtypes)} parameters"
        lines.append(f"{name}(" + ", ".join(st.name(a, f"launch {i} {name} argument {j}") if t is ctypes.c_void_p else repr(a)
                                            for j, (t, a) in enumerate(zip(argtypes, args))) + ")")
        if name == "pm_dec_layers":  # the layers' records live on the device: read them back
            raw = bytes(dec.table.cpu().numpy())
            for k in range(len(raw) // ctypes.sizeof(_hip.DecLayer)):
                rec = _hip.DecLayer.from_buffer_copy(raw, k * ctypes.sizeof(_hip.DecLayer))
                lines.append(f"  layer {k}: " + ", ".join(
                    f"{f}=" + (st.name(getattr(rec, f), f"launch {i} {name} layer {k} field {f}") if t is ctypes.c_void_p
                               else repr(getattr(rec, f))) for f, t in _hip.DecLayer._fields_))
    return lines, st.dangling


def render(dec) -> str:
    """the plan's text; LookupError if a pointer of it lies outside every tensor the decoder keeps alive"""
    return "\n".join(plan(dec)[0]) + "\n"


# ---- the decoder forms: tiny synthetic models, the smallest shapes that reach every branch of the plan builders ----
# Filled and rounded as the decode tests fill theirs (synthweights), but not built by tests/beam_cases.py, tests/ckpt_synth.py or
# tests/t5_generate_cases.py: those fix the geometry (Whisper(1000, 2, 128) with its 4 x d MLP, T5 at d = 512 and MLP 1024 only),
# and the plan's branches turn on what they fix - an MLP of 1024 at d = 128 for the K-split and fc2-parts launches, 256 for none,
# 9 and 5 heads, a decoder-only stack.  The T5 forms are the same T5Model(*geometry) call as t5_generate_cases.build.
class TinyDecoder(nn.Module):
    """the attributes GreedyDecoder reads of a WhisperDecoder (``cross``) or a GPT-2 (decoder-only), with a free MLP width"""
    max_seq_len = 16

    def __init__(self, vocab: int, n_layers: int, d: int, hid: int, cross: bool) -> None:
        from pytorch_models.transformer import Decoder, LayerNorm

        super().__init__()
        self.token_embs = nn.Embedding(vocab, d)
        self.pos_embs = nn.Parameter(torch.zeros(self.max_seq_len, d))
        self.layers = Decoder(n_layers, d, cross_attn=cross, mlp_ratio=hid / d, act="gelu" if cross else "approximate_gelu")
        self.norm = LayerNorm(d)


VOCAB, P, N_NEW, S = 300, 2, 3, 24


def _speech(B: int, d: int = 128, hid: int = 1024, cross: bool = True, f32_memory: bool = False):
    from synthweights import bf16_round_, fill_module, synth_input, synth_tokens

    dec = TinyDecoder(VOCAB, 2, d, hid, cross).eval()
    fill_module(dec, 5)
    bf16_round_(dec)
    dec = dec.to(torch.bfloat16).cuda()
    memory = synth_input("plan_mem", (B, S, d), 6).to(torch.float32 if f32_memory else torch.bfloat16).cuda() if cross else None
    return dec, memory, synth_tokens("plan_prompt", (B, P), VOCAB, 7).cuda()


def _with_rules(kw: dict) -> dict:
    """rules=True -> a WhisperRules inside the tiny vocabulary"""
    from pytorch_models.audio2text.generate import WhisperRules

    if kw.get("rules") is True:
        kw = dict(kw, rules=WhisperRules(eot=200, timestamp_begin=250, no_timestamps=249, max_initial_timestamp=10, suppress=(3, 17),
                                         blank=(5, 200)))
    return kw


def _greedy(B: int = 3, env: dict | None = None, model: dict | None = None, **kw):
    def build(setenv):
        from pytorch_models.audio2text.generate import GreedyDecoder

        for k, v in (env or {}).items():
            setenv(k, v)
        dec, memory, prompt = _speech(B, f32_memory=kw.get("kv32", False), **(model or {}))
        return GreedyDecoder(dec, memory, prompt, N_NEW, **_with_rules(kw)), dec

    return build


def _beam(**kw):
    def build(setenv):
        from pytorch_models.audio2text.generate import BeamDecoder

        dec, memory, prompt = _speech(2, f32_memory=kw.get("kv32", False))
        return BeamDecoder(dec, memory, prompt, N_NEW, 3, **_with_rules(kw)), dec

    return build


def _t5(B: int, heads: int = 2, mlp: int = 1024, **kw):
    def build(setenv):
        from pytorch_models.text import T5Model
        from pytorch_models.text.t5_generate import T5DecodeState
        from synthweights import bf16_round_, fill_module

        m = T5Model(VOCAB, 128, heads, 1, mlp).eval()
        fill_module(m, 9)
        bf16_round_(m)
        m = m.to(torch.bfloat16).cuda()
        return T5DecodeState(m, B, S, 1, N_NEW, **kw), m

    return build


# name -> build(setenv) -> (decoder, model); setenv(name, value) sets an environment switch for the build (the constructors
# read them) - os.environ.__setitem__ from the command line, monkeypatch.setenv from the test
CASES = {
    "whisper_chain": _greedy(),  # the default: fused blocks chained by deferred sums, K-split fc2 left as parts
    "whisper_no_chain": _greedy(env={"PM_DEC_CHAIN": "0"}),
    "whisper_unfused": _greedy(fused=False),
    "whisper_kv32": _greedy(kv32=True),
    "whisper_kv32_no_chain": _greedy(kv32=True, env={"PM_DEC_CHAIN": "0"}),  # pm_dec_attention_fused_kv32
    "whisper_topk4": _greedy(topk=4),
    "whisper_sample": _greedy(topk=0, temperature=0.7, top_p=0.9, return_logprobs=True, rules=True),  # pm_dec_sample: the log-prob buffer
    "whisper_logprobs": _greedy(return_logprobs=True),  # the arg-max of the defaults through the sampling tail
    "whisper_rules": _greedy(rules=True),
    "whisper_eos": _greedy(eos=200, margins=True),  # pm_dec_finish behind the default tail: the finished flags
    "whisper_controls": _greedy(rules=True, eos=200, min_new_tokens=2, repetition_penalty=1.3, no_repeat_ngram_size=2,
                                return_logprobs=True),  # pm_dec_controls in front of the rules, pm_dec_finish with the log-prob buffer
    "gpt2_ragged_controls": _greedy(model=dict(cross=False), lengths=(2, 1, 2), eos=5, no_repeat_ngram_size=2),  # key_start in the controls
    "whisper_margins": _greedy(margins=True),
    "whisper_mlp256": _greedy(model=dict(hid=256)),  # no K-split anywhere
    "gpt2_d128": _greedy(model=dict(cross=False)),
    "gpt2_d576": _greedy(model=dict(cross=False, d=576, hid=2304)),  # 9 heads: the final norm as its own launch
    "whisper_b64_h5": _greedy(B=64, model=dict(d=320, hid=1280)),  # B * n_heads > 256: the unfused self block
    "beam3": _beam(),
    "beam3_rules": _beam(rules=True),
    "beam3_kv32": _beam(kv32=True),
    "t5_b3": _t5(3),
    "t5_b33_h8": _t5(33, heads=8),  # B * n_heads > 256
    "t5_logits": _t5(3, return_logits=True),
    "t5_mlp256": _t5(3, mlp=256),  # GEGLU width < 1024: no K-split
    "whisper_persistent": _greedy(path="persistent"),  # the experiments build only
}


def needs_experiments(case: str) -> bool:
    return case.endswith("_persistent")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    text, bad = [], 0
    for case in args.cases:
        if needs_experiments(case) and not _hip.has_experiments():
            print(f"{case}: skipped (the experiments build only)", file=sys.stderr)
            continue
        before = {}  # the switches this case sets, and what they were

        def setenv(name, value):
            before.setdefault(name, os.environ.get(name))
            os.environ[name] = value

        dec, model = CASES[case](setenv)
        for name, old in before.items():
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old
        lines, dangling = plan(dec, model)
        text += [f"== {case}: path {getattr(dec, 'path', 'launches')}, {len(dec.launches)} launches"] + lines
        for where in dangling:
            bad += 1
            print(f"{case}: {where}: the decoder does not keep this tensor alive", file=sys.stderr)
    out = "\n".join(text) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out)
    else:
        sys.stdout.write(out)
    sys.exit(1 if bad else 0)
