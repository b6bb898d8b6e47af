"""Empty-batch contract: what every wrapper of pytorch_models/_hip/ops.py and every model entry point does
with an extent of 0, as one table built on wrapper_cases.ROWS and graph_cases.MODELS.

``Tensor.data_ptr()`` of a tensor without elements is null on every device, and every C entry point's first line refuses a null
pointer, in front of its own ``if (M == 0) return PM_OK``.  So the decision belongs to the wrapper, and it is one of two:

  "empty"   the call returns tensors of the shape, dtype and device the non-empty call returns, with the zeroed extent 0; a
            caller's ``out=`` (``lse_out=``, ``best_out=`` ...) is the returned object; every operand is bit-unchanged; the
            library is not called;
  "refuse"  the call raises ValueError (ops._need's type - not check()'s RuntimeError, not an error of torch's own) whose
            message names the wrapper, before any library call and with no operand modified.

Every extent is a COUNT (independent rows or problems: honoured - except in the decode-step family, whose state the launch plan
allocates per batch and whose C entries refuse rows <= 0), an INNER extent (reduced over or laid out by: refused) or the size of
one SAMPLE (H, W, a waveform's length: either, stated per row; refused everywhere today).

AXES[row id] lists the row's axes: ``ax(name, kind, "operand:dim ...", ints, seq=..., ws=..., res=...)``.  ``shrink(kw)`` is the
canonical call with every listed tensor dimension and integer argument 0, SeqLens and workspaces rebuilt by the project's own
helpers.  The CPU stage checks that every dimension of every tensor operand of every row is zeroed by some axis or listed in
EXEMPT_DIMS with its reason.  MUTANTS are wrappers broken on purpose; MODEL_EMPTY is the same table one level up."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable

import torch
from torch import Tensor

import graph_cases as GC
import wrapper_cases as WC

KINDS = ("count", "inner", "sample")
DECODE_FAMILY = ("dec_linear", "dec_linear_ksplit", "dec_argmax", "dec_attention", "dec_attention_ragged", "dec_embed_ragged",
                 "dec_next_token", "dec_sample_topk", "dec_whisper_rules", "dec_beam_topw", "dec_beam_select", "dec_beam_reorder")
DECODE_WHY = "decode-step family: its state (caches, tickets, K-split workspace) is allocated per batch and the C entry refuses rows <= 0"


def _ops():
    from pytorch_models._hip import ops
    return ops


def _paths(spec: str) -> tuple:
    """"x:0 w_ih[1]:1" -> (((\"x\",), 0), ((\"w_ih\", 1), 1))"""
    out = []
    for item in spec.split():
        m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?:(\d+)", item)
        assert m, item
        out.append(((m.group(1),) if m.group(2) is None else (m.group(1), int(m.group(2))), int(m.group(3))))
    return tuple(out)


@dataclass
class Axis:
    name: str
    kind: str                       # "count" | "inner" | "sample"
    dims: tuple                     # ((operand path, dimension), ...): zeroed together
    ints: dict = field(default_factory=dict)
    outcome: str = ""               # "empty" | "refuse"
    res: tuple | None = None        # "empty": the shapes of the results, in wrapper_cases.flat_outputs order
    seq: tuple | None = None        # (lengths, L): kw["seq"] rebuilt by ops.seq_lens
    ws: Callable | None = None      # ops -> byte count: kw["ws"] rebuilt at that size
    why: str = ""                   # the reason of a refused count axis

    def shrink(self, kw: dict) -> dict:
        zero: dict = {}
        for path, d in self.dims:
            zero.setdefault(path, set()).add(d)
        dev = next(t.device for _, t in WC.operands(kw))
        for path, ds in zero.items():
            t = WC.get(kw, path)
            kw = WC.replaced(kw, path, t.new_empty([0 if i in ds else n for i, n in enumerate(t.shape)]))
        kw = {**kw, **self.ints}
        if self.seq is not None:
            kw["seq"] = _ops().seq_lens(list(self.seq[0]), self.seq[1], dev)
        if self.ws is not None:
            kw["ws"] = torch.zeros(max(int(self.ws(_ops())), 0), dtype=torch.uint8, device=dev)
        return kw


def ax(name, kind, dims="", ints=None, *, res=None, seq=None, ws=None, outcome=None, why="") -> Axis:
    assert kind in KINDS, kind
    outcome = outcome or ("empty" if kind == "count" else "refuse")
    assert (res is not None) == (outcome == "empty"), (name, "an honoured axis states its result shapes")
    return Axis(name, kind, _paths(dims), dict(ints or {}), outcome, res, seq, ws, why)


def dec(name, dims, ints=None) -> Axis:
    """a count axis of the decode-step family: refused, with the family's reason"""
    return ax(name, "count", dims, ints, outcome="refuse", why=DECODE_WHY)


def _gemm(M, N, x="x", out=True, extra_m="", extra_n=""):
    o0, o1 = (" out:0", " out:1") if out else ("", "")
    return [ax("M", "count", f"{x}:0 resid:0{o0}{extra_m}", res=((0, N),)), ax("K", "inner", f"{x}:1 w:1"),
            ax("N", "inner", f"w:0 bias:0 resid:1{o1}{extra_n}")]


def _attn(D, Lq, out):
    o = (" out:0", " out:1", " out:2") if out else ("", "", "")
    return [ax("B", "count", "q:0 k:0 v:0 bias:0" + o[0], res=((0, Lq, D),)), ax("Lq", "count", "q:1 bias:2" + o[1], res=((2, 0, D),)),
            ax("Lk", "inner", "k:1 v:1 bias:3"), ax("D", "inner", "q:2 k:2 v:2" + o[2]), ax("H", "inner", "bias:1", {"n_heads": 0})]


def _embed(B_extra="", out=True, dtype_rows=32):
    o = (" out:0", " out:1", " out:2") if out else ("", "", "")
    return [ax("B", "count", "tokens:0" + B_extra + o[0], res=((0, 5, dtype_rows),)), ax("L", "count", "tokens:1" + o[1], res=((2, 0, dtype_rows),)),
            ax("V", "inner", "emb:0"), ax("d", "inner", "emb:1 pos:1" + o[2]), ax("positions", "inner", "pos:0")]


_TAIL_B = "prompt:0 tok_cur:0 tokens:0"
_TAIL = [ax("P", "inner", "prompt:1"), ax("V", "inner", "emb:0"), ax("d", "inner", "emb:1 pos_tab:1"), ax("positions", "inner", "pos_tab:0"),
         ax("pos", "inner", "pos:0"), ax("ticket", "inner", "ticket:0")]
_ALIGN_B = "q:0 k:0 lengths:0 frames:0"
_Z2 = ((0, 0), 6)   # every length 0
_B0 = ((), 6)       # no sequence at all
_CTC_B = "logp:0 targets:0 target_lengths:0"

AXES: dict[str, list[Axis]] = {
    "ln_stats_finalize": [ax("M", "count", "partials:0", res=((0, 2),)), ax("N", "inner", "partials:1", {"N": 0}), ax("pair", "inner", "partials:2")],
    "linear": _gemm(16, 64),
    "linear:ln_fold": [ax("M", "count", "x:0 ln_stats:0", res=((0, 64),)), ax("K", "inner", "x:1 w:1"), ax("N", "inner", "w:0 bias:0 ln_s:0"),
                       ax("pair", "inner", "ln_stats:1")],
    "linear_f32": _gemm(6, 12),
    "attention_f32": _attn(32, 3, False),
    "layernorm": [ax("M", "count", "x:0 resid:0 out:0", res=((0, 64),)), ax("d", "inner", "x:1 gamma:0 beta:0 resid:1 out:1")],
    "layernorm:plain": [ax("M", "count", "x:0", res=((0, 64),)), ax("d", "inner", "x:1 gamma:0 beta:0")],
    "rmsnorm": [ax("M", "count", "x:0", res=((0, 64),)), ax("d", "inner", "x:1 gamma:0")],
    "geglu": [ax("M", "count", "h:0", res=((0, 16),)), ax("F", "inner", "h:1")],
    "attention": _attn(192, 5, True),
    "conv2d_nhwc": [ax("N", "count", "x:0 resid:0", res=((0, 5, 6, 12),)), ax("H", "sample", "x:1 resid:1"), ax("W", "sample", "x:2 resid:2"),
                    ax("Cin", "inner", "x:3 w:3"), ax("Cout", "inner", "w:0 bias:0 resid:3"), ax("kh", "inner", "w:1"), ax("kw", "inner", "w:2")],
    "mean_rows": [ax("N", "count", "x:0", res=((0, 8),)), ax("R", "inner", "x:1"), ax("C", "inner", "x:2")],
    "vit_tokens": [ax("N", "count", "imgs:0", res=((0, 7, 192),)), ax("channels", "inner", "imgs:1"), ax("H", "sample", "imgs:2 pe:0"),
                   ax("W", "sample", "imgs:3 pe:0"), ax("d", "inner", "w2d:0 bias:0 pe:1 cls:0"), ax("K", "inner", "w2d:1")],
    "linear_strided": [ax("M", "count", "x:0 resid:0 out:0", {"M": 0}, res=((0, 32),)), ax("rows", "sample", "x:1"), ax("columns", "sample", "x:2"),
                       ax("K", "inner", "w:1", {"K": 0}), ax("N", "inner", "w:0 bias:0 resid:1 out:1")],
    "w2v_stem0": [ax("B", "count", "x:0", res=((0, 17, 16),)), ax("L", "sample", "x:1"), ax("C0", "inner", "w:0 bias:0 gamma:0 beta:0"),
                  ax("k", "inner", "w:1")],
    "group_windows": [ax("B", "count", "x:0", res=((0, 4, 9, 8),)), ax("T", "sample", "x:1"), ax("d", "inner", "x:2")],
    "grouped_conv": [ax("B", "count", "xg:0 resid:0", res=((0, 12),)), ax("G", "inner", "xg:1 w:0 bias:0 resid:1"), ax("Tp", "sample", "xg:2 resid:0"),
                     ax("cgp", "inner", "xg:3"), ax("cg", "inner", "w:1 bias:0 resid:1", {"cg": 0}), ax("Kp", "inner", "w:2")],
    "avgpool_time2": [ax("B", "count", "x:0", res=((0, 3, 8),)), ax("T", "sample", "x:1"), ax("d", "inner", "x:2")],
    "stft_mel": [ax("B", "count", "x:0", res=((0, 6, 24),)), ax("n_frames", "count", "", {"n_frames": 0}, res=((2, 6, 0),)), ax("T", "sample", "x:1"),
                 ax("tables", "inner", "tables[0]:0 tables[1]:0"), ax("n_mels", "inner", "csr[0]:0", {"n_mels": 0}),
                 ax("nnz", "inner", "csr[1]:0 csr[2]:0")],
    "whisper_stem1": [ax("B", "count", "x:0", res=((0, 14, 32),)), ax("C", "inner", "x:1"), ax("T", "sample", "x:2"), ax("d", "inner", "w1:0 b1:0"),
                      ax("K", "inner", "w1:1")],
    "embed_tokens": _embed(),
    "embed_tokens:f32_table": _embed(out=False),
    "dec_linear": [dec("M", "x:0 resid:0"), ax("K", "inner", "x:1 w:1 ln[0]:0 ln[1]:0"), ax("N", "inner", "w:0 bias:0 resid:1")],
    "dec_linear_ksplit": [dec("M", "x:0 resid:0"), ax("K", "inner", "x:1 w:1"), ax("N", "inner", "w:0 bias:0 resid:1")],
    "dec_argmax": [dec("M", "x:0"), ax("K", "inner", "x:1 w:1 ln[0]:0 ln[1]:0"), ax("N", "inner", "w:0")],
    "dec_attention": [dec("B", "q:0 k:0 v:0"), ax("H", "inner", "q:1 k:1 v:1"), ax("T", "inner", "k:2 v:2"), ax("hd", "inner", "k:3 v:3")],
    "prefill_attention": [ax("B", "count", "qkv:0 kc:0 vc:0 out:0", res=((0, 192),)), ax("H", "inner", "qkv:1 kc:1 vc:1 out:1", {"n_heads": 0}),
                          ax("T", "inner", "kc:2 vc:2"), ax("hd", "inner", "kc:3 vc:3")],
    "dec_attention_ragged": [dec("B", "q:0 k:0 v:0 key_start:0"), ax("H", "inner", "q:1 k:1 v:1"), ax("T", "inner", "k:2 v:2"),
                             ax("hd", "inner", "k:3 v:3")],
    "prefill_attention_ragged": [ax("B", "count", "qkv:0 kc:0 vc:0 out:0 key_start:0", res=((0, 192),)),
                                 ax("H", "inner", "qkv:1 kc:1 vc:1 out:1", {"n_heads": 0}), ax("T", "inner", "kc:2 vc:2"), ax("hd", "inner", "kc:3 vc:3")],
    "embed_tokens_ragged": _embed(" key_start:0"),
    "dec_embed_ragged": [dec("B", "tok_cur:0 key_start:0"), ax("V", "inner", "emb:0"), ax("d", "inner", "emb:1 pos_tab:1"),
                         ax("positions", "inner", "pos_tab:0"), ax("pos", "inner", "pos:0")],
    "dec_next_token": [dec("B", "ws_val:0 ws_idx:0 margins:0 key_start:0 " + _TAIL_B), ax("tiles", "inner", "ws_val:1 ws_idx:1"),
                       ax("Ttot", "inner", "tokens:1 margins:1"), *_TAIL],
    "dec_next_token:plain": [dec("B", "ws_val:0 ws_idx:0 margins:0 " + _TAIL_B), ax("tiles", "inner", "ws_val:1 ws_idx:1"),
                             ax("Ttot", "inner", "tokens:1 margins:1"), *_TAIL],
    "dec_sample_topk": [dec("B", "logits:0 key_start:0 " + _TAIL_B), ax("vocabulary", "inner", "logits:1"), ax("Ttot", "inner", "tokens:1"), *_TAIL],
    "dec_sample_topk:plain": [dec("B", "logits:0 " + _TAIL_B), ax("vocabulary", "inner", "logits:1"), ax("Ttot", "inner", "tokens:1"), *_TAIL],
    "dec_whisper_rules": [dec("B", "logits:0 tokens:0"), ax("V", "inner", "logits:1"), ax("Ttot", "inner", "tokens:1"), ax("pos", "inner", "pos:0")],
    "dec_beam_topw": [dec("B", "logits:0 scores:0 finished:0"), ax("W", "inner", "logits:0 scores:1 finished:1"), ax("V", "inner", "logits:1"),
                      ax("pos", "inner", "pos:0")],
    "dec_beam_select": [dec("B", "cand_score:0 cand_tok:0 scores:0 finished:0 parents:0 tokens:0 prompt:0 tok_cur:0 x:0"),
                        ax("W", "inner", "cand_score:0 cand_score:1 cand_tok:0 cand_tok:1 scores:1 finished:1 parents:1 tokens:0 prompt:0 tok_cur:0 x:0"),
                        ax("Ttot", "inner", "tokens:1"), ax("P", "inner", "prompt:1"), ax("V", "inner", "emb:0"), ax("d", "inner", "emb:1 pos_tab:1 x:1"),
                        ax("positions", "inner", "pos_tab:0"), ax("pos", "inner", "pos:0"), ax("ticket", "inner", "ticket:0")],
    "dec_beam_reorder": [dec("B", "caches[0]:0 caches[1]:0 parents:0"), ax("W", "inner", "caches[0]:0 caches[1]:0 parents:1"),
                         ax("H", "inner", "caches[0]:1 caches[1]:1"), ax("Tmax", "inner", "caches[0]:2 caches[1]:2"),
                         ax("hd", "inner", "caches[0]:3 caches[1]:3"), ax("pos", "inner", "pos:0")],
    "dwconv7_ln": [ax("N", "count", "x:0", res=((0, 64),)), ax("H", "sample", "x:1"), ax("W", "sample", "x:2"),
                   ax("C", "inner", "x:3 w:2 bias:0 gamma:0 beta:0"), ax("kh", "inner", "w:0"), ax("kw", "inner", "w:1")],
    "ln_space_to_depth": [ax("N", "count", "x:0", res=((0, 64),)), ax("H", "sample", "x:1"), ax("W", "sample", "x:2"),
                          ax("C", "inner", "x:3 gamma:0 beta:0")],
    "convnext_stem": [ax("N", "count", "imgs:0", res=((0, 2, 3, 16),)), ax("channels", "inner", "imgs:1"), ax("H", "sample", "imgs:2"),
                      ax("W", "sample", "imgs:3"), ax("d", "inner", "wt:1 bias:0 gamma:0 beta:0"), ax("K", "inner", "wt:0")],
    "mean_ln": [ax("N", "count", "x:0", res=((0, 8),)), ax("HW", "inner", "x:1"), ax("C", "inner", "x:2 gamma:0 beta:0")],
    "window_attention": [ax("N", "count", "q:0 k:0 v:0 out:0", {"N": 0}, res=((0, 96),)), ax("H", "sample", "q:0 k:0 v:0 out:0", {"H": 0}),
                         ax("W", "sample", "q:0 k:0 v:0 out:0", {"W": 0}), ax("width", "inner", "q:1 k:1 v:1 out:1"),
                         ax("heads", "inner", "bias:0", {"n_heads": 0}), ax("window", "inner", "bias:1 bias:2", {"ws": 0})],
    "dwconv3_bn_act": [ax("N", "count", "x:0 gate:0", res=((0, 5, 6, 8), (0, 5, 8))), ax("H", "sample", "x:1"), ax("W", "sample", "x:2"),
                       ax("C", "inner", "x:3 w:2 scale:0 shift:0 gate:1"), ax("kh", "inner", "w:0"), ax("kw", "inner", "w:1")],
    "se_gate": [ax("N", "count", "psum:0", res=((0, 8),)), ax("T", "inner", "psum:1"), ax("C", "inner", "psum:2 w1:1 w2:0 b2:0"),
                ax("R", "inner", "w1:0 b1:0 w2:1")],
    "maxvit_stem": [ax("N", "count", "imgs:0", res=((0, 4, 6, 16),)), ax("channels", "inner", "imgs:1"), ax("H", "sample", "imgs:2"),
                    ax("W", "sample", "imgs:3"), ax("d", "inner", "wt:1 shift:0"), ax("K", "inner", "wt:0")],
    "im2col3x3": [ax("N", "count", "x:0", res=((0, 128),)), ax("H", "sample", "x:1"), ax("W", "sample", "x:2"), ax("C", "inner", "x:3")],
    "avgpool2x2": [ax("N", "count", "x:0", res=((0, 2, 3, 8),)), ax("H", "sample", "x:1"), ax("W", "sample", "x:2"), ax("C", "inner", "x:3")],
    "conv_bf16": [ax("N", "count", "x:0 resid:0", res=((0, 3, 5, 16),)), ax("H", "sample", "x:1 resid:1"), ax("W", "sample", "x:2 resid:2"),
                  ax("Cin", "inner", "x:3 w:3"), ax("Cout", "inner", "w:0 bias:0 resid:3"), ax("kh", "inner", "w:1"), ax("kw", "inner", "w:2")],
    "resnet_stem": [ax("N", "count", "imgs:0", res=((0, 3, 4, 64),)), ax("channels", "inner", "imgs:1"), ax("H", "sample", "imgs:2"),
                    ax("W", "sample", "imgs:3"), ax("K", "inner", "wt:0"), ax("d", "inner", "wt:1 shift:0")],
    "attention_hd32": [ax("B", "count", "q:0 k:0 v:0", res=((0, 3, 96),)), ax("Lq", "count", "q:1", res=((2, 0, 96),)), ax("Lk", "inner", "k:1 v:1"),
                       ax("D", "inner", "q:2 k:2 v:2")],
    "mixer_token_mix": [ax("N", "count", "x:0 stats:0 out:0", res=((0, 12, 64), (0, 1, 2))), ax("T", "sample", "x:1 stats:0 b2:0 out:1 w1f:1 w2f:0"),
                        ax("C", "inner", "x:2 gamma:0 beta:0 out:2"), ax("Dt", "inner", "b1:0 w1f:0 w2f:1"), ax("pair", "inner", "stats:1"),
                        ax("fragment lanes", "inner", "w1f:2 w2f:2"), ax("fragment values", "inner", "w1f:3 w2f:3")],
    "row_stats": [ax("M", "count", "x:0", res=((0, 2),)), ax("C", "inner", "x:1")],
    "ln_mean": [ax("N", "count", "x:0 stats:0", res=((0, 8),)), ax("T", "inner", "x:1 stats:0"), ax("C", "inner", "x:2 gamma:0 beta:0"),
                ax("pair", "inner", "stats:1")],
    "transpose_add_f32": [ax("N", "count", "x:0 resid:0", res=((0, 5, 3),)), ax("R", "inner", "x:1 resid:2"), ax("Cc", "inner", "x:2 resid:1")],
    "conv1d_f32": [ax("B", "count", "x:0 resid:0", res=((0, 9, 8),)), ax("Tin", "sample", "x:1 resid:1"), ax("Cin", "inner", "x:2 w:1"),
                   ax("Cout", "inner", "w:0 bias:0 resid:2")],
    "lstm_f32": [ax("B", "count", "x:0", res=((0, 3, 64),)), ax("T", "sample", "x:1"),
                 ax("H", "inner", "x:2 w_ih[0]:1 w_ih[1]:1 w_hh[0]:1 w_hh[1]:1"),
                 ax("gates", "inner", "w_ih[0]:0 w_ih[1]:0 w_hh[0]:0 w_hh[1]:0 bias[0]:0 bias[1]:0")],
    "rvq_encode": [ax("M", "count", "z:0", res=((2, 0),)), ax("D", "inner", "z:1 codebooks:2"), ax("entries", "inner", "codebooks:1 norms:1"),
                   ax("n_q", "inner", "codebooks:0 norms:0", {"n_q": 0})],
    "rvq_decode": [ax("B", "count", "codes:0", res=((0, 5, 128),)), ax("n_q", "inner", "codes:1"), ax("T", "sample", "codes:2"),
                   ax("Q", "inner", "codebooks:0"), ax("entries", "inner", "codebooks:1"), ax("D", "inner", "codebooks:2")],
    "groupnorm1_": [ax("B", "count", "x:0 resid:0", res=((0, 5, 8),)), ax("T", "sample", "x:1 resid:1"), ax("C", "inner", "x:2 gamma:0 beta:0 resid:2")],
    "encodec_scale": [ax("B", "count", "x:0", res=((0, 1, 1),)), ax("C", "inner", "x:1"), ax("T", "sample", "x:2")],
    "scale_clips": [ax("B", "count", "x:0 scale:0", res=((0, 3, 7),)), ax("C", "sample", "x:1"), ax("T", "sample", "x:2"),
                    ax("scale 1", "inner", "scale:1"), ax("scale 2", "inner", "scale:2")],
    "cls_head_gemm": [ax("M", "count", "x:0", res=((0, 2, 64),)), ax("G", "inner", "x:1 w:0 bias:0"), ax("K", "inner", "x:2 w:2"),
                      ax("N", "inner", "w:1 bias:0")],
    "cls_attend": [ax("N", "count", "x:0 stats:0 u:0", res=((0, 3, 64),)), ax("L", "inner", "x:1 stats:0"), ax("d", "inner", "x:2 u:2"),
                   ax("H", "inner", "u:1"), ax("pair", "inner", "stats:1")],
    "lm_score": [ax("M", "count", "h:0 targets:0 out:0 lse_out:0 argmax_out:0", ws=lambda ops: ops.lm_score_ws_bytes(0, 11), res=((0,), (0,), (0,))),
                 ax("K", "inner", "h:1 w:1"), ax("V", "inner", "w:0"), ax("workspace", "inner", "ws:0")],
    "align_lse": [ax("B", "count", _ALIGN_B + " out:0", res=((0, 3, 5),)), ax("L", "sample", "q:1 out:2"), ax("S", "inner", "k:1"),
                  ax("width", "inner", "q:2 k:2"), ax("heads", "inner", "heads:0 out:1")],
    "align_matrix": [ax("B", "count", _ALIGN_B + " lse:0 m:0", res=((0, 5, 12),)), ax("L", "inner", "q:1 lse:2 m:1"), ax("S", "inner", "k:1 m:2"),
                     ax("width", "inner", "q:2 k:2"), ax("heads", "inner", "heads:0 lse:1")],
    "align_dtw": [ax("B", "count", "m:0 lengths:0 frames:0 out:0", ws=lambda ops: ops.align_ws_bytes(0, 5, 12), res=((0, 5),)),
                  ax("L", "inner", "m:1 out:1"), ax("S", "inner", "m:2"), ax("workspace", "inner", "ws:0")],
    "attention_varlen": [ax("T_total", "count", "q:0 k:0 v:0 out:0", seq=_Z2, res=((0, 128),)), ax("B", "count", "q:0 k:0 v:0 out:0", seq=_B0, res=((0, 128),)),
                         ax("D", "inner", "q:1 k:1 v:1 out:1"), ax("heads", "inner", "rel_lut:0", {"n_heads": 0}), ax("table", "inner", "rel_lut:1")],
    "attention_varlen:plain": [ax("T_total", "count", "q:0 k:0 v:0 out:0", seq=_Z2, res=((0, 128),)),
                               ax("B", "count", "q:0 k:0 v:0 out:0", seq=_B0, res=((0, 128),)), ax("D", "inner", "q:1 k:1 v:1 out:1")],
    "embed_tokens_varlen": [ax("B", "count", "tokens:0", seq=_B0, res=((0, 32),)), ax("L", "count", "tokens:1", seq=((0, 0), 0), res=((0, 32),)),
                            ax("T_total", "count", "", seq=_Z2, res=((0, 32),)), ax("V", "inner", "emb:0"), ax("d", "inner", "emb:1 pos:1"),
                            ax("positions", "inner", "pos:0")],
    "rows_pack": [ax("B", "count", "x:0", seq=_B0, res=((0, 16),)), ax("L", "count", "x:1", seq=((0, 0), 0), res=((0, 16),)),
                  ax("T_total", "count", "", seq=_Z2, res=((0, 16),)), ax("d", "inner", "x:2")],
    "rows_unpack": [ax("T_total", "count", "x:0", seq=_Z2, res=((2, 6, 16),)), ax("B", "count", "x:0", seq=_B0, res=((0, 6, 16),)), ax("d", "inner", "x:1")],
    "rows_zero_tail": [ax("B", "count", "x:0", seq=_B0, res=((0, 6, 16),)), ax("L", "count", "x:1", seq=((0, 0), 0), res=((2, 0, 16),)), ax("d", "inner", "x:2")],
    "segment_mean": [ax("T_total", "count", "x:0", seq=_Z2, res=((2, 16),)), ax("B", "count", "x:0", seq=_B0, res=((0, 16),)), ax("d", "inner", "x:1")],
    "ctc_head": [ax("M", "count", "h:0 out:0 best_out:0 best_logp_out:0", res=((0, 7), (0,), (0,))), ax("K", "inner", "h:1 w:1"),
                 ax("V", "inner", "w:0 bias:0 out:1")],
    "ctc_greedy": [ax("T_total", "count", "best:0 best_logp:0", seq=_Z2, res=((2, 6), (2,), (2, 6), (2,))),
                   ax("B", "count", "best:0 best_logp:0", seq=_B0, res=((0, 6), (0,), (0, 6), (0,)))],
    "ctc_forward": [ax("B", "count", _CTC_B + " out:0", seq=_B0, res=((0,),)), ax("frames", "sample", "logp:0", seq=_Z2), ax("V", "inner", "logp:1")],
    "ctc_viterbi": [ax("B", "count", _CTC_B, seq=_B0, ws=lambda ops: ops.ctc_ws_bytes(0, 0, 3), res=((0, 3), (0, 3), (0,))),
                    ax("frames", "sample", "logp:0", seq=_Z2), ax("V", "inner", "logp:1"), ax("workspace", "inner", "ws:0")],
}

# Operand dimensions that no axis zeroes, each with its reason.  Never a count.
_UMAX = "Umax = 0 is a served problem, not an empty one: every transcript is empty, the wrapper passes no targets pointer and the C entry "\
        "accepts it (tests/ctc_cases.py has the case)"
EXEMPT_DIMS: dict[tuple, str] = {
    ("ctc_forward", "targets", 1): _UMAX,
    ("ctc_viterbi", "targets", 1): _UMAX,
}


def missing_dims(rid: str, kw: dict) -> list[tuple]:
    """the (operand, dimension) pairs of a row's canonical build that no axis zeroes and EXEMPT_DIMS does not list"""
    covered = {(WC.path_name(p), d) for a in AXES.get(rid, ()) for p, d in a.dims}
    return [(WC.path_name(p), d) for p, t in WC.operands(kw) for d in range(t.dim())
            if (WC.path_name(p), d) not in covered and (rid, WC.path_name(p), d) not in EXEMPT_DIMS]


# ------------------------------------------------------------------------------------------------------------------ driver
def _all_tensors(kw: dict):
    for path, t in WC.operands(kw):
        yield WC.path_name(path), t
    seq = kw.get("seq")
    if seq is not None and hasattr(seq, "cu"):
        yield "seq.cu", seq.cu


def null_positions(canon_launches, launches) -> list[str]:
    """recorded calls that carry a null pointer (None or 0) where the canonical call of the same entry point carried a non-null one"""
    bad = []
    canon = {}
    for name, args in canon_launches:
        canon.setdefault(name, args)
    for name, args in launches:
        ref = canon.get(name)
        for i, a in enumerate(args):
            was = ref[i] if ref is not None and i < len(ref) else None
            if (a is None or a == 0) and isinstance(was, int) and not isinstance(was, bool) and abs(was) >= 2 ** 12:
                bad.append(f"{name} argument {i} is null; the canonical call passed a pointer there")
    return bad


def check_axis(ops, r: WC.Row, a: Axis, dev, canon_res, canon_kw, rec=None, canon_launches=()) -> list[str]:
    """One empty case against the contract: the problems found.  ``canon_res`` / ``canon_kw``: the canonical call's result and
    operands (for dtypes, devices and which operand is returned); ``rec``: the CPU stage's recorder."""
    where = f"{r.id} {a.name}"
    kw = a.shrink(r.build(dev))
    before = [(n, t, t.clone()) for n, t in _all_tensors(kw)]
    if rec is not None:
        rec.begin()
    try:
        res, exc = WC.call(ops, r, kw), None
        if dev.type == "cuda":
            torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001 - classified below
        if WC.is_fault(e):
            raise WC.GpuFault(f"{where}: {e}") from e
        res, exc = None, e
    problems = []
    launches = list(rec.launches) if rec is not None else []
    if launches:
        problems.append(f"{where}: the library was called ({[n for n, _ in launches]})" + (" before the refusal" if exc is not None else ""))
        problems += [f"{where}: {p}" for p in null_positions(canon_launches, launches)]
    changed = [n for n, t, was in before if not WC.same_bits(t, was)]
    if changed:
        problems.append(f"{where}: operands {changed} were modified")
    if a.outcome == "refuse":
        if exc is None:
            problems.append(f"{where}: accepted; the table says refuse")
        elif type(exc) is not ValueError:
            problems.append(f"{where}: refused with {type(exc).__name__} ({exc}), not ValueError")
        elif r.fn.rstrip("_") not in str(exc):
            problems.append(f"{where}: the refusal does not name the wrapper: {exc}")
        return problems
    if exc is not None:
        return problems + [f"{where}: raised {type(exc).__name__}: {exc}; the table says empty"]
    got, want = WC.flat_outputs(res), WC.flat_outputs(canon_res)
    if [tuple(t.shape) for t in got] != [tuple(s) for s in a.res]:
        problems.append(f"{where}: result shapes {[tuple(t.shape) for t in got]}, the table says {list(a.res)}")
    if [(t.dtype, t.device) for t in got] != [(t.dtype, t.device) for t in want]:
        problems.append(f"{where}: result dtypes / devices {[(t.dtype, t.device) for t in got]} vs the canonical call's {[(t.dtype, t.device) for t in want]}")
    for name in r.inplace:  # an operand the canonical call returns is returned by the empty call too, at the same place
        v = canon_kw.get(name)
        if isinstance(v, Tensor):
            for i, t in enumerate(want):
                if t is v and (i >= len(got) or got[i] is not kw[name]):
                    problems.append(f"{where}: result {i} is not the caller's {name}= itself")
    return problems


def check_row(ops, r: WC.Row, dev, rec=None, canon_ops=None) -> tuple[list[str], list[tuple[str, str, str]]]:
    """every axis of one row: (problems, (row, axis, outcome) of every case run).  ``canon_ops``: the module that makes the
    canonical call (the mutant test: the sound one, so that a mutant is not its own reference)"""
    kw0 = r.build(dev)
    if rec is not None:
        rec.begin()
    res0 = WC.call(canon_ops or ops, r, kw0)
    canon_launches = list(rec.launches) if rec is not None else ()
    problems, cases = [], []
    for a in AXES[r.id]:
        problems += check_axis(ops, r, a, dev, res0, kw0, rec, canon_launches)
        cases.append((r.id, a.name, a.outcome))
    return problems, cases


# ----------------------------------------------------------------------------------------------------------------- mutants
class _Patched:
    """ops with one wrapper replaced"""

    def __init__(self, ops, name, fn) -> None:
        self._ops, self._name, self._fn = ops, name, fn

    def __getattr__(self, name):
        return self._fn if name == self._name else getattr(self._ops, name)


def _m_null(ops):
    def layernorm(x, gamma, beta, eps, out_dtype=None, act="none", resid=None, out=None):
        out = out if out is not None else torch.empty_like(x)
        rc = ops.lib().pm_layernorm(x.data_ptr() or None, x.stride(0), 0, gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr() or None,
                                    out.stride(0), 0, x.shape[0], x.shape[1], 0)
        ops.check(rc, "pm_layernorm")
        return out
    return layernorm


def _m_canon_shape(ops):
    def rmsnorm(x, gamma, eps, out_dtype=None):
        ops.rmsnorm(x, gamma, eps, out_dtype)
        return torch.empty((6, 64), dtype=x.dtype, device=x.device)
    return rmsnorm


def _m_fresh_out(ops):
    def layernorm(x, gamma, beta, eps, out_dtype=None, act="none", resid=None, out=None):
        return ops.layernorm(x, gamma, beta, eps, out_dtype, act, resid, None)
    return layernorm


def _m_writes(ops):
    def linear(x, w, bias=None, **kw):
        if kw.get("out") is not None and kw["out"].numel():
            kw["out"].fill_(1.0)
        return ops.linear(x, w, bias, **kw)
    return linear


def _m_runtime(ops):
    def geglu(h):
        try:
            return ops.geglu(h)
        except ValueError as e:
            raise RuntimeError(str(e)) from e
    return geglu


def _m_late(ops):
    def mean_rows(x):
        if x.shape[1] == 0 or x.shape[2] == 0:
            ops.lib().pm_mean_rows_bf16(x.data_ptr() or None, None, *x.shape, 0)
        return ops.mean_rows(x)
    return mean_rows


# name -> (row id, wrapper name, ops -> broken wrapper, the words its report must contain)
MUTANTS = {
    "forwards the empty operand's null pointer to the library": ("layernorm:plain", "layernorm", _m_null, "is null"),
    "returns the canonical non-empty shape": ("rmsnorm", "rmsnorm", _m_canon_shape, "result shapes"),
    "returns a fresh tensor where out= was given": ("layernorm", "layernorm", _m_fresh_out, "is not the caller's out= itself"),
    "writes an in-place operand before returning": ("linear", "linear", _m_writes, "were modified"),
    "refuses with RuntimeError": ("geglu", "geglu", _m_runtime, "not ValueError"),
    "refuses after a library call": ("mean_rows", "mean_rows", _m_late, "before the refusal"),
}


def mutant_ops(ops, name: str):
    rid, fn, make, _ = MUTANTS[name]
    return rid, _Patched(ops, fn, make(ops))


# ------------------------------------------------------------------------------------------------------------------ models
@dataclass
class ModelEmpty:
    """One empty call of a model entry point.  ``model``: the key of graph_cases.MODELS that builds the module and its canonical
    inputs; ``call(module, inputs) -> result`` makes the empty call from the canonical inputs (the same builders at batch 0);
    ``outcome``: "empty" | "refuse" | None = the fp32 CPU module decides (a MODELS forward whose class has a CPU form); ``why``:
    the reason of a stated outcome."""
    model: str
    call: Callable
    outcome: str | None = None
    why: str = ""


def batch0(inputs):
    return tuple(t[:0] for t in inputs)


def _fwd(method=None):
    return (lambda m, i: m(*batch0(i))) if method is None else (lambda m, i: getattr(m, method)(*batch0(i)))


def _with_lengths(kind):
    """forward(..., lengths) with every length 0 ("0s": the canonical batch, nothing valid) or without any sequence ("[]")"""
    def run(m, i):
        if kind == "0s":
            return m(*i, torch.zeros(i[0].shape[0], dtype=torch.int64))
        return m(*batch0(i), torch.zeros(0, dtype=torch.int64))
    return run


NO_CPU_FORM = "the class has no CPU form to ask; the HIP path honours the batch as every wrapper under it does"
DECODING = "decoding allocates its caches and its launch plan per batch (the decode-step family): refused at the entry"
ZERO_LENGTH = "a sequence without a token (or a clip shorter than the receptive field) is refused by seq_lens' lower bound, as before"
ALIGNING = "the DTW needs at least one clip, one token and 4 frames: refused at the entry"
_STATED = {k: ("empty", NO_CPU_FORM) for k in ("MobileViT", "Wav2Vec2", "Wav2Vec2:hubert", "Data2VecAudio", "SEW", "BERT", "GPT", "GPT2",
                                               "T5Encoder", "T5Decoder", "T5Model")}
MODEL_EMPTY: dict[str, ModelEmpty] = {k: ModelEmpty(k, _fwd(m.method), *_STATED.get(k, (None, ""))) for k, m in GC.MODELS.items()}
MODEL_EMPTY.update({
    # the lengths= forwards of graph_cases.NOT_GRAPHED
    **{f"{k}.forward(lengths=[])": ModelEmpty(k, _with_lengths("[]"), "empty") for k, m in GC.MODELS.items() if m.lengths is not None},
    "Wav2Vec2CTC.forward(lengths=[])": ModelEmpty("Wav2Vec2CTC", _with_lengths("[]"), "refuse", "as its forward without lengths, which the CPU form decides"),
    **{f"{k}.forward(lengths=0s)": ModelEmpty(k, _with_lengths("0s"), "refuse", ZERO_LENGTH) for k, m in GC.MODELS.items() if m.lengths is not None},
    # generate / score / align / encode / embed
    "GPT2.generate": ModelEmpty("GPT2", lambda m, i: m.generate(i[0][:0], 4), "refuse", DECODING),
    "WhisperDecoder.generate": ModelEmpty("WhisperDecoder", lambda m, i: m.generate(i[1][:0], i[0][:0, :2], 4), "refuse", DECODING),
    "Whisper.generate": ModelEmpty("Whisper", lambda m, i: m.generate(i[0][:0], i[1][:0, :2], 4), "refuse", DECODING),
    "T5Model.generate": ModelEmpty("T5Model", lambda m, i: m.generate(i[0][:0], max_new_tokens=4), "refuse", DECODING),
    "GPT.score": ModelEmpty("GPT", lambda m, i: m.score(i[0][:0]), "empty"),
    "GPT2.score": ModelEmpty("GPT2", lambda m, i: m.score(i[0][:0]), "empty"),
    "GPT2.score(lengths=[])": ModelEmpty("GPT2", lambda m, i: m.score(i[0][:0], []), "empty"),
    "WhisperDecoder.score": ModelEmpty("WhisperDecoder", lambda m, i: m.score(i[0][:0], i[1][:0]), "empty"),
    "Whisper.score": ModelEmpty("Whisper", lambda m, i: m.score(i[0][:0], i[1][:0]), "empty"),
    "T5Model.score": ModelEmpty("T5Model", lambda m, i: m.score(i[0][:0], i[1][:0]), "empty"),
    "WhisperDecoder.align": ModelEmpty("WhisperDecoder", lambda m, i: m.align(i[0][:0], i[1][:0]), "refuse", ALIGNING),
    "Whisper.align": ModelEmpty("Whisper", lambda m, i: m.align(i[0][:0], i[1][:0]), "refuse", ALIGNING),
    "T5Model.encode": ModelEmpty("T5Model", lambda m, i: m.encode(i[0][:0]), "empty"),
    "T5Model.encode(lengths=[])": ModelEmpty("T5Model", lambda m, i: m.encode(i[0][:0], []), "empty"),
    "T5Model.encode(lengths=0s)": ModelEmpty("T5Model", lambda m, i: m.encode(i[0], [0] * i[0].shape[0]), "empty",
                                             "no valid row: the padded memory, all zero (the short-circuit of T5Model._encode_packed)"),
    "BERT.embed": ModelEmpty("BERT", lambda m, i: m.embed(i[0][:0]), "empty"),
    "BERT.embed(lengths=[])": ModelEmpty("BERT", lambda m, i: m.embed(i[0][:0], []), "empty"),
    "BERT.embed(lengths=0s)": ModelEmpty("BERT", lambda m, i: m.embed(i[0], [0] * i[0].shape[0]), "refuse", ZERO_LENGTH),
})

# MODELS forwards that the fp32 CPU module honours and the HIP module refuses (at most 4), each with its reason (also in DESIGN.md)
_ENCODEC = "the HIP entry points of EnCodec refuse an input without a clip or without a frame in one ValueError at the entry (encodec._gate, "\
           "decode_checkpoints): the reflect padding and the per-clip scale have nothing to work on when T = 0, and B = 0 shares the check"
MODEL_REFUSALS: dict[str, str] = {"EnCodecEncoder": _ENCODEC, "EnCodecDecoder": _ENCODEC, "EnCodec.encode": _ENCODEC, "EnCodec.decode": _ENCODEC}


def cpu_outcome(key: str):
    """What the fp32 CPU module of a MODELS entry does with its empty input: ("empty", [(shape, dtype) ...]), ("refuse", the exception),
    or ("none", the exception) where the class has no CPU form at all - its canonical input raises too."""
    m = GC.MODELS[key]
    mod = m.make(0).eval()
    call = (lambda *a: getattr(mod, m.method)(*a)) if m.method else mod
    with torch.no_grad():
        try:
            call(*m.inputs(0, 0))
        except Exception as e:  # noqa: BLE001 - no CPU form
            return "none", e
        try:
            res = MODEL_EMPTY[key].call(mod, m.inputs(0, 0))
        except Exception as e:  # noqa: BLE001 - whatever the reference module does with it
            return "refuse", e
    return "empty", [(tuple(t.shape), t.dtype) for _, t in GC.flat(res)]


def expected_model_outcome(key: str):
    """(outcome, result shapes or None) the HIP module must show: the table's statement, or the CPU module's verdict"""
    e = MODEL_EMPTY[key]
    if key in MODEL_REFUSALS:
        return "refuse", None
    if e.outcome is not None:
        return e.outcome, None
    kind, what = cpu_outcome(key)
    assert kind != "none", f"{key}: no CPU form: the table must state the outcome"
    return kind, (what if kind == "empty" else None)


def hip_module(key: str, dtype: str):
    """the filled HIP module of a MODELS entry and its canonical device inputs, as tests/test_hip_graph_models.py builds them"""
    import coherence_cases as CC

    case = GC.MODELS[key]
    m = CC.filled(case.make(0), 311)
    m = (m.to(torch.bfloat16) if dtype == "bf16" else m).cuda()
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype]
    return m, tuple((x.to(dt) if i in case.cast else x).cuda() for i, x in enumerate(case.inputs(0, 311)))
