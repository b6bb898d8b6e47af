"""Wrapper operand contract: the table of every tensor-taking wrapper of pytorch_models/_hip/ops.py and
the generated layout / dtype / rank variants of each of its operands.

ops.py turns a Tensor into a raw pointer plus a few integers, so it decides what memory a kernel believes it was given.  A
forgotten check is silent: the kernel reads numel elements from data_ptr() as if they were packed and of the assumed type.
The tests built on this table call every wrapper with every variant of every operand and accept two outcomes only: the call
raises before the first launch, or its results are bit-identical to the same call on a fresh contiguous tensor holding the
variant's values.  tests/test_wrapper_cases_cpu.py (no GPU: a recording stub for the library, which also audits that whatever
is accepted reaches the C call as a stride, a dtype code or a copy) and tests/test_hip_wrappers.py (the kernels).

One row per wrapper (ROWS): ``build(dev)`` returns the canonical keyword arguments at the smallest shape the kernel serves -
pairwise different dimensions wherever the kernel allows it, at least two rows and two batch entries - freshly on every call
(in-place operands are consumed).  ``inplace`` names the operands the call writes.  ``only`` restricts the operands that are
varied (a second row of a wrapper that exists for one more code path).  EXEMPT lists the public functions without a row.

Every variant is IN BOUNDS BY CONSTRUCTION: a view into a parent buffer at least as large as what a kernel would read if it
took data_ptr() for the start of a packed tensor of the widest dtype (8 bytes) and the canonical numel, and as large as any mix
of the view's and the packed strides can reach.  The parent's unused elements are NaN (floats) or SENTINEL (integers), so a
layout that is silently ignored poisons the result instead of leaving it nearly right."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import torch
from torch import Tensor

BF, F16, F32, F64, I32, I64, U8 = (torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int32, torch.int64,
                                   torch.uint8)
FLOATS, INTS = (BF, F16, F32, F64), (I32, I64)
WIDEST = 8            # bytes of the widest dtype of the variant lists
SENTINEL = 2 ** 30 + 12345  # no id, position or length of any row comes near it
SEED = 2611
REFUSALS = (ValueError, TypeError, IndexError, RuntimeError)
FAULT_WORDS = ("hip error", "hiperror", "cuda error", "illegal memory", "device-side assert", "unspecified launch failure")


class GpuFault(Exception):
    """a device error surfaced inside a call: never a refusal; the GPU test stops the whole run on it"""


def is_fault(e: BaseException) -> bool:
    return any(w in str(e).lower() for w in FAULT_WORDS)


# ---------------------------------------------------------------------------------------------------------------- variants
def _packed(shape) -> list[int]:
    st, n = [], 1
    for s in reversed(shape):
        st.append(n)
        n *= max(int(s), 1)
    return st[::-1]


@dataclass
class Variant:
    tag: str
    tensor: Tensor          # the view handed to the wrapper
    parent: Tensor          # the flat buffer it lives in
    offset: int             # storage offset of the view in the parent, elements
    canon_numel: int
    reshaped: bool = False  # the shape differs from the canonical one
    must_raise: bool = False

    def check_bounds(self) -> None:
        """the in-bounds rule of the module docstring, recomputed from the tensors themselves"""
        v, p = self.tensor, self.parent
        item = v.element_size()
        assert v.untyped_storage().data_ptr() == p.untyped_storage().data_ptr() and v.storage_offset() == self.offset, self.tag
        room = (p.numel() - self.offset) * item
        assert room >= self.canon_numel * WIDEST, (self.tag, room, self.canon_numel)
        mixed = 1 + sum((n - 1) * max(a, b) for n, a, b in zip(v.shape, v.stride(), _packed(v.shape)) if n > 0)
        assert v.numel() == 0 or self.offset + mixed <= p.numel(), (self.tag, mixed, p.numel())

    def outside_untouched(self, before: Tensor) -> bool:
        """the parent's elements outside the view still hold what ``before`` (a clone taken in front of the call) holds"""
        now = self.parent.clone()
        if 0 in self.tensor.stride() and self.tensor.numel() > 1:
            return True  # a broadcast view has no inside of its own
        now.as_strided(self.tensor.shape, self.tensor.stride(), self.offset).copy_(
            before.as_strided(self.tensor.shape, self.tensor.stride(), self.offset))
        return same_bits(now, before)


def _poison(n: int, dtype, device) -> Tensor:
    if dtype.is_floating_point:
        return torch.full((n,), float("nan"), dtype=dtype, device=device)
    return torch.full((n,), SENTINEL if dtype in INTS else 0x7F, dtype=dtype, device=device)


def _place(tag: str, values: Tensor, strides, offset: int, canon_numel: int, **kw) -> Variant:
    """``values`` (any layout) laid out with ``strides`` at ``offset`` of a fresh poisoned parent"""
    shape, item = tuple(values.shape), values.element_size()
    mixed = 1 + sum((n - 1) * max(a, b) for n, a, b in zip(shape, strides, _packed(shape)))
    need = max(mixed, -(-canon_numel * WIDEST // item)) + 8
    parent = _poison(offset + need, values.dtype, values.device)
    view = parent.as_strided(shape, tuple(strides), offset)
    view.copy_(values)
    return Variant(tag, view, parent, offset, canon_numel, **kw)


def variants(t: Tensor) -> list[Variant]:
    """Every variant of the contract's table that applies to the canonical operand ``t`` (a fresh contiguous tensor); the
    ``device`` variant is a property of the CPU stage (check_devices sees the operand), not a tensor."""
    assert t.is_contiguous(), "canonical operands are contiguous"
    out: list[Variant] = []
    shape, n, pk = tuple(t.shape), t.numel(), _packed(t.shape)
    if n == 0 or t.dim() == 0:
        return out
    if shape[-1] > 1:  # last dimension with stride 2: parent[..., ::2]
        out.append(_place("strided", t, _packed(shape[:-1] + (2 * shape[-1],))[:-1] + [2], 0, n))
    if t.dim() >= 2 and n > shape[-1]:  # leading-dimension padding: parent[..., :K] of a (..., K + 8) parent
        out.append(_place("rowpad", t, _packed(shape[:-1] + (shape[-1] + 8,)), 0, n))
    if t.dim() >= 3 and shape[0] > 1:  # the first dimension alone
        out.append(_place("rowpad0", t, [pk[0] + 8] + pk[1:], 0, n))
    if t.dim() >= 2:
        same = [(i, j) for i in range(t.dim()) for j in range(i + 1, t.dim()) if shape[i] == shape[j] and shape[i] > 1]
        if same:  # same shape, permuted strides
            i, j = same[-1]
            st = list(pk)
            st[i], st[j] = st[j], st[i]
            out.append(_place("transposed", t, st, 0, n))
        elif shape[-1] > 1 and shape[-2] > 1:  # the permuted shape: must raise
            tt = t.transpose(-1, -2)
            out.append(_place("transposed", tt, tt.stride(), 0, n, reshaped=True, must_raise=True))
    if shape[0] > 1:  # stride-0 broadcast of the first element or row; the parent holds the distinct canonical values
        parent = torch.cat([t.reshape(-1), _poison(-(-n * WIDEST // t.element_size()) + 8, t.dtype, t.device)])
        out.append(Variant("expanded", parent.as_strided(shape, [0] + pk[1:], 0), parent, 0, n))
    out.append(_place("offset", t, pk, 1, n))  # a storage offset of one element: an unaligned pointer
    family = FLOATS if t.dtype in FLOATS else INTS if t.dtype in INTS else ()
    for dt in family:
        if dt != t.dtype:
            out.append(_place("dtype:" + str(dt).replace("torch.", ""), t.to(dt), pk, 0, n))
    if t.dim() == 1:  # same numel, one dimension more
        out.append(_place("rank:col", t.reshape(n, 1), [1, 1], 0, n, reshaped=True))
        out.append(_place("rank:row", t.reshape(1, n), [n, 1], 0, n, reshaped=True))
    else:  # one more, one fewer
        out.append(_place("rank:up", t.reshape((1,) + shape), [n] + pk, 0, n, reshaped=True))
        out.append(_place("rank:down", t.reshape((shape[0] * shape[1],) + shape[2:]), pk[1:], 0, n, reshaped=True))
    return out


def applicable_tags(t: Tensor) -> set[str]:
    """the tags ``variants`` must produce for ``t``, derived from the contract's table alone (the completeness test)"""
    if t.numel() == 0 or t.dim() == 0:
        return set()
    s, tags = tuple(t.shape), {"offset"}
    if s[-1] > 1:
        tags.add("strided")
    if t.dim() >= 2 and t.numel() > s[-1]:
        tags.add("rowpad")
    if t.dim() >= 3 and s[0] > 1:
        tags.add("rowpad0")
    if t.dim() >= 2 and (len({d for d in s if d > 1}) < len([d for d in s if d > 1]) or (s[-1] > 1 and s[-2] > 1)):
        tags.add("transposed")
    if s[0] > 1:
        tags.add("expanded")
    fam = FLOATS if t.dtype in FLOATS else INTS if t.dtype in INTS else ()
    tags |= {"dtype:" + str(d).replace("torch.", "") for d in fam if d != t.dtype}
    tags |= {"rank:col", "rank:row"} if t.dim() == 1 else {"rank:up", "rank:down"}
    return tags


def same_bits(a: Tensor, b: Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.numel() == 0:
        return True
    as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.view(as_int), b.view(as_int)))


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(kw: dict):
    """(path, tensor) of every tensor operand of a call: direct, or inside a list or tuple"""
    for name, v in kw.items():
        if isinstance(v, Tensor):
            yield (name,), v
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                if isinstance(e, Tensor):
                    yield (name, i), e


def get(kw: dict, path) -> Tensor:
    return kw[path[0]] if len(path) == 1 else kw[path[0]][path[1]]


def replaced(kw: dict, path, t: Tensor) -> dict:
    kw = dict(kw)
    if len(path) == 1:
        kw[path[0]] = t
    else:
        seq = list(kw[path[0]])
        seq[path[1]] = t
        kw[path[0]] = type(kw[path[0]])(seq) if isinstance(kw[path[0]], tuple) else seq
    return kw


def path_name(path) -> str:
    return path[0] if len(path) == 1 else f"{path[0]}[{path[1]}]"


def flat_outputs(res) -> list[Tensor]:
    if res is None:
        return []
    if isinstance(res, Tensor):
        return [res]
    return [r for r in res if isinstance(r, Tensor)]


# -------------------------------------------------------------------------------------------------------------------- rows
class Gen:
    """deterministic values, drawn on the CPU and moved: every build of a row holds the same numbers"""

    def __init__(self, dev, seed: int) -> None:
        self.dev, self.g = dev, torch.Generator().manual_seed(seed)

    def f(self, *shape, scale: float = 1.0) -> Tensor:
        return (torch.randn(shape, generator=self.g) * scale).to(self.dev)

    def b(self, *shape, scale: float = 1.0) -> Tensor:
        return (torch.randn(shape, generator=self.g) * scale).to(BF).to(self.dev)

    def i(self, hi: int, *shape, dtype=I64, lo: int = 0) -> Tensor:
        return torch.randint(lo, hi, shape, generator=self.g).to(dtype).to(self.dev)

    def t(self, vals, dtype) -> Tensor:
        return torch.tensor(vals, dtype=dtype).to(self.dev)

    def z(self, *shape, dtype=F32) -> Tensor:
        return torch.zeros(shape, dtype=dtype).to(self.dev)

    def stats(self, m: int) -> Tensor:
        """(m, 2) [mean, rstd] with a positive second column"""
        s = torch.randn((m, 2), generator=self.g) * 0.25
        s[:, 1] = s[:, 1].abs() + 0.5
        return s.to(self.dev)


@dataclass
class Row:
    id: str
    fn: str
    build: Callable
    inplace: tuple = ()
    only: tuple | None = None
    host_ok: tuple = ()  # operands the wrapper documents as "host ints or a device tensor": a CPU tensor is uploaded, not refused
    free_shape: tuple = ()  # operands documented with free leading dimensions "(..., T)": another shape is another problem, not an error


ROWS: dict[str, Row] = {}


def row(fn: str, *, id: str | None = None, inplace=(), only=None, host_ok=(), free_shape=()):
    def deco(build):
        rid = id or fn
        assert rid not in ROWS, rid
        # ``seed``: an offset for a second operand set of the same shapes (tests/graph_cases.py); 0 is the canonical one
        ROWS[rid] = Row(rid, fn, lambda dev, seed=0, _b=build, _s=len(ROWS): _b(Gen(dev, SEED + _s + seed)), tuple(inplace), only,
                        tuple(host_ok), tuple(free_shape))
        return build
    return deco


def _ops():
    from pytorch_models._hip import ops
    return ops


EPS = 1e-5


@row("ln_stats_finalize")
def _(g):
    return dict(partials=g.f(3, 2, 2).abs() + 1.0, N=128, eps=EPS)


@row("linear", inplace=("out",))
def _(g):
    return dict(x=g.b(16, 128), w=g.b(64, 128, scale=0.1), bias=g.f(64), act="gelu", resid=g.b(16, 64), out=g.z(16, 64, dtype=BF))


@row("linear", id="linear:ln_fold", only=("ln_stats", "ln_s"))
def _(g):  # the LayerNorm fold is served from 4096 rows on
    return dict(x=g.b(4104, 128), w=g.b(64, 128, scale=0.1), bias=g.f(64), ln_stats=g.stats(4104), ln_s=g.f(64))


@row("linear_f32", inplace=("out",))
def _(g):
    return dict(x=g.f(6, 32), w=g.f(12, 32, scale=0.2), bias=g.f(12), act="relu", resid=g.f(6, 12), out=g.z(6, 12))


@row("attention_f32")
def _(g):
    return dict(q=g.f(2, 3, 32), k=g.f(2, 5, 32), v=g.f(2, 5, 32), n_heads=4, bias=g.f(2, 4, 3, 5))


@row("layernorm", inplace=("out",))
def _(g):
    return dict(x=g.b(6, 64), gamma=g.f(64), beta=g.f(64), eps=EPS, act="gelu", resid=g.b(6, 64), out=g.z(6, 64, dtype=BF))


@row("layernorm", id="layernorm:plain", only=("gamma", "beta"))
def _(g):  # pm_layernorm: no activation, no residual
    return dict(x=g.b(6, 64), gamma=g.f(64), beta=g.f(64), eps=EPS)


@row("rmsnorm")
def _(g):
    return dict(x=g.b(6, 64), gamma=g.f(64), eps=EPS)


@row("geglu")
def _(g):
    return dict(h=g.b(6, 32))


@row("attention", inplace=("out",))
def _(g):
    return dict(q=g.b(2, 5, 192), k=g.b(2, 7, 192), v=g.b(2, 7, 192), n_heads=3, bias=g.f(2, 3, 5, 7), out=g.z(2, 5, 192, dtype=BF))


@row("conv2d_nhwc")
def _(g):
    return dict(x=g.b(2, 5, 6, 8), w=g.b(12, 3, 3, 4, scale=0.2), bias=g.f(12), stride=1, pad=1, groups=2, act="silu",
                resid=g.b(2, 5, 6, 12))


@row("mean_rows")
def _(g):
    return dict(x=g.b(2, 5, 8))


@row("vit_tokens")
def _(g):
    return dict(imgs=g.f(2, 3, 32, 48), w2d=g.b(192, 768, scale=0.05), bias=g.f(192), pe=g.f(6, 192), cls=g.f(192), patch=16)


@row("linear_strided", inplace=("out",))
def _(g):
    return dict(x=g.b(2, 10, 64), M=8, K=128, row_stride=128, rows_per_batch=4, batch_stride=640, w=g.b(32, 128, scale=0.1),
                bias=g.f(32), act="gelu", resid=g.b(8, 32), out=g.z(8, 32, dtype=BF))


@row("w2v_stem0")
def _(g):
    return dict(x=g.f(2, 90), w=g.f(16, 10), bias=g.f(16), norm="layer", gamma=g.f(16), beta=g.f(16), eps=EPS, stride=5)


@row("group_windows")
def _(g):
    return dict(x=g.b(2, 6, 16), groups=4, cgp=8, pad_left=2, pad_right=1)


@row("grouped_conv")
def _(g):
    w = g.b(3, 4, 64, scale=0.2)
    w[:, :, 24:] = 0  # K = 3 taps x 8 channels, zero-padded to 64
    return dict(xg=g.b(2, 3, 9, 8), w=w, bias=g.f(12), k=3, stride=1, cg=4, act="gelu", resid=g.b(14, 12))


@row("avgpool_time2")
def _(g):
    return dict(x=g.b(2, 6, 8))


@row("stft_mel", free_shape=("x",))
def _(g):
    ops = _ops()
    filt = torch.rand((6, 33), generator=g.g)
    filt = (filt * (filt > 0.6)).to(g.dev)
    return dict(x=g.f(2, 400, scale=0.1), tables=ops.stft_tables(torch.hann_window(64).to(g.dev), 64), n_fft=64, hop=16, n_frames=24,
                mode=2, csr=ops.mel_csr(filt), n_mels=6)


@row("whisper_stem1")
def _(g):
    return dict(x=g.f(2, 5, 12), w1=g.b(32, 192, scale=0.1), b1=g.f(32))


@row("embed_tokens", inplace=("out",))
def _(g):
    return dict(tokens=g.i(11, 2, 5), emb=g.b(11, 32), pos=g.f(9, 32), pos0=1, out=g.z(2, 5, 32, dtype=BF))


@row("embed_tokens", id="embed_tokens:f32_table", only=("emb", "pos"))
def _(g):
    return dict(tokens=g.i(11, 2, 5), emb=g.f(11, 32), pos=g.f(9, 32), pos0=1)


@row("dec_linear")
def _(g):
    return dict(x=g.f(3, 64), w=g.b(48, 64, scale=0.1), bias=g.f(48), ln=(g.f(64), g.f(64), EPS), act="gelu", resid=g.f(3, 48))


@row("dec_linear_ksplit")
def _(g):
    return dict(x=g.f(3, 128), w=g.b(48, 128, scale=0.1), bias=g.f(48), k_split=2, act="gelu", resid=g.f(3, 48))


@row("dec_argmax")
def _(g):
    return dict(x=g.f(3, 64), w=g.b(200, 64, scale=0.1), ln=(g.f(64), g.f(64), EPS))


def _caches(g, B=2, H=3, T=12):
    return g.b(B, H, T, 64), g.b(B, H, T, 64)


@row("dec_attention")
def _(g):
    k, v = _caches(g)
    return dict(q=g.f(2, 192), k=k, v=v, lk=7)


@row("prefill_attention", inplace=("kc", "vc", "out"))
def _(g):
    kc, vc = _caches(g)
    return dict(qkv=g.b(8, 576), kc=kc, vc=vc, n_heads=3, p0=3, out=g.z(8, 192, dtype=BF))


@row("dec_attention_ragged")
def _(g):
    k, v = _caches(g)
    return dict(q=g.f(2, 192), k=k, v=v, lk=7, key_start=g.t([1, 3], I32))


@row("prefill_attention_ragged", inplace=("kc", "vc", "out"))
def _(g):
    kc, vc = _caches(g)
    return dict(qkv=g.b(8, 576), kc=kc, vc=vc, n_heads=3, p0=3, key_start=g.t([0, 2], I32), out=g.z(8, 192, dtype=BF))


@row("embed_tokens_ragged", inplace=("out",))
def _(g):
    return dict(tokens=g.i(11, 2, 5), emb=g.b(11, 32), pos=g.f(9, 32), key_start=g.t([0, 2], I32), pos0=1, out=g.z(2, 5, 32, dtype=BF))


@row("dec_embed_ragged")
def _(g):
    return dict(tok_cur=g.i(11, 2), emb=g.b(11, 32), pos_tab=g.f(9, 32), pos=g.t([4], I32), key_start=g.t([0, 2], I32))


def _tail(g, B=2):
    return dict(pos=g.t([3], I32), prompt=g.i(11, B, 2), tok_cur=g.i(11, B), tokens=g.i(11, B, 8), emb=g.b(11, 32), pos_tab=g.f(9, 32),
                ticket=g.t([0], I32))


@row("dec_next_token", inplace=("pos", "tok_cur", "tokens", "ticket", "margins"))
def _(g):
    return dict(ws_val=g.f(2, 3), ws_idx=g.i(11, 2, 3, dtype=I32), **_tail(g), margins=g.z(2, 8), key_start=g.t([0, 1], I32))


@row("dec_next_token", id="dec_next_token:plain", inplace=("pos", "tok_cur", "tokens", "ticket", "margins"))
def _(g):
    return dict(ws_val=g.f(2, 3), ws_idx=g.i(11, 2, 3, dtype=I32), **_tail(g), margins=g.z(2, 8))


@row("dec_sample_topk", inplace=("pos", "tok_cur", "tokens", "ticket"))
def _(g):
    return dict(logits=g.f(2, 11), k=3, seed=5, **_tail(g), key_start=g.t([0, 1], I32))


@row("dec_sample_topk", id="dec_sample_topk:plain", inplace=("pos", "tok_cur", "tokens", "ticket"))
def _(g):
    return dict(logits=g.f(2, 11), k=3, seed=5, **_tail(g))


@row("dec_whisper_rules", inplace=("logits",))
def _(g):
    return dict(logits=g.f(2, 20), tokens=g.i(20, 2, 8), pos=g.t([3], I32), P=2, eot=10, timestamp_begin=12, suppress=(1, 2), blank=(3,))


@row("dec_beam_topw")
def _(g):
    return dict(logits=g.f(6, 11), scores=g.f(2, 3), finished=g.t([[0, 1, 0], [0, 0, 0]], I32), pos=g.t([3], I32), P=2, eos=4)


@row("dec_beam_select", inplace=("scores", "finished", "parents", "tokens", "pos", "tok_cur", "x", "ticket"))
def _(g):
    t = _tail(g, 6)
    return dict(cand_score=g.f(6, 3), cand_tok=g.i(11, 6, 3, dtype=I32), scores=g.f(2, 3), finished=g.t([[0, 1, 0], [0, 0, 0]], I32),
                parents=g.z(2, 3, dtype=I32), tokens=t["tokens"], pos=t["pos"], prompt=t["prompt"], tok_cur=t["tok_cur"], emb=t["emb"],
                pos_tab=t["pos_tab"], x=g.z(6, 32), ticket=t["ticket"], eos=4)


@row("dec_beam_reorder", inplace=("caches",))
def _(g):
    return dict(caches=[g.b(6, 2, 5, 64), g.b(6, 2, 5, 64)], parents=g.t([[1, 0, 2], [2, 2, 0]], I32), pos=g.t([4], I32))


@row("dwconv7_ln")
def _(g):
    return dict(x=g.b(2, 5, 6, 8), w=g.f(7, 7, 8, scale=0.2), bias=g.f(8), gamma=g.f(8), beta=g.f(8), eps=EPS, out_dtype=BF)


@row("ln_space_to_depth")
def _(g):
    return dict(x=g.b(2, 4, 6, 8), gamma=g.f(8), beta=g.f(8), eps=EPS, out_dtype=BF)


@row("convnext_stem")
def _(g):
    return dict(imgs=g.f(2, 3, 8, 12), wt=g.f(48, 16, scale=0.2), bias=g.f(16), gamma=g.f(16), beta=g.f(16), eps=EPS)


@row("mean_ln")
def _(g):
    return dict(x=g.b(2, 5, 8), gamma=g.f(8), beta=g.f(8), eps=EPS, out_dtype=F32)


@row("window_attention", inplace=("out",))
def _(g):
    return dict(q=g.b(48, 96), k=g.b(48, 96), v=g.b(48, 96), N=2, H=4, W=6, n_heads=3, ws=2, mode="block", bias=g.f(3, 4, 4),
                out=g.z(48, 96, dtype=BF))


@row("dwconv3_bn_act")
def _(g):
    return dict(x=g.b(2, 5, 6, 8), w=g.f(3, 3, 8, scale=0.3), scale=g.f(8), shift=g.f(8), stride=1, gate=g.f(2, 8), want_psum=True)


@row("se_gate")
def _(g):
    return dict(psum=g.f(2, 5, 8), hw=30, w1=g.f(4, 8), b1=g.f(4), w2=g.f(8, 4), b2=g.f(8))


@row("maxvit_stem")
def _(g):
    return dict(imgs=g.f(2, 3, 9, 13), wt=g.f(27, 16, scale=0.2), shift=g.f(16))


@row("im2col3x3")
def _(g):
    return dict(x=g.b(2, 3, 5, 8))


@row("avgpool2x2")
def _(g):
    return dict(x=g.b(2, 4, 6, 8))


@row("conv_bf16")
def _(g):
    return dict(x=g.b(2, 3, 5, 64), w=g.b(16, 3, 3, 64, scale=0.1), bias=g.f(16), stride=1, relu=True, resid=g.b(2, 3, 5, 16))


@row("resnet_stem")
def _(g):
    return dict(imgs=g.f(2, 3, 9, 13), wt=g.f(147, 64, scale=0.1), shift=g.f(64))


@row("attention_hd32")
def _(g):
    return dict(q=g.b(2, 3, 96), k=g.b(2, 5, 96), v=g.b(2, 5, 96), n_heads=3)


@row("mixer_token_mix", inplace=("out",))
def _(g):
    ops = _ops()
    return dict(x=g.b(2, 12, 64), stats=g.stats(24), gamma=g.f(64), beta=g.f(64), w1f=ops.mixer_pack_weight(g.b(32, 12, scale=0.2)),
                b1=g.f(32), w2f=ops.mixer_pack_weight(g.b(12, 32, scale=0.2)), b2=g.f(12), out=g.z(2, 12, 64, dtype=BF),
                want_row_stats=True)


@row("row_stats")
def _(g):
    return dict(x=g.b(5, 24), eps=EPS)


@row("ln_mean")
def _(g):
    return dict(x=g.b(2, 5, 8), stats=g.stats(10), gamma=g.f(8), beta=g.f(8), out_dtype=F32)


@row("transpose_add_f32")
def _(g):
    return dict(x=g.f(2, 3, 5), resid=g.f(2, 5, 3))


@row("conv1d_f32")
def _(g):
    return dict(x=g.f(2, 9, 4), w=g.f(8, 12, scale=0.3), bias=g.f(8), k=3, stride=1, left=1, right=1, elu=True, resid=g.f(2, 9, 8))


@row("lstm_f32")
def _(g):
    return dict(x=g.f(2, 3, 64), w_ih=[g.f(256, 64, scale=0.1) for _ in range(2)], w_hh=[g.f(256, 64, scale=0.1) for _ in range(2)],
                bias=[g.f(256) for _ in range(2)], residual=True)


@row("rvq_encode")
def _(g):
    cb = g.f(2, 1024, 128)
    return dict(z=g.f(3, 128), codebooks=cb, norms=(cb * cb).sum(-1).contiguous(), n_q=2)


@row("rvq_decode")
def _(g):
    return dict(codes=g.i(1024, 2, 3, 5), codebooks=g.f(3, 1024, 128))


@row("groupnorm1_", inplace=("x",))
def _(g):
    return dict(x=g.f(2, 5, 8), gamma=g.f(8), beta=g.f(8), eps=EPS, resid=g.f(2, 5, 8))


@row("encodec_scale")
def _(g):
    return dict(x=g.f(2, 3, 7))


@row("scale_clips")
def _(g):
    return dict(x=g.f(2, 3, 7), scale=g.f(2, 1, 1).abs() + 0.5, divide=True)


@row("cls_head_gemm")
def _(g):
    return dict(x=g.b(5, 2, 32), w=g.b(2, 64, 32, scale=0.1), bias=g.f(128))


@row("cls_attend")
def _(g):
    return dict(x=g.b(2, 5, 64), stats=g.stats(10), u=g.b(2, 3, 64, scale=0.2), scale=0.125, eps=EPS)


@row("lm_score", inplace=("out", "lse_out", "argmax_out", "ws"))
def _(g):
    return dict(h=g.b(5, 16), w=g.b(11, 16), targets=g.i(11, 5, lo=-1), out=g.z(5), lse_out=g.z(5), argmax_out=g.z(5, dtype=I32),
                ws=g.z(_ops().lm_score_ws_bytes(5, 11), dtype=U8))


def _align(g):
    return dict(q=g.b(2, 5, 128, scale=0.5), k=g.b(2, 12, 128, scale=0.5), heads=g.t([1, 0, 1], I32), lengths=g.t([5, 3], I32),
                frames=g.t([12, 8], I32))


@row("align_lse", inplace=("out",))
def _(g):
    return dict(**_align(g), out=g.z(2, 3, 5))


@row("align_matrix", inplace=("m",))
def _(g):
    return dict(**_align(g), lse=g.f(2, 3, 5).abs() + 3.0, m=g.z(2, 5, 12), inv_heads=1.0 / 3, first=True)


@row("align_dtw", inplace=("out", "ws"), host_ok=("lengths", "frames"))
def _(g):
    return dict(m=g.f(2, 5, 12), lengths=g.t([5, 3], I32), frames=g.t([12, 8], I32), out=g.z(2, 5, dtype=I32),
                ws=g.z(_ops().align_ws_bytes(2, 5, 12), dtype=U8))


def _seq(g):
    return _ops().seq_lens([3, 5], 6, g.dev)


@row("attention_varlen", inplace=("out",))
def _(g):
    return dict(q=g.b(8, 128), k=g.b(8, 128), v=g.b(8, 128), n_heads=2, seq=_seq(g), out=g.z(8, 128, dtype=BF), rel_lut=g.f(2, 9), radius=4)


@row("attention_varlen", id="attention_varlen:plain", only=("q", "k", "v", "out"), inplace=("out",))
def _(g):
    return dict(q=g.b(8, 128), k=g.b(8, 128), v=g.b(8, 128), n_heads=2, seq=_seq(g), causal=True, out=g.z(8, 128, dtype=BF))


@row("embed_tokens_varlen")
def _(g):
    return dict(tokens=g.i(11, 2, 6), emb=g.b(11, 32), pos=g.f(9, 32), seq=_seq(g))


@row("rows_pack")
def _(g):
    return dict(x=g.b(2, 6, 16), seq=_seq(g))


@row("rows_unpack")
def _(g):
    return dict(x=g.b(8, 16), seq=_seq(g))


@row("rows_zero_tail", inplace=("x",))
def _(g):
    return dict(x=g.b(2, 6, 16), seq=_seq(g))


@row("segment_mean")
def _(g):
    return dict(x=g.b(8, 16), seq=_seq(g))


@row("ctc_head", inplace=("out", "best_out", "best_logp_out"))
def _(g):
    return dict(h=g.b(5, 16), w=g.b(7, 16), bias=g.f(7), out=g.z(5, 7), best_out=g.z(5, dtype=I32), best_logp_out=g.z(5))


@row("ctc_greedy")
def _(g):
    return dict(best=g.i(7, 8, dtype=I32), seq=_seq(g), best_logp=-g.f(8).abs(), blank=0)


def _ctc(g):
    return dict(logp=torch.log_softmax(g.f(8, 7), -1), seq=_seq(g), targets=g.i(7, 2, 3, dtype=I32, lo=1), target_lengths=g.t([1, 2], I32))


@row("ctc_forward", inplace=("out",), host_ok=("target_lengths",))
def _(g):
    return dict(**_ctc(g), out=g.z(2))


@row("ctc_viterbi", inplace=("ws",), host_ok=("target_lengths",))
def _(g):
    return dict(**_ctc(g), ws=g.z(_ops().ctc_ws_bytes(2, 5, 3), dtype=U8))


# Public functions of ops.py without a row, each with its reason.  Everything else that takes a Tensor must have one.
EXEMPT = {
    "check_devices": "the device check itself (tests/test_device_guard.py)",
    "linear_ln_supported": "host-only query, no tensor operand",
    "linear_plan": "host-only query: launches nothing and dereferences nothing; its checks are linear()'s own (_linear_args)",
    "linear_strided_plan": "host-only query: as linear_plan, through _linear_strided_args",
    "gemm_workspace": "allocates the stream-K workspace; no tensor operand",
    "grouped_conv_supported": "host-only query, no tensor operand",
    "stft_tables": "plain torch on the host (float64 tables); no launch",
    "mel_csr": "plain torch on the host; no launch",
    "dec_linear_plan": "host-only query, no tensor operand",
    "mixer_token_mix_supported": "host-only query, no tensor operand",
    "mixer_token_mix_plan": "host-only query, no tensor operand",
    "mixer_pack_weight": "plain torch repacking; no launch",
    "conv1d_supported": "host-only query, no tensor operand",
    "cls_attend_supported": "host-only query, no tensor operand",
    "lm_score_ws_bytes": "host-only query, no tensor operand",
    "align_ws_bytes": "host-only query, no tensor operand",
    "align_counts": "host validation and one upload; no launch (its device branch is exercised through align_dtw / ctc_*)",
    "seq_lens": "host validation and one upload; no launch",
    "ctc_ws_bytes": "host-only query, no tensor operand",
}

# Tensor parameters a wrapper has that no row passes, each with its reason
UNCOVERED: dict[tuple[str, str], str] = {}


# ------------------------------------------------------------------------------------------------------------------ driver
def call(ops, r: Row, kw: dict):
    return getattr(ops, r.fn)(**kw)


def snapshot(r: Row, kw: dict, res) -> list[tuple[str, Tensor]]:
    """clones of everything a call produced: its outputs and its in-place operands"""
    snap = [(f"output {i}", t.clone()) for i, t in enumerate(flat_outputs(res))]
    for name in r.inplace:
        v = kw.get(name)
        for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, Tensor):
                snap.append((f"{name}[{j}]" if isinstance(v, (list, tuple)) else name, t.clone()))
    return snap


def _diff(a, b) -> list[str]:
    if [n for n, _ in a] != [n for n, _ in b]:
        return [f"results differ in kind: {[n for n, _ in a]} vs {[n for n, _ in b]}"]
    return [n for (n, x), (_, y) in zip(a, b) if not same_bits(x, y)]


def check_row(ops, r: Row, dev, compare: bool, hook=None) -> tuple[list[str], list[tuple[str, str, str]]]:
    """Every variant of every operand of one row: (problems, accepted triples).  A refusal must leave the in-place operands as
    they were; with ``compare`` an accepted call must give the bits of the same call on a fresh contiguous tensor of the
    variant's values (and leave the variant's parent alone outside the view).  ``hook``: the CPU stage's recorder, an object with
    begin() / canonical(kw) / end(row, path, variant, kw, refused) -> list of problems."""
    problems: list[str] = []
    accepted: list[tuple[str, str, str]] = []
    kw0 = r.build(dev)
    if hook:
        hook.begin()
    canon = snapshot(r, kw0, call(ops, r, kw0))
    if hook:
        hook.canonical(kw0)
    for path, t in operands(r.build(dev)):
        if r.only is not None and path[0] not in r.only:
            continue
        for v in variants(t):
            where = f"{r.id} {path_name(path)} {v.tag}"
            v.check_bounds()
            kw = replaced(r.build(dev), path, v.tensor)
            fresh = v.tensor.contiguous().clone() if v.tensor.is_contiguous() else v.tensor.contiguous()
            parent_before = v.parent.clone()
            before = snapshot(r, kw, None)
            if hook:
                hook.begin()
            try:
                res, exc = call(ops, r, kw), None
            except REFUSALS as e:
                if is_fault(e):
                    raise GpuFault(f"{where}: {e}") from e
                res, exc = None, e
                if "pm_mi355x error 3" in str(e):  # PM_ELAUNCH: the launch itself failed - not a refusal in front of it
                    problems.append(f"{where}: {e}")
                    continue
            except Exception as e:  # noqa: BLE001 - anything else is not a refusal the contract allows
                problems.append(f"{where}: raised {type(e).__name__}: {e}")
                continue
            if hook:
                problems += [f"{where}: {p}" for p in hook.end(r, path, v, kw, exc is not None)]
            if exc is not None:
                changed = _diff(before, snapshot(r, kw, None))
                if changed or not same_bits(v.parent, parent_before):
                    problems.append(f"{where}: refused ({exc}) but wrote {changed or 'into the variant'}")
                continue
            accepted.append((r.id, path_name(path), v.tag))
            if v.tag == "expanded" and path[0] in r.inplace:
                problems.append(f"{where}: a stride-0 broadcast was accepted as an operand the kernel writes")
            if v.must_raise and path[0] not in r.free_shape:
                problems.append(f"{where}: a permuted shape was accepted")
            if not compare:
                continue
            got = snapshot(r, kw, res)
            if path[0] in r.inplace and not v.outside_untouched(parent_before):
                problems.append(f"{where}: wrote outside the view")
            if v.reshaped or v.tensor.dtype != t.dtype or v.tag == "expanded":
                kwr = replaced(r.build(dev), path, fresh)
                try:
                    want = snapshot(r, kwr, call(ops, r, kwr))
                except REFUSALS as e:
                    problems.append(f"{where}: accepted, but its contiguous form is refused ({e})")
                    continue
            else:
                want = canon
            bad = _diff(got, want)
            if bad:
                problems.append(f"{where}: accepted but {bad} differ from the contiguous call")
    return problems, accepted


# ------------------------------------------------------------------------------------------- far operands
# An operand whose leading stride carries its last row past 2^31 bytes, 2^32 bytes or 2^31 elements from its base: the three
# distances at which an int32 byte offset, a uint32 byte offset and an int32 element offset stop holding the truth.  Such an
# operand is refused before the first launch, or the call returns the bits of the same call on a compact copy and writes nowhere
# else.  Every far operand is a view into one ARENA, poisoned with POISON32 (NaN as bf16 and as f32, absurd as an integer) and
# based in its middle, sized so that any single ``width``-bit misreading of the far term (``misreadings``) stays inside it: a
# wrap poisons the result, it does not leave the allocation.  All arithmetic is written against ``width`` so that the CPU stage
# can run the same checker at 16 bits over a few hundred kilobytes, with toy kernels that hold one planted defect each.
POISON32 = 0x7FC07FC0
FAR_TAGS = ("far:2G", "far:4G", "far:2Ge")
FAR_ALIGN = 64                    # elements: every alignment a canonical operand has survives a stride that is a multiple of it
ARENA_CAP = 17 << 30              # bytes; a case that asks for more is a bug of the generator


def wrap(v: int, width: int, signed: bool) -> int:
    """``v`` as a ``width``-bit integer register holds it"""
    v &= (1 << width) - 1
    return v - (1 << width) if signed and v >> (width - 1) else v


def far_boundary(tag: str, item: int, width: int = 32) -> int | None:
    """bytes from the base that the last index must pass; None where the tag coincides with a byte distance (bf16 at 2^31
    elements is 2^32 bytes) or does not apply (elements wider than 4 bytes)"""
    half, full = 1 << (width - 1), 1 << width
    if tag == "far:2Ge":
        return None if item > 4 or half * item in (half, full) else half * item
    return {"far:2G": half, "far:4G": full}[tag]


def far_dims(t: Tensor) -> list[int]:
    """the stride-carrying dimensions that ``rowpad`` / ``rowpad0`` vary: the innermost leading dimension with more than one
    index, and the first one of a tensor of three or more dimensions"""
    if t.numel() == 0 or t.dim() < 2:
        return []
    s, dims = tuple(t.shape), []
    if t.numel() > s[-1]:
        dims.append(max(d for d in range(t.dim() - 1) if s[d] > 1))
    if t.dim() >= 3 and s[0] > 1 and 0 not in dims:
        dims.append(0)
    return dims


def far_stride(n: int, item: int, boundary: int) -> int:
    """elements: the smallest multiple of FAR_ALIGN that puts index n - 1 past ``boundary`` bytes"""
    s = -(-(boundary // item + 1) // (n - 1))
    return -(-s // FAR_ALIGN) * FAR_ALIGN


def misreadings(i: int, stride: int, item: int, width: int) -> set[int]:
    """byte offsets at which index ``i`` of the far dimension is looked for by code that forms the term in ``width`` bits at one
    place: the element offset or the byte offset held in a signed or unsigned register, or the stride (in elements or bytes)
    narrowed in front of a wide multiply.  The truth is among them."""
    out = {i * stride * item}
    for sg in (False, True):
        out |= {wrap(i * stride, width, sg) * item, wrap(i * stride * item, width, sg), wrap(stride, width, sg) * i * item,
                wrap(stride * item, width, sg) * i}
    return out


@dataclass
class FarCase:
    tag: str
    dim: int
    tensor: Tensor      # the view handed to the wrapper
    strides: tuple
    item: int
    canon_numel: int
    width: int

    @property
    def name(self) -> str:
        return f"{self.tag}@{self.dim}"

    def needs(self) -> tuple[int, int]:
        """(bytes in front of the base, bytes from the base on) that the containment rule asks of the arena"""
        shape, st, it, w = tuple(self.tensor.shape), self.strides, self.item, self.width
        packed = self.canon_numel * it
        others = sum((n - 1) * s for d, (n, s) in enumerate(zip(shape, st)) if d != self.dim) * it + it
        last = (shape[self.dim] - 1) * st[self.dim]
        # the stated rule: 2^(w-1) units below the base - elements where the element offset itself reaches 2^(w-1), bytes else
        before = ((1 << (w - 1)) * (it if last >= 1 << (w - 1) else 1)) + packed
        after = last * it + others + self.canon_numel * WIDEST
        # and every enumerated misreading of every index, with what the other dimensions add to it
        for i in range(shape[self.dim]):
            for o in misreadings(i, st[self.dim], it, w):
                before, after = max(before, -o), max(after, o + max(others, packed))
        return before, after


class Arena:
    """one allocation for every far operand of a test module: ``nbytes`` of POISON32, views based in the middle"""

    def __init__(self, nbytes: int, device, poisoned: bool = True) -> None:
        assert nbytes % 512 == 0 and nbytes <= ARENA_CAP, nbytes
        self.nbytes, self.base, self.poisoned = nbytes, nbytes // 2, poisoned
        self.words = torch.empty(nbytes // 4, dtype=I32, device=device)
        if poisoned:  # the CPU stage maps its arena lazily and touches the views only
            self.words.fill_(POISON32)

    @staticmethod
    def bytes_for(width: int = 32, slack: int = 16 << 20) -> int:
        """the largest need of any case: an f32 operand at 2^(width-1) elements, that distance on either side, plus slack"""
        return 2 * ((1 << (width - 1)) * 4 + slack)

    def view(self, shape, strides, dtype) -> Tensor:
        item = torch.empty(0, dtype=dtype).element_size()
        return self.words.view(dtype).as_strided(tuple(shape), tuple(strides), self.base // item)

    def holds(self, case: FarCase) -> list[str]:
        """the containment rule as pure arithmetic on base, strides and arena size: the gate in front of any run"""
        before, after = case.needs()
        bad = []
        if before + after > ARENA_CAP:
            bad.append(f"needs {before + after} bytes, more than the cap")
        if before > self.base or after > self.nbytes - self.base:
            bad.append(f"needs {before} bytes in front of the base and {after} behind it; the arena has {self.base} and {self.nbytes - self.base}")
        return bad

    def erase(self, view: Tensor) -> None:
        """the view's elements back to poison"""
        it = view.element_size()
        assert it in (2, 4, 8), "a one-byte far operand would need the poison's phase"
        as_int = {2: torch.int16, 4: I32, 8: I64}[it]
        view.view(as_int).fill_({2: 0x7FC0, 4: POISON32, 8: POISON32 << 32 | POISON32}[it])

    def dirty(self) -> int | None:
        """byte offset of the first word that is not poison, None if there is none (one read of the arena, in pieces)"""
        step = 1 << 28
        counts = [torch.count_nonzero(self.words[a:a + step] != POISON32) for a in range(0, self.words.numel(), step)]
        if not int(torch.stack(counts).sum()):
            return None
        k = next(i for i, c in enumerate(counts) if int(c))
        return 4 * (k * step + int((self.words[k * step:(k + 1) * step] != POISON32).nonzero()[0]))


def far_cases(t: Tensor, arena: Arena, width: int = 32) -> list[FarCase]:
    """every far variant of the canonical operand ``t``: one stride-carrying dimension far, every other stride packed"""
    assert t.is_contiguous()
    out = []
    for d in far_dims(t):
        for tag in FAR_TAGS:
            b = far_boundary(tag, t.element_size(), width)
            if b is None:
                continue
            st = _packed(t.shape)
            st[d] = far_stride(t.shape[d], t.element_size(), b)
            assert (t.shape[d] - 1) * st[d] * t.element_size() > b and st[d] % FAR_ALIGN == 0
            out.append(FarCase(tag, d, arena.view(t.shape, st, t.dtype), tuple(st), t.element_size(), t.numel(), width))
    return out


def applicable_far(t: Tensor, width: int = 32) -> set[tuple[str, int]]:
    """the (tag, dimension) pairs ``far_cases`` must produce, from the layout table's own ``rowpad`` / ``rowpad0`` entries"""
    tags, it, s = applicable_tags(t), t.element_size(), tuple(t.shape)
    dims = set()
    if "rowpad" in tags:
        dims.add(max(d for d in range(t.dim() - 1) if s[d] > 1))
    if "rowpad0" in tags:
        dims.add(0)
    dist = {}
    for tag in FAR_TAGS:  # one tag per distinct byte distance
        b = {"far:2G": 1 << (width - 1), "far:4G": 1 << width, "far:2Ge": (1 << (width - 1)) * it if it <= 4 else None}[tag]
        if b is not None:
            dist.setdefault(b, tag)
    return {(tag, d) for tag in dist.values() for d in dims}


def _far_row(rid: str, fn: str, build, only) -> Row:
    return Row(rid, fn, lambda dev, seed=0: build(Gen(dev, SEED + 977 + seed)), (), tuple(only))


# Rows of the far tests alone.  A stride passes 2^31 elements only where the far dimension has two indices (the last index lies
# just past the boundary, so three rows put the stride at 2^30): these are the table's decode-step GEMMs at M = 2, whose
# launchers hand their row strides to the kernels as int.
FAR_ROWS: dict[str, Row] = {
    "dec_linear:two_rows": _far_row("dec_linear:two_rows", "dec_linear", lambda g: dict(
        x=g.f(2, 64), w=g.b(48, 64, scale=0.1), bias=g.f(48), ln=(g.f(64), g.f(64), EPS), act="gelu", resid=g.f(2, 48)), ("x", "resid")),
    "dec_linear_ksplit:two_rows": _far_row("dec_linear_ksplit:two_rows", "dec_linear_ksplit", lambda g: dict(
        x=g.f(2, 128), w=g.b(48, 128, scale=0.1), bias=g.f(48), k_split=2, act="gelu", resid=g.f(2, 48)), ("x", "resid")),
    "dec_argmax:two_rows": _far_row("dec_argmax:two_rows", "dec_argmax", lambda g: dict(
        x=g.f(2, 64), w=g.b(200, 64, scale=0.1), ln=(g.f(64), g.f(64), EPS)), ("x",)),
}
ALL_FAR_ROWS = {**ROWS, **FAR_ROWS}


def check_row_far(ops, r: Row, dev, arena: Arena, compare: bool, hook=None, width: int = 32):
    """check_row for the far variants: (problems, accepted triples, refused triples).  One operand is far per call, the others
    compact.  A refusal leaves the in-place operands alone; an accepted call gives the canonical call's bits (a far ``out=`` /
    in-place operand holds them in the view) and the arena outside the view stays poison."""
    problems: list[str] = []
    accepted, refused = [], []
    kw0 = r.build(dev)
    if hook:
        hook.begin()
    canon = snapshot(r, kw0, call(ops, r, kw0))
    for path, t in operands(r.build(dev)):
        if r.only is not None and path[0] not in r.only:
            continue
        for c in far_cases(t, arena, width):
            where = f"{r.id} {path_name(path)} {c.name}"
            gate = arena.holds(c)
            if gate:  # never run what the arena cannot contain
                problems += [f"{where}: {g}" for g in gate]
                continue
            c.tensor.copy_(t)
            kw = replaced(r.build(dev), path, c.tensor)
            before = snapshot(r, kw, None)
            if hook:
                hook.begin()
            try:
                res, exc = call(ops, r, kw), None
            except REFUSALS as e:
                if is_fault(e):
                    raise GpuFault(f"{where}: {e}") from e
                res, exc = None, e
                if "pm_mi355x error 3" in str(e):
                    problems.append(f"{where}: {e}")
                    continue
            except Exception as e:  # noqa: BLE001
                problems.append(f"{where}: raised {type(e).__name__}: {e}")
                continue
            if hook:
                problems += [f"{where}: {p}" for p in hook.end_far(r, path, c, kw, exc is not None)]
            got = snapshot(r, kw, res)
            if arena.poisoned:
                arena.erase(c.tensor)
                at = arena.dirty()
                if at is not None:
                    problems.append(f"{where}: {'refused but ' if exc else ''}wrote outside the view, first at byte {at - arena.base:+d} from its base")
                    arena.words.fill_(POISON32)
            if exc is not None:
                refused.append((r.id, path_name(path), c.name))
                changed = _diff(before, got)
                if changed:
                    problems.append(f"{where}: refused ({exc}) but wrote {changed}")
                continue
            accepted.append((r.id, path_name(path), c.name))
            if compare:
                bad = _diff(got, canon)
                if bad:
                    problems.append(f"{where}: accepted but {bad} differ from the compact call")
    return problems, accepted, refused
