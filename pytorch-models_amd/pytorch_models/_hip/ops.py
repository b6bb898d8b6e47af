"""Tensor-level wrappers over the C ABI: validate on the host, pass raw device pointers and the
current torch stream, raise on a non-zero status.  PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes
import os

import torch
from torch import Tensor

from . import ACT, PM_BF16, PM_F32, check, decode_plan as plan, lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device (the capture stream inside torch.cuda.graph).  The raw
    accessors cost ~1 us; torch.cuda.current_stream() builds a Stream object per call (~8 us, a quarter of the host time of
    a launch, which matters for chains of 15-50 us kernels)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _current_device_index() -> int:
    return _cur_device() if _cur_device is not None else torch.cuda.current_device()


def check_devices(*ts) -> None:
    """Every operand on ONE HIP device, and that device the CURRENT one: the C ABI launches on the current device's
    stream with raw pointers, so a tensor of another GPU would be dereferenced by the wrong device (a page fault without
    peer mapping).  Raises instead: call under ``with torch.cuda.device(x.device):`` or, as intended, run one
    process per GPU with ``torch.cuda.set_device(LOCAL_RANK)``."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "pytorch_models (MI355X build) runs on HIP devices only: got a tensor on "
                f"{t.device}. There is no CPU path; move the module and its inputs to 'cuda'.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"pytorch_models (MI355X build): operands on different devices ({dev} and {t.device})")
    if dev is not None and dev.index != _current_device_index():
        raise RuntimeError(
            f"pytorch_models (MI355X build): operands live on {dev} but the current device is cuda:{_current_device_index()}; "
            f"kernels launch on the current device's stream - run under `with torch.cuda.device({dev.index}):` "
            "(one process per GPU with torch.cuda.set_device(LOCAL_RANK) is the intended use)")


# Optional per-launch timing (bench.py's roofline leg): when LAUNCH_LOG is a dict, every wrapped launch is
# bracketed by two HIP events recorded on the stream the kernel is launched on.
LAUNCH_LOG: dict | None = None


def _launch(name: str, work: float, fn):
    if LAUNCH_LOG is None:
        return fn()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    rc = fn()
    e1.record(st)
    LAUNCH_LOG.setdefault(name, []).append((e0, e1, work))
    return rc


def _dt(t: Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return PM_BF16
    if t.dtype == torch.float32:
        return PM_F32
    raise TypeError(f"pm_mi355x kernels take bf16 / f32 tensors, got {t.dtype}")


def _need(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _empty(who: str, count: int, *inner: int) -> bool:
    """The empty-batch contract, called once everything is validated and in front of the launch.  ``count``:
    the number of independent rows or problems of the call (a product where there are several); ``inner``: every extent a result
    element is reduced over or laid out by, and the size of one sample.  True for an empty batch - the caller returns its (empty)
    result and the library is not called: data_ptr() of a tensor without elements is null, which every C entry point refuses -,
    ValueError for an empty inner or sample extent, False (the hot path: two comparisons) otherwise."""
    if count > 0 and 0 not in inner:
        return False
    _need(0 not in inner and count == 0,
          f"{who}: an extent other than the batch is 0 (batch {count}, the others {inner}): only the batch may be empty")
    return True


def _rows(who: str, rows: int, *inner: int) -> None:
    """The decode-step family's side of the empty-batch contract: its state (caches, tickets, the K-split workspace) is allocated
    per batch by the launch plan and the C entry points refuse rows <= 0, so an empty batch is refused here, by name."""
    _need(rows > 0 and 0 not in inner,
          f"{who}: an empty batch or extent is refused (rows {rows}, the others {inner}): a decode step's state is allocated per batch")


def refuse_empty_batch(who: str, *ts) -> None:
    """A model entry point's side of the empty-batch contract where it refuses: ValueError naming the entry point and the empty batch,
    in front of any wrapper call."""
    for t in ts:
        if isinstance(t, Tensor) and t.dim() >= 1 and t.shape[0] == 0:
            raise ValueError(f"{who}: an empty batch is refused (an operand of shape {tuple(t.shape)}): the caches and the launch plan "
                             "of a decoder are allocated per batch")


def capturing() -> bool:
    """The current stream is being captured into a HIP graph.  False wherever no HIP context exists (a process that has not
    touched the GPU cannot be capturing), so the host-only helpers below stay usable without one."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def no_capture(who: str, why: str) -> None:
    """The capture guard: a wrapper or helper that reads device memory on the host, uploads host values or
    synchronises calls this FIRST, in front of any device access.  Under stream capture such a call would either die inside the
    HIP runtime or bake the values of capture time into the graph; it raises instead, naming itself."""
    if capturing():
        raise RuntimeError(f"{who}: {why}, which a stream capture (torch.cuda.graph, GraphedForward) cannot record - "
                           "call it outside the capture and pass device tensors in")


def _cuda(*ts: Tensor) -> None:
    check_devices(*ts)


def _apart(t: Tensor) -> bool:
    """No two elements of ``t`` share an address (strides read only): what a tensor the kernel WRITES through its strides must
    satisfy - a stride-0 broadcast or overlapping rows would be written by several workgroups at once.  Caller-supplied
    tensors only; the ones a wrapper allocates are contiguous."""
    if t.is_contiguous():
        return True
    ext = 1
    for s, n in sorted((s, n) for n, s in zip(t.shape, t.stride()) if n > 1):
        if s < ext:
            return False
        ext += (n - 1) * s
    return True


def _span(t: Tensor) -> tuple[int, int]:
    """[first byte, one past the last byte) of ``t``'s elements (attribute reads only; torch strides are never negative)"""
    p = t.data_ptr()
    if t.is_contiguous():
        return p, p + t.nbytes
    if t.numel() == 0:
        return p, p
    return p, p + (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


def _columns_apart(a: Tensor, b: Tensor) -> bool:
    """``a`` and ``b`` are proven to be disjoint column ranges of one row-major parent: unit last strides, one row pitch that every
    leading stride of both is a multiple of, and column windows [0, wa) and [d, d + wb) that fit side by side in one pitch."""
    if a.dim() < 2 or a.dim() != b.dim() or a.stride(-1) != 1 or b.stride(-1) != 1:
        return False
    ia, ib = a.element_size(), b.element_size()
    lead_a = [s * ia for n, s in zip(a.shape[:-1], a.stride()[:-1]) if n > 1]
    lead_b = [s * ib for n, s in zip(b.shape[:-1], b.stride()[:-1]) if n > 1]
    if not lead_a or not lead_b:
        return False
    pitch = min(lead_a)
    if pitch <= 0 or pitch != min(lead_b) or any(s % pitch for s in lead_a + lead_b):
        return False
    d, wa, wb = (b.data_ptr() - a.data_ptr()) % pitch, a.shape[-1] * ia, b.shape[-1] * ib
    return wa <= d and d + wb <= pitch


def _same_view(a: Tensor, b: Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()


def _unaliased(who: str, wname: str, w: Tensor, names: tuple, others: tuple, may: tuple = ()) -> None:
    """The aliasing contract for ONE caller-supplied operand ``w`` that the call writes, against every other
    tensor operand of the call (``names`` / ``others`` in step; None entries are absent operands): no byte of ``w`` is a byte of
    another operand.  The exception: an operand named in ``may`` - the pairs the kernels support, each "may alias" in
    include/pm_mi355x.h - may be the very same view (pointer, dtype, shape and strides).  Anything else raises ValueError before a
    launch.  Called after the shape and dtype checks, and only when the caller supplied ``w``: a wrapper that allocates its own
    output runs none of this.  Attribute reads only, no device work; the contiguous path is two comparisons per operand."""
    w0 = w.data_ptr()
    w1 = w0 + (w.nbytes if w.is_contiguous() else _span(w)[1] - w0)
    for i, t in enumerate(others):
        if t is None:
            continue
        p = t.data_ptr()
        if p >= w1 or (p < w0 and p + (t.nbytes if t.is_contiguous() else _span(t)[1] - p) <= w0) or w1 == w0:
            continue
        if t.numel() == 0 or _columns_apart(w, t) or (names[i] in may and _same_view(w, t)):
            continue
        raise ValueError(f"{who}: {wname} (written) shares memory with {names[i]}" + (
            f"; {wname} may only be {names[i]} itself, as the same view" if names[i] in may else
            ": an operand the call writes must not overlap another operand"))


def _all_unaliased(who: str, wnames: tuple, ws: tuple, names: tuple, others: tuple) -> None:
    """_unaliased for a call that writes several caller-supplied operands (None: not supplied): each against the written ones
    behind it and against every other operand - two written operands never share memory."""
    for i, w in enumerate(ws):
        if w is not None:
            _unaliased(who, wnames[i], w, wnames[i + 1:] + names, ws[i + 1:] + others)


def linear_ln_supported(M: int, N: int, K: int, act: str, produce: bool) -> bool:
    return bool(lib().pm_linear_ln_supported(M, N, K, ACT[act], int(produce)))


def ln_stats_finalize(partials: Tensor, N: int, eps: float) -> Tensor:
    """(M, N/64, 2) row partials [sum, sum of squares] -> (M, 2) [mean, rstd]."""
    _cuda(partials)
    _need(partials.dim() == 3 and partials.dtype == torch.float32 and partials.is_contiguous() and N % 64 == 0
          and partials.shape[1:] == (N // 64, 2), "ln_stats_finalize: partials must be contiguous f32 (M, N / 64, 2)")
    M = partials.shape[0]
    stats = torch.empty((M, 2), dtype=torch.float32, device=partials.device)
    if _empty("ln_stats_finalize", M, N):
        return stats
    rc = _launch("ln_stats_finalize", float(partials.numel() * 4), lambda: lib().pm_ln_stats_finalize(
        partials.data_ptr(), stats.data_ptr(), M, N, float(eps), _stream()))
    check(rc, "pm_ln_stats_finalize")
    return stats


_GEMM_WS: dict = {}


def gemm_workspace(device: torch.device) -> tuple[int, int]:
    """(pointer, bytes) of the stream-K workspace of (device, current stream): pm_linear_ws_bytes() bytes allocated once per
    stream that ever runs a large GEMM, ticket block zeroed (the kernels leave it zero).  Large GEMMs (M >= 4096) only:
    small problems never take the stream-K kernel, so they never allocate it."""
    key = (device.index, _stream())
    hit = _GEMM_WS.get(key)
    if hit is None:
        n = int(lib().pm_linear_ws_bytes())
        buf = torch.empty(n, dtype=torch.uint8, device=device)
        buf[:4096].zero_()
        hit = _GEMM_WS[key] = (buf, n)
    return hit[0].data_ptr(), hit[1]


_USE_WS = os.environ.get("PM_GEMM_HYBRID", "0") != "0" or os.environ.get("PM_GEMM_STREAMK", "0") != "0" or \
    os.environ.get("PM_GEMM_KERNEL") in ("4", "5")


def _ws_args(M: int, device: torch.device):
    """Workspace for the GEMMs that cut tiles along K (csrc/linear_bf16_sk.hip), both opt-in: the hybrid form (PM_GEMM_HYBRID=1:
    whole tiles plus the last round's tiles in two K halves) and stream-K (PM_GEMM_STREAMK=1).  Neither is on by default: a
    tile cut along K sums differently from a whole one, so a sample's rounding would depend on its position in the batch.
    One workspace per device and stream, allocated at the first large-M call; without it pm_linear_bf16_ws behaves as
    pm_linear_bf16_ln."""
    return gemm_workspace(device) if (_USE_WS and M >= 4096) else (None, 0)


def _linear_bytes(x: Tensor, w: Tensor, out: Tensor, resid: Tensor | None) -> float:
    """algorithmic bytes of one GEMM launch: every operand once (bias and LayerNorm-fold vectors are noise)"""
    n = x.numel() * x.element_size() + w.numel() * w.element_size() + out.numel() * out.element_size()
    return float(n + (resid.numel() * resid.element_size() if resid is not None else 0))


def linear(x: Tensor, w: Tensor, bias: Tensor | None = None, *, act: str = "none", resid: Tensor | None = None,
           out_dtype: torch.dtype = torch.bfloat16, out: Tensor | None = None, ln_stats: Tensor | None = None,
           ln_s: Tensor | None = None, want_row_stats: bool = False, resid_period: int = 0):
    """y = act(x @ w.T + bias) + resid.  x (M, K) bf16, w (N, K) bf16, bias f32 (N), resid (M, N) bf16|f32 - or, with
    resid_period = P > 0, (P, N): row m adds resid[m % P] (a position table broadcast over the batch).
    LayerNorm fold (pm_linear_bf16_ln): ln_stats (M, 2) + ln_s (N) normalise the input rows in the epilogue;
    want_row_stats=True additionally returns the (M, N/64, 2) partial statistics of the output rows."""
    _cuda(x, w, bias, resid, out, ln_stats, ln_s)
    args, out, rows = _linear_args(x, w, bias, act, resid, out_dtype, out, ln_stats, ln_s, want_row_stats, resid_period)
    M, N, K = args[14:17]
    if _empty("linear", M, N, K):
        return (out, rows) if want_row_stats else out
    rc = _launch("linear_bf16", (2.0 * M * N * K, _linear_bytes(x, w, out, resid)), lambda: lib().pm_linear_bf16_ws(*args, _stream()))
    check(rc, f"pm_linear_bf16_ws(M={M}, N={N}, K={K})")
    return (out, rows) if want_row_stats else out


def _linear_args(x, w, bias, act, resid, out_dtype, out, ln_stats, ln_s, want_row_stats, resid_period):
    """The checks of linear() and the arguments of pm_linear_bf16_ws without the stream: (args, out, rows)."""
    _need(x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1], f"linear: x {tuple(x.shape)} vs w {tuple(w.shape)}")
    _need(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "linear: x and w must be bf16")
    _need(x.stride(1) == 1 and w.stride(1) == 1, "linear: x and w must be K-contiguous")
    M, K = x.shape
    N = w.shape[0]
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N, "linear: bias must be f32 (N)")
    given = out is not None
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("linear: rows of out overlap")
    _need(out.shape == (M, N) and out.stride(1) == 1, "linear: bad out")
    if resid is not None:
        _need(resid_period >= 0 and resid.shape == (resid_period or M, N) and resid.stride(1) == 1,
              "linear: resid must be (M, N) - (resid_period, N) when periodic -, row-major")
    if ln_stats is not None or want_row_stats:
        _need((ln_stats is None) == (ln_s is None), "linear: ln_stats and ln_s go together")
        if ln_stats is not None:
            _need(ln_stats.shape == (M, 2) and ln_stats.dtype == torch.float32 and ln_stats.is_contiguous()
                  and ln_s.dtype == torch.float32 and ln_s.numel() == N and ln_s.is_contiguous(), "linear: bad LayerNorm-fold operands")
        rows = torch.empty((M, N // 64, 2), dtype=torch.float32, device=x.device) if want_row_stats else None
    else:
        rows = None
    ws, ws_bytes = _ws_args(M, x.device) if x.is_cuda else (None, 0)
    args = (x.data_ptr(), x.stride(0), 0, 0, w.data_ptr(), w.stride(0), bias.data_ptr() if bias is not None else None,
            resid.data_ptr() if resid is not None else None, resid.stride(0) if resid is not None else 0,
            _dt(resid) if resid is not None else 0, resid_period if resid is not None else 0, out.data_ptr(), out.stride(0),
            _dt(out), M, N, K, ACT[act], ln_stats.data_ptr() if ln_stats is not None else None,
            ln_s.data_ptr() if ln_s is not None else None, rows.data_ptr() if rows is not None else None, ws, ws_bytes)
    if given:
        # The aliasing contract on the integers the launch takes anyway: out's bytes [op, o1) against every
        # other operand's, each extent exact (last row's end).  Whatever this cannot prove apart goes to the shared helper, which
        # knows column ranges and the one honoured alias - resid may be out itself: every kernel reads a residual element in the
        # workgroup that stores it, before the store; a periodic residual row is read by many tiles, and the opt-in K-cut kernels
        # finish a tile in two workgroups - and refuses the rest.
        xp, ldx, _, _, wp, ldw, bp, rp, ldr, rdt, _, op, ldo, odt = args[:14]
        sp, lp = args[18], args[19]
        o1 = op + ((M - 1) * ldo + N) * (2 if odt == PM_BF16 else 4)
        if not ((xp >= o1 or xp + ((M - 1) * ldx + K) * 2 <= op) and (wp >= o1 or wp + ((N - 1) * ldw + K) * 2 <= op)
                and (bp is None or bp >= o1 or bp + 4 * N <= op)
                and (rp is None or rp >= o1 or rp + (((resid_period or M) - 1) * ldr + N) * (2 if rdt == PM_BF16 else 4) <= op)
                and (sp is None or sp >= o1 or sp + 8 * M <= op) and (lp is None or lp >= o1 or lp + 4 * N <= op)):
            _unaliased("linear", "out", out, ("x", "w", "bias", "resid", "ln_stats", "ln_s"), (x, w, bias, resid, ln_stats, ln_s),
                       ("resid",) if resid_period == 0 and not _USE_WS else ())
    return args, out, rows


def linear_plan(x: Tensor, w: Tensor, bias: Tensor | None = None, *, act: str = "none", resid: Tensor | None = None,
                out_dtype: torch.dtype = torch.bfloat16, out: Tensor | None = None, ln_stats: Tensor | None = None,
                ln_s: Tensor | None = None, want_row_stats: bool = False, resid_period: int = 0) -> int:
    """pm_linear_bf16_plan: the kernel id (1 .. 7) linear() would launch with these operands - the arguments are built by the
    same function -, 0 for M == 0 (linear() then returns its empty result without a launch, and the library is not asked: an empty
    operand's pointer is null, which the C query refuses as it refuses any null pointer), or minus the error code; N == 0 or K == 0
    raise as they do in linear().  Host arithmetic only: nothing is launched and the tensors may live on the CPU (pointers are looked
    at for null and alignment).  PM_GEMM_KERNEL is read once per process."""
    args, _, _ = _linear_args(x, w, bias, act, resid, out_dtype, out, ln_stats, ln_s, want_row_stats, resid_period)
    if _empty("linear_plan", *args[14:17]):
        return 0
    return int(lib().pm_linear_bf16_plan(*args))


def linear_f32(x: Tensor, w: Tensor, bias: Tensor | None = None, *, act: str = "none", resid: Tensor | None = None,
               resid_period: int = 0, out: Tensor | None = None, M: int | None = None, K: int | None = None, row_stride: int | None = None,
               rows_per_batch: int = 0, batch_stride: int = 0) -> Tensor:
    """pm_linear_f32: y = act(x @ w.T + bias) + resid with every operand fp32 (exact-fp32 MFMA).  Plain form: x (M, K) with unit
    column stride.  Window form (M, K, row_stride[, rows_per_batch, batch_stride] given): row m of the A operand is the K
    contiguous floats at x + (m // rows_per_batch) * batch_stride + (m % rows_per_batch) * row_stride, as in linear_strided."""
    _cuda(x, w, bias, resid, out)
    _need(x.dtype == torch.float32 and w.dtype == torch.float32 and w.dim() == 2 and w.stride(1) == 1, "linear_f32: x, w must be f32, w (N, K)")
    if M is None:
        _need(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == w.shape[1], f"linear_f32: x {tuple(x.shape)} vs w {tuple(w.shape)}")
        M, K, row_stride = x.shape[0], x.shape[1], x.stride(0)
    else:
        _need(K == w.shape[1] and row_stride is not None, "linear_f32: window form needs M, K, row_stride")
    N = w.shape[0]
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N, "linear_f32: bias must be f32 (N)")
    if resid is not None:
        _need(resid.dtype == torch.float32 and resid.dim() == 2 and resid.shape[1] == N and resid.stride(1) == 1
              and resid.shape[0] >= (resid_period or M), "linear_f32: resid must be f32 (rows, N)")
    given = out is not None
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("linear_f32: rows of out overlap")
    _need(out.dtype == torch.float32 and out.shape == (M, N) and out.stride(1) == 1, "linear_f32: bad out")
    if given:
        _unaliased("linear_f32", "out", out, ("x", "w", "bias", "resid"), (x, w, bias, resid))
    if _empty("linear_f32", M, N, K):
        return out
    rc = _launch("linear_f32", 2.0 * M * N * K, lambda: lib().pm_linear_f32(
        x.data_ptr(), row_stride, rows_per_batch, batch_stride, w.data_ptr(), w.stride(0), bias.data_ptr() if bias is not None else None,
        resid.data_ptr() if resid is not None else None, resid.stride(0) if resid is not None else 0, resid_period, out.data_ptr(),
        out.stride(0), M, N, K, ACT[act], _stream()))
    check(rc, f"pm_linear_f32(M={M}, N={N}, K={K})")
    return out


def attention_f32(q: Tensor, k: Tensor, v: Tensor, n_heads: int, causal: bool = False, bias: Tensor | None = None) -> Tensor:
    """attention() on fp32 operands: q (B, Lq, H*hd), k / v (B, Lk, H*hd) f32 views with unit last stride -> (B, Lq, H*hd) f32.
    head_dim % 4 == 0 (<= 128) or % 2 == 0 (<= 64), Lk <= 2048; bias as in attention()."""
    _cuda(q, k, v, bias)
    _need(q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "attention_f32: operands must be (B, L, H*hd)")
    B, Lq, D = q.shape
    Lk = k.shape[1]
    _need(n_heads > 0 and D % n_heads == 0 and k.shape == (B, Lk, D) and v.shape == (B, Lk, D), "attention_f32: shape mismatch")
    for t in (q, k, v):
        _need(t.dtype == torch.float32 and t.stride(2) == 1, "attention_f32: f32 operands with unit last stride")
    out = torch.empty((B, Lq, D), dtype=torch.float32, device=q.device)
    sb = sh = sq = 0
    if bias is not None:
        _need(bias.dim() == 4 and bias.dtype == torch.float32 and bias.shape[2:] == (Lq, Lk) and bias.stride(3) == 1
              and bias.shape[0] in (1, B) and bias.shape[1] in (1, n_heads), "attention_f32: bias must be f32 (1|B, 1|H, Lq, Lk)")
        sb = 0 if bias.shape[0] == 1 else bias.stride(0)
        sh = 0 if bias.shape[1] == 1 else bias.stride(1)
        sq = bias.stride(2)
    if _empty("attention_f32", B * Lq, Lk, D):
        return out
    rc = _launch("attention_f32", 4.0 * B * n_heads * Lq * Lk * (D // n_heads), lambda: lib().pm_attention_generic_f32(
        q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1),
        out.data_ptr(), out.stride(0), out.stride(1), B, n_heads, Lq, Lk, D // n_heads, int(causal),
        bias.data_ptr() if bias is not None else None, sb, sh, sq, _stream()))
    check(rc, f"pm_attention_generic_f32(B={B}, H={n_heads}, Lq={Lq}, Lk={Lk}, hd={D // n_heads})")
    return out


def layernorm(x: Tensor, gamma: Tensor | None, beta: Tensor | None, eps: float, out_dtype: torch.dtype | None = None,
              act: str = "none", resid: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """Row-wise LayerNorm of x (M, d) (bf16 | f32) with f32 gamma / beta (both None = no affine), optionally followed by
    GELU and a residual add (pm_layernorm_ex).  ``out``: a (M, d) row-major tensor to write instead of a new one."""
    _cuda(x, gamma, beta, resid, out)
    _need(x.dim() == 2 and x.stride(1) == 1, "layernorm: x must be (M, d), row-major")
    M, d = x.shape
    _need((gamma is None) == (beta is None), "layernorm: gamma and beta come together")
    if gamma is not None:
        _need(gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == d and beta.numel() == d
              and gamma.is_contiguous() and beta.is_contiguous(), "layernorm: gamma / beta must be contiguous f32 (d)")
    if resid is not None:
        _need(resid.shape == x.shape and resid.stride(1) == 1, "layernorm: resid must be (M, d), row-major")
    given = out is not None
    if out is None:
        out = torch.empty((M, d), dtype=out_dtype or x.dtype, device=x.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("layernorm: rows of out overlap")
    _need(out.shape == (M, d) and out.stride(1) == 1, "layernorm: out must be (M, d), row-major")
    if _empty("layernorm", M, d):
        return out
    gp, bp = (gamma.data_ptr(), beta.data_ptr()) if gamma is not None else (None, None)
    if given:  # a caller's out: every pointer and stride fetched once, for the aliasing check and for the launch; a call that lets
        # layernorm() allocate its result runs the code below, unchanged
        xp, ldx, xdt, ex, op, ldo, odt, eo = x.data_ptr(), x.stride(0), _dt(x), x.element_size(), out.data_ptr(), out.stride(0), _dt(out), out.element_size()
        rp, ldr, rdt, er = (resid.data_ptr(), resid.stride(0), _dt(resid), resid.element_size()) if resid is not None else (None, 0, 0, 0)
        # the aliasing contract on the integers the launch takes anyway: out's bytes [op, o1) against every other
        # operand's exact extent; what this cannot prove apart goes to the shared helper (column ranges of one parent, the refusal)
        m1 = M - 1
        o1 = op + (m1 * ldo + d) * eo
        if not ((xp >= o1 or xp + (m1 * ldx + d) * ex <= op)
                and (gp is None or ((gp >= o1 or gp + 4 * d <= op) and (bp >= o1 or bp + 4 * d <= op)))
                and (rp is None or rp >= o1 or rp + (m1 * ldr + d) * er <= op)):
            _unaliased("layernorm", "out", out, ("x", "gamma", "beta", "resid"), (x, gamma, beta, resid))
        nbytes = float(M * d * (ex + eo + er))
        if act == "none" and resid is None and gamma is not None:
            largs = (xp, ldx, xdt, gp, bp, float(eps), op, ldo, odt, M, d)  # (one closure variable: the plain path's cells stay as they were)
            rc = _launch("layernorm", nbytes, lambda: lib().pm_layernorm(*largs, _stream()))
        else:
            largs = (xp, ldx, xdt, gp, bp, float(eps), ACT[act], rp, ldr, rdt, op, ldo, odt, M, d)
            rc = _launch("layernorm", nbytes, lambda: lib().pm_layernorm_ex(*largs, _stream()))
        check(rc, f"pm_layernorm(M={M}, d={d})")
        return out
    nbytes = float(M * d * (x.element_size() + out.element_size() + (resid.element_size() if resid is not None else 0)))
    if act == "none" and resid is None and gamma is not None:
        rc = _launch("layernorm", nbytes, lambda: lib().pm_layernorm(
            x.data_ptr(), x.stride(0), _dt(x), gp, bp, float(eps), out.data_ptr(), out.stride(0), _dt(out), M, d, _stream()))
    else:
        rc = _launch("layernorm", nbytes, lambda: lib().pm_layernorm_ex(
            x.data_ptr(), x.stride(0), _dt(x), gp, bp, float(eps), ACT[act],
            resid.data_ptr() if resid is not None else None, resid.stride(0) if resid is not None else 0,
            _dt(resid) if resid is not None else 0, out.data_ptr(), out.stride(0), _dt(out), M, d, _stream()))
    check(rc, f"pm_layernorm(M={M}, d={d})")
    return out


def rmsnorm(x: Tensor, gamma: Tensor, eps: float, out_dtype: torch.dtype | None = None) -> Tensor:
    """pm_rmsnorm: x (M, d) bf16 | f32 -> x * rsqrt(mean(x^2) + eps) * gamma (f32 gamma)."""
    _cuda(x, gamma)
    _need(x.dim() == 2 and x.stride(1) == 1, "rmsnorm: x must be (M, d), row-major")
    M, d = x.shape
    _need(gamma.dtype == torch.float32 and gamma.numel() == d and gamma.is_contiguous(), "rmsnorm: gamma must be contiguous f32 (d)")
    out = torch.empty((M, d), dtype=out_dtype or x.dtype, device=x.device)
    if _empty("rmsnorm", M, d):
        return out
    rc = _launch("layernorm", float(M * d * (x.element_size() + out.element_size())), lambda: lib().pm_rmsnorm(
        x.data_ptr(), x.stride(0), _dt(x), gamma.data_ptr(), float(eps), out.data_ptr(), out.stride(0), _dt(out), M, d, _stream()))
    check(rc, f"pm_rmsnorm(M={M}, d={d})")
    return out


def geglu(h: Tensor) -> Tensor:
    """pm_geglu: bf16 (M, 2F) -> (M, F) = gelu_tanh(h[:, :F]) * h[:, F:]."""
    _cuda(h)
    _need(h.dim() == 2 and h.dtype == torch.bfloat16 and h.stride(1) == 1 and h.shape[1] % 2 == 0, "geglu: bf16 (M, 2F) rows")
    M, F = h.shape[0], h.shape[1] // 2
    out = torch.empty((M, F), dtype=torch.bfloat16, device=h.device)
    if _empty("geglu", M, F):
        return out
    rc = _launch("geglu", float(M * F * 6), lambda: lib().pm_geglu(h.data_ptr(), h.stride(0), out.data_ptr(), out.stride(0), M, F, _stream()))
    check(rc, f"pm_geglu(M={M}, F={F})")
    return out


def attention(q: Tensor, k: Tensor, v: Tensor, n_heads: int, causal: bool = False, bias: Tensor | None = None,
              out: Tensor | None = None) -> Tensor:
    """q (B, Lq, H*hd), k / v (B, Lk, H*hd) bf16 views with unit last stride (e.g. column slices of a packed
    QKV projection) -> (B, Lq, H*hd) bf16, heads already merged.  bias: optional additive f32 (b, h, Lq, Lk) with
    b in {1, B}, h in {1, H} (size-1 dims broadcast).  head_dim 64 runs on the MFMA kernel, other head dims
    (% 4 == 0 up to 128, % 2 == 0 up to 64: MobileViT's 16 .. 60) on the generic one.  ``out``: a bf16 (B, Lq, H*hd) tensor with
    unit last stride to write instead of a new one."""
    _cuda(q, k, v, bias, out)
    _need(q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "attention: operands must be (B, L, H*hd)")
    B, Lq, D = q.shape
    Lk = k.shape[1]
    _need(n_heads > 0 and D % n_heads == 0 and k.shape == (B, Lk, D) and v.shape == (B, Lk, D), "attention: shape mismatch")
    hd = D // n_heads
    for t in (q, k, v):
        _need(t.dtype == torch.bfloat16 and t.stride(2) == 1, "attention: bf16 operands with unit last stride")
    given = out is not None
    if out is None:
        out = torch.empty((B, Lq, D), dtype=torch.bfloat16, device=q.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("attention: rows of out overlap")
    _need(out.shape == (B, Lq, D) and out.dtype == torch.bfloat16 and out.stride(2) == 1, "attention: out must be bf16 (B, Lq, H*hd)")
    args = (q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0),
            v.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B, n_heads, Lq, Lk, int(causal))
    sb = sh = sq = 0
    bp = None
    empty = _empty("attention", B * Lq, Lk, D)
    if bias is not None:
        _need(bias.dim() == 4 and bias.dtype == torch.float32 and bias.shape[2:] == (Lq, Lk) and bias.stride(3) == 1
              and bias.shape[0] in (1, B) and bias.shape[1] in (1, n_heads), "attention: bias must be f32 (1|B, 1|H, Lq, Lk)")
        sb = 0 if bias.shape[0] == 1 else bias.stride(0)
        sh = 0 if bias.shape[1] == 1 else bias.stride(1)
        sq = bias.stride(2)
        bp = bias.data_ptr()
    if empty:
        return out
    if given:
        # the aliasing contract on the integers the launch takes anyway: out's bytes [op, oe) against the exact
        # extents of q, k, v and the bias (sb / sh are 0 for a broadcast dimension); whatever this cannot prove apart (column slices
        # of one packed projection) goes to the shared helper, which refuses what overlaps
        qp, q0, q1, kp, k0, k1, vp, v0, v1, op, o0, o1 = args[:12]
        b1, l1, m1 = B - 1, Lq - 1, Lk - 1
        oe = op + (b1 * o0 + l1 * o1 + D) * 2
        if not ((qp >= oe or qp + (b1 * q0 + l1 * q1 + D) * 2 <= op) and (kp >= oe or kp + (b1 * k0 + m1 * k1 + D) * 2 <= op)
                and (vp >= oe or vp + (b1 * v0 + m1 * v1 + D) * 2 <= op)
                and (bp is None or bp >= oe or bp + (b1 * sb + (n_heads - 1) * sh + l1 * sq + Lk) * 4 <= op)):
            _unaliased("attention", "out", out, ("q", "k", "v", "bias"), (q, k, v, bias))
    if hd != 64:
        rc = _launch("attention_generic", 4.0 * B * n_heads * Lq * Lk * hd, lambda: lib().pm_attention_generic_bf16(
            *args[:16], hd, int(causal), bp, sb, sh, sq, _stream()))
    elif bias is None:
        rc = _launch("attention_bf16", 4.0 * B * n_heads * Lq * Lk * 64, lambda: lib().pm_attention_bf16(*args, _stream()))
    else:
        rc = _launch("attention_bf16", 4.0 * B * n_heads * Lq * Lk * 64, lambda: lib().pm_attention_bias_bf16(
            *args, bp, sb, sh, sq, _stream()))
    check(rc, f"pm_attention_bf16(B={B}, H={n_heads}, Lq={Lq}, Lk={Lk})")
    return out


def conv2d_nhwc(x: Tensor, w: Tensor, bias: Tensor | None, stride: int = 1, pad: int = 0, groups: int = 1, act: str = "none",
                resid: Tensor | None = None) -> Tensor:
    """x (N, H, W, Cin) bf16, w (Cout, kh, kw, Cin / groups) bf16 (a BatchNorm already folded in), bias f32 (Cout) ->
    (N, Ho, Wo, Cout) bf16; optional residual of the output's shape added after the activation (pm_conv2d_nhwc_bf16)."""
    _cuda(x, w, bias, resid)
    _need(x.dim() == 4 and w.dim() == 4 and x.is_contiguous() and w.is_contiguous(), "conv2d_nhwc: contiguous NHWC x and (Cout, kh, kw, Cin/g) w")
    _need(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "conv2d_nhwc: bf16 operands")
    N, H, W, Cin = x.shape
    Cout, kh, kw, cg = w.shape
    _need(groups > 0 and stride > 0 and Cin % groups == 0 and Cout % groups == 0 and cg == Cin // groups, "conv2d_nhwc: channel / group mismatch")
    empty = _empty("conv2d_nhwc", N, H, W, Cin, Cout, kh, kw)
    _need(bias is None or (bias.dtype == torch.float32 and bias.numel() == Cout and bias.is_contiguous()),
          "conv2d_nhwc: bias must be contiguous f32 (Cout)")
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    out = torch.empty((N, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    _need(resid is None or (resid.shape == out.shape and resid.dtype == torch.bfloat16 and resid.is_contiguous()), "conv2d_nhwc: resid must match the output")
    if empty:
        return out
    rc = _launch("conv2d_nhwc", 2.0 * N * Ho * Wo * Cout * kh * kw * cg, lambda: lib().pm_conv2d_nhwc_bf16(
        x.data_ptr(), N, H, W, Cin, w.data_ptr(), bias.data_ptr() if bias is not None else None,
        resid.data_ptr() if resid is not None else None, out.data_ptr(), Cout, kh, kw, stride, pad, groups, ACT[act], _stream()))
    check(rc, f"pm_conv2d_nhwc_bf16(N={N}, H={H}, W={W}, Cin={Cin}, Cout={Cout}, k={kh}x{kw}, stride={stride}, groups={groups})")
    return out


def mean_rows(x: Tensor) -> Tensor:
    """x (N, R, C) bf16 contiguous -> (N, C) bf16: the mean over the R rows of each sample (pm_mean_rows_bf16)."""
    _cuda(x)
    _need(x.dim() == 3 and x.is_contiguous() and x.dtype == torch.bfloat16, "mean_rows: contiguous bf16 (N, R, C)")
    N, R, C = x.shape
    out = torch.empty((N, C), dtype=torch.bfloat16, device=x.device)
    if _empty("mean_rows", N, R, C):
        return out
    rc = _launch("mean_rows", 1.0 * N * R * C, lambda: lib().pm_mean_rows_bf16(x.data_ptr(), out.data_ptr(), N, R, C, _stream()))
    check(rc, f"pm_mean_rows_bf16(N={N}, R={R}, C={C})")
    return out


def vit_tokens(imgs: Tensor, w2d: Tensor, bias: Tensor, pe: Tensor, cls: Tensor | None, patch: int) -> Tensor:
    """imgs f32 (N, 3, H, W) -> tokens bf16 (N, L [+1], d): patch projection + pe (+ cls row)."""
    _cuda(imgs, w2d, bias, pe, cls)
    _need(imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype == torch.float32 and imgs.is_contiguous(),
          "vit_tokens: imgs must be contiguous f32 (N, 3, H, W)")
    N, _, H, W = imgs.shape
    d = w2d.shape[0]
    _need(patch > 0, "vit_tokens: the patch size must be positive")
    L = (H // patch) * (W // patch)
    K = 3 * patch * patch
    _need(w2d.dtype == torch.bfloat16 and w2d.is_contiguous() and w2d.shape[0] == d and w2d.shape[1] >= K, "vit_tokens: bad weight")
    _need(bias.dtype == torch.float32 and bias.numel() == d and bias.is_contiguous(), "vit_tokens: bias f32 (d)")
    _need(pe.dtype == torch.float32 and pe.numel() == L * d and pe.is_contiguous(),
          f"vit_tokens: pe must hold {L} x {d} f32 values (image {H}x{W}, patch {patch}); call resize_pe first")
    if cls is not None:
        _need(cls.dtype == torch.float32 and cls.numel() == d and cls.is_contiguous(), "vit_tokens: cls f32 (d)")
    out = torch.empty((N, L + (cls is not None), d), dtype=torch.bfloat16, device=imgs.device)
    if _empty("vit_tokens", N, L, d):
        return out
    if patch == 16 and w2d.shape[1] == K:
        rc = _launch("vit_tokens", float(imgs.numel() * 4 + out.numel() * 2), lambda: lib().pm_vit_tokens(
            imgs.data_ptr(), w2d.data_ptr(), bias.data_ptr(), pe.data_ptr(),
            cls.data_ptr() if cls is not None else None, out.data_ptr(), N, H, W, patch, d, _stream()))
    else:  # any other patch size: K zero-padded to a multiple of 64 in the packed weight
        _need(w2d.shape[1] % 64 == 0, "vit_tokens: generic path needs the weight zero-padded to a multiple of 64 columns")
        rc = _launch("vit_tokens", float(imgs.numel() * 4 + out.numel() * 2), lambda: lib().pm_vit_tokens_generic(
            imgs.data_ptr(), w2d.data_ptr(), w2d.shape[1], bias.data_ptr(), pe.data_ptr(),
            cls.data_ptr() if cls is not None else None, out.data_ptr(), N, H, W, patch, d, _stream()))
    check(rc, f"pm_vit_tokens(N={N}, H={H}, W={W}, P={patch}, d={d})")
    return out


def linear_strided(x: Tensor, *, M: int, K: int, row_stride: int, rows_per_batch: int, batch_stride: int, w: Tensor,
                   bias: Tensor | None = None, act: str = "none", resid: Tensor | None = None, resid_period: int = 0,
                   out_dtype: torch.dtype = torch.bfloat16, out: Tensor | None = None) -> Tensor:
    """pm_linear_bf16_ex: row m of the A operand is the K contiguous bf16 values at
    x.flat[(m // rows_per_batch) * batch_stride + (m % rows_per_batch) * row_stride : ... + K] (rows may overlap:
    that is how a strided conv window is expressed); resid rows repeat every resid_period rows."""
    _cuda(x, w, bias, resid, out)
    args, out = _linear_strided_args(x, M, K, row_stride, rows_per_batch, batch_stride, w, bias, act, resid, resid_period, out_dtype, out)
    N = w.shape[0]
    if _empty("linear_strided", M, N, K):
        return out
    rc = _launch("linear_bf16", 2.0 * M * N * K, lambda: lib().pm_linear_bf16_ws(*args, _stream()))
    check(rc, f"pm_linear_bf16_ws(M={M}, N={N}, K={K})")
    return out


def _linear_strided_args(x, M, K, row_stride, rows_per_batch, batch_stride, w, bias, act, resid, resid_period, out_dtype, out):
    """The checks of linear_strided() and the arguments of pm_linear_bf16_ws without the stream: (args, out)."""
    _need(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous() and w.dim() == 2 and w.stride(1) == 1,
          "linear_strided: contiguous bf16 x, K-contiguous bf16 w")
    _need(w.shape[1] == K and rows_per_batch > 0 and M % rows_per_batch == 0, "linear_strided: bad geometry")
    nb = M // rows_per_batch
    last = (nb - 1) * batch_stride + (rows_per_batch - 1) * row_stride + K
    _need(last <= x.numel(), f"linear_strided: window runs past the buffer ({last} > {x.numel()})")
    N = w.shape[0]
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N, "linear_strided: bias f32 (N)")
    if resid is not None:
        _need(resid.dim() == 2 and resid.shape[1] == N and resid.stride(1) == 1, "linear_strided: resid (rows, N)")
        _need(resid.shape[0] >= (resid_period or M), "linear_strided: resid has too few rows")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    else:  # e.g. a column slice of a wider matrix (one group of a grouped conv)
        _need(out.shape == (M, N) and out.stride(1) == 1 and (out.is_cuda or not x.is_cuda) and _apart(out),
              "linear_strided: out must be (M, N) with unit column stride and rows that do not overlap")
        _unaliased("linear_strided", "out", out, ("x", "w", "bias", "resid"), (x, w, bias, resid))
    ws, ws_bytes = _ws_args(M, out.device) if out.is_cuda else (None, 0)
    args = (x.data_ptr(), row_stride, rows_per_batch, batch_stride, w.data_ptr(), w.stride(0),
            bias.data_ptr() if bias is not None else None, resid.data_ptr() if resid is not None else None,
            resid.stride(0) if resid is not None else 0, _dt(resid) if resid is not None else 0, resid_period,
            out.data_ptr(), out.stride(0), _dt(out), M, N, K, ACT[act], None, None, None, ws, ws_bytes)
    return args, out


def linear_strided_plan(x: Tensor, *, M: int, K: int, row_stride: int, rows_per_batch: int, batch_stride: int, w: Tensor,
                        bias: Tensor | None = None, act: str = "none", resid: Tensor | None = None, resid_period: int = 0,
                        out_dtype: torch.dtype = torch.bfloat16, out: Tensor | None = None) -> int:
    """linear_plan for the window form: pm_linear_bf16_plan on the arguments linear_strided() would pass (built by the same
    function).  Host arithmetic only; the tensors may live on the CPU."""
    args, _ = _linear_strided_args(x, M, K, row_stride, rows_per_batch, batch_stride, w, bias, act, resid, resid_period, out_dtype, out)
    if _empty("linear_strided_plan", *args[14:17]):
        return 0
    return int(lib().pm_linear_bf16_plan(*args))


def w2v_stem0(x: Tensor, w: Tensor, bias: Tensor | None, norm: str, gamma: Tensor | None, beta: Tensor | None,
              eps: float, stride: int) -> Tensor:
    """pm_w2v_stem0: f32 waveform (B, L) -> bf16 (B, T0, C0) = GELU(norm(Conv1d(1, C0, k, stride)(x))), time-major.
    norm: "none" | "layer" (over channels) | "instance" (over time, per clip and channel)."""
    _cuda(x, w, bias, gamma, beta)
    _need(x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous(), "w2v_stem0: x must be contiguous f32 (B, L)")
    _need(w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous(), "w2v_stem0: w must be contiguous f32 (C0, k)")
    for t in (bias, gamma, beta):
        _need(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == w.shape[0]), "w2v_stem0: f32 (C0) vectors")
    B, L = x.shape
    C0, k = w.shape
    _need(L >= k and stride > 0, f"w2v_stem0: waveform shorter than the kernel ({L} < {k})")
    T0 = (L - k) // stride + 1
    empty = _empty("w2v_stem0", B, L, C0, k)
    mode = {"none": 0, "layer": 1, "instance": 2}[norm]
    out = torch.empty((B, T0, C0), dtype=torch.bfloat16, device=x.device)
    partials = stats = None
    if empty:
        return out
    if mode == 2:
        partials = torch.empty(int(lib().pm_w2v_stem0_scratch_floats(B, T0)), dtype=torch.float32, device=x.device)
        stats = torch.empty((B, C0, 2), dtype=torch.float32, device=x.device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = _launch("w2v_stem0", float(B * T0 * C0 * 2 + B * L * 4), lambda: lib().pm_w2v_stem0(
        x.data_ptr(), w.data_ptr(), ptr(bias), mode, ptr(gamma), ptr(beta), float(eps), ptr(partials), ptr(stats),
        out.data_ptr(), B, L, C0, k, stride, _stream()))
    check(rc, f"pm_w2v_stem0(B={B}, L={L}, C0={C0}, k={k}, norm={norm})")
    return out


def group_windows(x: Tensor, groups: int, cgp: int, pad_left: int, pad_right: int) -> Tensor:
    """pm_group_windows: (B, T, d) bf16 | f32 -> bf16 (B, G, pad_left + T + pad_right, cgp), group-major, zero-padded."""
    _cuda(x)
    _need(x.dim() == 3 and x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1), "group_windows: (B, T, d) rows")
    B, T, d = x.shape
    _need(groups > 0 and d % groups == 0, "group_windows: d must divide into the groups")
    cg = d // groups
    out = torch.empty((B, groups, pad_left + T + pad_right, cgp), dtype=torch.bfloat16, device=x.device)
    if _empty("group_windows", B, T, d, cgp):
        return out
    rc = _launch("group_windows", float(x.numel() * x.element_size() + out.numel() * 2), lambda: lib().pm_group_windows(
        x.data_ptr(), x.stride(1), _dt(x), out.data_ptr(), B, T, groups, cg, cgp, pad_left, pad_right, _stream()))
    check(rc, f"pm_group_windows(B={B}, T={T}, d={d}, G={groups})")
    return out


def grouped_conv_supported(cg: int, cgp: int) -> bool:
    return bool(lib().pm_grouped_conv_supported(cg, cgp))


def grouped_conv(xg: Tensor, w: Tensor, bias: Tensor | None, k: int, stride: int, cg: int, act: str = "none",
                 resid: Tensor | None = None) -> Tensor:
    """pm_grouped_conv_bf16: xg bf16 (B, G, Tp, cgp) from group_windows, w bf16 (G, cg, Kp) (K order (tap, channel), zero-padded to
    a multiple of 64) -> bf16 (B * To, G * cg) = act(conv + bias) + resid."""
    _cuda(xg, w, bias, resid)
    _need(xg.dim() == 4 and xg.dtype == torch.bfloat16 and xg.is_contiguous(), "grouped_conv: xg must be contiguous bf16 (B, G, Tp, cgp)")
    B, G, Tp, cgp = xg.shape
    _need(w.dtype == torch.bfloat16 and w.is_contiguous() and w.shape[:2] == (G, cg), "grouped_conv: w must be contiguous bf16 (G, cg, Kp)")
    Kp = w.shape[2]
    _need(stride > 0 and Tp >= k, f"grouped_conv: {Tp} padded steps are fewer than the {k} taps")
    To = (Tp - k) // stride + 1
    d = G * cg
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == d, "grouped_conv: bias f32 (G*cg)")
    if resid is not None:
        _need(resid.dtype == torch.bfloat16 and resid.shape == (B * To, d) and resid.stride(1) == 1, "grouped_conv: resid bf16 (B*To, d)")
    out = torch.empty((B * To, d), dtype=torch.bfloat16, device=xg.device)
    if _empty("grouped_conv", B, G, To, cg, cgp, k, Kp):
        return out
    rc = _launch("grouped_conv", 2.0 * B * To * d * k * cg, lambda: lib().pm_grouped_conv_bf16(
        xg.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None,
        resid.data_ptr() if resid is not None else None, resid.stride(0) if resid is not None else 0, out.data_ptr(), out.stride(0),
        B, G, Tp, cg, cgp, k, stride, Kp, ACT[act], _stream()))
    check(rc, f"pm_grouped_conv_bf16(B={B}, G={G}, Tp={Tp}, cg={cg}, k={k}, stride={stride})")
    return out


def avgpool_time2(x: Tensor) -> Tensor:
    """pm_avgpool_time2: bf16 (B, T, d) -> (B, T // 2, d), mean of adjacent steps."""
    _cuda(x)
    _need(x.dim() == 3 and x.dtype == torch.bfloat16 and x.is_contiguous(), "avgpool_time2: contiguous bf16 (B, T, d)")
    B, T, d = x.shape
    out = torch.empty((B, T // 2, d), dtype=torch.bfloat16, device=x.device)
    if _empty("avgpool_time2", B, T // 2, d):
        return out
    rc = _launch("avgpool_time2", float(3 * out.numel() * 2), lambda: lib().pm_avgpool_time2(x.data_ptr(), out.data_ptr(), B, T, d, _stream()))
    check(rc, f"pm_avgpool_time2(B={B}, T={T}, d={d})")
    return out


def stft_tables(window: Tensor, n_fft: int) -> tuple[Tensor, Tensor, bool]:
    """Twiddle tables of pm_stft_mel / pm_stft_mel_folded (window folded in), built in float64 on the host.  A symmetric window
    (w[k] == w[n_fft - k]: torch.hann_window and friends) gets the folded layout [ceil(nbins / 32)][(n_fft / 2 + 2) / 2][64] -
    half the contraction; anything else the plain [ceil(nbins / 32)][n_fft / 2][64] (see include/pm_mi355x.h).  The third item
    says which."""
    nbins = n_fft // 2 + 1
    nblk = (nbins + 31) // 32
    no_capture("stft_tables", "builds its tables on the host from the window and uploads them")
    w = window.detach().double().cpu()
    # symmetric up to the rounding of the window's own construction (torch.hann_window: 3e-7 between w[k] and w[N - k] in fp32);
    # the folded form then uses the mean of the two - a relative change of 1.5e-7 per term, two orders below the parity tolerance
    folded = n_fft % 2 == 0 and n_fft >= 4 and float((w[1:] - w[1:].flip(0)).abs().max()) <= 1e-6 * float(w.abs().max())
    if folded:
        w = w.clone()
        w[1:] = 0.5 * (w[1:] + w[1:].flip(0))
    nk = 2 * ((n_fft // 2 + 2) // 2) if folded else n_fft  # table positions k
    k = torch.arange(nk, dtype=torch.float64)
    b = torch.arange(nblk * 32, dtype=torch.float64)
    ang = 2.0 * torch.pi * torch.outer(k, b) / n_fft
    wk = torch.zeros(nk, dtype=torch.float64)
    if folded:
        wk[: n_fft // 2 + 1] = w[: n_fft // 2 + 1]
        wc, ws = wk.clone(), wk.clone()
        wc[n_fft // 2] *= 0.5  # this term meets its own mirror: x[N/2] + x[N/2]
        ws[0] = ws[n_fft // 2] = 0.0
    else:
        wc = ws = w
    valid = (b < nbins)[None, :]
    out = []
    for tab, wt in ((torch.cos(ang), wc), (torch.sin(ang), ws)):
        tab = (tab * wt[:, None] * valid).float()  # (nk, nblk * 32)
        tab = tab.view(nk // 2, 2, nblk, 32).permute(2, 0, 1, 3).contiguous().view(-1)
        out.append(tab.to(window.device))
    return out[0], out[1], folded


def mel_csr(filters: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """CSR form (int32 row pointers, int32 columns, f32 values) of a dense (n_mels, nbins) filterbank."""
    no_capture("mel_csr", "reads the filterbank on the host and uploads its CSR form")
    f = filters.detach().float().cpu()
    nz = f != 0
    ptr = torch.zeros(f.shape[0] + 1, dtype=torch.int32)
    ptr[1:] = nz.sum(1).cumsum(0)
    rows, cols = nz.nonzero(as_tuple=True)
    dev = filters.device
    return ptr.to(dev), cols.to(torch.int32).to(dev), f[rows, cols].contiguous().to(dev)


def stft_mel(x: Tensor, tables, n_fft: int, hop: int, n_frames: int, mode: int, csr=None, n_mels: int = 0) -> Tensor:
    """x (..., T) f32 -> mode 0: (..., n_fft/2+1, n_frames) power; 1: (..., n_mels, n_frames) mel power;
    2: Whisper log-mel (log10, per-clip max - 8 floor, (x + 4) / 4) via pm_stft_mel + pm_logmel_finalize."""
    ptr, col, val = csr if csr is not None else (None, None, None)
    _cuda(x, tables[0], tables[1], ptr, col, val)
    _need(all(t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous() for t in tables[:2]) and tables[0].shape == tables[1].shape,
          "stft_mel: tables must be stft_tables' two contiguous f32 vectors")
    _need(csr is None or (ptr.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32 and ptr.shape == (n_mels + 1,)
                          and col.dim() == 1 and val.shape == col.shape and ptr.is_contiguous() and col.is_contiguous() and val.is_contiguous()),
          "stft_mel: csr must be mel_csr's contiguous (int32 (n_mels + 1), int32 (nnz), f32 (nnz))")
    lead, T = x.shape[:-1], x.shape[-1]
    _need(T > 0, "stft_mel: an empty waveform (T = 0) has no frames")
    x2 = x.reshape(-1, T).float().contiguous()
    B = x2.shape[0]
    rows = n_fft // 2 + 1 if mode == 0 else n_mels
    out = torch.empty((B, rows, max(n_frames, 0)), dtype=torch.float32, device=x.device)
    if _empty("stft_mel", B * n_frames, T, rows, n_fft, hop, tables[0].numel()) or (csr is not None and _empty("stft_mel", 1, col.numel())):
        return out.view(*lead, rows, n_frames)
    peak = torch.empty(max(B, 1), dtype=torch.int32, device=x.device) if mode == 2 else None
    fn = lib().pm_stft_mel_folded if len(tables) > 2 and tables[2] else lib().pm_stft_mel
    rc = _launch("stft_mel", float(x2.numel() * 4 + out.numel() * 4), lambda: fn(
        x2.data_ptr(), T, B, T, tables[0].data_ptr(), tables[1].data_ptr(), n_fft, hop, n_frames, mode,
        ptr.data_ptr() if ptr is not None else None, col.data_ptr() if col is not None else None,
        val.data_ptr() if val is not None else None, n_mels, out.data_ptr(), peak.data_ptr() if peak is not None else None,
        _stream()))
    check(rc, f"pm_stft_mel(B={B}, T={T}, n_fft={n_fft}, hop={hop}, mode={mode})")
    if mode == 2:
        rc = _launch("logmel_finalize", float(out.numel() * 8), lambda: lib().pm_logmel_finalize(
            out.data_ptr(), peak.data_ptr(), B, rows * n_frames, _stream()))
        check(rc, "pm_logmel_finalize")
    return out.view(*lead, rows, n_frames)


def whisper_stem1(x: Tensor, w1: Tensor, b1: Tensor) -> Tensor:
    """x f32 (B, C, T) channel-major -> bf16 (B, T + 2, d) time-major, GELU(conv1d k3 s1 p1), zero rows 0 and T+1."""
    _cuda(x, w1, b1)
    _need(x.dim() == 3 and x.dtype == torch.float32 and x.is_contiguous(), "whisper_stem1: x must be contiguous f32 (B, C, T)")
    B, C, T = x.shape
    d, K = w1.shape
    _need(w1.dtype == torch.bfloat16 and w1.is_contiguous() and K % 3 == 0 and K // 3 >= C, "whisper_stem1: bad packed weight")
    _need(b1.dtype == torch.float32 and b1.numel() == d and b1.is_contiguous(), "whisper_stem1: bias must be contiguous f32 (d)")
    out = torch.empty((B, T + 2, d), dtype=torch.bfloat16, device=x.device)
    if _empty("whisper_stem1", B, C, T, d, K):
        return out
    rc = _launch("whisper_stem1", float(x.numel() * 4 + out.numel() * 2), lambda: lib().pm_whisper_stem1(
        x.data_ptr(), w1.data_ptr(), b1.data_ptr(), out.data_ptr(), B, C, K // 3, T, d, _stream()))
    check(rc, f"pm_whisper_stem1(B={B}, C={C}, T={T}, d={d})")
    return out


EMBED_CHECK_IDS = True  # embed_tokens validates ids against the vocabulary (one read-back per eager call)


def embed_tokens(tokens: Tensor, emb: Tensor, pos: Tensor | None, pos0: int = 0, out_dtype: torch.dtype = torch.bfloat16,
                 out: Tensor | None = None) -> Tensor:
    """tokens int64 (B, L) -> (B, L, d): emb[tokens] + pos[pos0 : pos0 + L] (pos None: no positional term).  ``out`` (bf16 table
    only): a contiguous (B, L, d) tensor to write instead of a new one."""
    _cuda(tokens, emb, pos, out)
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64, "embed_tokens: tokens must be int64 (B, L)")
    tokens = tokens.contiguous()
    B, L = tokens.shape
    V, d = emb.shape
    _need(emb.dtype in (torch.bfloat16, torch.float32) and emb.is_contiguous(), "embed_tokens: emb bf16 or f32 (V, d)")
    empty = _empty("embed_tokens", B * L, V, d)
    # nn.Embedding raises on an id outside [0, V) (whisper.py:48); the kernel clamps so that a bad id cannot fault, so
    # the range is checked here (skipped inside a graph capture, where the caller has validated the example inputs eagerly
    # during the warm-up pass)
    # ONE read-back (min and max were two host synchronisations per teacher-forced forward); EMBED_CHECK_IDS = False
    # skips it for loops that have validated their ids (a generator feeding back its own arg-max ids)
    if EMBED_CHECK_IDS and tokens.numel() and not torch.cuda.is_current_stream_capturing():
        if bool(((tokens < 0) | (tokens >= V)).any()):
            bad = tokens[(tokens < 0) | (tokens >= V)][0].item()
            raise IndexError(f"embed_tokens: token id {bad} outside the vocabulary [0, {V})")
    if pos is not None:
        _need(pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[1] == d and pos.shape[0] >= pos0 + L,
              f"embed_tokens: need {pos0 + L} position rows, have {pos.shape[0]}")
    if emb.dtype == torch.float32:  # fp32 table -> fp32 rows
        _need(out is None, "embed_tokens: out= goes with a bf16 table")
        out = torch.empty((B, L, d), dtype=torch.float32, device=emb.device)
        if empty:
            return out
        rc = lib().pm_embed_tokens_f32(tokens.data_ptr(), emb.data_ptr(), pos.data_ptr() if pos is not None else None, out.data_ptr(),
                                       B, L, pos0, d, V, _stream())
        check(rc, f"pm_embed_tokens_f32(B={B}, L={L}, d={d})")
        return out
    given = out is not None
    if out is None:
        out = torch.empty((B, L, d), dtype=out_dtype, device=emb.device)
    _need(out.shape == (B, L, d) and out.is_contiguous(), "embed_tokens: out must be contiguous (B, L, d)")
    if given:
        _unaliased("embed_tokens", "out", out, ("tokens", "emb", "pos"), (tokens, emb, pos))
    if empty:
        return out
    rc = lib().pm_embed_tokens(tokens.data_ptr(), emb.data_ptr(), pos.data_ptr() if pos is not None else None, out.data_ptr(), _dt(out), B, L, pos0, d, V,
                               _stream())
    check(rc, f"pm_embed_tokens(B={B}, L={L}, d={d})")
    return out


# ---- decode-step kernels as standalone ops (the decoders build their launch lists in decode_plan.py, whose argument builders
# these wrappers share; the wrappers serve tests) ----
def _dec_rows(who: str, x: Tensor, w: Tensor, bias: Tensor | None, resid: Tensor | None, ln: tuple | None) -> tuple[int, int, int]:
    """The operands of the pm_dec_linear family, whose argument builders (decode_plan.linear_args / ksplit_args) pass row strides
    and raw pointers only: f32 x (M, K) and bf16 w (N, K) rows with unit column stride, f32 bias (N), f32 resid (M, N) rows,
    ln = (gamma, beta, eps) with f32 (K) vectors.  Returns (M, N, K)."""
    _need(x.dim() == 2 and w.dim() == 2 and x.dtype == torch.float32 and w.dtype == torch.bfloat16 and x.shape[1] == w.shape[1]
          and x.stride(1) == 1 and w.stride(1) == 1, f"{who}: f32 x (M, K) and bf16 w (N, K) rows with unit column stride")
    M, K = x.shape
    N = w.shape[0]
    _need(bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N), f"{who}: bias must be contiguous f32 (N)")
    _need(resid is None or (resid.dtype == torch.float32 and resid.shape == (M, N) and resid.stride(1) == 1),
          f"{who}: resid must be f32 (M, N) rows with unit column stride")
    if ln is not None:
        _need(all(isinstance(t, Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == K for t in ln[:2]),
              f"{who}: ln must be (gamma, beta, eps) with contiguous f32 (K) vectors")
    _rows(who, M, N, K)
    return M, N, K


def dec_linear(x: Tensor, w: Tensor, bias: Tensor | None = None, *, ln: tuple | None = None, act: str = "none",
               resid: Tensor | None = None) -> Tensor:
    """y = act(LN?(x) @ w.T + bias) + resid for <= 64 rows of f32 x and bf16 w (fp32-exact: bf16x3 split)."""
    _cuda(x, w, bias, resid, *(ln[:2] if ln is not None else ()))
    M, N, K = _dec_rows("dec_linear", x, w, bias, resid, ln)
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    plan.call(lib().pm_dec_linear, plan.linear_args(x, w, out, M, ln=ln, bias=bias, resid=resid, act=ACT[act]), _stream(),
              f"pm_dec_linear(M={M}, N={N}, K={K})")
    return out


def dec_linear_ksplit(x: Tensor, w: Tensor, bias: Tensor | None = None, *, k_split: int, act: str = "none",
                      resid: Tensor | None = None) -> Tensor:
    """dec_linear without LayerNorm, K split over k_split workgroups per 16-feature tile (pm_dec_linear_ksplit)."""
    no_capture("dec_linear_ksplit", "reads its ticket counters back after the launch")
    _cuda(x, w, bias, resid)
    M, N, K = _dec_rows("dec_linear_ksplit", x, w, bias, resid, None)
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    ws, cnt = plan.ksplit_workspace(M, N, k_split, x.device)
    plan.call(lib().pm_dec_linear_ksplit, plan.ksplit_args(x, w, out, M, k_split, ws, cnt, bias=bias, resid=resid, act=ACT[act]),
              _stream(), f"pm_dec_linear_ksplit(M={M}, N={N}, K={K}, k_split={k_split})")
    _need(int(cnt.abs().sum()) == 0, "pm_dec_linear_ksplit left a ticket counter non-zero")
    return out


def dec_argmax(x: Tensor, w: Tensor, ln: tuple) -> tuple[Tensor, Tensor]:
    """Per-row argmax (and max) of LN(x) @ w.T without materialising the logits."""
    _need(isinstance(ln, tuple) and len(ln) == 3, "dec_argmax: ln must be (gamma, beta, eps)")
    _cuda(x, w, *ln[:2])
    M, N, K = _dec_rows("dec_argmax", x, w, None, None, ln)
    tile = lib().pm_dec_argmax_tile(K)
    nt = (N + tile - 1) // tile
    wv = torch.empty(M, nt, dtype=torch.float32, device=x.device)
    wi = torch.empty(M, nt, dtype=torch.int32, device=x.device)
    plan.call(lib().pm_dec_linear, plan.linear_args(x, w, None, M, ln=ln, mode=2, argmax_ws=(wv, wi)), _stream(), "pm_dec_linear(argmax)")
    best = wv.max(1)
    cand = torch.where(wv == best.values[:, None], wi, torch.full_like(wi, 2**31 - 1))
    idx = cand.min(1).values.long()
    # a row without a maximum (LN(x) not finite: every tile reports -inf and no index): index 0, as pm_dec_next_token writes
    return torch.where(idx == 2**31 - 1, torch.zeros_like(idx), idx), best.values


DEC_LINEAR_PLAN_FIELDS = ("kernel", "MT", "FT", "NSTEP", "LN", "waves", "gx", "gy", "gz", "tiles")


def dec_linear_plan(M: int, N: int, K: int, *, ln: bool = False, mode: int = 0, k_split: int = 0) -> dict:
    """pm_dec_linear_plan: the instantiation and grid pm_dec_linear (k_split 0; mode 0 plain, 1 q/k/v, 2 arg-max tiles),
    pm_dec_linear_ksplit (mode 0, k_split >= 2) or pm_dec_linear_kparts (mode 3) launches for these shapes - host only, the launchers
    decide by the same function.  kernel: "linear" (dec_linear_kernel) or "logits" (the persistent dec_logits_kernel).  A shape the
    launcher refuses comes back as {"refused": code}."""
    rep = (ctypes.c_int32 * 10)()
    rc = int(lib().pm_dec_linear_plan(M, N, K, int(bool(ln)), mode, k_split, ctypes.addressof(rep)))
    if rc:
        return {"refused": rc}
    out = dict(zip(DEC_LINEAR_PLAN_FIELDS, (int(v) for v in rep)))
    out["kernel"] = ("linear", "logits")[out["kernel"]]
    return out


def _dec_qkv(who: str, q: Tensor, k: Tensor, v: Tensor) -> tuple[int, int, int]:
    """q contiguous f32 (B, H*64); k, v bf16 (B, H, T, 64) caches of one layout with unit last stride (decode_plan.cache_kv passes
    the three leading strides of k for both).  Returns (B, H, T)."""
    _need(k.dim() == 4 and k.shape[3] == 64 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and v.shape == k.shape
          and v.stride() == k.stride() and k.stride(3) == 1, f"{who}: k / v must be bf16 (B, H, T, 64) caches with one layout and unit last stride")
    B, H, T, _ = k.shape
    _need(q.dtype == torch.float32 and q.shape == (B, H * 64) and q.is_contiguous(), f"{who}: q must be contiguous f32 (B, H*64)")
    _rows(who, B, H, T)
    return B, H, T


def dec_attention(q: Tensor, k: Tensor, v: Tensor, lk: int) -> Tensor:
    """q f32 (B, H*64); k, v bf16 (B, H, T, 64) caches; attends over the first lk keys."""
    _cuda(q, k, v)
    B, H, T = _dec_qkv("dec_attention", q, k, v)
    _need(1 <= lk <= T, "dec_attention: 1 <= lk <= cache length")
    out = torch.empty_like(q)
    plan.call(lib().pm_dec_attention, plan.attention_args(q, plan.cache_kv(k, v), out, B, H, pos=None, lk_add=lk, lk_max=T), _stream())
    return out


def prefill_attention(qkv: Tensor, kc: Tensor, vc: Tensor, n_heads: int, p0: int, out: Tensor | None = None) -> Tensor:
    """pm_prefill_attention_bf16: the chunk of positions p0 .. p0 + C - 1 of every sequence attends, causally on absolute
    positions, over the caches' keys < p0 and its own rows, and appends its k / v to the caches.  qkv bf16 (B * C, 3 * H * 64)
    rows [q | k | v] with unit last stride; kc, vc bf16 (B, H, T, 64) caches (p0 + C <= T <= 4096) -> bf16 (B * C, H * 64)."""
    _cuda(qkv, kc, vc, out)
    _need(kc.dim() == 4 and kc.shape[3] == 64 and kc.shape[1] == n_heads and vc.shape == kc.shape and vc.stride() == kc.stride()
          and kc.stride(3) == 1, "prefill_attention: caches must be (B, H, T, 64) with one layout and unit last stride")
    B, H, T, _ = kc.shape
    _need(qkv.dim() == 2 and qkv.shape[1] == 3 * H * 64 and qkv.stride(1) == 1
          and (qkv.shape[0] % B == 0 and qkv.shape[0] > 0 if B > 0 else qkv.shape[0] == 0),
          "prefill_attention: qkv must be (B * C, 3 * H * 64) rows with unit last stride, C >= 1")
    for t in (qkv, kc, vc):
        _need(t.dtype == torch.bfloat16, "prefill_attention: bf16 operands (fp32 caches keep the token-by-token prompt)")
    C = qkv.shape[0] // B if B else 0
    _need(0 <= p0 and p0 + C <= T <= 4096, f"prefill_attention: positions {p0} .. {p0 + C - 1} do not fit caches of {T} (<= 4096) keys")
    given = out is not None
    if out is None:
        out = torch.empty((B * C, H * 64), dtype=torch.bfloat16, device=qkv.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("prefill_attention: rows of out overlap")
    _need(_apart(kc) and _apart(vc), "prefill_attention: cache rows overlap")
    _need(out.shape == (B * C, H * 64) and out.dtype == torch.bfloat16 and out.stride(1) == 1, "prefill_attention: out must be bf16 (B * C, H * 64)")
    _unaliased("prefill_attention", "kc", kc, ("qkv", "vc"), (qkv, vc))  # the caches are always the caller's
    _unaliased("prefill_attention", "vc", vc, ("qkv",), (qkv,))
    if given:
        _unaliased("prefill_attention", "out", out, ("qkv", "kc", "vc"), (qkv, kc, vc))
    if _empty("prefill_attention", B, H, T):
        return out
    kv = plan.cache_kv(kc, vc)
    rc = _launch("prefill_attention", 2.0 * B * H * C * (2 * p0 + C) * 64, lambda: lib().pm_prefill_attention_bf16(
        *plan.prefill_attention_args(qkv, kv, out, B, H, C, p0, T)[:-1], _stream()))
    check(rc, f"pm_prefill_attention_bf16(B={B}, H={H}, C={C}, p0={p0})")
    return out


# ---- ragged prompt batches (right-aligned sequences, key_start int32 (B,) on the device): eager wrappers for the tests; the
# decoder builds the same launches through decode_plan's ragged_* builders ----
def _key_start(key_start: Tensor, B: int, what: str) -> None:
    _need(key_start.dtype == torch.int32 and key_start.shape == (B,) and key_start.is_contiguous(), f"{what}: key_start must be int32 ({B},)")


def dec_attention_ragged(q: Tensor, k: Tensor, v: Tensor, lk: int, key_start: Tensor) -> Tensor:
    """dec_attention over keys min(key_start[b], lk - 1) .. lk - 1 of row b (pm_dec_attention_ragged)."""
    _cuda(q, k, v, key_start)
    B, H, T = _dec_qkv("dec_attention_ragged", q, k, v)
    _key_start(key_start, B, "dec_attention_ragged")
    _need(1 <= lk <= T, "dec_attention_ragged: 1 <= lk <= cache length")
    out = torch.empty_like(q)
    plan.call(lib().pm_dec_attention_ragged, plan.ragged_attention_args(q, plan.cache_kv(k, v), out, B, H, pos=None, lk_add=lk, lk_max=T,
                                                                       key_start=key_start), _stream())
    return out


def prefill_attention_ragged(qkv: Tensor, kc: Tensor, vc: Tensor, n_heads: int, p0: int, key_start: Tensor,
                             out: Tensor | None = None) -> Tensor:
    """pm_prefill_attention_ragged_bf16: prefill_attention whose query at position p of row b keeps keys min(key_start[b], p) .. p."""
    _cuda(qkv, kc, vc, out, key_start)
    _need(kc.dim() == 4 and kc.shape[3] == 64 and kc.shape[1] == n_heads and vc.shape == kc.shape and vc.stride() == kc.stride()
          and kc.stride(3) == 1, "prefill_attention_ragged: caches must be (B, H, T, 64) with one layout and unit last stride")
    B, H, T, _ = kc.shape
    _need(qkv.dim() == 2 and qkv.shape[1] == 3 * H * 64 and qkv.stride(1) == 1
          and (qkv.shape[0] % B == 0 and qkv.shape[0] > 0 if B > 0 else qkv.shape[0] == 0),
          "prefill_attention_ragged: qkv must be (B * C, 3 * H * 64) rows with unit last stride, C >= 1")
    for t in (qkv, kc, vc):
        _need(t.dtype == torch.bfloat16, "prefill_attention_ragged: bf16 operands")
    _key_start(key_start, B, "prefill_attention_ragged")
    C = qkv.shape[0] // B if B else 0
    _need(0 <= p0 and p0 + C <= T <= 4096, f"prefill_attention_ragged: positions {p0} .. {p0 + C - 1} do not fit caches of {T} (<= 4096) keys")
    given = out is not None
    if out is None:
        out = torch.empty((B * C, H * 64), dtype=torch.bfloat16, device=qkv.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("prefill_attention_ragged: rows of out overlap")
    _need(_apart(kc) and _apart(vc), "prefill_attention_ragged: cache rows overlap")
    _need(out.shape == (B * C, H * 64) and out.dtype == torch.bfloat16 and out.stride(1) == 1, "prefill_attention_ragged: out must be bf16 (B * C, H * 64)")
    _unaliased("prefill_attention_ragged", "kc", kc, ("qkv", "vc", "key_start"), (qkv, vc, key_start))  # the caches are always the caller's
    _unaliased("prefill_attention_ragged", "vc", vc, ("qkv", "key_start"), (qkv, key_start))
    if given:
        _unaliased("prefill_attention_ragged", "out", out, ("qkv", "kc", "vc", "key_start"), (qkv, kc, vc, key_start))
    if _empty("prefill_attention_ragged", B, H, T):
        return out
    kv = plan.cache_kv(kc, vc)
    rc = _launch("prefill_attention_ragged", 2.0 * B * H * C * (2 * p0 + C) * 64, lambda: lib().pm_prefill_attention_ragged_bf16(
        *plan.ragged_prefill_attention_args(qkv, kv, out, B, H, C, p0, T, key_start)[:-1], _stream()))
    check(rc, f"pm_prefill_attention_ragged_bf16(B={B}, H={H}, C={C}, p0={p0})")
    return out


def embed_tokens_ragged(tokens: Tensor, emb: Tensor, pos: Tensor, key_start: Tensor, pos0: int = 0,
                        out_dtype: torch.dtype = torch.bfloat16, out: Tensor | None = None) -> Tensor:
    """tokens int64 (B, L) -> (B, L, d): emb[tokens[b, l]] + pos[max(0, pos0 + l - key_start[b])] (bf16 table)."""
    _cuda(tokens, emb, pos, out, key_start)
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64, "embed_tokens_ragged: tokens must be int64 (B, L)")
    tokens = tokens.contiguous()
    B, L = tokens.shape
    V, d = emb.shape
    _need(emb.dtype == torch.bfloat16 and emb.is_contiguous(), "embed_tokens_ragged: emb bf16 (V, d)")
    empty = _empty("embed_tokens_ragged", B * L, V, d)
    _key_start(key_start, B, "embed_tokens_ragged")
    if EMBED_CHECK_IDS and tokens.numel() and not torch.cuda.is_current_stream_capturing():
        if bool(((tokens < 0) | (tokens >= V)).any()):
            bad = tokens[(tokens < 0) | (tokens >= V)][0].item()
            raise IndexError(f"embed_tokens_ragged: token id {bad} outside the vocabulary [0, {V})")
    _need(pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[1] == d and pos.shape[0] >= pos0 + L,
          f"embed_tokens_ragged: need {pos0 + L} position rows, have {pos.shape[0]}")
    given = out is not None
    if out is None:
        out = torch.empty((B, L, d), dtype=out_dtype, device=emb.device)
    _need(out.shape == (B, L, d) and out.is_contiguous(), "embed_tokens_ragged: out must be contiguous (B, L, d)")
    if given:
        _unaliased("embed_tokens_ragged", "out", out, ("tokens", "emb", "pos", "key_start"), (tokens, emb, pos, key_start))
    if empty:
        return out
    rc = lib().pm_embed_tokens_ragged(tokens.data_ptr(), emb.data_ptr(), pos.data_ptr(), key_start.data_ptr(), out.data_ptr(), _dt(out),
                                      B, L, pos0, d, V, _stream())
    check(rc, f"pm_embed_tokens_ragged(B={B}, L={L}, d={d})")
    return out


def dec_embed_ragged(tok_cur: Tensor, emb: Tensor, pos_tab: Tensor, pos: Tensor, key_start: Tensor) -> Tensor:
    """x (B, d) f32: emb[tok_cur[b]] + pos_tab[max(0, pos - key_start[b])]; pos = the int32 (1,) device position."""
    _cuda(tok_cur, emb, pos_tab, pos, key_start)
    _need(tok_cur.dim() == 1 and tok_cur.is_contiguous() and emb.dim() == 2 and emb.is_contiguous() and pos_tab.dim() == 2
          and pos_tab.is_contiguous() and pos_tab.shape[1] == emb.shape[1] and pos.numel() == 1,
          "dec_embed_ragged: contiguous tok_cur (B,), emb (V, d), pos_tab (rows, d); pos is one device int32")
    B = tok_cur.shape[0]
    _rows("dec_embed_ragged", B, emb.shape[0], emb.shape[1], pos_tab.shape[0])
    _key_start(key_start, B, "dec_embed_ragged")
    _need(emb.dtype == torch.bfloat16 and pos_tab.dtype == torch.float32 and pos.dtype == torch.int32 and tok_cur.dtype == torch.int64,
          "dec_embed_ragged: bf16 table, f32 positions, int32 position, int64 tokens")
    # (a validation that reads *pos back: not under capture, where the position is whatever the replay finds there)
    _need(capturing() or 0 <= int(pos) < pos_tab.shape[0], "dec_embed_ragged: position outside the positional table")
    x = torch.empty(B, emb.shape[1], dtype=torch.float32, device=emb.device)
    plan.call(lib().pm_dec_embed_ragged, plan.ragged_embed_args(tok_cur, emb, pos_tab, pos, key_start, x), _stream())
    return x


def _tail_state(what: str, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor, emb: Tensor, pos_tab: Tensor, ticket: Tensor) -> None:
    B = prompt.shape[0]
    _need(pos.dtype == torch.int32 and ticket.dtype == torch.int32 and pos.numel() == 1 and ticket.numel() == 1, f"{what}: int32 position and ticket")
    _need(prompt.dtype == torch.int64 and prompt.is_contiguous() and tokens.dtype == torch.int64 and tokens.is_contiguous()
          and tokens.shape[0] == B and tokens.shape[1] >= prompt.shape[1] and tok_cur.dtype == torch.int64 and tok_cur.shape == (B,) and tok_cur.is_contiguous(),
          f"{what}: contiguous int64 prompt (B, P), tokens (B, Ttot >= P), tok_cur (B,)")
    _need(emb.dtype == torch.bfloat16 and emb.is_contiguous() and pos_tab.dtype == torch.float32 and pos_tab.is_contiguous()
          and pos_tab.shape[1] == emb.shape[1], f"{what}: bf16 table, f32 positions")
    _rows(what, B, prompt.shape[1], tokens.shape[1], emb.shape[0], emb.shape[1], pos_tab.shape[0])


def _tail_pos(what: str, pos: Tensor, pos_tab: Tensor) -> None:
    """the one check of the tail's state that reads a VALUE (behind the aliasing check: a position that shares memory with another
    operand holds whatever that operand holds).  It reads *pos back: not under capture, where the position is whatever the replay
    finds there."""
    _need(capturing() or 0 <= int(pos) + 1 < pos_tab.shape[0], f"{what}: the positional table must cover position + 1")


def dec_next_token(ws_val: Tensor, ws_idx: Tensor, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor, emb: Tensor,
                   pos_tab: Tensor, ticket: Tensor, *, margins: Tensor | None = None, key_start: Tensor | None = None) -> Tensor:
    """pm_dec_next_token (key_start None) or pm_dec_next_token_ragged on explicit state: picks the token after position *pos from the
    per-tile (max, index) pairs ws_val / ws_idx (B, n_tiles), updates tok_cur, tokens, margins, pos and ticket IN PLACE and returns
    the next step's rows x (B, d) f32."""
    _cuda(ws_val, ws_idx, pos, prompt, tok_cur, tokens, emb, pos_tab, ticket, margins, key_start)
    _tail_state("dec_next_token", pos, prompt, tok_cur, tokens, emb, pos_tab, ticket)
    B, P = prompt.shape
    V, d = emb.shape
    _need(ws_val.dtype == torch.float32 and ws_idx.dtype == torch.int32 and ws_val.shape == ws_idx.shape and ws_val.shape[0] == B
          and ws_val.is_contiguous() and ws_idx.is_contiguous(), "dec_next_token: ws_val f32 / ws_idx int32 (B, n_tiles)")
    _rows("dec_next_token", B, ws_val.shape[1])
    _need(margins is None or (margins.dtype == torch.float32 and margins.shape == tokens.shape and margins.is_contiguous()),
          "dec_next_token: margins f32 like tokens")
    _all_unaliased("dec_next_token", ("pos", "tok_cur", "tokens", "ticket", "margins"), (pos, tok_cur, tokens, ticket, margins),
                   ("ws_val", "ws_idx", "prompt", "emb", "pos_tab", "key_start"), (ws_val, ws_idx, prompt, emb, pos_tab, key_start))
    _tail_pos("dec_next_token", pos, pos_tab)
    x = torch.empty(B, d, dtype=torch.float32, device=emb.device)
    if key_start is None:
        args = (ws_val.data_ptr(), ws_idx.data_ptr(), ws_val.shape[1], pos.data_ptr(), prompt.data_ptr(), P, tok_cur.data_ptr(),
                tokens.data_ptr(), tokens.shape[1], plan.ptr(margins), emb.data_ptr(), pos_tab.data_ptr(), x.data_ptr(), d, V,
                ticket.data_ptr(), B, None)
        plan.call(lib().pm_dec_next_token, args, _stream())
    else:
        _key_start(key_start, B, "dec_next_token")
        plan.call(lib().pm_dec_next_token_ragged, plan.ragged_next_token_args(ws_val, ws_idx, pos, prompt, tok_cur, tokens, margins, emb,
                                                                             pos_tab, key_start, x, ticket), _stream())
    return x


def dec_sample_topk(logits: Tensor, k: int, seed: int, pos: Tensor, prompt: Tensor, tok_cur: Tensor, tokens: Tensor, emb: Tensor,
                    pos_tab: Tensor, ticket: Tensor, *, key_start: Tensor | None = None) -> Tensor:
    """pm_dec_sample_topk (key_start None) or pm_dec_sample_topk_ragged on explicit state, as dec_next_token; logits (B, V) f32."""
    _cuda(logits, pos, prompt, tok_cur, tokens, emb, pos_tab, ticket, key_start)
    _tail_state("dec_sample_topk", pos, prompt, tok_cur, tokens, emb, pos_tab, ticket)
    B, P = prompt.shape
    V, d = emb.shape
    _need(logits.dtype == torch.float32 and logits.shape == (B, V) and logits.stride(1) == 1 and 1 <= k <= min(64, V),
          "dec_sample_topk: logits f32 (B, V), 1 <= k <= 64")
    _all_unaliased("dec_sample_topk", ("pos", "tok_cur", "tokens", "ticket"), (pos, tok_cur, tokens, ticket),
                   ("logits", "prompt", "emb", "pos_tab", "key_start"), (logits, prompt, emb, pos_tab, key_start))
    _tail_pos("dec_sample_topk", pos, pos_tab)
    x = torch.empty(B, d, dtype=torch.float32, device=emb.device)
    if key_start is None:
        args = (logits.data_ptr(), logits.stride(0), V, k, int(seed) & (2**64 - 1), pos.data_ptr(), prompt.data_ptr(), P, tok_cur.data_ptr(),
                tokens.data_ptr(), tokens.shape[1], emb.data_ptr(), pos_tab.data_ptr(), x.data_ptr(), d, ticket.data_ptr(), B, None)
        plan.call(lib().pm_dec_sample_topk, args, _stream())
    else:
        _key_start(key_start, B, "dec_sample_topk")
        plan.call(lib().pm_dec_sample_topk_ragged, plan.ragged_sample_topk_args(logits, k, seed, pos, prompt, tok_cur, tokens, emb, pos_tab,
                                                                               key_start, x, ticket), _stream())
    return x


def dec_whisper_rules(logits: Tensor, tokens: Tensor, pos: Tensor, P: int, *, eot: int, timestamp_begin: int, no_timestamps: int = -1,
                      max_initial_timestamp: int = -1, suppress=(), blank=()) -> Tensor:
    """pm_dec_whisper_rules as a standalone op (the generator puts it into its launch list): filters logits (B, V) f32 IN PLACE for
    the token at index pos + 1 of tokens (B, Ttot) int64; returns logits."""
    if len(suppress) or len(blank):
        no_capture("dec_whisper_rules", "uploads the suppress / blank id lists")
    _cuda(logits, tokens, pos)
    _need(logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and _apart(logits),
          "dec_whisper_rules: logits f32 (B, V) rows that do not overlap")
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.shape[0] == logits.shape[0],
          "dec_whisper_rules: tokens int64 (B, Ttot)")
    _need(pos.dtype == torch.int32 and pos.numel() == 1, "dec_whisper_rules: pos is one device int32")
    _rows("dec_whisper_rules", logits.shape[0], logits.shape[1], tokens.shape[1])
    _unaliased("dec_whisper_rules", "logits", logits, ("tokens", "pos"), (tokens, pos))
    i32 = dict(dtype=torch.int32, device=logits.device)
    sup, blk = torch.tensor(list(suppress), **i32), torch.tensor(list(blank), **i32)
    B, V = logits.shape
    rc = lib().pm_dec_whisper_rules(logits.data_ptr(), logits.stride(0), V, tokens.data_ptr(), tokens.shape[1], pos.data_ptr(), P, eot,
                                    no_timestamps, timestamp_begin, max_initial_timestamp, sup.data_ptr() if sup.numel() else None,
                                    sup.numel(), blk.data_ptr() if blk.numel() else None, blk.numel(), B, _stream())
    check(rc, f"pm_dec_whisper_rules(B={B}, V={V})")
    return logits


def _beam_state(what: str, W: int, **named: Tensor) -> int:
    """the (B, W) state tensors of the beam ops: contiguous, one shape; returns B"""
    shape = None
    for name, (t, dt) in named.items():
        _need(t.dim() == 2 and t.shape[1] == W and t.dtype == dt and t.is_contiguous() and (shape is None or t.shape == shape),
              f"{what}: {name} must be {dt} (B, W) contiguous")
        shape = t.shape
    return shape[0]


def dec_beam_topw(logits: Tensor, scores: Tensor, finished: Tensor, pos: Tensor, P: int, eos: int | None):
    """pm_dec_beam_topw as a standalone op: logits (B * W, V) f32, scores (B, W) f32, finished (B, W) int32 ->
    (cand_score (B * W, W) f32, cand_tok (B * W, W) int32)."""
    _cuda(logits, scores, finished, pos)
    W = scores.shape[-1]
    B = _beam_state("dec_beam_topw", W, scores=(scores, torch.float32), finished=(finished, torch.int32))
    _need(logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[0] == B * W,
          "dec_beam_topw: logits f32 (B * W, V)")
    _need(pos.dtype == torch.int32 and pos.numel() == 1, "dec_beam_topw: pos is one device int32")
    V = logits.shape[1]
    _rows("dec_beam_topw", B, W, V)
    cs = torch.empty(B * W, W, dtype=torch.float32, device=logits.device)
    ct = torch.empty(B * W, W, dtype=torch.int32, device=logits.device)
    rc = lib().pm_dec_beam_topw(logits.data_ptr(), logits.stride(0), V, W, scores.data_ptr(), finished.data_ptr(),
                                -1 if eos is None else eos, pos.data_ptr(), P, cs.data_ptr(), ct.data_ptr(), B * W, _stream())
    check(rc, f"pm_dec_beam_topw(rows={B * W}, V={V}, W={W})")
    return cs, ct


def dec_beam_select(cand_score: Tensor, cand_tok: Tensor, scores: Tensor, finished: Tensor, parents: Tensor, tokens: Tensor,
                    pos: Tensor, prompt: Tensor, tok_cur: Tensor, emb: Tensor, pos_tab: Tensor, x: Tensor, ticket: Tensor,
                    eos: int | None) -> None:
    """pm_dec_beam_select as a standalone op; scores / finished / parents (B, W), tokens (B * W, Ttot) int64, tok_cur (B * W) and
    x (B * W, d) f32 are updated IN PLACE and *pos advances by one."""
    _cuda(cand_score, cand_tok, scores, finished, parents, tokens, pos, prompt, tok_cur, emb, pos_tab, x, ticket)
    W = scores.shape[-1]
    B = _beam_state("dec_beam_select", W, scores=(scores, torch.float32), finished=(finished, torch.int32),
                    parents=(parents, torch.int32))
    R = B * W
    _need(cand_score.shape == (R, W) and cand_score.dtype == torch.float32 and cand_score.is_contiguous()
          and cand_tok.shape == (R, W) and cand_tok.dtype == torch.int32 and cand_tok.is_contiguous(),
          "dec_beam_select: candidates (B * W, W) f32 / int32")
    _need(tokens.dim() == 2 and tokens.shape[0] == R and tokens.dtype == torch.int64 and tokens.is_contiguous()
          and prompt.dim() == 2 and prompt.shape[0] == R and prompt.dtype == torch.int64 and prompt.is_contiguous()
          and tokens.shape[1] >= prompt.shape[1] and tok_cur.shape == (R,) and tok_cur.dtype == torch.int64 and tok_cur.is_contiguous(),
          "dec_beam_select: tokens (B * W, Ttot), prompt (B * W, P), tok_cur (B * W) int64")
    V, d = emb.shape
    _need(emb.dtype == torch.bfloat16 and emb.is_contiguous() and pos_tab.dtype == torch.float32 and pos_tab.is_contiguous()
          and pos_tab.shape[1] == d and pos_tab.shape[0] >= tokens.shape[1] and x.shape == (R, d) and x.dtype == torch.float32
          and x.is_contiguous(), "dec_beam_select: emb bf16 (V, d), pos f32 (>= Ttot, d), x f32 (B * W, d)")
    _need(pos.dtype == torch.int32 and pos.numel() == 1 and ticket.dtype == torch.int32 and ticket.numel() == 1,
          "dec_beam_select: pos and ticket are one device int32 each")
    _rows("dec_beam_select", B, W, V, d, tokens.shape[1], prompt.shape[1])
    _all_unaliased("dec_beam_select", ("scores", "finished", "parents", "tokens", "pos", "tok_cur", "x", "ticket"),
                   (scores, finished, parents, tokens, pos, tok_cur, x, ticket),
                   ("cand_score", "cand_tok", "prompt", "emb", "pos_tab"), (cand_score, cand_tok, prompt, emb, pos_tab))
    rc = lib().pm_dec_beam_select(cand_score.data_ptr(), cand_tok.data_ptr(), W, scores.data_ptr(), finished.data_ptr(),
                                  parents.data_ptr(), -1 if eos is None else eos, tokens.data_ptr(), tokens.shape[1], pos.data_ptr(),
                                  prompt.data_ptr(), prompt.shape[1], tok_cur.data_ptr(), emb.data_ptr(), pos_tab.data_ptr(),
                                  x.data_ptr(), d, V, ticket.data_ptr(), B, _stream())
    check(rc, f"pm_dec_beam_select(B={B}, W={W})")


_CACHE_NAMES = tuple("caches[%d]" % i for i in range(128))  # the operand names of dec_beam_reorder's refusals, built once


def dec_beam_reorder(caches: list[Tensor], parents: Tensor, pos: Tensor) -> None:
    """pm_dec_beam_reorder as a standalone op: every cache (B * W, H, Tmax, 64) (all bf16 or all f32, one geometry) is re-gathered
    IN PLACE, rows 0 .. pos - 1 of row (b, j) from row (b, parents[b, j])."""
    no_capture("dec_beam_reorder", "reads parents and pos on the host, uploads its pointer table and synchronises")
    _cuda(parents, pos, *caches)
    B, W = parents.shape
    _need(parents.dtype == torch.int32 and parents.is_contiguous(), "dec_beam_reorder: parents int32 (B, W)")
    _need(bool(((parents >= 0) & (parents < W)).all()), "dec_beam_reorder: parents outside 0 .. W - 1")
    _need(pos.dtype == torch.int32 and pos.numel() == 1, "dec_beam_reorder: pos is one device int32")
    c0 = caches[0]
    _need(c0.dim() == 4 and c0.shape[0] == B * W and c0.shape[3] == 64 and c0.dtype in (torch.bfloat16, torch.float32),
          "dec_beam_reorder: caches (B * W, H, Tmax, 64) bf16 or f32")
    _rows("dec_beam_reorder", B, W, c0.shape[1], c0.shape[2])
    _need(int(pos.item()) <= c0.shape[2], "dec_beam_reorder: position beyond the caches")
    for c in caches:
        _need(c.shape == c0.shape and c.dtype == c0.dtype and c.is_contiguous() and c.data_ptr() % 16 == 0,
              "dec_beam_reorder: caches of one geometry, contiguous, 16-byte aligned")
    _all_unaliased("dec_beam_reorder", _CACHE_NAMES[:len(caches)] if len(caches) <= len(_CACHE_NAMES) else
                   tuple("caches[%d]" % i for i in range(len(caches))), tuple(caches), ("parents", "pos"), (parents, pos))
    table = torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64, device=c0.device)
    rc = lib().pm_dec_beam_reorder(table.data_ptr(), len(caches), parents.data_ptr(), pos.data_ptr(), B, W, c0.shape[1], c0.shape[2],
                                   int(c0.dtype == torch.float32), _stream())
    check(rc, f"pm_dec_beam_reorder(B={B}, W={W}, caches={len(caches)})")
    torch.cuda.current_stream().synchronize()  # the pointer table must outlive the launch


# ------------------------------------------------------------------------------------------------ ConvNeXt (csrc/convnext.hip)
def _f32vec(t: Tensor, n: int, what: str) -> None:
    _need(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, f"{what} must be f32 ({n})")


def dwconv7_ln(x: Tensor, w: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype: torch.dtype,
               ldy: int | None = None) -> Tensor:
    """pm_dwconv7_ln: x (N, H, W, C) bf16 | f32 contiguous, w f32 (7, 7, C) -> LayerNorm_C(dwconv7x7(x) + bias) as
    (N*H*W, ldy) rows of out_dtype, columns C .. ldy-1 zero (ldy defaults to C rounded up to 64)."""
    _cuda(x, w, bias, gamma, beta)
    _need(x.dim() == 4 and x.is_contiguous(), "dwconv7_ln: x must be contiguous (N, H, W, C)")
    N, H, W, C = x.shape
    _need(w.shape == (7, 7, C) and w.dtype == torch.float32 and w.is_contiguous(), "dwconv7_ln: w must be f32 (7, 7, C)")
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _f32vec(t, C, f"dwconv7_ln: {nm}")
    ldy = ldy if ldy is not None else -(-C // 64) * 64
    out = torch.empty((N * H * W, ldy), dtype=out_dtype, device=x.device)
    if _empty("dwconv7_ln", N, H, W, C):
        return out
    nbytes = float(x.numel() * x.element_size() + out.numel() * out.element_size())
    rc = _launch("dwconv7_ln", (98.0 * x.numel(), nbytes), lambda: lib().pm_dwconv7_ln(
        x.data_ptr(), _dt(x), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), ldy,
        _dt(out), N, H, W, C, _stream()))
    check(rc, f"pm_dwconv7_ln(N={N}, H={H}, W={W}, C={C})")
    return out


def ln_space_to_depth(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype: torch.dtype, ldy: int | None = None) -> Tensor:
    """pm_ln_space_to_depth: x (N, H, W, C) -> (N*H/2*W/2, ldy) rows [LN(x[2i, 2j]), LN(x[2i, 2j+1]), LN(x[2i+1, 2j]),
    LN(x[2i+1, 2j+1]), 0 ...] (ldy defaults to 4C rounded up to 64)."""
    _cuda(x, gamma, beta)
    _need(x.dim() == 4 and x.stride(3) == 1 and x.stride(2) >= x.shape[3] and x.stride(1) == x.shape[2] * x.stride(2)
          and x.stride(0) == x.shape[1] * x.stride(1), "ln_space_to_depth: x must be (N, H, W, C) pixel rows")
    N, H, W, C = x.shape
    _need(H % 2 == 0 and W % 2 == 0, f"ln_space_to_depth: even sides needed, got {H} x {W}")
    _f32vec(gamma, C, "ln_space_to_depth: gamma")
    _f32vec(beta, C, "ln_space_to_depth: beta")
    ldy = ldy if ldy is not None else -(-4 * C // 64) * 64
    out = torch.empty((N * (H // 2) * (W // 2), ldy), dtype=out_dtype, device=x.device)
    if _empty("ln_space_to_depth", N, H, W, C):
        return out
    nbytes = float(x.numel() * x.element_size() + out.numel() * out.element_size())
    rc = _launch("ln_space_to_depth", (0.0, nbytes), lambda: lib().pm_ln_space_to_depth(
        x.data_ptr(), x.stride(2), _dt(x), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), ldy, _dt(out), N, H, W, C,
        _stream()))
    check(rc, f"pm_ln_space_to_depth(N={N}, H={H}, W={W}, C={C})")
    return out


def convnext_stem(imgs: Tensor, wt: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, eps: float,
                  out_dtype: torch.dtype = torch.float32) -> Tensor:
    """pm_convnext_stem: imgs f32 (N, 3, H, W), wt f32 (48, d) -> LayerNorm_d(Conv2d(3, d, 4, 4)(imgs) + bias) as NHWC
    (N, H/4, W/4, d) of out_dtype."""
    _cuda(imgs, wt, bias, gamma, beta)
    _need(imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype == torch.float32 and imgs.is_contiguous(),
          "convnext_stem: imgs must be contiguous f32 (N, 3, H, W)")
    d = wt.shape[1]
    _need(wt.shape == (48, d) and wt.dtype == torch.float32 and wt.is_contiguous(), "convnext_stem: wt must be f32 (48, d)")
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _f32vec(t, d, f"convnext_stem: {nm}")
    N, _, H, W = imgs.shape
    out = torch.empty((N, H // 4, W // 4, d), dtype=out_dtype, device=imgs.device)
    if _empty("convnext_stem", N, H // 4, W // 4, d):
        return out
    flops = 2.0 * 48 * d * out.numel() / d
    nbytes = float(imgs.numel() * 4 + out.numel() * out.element_size())
    rc = _launch("convnext_stem", (flops, nbytes), lambda: lib().pm_convnext_stem(
        imgs.data_ptr(), wt.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), d,
        _dt(out), N, H, W, d, _stream()))
    check(rc, f"pm_convnext_stem(N={N}, H={H}, W={W}, d={d})")
    return out


def mean_ln(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype: torch.dtype) -> Tensor:
    """pm_mean_ln: x (N, HW, C) rows (unit channel stride) -> (N, C) = LayerNorm_C(mean over the HW rows)."""
    _cuda(x, gamma, beta)
    _need(x.dim() == 3 and x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1), "mean_ln: x must be (N, HW, C) rows")
    N, HW, C = x.shape
    _f32vec(gamma, C, "mean_ln: gamma")
    _f32vec(beta, C, "mean_ln: beta")
    out = torch.empty((N, C), dtype=out_dtype, device=x.device)
    if _empty("mean_ln", N, HW, C):
        return out
    rc = _launch("mean_ln", (0.0, float(x.numel() * x.element_size())), lambda: lib().pm_mean_ln(
        x.data_ptr(), x.stride(1), _dt(x), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), _dt(out), N, HW, C,
        _stream()))
    check(rc, f"pm_mean_ln(N={N}, HW={HW}, C={C})")
    return out


# ------------------------------------------------------------------------------------------------ MaxViT (csrc/maxvit.hip)
WINDOW_MODES = dict(block=0, grid=1)


def window_attention(q: Tensor, k: Tensor, v: Tensor, N: int, H: int, W: int, n_heads: int, ws: int, mode: str,
                     bias: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """pm_window_attention_bf16: q / k / v bf16 (N*H*W, >= 32*n_heads) pixel rows sharing one row stride (column slices of the packed
    QKV projection), head h in columns 32h .. 32h+31 -> (N*H*W, 32*n_heads) bf16, softmax(q k^T / sqrt(32) + bias[h]) v over the
    ws x ws windows of ``mode`` 'block' or 'grid'; bias f32 (n_heads, ws*ws, ws*ws) or None."""
    _cuda(q, k, v, bias, out)
    M, D = N * H * W, 32 * n_heads
    for t in (q, k, v):
        _need(t.dim() == 2 and t.dtype == torch.bfloat16 and t.shape[0] == M and t.shape[1] >= D and t.stride(1) == 1,
              f"window_attention: q / k / v must be bf16 ({M}, >= {D}) rows")
    _need(q.stride(0) == k.stride(0) == v.stride(0), "window_attention: q / k / v share one row stride")
    _need(mode in WINDOW_MODES, f"window_attention: mode must be 'block' or 'grid', got {mode!r}")
    L = ws * ws
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.shape == (n_heads, L, L) and bias.is_contiguous(),
              f"window_attention: bias must be contiguous f32 ({n_heads}, {L}, {L})")
    given = out is not None
    if out is None:
        out = torch.empty((M, D), dtype=torch.bfloat16, device=q.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("window_attention: rows of out overlap")
    _need(out.dtype == torch.bfloat16 and out.shape[0] == M and out.shape[1] >= D and out.stride(1) == 1, "window_attention: bad out")
    if given:
        _unaliased("window_attention", "out", out, ("q", "k", "v", "bias"), (q, k, v, bias))
    if _empty("window_attention", N, H, W, n_heads, ws):
        return out
    nbytes = float(M * D * 2 * 4)
    rc = _launch("window_attention", (4.0 * M * L * D, nbytes), lambda: lib().pm_window_attention_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), out.data_ptr(), out.stride(0),
        bias.data_ptr() if bias is not None else None, N, H, W, n_heads, ws, WINDOW_MODES[mode], _stream()))
    check(rc, f"pm_window_attention_bf16(N={N}, H={H}, W={W}, heads={n_heads}, ws={ws}, mode={mode})")
    return out


def dwconv3_bn_act(x: Tensor, w: Tensor, scale: Tensor, shift: Tensor, stride: int, *, gate: Tensor | None = None,
                   out_dtype: torch.dtype | None = None, want_psum: bool = False, write_y: bool = True):
    """pm_dwconv3_bn_act: x (N, H, W, C) bf16 | f32 contiguous, w f32 (3, 3, C) -> gelu_tanh(dwconv3x3(x) * scale + shift) [* gate]
    as (N, Ho, Wo, C) of out_dtype (stride 2: the reference's right / bottom zero pad).  want_psum: also (or, with write_y=False,
    only) the f32 (N, Ho, C) per-row channel sums of the ungated output.  Returns y, psum, or (y, psum)."""
    _cuda(x, w, scale, shift, gate)
    _need(x.dim() == 4 and x.is_contiguous(), "dwconv3_bn_act: x must be contiguous (N, H, W, C)")
    _need(stride in (1, 2), "dwconv3_bn_act: stride 1 or 2")
    N, H, W, C = x.shape
    _need(w.shape == (3, 3, C) and w.dtype == torch.float32 and w.is_contiguous(), "dwconv3_bn_act: w must be f32 (3, 3, C)")
    _f32vec(scale, C, "dwconv3_bn_act: scale")
    _f32vec(shift, C, "dwconv3_bn_act: shift")
    if gate is not None:
        _need(gate.dtype == torch.float32 and gate.shape == (N, C) and gate.is_contiguous(), "dwconv3_bn_act: gate must be f32 (N, C)")
    _need(write_y or want_psum, "dwconv3_bn_act: nothing to compute")
    Ho, Wo = (H, W) if stride == 1 else ((H - 2) // 2 + 1, (W - 2) // 2 + 1)
    y = torch.empty((N, Ho, Wo, C), dtype=out_dtype or x.dtype, device=x.device) if write_y else None
    ps = torch.empty((N, Ho, C), dtype=torch.float32, device=x.device) if want_psum else None
    if _empty("dwconv3_bn_act", N, Ho, Wo, C):
        return (y, ps) if write_y and want_psum else (y if write_y else ps)
    nbytes = float(x.numel() * x.element_size() + (y.numel() * y.element_size() if y is not None else 0))
    rc = _launch("dwconv3_bn_act", (18.0 * N * Ho * Wo * C, nbytes), lambda: lib().pm_dwconv3_bn_act(
        x.data_ptr(), _dt(x), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), gate.data_ptr() if gate is not None else None,
        ps.data_ptr() if ps is not None else None, y.data_ptr() if y is not None else None, _dt(y) if y is not None else PM_F32,
        N, H, W, C, stride, _stream()))
    check(rc, f"pm_dwconv3_bn_act(N={N}, H={H}, W={W}, C={C}, stride={stride})")
    if write_y and want_psum:
        return y, ps
    return y if write_y else ps


def se_gate(psum: Tensor, hw: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """pm_se_gate: psum f32 (N, T, C) partial sums over hw pixels, w1 f32 (R, C), w2 f32 (C, R) -> gate f32 (N, C) =
    sigmoid(w2 @ silu(w1 @ mean + b1) + b2)."""
    _cuda(psum, w1, b1, w2, b2)
    _need(psum.dim() == 3 and psum.dtype == torch.float32 and psum.is_contiguous(), "se_gate: psum must be contiguous f32 (N, T, C)")
    N, T, C = psum.shape
    R = w1.shape[0]
    _need(w1.shape == (R, C) and w2.shape == (C, R) and w1.dtype == w2.dtype == torch.float32 and w1.is_contiguous()
          and w2.is_contiguous(), "se_gate: w1 f32 (R, C), w2 f32 (C, R)")
    _f32vec(b1, R, "se_gate: b1")
    _f32vec(b2, C, "se_gate: b2")
    gate = torch.empty((N, C), dtype=torch.float32, device=psum.device)
    if _empty("se_gate", N, T, C, R, hw):
        return gate
    rc = _launch("se_gate", (4.0 * N * C * R, float(psum.numel() * 4)), lambda: lib().pm_se_gate(
        psum.data_ptr(), T, hw, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gate.data_ptr(), N, C, R, _stream()))
    check(rc, f"pm_se_gate(N={N}, T={T}, C={C}, R={R})")
    return gate


def maxvit_stem(imgs: Tensor, wt: Tensor, shift: Tensor, out_dtype: torch.dtype = torch.float32, ldy: int | None = None) -> Tensor:
    """pm_maxvit_stem: imgs f32 (N, 3, H, W), wt f32 (27, d) (BatchNorm scale folded) -> gelu_tanh(conv3x3/2(imgs) + shift) as
    (N, Ho, Wo, ldy) NHWC rows of out_dtype (columns d .. ldy-1 zero)."""
    _cuda(imgs, wt, shift)
    _need(imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype == torch.float32 and imgs.is_contiguous(),
          "maxvit_stem: imgs must be contiguous f32 (N, 3, H, W)")
    d = wt.shape[1]
    _need(wt.shape == (27, d) and wt.dtype == torch.float32 and wt.is_contiguous(), "maxvit_stem: wt must be f32 (27, d)")
    _f32vec(shift, d, "maxvit_stem: shift")
    N, _, H, W = imgs.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    ldy = ldy or d
    out = torch.empty((N, Ho, Wo, ldy), dtype=out_dtype, device=imgs.device)
    if _empty("maxvit_stem", N, Ho, Wo, d):
        return out
    rc = _launch("maxvit_stem", (54.0 * N * Ho * Wo * d, float(imgs.numel() * 4 + out.numel() * out.element_size())),
                 lambda: lib().pm_maxvit_stem(imgs.data_ptr(), wt.data_ptr(), shift.data_ptr(), out.data_ptr(), ldy, _dt(out), N, H, W,
                                              d, _stream()))
    check(rc, f"pm_maxvit_stem(N={N}, H={H}, W={W}, d={d})")
    return out


def im2col3x3(x: Tensor, out_dtype: torch.dtype | None = None, ldy: int | None = None) -> Tensor:
    """pm_im2col3x3_nhwc: x (N, H, W, C) contiguous -> (N*H*W, ldy) rows of pad-1 3 x 3 patches in (kh, kw, C) order, zero past
    9C (ldy defaults to 9C rounded up to 64)."""
    _cuda(x)
    _need(x.dim() == 4 and x.is_contiguous(), "im2col3x3: x must be contiguous (N, H, W, C)")
    N, H, W, C = x.shape
    ldy = ldy if ldy is not None else -(-9 * C // 64) * 64
    out = torch.empty((N * H * W, ldy), dtype=out_dtype or x.dtype, device=x.device)
    if _empty("im2col3x3", N, H, W, C):
        return out
    rc = _launch("im2col3x3", (0.0, float(x.numel() * x.element_size() + out.numel() * out.element_size())), lambda: lib().pm_im2col3x3_nhwc(
        x.data_ptr(), _dt(x), out.data_ptr(), ldy, _dt(out), N, H, W, C, _stream()))
    check(rc, f"pm_im2col3x3_nhwc(N={N}, H={H}, W={W}, C={C}, ldy={ldy})")
    return out


def avgpool2x2(x: Tensor, out_dtype: torch.dtype | None = None) -> Tensor:
    """pm_avgpool2x2_nhwc: x (N, H, W, C) contiguous -> (N, H/2, W/2, C) 2 x 2 means."""
    _cuda(x)
    _need(x.dim() == 4 and x.is_contiguous(), "avgpool2x2: x must be contiguous (N, H, W, C)")
    N, H, W, C = x.shape
    out = torch.empty((N, H // 2, W // 2, C), dtype=out_dtype or x.dtype, device=x.device)
    if _empty("avgpool2x2", N, H // 2, W // 2, C):
        return out
    rc = _launch("avgpool2x2", (0.0, float(x.numel() * x.element_size() + out.numel() * out.element_size())), lambda: lib().pm_avgpool2x2_nhwc(
        x.data_ptr(), _dt(x), out.data_ptr(), _dt(out), N, H, W, C, _stream()))
    check(rc, f"pm_avgpool2x2_nhwc(N={N}, H={H}, W={W}, C={C})")
    return out


# --------------------------------------------------------------------------------------------------------------- DETR
def conv_bf16(x: Tensor, w: Tensor, bias: Tensor | None, stride: int = 1, relu: bool = False, resid: Tensor | None = None) -> Tensor:
    """pm_conv_bf16: x (N, H, W, Cin) bf16 NHWC, w (Cout, k, k, Cin) bf16 with k = 3 (pad 1) or 1 (pad 0), bias f32 (Cout) ->
    relu?(conv(x, w) + bias [+ resid]) as (N, Ho, Wo, Cout) bf16; the ReLU comes after the residual add.  Cin % 64 == 0."""
    _cuda(x, w, bias, resid)
    _need(x.dim() == 4 and w.dim() == 4 and x.is_contiguous() and w.is_contiguous(), "conv_bf16: contiguous NHWC x and (Cout, k, k, Cin) w")
    _need(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "conv_bf16: bf16 operands")
    N, H, W, Cin = x.shape
    Cout, kh, kw, ci = w.shape
    _need(kh == kw and kh in (1, 3), f"conv_bf16: 3 x 3 or 1 x 1 kernels, got {kh} x {kw}")
    _need(ci == Cin and Cin % 64 == 0, f"conv_bf16: Cin must match the weight and be a multiple of 64 (x {Cin}, w {ci})")
    _need(stride in (1, 2), "conv_bf16: stride 1 or 2")
    _need(bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout), "conv_bf16: bias must be f32 (Cout)")
    pad = 1 if kh == 3 else 0
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kh) // stride + 1
    out = torch.empty((N, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    _need(resid is None or (resid.shape == out.shape and resid.dtype == torch.bfloat16 and resid.is_contiguous()),
          "conv_bf16: resid must be bf16 of the output's shape")
    if _empty("conv_bf16", N, Ho, Wo, Cin, Cout):
        return out
    rc = _launch("conv_bf16", (2.0 * N * Ho * Wo * Cout * kh * kw * Cin, float(2 * (x.numel() + w.numel() + out.numel() * (2 if resid is not None else 1)))),
                 lambda: lib().pm_conv_bf16(x.data_ptr(), N, H, W, Cin, w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                            resid.data_ptr() if resid is not None else None, out.data_ptr(), Cout, kh, stride,
                                            int(relu), _stream()))
    check(rc, f"pm_conv_bf16(N={N}, H={H}, W={W}, Cin={Cin}, Cout={Cout}, k={kh}, stride={stride})")
    return out


def resnet_stem(imgs: Tensor, wt: Tensor, shift: Tensor) -> Tensor:
    """pm_resnet_stem: imgs f32 (N, 3, H, W), wt f32 (147, 64) (BatchNorm scale folded), shift f32 (64) ->
    maxpool3x3/2(relu(conv7x7/2(imgs) + shift)) as bf16 NHWC (N, Hp, Wp, 64)."""
    _cuda(imgs, wt, shift)
    _need(imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype == torch.float32 and imgs.is_contiguous(),
          "resnet_stem: imgs must be contiguous f32 (N, 3, H, W)")
    _need(wt.shape == (147, 64) and wt.dtype == torch.float32 and wt.is_contiguous(), "resnet_stem: wt must be f32 (147, 64)")
    _f32vec(shift, 64, "resnet_stem: shift")
    N, _, H, W = imgs.shape
    _need(H >= 1 and W >= 1, "resnet_stem: empty image")
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    conv_map = torch.empty((N, Hc, Wc, 64), dtype=torch.bfloat16, device=imgs.device)
    out = torch.empty((N, Hp, Wp, 64), dtype=torch.bfloat16, device=imgs.device)
    if _empty("resnet_stem", N, H, W):
        return out
    rc = _launch("resnet_stem", (2.0 * 147 * 64 * N * Hc * Wc, float(imgs.numel() * 4 + 4 * conv_map.numel() + 2 * out.numel())),
                 lambda: lib().pm_resnet_stem(imgs.data_ptr(), wt.data_ptr(), shift.data_ptr(), conv_map.data_ptr(), out.data_ptr(),
                                              N, H, W, _stream()))
    check(rc, f"pm_resnet_stem(N={N}, H={H}, W={W})")
    return out


def attention_hd32(q: Tensor, k: Tensor, v: Tensor, n_heads: int) -> Tensor:
    """pm_attention_hd32_bf16: q (B, Lq, H*32), k / v (B, Lk, H*32) bf16 views with unit last stride (column slices of packed
    projections, stride-0 batch broadcasts) -> softmax(q k^T / sqrt(32)) v as (B, Lq, H*32) bf16, heads merged.  No bias, not
    causal.  (ops.attention's dispatch is unchanged: it sends head dim 32 to the generic kernel.)"""
    _cuda(q, k, v)
    _need(q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "attention_hd32: operands must be (B, L, H*32)")
    B, Lq, D = q.shape
    Lk = k.shape[1]
    _need(D == n_heads * 32, f"attention_hd32: head dim must be 32 (got {D} / {n_heads})")
    _need(k.shape == (B, Lk, D) and v.shape == (B, Lk, D), "attention_hd32: shape mismatch")
    _need(Lk >= 1 and n_heads >= 1, "attention_hd32: empty sequence")
    for t in (q, k, v):
        _need(t.dtype == torch.bfloat16 and t.stride(2) == 1, "attention_hd32: bf16 operands with unit last stride")
    out = torch.empty((B, Lq, D), dtype=torch.bfloat16, device=q.device)
    if _empty("attention_hd32", B * Lq, Lk, D):
        return out
    rc = _launch("attention_hd32", 4.0 * B * n_heads * Lq * Lk * 32, lambda: lib().pm_attention_hd32_bf16(
        q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1),
        out.data_ptr(), out.stride(0), out.stride(1), B, n_heads, Lq, Lk, _stream()))
    check(rc, f"pm_attention_hd32_bf16(B={B}, H={n_heads}, Lq={Lq}, Lk={Lk})")
    return out


# ------------------------------------------------------------------------------------------------ MLP-Mixer (csrc/mixer.hip)
def mixer_token_mix_supported(T: int, Dt: int, C: int) -> bool:
    return bool(lib().pm_mixer_token_mix_supported(T, Dt, C))


MIXER_TOKEN_MIX_PLAN_FIELDS = ("NB", "lds", "region_a", "nk1", "nk2", "nd", "nt", "scratch")


def mixer_token_mix_plan(T: int, Dt: int, C: int) -> dict:
    """pm_mixer_token_mix_plan: the slab width (NB x 32 channels), LDS layout and strip counts pm_mixer_token_mix_bf16 launches
    with for these shapes - host only, the launcher decides by the same functions.  scratch: region_a is the per-wave scratch's
    size (True) or the slab's (False).  A shape the launcher refuses comes back as {"refused": code}."""
    rep = (ctypes.c_int32 * 8)()
    rc = int(lib().pm_mixer_token_mix_plan(T, Dt, C, ctypes.addressof(rep)))
    if rc:
        return {"refused": rc}
    out = dict(zip(MIXER_TOKEN_MIX_PLAN_FIELDS, (int(v) for v in rep)))
    out["scratch"] = bool(out["scratch"])
    return out


def mixer_pack_weight(w: Tensor) -> Tensor:
    """An nn.Linear weight (R, K) -> bf16 [ceil(R/32)][ceil(K/16)][64][8], the fragment-major, zero-padded form
    pm_mixer_token_mix_bf16 reads (include/pm_mi355x.h): lane l of strip s, step k holds w[32 s + (l & 31)][16 k + 8 (l >> 5) + 0..7]."""
    R, K = w.shape
    R32, K16 = -(-R // 32) * 32, -(-K // 16) * 16
    wp = torch.zeros((R32, K16), dtype=torch.bfloat16, device=w.device)
    wp[:R, :K] = w.detach()
    return wp.view(R32 // 32, 32, K16 // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(R32 // 32, K16 // 16, 64, 8)


def mixer_token_mix(x: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor, w1f: Tensor, b1: Tensor, w2f: Tensor, b2: Tensor, *,
                    out: Tensor | None = None, want_row_stats: bool = False):
    """pm_mixer_token_mix_bf16: x bf16 (N, T, C) -> x + token_mixing(LN(x)^T)^T, bf16 (``out`` may be x itself).  stats f32 (N*T, 2)
    [mean, rstd] of x's rows; gamma / beta f32 (C); w1f = mixer_pack_weight(W1 (Dt, T)), w2f = mixer_pack_weight(W2 (T, Dt));
    b1 f32 (Dt); b2 f32 (T).  want_row_stats=True also returns the (N*T, C/64, 2) partial statistics of the output rows
    (ln_stats_finalize reads them)."""
    _cuda(x, stats, gamma, beta, w1f, b1, w2f, b2, out)
    _need(x.dim() == 3 and x.dtype == torch.bfloat16 and x.is_contiguous(), "mixer_token_mix: x must be contiguous bf16 (N, T, C)")
    N, T, C = x.shape
    Dt = b1.numel()
    _need(C % 64 == 0 and C >= 64, f"mixer_token_mix: d_model must be a multiple of 64, got {C}")
    _need(Dt % 32 == 0 and Dt >= 32, f"mixer_token_mix: the token-mixing hidden width must be a multiple of 32, got {Dt}")
    _need(T > 0, "mixer_token_mix: an image without tokens (T = 0)")
    _need(mixer_token_mix_supported(T, Dt, C),
          f"mixer_token_mix: T={T} tokens with hidden width {Dt} do not fit: 64 channels of LN(x) and of the hidden activations, "
          f"64 * 2 * ((T rounded up to 16) + 8 + Dt + 8) bytes, must fit the 160 KiB LDS")
    _need(N <= 65535, "mixer_token_mix: at most 65535 images per call")
    for w, shape, what in ((w1f, (Dt // 32, -(-T // 16), 64, 8), "w1f"), (w2f, (-(-T // 32), Dt // 16, 64, 8), "w2f")):
        _need(w.dtype == torch.bfloat16 and tuple(w.shape) == shape and w.is_contiguous(),
              f"mixer_token_mix: {what} must be mixer_pack_weight's bf16 {shape}, got {tuple(w.shape)}")
    _need(stats.shape == (N * T, 2) and stats.dtype == torch.float32 and stats.is_contiguous(), "mixer_token_mix: stats must be f32 (N*T, 2)")
    _f32vec(gamma, C, "mixer_token_mix: gamma")
    _f32vec(beta, C, "mixer_token_mix: beta")
    _f32vec(b1, Dt, "mixer_token_mix: b1")
    _f32vec(b2, T, "mixer_token_mix: b2")
    given = out is not None
    if out is None:
        out = torch.empty_like(x)
    _need(out.shape == x.shape and out.dtype == torch.bfloat16 and out.is_contiguous(), "mixer_token_mix: out must be like x")
    if given:  # out may be x itself: a workgroup stages its own (image, channel slab) of x in LDS behind a barrier, then every
        # thread reads the residual elements it stores before it stores them (csrc/mixer.hip, phases 0 and 2)
        _unaliased("mixer_token_mix", "out", out, ("x", "stats", "gamma", "beta", "w1f", "b1", "w2f", "b2"),
                   (x, stats, gamma, beta, w1f, b1, w2f, b2), ("x",))
    rows = torch.empty((N * T, C // 64, 2), dtype=torch.float32, device=x.device) if want_row_stats else None
    if _empty("mixer_token_mix", N, T, C, Dt):
        return (out, rows) if want_row_stats else out
    work = (4.0 * N * C * w1f.shape[1] * 16 * Dt, float(4 * x.numel() + 2 * (w1f.numel() + w2f.numel())))
    rc = _launch("mixer_token_mix", work, lambda: lib().pm_mixer_token_mix_bf16(
        x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w1f.data_ptr(), b1.data_ptr(), w2f.data_ptr(),
        b2.data_ptr(), out.data_ptr(), rows.data_ptr() if rows is not None else None, N, T, Dt, C, _stream()))
    check(rc, f"pm_mixer_token_mix_bf16(N={N}, T={T}, Dt={Dt}, C={C})")
    return (out, rows) if want_row_stats else out


def row_stats(x: Tensor, eps: float) -> Tensor:
    """pm_row_stats: x (M, C) bf16 | f32 rows (unit column stride) -> f32 (M, 2) [mean, rsqrt(var + eps)]."""
    _cuda(x)
    _need(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= 1, "row_stats: x must be (M, C) rows")
    M, C = x.shape
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    if _empty("row_stats", M, C):
        return stats
    rc = _launch("row_stats", (0.0, float(x.numel() * x.element_size())), lambda: lib().pm_row_stats(
        x.data_ptr(), x.stride(0) if M > 1 else C, _dt(x), stats.data_ptr(), M, C, float(eps), _stream()))
    check(rc, f"pm_row_stats(M={M}, C={C})")
    return stats


def ln_mean(x: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor, out_dtype: torch.dtype) -> Tensor:
    """pm_ln_mean: x (N, T, C) contiguous, stats (N*T, 2) of its rows -> (N, C) = mean over the tokens of LayerNorm_C(x)."""
    _cuda(x, stats, gamma, beta)
    _need(x.dim() == 3 and x.is_contiguous() and x.shape[1] >= 1, "ln_mean: x must be contiguous (N, T, C)")
    N, T, C = x.shape
    _need(stats.shape == (N * T, 2) and stats.dtype == torch.float32 and stats.is_contiguous(), "ln_mean: stats must be f32 (N*T, 2)")
    _f32vec(gamma, C, "ln_mean: gamma")
    _f32vec(beta, C, "ln_mean: beta")
    _need(N <= 65535, "ln_mean: at most 65535 images per call")
    out = torch.empty((N, C), dtype=out_dtype, device=x.device)
    if _empty("ln_mean", N, T, C):
        return out
    rc = _launch("ln_mean", (0.0, float(x.numel() * x.element_size())), lambda: lib().pm_ln_mean(
        x.data_ptr(), _dt(x), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), _dt(out), N, T, C, _stream()))
    check(rc, f"pm_ln_mean(N={N}, T={T}, C={C})")
    return out


def transpose_add_f32(x: Tensor, resid: Tensor | None = None, ldy: int | None = None) -> Tensor:
    """pm_transpose_add_f32: x f32 (N, R, Cc) contiguous -> x transposed per n (+ resid of that shape), as the first R columns of
    an (N, Cc, ldy) buffer (ldy defaults to R; the columns past R are left unwritten)."""
    _cuda(x, resid)
    _need(x.dim() == 3 and x.dtype == torch.float32 and x.is_contiguous(), "transpose_add_f32: x must be contiguous f32 (N, R, Cc)")
    N, R, Cc = x.shape
    ldy = R if ldy is None else ldy
    _need(R >= 1 and Cc >= 1 and N <= 65535 and ldy >= R, "transpose_add_f32: empty rows, more than 65535 images or ldy < R")
    _need(resid is None or (resid.shape == (N, Cc, R) and resid.dtype == torch.float32 and resid.stride() == (Cc * ldy, ldy, 1)),
          "transpose_add_f32: resid must be f32 (N, Cc, R) with the output's strides")
    out = torch.empty((N, Cc, ldy), dtype=torch.float32, device=x.device)[:, :, :R]
    if _empty("transpose_add_f32", N, R, Cc):
        return out
    rc = _launch("transpose_add_f32", (0.0, float(x.numel() * 4 * (3 if resid is not None else 2))), lambda: lib().pm_transpose_add_f32(
        x.data_ptr(), resid.data_ptr() if resid is not None else None, out.data_ptr(), ldy, N, R, Cc, _stream()))
    check(rc, f"pm_transpose_add_f32(N={N}, R={R}, Cc={Cc})")
    return out


# ---- EnCodec (csrc/encodec.hip): fp32, activations time-major (B, T, C)
def _f32c(t: Tensor, what: str) -> None:
    _need(t.dtype == torch.float32 and t.is_contiguous(), f"{what} must be contiguous f32")


def conv1d_supported(Tin: int, Cin: int, Cout: int, k: int, stride: int, left: int, right: int, zero_pad: bool = False, up: int = 1) -> bool:
    return bool(lib().pm_conv1d_f32_supported(Tin, Cin, Cout, k, stride, left, right, int(zero_pad), up))


def conv1d_f32(x: Tensor, w: Tensor, bias: Tensor | None, *, k: int, stride: int = 1, left: int = 0, right: int = 0, elu: bool = False,
               resid: Tensor | None = None, zero_pad: bool = False, up: int = 1, trim: int = 0, t_out: int | None = None) -> Tensor:
    """pm_conv1d_f32: x f32 (B, Tin, Cin) time-major (clips may be a time slice of a larger buffer: strides (any, Cin, 1)), w f32
    (up * Cout, k * Cin) with column tap * Cin + ci -> (B, Tout, Cout).  ``left`` / ``right`` are mirrored (or zero) frames, ``right``
    including the extra padding; ``elu`` applies ELU to the operand as it is loaded; ``resid`` (B, Tout, Cout) is added in the
    epilogue.  ``up`` / ``trim`` / ``zero_pad``: the transposed-convolution form (include/pm_mi355x.h)."""
    _cuda(x, w, bias, resid)
    _need(x.dim() == 3 and x.dtype == torch.float32, "conv1d_f32: x must be f32 (B, Tin, Cin) time-major")
    B, Tin, Cin = x.shape
    _need((Cin == 1 or x.stride(2) == 1) and (Tin == 1 or x.stride(1) == Cin), "conv1d_f32: x must be f32 (B, Tin, Cin) time-major")  # (a dimension of one has no stride to speak of)
    _f32c(w, "conv1d_f32: w")
    _need(w.dim() == 2 and w.shape[1] == k * Cin and w.shape[0] % up == 0, f"conv1d_f32: w {tuple(w.shape)} is not (up * Cout, {k} * {Cin})")
    Cout = w.shape[0] // up
    empty = _empty("conv1d_f32", B, Tin, Cin, Cout, k, stride)
    _need(conv1d_supported(Tin, Cin, Cout, k, stride, left, right, zero_pad, up),
          f"conv1d_f32: {Tin} frames with padding ({left}, {right}), kernel {k}, stride {stride} are not served (reflect padding must be shorter than the clip)")
    Mr = (Tin + left + right - k) // stride + 1
    Tout = Mr * up - trim if t_out is None else t_out
    _need(1 <= Tout <= Mr * up, "conv1d_f32: bad output length")
    if bias is not None:
        _f32vec(bias, Cout, "conv1d_f32: bias")
    if resid is not None:
        _need(resid.shape == (B, Tout, Cout) and up == 1 and trim == 0, "conv1d_f32: resid must be (B, Tout, Cout)")
        _f32c(resid, "conv1d_f32: resid")
    out = torch.empty((B, Tout, Cout), dtype=torch.float32, device=x.device)
    if empty:
        return out
    rc = _launch("conv1d_f32", 2.0 * B * Mr * w.shape[0] * w.shape[1], lambda: lib().pm_conv1d_f32(
        x.data_ptr(), x.stride(0) if B > 1 else Tin * Cin, w.data_ptr(), bias.data_ptr() if bias is not None else None,
        resid.data_ptr() if resid is not None else None, out.data_ptr(), B, Tin, Cin, Cout, k, stride, left, right, int(zero_pad),
        int(elu), up, trim, Tout, _stream()))
    check(rc, f"pm_conv1d_f32(B={B}, Tin={Tin}, Cin={Cin}, Cout={Cout}, k={k}, stride={stride}, up={up})")
    return out


def lstm_f32(x: Tensor, w_ih: list[Tensor], w_hh: list[Tensor], bias: list[Tensor], residual: bool = False, plain: bool = False) -> Tensor:
    """pm_lstm_f32: x f32 (B, T, H) time-major through len(w_ih) stacked LSTM layers (nn.LSTM's gate order; ``bias`` = bias_ih +
    bias_hh per layer) -> the last layer's h (+ x when ``residual``).  One ctypes call.  Two layers run as a wavefront (one GEMM,
    T + 1 launches); ``plain`` forces a GEMM and T step launches per layer (kept for the comparison in tools/encodec_bench.py)."""
    import ctypes

    _cuda(x, *w_ih, *w_hh, *bias)
    _need(x.dim() == 3, "lstm_f32: x must be (B, T, H)")
    _f32c(x, "lstm_f32: x")
    B, T, H = x.shape
    n = len(w_ih)
    _need(n >= 1 and len(w_hh) == n and len(bias) == n and T >= 1, "lstm_f32: one (w_ih, w_hh, bias) per layer, T >= 1")
    _need(H % 64 == 0 and H >= 64, f"lstm_f32: the hidden size must be a multiple of 64 (got {H})")
    for a, b_, c in zip(w_ih, w_hh, bias):
        _need(a.shape == (4 * H, H) and b_.shape == (4 * H, H) and c.shape == (4 * H,), "lstm_f32: weights must be (4H, H), input size == hidden size")
        for t in (a, b_, c):
            _f32c(t, "lstm_f32: weights")
    out = torch.empty_like(x)
    if _empty("lstm_f32", B, T, H):
        return out
    work = torch.empty((lib().pm_lstm_workspace_floats(B, T, H),), dtype=torch.float32, device=x.device)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    rc = _launch("lstm_f32", 2.0 * B * T * 8 * H * H * n, lambda: lib().pm_lstm_f32(
        x.data_ptr(), arr(w_ih), arr(w_hh), arr(bias), n, work.data_ptr(), out.data_ptr(), int(residual) | (2 if plain else 0), B, T, H, _stream()))
    check(rc, f"pm_lstm_f32(B={B}, T={T}, H={H}, layers={n})")
    return out


def rvq_encode(z: Tensor, codebooks: Tensor, norms: Tensor, n_q: int) -> Tensor:
    """pm_rvq_encode_f32: z f32 (M, 128) rows, codebooks (Q, 1024, 128), norms (Q, 1024) -> int64 codes (n_q, M)."""
    _cuda(z, codebooks, norms)
    _need(z.dim() == 2 and codebooks.dim() == 3 and z.shape[1] == codebooks.shape[2], "rvq_encode: z (M, D), codebooks (Q, N, D)")
    for t in (z, codebooks, norms):
        _f32c(t, "rvq_encode: operands")
    Q, N, D = codebooks.shape
    _need(1 <= n_q <= Q and norms.shape == (Q, N), f"rvq_encode: n_quantizers must be in 1..{Q}")
    M = z.shape[0]
    codes = torch.empty((n_q, M), dtype=torch.int64, device=z.device)
    if _empty("rvq_encode", M, D, N):
        return codes
    rc = _launch("rvq_encode_f32", 2.0 * M * N * D * n_q, lambda: lib().pm_rvq_encode_f32(
        z.data_ptr(), codebooks.data_ptr(), norms.data_ptr(), codes.data_ptr(), M, n_q, D, N, _stream()))
    check(rc, f"pm_rvq_encode_f32(M={M}, n_q={n_q}, dim={D}, codebook={N})")
    return codes


def rvq_decode(codes: Tensor, codebooks: Tensor) -> Tensor:
    """pm_rvq_decode_f32: int64 codes (B, n_q, T) (any strides), codebooks (Q, 1024, 128) -> f32 (B, T, 128) time-major."""
    _cuda(codes, codebooks)
    _need(codes.dim() == 3 and codes.dtype == torch.int64, "rvq_decode: codes must be int64 (B, n_q, T)")
    _f32c(codebooks, "rvq_decode: codebooks")
    B, n_q, T = codes.shape
    Q, N, D = codebooks.shape
    _need(1 <= n_q <= Q, f"rvq_decode: {n_q} code streams for {Q} codebooks")
    out = torch.empty((B, T, D), dtype=torch.float32, device=codes.device)
    if _empty("rvq_decode", B, T, D, N):
        return out
    rc = _launch("rvq_decode_f32", (0.0, float(out.numel() * 4 * (n_q + 1))), lambda: lib().pm_rvq_decode_f32(
        codes.data_ptr(), codes.stride(0), codes.stride(1), codes.stride(2), codebooks.data_ptr(), out.data_ptr(), B, T, n_q, D, N, _stream()))
    check(rc, f"pm_rvq_decode_f32(B={B}, T={T}, n_q={n_q})")
    return out


def groupnorm1_(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, resid: Tensor | None = None) -> Tensor:
    """pm_groupnorm1_f32: GroupNorm(1, C) of x f32 (B, T, C) contiguous IN PLACE (statistics over the whole clip), + resid."""
    _cuda(x, gamma, beta, resid)
    _need(x.dim() == 3, "groupnorm1_: x must be (B, T, C)")
    _f32c(x, "groupnorm1_: x")
    B, T, C = x.shape
    _f32vec(gamma, C, "groupnorm1_: gamma")
    _f32vec(beta, C, "groupnorm1_: beta")
    if resid is not None:
        _need(resid.shape == x.shape, "groupnorm1_: resid must have x's shape")
        _f32c(resid, "groupnorm1_: resid")
    _need(B <= 65535 and T >= 1, "groupnorm1_: at most 65535 clips, at least one frame")
    _unaliased("groupnorm1_", "x", x, ("gamma", "beta", "resid"), (gamma, beta, resid))
    if _empty("groupnorm1_", B, T, C):
        return x
    work = torch.empty((lib().pm_groupnorm1_workspace_doubles(B, T * C),), dtype=torch.float64, device=x.device)
    rc = _launch("groupnorm1_f32", (0.0, float(x.numel() * 12)), lambda: lib().pm_groupnorm1_f32(
        x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), resid.data_ptr() if resid is not None else None, work.data_ptr(), B, T * C, C,
        float(eps), _stream()))
    check(rc, f"pm_groupnorm1_f32(B={B}, T={T}, C={C})")
    return x


def encodec_scale(x: Tensor) -> Tensor:
    """pm_encodec_scale_f32: x f32 (B, C, T) -> (B, 1, 1): sqrt(mean_t(mean_c(x)^2)) + 1e-8."""
    _cuda(x)
    _need(x.dim() == 3, "encodec_scale: x must be (B, C, T)")
    _f32c(x, "encodec_scale: x")
    B, C, T = x.shape
    _need(T >= 1 and C >= 1, "encodec_scale: empty clip")
    out = torch.empty((B, 1, 1), dtype=torch.float32, device=x.device)
    if _empty("encodec_scale", B, C, T):
        return out
    rc = _launch("encodec_scale_f32", (0.0, float(x.numel() * 4)), lambda: lib().pm_encodec_scale_f32(x.data_ptr(), out.data_ptr(), B, C, T, _stream()))
    check(rc, f"pm_encodec_scale_f32(B={B}, C={C}, T={T})")
    return out


def scale_clips(x: Tensor, scale: Tensor, divide: bool) -> Tensor:
    """pm_scale_clips_f32: x f32 (B, ...) contiguous divided (or multiplied) by scale[b]."""
    _cuda(x, scale)
    _f32c(x, "scale_clips: x")
    _f32c(scale, "scale_clips: scale")
    _need(x.dim() >= 2, "scale_clips: x must be (B, ...)")
    B, per_clip = x.shape[0], x.shape[1:].numel()
    _need(scale.numel() == B and B <= 65535, "scale_clips: one scale per clip, at most 65535 clips")
    out = torch.empty_like(x)
    if _empty("scale_clips", B, per_clip):
        return out
    rc = _launch("scale_clips_f32", (0.0, float(x.numel() * 8)), lambda: lib().pm_scale_clips_f32(
        x.data_ptr(), scale.data_ptr(), out.data_ptr(), B, x.numel() // B, int(divide), _stream()))
    check(rc, "pm_scale_clips_f32")
    return out


def cls_attend_supported(L: int, d: int, H: int) -> bool:
    return bool(lib().pm_cls_attend_supported(L, d, H))


def cls_head_gemm(x: Tensor, w: Tensor, bias: Tensor | None = None) -> Tensor:
    """pm_cls_head_gemm: x bf16 (M, G, K) or (M, G*K) rows, w bf16 (G, N, K), bias f32 (G*N) | None -> bf16 (M, G, N):
    y[:, g] = x[:, g] @ w[g].T + bias[g] for every group in one launch."""
    _cuda(x, w, bias)
    G, N, K = w.shape
    _need(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.is_contiguous(), "cls_head_gemm: bf16 x, contiguous bf16 w (G, N, K)")
    M = x.shape[0]
    _need(x.shape[1:] in ((G, K), (G * K,)), "cls_head_gemm: x must be (M, G, K) or (M, G * K) for w (G, N, K)")
    x2 = x.reshape(M, G * K)
    _need(x2.stride(1) == 1, "cls_head_gemm: x rows must be contiguous")
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == G * N, "cls_head_gemm: bias must be f32 (G * N)")
    out = torch.empty((M, G, N), dtype=torch.bfloat16, device=x.device)
    if _empty("cls_head_gemm", M, G, N, K):
        return out
    rc = _launch("cls_head_gemm", (2.0 * M * G * N * K, float(2 * (x2.numel() + w.numel() + out.numel()))), lambda: lib().pm_cls_head_gemm(
        x2.data_ptr(), x2.stride(0), K, w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), G * N, N,
        M, N, K, G, _stream()))
    check(rc, f"pm_cls_head_gemm(M={M}, N={N}, K={K}, G={G})")
    return out


def cls_attend(x: Tensor, stats: Tensor | None, u: Tensor, scale: float, eps: float) -> Tensor:
    """pm_cls_attend: x bf16 (N, L, d) (unit last stride), stats f32 (N*L, 2) [mean, rstd] of its rows | None (computed in the
    kernel with eps), u bf16 (N, H, d) -> ctx bf16 (N, H, d): ctx_h = sum_j softmax_j(scale * rstd_j * (u_h . x_j - mean_j * sum(u_h)))
    * rstd_j * (x_j - mean_j)."""
    _cuda(x, stats, u)
    _need(x.dim() == 3 and u.dim() == 3 and x.dtype == torch.bfloat16 and u.dtype == torch.bfloat16 and x.stride(2) == 1
          and u.is_contiguous() and u.shape[0] == x.shape[0] and u.shape[2] == x.shape[2], "cls_attend: x (N, L, d), u (N, H, d) bf16")
    N, L, d = x.shape
    H = u.shape[1]
    if stats is not None:
        _need(stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape == (N * L, 2), "cls_attend: stats must be f32 (N*L, 2)")
    out = torch.empty((N, H, d), dtype=torch.bfloat16, device=x.device)
    if _empty("cls_attend", N, L, d, H):
        return out
    rc = _launch("cls_attend", (4.0 * N * H * L * d, float(2 * (x.numel() + 2 * u.numel()))), lambda: lib().pm_cls_attend(
        x.data_ptr(), x.stride(1), x.stride(0), stats.data_ptr() if stats is not None else None, u.data_ptr(), out.data_ptr(),
        N, L, d, H, float(scale), float(eps), _stream()))
    check(rc, f"pm_cls_attend(N={N}, L={L}, d={d}, H={H})")
    return out


# ---- sequence scoring (csrc/lm_score.hip) ----
LM_SCORE_CHECK_IDS = True  # lm_score validates the targets against [-1, V) (one read-back per eager call, as embed_tokens does)


def lm_score_ws_bytes(M: int, V: int) -> int:
    return int(lib().pm_lm_score_ws_bytes(M, V))


def lm_score(h: Tensor, w: Tensor, targets: Tensor, *, want_lse: bool = False, want_argmax: bool = False, out: Tensor | None = None,
             lse_out: Tensor | None = None, argmax_out: Tensor | None = None, ws: Tensor | None = None):
    """pm_lm_score_bf16: h bf16 (M, K), w bf16 (V, K) (unit last strides, row strides % 8), targets int64 (M) in [-1, V) ->
    logprob f32 (M): x[m, targets[m]] - log sum_v exp(x[m, v]) for x = h @ w.T in fp32, 0 where the target is -1 ("ignore");
    with want_lse the f32 (M) log-sum-exp, with want_argmax the int32 (M) lowest arg-max index: (logprob[, lse][, argmax]).
    The (M, V) logits are never stored: the only scratch is lm_score_ws_bytes(M, V) bytes (20 per row and 2048 columns).
    ``out`` / ``lse_out`` / ``argmax_out`` / ``ws`` (uint8): caller-owned contiguous buffers instead of new ones."""
    _cuda(h, w, targets, out, lse_out, argmax_out, ws)
    _need(h.dim() == 2 and w.dim() == 2 and h.shape[1] == w.shape[1], f"lm_score: h {tuple(h.shape)} vs w {tuple(w.shape)}")
    _need(h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "lm_score: h and w must be bf16")
    _need(h.stride(1) == 1 and w.stride(1) == 1, "lm_score: h and w must be K-contiguous")
    M, K = h.shape
    V = w.shape[0]
    _need(V >= 1 and K >= 1, "lm_score: empty operand")
    _need(h.stride(0) % 8 == 0 and w.stride(0) % 8 == 0, "lm_score: row strides must be multiples of 8 elements")
    _need(targets.dtype == torch.int64 and targets.shape == (M,), f"lm_score: targets must be int64 ({M},)")
    targets = targets.contiguous()
    if LM_SCORE_CHECK_IDS and not torch.cuda.is_current_stream_capturing():
        bad = (targets < -1) | (targets >= V)
        if bool(bad.any()):
            raise IndexError(f"lm_score: target id {targets[bad][0].item()} outside [-1, {V})")
    dev = h.device
    given_out = out
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=dev)
    _need(out.dtype == torch.float32 and out.shape == (M,) and out.is_contiguous(), "lm_score: out must be contiguous f32 (M,)")
    lse = lse_out if lse_out is not None else (torch.empty(M, dtype=torch.float32, device=dev) if want_lse else None)
    am = argmax_out if argmax_out is not None else (torch.empty(M, dtype=torch.int32, device=dev) if want_argmax else None)
    if lse is not None:
        _need(lse.dtype == torch.float32 and lse.shape == (M,) and lse.is_contiguous(), "lm_score: lse_out must be contiguous f32 (M,)")
    if am is not None:
        _need(am.dtype == torch.int32 and am.shape == (M,) and am.is_contiguous(), "lm_score: argmax_out must be contiguous int32 (M,)")
    res = (out,) + ((lse,) if want_lse or lse_out is not None else ()) + ((am,) if want_argmax or argmax_out is not None else ())
    if _empty("lm_score", M, V, K):
        return res[0] if len(res) == 1 else res
    nws = lm_score_ws_bytes(M, V)
    given_ws = ws
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _need(ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nws, f"lm_score: ws must hold {nws} bytes")
    if given_out is not None or lse_out is not None or argmax_out is not None or given_ws is not None:
        _all_unaliased("lm_score", ("out", "lse_out", "argmax_out", "ws"), (given_out, lse_out, argmax_out, given_ws),
                       ("h", "w", "targets"), (h, w, targets))
    nbytes = float(2 * (h.numel() + w.numel()) + nws + 8 * M + 4 * M)
    rc = _launch("lm_score", (2.0 * M * V * K, nbytes), lambda: lib().pm_lm_score_bf16(
        h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), targets.data_ptr(), out.data_ptr(),
        lse.data_ptr() if lse is not None else None, am.data_ptr() if am is not None else None, ws.data_ptr(), M, V, K, _stream()))
    check(rc, f"pm_lm_score_bf16(M={M}, V={V}, K={K})")
    return res[0] if len(res) == 1 else res


# ---- token timestamps (csrc/align.hip) ----
ALIGN_MAX_ROWS = 448  # token rows one workgroup of pm_align_matrix_bf16 / pm_align_dtw_f32 holds


def align_ws_bytes(B: int, L: int, S: int) -> int:
    return int(lib().pm_align_ws_bytes(B, L, S))


def align_counts(v, n: int, lo: int, hi: int, name: str, device) -> Tensor:
    """Host ints (one int or a sequence of n) in [lo, hi] -> int32 (n) on ``device`` (one upload, before any launch); a device
    int32 (n) tensor passes through unchecked (the kernels clamp what they read)."""
    if isinstance(v, Tensor) and v.is_cuda:
        _need(v.dtype == torch.int32 and v.shape == (n,) and v.is_contiguous(), f"{name} must be a contiguous int32 ({n},) tensor")
        return v
    no_capture(name.split(":")[0], f"uploads {name.split(':')[-1].strip()} from the host")
    vals = [int(v)] * n if isinstance(v, int) else [int(x) for x in (v.tolist() if isinstance(v, Tensor) else v)]
    _need(len(vals) == n and all(lo <= x <= hi for x in vals), f"{name} must hold {n} values in [{lo}, {hi}], got {vals}")
    return torch.tensor(vals, dtype=torch.int32).to(device)


def _align_qk(who: str, q: Tensor, k: Tensor, heads: Tensor, lengths: Tensor, frames: Tensor):
    _cuda(q, k, heads, lengths, frames)
    _need(q.dim() == 3 and k.dim() == 3 and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2],
          f"{who}: q {tuple(q.shape)} vs k {tuple(k.shape)}")
    _need(q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16, f"{who}: q and k must be bf16")
    B, L, inner = q.shape
    S = k.shape[1]
    _need(L >= 1 and S >= 4 and inner >= 64 and inner % 64 == 0, f"{who}: q {tuple(q.shape)}, k {tuple(k.shape)}: head dim 64 only")
    _need(q.stride(2) == 1 and k.stride(2) == 1, f"{who}: q and k must have unit last strides")
    _need(all(s % 8 == 0 for s in (q.stride(0), q.stride(1), k.stride(0), k.stride(1))), f"{who}: strides must be multiples of 8 elements")
    for t, n, name in ((heads, None, "heads"), (lengths, B, "lengths"), (frames, B, "frames")):
        _need(t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and (t.numel() >= 1 if n is None else t.numel() == n),
              f"{who}: {name} must be a contiguous int32 vector" + ("" if n is None else f" of {n}"))
    return B, L, S, inner // 64, heads.numel()


def align_lse(q: Tensor, k: Tensor, heads: Tensor, lengths: Tensor, frames: Tensor, out: Tensor | None = None) -> Tensor:
    """pm_align_lse_bf16: q bf16 (B, L, H * 64), k bf16 (B, S, H * 64) (views with unit last stride; strides % 8), heads int32 (n)
    head indices, lengths / frames int32 (B), all on the device -> lse f32 (B, n, L): log sum_{f < F_b} exp(q_t . k_f / 8) of each
    selected head; rows t >= len_b are not written."""
    B, L, S, H, nh = _align_qk("align_lse", q, k, heads, lengths, frames)
    _cuda(q, out)
    given = out is not None
    if out is None:
        out = torch.empty((B, nh, L), dtype=torch.float32, device=q.device)
    _need(out.dtype == torch.float32 and out.shape == (B, nh, L) and out.is_contiguous(), f"align_lse: out must be contiguous f32 {(B, nh, L)}")
    if given:
        _unaliased("align_lse", "out", out, ("q", "k", "heads", "lengths", "frames"), (q, k, heads, lengths, frames))
    if _empty("align_lse", B, L, S, nh):
        return out
    rc = _launch("align_lse", (2.0 * B * nh * L * S * 64, float(2 * B * nh * (L + S) * 64)), lambda: lib().pm_align_lse_bf16(
        q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0), heads.data_ptr(), lengths.data_ptr(),
        frames.data_ptr(), out.data_ptr(), B, L, S, nh, H, _stream()))
    check(rc, f"pm_align_lse_bf16(B={B}, L={L}, S={S}, heads={nh})")
    return out


def align_matrix(q: Tensor, k: Tensor, heads: Tensor, lengths: Tensor, frames: Tensor, lse: Tensor, m: Tensor, inv_heads: float,
                 first: bool) -> Tensor:
    """pm_align_matrix_bf16: folds the selected heads of one layer (operands as align_lse, lse its result) into m f32 (B, L, S)
    (unit last stride) with weight inv_heads: normalised over the tokens, median-filtered (7) along the frames.  ``first``
    overwrites m and writes the zeros outside len_b / F_b; otherwise the call adds.  L <= 448."""
    B, L, S, H, nh = _align_qk("align_matrix", q, k, heads, lengths, frames)
    _cuda(q, lse, m)
    _need(L <= ALIGN_MAX_ROWS, f"align_matrix: at most {ALIGN_MAX_ROWS} token rows, got {L}")
    _need(lse.dtype == torch.float32 and lse.shape == (B, nh, L) and lse.is_contiguous(), f"align_matrix: lse must be contiguous f32 {(B, nh, L)}")
    _need(m.dtype == torch.float32 and m.shape == (B, L, S) and m.stride(2) == 1 and m.stride(1) >= S and _apart(m),
          f"align_matrix: m must be f32 {(B, L, S)} with a unit last stride and rows that do not overlap")
    _unaliased("align_matrix", "m", m, ("q", "k", "heads", "lengths", "frames", "lse"), (q, k, heads, lengths, frames, lse))
    if _empty("align_matrix", B, L, S, nh):
        return m
    rc = _launch("align_matrix", (2.0 * B * nh * L * S * 64, float(4 * B * L * S)), lambda: lib().pm_align_matrix_bf16(
        q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0), heads.data_ptr(), lengths.data_ptr(),
        frames.data_ptr(), lse.data_ptr(), m.data_ptr(), m.stride(1), m.stride(0), B, L, S, nh, H, float(inv_heads), int(bool(first)),
        _stream()))
    check(rc, f"pm_align_matrix_bf16(B={B}, L={L}, S={S}, heads={nh})")
    return m


def align_dtw(m: Tensor, lengths, frames, skip_first: int = 0, skip_last: int = 0, *, out: Tensor | None = None,
              ws: Tensor | None = None) -> Tensor:
    """pm_align_dtw_f32: m f32 (B, L, S) (unit last stride), lengths / frames host ints (checked: 1 <= len_b <= L,
    4 <= F_b <= S) or device int32 (B) -> start int32 (B, L): the first frame of each token row on the DTW path through
    -m[b, skip_first : len_b - skip_last, : F_b] (fp32 additions and strict comparisons: the path is bit-determined), -1 outside
    the window.  ``out`` / ``ws`` (uint8, align_ws_bytes(B, L, S)): caller-owned buffers.  L <= 448."""
    _need(m.dim() == 3 and m.dtype == torch.float32 and m.stride(2) == 1, "align_dtw: m must be f32 (B, L, S) with a unit last stride")
    B, L, S = m.shape
    _need(1 <= L <= ALIGN_MAX_ROWS and S >= 4, f"align_dtw: m {tuple(m.shape)}: 1 <= L <= {ALIGN_MAX_ROWS}, S >= 4")
    _need(m.stride(1) >= S, "align_dtw: rows of m overlap")
    _need(isinstance(skip_first, int) and isinstance(skip_last, int) and skip_first >= 0 and skip_last >= 0,
          f"align_dtw: skip_first / skip_last must be ints >= 0, got {skip_first!r}, {skip_last!r}")
    lengths = align_counts(lengths, B, 1, L, "align_dtw: lengths", m.device)
    frames = align_counts(frames, B, 4, S, "align_dtw: frames", m.device)
    _cuda(m, lengths, frames, out, ws)
    given_out = out
    if out is None:
        out = torch.empty((B, L), dtype=torch.int32, device=m.device)
    _need(out.dtype == torch.int32 and out.shape == (B, L) and out.is_contiguous(), f"align_dtw: out must be contiguous int32 {(B, L)}")
    if _empty("align_dtw", B, L, S):
        return out
    nws = align_ws_bytes(B, L, S)
    given_ws = ws
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=m.device)
    _need(ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nws and ws.data_ptr() % 8 == 0,
          f"align_dtw: ws must hold {nws} bytes, 8-byte aligned")
    if given_out is not None or given_ws is not None:
        _all_unaliased("align_dtw", ("out", "ws"), (given_out, given_ws), ("m", "lengths", "frames"), (m, lengths, frames))
    rc = _launch("align_dtw", (float(B * L * S), float(4 * B * L * S + nws)), lambda: lib().pm_align_dtw_f32(
        m.data_ptr(), m.stride(1), m.stride(0), lengths.data_ptr(), frames.data_ptr(), out.data_ptr(), ws.data_ptr(), B, L, S,
        skip_first, skip_last, _stream()))
    check(rc, f"pm_align_dtw_f32(B={B}, L={L}, S={S})")
    return out


# ---- variable-length (packed) encoder batches: csrc/varlen.hip and pm_attention_varlen_bf16 ("packed sequences") ----
class SeqLens:
    """The extents of a right-padded batch, built once per forward by ``seq_lens``: ``lengths`` (host ints, B of them),
    ``cu`` (int32 (B + 1) cumulative row offsets on the device, cu[0] = 0), ``total`` = sum(lengths), ``max_len``, ``B``, ``L``."""
    __slots__ = ("lengths", "cu", "total", "max_len", "B", "L")

    def __init__(self, lengths: list[int], cu: Tensor, L: int) -> None:
        self.lengths, self.cu, self.L = lengths, cu, L
        self.B, self.total, self.max_len = len(lengths), sum(lengths), max(lengths, default=0)


def seq_lens(lengths, L: int, device, lo: int = 0) -> SeqLens:
    """lengths: B host ints, or a 1-D integer tensor (read back once), each in [lo, L] -> SeqLens with cu_seqlens on ``device``
    (one upload, in front of every launch).  Validated on the host: the kernels trust cu_seqlens."""
    no_capture("seq_lens", "reads the lengths on the host and uploads cu_seqlens")
    if isinstance(lengths, Tensor):
        _need(lengths.dim() == 1 and not lengths.dtype.is_floating_point and lengths.dtype != torch.bool,
              f"lengths must be a 1-D integer tensor, got {tuple(lengths.shape)} {lengths.dtype}")
        vals = [int(v) for v in lengths.tolist()]
    else:
        vals = list(lengths)
        _need(all(isinstance(v, int) and not isinstance(v, bool) for v in vals), f"lengths must be ints, got {vals}")
    _need(all(lo <= v <= L for v in vals), f"lengths must lie in [{lo}, {L}], got {vals}")
    cu = [0]
    for v in vals:
        cu.append(cu[-1] + v)
    _need(cu[-1] < 2 ** 31, "lengths: more than 2^31 rows")
    return SeqLens(vals, torch.tensor(cu, dtype=torch.int32).to(device), int(L))


def _seq(seq: SeqLens, what: str, *ts: Tensor) -> None:
    _need(isinstance(seq, SeqLens) and seq.cu.dtype == torch.int32 and seq.cu.shape == (seq.B + 1,) and seq.cu.is_contiguous(),
          f"{what}: seq must come from ops.seq_lens")
    _cuda(seq.cu, *ts)


RELBIAS_MAX_RADIUS = 512  # PM_RELBIAS_MAX_RADIUS of include/pm_mi355x.h: the head's table is staged in LDS


def attention_varlen(q: Tensor, k: Tensor, v: Tensor, n_heads: int, seq: SeqLens, causal: bool = False,
                     out: Tensor | None = None, *, rel_lut: Tensor | None = None, radius: int | None = None) -> Tensor:
    """q / k / v bf16 (T_total, H*64) views with unit last stride (column slices of one packed QKV projection), seq from
    seq_lens -> (T_total, H*64) bf16: every sequence attends to itself only (pm_attention_varlen_bf16).  ``out``: a bf16
    (T_total, H*64) tensor with unit last stride to write instead of a new one; rows of no sequence are not written.
    ``rel_lut`` f32 (H, >= 2 * radius + 1) with unit last stride adds bias(h, i, j) = rel_lut[h, clamp(j - i, -radius, radius)
    + radius] to the scores (natural-log units, -inf allowed; i, j positions inside the sequence):
    pm_attention_varlen_relbias_bf16, T5's relative-position bias without a (B, H, L, L) table."""
    _need((rel_lut is None) == (radius is None), "attention_varlen: rel_lut and radius come together")
    if rel_lut is not None:  # checked in front of everything that could launch
        _need(isinstance(rel_lut, Tensor) and rel_lut.dtype == torch.float32 and rel_lut.device == q.device,
              "attention_varlen: rel_lut must be an f32 tensor on the operands' device")
        _need(isinstance(radius, int) and not isinstance(radius, bool) and 0 <= radius <= RELBIAS_MAX_RADIUS,
              f"attention_varlen: radius must be an int in [0, {RELBIAS_MAX_RADIUS}], got {radius!r}")
        _need(rel_lut.dim() == 2 and rel_lut.shape[0] == n_heads and rel_lut.shape[1] >= 2 * radius + 1,
              f"attention_varlen: rel_lut must be ({n_heads}, >= {2 * radius + 1}), got {tuple(rel_lut.shape)}")
        _need(rel_lut.stride(1) == 1 and rel_lut.stride(0) >= 2 * radius + 1, "attention_varlen: rel_lut needs unit last stride and rows that do not overlap")
    _seq(seq, "attention_varlen", q, k, v, out, rel_lut)
    _need(q.dim() == 2 and k.shape == q.shape and v.shape == q.shape, "attention_varlen: operands must be (T_total, H*hd), one shape")
    T, D = q.shape
    _need(T == seq.total, f"attention_varlen: {T} rows for lengths that sum to {seq.total}")
    _need(n_heads >= 1 and D == n_heads * 64, f"attention_varlen: head_dim 64 only (width {D}, {n_heads} heads)")
    for t in (q, k, v):
        _need(t.dtype == torch.bfloat16 and t.stride(1) == 1, "attention_varlen: bf16 operands with unit last stride")
    given = out is not None
    if out is None:
        out = torch.empty((T, D), dtype=torch.bfloat16, device=q.device)
    elif not (out.is_contiguous() or _apart(out)):
        raise ValueError("attention_varlen: rows of out overlap")
    _need(out.shape == (T, D) and out.dtype == torch.bfloat16 and out.stride(1) == 1, "attention_varlen: out must be bf16 (T_total, H*64)")
    if given:
        _unaliased("attention_varlen", "out", out, ("q", "k", "v", "seq.cu", "rel_lut"), (q, k, v, seq.cu, rel_lut))
    if T == 0:
        return out
    work = 4.0 * n_heads * 64 * sum(n * n for n in seq.lengths)
    if rel_lut is not None:
        rc = _launch("attention_varlen_relbias", work, lambda: lib().pm_attention_varlen_relbias_bf16(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), out.data_ptr(), out.stride(0),
            seq.cu.data_ptr(), seq.B, n_heads, seq.max_len, int(causal), rel_lut.data_ptr(), rel_lut.stride(0), radius, _stream()))
        check(rc, f"pm_attention_varlen_relbias_bf16(B={seq.B}, H={n_heads}, T={T}, max_len={seq.max_len}, radius={radius})")
        return out
    rc = _launch("attention_varlen", work, lambda: lib().pm_attention_varlen_bf16(
        q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), out.data_ptr(), out.stride(0),
        seq.cu.data_ptr(), seq.B, n_heads, seq.max_len, int(causal), _stream()))
    check(rc, f"pm_attention_varlen_bf16(B={seq.B}, H={n_heads}, T={T}, max_len={seq.max_len})")
    return out


def embed_tokens_varlen(tokens: Tensor, emb: Tensor, pos: Tensor | None, seq: SeqLens, out_dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """tokens int64 (B, L) right-padded -> packed (T_total, d): row cu[b] + t = emb[tokens[b, t]] + pos[t] for t < len_b.  A bf16
    table makes ``out_dtype`` rows, an fp32 table fp32 rows, like embed_tokens.  Ids are range-checked at valid positions only."""
    _seq(seq, "embed_tokens_varlen", tokens, emb, pos)
    _need(tokens.dim() == 2 and tokens.dtype == torch.int64, "embed_tokens_varlen: tokens must be int64 (B, L)")
    tokens = tokens.contiguous()
    B, L = tokens.shape
    V, d = emb.shape
    _need(B == seq.B and L == seq.L, f"embed_tokens_varlen: tokens {(B, L)} against lengths for {(seq.B, seq.L)}")
    _need(emb.dtype in (torch.bfloat16, torch.float32) and emb.is_contiguous(), "embed_tokens_varlen: emb bf16 or f32 (V, d)")
    empty = _empty("embed_tokens_varlen", seq.total, V, d)
    if EMBED_CHECK_IDS and seq.total and not torch.cuda.is_current_stream_capturing():
        valid = torch.arange(L, device=tokens.device)[None, :] < (seq.cu[1:] - seq.cu[:-1])[:, None]
        bad = valid & ((tokens < 0) | (tokens >= V))
        if bool(bad.any()):
            raise IndexError(f"embed_tokens_varlen: token id {tokens[bad][0].item()} outside the vocabulary [0, {V})")
    if pos is not None:
        _need(pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[1] == d and pos.shape[0] >= seq.max_len,
              f"embed_tokens_varlen: need {seq.max_len} position rows, have {pos.shape[0]}")
    if emb.dtype == torch.float32:
        out_dtype = torch.float32
    out = torch.empty((seq.total, d), dtype=out_dtype, device=emb.device)
    if empty:
        return out
    rc = lib().pm_embed_tokens_varlen(tokens.data_ptr(), emb.data_ptr(), _dt(emb), pos.data_ptr() if pos is not None else None,
                                      seq.cu.data_ptr(), out.data_ptr(), _dt(out), B, L, d, V, _stream())
    check(rc, f"pm_embed_tokens_varlen(B={B}, L={L}, d={d}, T={seq.total})")
    return out


def _padded(x: Tensor, seq: SeqLens, what: str) -> tuple[int, int, int]:
    _need(x.dim() == 3 and x.dtype in (torch.bfloat16, torch.float32) and x.stride(2) == 1, f"{what}: (B, L, d) bf16 or f32 with unit last stride")
    B, L, d = x.shape
    _need(B == seq.B and L == seq.L, f"{what}: {(B, L)} rows against lengths for {(seq.B, seq.L)}")
    eb = x.element_size()
    _need((d * eb) % 16 == 0 and (x.stride(0) * eb) % 16 == 0 and (x.stride(1) * eb) % 16 == 0 and x.stride(1) >= d,
          f"{what}: rows and strides must be multiples of 16 bytes")
    return B, L, d


def rows_pack(x: Tensor, seq: SeqLens) -> Tensor:
    """padded (B, L, d) -> packed (T_total, d): row cu[b] + t = x[b, t] for t < len_b (pm_rows_pack; padded rows are not read)."""
    _seq(seq, "rows_pack", x)
    B, L, d = _padded(x, seq, "rows_pack")
    out = torch.empty((seq.total, d), dtype=x.dtype, device=x.device)
    if _empty("rows_pack", seq.total, d):
        return out
    rc = _launch("rows_pack", (0.0, 2.0 * seq.total * d * x.element_size()), lambda: lib().pm_rows_pack(
        x.data_ptr(), x.stride(0), x.stride(1), seq.cu.data_ptr(), out.data_ptr(), out.stride(0), B, L, d, x.element_size(), _stream()))
    check(rc, f"pm_rows_pack(B={B}, L={L}, d={d})")
    return out


def rows_unpack(x: Tensor, seq: SeqLens) -> Tensor:
    """packed (T_total, d) -> padded (B, L, d) contiguous, rows t >= len_b zero (pm_rows_unpack)."""
    _seq(seq, "rows_unpack", x)
    _need(x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float32) and x.stride(1) == 1 and x.shape[0] == seq.total,
          f"rows_unpack: packed ({seq.total}, d) bf16 or f32 with unit last stride")
    d, eb = x.shape[1], x.element_size()
    _need((d * eb) % 16 == 0 and (x.stride(0) * eb) % 16 == 0 and x.stride(0) >= d, "rows_unpack: rows and strides must be multiples of 16 bytes")
    out = torch.empty((seq.B, seq.L, d), dtype=x.dtype, device=x.device)
    if _empty("rows_unpack", seq.total, d):  # no packed row at all: every padded row is a tail row
        return out.zero_()
    rc = _launch("rows_unpack", (0.0, float(seq.total + seq.B * seq.L) * d * eb), lambda: lib().pm_rows_unpack(
        x.data_ptr(), x.stride(0), seq.cu.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), seq.B, seq.L, d, eb, _stream()))
    check(rc, f"pm_rows_unpack(B={seq.B}, L={seq.L}, d={d})")
    return out


def rows_zero_tail(x: Tensor, seq: SeqLens) -> Tensor:
    """Zeroes rows t >= len_b of a padded (B, L, d) tensor IN PLACE and returns it (pm_rows_zero_tail)."""
    _seq(seq, "rows_zero_tail", x)
    B, L, d = _padded(x, seq, "rows_zero_tail")
    _need(_apart(x), "rows_zero_tail: rows of x overlap")
    _unaliased("rows_zero_tail", "x", x, ("seq.cu",), (seq.cu,))
    if _empty("rows_zero_tail", B * L, d):
        return x
    rc = _launch("rows_zero_tail", (0.0, float(B * L - seq.total) * d * x.element_size()), lambda: lib().pm_rows_zero_tail(
        x.data_ptr(), x.stride(0), x.stride(1), seq.cu.data_ptr(), B, L, d, x.element_size(), _stream()))
    check(rc, f"pm_rows_zero_tail(B={B}, L={L}, d={d})")
    return x


def segment_mean(x: Tensor, seq: SeqLens) -> Tensor:
    """packed (T_total, d) bf16 or f32 -> f32 (B, d): the mean of each sequence's rows, fp32 sums in row order (pm_segment_mean)."""
    _seq(seq, "segment_mean", x)
    _need(x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float32) and x.stride(1) == 1 and x.shape[0] == seq.total,
          f"segment_mean: packed ({seq.total}, d) bf16 or f32 with unit last stride")
    d, eb = x.shape[1], x.element_size()
    _need((d * eb) % 16 == 0 and (x.stride(0) * eb) % 16 == 0 and x.stride(0) >= d and seq.B <= 65535,
          "segment_mean: rows and strides must be multiples of 16 bytes, at most 65535 sequences")
    out = torch.empty((seq.B, d), dtype=torch.float32, device=x.device)
    if _empty("segment_mean", seq.total, d):  # no packed row at all: the mean of a sequence without rows is 0, as the kernel writes it
        return out.zero_()
    rc = _launch("segment_mean", (float(seq.total * d), float(seq.total * d * eb)), lambda: lib().pm_segment_mean(
        x.data_ptr(), x.stride(0), _dt(x), seq.cu.data_ptr(), out.data_ptr(), seq.B, d, _stream()))
    check(rc, f"pm_segment_mean(B={seq.B}, d={d}, T={seq.total})")
    return out


# ---- CTC heads of the wav2vec2 family (csrc/ctc.hip; DESIGN.md, "CTC heads") ----
CTC_MAX_VOCAB = 256    # columns one workgroup of pm_ctc_head_bf16 owns
CTC_MAX_TARGET = 511   # labels per clip: 2 U + 1 <= 1023 states, four per thread of the recursion kernels


def ctc_ws_bytes(B: int, Tmax: int, Umax: int) -> int:
    return int(lib().pm_ctc_ws_bytes(B, Tmax, Umax))


def ctc_head(h: Tensor, w: Tensor, bias: Tensor | None = None, *, want_best_logp: bool = True, out: Tensor | None = None,
             best_out: Tensor | None = None, best_logp_out: Tensor | None = None):
    """pm_ctc_head_bf16: h bf16 (M, K), w bf16 (V, K) (unit last strides, row strides % 8), bias f32 (V) or None ->
    (logp f32 (M, V), best int32 (M), best_logp f32 (M) | None): logp = log_softmax(h @ w.T + bias) with fp32 accumulation, best the
    LOWEST arg-max index of the logits, best_logp = logp[m, best[m]].  2 <= V <= 256, K % 8 == 0.  ``out``: an f32 (M, V) tensor
    with a unit last stride (its padding columns are not written); ``best_out`` / ``best_logp_out``: contiguous (M,) buffers."""
    _cuda(h, w, bias, out, best_out, best_logp_out)
    _need(h.dim() == 2 and w.dim() == 2 and h.shape[1] == w.shape[1], f"ctc_head: h {tuple(h.shape)} vs w {tuple(w.shape)}")
    _need(h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "ctc_head: h and w must be bf16")
    _need(h.stride(1) == 1 and w.stride(1) == 1, "ctc_head: h and w must be K-contiguous")
    M, K = h.shape
    V = w.shape[0]
    _need(K >= 8 and K % 8 == 0, f"ctc_head: K a multiple of 8, got M={M}, K={K}")
    _need(2 <= V <= CTC_MAX_VOCAB, f"ctc_head: 2 <= V <= {CTC_MAX_VOCAB}, got {V}")
    _need(h.stride(0) % 8 == 0 and w.stride(0) % 8 == 0 and h.stride(0) >= K and w.stride(0) >= K,
          "ctc_head: row strides must be multiples of 8 elements")
    _need(h.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0, "ctc_head: h and w must be 16-byte aligned")
    if bias is not None:
        _need(bias.dtype == torch.float32 and bias.shape == (V,) and bias.is_contiguous(), f"ctc_head: bias must be contiguous f32 ({V},)")
    dev = h.device
    given_out = out
    if out is None:
        out = torch.empty((M, V), dtype=torch.float32, device=dev)
    _need(out.dtype == torch.float32 and out.shape == (M, V) and out.stride(1) == 1 and (out.stride(0) >= V or M == 1),
          f"ctc_head: out must be f32 {(M, V)} with a unit last stride")
    best = best_out if best_out is not None else torch.empty(M, dtype=torch.int32, device=dev)
    _need(best.dtype == torch.int32 and best.shape == (M,) and best.is_contiguous(), "ctc_head: best_out must be contiguous int32 (M,)")
    blp = best_logp_out if best_logp_out is not None else (torch.empty(M, dtype=torch.float32, device=dev) if want_best_logp else None)
    if blp is not None:
        _need(blp.dtype == torch.float32 and blp.shape == (M,) and blp.is_contiguous(), "ctc_head: best_logp_out must be contiguous f32 (M,)")
    if given_out is not None or best_out is not None or best_logp_out is not None:
        _all_unaliased("ctc_head", ("out", "best_out", "best_logp_out"), (given_out, best_out, best_logp_out), ("h", "w", "bias"), (h, w, bias))
    if _empty("ctc_head", M, V, K):
        return out, best, blp
    ldl = max(out.stride(0), V)
    nbytes = float(2 * (h.numel() + w.numel()) + 4 * M * V + 8 * M)
    rc = _launch("ctc_head", (2.0 * M * V * K, nbytes), lambda: lib().pm_ctc_head_bf16(
        h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr() if bias is not None else None, out.data_ptr(), ldl,
        best.data_ptr(), blp.data_ptr() if blp is not None else None, M, V, K, _stream()))
    check(rc, f"pm_ctc_head_bf16(M={M}, V={V}, K={K})")
    return out, best, blp


def _ctc_frames(who: str, seq: SeqLens, rows: int, *ts: Tensor) -> None:
    _seq(seq, who, *ts)
    _need(rows == seq.total, f"{who}: {rows} packed frames for lengths that sum to {seq.total}")


def ctc_greedy(best: Tensor, seq: SeqLens, best_logp: Tensor | None = None, blank: int = 0):
    """pm_ctc_greedy: best int32 (T_total) packed arg-max ids, seq from seq_lens (frames per clip, L = the padded frame count),
    best_logp f32 (T_total) or None -> (ids int32 (B, L), n int32 (B), start int32 (B, L), path_logp f32 (B) | None): per clip the
    arg-max sequence with repeats merged and ``blank`` removed (then -1), the count, the first frame of each emitted id (then -1)
    and the sum of best_logp over the clip's frames.  A clip of 0 frames gives n = 0."""
    _ctc_frames("ctc_greedy", seq, best.shape[0] if best.dim() == 1 else -1, best, best_logp)
    _need(best.dtype == torch.int32 and best.is_contiguous(), "ctc_greedy: best must be contiguous int32 (T_total,)")
    _need(isinstance(blank, int) and not isinstance(blank, bool) and -2 ** 31 < blank < 2 ** 31, f"ctc_greedy: blank must be an int, got {blank!r}")
    if best_logp is not None:
        _need(best_logp.dtype == torch.float32 and best_logp.shape == best.shape and best_logp.is_contiguous(),
              "ctc_greedy: best_logp must be contiguous f32 (T_total,)")
    B, L, dev = seq.B, seq.L, seq.cu.device
    ids = torch.empty((B, L), dtype=torch.int32, device=dev)
    start = torch.empty((B, L), dtype=torch.int32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    path = torch.empty(B, dtype=torch.float32, device=dev) if best_logp is not None else None
    T = seq.total
    if B == 0 or L == 0 or T == 0:  # every clip is empty: nothing to launch on
        ids.fill_(-1)
        start.fill_(-1)
        n.zero_()
        if path is not None:
            path.zero_()
        return ids, n, start, path
    rc = _launch("ctc_greedy", (float(T), float(8 * T + 8 * B * L)), lambda: lib().pm_ctc_greedy(
        best.data_ptr(), seq.cu.data_ptr(), best_logp.data_ptr() if best_logp is not None else None, ids.data_ptr(), n.data_ptr(),
        start.data_ptr(), path.data_ptr() if path is not None else None, T, B, L, blank, _stream()))
    check(rc, f"pm_ctc_greedy(B={B}, T={T}, L={L})")
    return ids, n, start, path


def _ctc_rec(who: str, logp: Tensor, seq: SeqLens, targets: Tensor, target_lengths, blank: int):
    if not (isinstance(target_lengths, Tensor) and target_lengths.is_cuda):
        no_capture(who, "uploads target_lengths from the host")
    _need(logp.dim() == 2 and logp.dtype == torch.float32 and logp.stride(1) == 1, f"{who}: logp must be f32 (T_total, V) with a unit last stride")
    _need(isinstance(targets, Tensor) and targets.dim() == 2 and targets.dtype == torch.int32 and (targets.shape[1] == 0 or targets.stride(1) == 1),
          f"{who}: targets must be int32 (B, Umax) with a unit last stride")
    _ctc_frames(who, seq, logp.shape[0], logp, targets)
    T, V = logp.shape
    B, Umax = targets.shape
    _need(B == seq.B, f"{who}: {B} target rows for {seq.B} clips")
    _need(V >= 1 and (logp.stride(0) >= V or T <= 1), f"{who}: rows of logp overlap")
    _need(Umax <= CTC_MAX_TARGET, f"{who}: at most {CTC_MAX_TARGET} labels per clip, got {Umax}")
    _need(Umax == 0 or B == 1 or targets.stride(0) >= Umax, f"{who}: rows of targets overlap")
    _need(isinstance(blank, int) and not isinstance(blank, bool) and 0 <= blank < V, f"{who}: blank must be an int in [0, {V}), got {blank!r}")
    _need(all(n >= 1 for n in seq.lengths), f"{who}: every clip needs at least one frame, got {seq.lengths}")
    tl = align_counts(target_lengths, B, 0, Umax, f"{who}: target_lengths", logp.device)
    _cuda(logp, tl)
    return T, V, B, Umax, tl


def ctc_forward(logp: Tensor, seq: SeqLens, targets: Tensor, target_lengths, blank: int = 0, out: Tensor | None = None) -> Tensor:
    """pm_ctc_forward_f32: logp f32 (T_total, V) packed frames (ctc_head's output or any f32 matrix, -inf allowed), seq from seq_lens
    (every clip >= 1 frame), targets int32 (B, Umax <= 511) right-padded on the device, target_lengths host ints (checked:
    0 <= U_b <= Umax) or a device int32 (B) -> loglik f32 (B) = log p(target_b | clip_b) by the alpha recursion in log space;
    exactly -inf for a pair with too few frames.  Target ids are NOT validated here (the kernel clamps them)."""
    T, V, B, Umax, tl = _ctc_rec("ctc_forward", logp, seq, targets, target_lengths, blank)
    given = out is not None
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=logp.device)
    _cuda(out)
    _need(out.dtype == torch.float32 and out.shape == (B,) and out.is_contiguous(), f"ctc_forward: out must be contiguous f32 ({B},)")
    if given:
        _unaliased("ctc_forward", "out", out, ("logp", "seq.cu", "targets", "target_lengths"), (logp, seq.cu, targets, tl))
    if _empty("ctc_forward", B, V):
        return out
    rc = _launch("ctc_forward", (float(T * (2 * Umax + 1)), float(4 * T * (Umax + 1))), lambda: lib().pm_ctc_forward_f32(
        logp.data_ptr(), max(logp.stride(0), V), seq.cu.data_ptr(), targets.data_ptr() if Umax else None, max(targets.stride(0), Umax),
        tl.data_ptr(), out.data_ptr(), T, B, Umax, V, blank, _stream()))
    check(rc, f"pm_ctc_forward_f32(B={B}, T={T}, Umax={Umax}, V={V})")
    return out


def ctc_viterbi(logp: Tensor, seq: SeqLens, targets: Tensor, target_lengths, blank: int = 0, ws: Tensor | None = None):
    """pm_ctc_viterbi_f32: operands as ctc_forward -> (start int32 (B, Umax), stop int32 (B, Umax), score f32 (B)): the first frame
    and one past the last frame of each target token on the best path (-1 at u >= U_b) and the path's score; fp32 max and add
    only, a fixed tie rule: the path is bit-determined by logp.  An infeasible pair gives -1 everywhere and -inf.
    ``ws`` (uint8, ctc_ws_bytes(B, seq.max_len, Umax), 16-byte aligned): a caller-owned workspace."""
    T, V, B, Umax, tl = _ctc_rec("ctc_viterbi", logp, seq, targets, target_lengths, blank)
    dev = logp.device
    start = torch.empty((B, Umax), dtype=torch.int32, device=dev)
    stop = torch.empty((B, Umax), dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    Tmax = seq.max_len
    if _empty("ctc_viterbi", B, V):
        return start, stop, score
    nws = ctc_ws_bytes(B, Tmax, Umax)
    given = ws is not None
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _cuda(ws)
    _need(ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nws and ws.data_ptr() % 16 == 0,
          f"ctc_viterbi: ws must hold {nws} bytes, 16-byte aligned")
    if given:
        _unaliased("ctc_viterbi", "ws", ws, ("logp", "seq.cu", "targets", "target_lengths"), (logp, seq.cu, targets, tl))
    rc = _launch("ctc_viterbi", (float(T * (2 * Umax + 1)), float(4 * T * (Umax + 1) + nws)), lambda: lib().pm_ctc_viterbi_f32(
        logp.data_ptr(), max(logp.stride(0), V), seq.cu.data_ptr(), targets.data_ptr() if Umax else None, max(targets.stride(0), Umax),
        tl.data_ptr(), start.data_ptr() if Umax else None, stop.data_ptr() if Umax else None, score.data_ptr(), ws.data_ptr(),
        T, B, Tmax, Umax, V, blank, _stream()))
    check(rc, f"pm_ctc_viterbi_f32(B={B}, T={T}, Tmax={Tmax}, Umax={Umax}, V={V})")
    return start, stop, score
