"""Replay a module's forward as ONE HIP graph.

Every operator of this package is a kernel launch on the current stream with no host synchronisation, so a forward at fixed
input shapes can be captured once and replayed: the ~150 launches of an encoder forward then cost one graph launch of host
time instead of ~150 ctypes calls.  That matters where the GPU work per forward is only a few milliseconds (wav2vec2-base on
32 x 10 s clips: 6.6 ms of kernels, 6-9 ms of host time to launch them eagerly); the KV-cached decoders capture their step
the same way (audio2text/generate.py).  No tracing, no compiler: the captured launches are the eager ones.

    enc = GraphedForward(model, example_waveforms)      # warm-up (builds the derived weight caches), then capture
    out = enc(waveforms)                                 # copies the inputs into the captured buffers, replays

The result tensor is the graph's own output buffer: it is overwritten by the next call (clone it to keep it).

The captured launches hold raw pointers into the module's parameters AND into the values derived from them (f32 biases,
packed and folded weights).  The signature of every parameter and buffer (transformer.state_signature) is recorded at
capture; a call that finds it changed - an in-place ``copy_``, ``load_state_dict``, ``.to()`` - warms up and captures again
before it replays, so a replay never mixes two checkpoints.  The output buffer is then a NEW tensor: do not hold on to the
old one across a weight update.  The comparison is host work on every call - a handful of attribute reads per parameter
and buffer, in Python - on the very path that exists to remove host work; it has not been measured on small graphed modules
(the benchmark legs, ViT-B/16 at batch 256 and Whisper-base, do not go through this class).
Writes the signature cannot see (``p.data.copy_``, inference-mode parameters) need
``transformer.clear_derived(module)`` and a new GraphedForward.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .transformer import state_signature


class GraphedForward:
    def __init__(self, module: nn.Module, *example_inputs: Tensor, warmup: int = 2) -> None:
        if not example_inputs or not all(isinstance(x, Tensor) and x.is_cuda for x in example_inputs):
            raise RuntimeError("GraphedForward: tensor inputs on a HIP device (there is no CPU path)")
        self.module = module
        self.inputs = [x.clone() for x in example_inputs]
        self._warmup = max(1, warmup)
        self._capture()

    def _capture(self) -> None:
        module = self.module
        self._sig = state_signature(module)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(self._warmup):  # derived weights, position tables, kernel attributes: everything lazy happens here
                module(*self.inputs)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.output = module(*self.inputs)

    def __call__(self, *inputs: Tensor):
        if len(inputs) != len(self.inputs):
            raise ValueError(f"GraphedForward: captured with {len(self.inputs)} inputs, called with {len(inputs)}")
        for dst, src in zip(self.inputs, inputs):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError(f"GraphedForward: captured for {tuple(dst.shape)} {dst.dtype}, got {tuple(src.shape)} {src.dtype}")
            dst.copy_(src)
        if state_signature(self.module) != self._sig:  # the weights changed: the old launches point at a mixture of old and new
            torch.cuda.current_stream().synchronize()  # the last replay may still read what the rebuild frees
            self._capture()
        self.graph.replay()
        return self.output
