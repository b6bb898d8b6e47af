"""Host time per eager wrapper call at the shapes of tests/wrapper_cases.py: a loop of N calls of linear, layernorm, attention and
dwconv7_ln in one process, synchronised once at the end of each repeat (profiles/wrappers/README.md).  One JSON line.
    python tools/wrapper_host_cost.py [label]           on a GPU
    python tools/wrapper_host_cost.py [label] --stub    anywhere: the library replaced by a stub that returns 0, CPU tensors -
                                                        the Python work of the wrapper alone"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-models_amd")]
import torch  # noqa: E402

import wrapper_cases as WC  # noqa: E402
from pytorch_models._hip import ops  # noqa: E402

torch.set_grad_enabled(False)
N, REPS = 4000, 7
stub = "--stub" in sys.argv
label = next((a for a in sys.argv[1:] if not a.startswith("--")), "tree")
if stub:
    class _Stub:
        def __getattr__(self, name):
            return lambda *a: 0
    _lib = _Stub()
    ops.lib, ops._stream, ops.check_devices = (lambda: _lib), (lambda: 0), (lambda *ts: None)
dev = torch.device("cpu" if stub else "cuda")
sync = (lambda: None) if stub else torch.cuda.synchronize
res = {}
for rid in ("linear", "layernorm", "attention", "dwconv7_ln"):
    row = WC.ROWS[rid]
    kw = row.build(dev)
    fn = getattr(ops, row.fn)
    for _ in range(300):
        fn(**kw)
    sync()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(N):
            fn(**kw)
        t1 = time.perf_counter()
        sync()
        ts.append(round((t1 - t0) / N * 1e6, 3))
    res[rid] = ts
print(json.dumps({"tree": label, "stub": stub, "us_per_call": res}))
