"""Child process of the decode-step parity suite: PM_DEC_ROWSPLIT, PM_DEC_LOGITS_PERSIST and PM_DEC_LOGITS_WAVES are read once per
process, so every switch gets a fresh one.

    python decode_child.py plan <env>         host only: pm_dec_linear_plan's report for every case listed under <env>; prints {case id: report}
    python decode_child.py run <env> <out>    on the GPU: decode_cases.judge on every case listed under <env>, one JSON record per case appended
                                              to <out> (flushed per case, so a crash leaves what was done); the first HIP error ends the run
Started by tests/test_decode_cases_cpu.py and tests/test_hip_decode_adversarial.py with sys.executable; not a test module."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "pytorch-models_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import decode_cases as DC  # noqa: E402


def main() -> int:
    mode, env = sys.argv[1], sys.argv[2]
    for k, v in DC.ENVS[env].items():
        assert os.environ.get(k) == v, f"start me with {k}={v}"
    torch.set_grad_enabled(False)
    from pytorch_models._hip import lib, ops

    if mode == "plan":
        print(json.dumps({c.id: ops.dec_linear_plan(**DC.plan_args(c)) for c in DC.CASES if c.env == env}))
        return 0
    assert torch.cuda.is_available()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = lib()
    with open(sys.argv[3], "a") as f:
        for i, c in ((i, c) for i, c in enumerate(DC.cases(cus)) if c.env == env):  # i: the case's place in decode_cases.CASES
            rep = ops.dec_linear_plan(**DC.plan_args(c)) if c.op in DC.MODE else {}
            inp = DC.build(c, cus)
            rec = DC.judge(c, inp, DC.reference(c, inp), lambda c_, P: DC.run(L, c_, P), dev="cuda")
            rec["plan_ok"] = all(rep.get(k) == v for k, v in c.expect)
            rec["plan"] = rep
            rec["i"] = i
            rec["ratio"] = rec["ratio"] if rec["ratio"] != float("inf") else 1e300
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(DC.figure(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
