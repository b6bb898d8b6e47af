"""Child process of the GEMM parity suite: PM_GEMM_KERNEL is read once per process, so every forced kernel id gets a fresh one.

    python linear_child.py plan <id>        host only: pm_linear_bf16_plan for every case forced to <id>; prints {case id: kernel} as JSON
    python linear_child.py run <id> <out>   on the GPU: asserts the plan of every placement, runs linear_cases.judge on every case forced to <id>, appends
                                            one JSON record per case to <out> (flushed per case, so a crash leaves what was done)
    python linear_child.py reach <id>       host only: pm_linear_bf16_plan on linear_cases.reach_probes(<id>), made-up pointers; prints {probe: kernel} as JSON
    python linear_child.py far <id> <out>   on the GPU: linear_cases.judge_far on every far case forced to <id>, one poisoned arena for all of them; a
                                            record per case as `run` writes them, with `planned` RECORDED, not asserted: the dispatcher may move a case
                                            it cannot address
Started by tests/test_linear_cases_cpu.py and tests/test_hip_linear_adversarial.py with sys.executable; not a test module."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "pytorch-models_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import linear_cases as LC  # noqa: E402


def main() -> int:
    mode, kid = sys.argv[1], int(sys.argv[2])
    assert os.environ.get("PM_GEMM_KERNEL") == str(kid), "start me with PM_GEMM_KERNEL=<id>"
    torch.set_grad_enabled(False)
    from pytorch_models._hip import ops

    if mode == "plan":
        got = {}
        for case in LC.FORCED_CASES[kid]:
            inp = LC.build(case)
            got[case.id] = LC.plan(ops, case, LC.place(case, inp))
            if case.family == "poison":
                poisoned = LC.plan(ops, case, LC.place(case, inp, poison=True))
                got[case.id] = got[case.id] if poisoned == got[case.id] else -100 - poisoned
        print(json.dumps(got))
        return 0
    if mode == "reach":
        from pytorch_models._hip import lib

        print(json.dumps({name: int(lib().pm_linear_bf16_plan(*LC.plan_args(**g))) for name, (g, _) in LC.reach_probes(kid).items()}))
        return 0
    assert torch.cuda.is_available()
    if mode == "far":
        import wrapper_cases as WC

        arena = WC.Arena(WC.Arena.bytes_for(32), "cuda")
        with open(sys.argv[3], "a") as f:
            for case in LC.FAR_FORCED[kid]:
                inp = LC.build(case)
                rec = LC.judge_far(case, inp, LC.reference(case, inp), ops, arena)  # a HIP error ends the child: exit code 1, no further case
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(LC.figure(rec), "planned", rec.get("planned"), "refused" if rec.get("refused") else "ran", flush=True)
        return 0
    with open(sys.argv[3], "a") as f:
        for case in LC.FORCED_CASES[kid]:
            inp = LC.build(case)
            plans = []  # pm_linear_bf16_plan on every placement the case launches: plain, poisoned (other lds and bases), permuted

            def ask(P, case=case, plans=plans):
                plans.append(LC.plan(ops, case, P))
                assert plans[-1] == kid, f"{case.id}: PM_GEMM_KERNEL={kid} reaches kernel {plans[-1]} (poison={P['poison']})"

            try:
                rec = LC.judge(case, inp, LC.reference(case, inp), lambda c, P: LC.run(ops, c, P), dev="cuda", on_place=ask)
            except AssertionError:
                rec = dict(id=case.id, op=case.op, kid=kid, family=case.family, ok=False, ratio=float("inf"), mismatches=-1)
            rec["planned"] = next((p for p in plans if p != kid), kid)
            rec["placements"] = len(plans)
            rec["ratio"] = rec["ratio"] if rec["ratio"] != float("inf") else 1e300
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(LC.figure(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
