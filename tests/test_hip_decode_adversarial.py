"""Adversarial fp64 parity of the decode-step kernels of csrc/decode.hip through their C entry points: pm_dec_linear in its plain, q/k/v
(DL_QKV) and arg-max (DL_ARGMAX, the persistent dec_logits_kernel included) modes, pm_dec_linear_ksplit, pm_dec_linear_kparts,
pm_dec_embed, pm_dec_argmax_reduce, pm_dec_next_token, pm_dec_sample_topk and the self form of the fused attention block
(pm_dec_attention_fused, pm_dec_attention_fused_kv32, pm_dec_attention_chain on both of its sides); the cross form's extra key counts
joined attn_cases.DCASES, pm_dec_whisper_rules, pm_dec_advance and the *_ragged forms keep their own tests.  References, derived bounds, input families and the case list live in tests/decode_cases.py (its docstring maps every
launcher path to the cases that reach it; DESIGN.md "2g. Decode-step numerics contract" holds the derivations);
tests/test_decode_cases_cpu.py proves on the CPU that a correct kernel satisfies every assertion made here, that each defect in
decode_cases.MUTANTS does not, and that pm_dec_linear_plan sends every case to the instantiation it is listed under.

Per case (decode_cases.judge): the exact family EQUALS the reference, K parts and cache rows included; every other family stays within
1.5 x the derived bound (no measured number enters an assertion); every sentinel around every output - out, parts, ws_val / ws_idx,
tickets, both caches - is unchanged, and of a cache exactly row `pos` of each (b, h) is written; poison: operands cut out of NaN-filled
buffers; perm: permuted rows give the same bits; scale: out(2^k x) == 2^k out(x); tie: the lowest index wins in every arg-max tile and
over all tiles; the token tails - tok_cur, tokens_out, margin_out, the next x row, the position, the ticket - and the sampled token EQUAL
the reference's; the fused block's x_out is the fp32 row bit for bit, its stored k / v row is held to the half-ulp bound and the
attention is referred to the stored row; the K split leaves its tickets at zero and a second launch gives the same bits; the LayerNorm shape the launcher cannot
serve is refused with nothing written.  Each case prints "RATIO <op> <family> <case id> <max |err| / bound>" (pytest -s).

Default-dispatch cases run in this process.  PM_DEC_ROWSPLIT, PM_DEC_LOGITS_PERSIST and PM_DEC_LOGITS_WAVES are read once per process,
so their cases run in one child each (tests/decode_child.py, started with sys.executable one after another, each under a time limit
and with its exit status checked).  A child that times out, dies on a signal or exits with an error ends that part: no further child is
started and the remaining child tests fail, naming it; a HIP error in this process ends the rest of the file the same way.

Bit-identities across the switches: the 4-wave persistent kernel (PM_DEC_LOGITS_WAVES=4) gives the non-persistent kernel's
(PM_DEC_LOGITS_PERSIST=0) (max, index) pairs bit for bit at every K; the default 8-wave form partitions K over eight waves, so it does
at K <= 128 (four K steps: waves 4 - 7 add zeros) and is held to the bound beyond."""
import json
import os
import subprocess
import sys

import pytest
import torch

import decode_cases as DC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240  # seconds: a child takes ~15 s, most of it start-up and the float64 references on the CPU
FAULT: list[str] = []  # the first HIP error seen in this process: after it nothing more of this file touches the GPU
CHILD_ENVS = [e for e in DC.ENVS if e]
INDEX = {c.id: i for i, c in enumerate(DC.CASES)}


def _on_gpu(what: str, fn):
    assert not FAULT, f"not run: {FAULT[0]}"
    try:
        return fn()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory" in str(e):
            FAULT.append(f"{what} raised a HIP error: {str(e)[:200]}")
        raise


@pytest.fixture(scope="module")
def gpu():
    """(library, the device's case list: decode_cases.CASES with the CU count of this device where a shape depends on it)"""
    assert torch.cuda.is_available()
    from pytorch_models._hip import lib

    return lib(), DC.cases(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def default_records():
    return {}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """switch -> {case index: record} from one child process per switch, or a string that says why there are none."""
    out = {}
    broken = None
    for env in CHILD_ENVS:
        broken = broken or (FAULT[0] if FAULT else None)
        if broken:
            out[env] = f"not started: {broken}"
            continue
        path = str(tmp_path_factory.mktemp("decode") / f"{env}.jsonl")
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "decode_child.py"), "run", env, path], env=dict(os.environ, **DC.ENVS[env]),
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            rc, log = r.returncode, r.stdout + r.stderr[-3000:]
        except subprocess.TimeoutExpired as e:
            rc, log = None, f"{e.stdout or ''}"
        print(log)
        recs = {}
        if os.path.exists(path):
            recs = {d["i"]: d for d in map(json.loads, open(path).read().splitlines())}
        out[env] = recs
        if rc != 0:  # a hang, a fault or an exception in the child - a HIP error included: nothing more of this file touches the GPU
            how = "timed out" if rc is None else f"died on signal {-rc}" if rc < 0 else f"exited with {rc}"
            broken = f"the child of {env} {how} after {len(recs)} cases: {log[-1500:]}"
            out[f"broken:{env}"] = broken
            FAULT.append(broken)
    return out


def _judge_here(gpu, case_id):
    L, real = gpu
    c = real[INDEX[case_id]]
    inp = DC.build(c, torch.cuda.get_device_properties(0).multi_processor_count)
    return c, _on_gpu(c.id, lambda: DC.judge(c, inp, DC.reference(c, inp), lambda c_, P: DC.run(L, c_, P), dev="cuda"))


@pytest.mark.parametrize("case", [c for c in DC.CASES if not c.env], ids=lambda c: c.id)
def test_default_dispatch(gpu, default_records, case):
    from pytorch_models._hip import ops

    c = gpu[1][INDEX[case.id]]
    if c.op in DC.MODE:
        rep = ops.dec_linear_plan(**DC.plan_args(c))
        if c.refused:
            assert rep == {"refused": c.refused}, rep
        else:
            wrong = {k: (v, rep.get(k)) for k, v in c.expect if rep.get(k) != v}
            assert not wrong, f"{c.id}: the default dispatch goes elsewhere (field: (listed, reported)): {wrong}"
    c, rec = _judge_here(gpu, case.id)
    default_records[INDEX[case.id]] = rec
    print(DC.figure(rec))
    assert rec["ok"], DC.explain(rec)


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.env], ids=lambda c: c.id)
def test_switched_dispatch(children, case):
    recs = children[case.env]
    assert not isinstance(recs, str), recs
    rec = recs.get(INDEX[case.id])
    assert rec is not None, children.get(f"broken:{case.env}", f"{case.id}: the child of {case.env} left no record")
    print(DC.figure(rec))
    assert rec["plan_ok"], f"{case.id}: {DC.ENVS[case.env]} reaches {rec['plan']}, listed {dict(case.expect)}"
    assert rec["ok"], DC.explain(rec)


def _twin(case, env):
    """The index of the same launch under another switch."""
    ids = [i for i, c in enumerate(DC.CASES) if c.env == env and (c.op, c.family, c.M, c.N, c.K, c.ln, c.bias) == (case.op, case.family, case.M, case.N, case.K, case.ln, case.bias)]
    return ids[0] if ids else None


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.env == "waves4"], ids=lambda c: c.id)
def test_four_wave_persistent_pairs_equal_the_non_persistent_kernels(children, case):
    """dec_logits_kernel<MT, 4, 2> forms every sum in dec_linear_kernel's order: the same (max, index) pairs bit for bit, at every K."""
    a, b = children["waves4"], children["persist0"]
    assert not isinstance(a, str) and not isinstance(b, str), (a, b)
    j = _twin(case, "persist0")
    assert j is not None and INDEX[case.id] in a and j in b, children.get("broken:waves4") or children.get("broken:persist0") or "no record"
    assert a[INDEX[case.id]]["digest"] == b[j]["digest"]


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.op == "argmax" and not c.env and c.ln and c.N >= 4040 and c.M <= 32 and c.K <= 128], ids=lambda c: c.id)
def test_eight_wave_persistent_pairs_equal_the_non_persistent_kernels_up_to_four_k_steps(children, default_records, case):
    """dec_logits_kernel<MT, 8, 4> gives wave w the K steps w, w + 8: with at most four K steps (K <= 128) waves 4 - 7 add zeros to the
    four-wave sums, LayerNorm statistics included, and the pairs are the non-persistent kernel's bit for bit.  Beyond, the partition
    differs and each kernel is held to the bound on its own (test_default_dispatch, test_switched_dispatch)."""
    j = _twin(case, "persist0")
    assert j is not None, "no PM_DEC_LOGITS_PERSIST=0 twin listed"
    b = children["persist0"]
    assert not isinstance(b, str), b
    assert INDEX[case.id] in default_records and j in b, children.get("broken:persist0") or "no record (run the whole file)"
    assert default_records[INDEX[case.id]]["digest"] == b[j]["digest"]
