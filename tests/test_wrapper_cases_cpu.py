"""CPU: the wrapper operand contract without a GPU (tests/wrapper_cases.py).

``lib()`` is replaced by a recording stub - every pm_* entry point records its arguments and returns 0, the host-only size
and *_supported queries return constants -, ``_stream`` returns 0 and ``check_devices`` is wrapped by a recorder that notes
the ``id`` of what it is given and does not raise.  Canonical operands are CPU tensors.  Asserted:
  * completeness: every function of ops.py that takes a Tensor has a row or an exemption, every Tensor parameter is passed
    by a row, every operand gets every variant of the contract's table that applies to it (by introspection);
  * the canonical call of every row reaches a launch;
  * device coverage: every tensor operand, nested ones included, has been seen by check_devices before the first launch;
  * refusals happen with zero recorded launches and leave the in-place operands alone;
  * bounds: the in-bounds rule holds for every variant;
  * the audit: a variant that reaches a launch does so with the information that makes it right.  A contiguous variant of
    the canonical dtype (offset, rank) must launch with the canonical integers; any other one must change the launch - a
    stride, a dtype code, a size, or a copy in place of the operand's own pointer.  Accepted with the canonical integers and
    its own pointer = the kernel reads data_ptr() as packed: a hole.
Far operands (wrapper_cases.check_row_far): every operand with a ``rowpad`` / ``rowpad0`` variant gets its
far variants, as views into one lazily mapped arena of which only the views are touched.  Asserted:
  * completeness and containment (pure arithmetic on base, strides and arena size: the gate in front of any GPU run);
  * refusals happen with zero recorded launches and leave the in-place operands alone;
  * the audit: an accepted far operand reaches the C call with its own pointer and the far stride among the integers (or as a
    copy); the width audit: every recorded integer of magnitude >= 2^31 sits at a position SIGNATURES declares 64 bits wide
    (ctypes masks an int given to a c_int parameter without raising);
  * the driver has teeth: the same checker at a 16-bit width over a tiny arena reports each of five toy kernels with one
    planted 16-bit defect, and passes their wide twin.
``python tests/test_wrapper_cases_cpu.py`` prints the accepted (wrapper, operand, variant) triples, then the far ones."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "pytorch-models_amd")):  # also when run as a script
    if _p not in sys.path:
        sys.path.insert(0, _p)
import wrapper_cases as WC  # noqa: E402
from pytorch_models._hip import SIGNATURES, decode_plan, ops  # noqa: E402

torch.set_grad_enabled(False)
CPU = torch.device("cpu")
SIZE_QUERIES = ("_ws_bytes", "_scratch_floats", "_workspace_floats", "_workspace_doubles", "pm_dec_argmax_tile")


class Recorder:
    """the stub library, the check_devices recorder and the audit of one row"""

    def __init__(self) -> None:
        self.launches: list = []
        self.seen: list = []  # (id, launches recorded so far)
        self.canon: list | None = None

    def __getattr__(self, name: str):
        if not name.startswith("pm_"):
            raise AttributeError(name)
        if name.endswith("_supported"):
            return lambda *a: 1
        if name.endswith(SIZE_QUERIES):
            return lambda *a: 64
        if name == "pm_strerror":
            return lambda code: b"stub"

        def launch(*args):
            self.launches.append((name, args))
            return 0
        launch.__name__ = name
        return launch

    def check_devices(self, *ts) -> None:
        self.seen += [(id(t), len(self.launches)) for t in ts if t is not None]

    # ---- the hook of wrapper_cases.check_row
    def begin(self) -> None:
        self.launches, self.seen = [], []

    def normal(self, kw: dict) -> list:
        """the recorded launches with every pointer replaced by the operand it points to ('buf' for anything else)"""
        names = {t.data_ptr(): WC.path_name(p) for p, t in WC.operands(kw)}

        def one(a):
            if isinstance(a, ctypes.Array):
                return tuple(one(int(v or 0)) for v in a)
            if isinstance(a, int) and not isinstance(a, bool):
                return names.get(a, "buf" if abs(a) >= 2 ** 32 else a)
            return a
        return [(name, tuple(one(a) for a in args)) for name, args in self.launches]

    def canonical(self, kw: dict) -> None:
        self.canon = self.normal(kw)

    def end(self, r, path, v, kw: dict, refused: bool) -> list[str]:
        if refused:
            return [f"refused after {len(self.launches)} launches"] if self.launches else []
        if path[0] in r.host_ok or (path[0] in r.free_shape and v.reshaped):
            return []  # a CPU tensor of a host-or-device operand is read back and uploaded; a free-shape operand is another problem
        got = self.normal(kw)
        plain = v.tensor.is_contiguous() and v.tensor.dtype == WC.get(kw, path).dtype and not v.tag.startswith("dtype")
        if plain and got != self.canon:
            return [f"HOLE: a contiguous operand of another rank changes the launch: {_delta(self.canon, got)}"]
        if not plain and got == self.canon:
            return ["HOLE: accepted, and the launch is the canonical one: the kernel reads data_ptr() as packed " + v.tag.split(":")[0]]
        return []

    def end_far(self, r, path, c, kw: dict, refused: bool) -> list[str]:
        """the hook of wrapper_cases.check_row_far"""
        if refused:
            return [f"refused after {len(self.launches)} launches"] if self.launches else []
        bad, ptr, far = [], c.tensor.data_ptr(), c.strides[c.dim]
        flat = [(name, [int(v or 0) for a in args for v in (a if isinstance(a, ctypes.Array) else [a])
                        if isinstance(v, int) and not isinstance(v, bool) or v is None]) for name, args in self.launches]
        if any(ptr in ints for _, ints in flat) and not any(ptr in ints and far in ints for _, ints in flat):
            bad.append(f"HOLE: accepted with its own pointer, and no launch that takes it is told the stride {far}")
        return bad + width_audit(self.launches)


def width_audit(launches) -> list[str]:
    """every recorded integer argument of magnitude >= 2^31 must be declared 64 bits wide at its position"""
    bad = []
    for name, args in launches:
        types = SIGNATURES[name][0]
        for i, a in enumerate(args):
            if isinstance(a, int) and not isinstance(a, bool) and abs(a) >= 2 ** 31 and \
                    types[i] not in (ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64):
                bad.append(f"HOLE: {name} argument {i} = {a} is declared {types[i].__name__}: ctypes masks it without raising")
    return bad


def _delta(a, b) -> str:
    for (n1, x), (n2, y) in zip(a, b):
        if n1 != n2:
            return f"{n1} vs {n2}"
        d = [(i, p, q) for i, (p, q) in enumerate(zip(x, y)) if p != q]
        if d:
            return f"{n1} args {d}"
    return f"{len(a)} vs {len(b)} launches"


def _install(monkeypatch) -> Recorder:
    r = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: r)
    monkeypatch.setattr(decode_plan, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "check_devices", r.check_devices)
    monkeypatch.setattr(ops, "LAUNCH_LOG", None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)

    class _Stream:
        cuda_stream = 0

        def synchronize(self):
            pass
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _Stream())
    return r


@pytest.fixture
def rec(monkeypatch):
    return _install(monkeypatch)


def _public_functions():
    return {n: f for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")}


def _takes_tensor(f) -> bool:
    sig = inspect.signature(f)
    return any("Tensor" in str(p.annotation) for p in sig.parameters.values()) or ".data_ptr()" in inspect.getsource(f)


def test_every_tensor_taking_wrapper_has_a_row_or_an_exemption():
    fns = _public_functions()
    rows = {r.fn for r in WC.ROWS.values()}
    assert rows <= set(fns), rows - set(fns)
    assert set(WC.EXEMPT) <= set(fns) and not rows & set(WC.EXEMPT), "stale exemptions"
    missing = [n for n, f in fns.items() if _takes_tensor(f) and n not in rows and n not in WC.EXEMPT]
    assert not missing, f"ops.py functions that take a Tensor without a row in tests/wrapper_cases.py: {missing}"
    # no-tensor helpers may be exempt only as what they are
    for n in WC.EXEMPT:
        assert WC.EXEMPT[n], n


def test_every_tensor_parameter_is_an_operand_of_some_row(rec):
    fns = _public_functions()
    passed: dict = {}
    for r in WC.ROWS.values():
        kw = r.build(CPU)
        passed.setdefault(r.fn, set()).update(p[0] for p, _ in WC.operands(kw))
    lacking = []
    for fn, names in passed.items():
        for p in inspect.signature(fns[fn]).parameters.values():
            if "Tensor" in str(p.annotation) and p.name not in names and (fn, p.name) not in WC.UNCOVERED:
                lacking.append(f"{fn}({p.name})")
    assert not lacking, f"Tensor parameters that no row of tests/wrapper_cases.py passes: {lacking}"


def test_every_operand_gets_every_variant_that_applies(rec):
    for r in WC.ROWS.values():
        for path, t in WC.operands(r.build(CPU)):
            vs = WC.variants(t)
            tags = [v.tag for v in vs]
            assert len(tags) == len(set(tags)) and set(tags) == WC.applicable_tags(t), (r.id, path, tags, WC.applicable_tags(t))
            for v in vs:
                v.check_bounds()
                assert v.tensor.shape == t.shape or v.reshaped, (r.id, path, v.tag)
                if v.tag != "expanded" and not v.tag.startswith("dtype"):
                    assert WC.same_bits(v.tensor.reshape(-1) if not v.must_raise else v.tensor.transpose(-1, -2).reshape(-1), t.reshape(-1))
                if v.tag != "expanded":  # everything outside the view is poison
                    inside = torch.zeros(v.parent.numel(), dtype=torch.bool)
                    inside.as_strided(v.tensor.shape, v.tensor.stride(), v.offset).fill_(True)
                    rest = v.parent[~inside]
                    assert rest.numel() and bool((rest.isnan() if rest.dtype.is_floating_point else (rest == WC.SENTINEL) | (rest == 0x7F)).all())


@pytest.mark.parametrize("rid", list(WC.ROWS))
def test_canonical_call_launches_after_the_device_check(rid, rec):
    r = WC.ROWS[rid]
    kw = r.build(CPU)
    rec.begin()
    WC.call(ops, r, kw)
    assert rec.launches, f"{rid}: the canonical call launched nothing"
    early = {i for i, n in rec.seen if n == 0}
    unseen = [WC.path_name(p) for p, t in WC.operands(kw) if id(t) not in early and p[0] not in r.host_ok]
    assert not unseen, f"{rid}: operands check_devices has not seen before the first launch: {unseen}"


@pytest.mark.parametrize("rid", list(WC.ROWS))
def test_variants_are_refused_before_a_launch_or_reach_it_whole(rid, rec):
    problems, _ = WC.check_row(ops, WC.ROWS[rid], CPU, compare=False, hook=rec)
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


# ------------------------------------------------------------------------------------------------------------ far operands
@pytest.fixture(scope="module")
def arena():
    a = WC.Arena(WC.Arena.bytes_for(32), CPU, poisoned=False)  # torch.empty maps lazily: only the views are ever touched
    yield a
    del a.words


def test_every_padded_dimension_gets_its_far_variants(arena):
    n = 0
    for r in WC.ALL_FAR_ROWS.values():
        for path, t in WC.operands(r.build(CPU)):
            cs = WC.far_cases(t, arena)
            got = [(c.tag, c.dim) for c in cs]
            assert len(got) == len(set(got)) and set(got) == WC.applicable_far(t), (r.id, path, got, WC.applicable_far(t))
            for c in cs:
                n += 1
                where = (r.id, WC.path_name(path), c.name)
                assert not arena.holds(c), (where, arena.holds(c))
                assert sum(c.needs()) <= WC.ARENA_CAP, where
                v, last = c.tensor, (t.shape[c.dim] - 1) * c.strides[c.dim] * c.item
                assert v.shape == t.shape and v.stride() == c.strides and v.data_ptr() == arena.words.data_ptr() + arena.base, where
                assert last > WC.far_boundary(c.tag, c.item) and c.strides[c.dim] % WC.FAR_ALIGN == 0, where
                assert last - WC.far_boundary(c.tag, c.item) <= (t.shape[c.dim] - 1) * WC.FAR_ALIGN * c.item, (where, "not just past")
                assert all(s == p for d, (s, p) in enumerate(zip(c.strides, WC._packed(t.shape))) if d != c.dim), where
                assert ops._apart(v), where
    assert n > 300, n


@pytest.mark.parametrize("rid", list(WC.ALL_FAR_ROWS))
def test_far_variants_are_refused_before_a_launch_or_reach_it_whole(rid, rec, arena):
    problems, _, _ = WC.check_row_far(ops, WC.ALL_FAR_ROWS[rid], CPU, arena, compare=False, hook=rec)
    assert not problems, "\n".join([f"{len(problems)} problems:"] + problems)


def test_width_audit_sees_a_narrow_parameter():
    assert width_audit([("pm_geglu", (1 << 40, 2 ** 31 + 64, 1 << 41, 8, 2, 4, 0))]) == []
    bad = width_audit([("pm_layernorm", (1 << 40, 64, 2 ** 31 + 64, None, None, 1e-5, 1 << 41, 64, 0, 2, 64, 0))])
    assert len(bad) == 1 and "argument 2" in bad[0] and "c_int" in bad[0], bad


# ---- teeth: toy kernels at a 16-bit width over a tiny arena, through the same driver
TOY_W = 16


def _toy(defect: str):
    """y[m, :] = 2 * x[m, :] + 1 over raw words of the arena, offsets formed as a C launcher would form them; ``defect`` names
    the one place where the arithmetic is ``TOY_W`` bits wide"""
    def row(t, off, K):  # K floats at byte address data_ptr() + off, as a kernel sees them
        return torch.frombuffer((ctypes.c_float * K).from_address(t.data_ptr() + off), dtype=torch.float32)

    def fn(x, out):
        (M, K), it = x.shape, x.element_size()
        ldx, ldo = x.stride(0), out.stride(0)
        if ldx < K or ldo < K:
            raise ValueError("toy: rows overlap")
        for m in range(M):
            xo, oo = m * ldx * it, m * ldo * it
            if defect == "int32 elements":
                xo = WC.wrap(m * ldx, TOY_W, True) * it
            elif defect == "uint32 bytes":
                xo = WC.wrap(m * ldx * it, TOY_W, False)
            elif defect == "int32 bytes":
                xo = WC.wrap(m * ldx * it, TOY_W, True)
            elif defect == "(int)ld":
                xo = m * WC.wrap(ldx, TOY_W, True) * it
            elif defect == "wrapped write":
                oo = WC.wrap(m * ldo * it, TOY_W, False)
            row(out, oo, K).copy_(row(x, xo, K) * 2 + 1)
        return None
    return fn


def _toy_row(arena):
    def build(g):
        return dict(x=g.f(2, 8), out=g.z(2, 8))
    return WC.Row("toy", "toy", lambda dev, seed=0: build(WC.Gen(dev, WC.SEED)), ("out",))


# defect (named at its 32-bit width; planted at TOY_W bits) -> the variants that must report it, from the arithmetic alone: with two
# f32 rows the element offset and the stride itself pass 2^(w-1) only at far:2Ge; a byte offset passes 2^w from far:4G on, and as a
# signed register it is wrong from 2^(w-1) on - negative at far:2G, short by 2^w behind it
TOY_DEFECTS = {"int32 elements": ("x far:2Ge@0",), "uint32 bytes": ("x far:4G@0", "x far:2Ge@0"), "int32 bytes": ("x far:2G@0", "x far:4G@0", "x far:2Ge@0"),
               "(int)ld": ("x far:2Ge@0",), "wrapped write": ("out far:4G@0", "out far:2Ge@0")}


@pytest.mark.parametrize("defect", [None] + list(TOY_DEFECTS))
def test_far_driver_reports_each_planted_narrow_offset(defect):
    import types
    toy_arena = WC.Arena(WC.Arena.bytes_for(TOY_W, slack=4096), CPU)
    problems, acc, ref = WC.check_row_far(types.SimpleNamespace(toy=_toy(defect)), _toy_row(toy_arena), CPU, toy_arena, compare=True,
                                          width=TOY_W)
    assert len(acc) == 6 and not ref, (acc, ref)  # x and out at the three distances
    if defect is None:
        assert not problems, problems
        return
    hit = {p.split(": ")[0].replace("toy ", "", 1) for p in problems}
    assert hit == set(TOY_DEFECTS[defect]), (defect, problems)
    if defect == "wrapped write":
        assert any("wrote outside the view" in p for p in problems), problems


def far_triples():
    """(accepted, refused, problems) of the far variants on the CPU stage"""
    mp = pytest.MonkeyPatch()
    try:
        r = _install(mp)
        a = WC.Arena(WC.Arena.bytes_for(32), CPU, poisoned=False)
        acc, ref, probs = [], [], []
        for row in WC.ALL_FAR_ROWS.values():
            p, x, y = WC.check_row_far(ops, row, CPU, a, compare=False, hook=r)
            acc, ref, probs = acc + x, ref + y, probs + p
        return acc, ref, probs
    finally:
        mp.undo()


def accepted_triples() -> list:
    """the accepted set: every (row, operand, variant) that reaches a launch on the CPU stage"""
    mp = pytest.MonkeyPatch()
    try:
        r = _install(mp)
        out = []
        for row in WC.ROWS.values():
            problems, acc = WC.check_row(ops, row, CPU, compare=False, hook=r)
            out += [(a, "HOLE" if any(p.startswith(f"{a[0]} {a[1]} {a[2]}:") for p in problems) else "ok") for a in acc]
        return out
    finally:
        mp.undo()


if __name__ == "__main__":
    for (rid, operand, tag), verdict in accepted_triples():
        print(f"{rid:28s} {operand:18s} {tag:16s} {verdict}")
    acc, ref, probs = far_triples()
    for kind, ts in (("accepted", acc), ("refused", ref)):
        for rid, operand, tag in ts:
            print(f"{rid:28s} {operand:18s} {tag:16s} {kind}")
    print(f"far: {len(acc) + len(ref)} generated, {len(acc)} accepted, {len(ref)} refused, {len(probs)} problems")
    for p in probs:
        print("  ", p)
