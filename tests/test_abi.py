"""CPU: the C-ABI library loads and exports every function include/pm_mi355x.h declares (no compute)."""
import ctypes
import os

from pytorch_models import _hip


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_hip.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    L = ctypes.CDLL(_hip.LIB_PATH)
    declared = _hip.header_functions()
    assert declared, "no functions parsed from the header"
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/pm_mi355x.h but not exported"
    assert sorted(_hip.SIGNATURES) == declared, "ctypes SIGNATURES table out of sync with the header"


def test_library_exports_nothing_the_header_does_not_declare():
    """exported pm_* == declared: the shipped library carries no undeclared entry point (an experiment's bench export
    rode along).  The product library is checked against pm_mi355x.h; an experiments build (PM_MI355X_LIB=...libpm_mi355x_exp.so)
    additionally against pm_mi355x_experiments.h."""
    import re
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({l.split()[-1] for l in out.splitlines() if re.match(r"^[0-9a-f]+ T pm_[a-z0-9_]+$", l.strip())})
    allowed = set(_hip.header_functions())
    if os.path.basename(_hip.LIB_PATH) != "libpm_mi355x.so":
        allowed |= set(_hip.EXPERIMENT_SIGNATURES)
    extra = [n for n in exported if n not in allowed]
    assert exported and not extra, f"exported but not declared: {extra}"


def test_abi_version_and_error_strings():
    L = _hip.lib()
    assert L.pm_abi_version() == 1
    for code in range(0, 5):
        assert L.pm_strerror(code)
    assert b"unknown" in L.pm_strerror(99)


def test_host_side_validation_launches_nothing():
    """Rejected calls return an error code before any HIP call, so this is safe without a GPU."""
    L = _hip.lib()
    assert L.pm_linear_bf16(None, 0, None, 0, None, None, 0, 0, None, 0, 0, 1, 1, 1, 0, None) == 1  # PM_EINVAL
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    # K not a multiple of 8 -> PM_EUNSUPPORTED
    assert L.pm_linear_bf16(p, 72, p, 72, None, None, 0, 0, p, 8, 0, 4, 8, 68, 0, None) == 2
    # misaligned leading dimension -> PM_EALIGN
    assert L.pm_linear_bf16(p, 65, p, 64, None, None, 0, 0, p, 8, 0, 4, 8, 64, 0, None) == 4
    assert L.pm_layernorm(p, 12, 0, p, p, 1e-5, p, 12, 0, 4, 12, None) == 2
    assert L.pm_vit_tokens(p, p, p, p, None, p, 1, 224, 224, 14, 384, None) == 2


def test_dec_linear_plan_is_a_host_side_query():
    """pm_dec_linear_plan dereferences nothing but its report and launches nothing: shapes in, the launchers' decision or refusal out."""
    L = _hip.lib()
    rep = (ctypes.c_int32 * 12)(*([-1] * 12))
    p = ctypes.addressof(rep)
    assert L.pm_dec_linear_plan(17, 130, 160, 0, 0, 0, None) == 1  # PM_EINVAL: no report
    assert L.pm_dec_linear_plan(0, 130, 160, 0, 0, 0, p) == 1 and L.pm_dec_linear_plan(65, 130, 160, 0, 0, 0, p) == 2
    assert L.pm_dec_linear_plan(17, 130, 1312, 1, 0, 0, p) == 2 and L.pm_dec_linear_plan(17, 130, 160, 0, 0, 9, p) == 1
    assert list(rep) == [-1] * 12  # a refusal writes nothing
    assert L.pm_dec_linear_plan(1, 16, 32, 0, 0, 0, p) == 0
    assert list(rep) == [0, 1, 1, 4, 0, 4, 1, 1, 1, 1, -1, -1]  # dec_linear_kernel<., 1, 1, 4, false>, one workgroup; 10 fields, no more
    assert L.pm_dec_linear_plan(1, 300, 1280, 1, 2, 0, p) == 0 and rep[2] * 16 == L.pm_dec_argmax_tile(1280)  # FT x 16 = the arg-max tile


def test_mixer_token_mix_plan_is_a_host_side_query():
    """pm_mixer_token_mix_plan dereferences nothing but its report and launches nothing, and agrees with pm_mixer_token_mix_supported."""
    L = _hip.lib()
    rep = (ctypes.c_int32 * 10)(*([-1] * 10))
    p = ctypes.addressof(rep)
    assert L.pm_mixer_token_mix_plan(16, 32, 64, None) == 1  # PM_EINVAL: no report
    for T, Dt, C in ((0, 32, 64), (16, 48, 64), (16, 32, 96), (16, 1024, 128), (4097, 32, 64)):
        assert L.pm_mixer_token_mix_plan(T, Dt, C, p) == 2 and not L.pm_mixer_token_mix_supported(T, Dt, C), (T, Dt, C)
    assert list(rep) == [-1] * 10  # a refusal writes nothing
    assert L.pm_mixer_token_mix_plan(196, 384, 768, p) == 0 and L.pm_mixer_token_mix_supported(196, 384, 768)
    # NB 4: the slab 128 x (208 + 8) x 2 B is region_a, + 128 x (384 + 8) x 2 B of hidden activations; 8 fields, no more
    assert list(rep) == [4, 55296 + 100352, 55296, 13, 24, 12, 7, 0, -1, -1]
    assert L.pm_mixer_token_mix_plan(1, 32, 64, p) == 0
    assert list(rep)[:8] == [2, 33792 + 64 * 40 * 2, 33792, 1, 2, 1, 1, 1]  # NB 2 (C % 128), region_a = 8 waves x 32 x 33 x 4 B of scratch


# ---- the types, not only the names: every argtypes list and restype against the header's prototypes
_C_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}


def _strip(src: str) -> str:
    """the header without comments and preprocessor lines"""
    import re

    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))


def _ctype(decl: str, name: bool):
    """the ctypes type of one C declarator: a pointer is c_void_p (``const char*``: c_char_p), a scalar by its type name"""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if words[:2] == ["const", "char"] else ctypes.c_void_p
    words = [w for w in words if w != "const"]
    assert len(words) == (2 if name else 1), decl
    return _C_TYPES[words[0]]


def _prototypes(path: str) -> dict:
    import re

    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(pm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _strip(open(path).read())):
        params = params.strip()
        args = [] if params in ("", "void") else [_ctype(p.strip(), True) for p in params.split(",")]
        assert name not in out, f"{name} declared twice"
        out[name] = (args, _ctype(ret.strip(), False))
    return out


def _mismatches(table: dict, protos: dict) -> list:
    bad = [f"{n}: in the table, not in the header" for n in table if n not in protos]
    for n, (args, ret) in protos.items():
        if n not in table:
            bad.append(f"{n}: declared, not in the table")
            continue
        targs, tret = table[n]
        if len(targs) != len(args):
            bad.append(f"{n}: {len(targs)} argtypes for {len(args)} parameters")
        bad += [f"{n}: argument {i} is {t.__name__} in the table, {a.__name__} in the header" for i, (t, a) in enumerate(zip(targs, args)) if t is not a]
        if tret is not ret:
            bad.append(f"{n}: restype {tret.__name__} in the table, {ret.__name__} in the header")
    return bad


def test_signature_table_matches_the_header_prototypes_type_by_type():
    """sorted(SIGNATURES) == the declared names says nothing about the 119 hand-written argtypes lists: a c_int where the header
    takes an int64_t passes the upper half of a stride as the next argument's garbage on no platform ctypes checks."""
    protos = _prototypes(_hip.HEADER_PATH)
    assert len(protos) == len(_hip.header_functions()), sorted(set(_hip.header_functions()) ^ set(protos))
    bad = _mismatches(_hip.SIGNATURES, protos)
    assert not bad, "\n".join(bad)
    args, ret = _hip.SIGNATURES["pm_linear_bf16"]  # the comparison itself: one stride narrowed to an int must be reported
    assert args[1] is ctypes.c_int64 and _mismatches({**_hip.SIGNATURES, "pm_linear_bf16": ([args[0], ctypes.c_int] + args[2:], ret)}, protos)


def test_experiment_signatures_and_dec_layer_match_their_header():
    import re

    path = os.path.join(os.path.dirname(_hip.HEADER_PATH), "pm_mi355x_experiments.h")
    bad = _mismatches(_hip.EXPERIMENT_SIGNATURES, _prototypes(path))
    assert not bad, "\n".join(bad)
    body = re.search(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*pm_dec_layer_t\s*;", _strip(open(path).read()), flags=re.S)
    assert body, "pm_dec_layer_t not found"
    fields = []
    for decl in body.group(1).split(";"):
        if not decl.strip():
            continue
        head, *more = [d.strip() for d in decl.split(",")]  # "const void *a, *b" or "float x, y"
        base = head.replace("*", " * ").split()
        star, base_name = "*" in base, base[-1]
        ctype = _ctype(head, True)
        fields.append((base_name, ctype))
        for m in more:
            fields.append((m.replace("*", "").strip(), ctypes.c_void_p if "*" in m else (ctype if not star else _C_TYPES[[w for w in base if w not in ("const", "*")][0]])))
    assert fields == list(_hip.DecLayer._fields_), (fields, _hip.DecLayer._fields_)
