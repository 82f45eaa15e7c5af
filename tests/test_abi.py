"""CPU-side checks of the drop-in boundary: the shared library loads without a GPU, exports every
symbol include/deepaco_hip.h declares, the ctypes table covers them all, and argument validation
answers with error codes (no compute is launched here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from deepaco_amd import _lib
import oracle


def header_symbols():
    text = open(os.path.join(ROOT, "include", "deepaco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(daco_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_something():
    syms = header_symbols()
    assert "daco_tsp_sample" in syms and "daco_pheromone_update" in syms and len(syms) >= 9


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    for s in header_symbols():
        assert hasattr(L, s), f"{s} declared in include/deepaco_hip.h but not exported"


_C_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
              "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64}


def header_signatures():
    """name -> (restype, argtypes) of every prototype in include/deepaco_hip.h, in ctypes: any pointer argument a c_void_p,
    a `const char *` return a c_char_p, the scalar types by name."""
    text = open(os.path.join(ROOT, "include", "deepaco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    sigs = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(daco_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        res = C.c_char_p if ret == "const char *" else _C_SCALARS[ret]
        argtypes = []
        for a in ([] if args.strip() in ("", "void") else args.split(",")):
            words = [w for w in a.replace("*", " * ").split() if w != "const"]
            argtypes.append(C.c_void_p if "*" in words else _C_SCALARS[words[0]])
        assert name not in sigs, f"{name} declared twice"
        sigs[name] = (res, argtypes)
    return sigs


def signature_mismatches(table, header):
    """One line per function of `header` whose row of `table` differs: the function and the first differing position."""
    out = []
    for name, (res, args) in sorted(header.items()):
        if name not in table:
            out.append(f"{name}: no row")
            continue
        tres, targs = table[name]
        if tres is not res:
            out.append(f"{name}: returns {res.__name__} in the header, {tres.__name__} in the table")
            continue
        for i, (h, t) in enumerate(zip(args, targs)):
            if h is not t:
                out.append(f"{name}: argument {i} is {h.__name__} in the header, {t.__name__} in the table")
                break
        else:
            if len(args) != len(targs):
                out.append(f"{name}: {len(args)} arguments in the header, {len(targs)} in the table")
    return out


def test_ctypes_table_matches_header():
    assert sorted(_lib.SIGNATURES) == header_symbols()
    header = header_signatures()
    assert sorted(header) == header_symbols()                        # (the prototype parser misses no declaration)
    assert signature_mismatches(_lib.SIGNATURES, header) == []
    # the comparison can fail: one row with a float where the header says double, one with its last argument dropped
    res, args = _lib.SIGNATURES["daco_rcpsp_sample"]
    at = args.index(C.c_double)
    wrong = dict(_lib.SIGNATURES, daco_rcpsp_sample=(res, args[:at] + [C.c_float] + args[at + 1:]),
                 daco_tour_costs=(_lib.SIGNATURES["daco_tour_costs"][0], _lib.SIGNATURES["daco_tour_costs"][1][:-1]))
    assert signature_mismatches(wrong, header) == [
        f"daco_rcpsp_sample: argument {at} is c_double in the header, c_float in the table",
        "daco_tour_costs: 10 arguments in the header, 9 in the table"]


def test_version_and_layout_helpers_agree_with_oracle():
    L = _lib.lib()
    assert L.daco_version() >= 123
    for n in (2, 5, 63, 64, 65, 100, 128, 129, 255, 256, 257, 500, 1000, 4096):
        assert L.daco_vec_for_n(n) == oracle.vec_for_n(n)
        assert L.daco_ld_for_n(n) == oracle.ld_for_n(n)
        assert L.daco_ld_for_n(n) >= n and L.daco_ld_for_n(n) % (64 * L.daco_vec_for_n(n)) == 0


def test_bad_arguments_return_error_codes():
    L = _lib.lib()
    assert L.daco_tour_costs(None, 0, 0, 0, 0, None, 0, None, 0, None) == -1
    assert b"bad argument" in L.daco_last_error()
    # n above the register plan of the sampler -> DACO_E_TOOLARGE before anything is launched
    rc = L.daco_tsp_sample(None, 1, 5000, 4, 1, 0, 1, 0, 1.0, 1.0, 2, 1, None, -1, None, 0, 0, None, 0, 0, 1, None, None,
                           None, None, 0, None, None, 1, 1 << 40, None, None)
    assert rc == -2 and b"DACO_MAX_NODES" in L.daco_last_error()
    # workspace too small
    rc = L.daco_tsp_sample(None, 1, 100, 4, 1, 0, 1, 0, 1.0, 1.0, 2, 1, None, -1, None, 0, 0, None, 0, 0, 1, None, None,
                           None, None, 0, None, None, 1, 16, None, None)
    assert rc == -4
    assert L.daco_tsp_sample_workspace_bytes(64, 500, _lib.SCAN) == 64 * 500 * 512 * 4
    assert L.daco_tsp_sample_workspace_bytes(64, 500, _lib.RACE_PHILOX) == 2 * 64 * 500 * 512 * 4


def test_product_has_no_cpu_path():
    import torch
    from deepaco_amd import engine
    from deepaco_amd.tsp.aco import ACO
    d = torch.rand(5, 5)
    if torch.cuda.is_available():          # host tensors are staged to the HIP device, never computed on the CPU
        assert ACO(d, n_ants=4).distances.is_cuda
    else:
        with pytest.raises(_lib.DacoError):
            ACO(d, n_ants=4)
    with pytest.raises(_lib.DacoError):
        engine.tsp_sample(d, d, 4)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "deepaco_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
                assert "daco_oracle" not in src or f.endswith(".h") and "restated in" in src, f


def test_two_opt_candidate_entry_points_validate_arguments():
    import torch
    from deepaco_amd import engine
    L = _lib.lib()
    n = 500
    al = lambda x: (x + 255) & ~255
    assert L.daco_two_opt_tables_bytes(3, n) == 3 * (256 + al(8 * n * n) + al(2 * n * n))
    assert L.daco_two_opt_tables_bytes(0, n) == 0
    assert L.daco_two_opt_prepare(None, 0, n, None, 0, None, 0) == -1
    assert L.daco_two_opt_prepare(None, 1, 2000, 1, 0, 1, 1 << 40) == -2 and b"1024" in L.daco_last_error()
    assert L.daco_two_opt_prepare(None, 1, n, 1, 0, 1, 16) == -4                      # tables buffer too small
    assert L.daco_two_opt_nbr(None, 1, 1, 2000, 1, 0, 1, 1, 1, 10, None) == -2
    assert L.daco_two_opt_nbr(None, 1, 1, n, 1, 0, None, None, 1, 10, None) == -1
    assert L.daco_two_opt_auto(None, 1, 1, n, 1, None, 0, 1, 1, 1, 10, None) == -1    # sweeps is required (hand-over state)
    # above the table kernels' size the host falls back to the dense kernel (no tables)
    assert engine.two_opt_tables(torch.zeros(1, 1025, 1025)) is None


# knobs that no test or tool sets, each with the reason it is read all the same
KNOBS_WITHOUT_A_USER = {
    "DACO_LIB_PATH": "selects the build: how two builds of the library are compared in one checkout",
}


def _files(top, suffixes):
    for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
        for f in files:
            if f.endswith(suffixes):
                yield os.path.join(dirpath, f)


def test_every_knob_is_documented_and_used():
    """Every DACO_* environment variable the library (getenv) or the package (os.environ) reads is a row of the knob table of
    DESIGN.md section 9 and every row is read somewhere; and each is named by a test or a tool, so that no kernel is left that only
    a variable in somebody's shell can select."""
    read = set()
    for f in _files(os.path.join("deepaco_amd", "csrc"), (".hip", ".h", ".cpp")):
        read |= set(re.findall(r'getenv\(\s*"(DACO_[A-Z0-9_]+)"', open(f).read()))
    for f in _files("deepaco_amd", (".py",)):
        read |= set(re.findall(r'os\.environ[^\n]*?["\'](DACO_[A-Z0-9_]+)["\']', open(f).read()))
    assert "DACO_SCAN_LAYOUT" in read and "DACO_LIB_PATH" in read          # (the collection itself works)
    rows = [line.split("|")[1] for line in open(os.path.join(ROOT, "DESIGN.md")) if line.startswith("| `DACO_")]
    table = set(re.findall(r"DACO_[A-Z0-9_]+", " ".join(rows)))
    assert read - table == set(), "read by the code, missing from DESIGN.md's knob table"
    assert table - read == set(), "in DESIGN.md's knob table, read by nothing"
    me = os.path.abspath(__file__)
    users = "".join(open(f).read() for top in ("tests", "tools") for f in _files(top, (".py", ".sh", ".hip", ".cpp")) if os.path.abspath(f) != me)
    orphans = {k for k in read if not re.search(r"\b%s\b" % k, users)}
    assert orphans == set(KNOBS_WITHOUT_A_USER), "knobs that no test and no tool sets"
