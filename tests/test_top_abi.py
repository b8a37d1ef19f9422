"""Top talkers without a GPU (include/patrolhip.h "Top talkers"): the new
symbols, structs and constants, and phip_top_merge -- through the binding
against tests/_top_cases.py's Python merge, and again as
tools/top_merge_check.cpp, a stand-alone program built with the host file that
holds the merge under ASan and UBSan.  No device calls."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import patrol_amd
from patrol_amd import _lib
from tests import _top_cases as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
STATE_DT = [("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")]


def header():
    return open(os.path.join(ROOT, "include", "patrolhip.h")).read()


def code():
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def test_header_declares_the_entry_points_and_structs():
    src = code()
    assert re.search(r"\bint\s+phip_export_top\s*\(", src)
    assert re.search(r"\bint\s+phip_top_merge\s*\(", src)
    for s in ("phip_top_query", "phip_top_out", "phip_top_stats"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{[^}]*\}\s*%s\s*;" % (s, s), src), s
    assert re.search(r"#define PHIP_TOP_MAX\s+4096\b", src)
    assert _lib.TOP_MAX == TP.TOP_MAX == 4096
    # the section stands behind the throttled sweep
    assert header().index("Throttled sweep:") < header().index("Top talkers:") < \
        header().index("host helpers (no device work)")
    L = _lib.load()
    for name in ("phip_export_top", "phip_top_merge"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert callable(patrol_amd.top_merge)
    for m in ("top", "top_device", "top_count"):
        assert callable(getattr(patrol_amd.GPURepo, m)), m
    assert callable(patrol_amd.GPUGroup.top)


def test_struct_layouts():
    Q, O, S = _lib.phip_top_query, _lib.phip_top_out, _lib.phip_top_stats
    assert C.sizeof(Q) == 48
    assert [(f, getattr(Q, f).offset) for f, _ in Q._fields_] == \
        [("prefix", 0), ("prefix_len", 16), ("metric", 20), ("now", 24), ("idle_ns", 32), ("k", 40),
         ("reserved", 44)]
    assert C.sizeof(O) == 40
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == \
        [("names", 0), ("names_cap", 8), ("offs", 16), ("taken", 24), ("state", 32)]
    assert C.sizeof(S) == 32
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == \
        [("n", 0), ("bytes", 8), ("population", 16), ("passes", 24), ("truncated", 28)]
    # the header's fields, in the header's order
    src = code()
    for s, fields in (("phip_top_query", [f for f, _ in Q._fields_]),
                      ("phip_top_out", [f for f, _ in O._fields_]),
                      ("phip_top_stats", [f for f, _ in S._fields_])):
        body = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}" % s, src).group(1)
        assert re.findall(r"\b(%s)\b\s*[\[,;]" % "|".join(fields), body) == fields, s


def test_abi_version_stays_3():
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", header())
    assert _lib.load().phip_abi_version() == 3


def as_dict(lst):
    st = np.array([e[2] for e in lst], STATE_DT) if lst else np.zeros(0, STATE_DT)
    return dict(names=[e[0] for e in lst], taken=np.array([e[1] for e in lst], np.uint64), state=st)


@pytest.mark.parametrize("case", TP.merge_cases(), ids=lambda c: c[0])
def test_merge_against_the_python_merge(case):
    _, lists, k = case
    want = TP.merge(lists, k)
    d = patrol_amd.top_merge([as_dict(lst) for lst in lists], k)
    assert TP.entries(d) == want and d["n"] == len(want)
    # the total order: taken descending
    assert list(d["taken"]) == sorted(d["taken"], reverse=True)
    # without the state columns
    d2 = patrol_amd.top_merge([dict(names=x["names"], taken=x["taken"])
                               for x in map(as_dict, lists)], k)
    assert d2["state"] is None and TP.entries(d2) == [(nm, t, None) for nm, t, _ in want]


def test_merge_case_properties():
    """What the generated cases hold, from the Python merge alone."""
    cases = {c[0]: c for c in TP.merge_cases()}
    _, lists, k = cases["a name in two lists"]
    got = TP.merge(lists, k)
    assert [e[0] for e in got].count(b"shared") == 1 and got[0][0] == b"shared"
    assert got[0][1] == TP.f2b(300.0) and got[0][2] == [e for e in lists[1] if e[0] == b"shared"][0][2]
    # equal taken: the first list's entry stays
    assert [e for e in got if e[0] == b"same"][0][2] == [e for e in lists[0] if e[0] == b"same"][0][2]
    _, lists, k = cases["ties across lists"]
    got = TP.merge(lists, k)
    assert [e[0] for e in got] == [b"t2-4", b"t2-5", b"t1-0", b"t1-1", b"t1-2"]
    _, lists, k = cases["k above the total"]
    assert len(TP.merge(lists, k)) == sum(map(len, lists))


def test_merge_names_cap_cuts_at_an_entry():
    lst = [(b"abc", TP.f2b(3.0), (1, 2, 3, 4)), (b"defgh", TP.f2b(2.0), (1, 2, 3, 4)),
           (b"i", TP.f2b(1.0), (1, 2, 3, 4))]
    d = patrol_amd.top_merge([as_dict(lst)], 3, names_cap=7)
    assert d["names"] == [b"abc"] and d["n"] == 1      # "defgh" does not fit; nothing behind it is tried
    assert patrol_amd.top_merge([as_dict(lst)], 3, names_cap=9)["names"] == [b"abc", b"defgh", b"i"]


def test_merge_refusals():
    L = _lib.load()
    blob = np.frombuffer(b"ab", np.uint8).copy()
    offs = np.array([0, 1, 2], np.uint64)
    tk = np.array([TP.f2b(2.0), TP.f2b(1.0)], np.uint64)
    lists = (_lib.phip_top_out * 1)(_lib.phip_top_out(blob.ctypes.data, 2, offs.ctypes.data,
                                                      tk.ctypes.data, None))
    ns = (C.c_uint64 * 1)(2)
    on, oo = np.full(8, 0x5A, np.uint8), np.full(4, 0x5A, np.uint64)

    def out(**kw):
        f = dict(names=on.ctypes.data, names_cap=8, offs=oo.ctypes.data, taken=None, state=None)
        f.update(kw)
        return _lib.phip_top_out(f["names"], f["names_cap"], f["offs"], f["taken"], f["state"])
    n = C.c_uint64(99)
    o = out()
    assert L.phip_top_merge(lists, ns, 0, 2, C.byref(o), C.byref(n)) == INVALID
    assert L.phip_top_merge(lists, ns, 1, 0, C.byref(o), C.byref(n)) == INVALID
    assert L.phip_top_merge(lists, ns, 1, 4097, C.byref(o), C.byref(n)) == INVALID
    assert L.phip_top_merge(None, ns, 1, 2, C.byref(o), C.byref(n)) == INVALID
    assert L.phip_top_merge(lists, None, 1, 2, C.byref(o), C.byref(n)) == INVALID
    assert L.phip_top_merge(lists, ns, 1, 2, None, C.byref(n)) == INVALID
    assert L.phip_top_merge(lists, ns, 1, 2, C.byref(o), None) == INVALID
    for bad in (out(names=None), out(offs=None)):
        assert L.phip_top_merge(lists, ns, 1, 2, C.byref(bad), C.byref(n)) == INVALID
    no_taken = (_lib.phip_top_out * 1)(_lib.phip_top_out(blob.ctypes.data, 2, offs.ctypes.data,
                                                         None, None))
    assert L.phip_top_merge(no_taken, ns, 1, 2, C.byref(o), C.byref(n)) == INVALID
    assert n.value == 99 and (on == 0x5A).all() and (oo == 0x5A).all()
    assert L.phip_top_merge(lists, ns, 1, 4096, C.byref(o), C.byref(n)) == 0 and n.value == 2
    assert on[:2].tobytes() == b"ab" and list(oo[:3]) == [0, 1, 2] and (on[2:] == 0x5A).all()
    assert oo[3] == 0x5A
    # the export itself refuses a NULL handle before anything else
    q, st = _lib.phip_top_query(), _lib.phip_top_stats()
    q.k = 1
    assert L.phip_export_top(None, C.byref(q), None, C.byref(st), _lib.SWEEP_COUNT) == INVALID


def write_cases(path):
    def row(nm, t, s):
        return "%s %d %d %d %d\n" % (nm.hex() or "-", t, s[0], s[2], s[3])
    cases = TP.merge_cases()
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for _, lists, k in cases:
            f.write("%d %d\n" % (k, len(lists)))
            for lst in lists:
                f.write("%d\n" % len(lst))
                f.writelines(row(*e) for e in lst)
            want = TP.merge(lists, k)
            f.write("%d\n" % len(want))
            f.writelines(row(*e) for e in want)
    return len(cases)


def test_merge_check_program_under_the_host_sanitizers(tmp_path):
    """tools/top_merge_check.cpp with patrol_amd/csrc/phip_top.cpp, built for
    the CPU with -fsanitize=address,undefined and run over the same cases."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "top_merge_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tools", "top_merge_check.cpp"),
                    os.path.join(ROOT, "patrol_amd", "csrc", "phip_top.cpp")], check=True)
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "%d cases" % n in r.stdout and "clean" in r.stdout, r.stdout
