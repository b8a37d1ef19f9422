"""Windowed top talkers without a GPU (include/patrolhip.h "Windowed top
talkers"): the new symbol, struct, constants and binding, and what the model
of tests/_usage_cases.py holds -- the activity recipe's classes and the edge
table's expected keys -- so that tests/test_usage.py cannot pass by checking
nothing.  No device calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import patrol_amd
from patrol_amd import _lib
from tests import _top_cases as TP
from tests import _usage_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def header():
    return open(os.path.join(ROOT, "include", "patrolhip.h")).read()


def code():
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def test_symbol_exported_and_bound():
    src = code()
    assert re.search(r"\bint\s+phip_usage_mark\s*\(\s*phip_handle\s*\*\s*h\s*,\s*phip_usage_stats\s*\*"
                     r"\s*st\s*,\s*uint32_t\s+flags\s*\)", src)
    L = _lib.load()
    assert "phip_usage_mark" in _lib.EXPORTS and hasattr(L, "phip_usage_mark")
    assert L.phip_usage_mark.argtypes[1] == C.POINTER(_lib.phip_usage_stats)
    # a NULL handle is refused before anything else
    st = _lib.phip_usage_stats(7, 7)
    assert L.phip_usage_mark(None, C.byref(st), 0) == INVALID and (st.buckets, st.active) == (7, 7)
    assert callable(patrol_amd.GPURepo.usage_mark) and callable(patrol_amd.GPUGroup.usage_mark)
    for fn, params in ((patrol_amd.GPURepo.__init__, ["track_usage"]),
                       (patrol_amd.GPURepo.top, ["metric", "mark"]),
                       (patrol_amd.GPURepo.top_device, ["metric", "mark"]),
                       (patrol_amd.GPURepo.top_count, ["metric"]),
                       (patrol_amd.GPUGroup.open_all, ["track_usage"]),
                       (patrol_amd.GPUGroup.top, ["metric", "mark"])):
        sig = inspect.signature(fn).parameters
        for p in params:
            assert p in sig and sig[p].default in (0, False), (fn, p)


def test_constants_in_the_header_and_the_binding():
    src = code()
    assert re.search(r"#define PHIP_CFG_TRACK_USAGE\s+0x40u\b", src) and _lib.CFG_TRACK_USAGE == 0x40
    assert re.search(r"#define PHIP_TOP_SINCE_MARK\s+1\b", src) and _lib.TOP_SINCE_MARK == 1
    assert re.search(r"#define PHIP_TOP_MARK\s+0x400u\b", src) and _lib.TOP_MARK == 0x400
    # the config flags are distinct bits
    cfg = [int(v, 16) for v in re.findall(r"#define PHIP_CFG_\w+\s+(0x[0-9a-fA-F]+)u", src)]
    assert len(cfg) == 7 and sum(cfg) == 0x7F and all(v & (v - 1) == 0 for v in cfg)
    # the section stands with the top talkers, and states the column's cost by the flag
    h = header()
    assert h.index("Top talkers:") < h.index("Windowed top talkers:") < h.index("#define PHIP_TOP_MAX")
    flag_doc = h[h.index("#define PHIP_CFG_TRACK_USAGE"):h.index("typedef struct phip_config")]
    assert "8 bytes a slot" in flag_doc and "256 MB" in flag_doc
    assert "a caller who wants\n * a rate diffs two lists" not in h


def test_usage_stats_layout():
    S = _lib.phip_usage_stats
    assert C.sizeof(S) == 16
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("buckets", 0), ("active", 8)]
    body = re.search(r"typedef\s+struct\s+phip_usage_stats\s*\{([^}]*)\}\s*phip_usage_stats\s*;",
                     code()).group(1)
    assert re.findall(r"\b(buckets|active)\b\s*;", body) == ["buckets", "active"]
    # no struct of the top call changed
    assert (C.sizeof(_lib.phip_top_query), C.sizeof(_lib.phip_top_out), C.sizeof(_lib.phip_top_stats),
            C.sizeof(_lib.phip_config)) == (48, 40, 32, 40)


def test_abi_version_stays_3():
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", header())
    assert _lib.load().phip_abi_version() == 3


def test_top_mark_clashes_with_no_flag_of_the_call():
    """phip_export_top takes PHIP_DEVICE_PTRS, PHIP_SWEEP_COUNT and PHIP_TOP_MARK."""
    src = code()
    flags = {n: int(v, 16) for n, v in re.findall(r"#define (PHIP_(?:DEVICE_PTRS|SWEEP_COUNT|TOP_MARK))"
                                                  r"\s+(0x[0-9a-fA-F]+)u", src)}
    assert flags == {"PHIP_DEVICE_PTRS": 0x1, "PHIP_SWEEP_COUNT": 0x200, "PHIP_TOP_MARK": 0x400}
    assert (_lib.DEVICE_PTRS, _lib.SWEEP_COUNT, _lib.TOP_MARK) == (0x1, 0x200, 0x400)
    # nor with any other call flag the header defines (the config and evict flags are other words)
    others = {n: int(v, 16) for n, v in re.findall(r"#define (PHIP_\w+)\s+(0x[0-9a-fA-F]+)u", src)
              if n != "PHIP_TOP_MARK"}
    assert others and not any(v & 0x400 for v in others.values()), others


# ------------------------------------------------------------ the recipe ----
def test_recipe_meets_its_class_counts():
    names, cols, rows, steps = UC.plan()
    assert len(names) == 600 and len(rows) == 600
    now_rows = UC.run_model(rows, steps)
    ref = UC.reference(rows, now_rows)
    calls = [c for c, _ in steps]
    assert {"receive", "take", "mixed"} <= set(calls)
    raised = {nm for nm in rows if now_rows[nm][1] != rows[nm][1]}
    by_receive = set(steps[0][1][0]) & raised
    by_take = (set(steps[1][1][0]) | set(steps[3][1][1][:40])) & raised
    new = set(now_rows) - set(rows)
    assert len(by_receive) >= 150 and len(by_take) >= 50 and not by_receive & by_take
    assert len(new) >= 40
    assert sum(nm.startswith(b"usage-new-take") for nm in new) >= 20
    assert sum(nm.startswith(b"org:usage-new-recv") for nm in new) >= 20
    untouched = [nm for nm in rows if now_rows[nm] == rows[nm]]
    assert len(untouched) >= 200 and not any(nm in ref for nm in untouched)
    # every raised or new bucket ranks (all names are at most 231 bytes), nothing else does
    assert set(ref) == raised | new and len(ref) == UC.active(rows, now_rows)
    # equal differences over different totals
    groups = UC.tie_groups(ref)
    wide = [v for v in groups.values() if len(set(now_rows[nm][1] for nm in v)) == len(v)]
    assert len(groups) >= 10 and len(wide) >= 10
    assert max(map(len, groups.values())) >= 50
    # a new bucket's difference is its whole taken; an old one's is not
    for nm in new:
        assert ref[nm] == now_rows[nm][1]
    assert all(ref[nm] != now_rows[nm][1] for nm in raised)
    # the order by difference is not the order by total: metric 0's list is another list
    top0 = sorted(TP.reference(now_rows), key=lambda nm: -now_rows[nm][1])[:64]
    top1 = sorted(ref, key=lambda nm: -ref[nm])[:64]
    assert set(top0) != set(top1)
    # the filters of the GPU test cut the population without emptying it
    pre = UC.reference(rows, now_rows, b"org:")
    assert 20 <= len(pre) < len(ref)
    idle = UC.reference(rows, now_rows, b"", UC.TAKE_NOW, 4500 * UC.SEC)
    assert 20 <= len(idle) < len(ref)
    # before any mark the model is metric 0's
    assert UC.reference({}, rows) == TP.reference(rows)


def test_edge_table_expected_keys():
    f2b, INF = UC.f2b, UC.INF
    for s in TP.SHIFTS:
        exp = UC.edge_expected(s)
        keys = dict(exp)
        assert len(set(keys.values())) == len(exp), "the edge list must not depend on slots"
        assert exp[0] == (b"inf-finite", INF) and exp[-1] == (b"denormal", 1)
        assert not any(nm.startswith(b"never") for nm in keys) and len(exp) == 11 + 8
        assert keys[b"round-a"] == f2b(2.0 ** 53)           # 2^53 + 1 ties to even
        assert keys[b"round-b"] == f2b(2.0 ** 53 + 4)       # 2^53 + 5 ties to even
        assert keys[b"round-c"] == f2b(np.float64(0.3) - np.float64(0.1)) != f2b(0.2)
        assert keys[b"round-d"] == f2b(np.float64(1e10 + 0.7) - np.float64(1.0 / 3.0))
        assert keys[b"ulp-1"] == f2b(2.0 ** -52) and keys[b"ulp-2"] == f2b(2.0 ** -33)
        assert keys[b"ulp-3"] == f2b(np.spacing(np.float64(1e-300)))
        assert keys[b"ulp-4"] == f2b(np.spacing(np.float64(1.5e300)))
        assert keys[b"negzero-base"] == f2b(3.0)
        for i in range(1, 9):
            assert keys[b"fam-%d" % i] == TP.BASE + (i << s)
        fam = [nm for nm, _ in exp if nm.startswith(b"fam")]
        assert fam == [b"fam-%d" % i for i in range(8, 0, -1)]
    # the cases that never rank, one by one
    assert UC.delta_bits(INF, INF) > INF                     # Inf - Inf: a NaN
    assert UC.delta_bits(UC.NAN, f2b(5.0)) > INF
    assert UC.delta_bits(f2b(42.0), f2b(42.0)) == 0
    assert UC.delta_bits(UC.SIGN, UC.SIGN) == 0              # -0.0 - -0.0 = +0.0
    assert UC.delta_bits(f2b(1.0), f2b(2.0)) == f2b(-1.0) > INF
