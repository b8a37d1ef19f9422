"""The throttled sweep without a GPU (include/patrolhip.h "Throttled sweep"):
the new symbols, structs and constants, the recipe's mix, and
phip_throttle_match -- the host build of the function the sweep's kernels
call -- against tests/_throttled_cases.py's restatement of the match rule.
No device calls."""
import ctypes as C
import os
import re

import patrol_amd
from patrol_amd import _lib
from tests import _throttled_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def header():
    return open(os.path.join(ROOT, "include", "patrolhip.h")).read()


def test_header_declares_the_entry_points_and_structs():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+phip_export_throttled\s*\(", src)
    assert re.search(r"\bint\s+phip_throttle_match\s*\(", src)
    assert re.search(r"typedef\s+struct\s+phip_throttle_rule\s*\{[^}]*\}\s*phip_throttle_rule\s*;", src)
    assert re.search(r"typedef\s+struct\s+phip_throttled_out\s*\{[^}]*\}\s*phip_throttled_out\s*;", src)
    assert re.search(r"#define PHIP_THROTTLE_MAX_RULES\s+8\b", src)
    assert re.search(r"#define PHIP_THROTTLE_MAX_PREFIX\s+16\b", src)
    assert (_lib.THROTTLE_MAX_RULES, _lib.THROTTLE_MAX_PREFIX) == (8, 16)
    assert int(re.search(r"#define PHIP_MAX_NAME_LEN\s+(\d+)", src).group(1)) == _lib.MAX_NAME_LEN == \
        TC.MAX_NAME
    L = _lib.load()
    for name in ("phip_export_throttled", "phip_throttle_match"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # the sweep is no longer listed as missing
    assert '"currently throttled" sweep' not in header()


def test_struct_layouts():
    R, O = _lib.phip_throttle_rule, _lib.phip_throttled_out
    assert C.sizeof(R) == 48
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == \
        [("prefix", 0), ("prefix_len", 16), ("reserved", 20), ("freq", 24), ("per", 32), ("count", 40)]
    assert C.sizeof(O) == 56
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == \
        [("names", 0), ("names_cap", 8), ("offs", 16), ("max_entries", 24), ("reserved", 28),
         ("retry_at", 32), ("remaining", 40), ("rule", 48)]
    # the header's fields, in the header's order
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+phip_throttle_rule\s*\{([^}]*)\}", src).group(1)
    assert re.findall(r"\b(prefix|prefix_len|reserved|freq|per|count)\b\s*[\[,;]", body) == \
        ["prefix", "prefix_len", "reserved", "freq", "per", "count"]


def test_abi_version_stays_3():
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", header())
    assert _lib.load().phip_abi_version() == 3


def test_recipe_mix():
    """The conditions the GPU tests rest on, from the reference alone."""
    tab = TC.table_case(7)
    assert len(tab["rows"]) == 600 and sum(len(n) == 0 for n in tab["names"]) == 1
    for now in (TC.NOW, TC.NOW_EARLY):
        print(now - TC.T0, TC.check_mix(tab["rows"], TC.RULES, now))
    lens = {len(n) for n in tab["names"]}
    assert all(any(lo <= x <= hi for x in lens) for lo, hi in TC.CLASSES)


def test_match_agrees_with_the_restatement_over_the_recipe():
    tab = TC.table_case(7)
    hits = [patrol_amd.throttle_match(TC.RULES, nm) for nm in tab["names"]]
    assert hits == [TC.match(TC.RULES, nm) for nm in tab["names"]]
    assert set(hits) == {-1, 0, 1, 2, 3}
    # the head that differs from rule 0's prefix in its 16th byte falls to rule 1
    assert patrol_amd.throttle_match(TC.RULES, b"org:acme:012345_" + b"z" * 20) == 1
    assert patrol_amd.throttle_match(TC.RULES, b"org:acme:0123456" + b"z" * 200) == 0


def test_match_edges():
    m = patrol_amd.throttle_match
    p16 = b"0123456789abcdef"
    cases = [
        # prefix_len 0 matches every name, the empty one too
        ([(b"", 1, 1, 1)], b"", 0), ([(b"", 1, 1, 1)], b"anything", 0),
        ([(b"", 1, 1, 1)], b"x" * 231, 0),
        # prefix_len 16
        ([(p16, 1, 1, 1)], p16, 0), ([(p16, 1, 1, 1)], p16 + b"tail", 0),
        ([(p16, 1, 1, 1)], p16[:15] + b"F", -1), ([(p16, 1, 1, 1)], p16 + b"x" * 200, 0),
        ([(p16, 1, 1, 1)], b"1" + p16[1:] + b"x" * 200, -1),
        # a name equal to the prefix, and one byte short of it
        ([(b"u:", 1, 1, 1)], b"u:", 0), ([(b"u:", 1, 1, 1)], b"u", -1),
        ([(p16, 1, 1, 1)], p16[:15], -1), ([(b"u:", 1, 1, 1)], b"", -1),
        # prefixes that end at a word boundary of the record's name bytes
        ([(p16[:8], 1, 1, 1)], p16[:8], 0), ([(p16[:8], 1, 1, 1)], p16[:7] + b"x", -1),
        ([(p16[:9], 1, 1, 1)], p16[:8] + b"x", -1), ([(p16[:9], 1, 1, 1)], p16[:9], 0),
        # rule order decides between two rules that both match
        ([(b"org:", 1, 1, 1), (b"org:acme", 2, 2, 2)], b"org:acme:1", 0),
        ([(b"org:acme", 2, 2, 2), (b"org:", 1, 1, 1)], b"org:acme:1", 0),
        ([(b"org:acme", 2, 2, 2), (b"org:", 1, 1, 1)], b"org:other", 1),
        ([(b"zz", 1, 1, 1), (b"", 2, 2, 2), (b"a", 3, 3, 3)], b"a", 1),
        # high bytes and NULs are bytes like any other
        ([(b"\xff\x00\x80", 1, 1, 1)], b"\xff\x00\x80\x00", 0),
        ([(b"\xff\x00\x80", 1, 1, 1)], b"\xff\x00\x81", -1),
        ([(b"a\x00", 1, 1, 1)], b"a", -1),
    ]
    for rules, name, want in cases:
        assert m(rules, name) == want == TC.match(rules, name), (rules, name)
    # eight rules, the last one hit
    eight = [(b"r%d" % i, 1, 1, 1) for i in range(8)]
    assert m(eight, b"r7x") == 7 and m(eight, b"r8") == -1


def raw_match(rules, n_rules, name, out):
    return _lib.load().phip_throttle_match(rules, n_rules, name, len(name), out)


def test_bytes_past_prefix_len_are_ignored():
    rule = (_lib.phip_throttle_rule * 1)()
    rule[0].prefix[:16] = list(b"u:GARBAGEGARBAGE")
    rule[0].prefix_len = 2
    out = C.c_int32(-2)
    assert raw_match(rule, 1, b"u:alice", C.byref(out)) == 0 and out.value == 0
    assert raw_match(rule, 1, b"u:", C.byref(out)) == 0 and out.value == 0
    assert raw_match(rule, 1, b"u;GARBAGE", C.byref(out)) == 0 and out.value == -1
    rule[0].prefix_len = 0
    assert raw_match(rule, 1, b"", C.byref(out)) == 0 and out.value == 0


def test_match_refusals():
    rules = (_lib.phip_throttle_rule * 9)()
    for i in range(9):
        rules[i].prefix[0] = ord("a")
        rules[i].prefix_len = 1
    out = C.c_int32(-2)
    assert raw_match(rules, 0, b"a", C.byref(out)) == INVALID
    assert raw_match(rules, 9, b"a", C.byref(out)) == INVALID
    assert raw_match(rules, 8, b"a", None) == INVALID
    assert raw_match(None, 1, b"a", C.byref(out)) == INVALID
    rules[3].prefix_len = 17
    assert raw_match(rules, 8, b"a", C.byref(out)) == INVALID
    assert raw_match(rules, 3, b"a", C.byref(out)) == 0     # (rule 3 is not among the first three)
    assert out.value == 0
    # the export itself refuses a NULL handle before anything else
    cur, st = _lib.phip_sweep_cursor(), _lib.phip_sweep_stats()
    assert _lib.load().phip_export_throttled(None, C.byref(cur), rules, 1, 0, 0, None, C.byref(st),
                                             _lib.SWEEP_COUNT) == INVALID
