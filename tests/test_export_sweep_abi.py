"""phip_export_sweep without a GPU: the binding's constants and structs match
include/patrolhip.h, and the model the GPU tests hold the sweep to
(tests/_sweep_cases.py) does what the sweep is for: a peer that receives the
model's datagrams ends where it would have ended merging the sender's
non-zero buckets one by one (checked with the oracle alone)."""
import ctypes as C
import os
import re

import numpy as np

from patrol_amd import _lib
from oracle import oracle as O
from tests import _gen
from tests import _sweep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_declared_and_listed():
    assert re.search(r"\bint phip_export_sweep\s*\(", CODE)
    assert "phip_export_sweep" in _lib.EXPORTS
    m = re.search(r"#define PHIP_SWEEP_TILE\s+(\d+)", CODE)
    assert m and int(m.group(1)) == _lib.SWEEP_TILE == SC.TILE == 4096
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", CODE)


def test_cursor_and_stats_layout():
    assert C.sizeof(_lib.phip_sweep_cursor) == 16
    assert [f for f, _ in _lib.phip_sweep_cursor._fields_] == ["slot", "layout"]
    body = re.search(r"typedef struct phip_sweep_cursor \{(.*?)\} phip_sweep_cursor;", CODE, re.S)
    assert re.findall(r"uint64_t (\w+);", body.group(1)) == ["slot", "layout"]
    # the stats fields in the header's order, at the offsets C gives them
    body = re.search(r"typedef struct phip_sweep_stats \{(.*?)\} phip_sweep_stats;", CODE, re.S)
    fields = re.findall(r"(uint64_t|uint32_t) (\w+);", body.group(1))
    assert [f for _, f in fields] == [f for f, _ in _lib.phip_sweep_stats._fields_] == \
        ["n", "bytes", "slots_scanned", "done", "restarted"]
    off = 0
    for typ, name in fields:
        size = 8 if typ == "uint64_t" else 4
        assert off % size == 0
        fld = getattr(_lib.phip_sweep_stats, name)
        assert (fld.offset, fld.size) == (off, size), name
        off += size
    assert C.sizeof(_lib.phip_sweep_stats) == off == 32


def test_count_flag_collides_with_no_other_flag():
    defs = {m.group(1): int(m.group(2), 16)
            for m in re.finditer(r"#define PHIP_([A-Z_0-9]+)\s+(0x[0-9a-fA-F]+)u", CODE)}
    assert defs["SWEEP_COUNT"] == _lib.SWEEP_COUNT == 0x200
    others = {k: v for k, v in defs.items() if k != "SWEEP_COUNT"}
    assert len(others) >= 12
    assert all(v & 0x200 == 0 for v in others.values()), others


def _rows(rng, names):
    a, t, e = _gen.dirty_states(rng, len(names), p_special=0.3)
    return {nm: (int(a[i]), int(t[i]), int(e[i]), _gen.T0) for i, nm in enumerate(names)}


def _seeded(rows):
    o = O.Repo()
    ks = list(rows)
    o.seed(ks, *[[rows[k][j] for k in ks] for j in range(4)])
    return o


def test_model_against_oracle():
    """Receiving the model's datagrams of A into a repo seeded as B equals
    merging A's non-zero buckets into B one by one; no datagram is an incast."""
    rng = np.random.default_rng(3)
    lens = [0, 1, 14, 15, 22, 23, 40, 231]
    names = sorted({(b"%04d" % k).ljust(lens[k % 8], b"n")[:lens[k % 8]] for k in range(400)})
    a_rows = _rows(rng, names)
    zero = b"A-zero-state"
    a_rows[zero] = (1 << 63, 0, 0, _gen.T0)            # -0.0 is zero too (bucket.go:165-170)
    a_rows[b"x" * 232] = (SC.A1, SC.T1, 5, _gen.T0)    # MarshalBinary refuses it
    b_names = names[::3] + [b"only-in-B-%d" % k for k in range(40)]
    b_rows = _rows(rng, b_names)
    model = SC.exported(a_rows)
    nonzero = [k for k, v in a_rows.items() if not SC.is_zero(*v[:3]) and len(k) <= 231]
    assert sorted(model) == sorted(nonzero)
    assert zero not in model and 0 < len(a_rows) - len(model) < len(a_rows)
    now = _gen.T0 + 5
    got = _seeded(b_rows)
    st, _, _, _, stop = got.receive(list(model.values()), now)
    assert stop == len(model) and (st & 0x7F == 1).all()      # every one PHIP_ST_MERGED
    want = _seeded(b_rows)
    for k in nonzero:
        v = a_rows[k]
        want.receive_soa([k], [v[0]], [v[1]], [v[2]], now)
    assert got.dump() == want.dump()
    assert len(got) == len(set(b_rows) | set(nonzero))


def test_model_filter_is_the_eviction_rule():
    rows = SC.filter_rows()
    seen = set()
    for idle_ns in SC.IDLE_NS:
        kept = SC.exported(rows, SC.NOW, idle_ns)
        for k, (a, t, e, c) in rows.items():
            assert (k in kept) == (SC.idle_of(c, e, SC.NOW) < idle_ns), (k, idle_ns)
        seen.add(len(kept))
    assert len(seen) >= 5                                      # the thresholds cut differently
    assert len(SC.exported(rows, SC.NOW, 0)) == len(rows)      # 0: no filter
    assert SC.window(1) == 4096 and SC.window(1024) == 4096 and SC.window(1025) == 8192
