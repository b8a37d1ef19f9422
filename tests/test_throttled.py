"""phip_export_throttled on the GPU (include/patrolhip.h "Throttled sweep"),
through the binding.

What a sweep must report is tests/_throttled_cases.py's expected(): the match
rule restated in Python over the table's dump, and the oracle's pure Take on a
copy of each state (tests/_peek_cases.py) -- never the library.  remaining is
compared on bits, retry_at by its definition, and both again bit for bit with
phip_peek (the kernel that was there before) and phip_peek_eval.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import _peek_cases as PC  # noqa: E402
from tests import _throttled_cases as TC  # noqa: E402

T0, SEC = TC.T0, TC.SEC
RULES = TC.RULES
FILL = 0x5A
FILL64 = 0x5A5A5A5A5A5A5A5A
INVALID = -1


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def gpu_dump(repo):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}
    assert len(repo) == len(d), (len(repo), len(d))
    return d


def seeded(pa, tab, **kw):
    kw.setdefault("log2_slots", 10)
    kw.setdefault("hash_seed", 11)
    g = pa.GPURepo(**kw)
    g.seed(tab["names"], *tab["cols"])
    assert len(g) == len(tab["names"])
    return g


@pytest.fixture(scope="module")
def small(pa):
    """The recipe's 600 buckets in 2^10 slots under 3-bit tags (forced
    collisions), the mix's conditions asserted from the reference first.
    Shared, never changed."""
    tab = TC.table_case(7)
    for now in (TC.NOW, TC.NOW_EARLY):
        print("mix at T0%+d s: %s" % ((now - T0) // SEC, TC.check_mix(tab["rows"], RULES, now)))
    g = seeded(pa, tab, debug_tag_bits=3)
    assert g.capacity == 1024
    rows = gpu_dump(g)
    assert rows == tab["rows"]
    yield g, rows
    g.close()


def check_call(d, max_entries, names_cap):
    assert d["n"] == len(d["names"]) == len(d["retry_at"]) == len(d["remaining"]) == len(d["rule"])
    assert d["n"] <= max_entries and d["bytes"] == sum(map(len, d["names"])) <= names_cap
    assert d["slots_scanned"] <= TC.window(max_entries)


def entries(d):
    return [(nm, int(d["rule"][i]), int(d["remaining"][i]), int(d["retry_at"][i]))
            for i, nm in enumerate(d["names"])]


def sweep_all(g, rules, now, min_wait, max_entries, names_cap=None, cursor=None):
    """Loop to done -> (entries in order, the dict of every call)."""
    cap = names_cap if names_cap is not None else 231 * max_entries
    got, calls = [], []
    while True:
        d = g.export_throttled(rules, now, min_wait, cursor, max_entries, names_cap)
        check_call(d, max_entries, cap)
        cursor = d["cursor"]
        got += entries(d)
        calls.append(d)
        assert len(calls) <= 20000
        if d["done"]:
            return got, calls


def assert_exact(got, exp, rules, now):
    names = [e[0] for e in got]
    assert len(names) == len(set(names)), "a bucket was reported twice"
    assert set(names) == set(exp), (sorted(set(exp) - set(names))[:5], sorted(set(names) - set(exp))[:5])
    for nm, rule, rem, at in got:
        TC.check_entry(exp, rules, now, nm, rule, rem, at)


# ------------------------------------------------------------- 1. parity ----
@pytest.mark.parametrize("now", [TC.NOW, TC.NOW_EARLY])
@pytest.mark.parametrize("min_wait", [0, TC.MIN_WAIT])
def test_parity(pa, small, now, min_wait):
    g, rows = small
    exp, tally = TC.expected(rows, RULES, now, min_wait)
    assert len(exp) >= 60 and (min_wait == 0 or tally["held_out"] >= 10)
    d = g.export_throttled(RULES, now, min_wait, None, max_entries=1024)
    check_call(d, 1024, 231 * 1024)
    assert (d["done"], d["restarted"], d["slots_scanned"], d["cursor"][0]) == (1, 0, 1024, 1024)
    got = entries(d)
    assert_exact(got, exp, RULES, now)
    # bit for bit what phip_peek and phip_peek_eval say of the same query
    names = [e[0] for e in got]
    q = [RULES[e[1]] for e in got]
    pk = g.peek(names, [now] * len(got), [r[1] for r in q], [r[2] for r in q], [r[3] for r in q])
    for i, (nm, rule, rem, at) in enumerate(got):
        assert int(pk["status"][i]) == PC.DENIED, nm
        assert (int(pk["remaining"][i]), int(pk["retry_at"][i])) == (rem, at), (nm, rule)
        ev = pa.peek_eval(rows[nm], now, *RULES[rule][1:])
        assert ev[0] == PC.DENIED and (ev[1], ev[3]) == (rem, at), (nm, ev)
        if min_wait:   # the predicate, restated through the formula it implies
            assert at == PC.NEVER or at > TC.later_of(now, min_wait), (nm, at)
    # count mode: the same totals, the cursor untouched
    cnt = g.throttled_count(RULES, now, min_wait)
    assert (cnt["n"], cnt["bytes"], cnt["slots_scanned"]) == (d["n"], d["bytes"], 1024)
    # slot order: the same sequence again, and the export sweep's order
    assert entries(g.export_throttled(RULES, now, min_wait, None, max_entries=1024)) == got
    order = {dg[25:]: i for i, dg in enumerate(g.export_sweep(None, max_msgs=1024)[0])}
    pos = [order[nm] for nm in names if nm in order]
    assert len(pos) >= len(names) // 2 and pos == sorted(pos)
    # the generator, in small calls
    assert [e for c in g.throttled(RULES, now, min_wait, max_entries=50) for e in entries(c)] == got


def test_empty_name_and_catch_all_rule(pa):
    """The empty name qualifies with a size of 0: first, last and only entry,
    and under a cut (its qualify bit is its own, not `size != 0`)."""
    g = pa.GPURepo(log2_slots=10, hash_seed=3)
    drained = (PC.G.f2b(3.0), PC.G.f2b(3.0), 0, T0)    # no tokens left
    names = [b"", b"a", b"bb"]
    g.seed(names, *[[drained[j]] * 3 for j in range(4)])
    rules = [(b"", 3, SEC, 1)]
    exp, _ = TC.expected(gpu_dump(g), rules, T0)
    assert set(exp) == set(names)
    one = g.export_throttled(rules, T0, max_entries=8)
    assert sorted(one["names"]) == sorted(names) and one["bytes"] == 3 and one["done"] == 1
    assert_exact(entries(one), exp, rules, T0)
    cnt = g.throttled_count(rules, T0)
    assert (cnt["n"], cnt["bytes"]) == (3, 3)
    got, calls = sweep_all(g, rules, T0, 0, 1)
    assert got == entries(one) and [c["n"] for c in calls if c["n"]] == [1, 1, 1]
    g.close()
    # alone in the table
    g = pa.GPURepo(log2_slots=10, hash_seed=3)
    g.seed([b""], *[[drained[j]] for j in range(4)])
    d = g.export_throttled(rules, T0, max_entries=1)
    assert (d["names"], d["n"], d["bytes"], d["done"]) == ([b""], 1, 0, 1)
    assert g.throttled_count(rules, T0)["n"] == 1
    g.close()


# -------------------------------------------------------- 2. device form ----
def device_call(g, rules, now, min_wait, max_entries, names_cap, cols=("retry_at", "remaining", "rule")):
    import torch
    dev = torch.device("cuda", 0)
    names = torch.full((names_cap,), FILL, dtype=torch.uint8, device=dev)
    offs = torch.full((max_entries + 1,), FILL64, dtype=torch.int64, device=dev)
    kw = {}
    for c in cols:
        kw[c] = torch.full((max_entries,), FILL if c == "rule" else FILL64,
                           dtype=torch.uint8 if c == "rule" else torch.int64, device=dev)
    n, cur, st = g.export_throttled_device(rules, now, names, offs, None, max_entries, min_wait, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in kw.items()}
    return n, cur, st, names.cpu().numpy(), offs.cpu().numpy(), out


@pytest.mark.parametrize("drop", [None, "retry_at", "remaining", "rule"])
def test_device_form(pa, small, drop):
    g, rows = small
    host = g.export_throttled(RULES, TC.NOW, 0, None, max_entries=1024)
    cols = tuple(c for c in ("retry_at", "remaining", "rule") if c != drop)
    M, CAP = 1024, 231 * 300
    n, cur, st, names, offs, out = device_call(g, RULES, TC.NOW, 0, M, CAP, cols)
    assert (n, st["bytes"], st["done"], st["restarted"], cur) == \
        (host["n"], host["bytes"], 1, 0, host["cursor"])
    assert offs[0] == 0 and int(offs[n]) == st["bytes"]
    raw = names.tobytes()
    assert [raw[int(offs[i]):int(offs[i + 1])] for i in range(n)] == host["names"]
    for c in cols:
        assert np.array_equal(out[c][:n].view(host[c].dtype), host[c]), c
        # nothing past entry n of a column
        assert (out[c][n:] == (FILL if c == "rule" else FILL64)).all(), c
    # nothing past offs[n]
    assert (names[st["bytes"]:] == FILL).all() and (offs[n + 1:] == FILL64).all()


# ---------------------------------------------------- 3. windows and cuts ----
@pytest.fixture(scope="module")
def four_tiles(pa):
    tab = TC.table_case(5, n=3000)
    g = seeded(pa, tab, log2_slots=14)
    assert g.capacity == 1 << 14
    rows = gpu_dump(g)
    exp, _ = TC.expected(rows, RULES, TC.NOW)
    assert len(exp) >= 300
    one = g.export_throttled(RULES, TC.NOW, 0, None, max_entries=4096)
    yield g, exp, one
    g.close()


def test_one_call_covers_four_tiles(four_tiles):
    g, exp, one = four_tiles
    check_call(one, 4096, 231 * 4096)
    assert (one["done"], one["slots_scanned"], one["cursor"][0]) == (1, 1 << 14, 1 << 14)
    assert_exact(entries(one), exp, RULES, TC.NOW)
    cnt = g.throttled_count(RULES, TC.NOW)
    assert (cnt["n"], cnt["bytes"]) == (one["n"], one["bytes"])


@pytest.mark.parametrize("max_entries", [1, 7, 64])
def test_cursor_loop_equals_one_call(four_tiles, max_entries):
    g, exp, one = four_tiles
    got, calls = sweep_all(g, RULES, TC.NOW, 0, max_entries)
    assert got == entries(one)                   # the same entries, the same order, none twice
    assert all(c["restarted"] == 0 for c in calls)
    assert all(c["slots_scanned"] <= 4096 for c in calls)    # W = one tile for these caps
    assert len(calls) >= max(len(exp) // max_entries, 4)
    if max_entries < 64:
        assert sum(c["n"] == max_entries for c in calls) >= len(exp) // max_entries - 4


def test_byte_cuts(pa):
    """names_cap = 231 and names of 200-231 bytes: one name fills a call, the
    cut falls where the bytes run out, before max_entries."""
    tab = TC.table_case(9, n=3000, classes=[(200, 231), (0, 14), (200, 231), (200, 231)])
    g = seeded(pa, tab, log2_slots=14, arena_bytes=1 << 21)
    exp, _ = TC.expected(gpu_dump(g), RULES, TC.NOW)
    assert sum(len(k) >= 200 for k in exp) >= 100
    full = entries(g.export_throttled(RULES, TC.NOW, 0, None, max_entries=4096))
    assert_exact(full, exp, RULES, TC.NOW)
    got, calls = sweep_all(g, RULES, TC.NOW, 0, 64, names_cap=231)
    assert got == full
    # a call was cut by bytes when the next entry of the sweep would not have fitted
    k = byte_cuts = 0
    for c in calls:
        k += c["n"]
        if c["n"] < 64 and k < len(full) and c["bytes"] + len(full[k][0]) > 231:
            byte_cuts += 1
    assert byte_cuts >= 5, byte_cuts
    assert max(c["n"] for c in calls) > 1
    g.close()


# ------------------------------------------------------------ 4. rebuild ----
def test_cursor_across_growth_restarts(pa):
    tab = TC.table_case(7)
    g = seeded(pa, tab, debug_tag_bits=3)
    first = g.export_throttled(RULES, TC.NOW, 0, None, max_entries=5)
    assert first["n"] == 5 and not first["done"] and first["restarted"] == 0
    more = TC.table_case(8, n=500)
    fresh = [i for i, nm in enumerate(more["names"]) if nm not in tab["rows"]]
    g.receive_soa([more["names"][i] for i in fresh], *[c[fresh] for c in more["cols"][:3]], T0 - SEC)
    assert g.capacity > 1024            # past the load limit: the table was rebuilt
    rows = gpu_dump(g)
    exp, _ = TC.expected(rows, RULES, TC.NOW)
    assert len(exp) > len(TC.expected(tab["rows"], RULES, TC.NOW)[0])
    d = g.export_throttled(RULES, TC.NOW, 0, first["cursor"], max_entries=4096)
    assert d["restarted"] == 1
    got, calls = entries(d), [d]
    while not calls[-1]["done"]:
        calls.append(g.export_throttled(RULES, TC.NOW, 0, calls[-1]["cursor"], max_entries=4096))
        got += entries(calls[-1])
    assert all(c["restarted"] == 0 for c in calls[1:])
    assert_exact(got, exp, RULES, TC.NOW)
    # a zeroed cursor never reports it
    assert g.export_throttled(RULES, TC.NOW, 0, None, max_entries=16)["restarted"] == 0
    assert g.export_throttled(RULES, TC.NOW, 0, (0, 0), max_entries=16)["restarted"] == 0
    g.close()


# ---------------------------------------------------------- 5. read-only ----
def test_nothing_is_written_to_the_handle(pa):
    tab = TC.table_case(7)
    g = seeded(pa, tab, debug_tag_bits=3, track_changes=True)
    # a change set with something in it, and an export sweep under way
    tk = tab["names"][:40]
    g.apply_mixed(np.zeros(40, np.uint8), tk, np.full(40, TC.NOW, np.int64), np.full(40, 100, np.int64),
                  np.full(40, SEC, np.int64), np.ones(40, np.uint64), *[np.zeros(40, t) for t in
                                                                         (np.uint64, np.uint64, np.int64)])
    whole = g.export_sweep(None, max_msgs=1024)[0]
    head, cur, st0 = g.export_sweep(None, max_msgs=8)
    assert len(head) == 8 and not st0["done"]
    before = (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity)
    assert before[2]["n"] > 0
    rows = gpu_dump(g)
    got, _ = sweep_all(g, RULES, TC.NOW, 0, 16)
    assert_exact(got, TC.expected(rows, RULES, TC.NOW)[0], RULES, TC.NOW)
    cnt = g.throttled_count(RULES, TC.NOW, TC.MIN_WAIT)
    assert cnt["n"] == len(TC.expected(rows, RULES, TC.NOW, TC.MIN_WAIT)[0])
    assert (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity) == before
    tail, _, st = g.export_sweep(cur, max_msgs=1024)
    assert st["restarted"] == 0 and st["done"] == 1 and head + tail == whole
    g.close()


# ----------------------------------------------------------- 6. refusals ----
def test_refusals_touch_nothing(pa, small):
    g, _ = small
    L, lib = g.L, pa._lib
    M, CAP = 16, 231 * 16
    bufs = dict(names=np.full(CAP, FILL, np.uint8), offs=np.full(M + 1, FILL64, np.uint64),
                retry_at=np.full(M, FILL64, np.int64), remaining=np.full(M, FILL64, np.uint64),
                rule=np.full(M, FILL, np.uint8))

    def rules_arr(n=4, prefix_len=None):
        arr = (lib.phip_throttle_rule * 9)()
        for i in range(9):
            p, f, per, c = RULES[i % 4]
            arr[i].prefix[:len(p)] = list(p)
            arr[i].prefix_len, arr[i].freq, arr[i].per, arr[i].count = len(p), f, per, c
        if prefix_len is not None:
            arr[n - 1].prefix_len = prefix_len
        return arr

    def out_struct(**kw):
        f = dict(names=bufs["names"].ctypes.data, names_cap=CAP, offs=bufs["offs"].ctypes.data,
                 max_entries=M, retry_at=bufs["retry_at"].ctypes.data,
                 remaining=bufs["remaining"].ctypes.data, rule=bufs["rule"].ctypes.data)
        f.update(kw)
        return lib.phip_throttled_out(f["names"], f["names_cap"], f["offs"], f["max_entries"], 0,
                                      f["retry_at"], f["remaining"], f["rule"])

    def call(rules=None, n_rules=4, now=TC.NOW, min_wait=0, out="default", flags=0, cur="default",
             st="default"):
        c, s = lib.phip_sweep_cursor(5, 77), lib.phip_sweep_stats(7, 7, 7, 7, 7)
        o = out_struct() if out == "default" else out
        rc = L.phip_export_throttled(g.h, C.byref(c) if cur == "default" else None,
                                     rules_arr() if rules is None else rules, n_rules, now, min_wait,
                                     C.byref(o) if o is not None else None,
                                     C.byref(s) if st == "default" else None, flags)
        assert (c.slot, c.layout) == (5, 77), "the cursor moved"
        assert (s.n, s.bytes, s.slots_scanned, s.done, s.restarted) == (7, 7, 7, 7, 7)
        for k, b in bufs.items():
            assert (b == (FILL if b.dtype == np.uint8 else FILL64)).all(), k
        return rc

    null_rules = C.cast(None, C.POINTER(lib.phip_throttle_rule))
    assert call(n_rules=0) == INVALID
    assert call(n_rules=9) == INVALID
    assert call(rules=rules_arr(4, 17)) == INVALID
    assert call(rules=rules_arr(1, 17), n_rules=1) == INVALID
    assert call(rules=null_rules) == INVALID
    assert call(cur=None) == INVALID
    assert call(st=None) == INVALID
    assert call(min_wait=-1) == INVALID
    assert call(flags=0x2) == INVALID
    assert call(flags=lib.SWEEP_COUNT | 0x40) == INVALID
    assert call(out=out_struct(max_entries=0)) == INVALID
    assert call(out=out_struct(names_cap=230)) == INVALID
    assert call(out=None) == INVALID                       # outside count mode
    assert call(out=out_struct(names=None)) == INVALID
    assert call(out=out_struct(offs=None)) == INVALID
    assert call(flags=lib.SWEEP_COUNT) == INVALID          # count mode takes no output
    with pytest.raises(pa.PatrolHipError):
        g.export_throttled(RULES + [(b"seventeen bytes!!", 1, 1, 1)], TC.NOW)
    # and the same buffers in a valid call (names_cap of exactly one name)
    c, s, o = lib.phip_sweep_cursor(), lib.phip_sweep_stats(), out_struct(names_cap=231)
    assert L.phip_export_throttled(g.h, C.byref(c), rules_arr(), 4, TC.NOW, 0, C.byref(o), C.byref(s), 0) == 0
    assert s.n >= 1 and bufs["offs"][0] == 0 and bufs["offs"][s.n] == s.bytes <= 231


# ------------------------------------------------------- 7. queued batch ----
def test_sees_a_queued_batch(pa):
    """A PHIP_RECV_ASYNC batch is finished first: the sweep sees its merges."""
    import torch
    dev = torch.device("cuda", 0)
    tab = TC.table_case(7)
    g = seeded(pa, tab, log2_slots=18)
    exp0, _ = TC.expected(tab["rows"], RULES, TC.NOW)
    # (the plain states: every third is an extreme one, whose added may be +Inf or NaN)
    granted = [nm for k, nm in enumerate(tab["names"])
               if k % 3 and TC.match(RULES, nm) >= 0 and nm not in exp0]
    assert len(granted) >= 100
    # 2^16 messages: every other granted bucket's `taken` raised far past its `added`
    n = 1 << 16
    hit = granted[::2]
    names = [hit[i % len(hit)] if i % 3 == 0 else b"filler-%d" % (i % 5000) for i in range(n)]
    a = np.zeros(n, np.float64)
    t = np.where(np.arange(n) % 3 == 0, 1e6, 1.0)
    e = np.ones(n, np.int64)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in names])
    blob = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()).to(dev)
    to = torch.from_numpy(offs).to(dev)
    ta, tt, te = (torch.from_numpy(x.view(np.int64).copy()).to(dev) for x in (a, t, e))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.receive_soa(blob, ta, tt, te, TC.NOW, name_offs=to, n=n, status=status, device=True, queue=True)
    got = []
    for d in g.throttled(RULES, TC.NOW, max_entries=1 << 16):
        got += entries(d)
    rows = gpu_dump(g)
    exp, _ = TC.expected(rows, RULES, TC.NOW)
    assert_exact(got, exp, RULES, TC.NOW)
    assert set(hit) <= set(exp) and not set(hit) & set(exp0)     # the merges are what it saw
    assert len(rows) == 600 + 5000
    g.close()


# ------------------------------------- a window of more than 512 tiles ----
def test_window_past_one_chunk_of_the_tile_scan(pa):
    """The export sweep's table of 2^22 slots (tests/_sweep_cases.chunk_repo)
    under one rule that denies half of it; max_entries = 525312 makes a window
    of 513 tiles, whose last tile's bases and whose totals come through the
    carry of k_sweep_scan's second chunk."""
    from tests import _sweep_cases as SC
    rules, now, M, cap = SC.CHUNK_RULE, SC.NOW, SC.CHUNK_MSGS, SC.CHUNK_CAP
    g = SC.chunk_repo(pa)
    rows = gpu_dump(g)
    exp, _ = TC.expected(rows, rules, now)
    assert 0.4 * len(rows) <= len(exp) <= 0.6 * len(rows)
    d = g.export_throttled(rules, now, 0, None, M, names_cap=cap)
    check_call(d, M, cap)
    assert d["slots_scanned"] == 513 * TC.TILE and (d["done"], d["cursor"][0]) == (0, 513 * TC.TILE)
    d2 = g.export_throttled(rules, now, 0, d["cursor"], M, names_cap=cap)
    check_call(d2, M, cap)
    assert (d2["done"], d2["cursor"][0]) == (1, g.capacity)
    got = entries(d) + entries(d2)
    assert_exact(got, exp, rules, now)
    cnt = g.throttled_count(rules, now)
    assert (cnt["n"], cnt["bytes"]) == (d["n"] + d2["n"], d["bytes"] + d2["bytes"])
    # slot order: windows of 64 tiles, one chunk of the scan each, no carry
    ref, calls = sweep_all(g, rules, now, 0, 1 << 16, names_cap=cap)
    assert len(calls) == 16 and got == ref
    # tile 512 alone (a window of one tile) holds entries, and they end the first call
    in512 = entries(g.export_throttled(rules, now, 0, (512 * TC.TILE, d["cursor"][1]), 1024))
    assert in512 and entries(d)[-len(in512):] == in512
    assert sum(c["n"] for c in calls[:8]) + len(in512) == d["n"]
    g.close()
