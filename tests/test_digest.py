"""Partition digests and the digest-filtered sweep on the GPU
(include/patrolhip.h "Partition digests"), through the C ABI via the binding.

What a digest must hold and what a filtered sweep must write is computed in
Python from the table's dump (tests/_digest_cases.py); what a reconcile round
leaves behind is two oracle Repos that received the same datagrams in the same
order.  Bit-exact throughout.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _digest_cases as DC  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _sweep_cases as SC  # noqa: E402
from tests.test_digest_abi import ab_rows  # noqa: E402
from tests.test_export_sweep import (LENGTHS, assert_exact, gpu_dump, kinds_table,  # noqa: E402
                                     make_names, name_of, seed)

T0, SEC = _gen.T0, _gen.SEC


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def model_arrays(rows, k, tag_bits=0):
    s, c, n, b = DC.digest(rows, k, tag_bits)
    return np.array(s, np.uint64), np.array(c, np.uint64), n, b


def assert_digest(repo, rows, k, tag_bits=0):
    s, c, st = repo.digest(k)
    ws, wc, n, b = model_arrays(rows, k, tag_bits)
    assert s.shape == c.shape == (1 << k,)
    assert (c == wc).all(), (k, np.flatnonzero(c != wc)[:5])
    assert (s == ws).all(), (k, np.flatnonzero(s != ws)[:5])
    assert (st["records"], st["bytes"], st["slots_scanned"]) == (n, b, repo.capacity), k
    return s, c, st


def same(d1, d2):
    return (d1[0] == d2[0]).all() and (d1[1] == d2[1]).all()


def test_every_kind_of_record(pa):
    repo = kinds_table(pa)
    rows = gpu_dump(repo)
    assert {len(k) for k in SC.exported(rows)} == set(LENGTHS)
    cnt = repo.sweep_count()
    for k in (0, 1, 6, 12, 13, 20):
        _, c, st = assert_digest(repo, rows, k)
        assert (st["records"], st["bytes"]) == (cnt["n"], cnt["bytes"])
        assert int(c.sum()) == cnt["n"] and 450 <= cnt["n"] < len(rows)
    assert gpu_dump(repo) == rows                       # the table is left untouched
    repo.close()


def test_folding_crosses_the_two_paths(pa):
    repo = kinds_table(pa)
    d = {k: repo.digest(k)[:2] for k in (0, 12, 13, 20)}
    assert same(pa.digest_fold(d[13], 12), d[12])       # global adds against LDS sums
    assert same(pa.digest_fold(d[20], 13), d[13])
    assert same(pa.digest_fold(d[12], 0), d[0])
    assert same(pa.digest_fold(d[20], 0), d[0])
    repo.close()


def test_several_workgroups_and_device_pointers(pa):
    import torch
    repo = pa.GPURepo(log2_slots=14, arena_bytes=1 << 18)
    rng = np.random.default_rng(9)
    names = make_names(5000)
    a, t, e = _gen.clean_states(rng, len(names))
    seed(repo, {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)})
    assert repo.capacity == 1 << 14                     # eight workgroups stride over it
    rows = gpu_dump(repo)
    for k in (0, 3, 12, 13):
        s, c, st = assert_digest(repo, rows, k)
        assert st["records"] == len(names)
        out = torch.full(((1 << k) + 1, 2), -1, dtype=torch.int64, device="cuda:0")
        st2 = repo.digest_device(out, k)
        assert st2 == st
        got = out.cpu().numpy().view(np.uint64)
        assert (got[:-1, 0] == s).all() and (got[:-1, 1] == c).all()
        assert (out[-1].cpu().numpy() == -1).all()      # nothing past 2^k entries
    repo.close()


def test_placement_independence(pa):
    """Another seed, another table size, growth, a rebuild, a restore: the
    digests do not move."""
    names = make_names(1900)
    # (dirty states without special_rows' extremes: an elapsed of INT64_MIN is
    # idle under every rule, and the rebuild below must evict nothing covered)
    a, t, e = _gen.dirty_states(np.random.default_rng(21), len(names), p_special=0.25)
    rows = {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)}
    small = pa.GPURepo(log2_slots=10, arena_bytes=1 << 17, hash_seed=1)
    big = pa.GPURepo(log2_slots=13, arena_bytes=1 << 17, hash_seed=2)
    ks = list(rows)
    for part in (ks[:700], ks[700:]):                   # the small table grows while it is filled
        seed(small, {k: rows[k] for k in part})
    seed(big, rows)
    assert small.capacity > 1024 and big.capacity == 1 << 13
    levels = (0, 6, 12, 13, 16)
    want = {k: assert_digest(big, rows, k)[:2] for k in levels}
    for k in levels:
        assert same(small.digest(k)[:2], want[k]), k
    # a rebuild by eviction.  phip_evict_idle with nothing idle only counts and
    # leaves the table as it is, so one idle zero-state bucket is added first:
    # evicting it rebuilds the table and removes nothing a digest covers.
    small.receive_soa([b"idle-zero-state"], [0], [0], [0], T0 - 10**6 * SEC)
    st = small.evict_idle(T0, 10**5 * SEC)
    assert st["evicted"] == 1 and st["buckets"] == len(rows)
    for k in levels:
        assert same(small.digest(k)[:2], want[k]), k
    img = small.snapshot()
    other = pa.GPURepo(log2_slots=10, arena_bytes=1 << 17, hash_seed=3)
    other.restore(img)
    small.restore(img)
    for k in levels:
        assert same(small.digest(k)[:2], want[k]) and same(other.digest(k)[:2], want[k]), k
    for r in (small, big, other):
        r.close()


# ---- the filtered sweep ----------------------------------------------------
def sweep_all(repo, max_msgs, parts, now=0, idle_ns=0, cursor=None):
    """Loop to done -> (datagrams in order, stats of every call)."""
    k, mask = parts
    m = sum(DC.in_mask(mask, p) for p in range(1 << k))
    got, sts = [], []
    while True:
        dgs, cursor, st = repo.export_sweep(cursor, max_msgs, None, now, idle_ns, parts=parts)
        offs = st["offs"]
        assert st["n"] == len(dgs) <= max_msgs
        assert offs[0] == 0 and int(offs[-1]) == st["bytes"] <= 256 * max_msgs
        assert [len(d) for d in dgs] == list(np.diff(offs.astype(np.int64)))
        assert st["slots_scanned"] <= (DC.window(max_msgs, k, m) if m else 0)
        got += dgs
        sts.append(st)
        assert len(sts) <= 2000
        if st["done"]:
            assert cursor[0] == repo.capacity
            return got, sts


def masks_of(k, rows, rng, tag_bits=0):
    """A random half, its complement, one populated partition, all, none."""
    n = 1 << k
    words = max(1, n // 64)
    full = np.array(DC.mask_words(range(n), k), np.uint64)
    half = rng.integers(0, 1 << 63, words, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, words, dtype=np.uint64)
    half &= full
    one = DC.part(DC.tag(sorted(SC.exported(rows))[5], tag_bits), k)
    return dict(half=half, complement=full & ~half,
                single=np.array(DC.mask_words({one}, k), np.uint64), full=full,
                empty=np.zeros(words, np.uint64))


def is_subsequence(got, whole):
    it = iter(whole)
    return all(any(d == w for w in it) for d in got)


@pytest.mark.parametrize("k", [0, 4, 12, 16])
def test_filtered_sweep_is_exact(pa, k):
    repo = kinds_table(pa)
    rows = gpu_dump(repo)
    unfiltered = repo.export_sweep(None, max_msgs=1024)[0]
    assert_exact(unfiltered, SC.exported(rows))
    masks = masks_of(k, rows, np.random.default_rng(100 + k))
    by_mask = {}
    for label, mask in masks.items():
        model = DC.exported(rows, k, mask)
        for max_msgs in (1, 16, 1024):
            got, sts = sweep_all(repo, max_msgs, (k, mask))
            assert_exact(got, model)
            assert is_subsequence(got, unfiltered), (label, max_msgs)     # slot order
            assert all(s["restarted"] == 0 for s in sts)
            if label == "empty":
                assert len(sts) == 1 and sts[0]["slots_scanned"] == 0 and sts[0]["n"] == 0
                assert list(sts[0]["offs"]) == [0]
        by_mask[label] = got
        # count mode: the same totals, the cursor left alone
        cnt = repo.sweep_count(parts=(k, mask))
        assert (cnt["n"], cnt["bytes"]) == (len(model), sum(map(len, model.values())))
        c, s = pa._lib.phip_sweep_cursor(5, 7), pa._lib.phip_sweep_stats()
        assert repo.L.phip_export_sweep_parts(repo.h, C.byref(c), 0, 0, k, mask.ctypes.data, None,
                                              0, None, 0, C.byref(s), 0x200) == 0
        assert (c.slot, c.layout, s.n, s.bytes) == (5, 7, cnt["n"], cnt["bytes"])
    assert len(by_mask["single"]) >= 1 and by_mask["full"] == unfiltered
    assert sorted(by_mask["half"] + by_mask["complement"]) == sorted(unfiltered)
    if k:
        assert by_mask["half"] and by_mask["complement"]
    repo.close()


def test_filtered_sweep_over_several_tiles(pa):
    """2^14 slots are four tiles: with one partition of 2^16 asked for, the
    write pass skips the tiles the count pass found empty -- whichever tile
    the few records sit in, the first and the last included."""
    repo = pa.GPURepo(log2_slots=14, arena_bytes=1 << 18)
    rng = np.random.default_rng(19)
    names = make_names(5000)
    a, t, e = _gen.clean_states(rng, len(names))
    seed(repo, {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)})
    rows = gpu_dump(repo)
    unfiltered = [d for ds, _ in repo.sweep(max_msgs=8192) for d in ds]
    assert_exact(unfiltered, SC.exported(rows))
    assert repo.capacity == 1 << 14
    k = 16
    for pos in (0, 1, len(unfiltered) // 3, len(unfiltered) // 2, len(unfiltered) - 1):
        mask = np.array(DC.mask_words({DC.part(DC.tag(name_of(unfiltered[pos])), k)}, k), np.uint64)
        model = DC.exported(rows, k, mask)
        assert 1 <= len(model) <= 4
        for max_msgs in (1, 4096):
            got, sts = sweep_all(repo, max_msgs, (k, mask))
            assert_exact(got, model)
            assert is_subsequence(got, unfiltered)
        assert len(sts) == 1 and sts[0]["slots_scanned"] == 1 << 14    # the window is the table
    half = masks_of(4, rows, rng)["half"]
    for max_msgs in (64, 1000):
        got, sts = sweep_all(repo, max_msgs, (4, half))
        assert_exact(got, DC.exported(rows, 4, half))
        assert is_subsequence(got, unfiltered) and len(sts) >= 2
    repo.close()


def test_full_mask_at_level_zero_is_the_unfiltered_sweep_call_for_call(pa):
    repo = kinds_table(pa)
    full = np.array([1], np.uint64)
    c1 = c2 = None
    calls = 0
    while True:
        d1, c1, s1 = repo.export_sweep(c1, 16)
        d2, c2, s2 = repo.export_sweep(c2, 16, parts=(0, full))
        o1, o2 = s1.pop("offs"), s2.pop("offs")
        assert d1 == d2 and c1 == c2 and s1 == s2 and (o1 == o2).all()
        calls += 1
        if s1["done"]:
            break
    assert calls >= 30
    repo.close()


def test_idle_filter_composes_with_the_mask(pa):
    repo = pa.GPURepo(log2_slots=10, arena_bytes=1 << 12)
    rows = SC.filter_rows()
    seed(repo, rows)
    k = 4
    mask = masks_of(k, rows, np.random.default_rng(3))["half"]
    sizes = set()
    for idle_ns in (SC.IDLE_NS[3], SC.IDLE_NS[5]):
        model = DC.exported(rows, k, mask, SC.NOW, idle_ns)
        assert 0 < len(model) < len(SC.exported(rows, SC.NOW, idle_ns))
        assert len(model) < len(DC.exported(rows, k, mask))
        got, _ = sweep_all(repo, 16, (k, mask), now=SC.NOW, idle_ns=idle_ns)
        assert_exact(got, model)
        cnt = repo.sweep_count(SC.NOW, idle_ns, parts=(k, mask))
        assert (cnt["n"], cnt["bytes"]) == (len(model), sum(map(len, got)))
        sizes.add(len(model))
    assert len(sizes) == 2
    repo.close()


def test_three_tag_bits(pa):
    """debug_tag_bits = 3 and a fixed seed: eight tags, so at most eight
    partitions are populated at any level; digest and filtered sweep follow
    the truncated tags."""
    repo = kinds_table(pa, log2_slots=9, count=240, zeros=10, debug_tag_bits=3, hash_seed=0)
    rows = gpu_dump(repo)
    for k in (0, 3, 12, 13):
        _, c, _ = assert_digest(repo, rows, k, tag_bits=3)
        assert 1 <= np.count_nonzero(c) <= 8
        assert not (k == 12 and (c == model_arrays(rows, k)[1]).all())   # full tags differ
    k = 12
    c = repo.digest(k)[1]
    filled = [int(p) for p in np.flatnonzero(c)]
    assert len(filled) >= 4
    mask = np.array(DC.mask_words(filled[::2], k), np.uint64)
    model = DC.exported(rows, k, mask, tag_bits=3)
    assert len(model) == int(c[filled[::2]].sum()) > 0
    for max_msgs in (16, 512):
        got, _ = sweep_all(repo, max_msgs, (k, mask))
        assert_exact(got, model)
    repo.close()


def test_rebuild_mid_sweep_with_a_mask(pa):
    repo = kinds_table(pa, count=500, zeros=20)
    k = 4
    mask = masks_of(k, gpu_dump(repo), np.random.default_rng(6))["half"]
    part, cursor, st = repo.export_sweep(None, 64, parts=(k, mask))
    assert st["n"] == 64 and st["done"] == 0 and 0 < cursor[0] < 1024
    more = [b"grown-%d" % i for i in range(500)]
    a, t, e = _gen.clean_states(np.random.default_rng(2), 500)
    repo.receive_soa(more, a, t, e, T0 + 9)
    assert repo.capacity > 1024
    dgs, cursor, st = repo.export_sweep(cursor, 64, parts=(k, mask))
    assert st["restarted"] == 1
    rest = list(dgs)
    while not st["done"]:
        dgs, cursor, st = repo.export_sweep(cursor, 64, parts=(k, mask))
        assert st["restarted"] == 0
        rest += dgs
    model = DC.exported(gpu_dump(repo), k, mask)
    assert_exact(rest, model)                           # the restarted sweep alone is exact
    assert any(name_of(d).startswith(b"grown-") for d in rest)
    repo.close()


# ---- a reconcile round on the device ---------------------------------------
def oracle_of(rows):
    o = O.Repo()
    ks = list(rows)
    o.seed(ks, *[[rows[k][j] for k in ks] for j in range(4)])
    return o


def sweep_into(src, dst, dst_oracle, parts, now, max_msgs=48):
    """src's buckets of `parts` straight into dst (device pointers), and the
    same datagrams in the same order into dst's oracle."""
    import torch
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")          # the byte cap binds too
    offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device="cuda:0")
    cursor, sent = None, []
    while True:
        n, cursor, st = src.export_sweep_device(out, offs, cursor, max_msgs, parts=parts)
        h_offs = offs[:n + 1].cpu().numpy()
        raw = out[:st["bytes"]].cpu().numpy().tobytes()
        dgs = [raw[h_offs[i]:h_offs[i + 1]] for i in range(n)]
        assert dst.receive_datagrams_device(out, offs, n, now) == n
        rs = dst_oracle.receive(dgs, now)
        assert rs[4] == n and ((rs[0] & 0x7F) == 1).all()
        sent += dgs
        if st["done"]:
            return sent


@pytest.mark.parametrize("dirty", [False, True])
def test_reconcile_round_trip(pa, dirty):
    """The dirty variant's inputs are ab_rows': dirty states on both sides, but
    no negative field against an absent bucket or a zero state (one-sided names
    are clean).  Merge never lowers a field, so such a pair does not converge in
    one round (patrolhip.h "Limits", pinned on the CPU by
    test_digest_abi.py::test_negative_field_against_an_absent_bucket), and the
    partitions left after the round are the NaN partitions alone."""
    a_rows, b_rows = ab_rows(np.random.default_rng(41 + dirty), 40, dirty, only=10)
    A = pa.GPURepo(log2_slots=12, arena_bytes=1 << 16, hash_seed=1)
    B = pa.GPURepo(log2_slots=11, arena_bytes=1 << 16, hash_seed=2)
    seed(A, a_rows)
    seed(B, b_rows)
    oa, ob = oracle_of(a_rows), oracle_of(b_rows)
    k = 12
    mask, nd = pa.digest_diff(A.digest(k)[:2], B.digest(k)[:2])
    want = DC.diff(DC.digest(a_rows, k), DC.digest(b_rows, k))
    assert [int(w) for w in mask] == DC.mask_words(want, k) and nd == len(want)
    assert (35 if dirty else 55) <= nd <= 62
    a_to_b = sweep_into(A, B, ob, (k, mask), T0 + 77)
    assert_exact(a_to_b, DC.exported(a_rows, k, mask))
    b_mid = ob.dump()
    b_to_a = sweep_into(B, A, oa, (k, mask), T0 + 78)
    assert_exact(b_to_a, DC.exported(b_mid, k, mask))
    assert gpu_dump(A) == oa.dump() and gpu_dump(B) == ob.dump() == b_mid
    full = len(SC.exported(a_rows)) + len(SC.exported(b_mid))
    print("sent %d + %d of %d" % (len(a_to_b), len(b_to_a), full))
    assert len(a_to_b) + len(b_to_a) < full / 10
    da, db = A.digest(k), B.digest(k)
    left = pa.digest_diff(da[:2], db[:2])
    if dirty:
        nan = DC.nan_parts([a_rows, b_rows], k)
        still = {p for p in range(1 << k) if DC.in_mask(left[0], p)}
        assert still <= nan, sorted(still - nan)
        assert still == DC.diff(DC.digest(oa.dump(), k), DC.digest(ob.dump(), k))
    else:
        assert left[1] == 0 and same(da, db) and da[2]["records"] == db[2]["records"]
        assert same(A.digest(16), B.digest(16))
    A.close()
    B.close()


def test_invalid_arguments(pa):
    import torch
    repo = kinds_table(pa, count=80, zeros=4)
    L, lib = repo.L, pa._lib
    out, offs = np.zeros(4096, np.uint8), np.zeros(9, np.uint64)
    full4 = np.array([0xFFFF], np.uint64)
    p = lambda x: None if x is None else (x.data_ptr() if hasattr(x, "data_ptr")   # noqa: E731
                                          else x.ctypes.data)

    def call(idle_ns=0, max_msgs=8, out_cap=4096, flags=0, o=out, f=offs, k=4, mask=full4):
        c, s = lib.phip_sweep_cursor(), lib.phip_sweep_stats()
        return L.phip_export_sweep_parts(repo.h, C.byref(c), 0, idle_ns, k, p(mask), p(o), out_cap,
                                         p(f), max_msgs, C.byref(s), flags), c, s

    assert call()[0] == 0
    assert call(out_cap=256, max_msgs=1)[0] == 0
    assert call(k=20, mask=np.zeros(1 << 14, np.uint64))[0] == 0
    for kw in (dict(idle_ns=-1), dict(idle_ns=-2**63), dict(max_msgs=0), dict(out_cap=255),
               dict(flags=0x2), dict(flags=0x40), dict(flags=0x80), dict(flags=0x400),
               dict(flags=0x80000000), dict(flags=0x200),       # (count mode takes no buffer)
               dict(k=21), dict(k=0xFFFFFFFF), dict(mask=None), dict(mask=None, flags=0x200, o=None)):
        out[:] = 0xAB
        rc, c, s = call(**kw)
        assert rc == -1, kw
        assert (c.slot, c.layout) == (0, 0) and (out == 0xAB).all(), kw   # a refused call moves nothing
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(4096 + 16, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(9, dtype=torch.int64, device=dev)
    assert call(flags=1, o=d_out, f=d_offs)[0] == 0
    assert call(flags=1, o=d_out[1:], f=d_offs)[0] == -1        # misaligned
    assert call(flags=1, o=d_out, f=d_offs, out_cap=4092)[0] == -1   # not a multiple of 8
    assert call(flags=1, o=d_out, f=d_offs, out_cap=256)[0] == -1    # budget below one datagram
    assert call(flags=1, o=d_out, f=d_offs, out_cap=264, max_msgs=1)[0] == 0
    with pytest.raises(ValueError):
        repo.export_sweep(None, 8, parts=(12, np.zeros(3, np.uint64)))   # a short mask

    # phip_table_digest
    ent = np.full((16, 2), 0xCD, np.uint64)
    st = lib.phip_digest_stats(1, 2, 3)

    def dig(k=4, o=ent, flags=0):
        return L.phip_table_digest(repo.h, k, p(o), C.byref(st), flags)

    assert dig() == 0 and st.slots_scanned == 1024 and st.records == int(ent[:, 1].sum()) > 0
    assert L.phip_table_digest(repo.h, 4, ent.ctypes.data, None, 0) == 0     # st may be NULL
    d_ent = torch.zeros(17, 2, dtype=torch.int64, device=dev)
    assert dig(o=d_ent, flags=1) == 0
    for kw in (dict(k=21), dict(k=0xFFFFFFFF), dict(o=None), dict(flags=0x2), dict(flags=0x200),
               dict(flags=0x20), dict(flags=0x80000000), dict(flags=0x3, o=d_ent),
               dict(flags=1, o=d_ent.view(torch.uint8).flatten()[4:])):   # a misaligned device buffer
        ent[:] = 0xCD
        st.records, st.bytes, st.slots_scanned = 1, 2, 3
        assert dig(**kw) == -1, kw
        assert (ent == 0xCD).all() and (st.records, st.bytes, st.slots_scanned) == (1, 2, 3), kw
    with pytest.raises(pa.PatrolHipError):
        repo.digest(21)
    assert dig() == 0                                   # the handle is fine afterwards
    repo.close()
