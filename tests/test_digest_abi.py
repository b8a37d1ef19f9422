"""Partition digests without a GPU (include/patrolhip.h "Partition digests"):
the header and the binding agree, the two host helpers (phip_digest_diff,
phip_digest_fold) do what the header says, and the model the GPU tests hold
the kernels to (tests/_digest_cases.py) does what digests are for: two oracle
repos that exchange only the partitions their digests differ in end with
equal digests, having sent a few per cent of a full sweep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import patrol_amd
from patrol_amd import _lib
from oracle import oracle as O
from tests import _digest_cases as DC
from tests import _gen
from tests import _sweep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
T0 = _gen.T0
LENS = [0, 1, 14, 15, 22, 23, 40, 231]


def test_declared_and_listed():
    for fn in ("phip_table_digest", "phip_digest_diff", "phip_digest_fold",
               "phip_export_sweep_parts"):
        assert re.search(r"\bint %s\s*\(" % fn, CODE), fn
        assert fn in _lib.EXPORTS and hasattr(_lib.load(), fn), fn
    m = re.search(r"#define PHIP_DIGEST_MAX_LOG2_PARTS\s+(\d+)", CODE)
    assert m and int(m.group(1)) == _lib.DIGEST_MAX_LOG2_PARTS == DC.MAX_LOG2 == 20
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", CODE)
    # the header says when two tables are comparable
    assert "same debug_tag_bits" in HEADER


def test_struct_layouts():
    for name, want in (("phip_digest_part", ["sum", "count"]),
                       ("phip_digest_stats", ["records", "bytes", "slots_scanned"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), CODE, re.S)
        assert re.findall(r"uint64_t (\w+);", body.group(1)) == want
        cls = getattr(_lib, name)
        assert [f for f, _ in cls._fields_] == want
        assert C.sizeof(cls) == 8 * len(want)
        assert [getattr(cls, f).offset for f in want] == [8 * i for i in range(len(want))]


def test_fnv_and_fmix_are_the_library_s():
    names = [b"", b"a", b"b12345", b"x" * 23, b"y" * 231, bytes(range(256))[:200]]
    blob, offs = patrol_amd.names_blob(names)
    out = np.zeros(len(names), np.uint64)
    assert _lib.load().phip_hash_names(None, blob.ctypes.data, offs.ctypes.data, len(names),
                                       out.ctypes.data, 0) == 0
    assert [int(x) for x in out] == [DC.fnv1a64(n) for n in names]
    assert DC.fnv1a64(b"") == 0xcbf29ce484222325 and DC.fnv1a64(b"a") == 0xaf63dc4c8601ec8c
    # fmix: the placement mix of tests/test_abi.py with seed 0
    M = (1 << 64) - 1

    def mix(t, s):
        x = t ^ s
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & M
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & M
        x ^= x >> 33
        return x
    rng = np.random.default_rng(1)
    for t in [0, 1, M] + [int(x) for x in rng.integers(0, 1 << 63, 200, dtype=np.uint64)]:
        assert DC.fmix(t) == mix(t, 0)
    assert DC.tag(b"a", 3) == 0xaf63dc4c8601ec8c & 7 and DC.part(5, 0) == 0
    assert DC.canon(1 << 63) == 0 and DC.canon(1) == 1 and DC.canon(0) == 0


def _entries(rng, k):
    return (rng.integers(0, 1 << 63, 1 << k, dtype=np.uint64),
            rng.integers(0, 50, 1 << k, dtype=np.uint64))


@pytest.mark.parametrize("k", [0, 5, 7, 12])
def test_digest_diff(k):
    rng = np.random.default_rng(k)
    a = _entries(rng, k)
    mask, nd = patrol_amd.digest_diff(a, (a[0].copy(), a[1].copy()))
    assert nd == 0 and not mask.any() and mask.size == max(1, (1 << k) // 64)
    n = 1 << k
    ps, pc = int(rng.integers(0, n)), int(rng.integers(0, n))
    s2, c2 = a[0].copy(), a[1].copy()
    s2[ps] ^= np.uint64(1 << 40)                     # a sum alone
    mask, nd = patrol_amd.digest_diff(a, (s2, a[1]))
    assert nd == 1 and DC.mask_words({ps}, k) == [int(w) for w in mask]
    c2[pc] += np.uint64(1)                           # a count alone
    mask, nd = patrol_amd.digest_diff(a, (a[0], c2))
    assert nd == 1 and DC.mask_words({pc}, k) == [int(w) for w in mask]
    # everything differs: the unused bits of the last word stay zero
    mask, nd = patrol_amd.digest_diff(a, (a[0] + np.uint64(1), a[1]))
    assert nd == n and [int(w) for w in mask] == DC.mask_words(range(n), k)
    if n < 64:
        assert int(mask[0]) == (1 << n) - 1
    # ndiff may be NULL; the mask is written over, not or-ed into
    L = _lib.load()
    ea = np.ascontiguousarray(np.stack(a, axis=1))
    eb = np.ascontiguousarray(np.stack((s2, c2), axis=1))
    raw = np.full(max(1, n // 64), 0xFFFFFFFFFFFFFFFF, np.uint64)
    assert L.phip_digest_diff(ea.ctypes.data, eb.ctypes.data, k, raw.ctypes.data, None) == 0
    assert [int(w) for w in raw] == DC.mask_words({ps, pc}, k)
    assert L.phip_digest_diff(ea.ctypes.data, eb.ctypes.data, 21, raw.ctypes.data, None) == -1
    assert L.phip_digest_diff(None, eb.ctypes.data, k, raw.ctypes.data, None) == -1


def _random_rows(rng, n, dirty=False):
    # n distinct names over the lengths (the empty name and a few single bytes among them)
    names = sorted({(b"%05d" % i).ljust(LENS[i % 8], b"n")[:LENS[i % 8]] if i % 64 < 8
                    else b"%05d" % i + b"m" * (i % 19) for i in range(n)})
    names += [b"fill-%d" % i for i in range(n - len(names))]
    a, t, e = (_gen.dirty_states(rng, len(names), p_special=0.3) if dirty
               else _gen.clean_states(rng, len(names)))
    return {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)}


def test_digest_fold_matches_the_model_at_every_level():
    rows = _random_rows(np.random.default_rng(11), 2000, dirty=True)
    top = DC.digest(rows, 20)
    d = (np.array(top[0], np.uint64), np.array(top[1], np.uint64))
    assert int(d[1].sum()) == top[2] > 1500
    for k in range(20, -1, -1):
        s, c = patrol_amd.digest_fold(d, k)
        want = DC.digest(rows, k)
        assert [int(x) for x in s] == want[0] and [int(x) for x in c] == want[1], k
    # step by step gives the same as in one go
    step = d
    for k in range(19, 11, -1):
        step = patrol_amd.digest_fold(step, k)
    one = patrol_amd.digest_fold(d, 12)
    assert (step[0] == one[0]).all() and (step[1] == one[1]).all()


def test_digest_fold_in_place_and_refusals():
    L = _lib.load()
    rng = np.random.default_rng(4)
    e = np.ascontiguousarray(np.stack(_entries(rng, 10), axis=1))
    ref = e.copy()
    out = np.zeros((1 << 6, 2), np.uint64)
    assert L.phip_digest_fold(e.ctypes.data, 10, 6, out.ctypes.data) == 0
    assert (e == ref).all()
    want = ref.reshape(64, 16, 2).sum(axis=1, dtype=np.uint64)
    assert (out == want).all()
    assert L.phip_digest_fold(e.ctypes.data, 10, 6, e.ctypes.data) == 0      # in place
    assert (e[:64] == want).all() and (e[64:] == ref[64:]).all()
    e2 = ref.copy()
    assert L.phip_digest_fold(e2.ctypes.data, 10, 10, e2.ctypes.data) == 0   # same level
    assert (e2 == ref).all()
    assert L.phip_digest_fold(ref.ctypes.data, 6, 7, out.ctypes.data) == -1
    assert L.phip_digest_fold(ref.ctypes.data, 21, 7, out.ctypes.data) == -1
    assert L.phip_digest_fold(None, 6, 5, out.ctypes.data) == -1
    with pytest.raises(patrol_amd.PatrolHipError):
        patrol_amd.digest_fold((ref[:64, 0], ref[:64, 1]), 7)


# ---- the model against the oracle alone ------------------------------------
def _seeded(rows):
    o = O.Repo()
    ks = list(rows)
    o.seed(ks, *[[rows[k][j] for k in ks] for j in range(4)])
    return o


def ab_rows(rng, ndiff, dirty, n=1500, only=5):
    """A and B hold the same n buckets, but for `ndiff` of them whose state
    was drawn again on B (dirty: with NaN, -0.0, infinities, negatives and
    zero states on both sides), and `only` more names each that the other
    side lacks (clean states: a negative field of a bucket the receiver has
    to create is test_negative_field_against_an_absent_bucket's subject)."""
    a_rows = _random_rows(rng, n, dirty)
    b_rows = {k: v[:3] + (T0 - 5,) for k, v in a_rows.items()}
    names = sorted(a_rows)
    redrawn = _random_rows(rng, n, dirty)

    def below_zero(v):
        return any(b >> 63 and 0 < (b & ~DC.SIGN) <= 0x7FF0000000000000 for b in v[:2]) or v[2] < 0
    for i in rng.choice(len(names), ndiff, replace=False):
        va, vb = a_rows[names[i]], redrawn[names[i]]
        # (a zero state against a negative field: that test's subject too)
        if (SC.is_zero(*va[:3]) and below_zero(vb)) or (SC.is_zero(*vb[:3]) and below_zero(va)):
            continue
        b_rows[names[i]] = vb[:3] + (T0 - 5,)
    a, t, e = _gen.clean_states(rng, 2 * only)
    for i in range(only):
        a_rows[b"A-only-%d" % i] = (int(a[i]), int(t[i]), int(e[i]), T0)
        j = only + i
        b_rows[b"B-only-%d-with-a-long-name" % i] = (int(a[j]), int(t[j]), int(e[j]), T0)
    return a_rows, b_rows


def exchange(a_rows, b_rows, k):
    """One reconcile round through the model: both sides send what the diff
    of their digests asks for, at the same time.  -> (A's rows after, B's rows
    after, datagrams A sent, datagrams B sent, the partitions that differed)."""
    parts = DC.diff(DC.digest(a_rows, k), DC.digest(b_rows, k))
    mask = DC.mask_words(parts, k)
    from_a, from_b = DC.exported(a_rows, k, mask), DC.exported(b_rows, k, mask)
    oa, ob = _seeded(a_rows), _seeded(b_rows)
    now = T0 + 9
    for o, dgs in ((oa, from_b), (ob, from_a)):
        st, _, _, _, stop = o.receive(list(dgs.values()), now)
        assert stop == len(dgs) and (st & 0x7F == 1).all()
    return oa.dump(), ob.dump(), from_a, from_b, parts


def test_clean_replicas_converge_on_a_few_per_cent_of_a_sweep():
    a_rows, b_rows = ab_rows(np.random.default_rng(31), 20, dirty=False)
    assert sum(a_rows[k][:3] != b_rows[k][:3] for k in a_rows if k in b_rows) == 20
    a2, b2, from_a, from_b, parts = exchange(a_rows, b_rows, 12)
    assert 20 <= len(parts) <= 30
    for k in (12, 16):
        assert DC.digest(a2, k) == DC.digest(b2, k)
    assert {k: v[:3] for k, v in a2.items()} == {k: v[:3] for k, v in b2.items()}
    full_a, full_b = SC.exported(a_rows), SC.exported(b_rows)
    assert len(full_a) >= 1500 and len(full_b) >= 1500
    print("sent %d of %d and %d of %d" % (len(from_a), len(full_a), len(from_b), len(full_b)))
    assert 20 <= len(from_a) < 0.05 * len(full_a) and 20 <= len(from_b) < 0.05 * len(full_b)
    # a finer level sends no more: only what shares a partition with a difference
    _, _, fa16, fb16, _ = exchange(a_rows, b_rows, 16)
    assert 25 <= len(fa16) <= len(from_a) and 25 <= len(fb16) <= len(from_b)
    a3, b3, _, _, _ = exchange(a_rows, b_rows, 16)
    assert DC.digest(a3, 12) == DC.digest(b3, 12) and DC.digest(a3, 16) == DC.digest(b3, 16)


def test_dirty_replicas_differ_only_where_a_nan_sits():
    """dirty_states rows (p_special = 0.3) on both sides.  Narrower than plain
    dirty rows in one respect (ab_rows): no negative field meets an absent
    bucket or a zero state, because Merge never lowers a field and such a pair
    does not converge in one round whatever the digests do (patrolhip.h
    "Limits"; test_negative_field_against_an_absent_bucket pins it).  What is
    left after a round is then the NaN partitions alone."""
    a_rows, b_rows = ab_rows(np.random.default_rng(32), 300, dirty=True)
    for k in (12, 16):
        a2, b2, from_a, from_b, parts = exchange(a_rows, b_rows, k)
        nan = DC.nan_parts([a_rows, b_rows], k)
        left = DC.diff(DC.digest(a2, k), DC.digest(b2, k))
        assert len(parts) >= 250 and nan and left
        assert left <= nan, sorted(left - nan)
        # a second round asks for those partitions alone, sends only their
        # buckets, and a NaN that sticks leaves them as they were
        a3, b3, fa2, fb2, parts2 = exchange(a2, b2, k)
        assert parts2 == left
        assert len(fa2) < len(from_a) and len(fb2) < len(from_b)
        assert set(fa2) == set(DC.exported(a2, k, DC.mask_words(left, k)))
        assert DC.diff(DC.digest(a3, k), DC.digest(b3, k)) == left


def test_negative_field_against_an_absent_bucket():
    """Merge never lowers a field and a created bucket starts at zero
    (repo.go:78-90), so a negative field of a bucket only one side holds does
    not arrive in the round that creates it: the creator's 0 comes back in the
    next round and both sides end at 0.  All fields <= 0 against an absent
    bucket (or a zero state) never converge: the other side's state stays zero
    and a zero state is never sent.  The digests report both truthfully."""
    neg, one = 0xBFF0000000000000, 0x3FF0000000000000
    base = _random_rows(np.random.default_rng(5), 50)
    a_rows = dict(base)
    a_rows[b"neg-added"] = (neg, one, 7, T0)
    a_rows[b"all-below-zero"] = (neg, 1 << 63, -3, T0)
    b_rows = dict(base)
    k = 12
    a2, b2, from_a, from_b, parts = exchange(a_rows, b_rows, k)
    want = {DC.part(DC.tag(n), k) for n in (b"neg-added", b"all-below-zero")}
    assert parts == want and len(from_b) <= len(from_a) <= 4
    assert b2[b"neg-added"][:3] == (0, one, 7) and b2[b"all-below-zero"][:3] == (0, 0, 0)
    assert DC.diff(DC.digest(a2, k), DC.digest(b2, k)) == want
    a3, b3, _, _, _ = exchange(a2, b2, k)
    assert a3[b"neg-added"][:3] == b3[b"neg-added"][:3] == (0, one, 7)
    assert DC.diff(DC.digest(a3, k), DC.digest(b3, k)) == {DC.part(DC.tag(b"all-below-zero"), k)}


def test_equal_for_anti_entropy():
    """Replicas that differ only in the sign of a zero, in `created`, or in
    zero-state buckets one side lacks have equal digests."""
    rng = np.random.default_rng(8)
    rows = _random_rows(rng, 600, dirty=True)
    rows[b"pz"] = (0, DC.SIGN, 5, T0)
    rows[b"nz"] = (DC.SIGN, 0x4008000000000000, 0, T0)
    flip = {0: DC.SIGN, DC.SIGN: 0}
    other = {k: (flip.get(a, a), flip.get(t, t), e, c + 12345) for k, (a, t, e, c) in rows.items()}
    assert sum(other[k][:2] != rows[k][:2] for k in rows) >= 40
    more = dict(other)
    for i in range(30):
        more[b"zero-state-%d" % i] = (0 if i % 2 else DC.SIGN, 0, 0, T0)
    for k in (0, 7, 12, 20):
        d = DC.digest(rows, k)
        assert d == DC.digest(other, k) == DC.digest(more, k)
        assert d[2] == len(SC.exported(rows)) and d[3] == sum(map(len, SC.exported(rows).values()))
    # while any other difference shows
    changed = dict(rows)
    changed[b"pz"] = (0, DC.SIGN, 6, T0)
    assert DC.diff(DC.digest(rows, 12), DC.digest(changed, 12)) == {DC.part(DC.tag(b"pz"), 12)}
