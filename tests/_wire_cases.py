"""Wire datagrams for the group's wire tests (tests/test_group_wire.py).

MarshalBinary (bucket.go:51-68) vectorised with numpy, since a test batch
holds up to 2^20 datagrams per member: added, taken, elapsed big-endian, one
length byte, the name, and optionally trailing junk that UnmarshalBinary
ignores (bucket.go:78-87).  check_against_marshal() pins the layout to
patrol_amd.marshal on a sample, so the builder is not its own reference.
"""
from __future__ import annotations

import numpy as np


def wire_blob(names, a, t, e, junk=None, rng=None):
    """-> (bytes uint8 up to the next 8-byte boundary past the last datagram,
    offs int64[n+1]).  junk: trailing bytes per datagram (int array) or None."""
    n = len(names)
    lens = np.fromiter((len(x) for x in names), np.int64, n)
    jk = np.zeros(n, np.int64) if junk is None else np.asarray(junk, np.int64)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(25 + lens + jk)
    total = int(offs[-1])
    size = (total // 8 + 1) * 8
    blob = (rng.integers(0, 256, size, dtype=np.uint8) if rng is not None
            else np.full(size, 0xA5, np.uint8))
    if n == 0:
        return blob, offs
    hdr = np.empty((n, 25), np.uint8)
    hdr[:, 0:8] = np.ascontiguousarray(a, np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    hdr[:, 8:16] = np.ascontiguousarray(t, np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    hdr[:, 16:24] = np.ascontiguousarray(e, np.int64).astype(">i8").view(np.uint8).reshape(n, 8)
    hdr[:, 24] = lens
    for c in range(25):   # (column by column: no n x 25 index array)
        blob[offs[:-1] + c] = hdr[:, c]
    nb = np.frombuffer(b"".join(names), np.uint8)
    if nb.size:
        no = np.zeros(n + 1, np.int64)
        no[1:] = np.cumsum(lens)
        pos = np.repeat(offs[:-1] + 25 - no[:-1], lens) + np.arange(nb.size)
        blob[pos] = nb
    return blob, offs


def datagram_list(blob, offs):
    bb = blob.tobytes()
    o = offs.tolist()
    return [bb[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def check_against_marshal(pa, names, a, t, e, blob, offs, junk=None, step=997):
    """Every step-th datagram of the blob is patrol_amd.marshal's bytes (then junk)."""
    for i in range(0, len(names), step):
        st = pa.BucketState(int(a[i]), int(t[i]), int(e[i]), 0)
        want = pa.marshal(names[i], st)
        got = blob[int(offs[i]):int(offs[i + 1])].tobytes()
        j = int(junk[i]) if junk is not None else 0
        assert got[:len(got) - j] == want, i


# The three malformed kinds of the stop rule (repo.go:70-74, bucket.go:71-91).
def malformed(kind: str, good: bytes) -> bytes:
    if kind == "short":          # fewer than the 25 fixed bytes
        return good[:24]
    if kind == "len_too_large":  # the length byte asks for more than is left
        return good[:24] + bytes([len(good) - 25 + 1]) + good[25:]
    if kind == "zero_size":
        return b""
    raise ValueError(kind)
