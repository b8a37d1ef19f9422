"""Packed frames (include/patrolhip.h "Packed frames"): the two rules restated
in plain Python, from the header's text and not from the C++, and the case
builders of tests/test_frames_abi.py (no GPU) and tests/test_frames.py.

Everything compared is an integer or a byte string: exact equality.
"""
from __future__ import annotations

import struct

import numpy as np

FIXED = 25                 # added, taken, elapsed, name length
FRAME_MIN, FRAME_DEFAULT, FRAME_MAX, FRAME_TILE = 256, 1472, 65507, 4096
INVALID, SHORT_BUFFER = -1, -5


# ------------------------------------------------------------- the rules ---
def split_frame(frame: bytes):
    """The splitting rule over one frame -> the sizes of its records."""
    if len(frame) == 0:
        return [0]                               # an empty frame: one empty record
    sizes, p = [], 0
    while len(frame) - p >= FIXED:
        sz = FIXED + frame[p + 24]
        if sz > len(frame) - p:
            break
        sizes.append(sz)
        p += sz
    if p < len(frame):
        sizes.append(len(frame) - p)             # the malformed tail, 1 byte or more
    return sizes


def unframe_model(frames):
    """-> (rec_offs, rec_frame) over the frames laid back to back."""
    rec_offs, rec_frame, pos = [], [], 0
    for f, fr in enumerate(frames):
        for sz in split_frame(fr):
            rec_offs.append(pos)
            rec_frame.append(f)
            pos += sz
    rec_offs.append(pos)
    return rec_offs, rec_frame


def records_of(frames):
    """The frames' records as byte strings, in order."""
    out = []
    for fr in frames:
        p = 0
        for sz in split_frame(fr):
            out.append(fr[p:p + sz])
            p += sz
    return out


def cuts_model(offs, frame_bytes, tile=FRAME_TILE):
    """The cut rule -> (frame_offs, frame_first), or None when a record is
    longer than frame_bytes.  tile=None: greedy without the runs."""
    n = len(offs) - 1
    tile = tile or max(n, 1)
    frame_offs, frame_first = [], []
    for r0 in range(0, n, tile):
        r1 = min(n, r0 + tile)
        first = r0
        while first < r1:
            j = first
            while j < r1 and offs[j + 1] - offs[first] <= frame_bytes:
                j += 1
            if j == first:
                return None
            frame_offs.append(offs[first])
            frame_first.append(first)
            first = j
    frame_offs.append(offs[n])
    return frame_offs, frame_first


# ------------------------------------------------------------ the cases ----
def record(name: bytes, a: int = 1, t: int = 2, e: int = 3) -> bytes:
    return struct.pack(">QQQ", a, t, e & (2**64 - 1)) + bytes([len(name)]) + name


def name_of(k: int, length: int) -> bytes:
    return (b"%d-" % k + b"x" * length)[:length]


def unframe_cases():
    """name -> list of frames, every case the issue lists (frame_bytes 1472)."""
    rng = np.random.default_rng(11)
    c = {}
    c["one_record_each"] = [record(b"b%d" % k, k, k, k) for k in range(40)]
    c["58_empty_names"] = [record(b"") * 58]
    c["58_empty_names_and_tail"] = [record(b"") * 58 + bytes(range(22))]
    c["name_lengths"] = [record(name_of(1, 0)) + record(name_of(2, 1)) + record(name_of(3, 230)) +
                         record(name_of(4, 231)), record(name_of(5, 231)) * 5,
                         record(name_of(6, 230)) + record(name_of(7, 1))]
    c["empty_frame"] = [record(b"a"), b"", record(b"bc") * 2, b"", b""]
    over = record(b"abcdef")
    c["length_byte_overruns"] = [record(b"ok") + over[:24] + bytes([7]) + over[25:],
                                 record(b"after")]
    c["short_tails"] = [b"\x01", bytes(24), record(b"n") + bytes(24), bytes(25) + b"\xff"]
    for nf in (0, 1, 63, 64, 65, 4096, 4097):
        frames = []
        for f in range(nf):
            k = int(rng.integers(1, 4)) if nf > 100 else int(rng.integers(1, 45))
            frames.append(b"".join(record(name_of(f * 50 + j, int(rng.integers(0, 9))), f, j, f + j)
                                   for j in range(k)))
        c["frames_%d" % nf] = frames
    return c


def offsets_of(sizes):
    offs = np.zeros(len(sizes) + 1, np.uint64)
    if len(sizes):
        offs[1:] = np.cumsum(np.asarray(sizes, np.uint64))
    return offs


def cuts_cases():
    """name -> (offs uint64[n+1], frame_bytes)."""
    rng = np.random.default_rng(12)
    c = {}
    for n in (0, 1, 4095, 4096, 4097, 8193):
        for fb in (256, 1472, 8972):
            c["n%d_fb%d" % (n, fb)] = (offsets_of(rng.integers(25, 257, n)), fb)
    # more than 64 records per frame: the repeat path of the wave's walk
    c["tile_of_25_byte_records"] = (offsets_of(np.full(4096, 25)), 8972)
    c["exact_fit"] = (offsets_of([256] * 9 + [128, 128] * 5), 256)
    return c


def frames_blob(frames):
    """-> (data uint8, padded to the next 8-byte boundary and 8 more; foffs uint64)."""
    foffs = offsets_of([len(f) for f in frames])
    total = int(foffs[-1])
    data = np.zeros((total + 7) // 8 * 8 + 8, np.uint8)
    data[:total] = np.frombuffer(b"".join(frames), np.uint8)
    return data, foffs


def pack_frames(records, frame_bytes):
    """Records -> frames by the cut rule (the model's)."""
    offs = [0]
    for r in records:
        offs.append(offs[-1] + len(r))
    fo, _ = cuts_model(offs, frame_bytes)
    blob = b"".join(records)
    return [blob[fo[k]:fo[k + 1]] for k in range(len(fo) - 1)]
