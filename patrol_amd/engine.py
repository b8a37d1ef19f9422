"""Python mirror of Patrol's Repo seam over libpatrolhip.

Patrol (Go) exposes its bucket map through the `Repo` interface
(repo.go:15-18) and drives it from two loops: the UDP `Receive` loop
(repo.go:54-92) and the HTTP `takeBucket` handler (api.go:51-86).  A
device-resident table cannot hand out mutable `*Bucket` pointers, so the
unit of work here is a batch of ops, each with the exact Go semantics in
batch order (include/patrolhip.h).  This module is a thin ctypes layer used by
the tests and bench.py; a Go deployment binds the same C ABI with cgo
(INTEGRATION.md).

Arrays may be numpy (host) or torch CUDA tensors (device, zero-copy: the
call then passes PHIP_DEVICE_PTRS).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import (DEVICE_PTRS, phip_config, phip_msgs, phip_ops, phip_results, phip_state,
                   phip_take_reply, phip_wire)


class PatrolHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpatrolhip error {code} ({_lib.PHIP_ERR.get(code, '?')}): {msg}")
        self.code = code


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


def _names_len(names, names_len=None):
    """phip_msgs / phip_ops names_len of a device names blob: the length the
    device checks every name offset against (patrolhip.h), by default the
    blob's own size; 0 (or a blob past 4 GiB) leaves the offsets unchecked."""
    if names_len is not None:
        return int(names_len)
    nb = int(names.numel() * names.element_size()) if _is_torch(names) else int(names.nbytes)
    return nb if 0 < nb < (1 << 32) else 0


def _np(x, dtype):
    if x is None:
        return None
    a = np.ascontiguousarray(x, dtype=dtype)
    return a if a.size else np.zeros(1, dtype)


def names_blob(names: Sequence[bytes]):
    """list[bytes] -> (blob uint8 (8 bytes of read slack), offsets uint32[n+1])."""
    offs = np.zeros(len(names) + 1, dtype=np.uint32)
    if len(names):
        offs[1:] = np.cumsum(np.fromiter((len(x) for x in names), np.int64, len(names)))
    blob = np.zeros(int(offs[-1]) + 8, dtype=np.uint8)
    if offs[-1]:
        blob[:offs[-1]] = np.frombuffer(b"".join(names), dtype=np.uint8)
    return blob, offs


def _evict_flags(shrink: bool, dry_run: bool) -> int:
    return (_lib.EVICT_SHRINK if shrink else 0) | (_lib.EVICT_DRY_RUN if dry_run else 0)


def _evict_dict(st) -> dict:
    return {k: int(getattr(st, k)) for k, _ in _lib.phip_evict_stats._fields_}


def _part_mask(log2_parts: int, mask):
    """A partition mask as the uint64 words phip_export_sweep_parts reads
    (max(1, 2^k / 64) of them; shorter input is an error, not an over-read)."""
    m = np.ascontiguousarray(mask, np.uint64)
    k = int(log2_parts)
    if 0 <= k <= _lib.DIGEST_MAX_LOG2_PARTS and m.size < max(1, (1 << k) // 64):
        raise ValueError("partition mask shorter than 2^log2_parts bits")
    return m if m.size else np.zeros(1, np.uint64)


def _digest_entries(d):
    """(sum, count[, stats]) -> (interleaved uint64[2^k, 2], k)."""
    s, c = np.asarray(d[0], np.uint64), np.asarray(d[1], np.uint64)
    k = int(s.size).bit_length() - 1
    if s.size != c.size or s.size != 1 << k or k > _lib.DIGEST_MAX_LOG2_PARTS:
        raise ValueError("a digest is 2^k sums and 2^k counts, k <= 20")
    return np.ascontiguousarray(np.stack([s, c], axis=1)), k


def digest_diff(a, b):
    """phip_digest_diff of two digests (sum, count) of one level: -> (mask
    uint64 words, bit p set iff partition p differs; how many differ).  The
    mask goes into export_sweep(parts=(log2_parts, mask))."""
    (ea, k), (eb, kb) = _digest_entries(a), _digest_entries(b)
    if k != kb:
        raise ValueError("digest_diff: the digests are of different levels")
    mask = np.zeros(max(1, (1 << k) // 64), np.uint64)
    nd = C.c_uint64()
    rc = _lib.load().phip_digest_diff(ea.ctypes.data, eb.ctypes.data, k, mask.ctypes.data,
                                      C.byref(nd))
    if rc:
        raise PatrolHipError(rc, "phip_digest_diff")
    return mask, int(nd.value)


def digest_fold(d, log2_out: int):
    """phip_digest_fold: the digest (sum, count) at the coarser level
    log2_out (entry p = entries 2p + 2p+1 of the level below)."""
    e, k = _digest_entries(d)
    rc = _lib.load().phip_digest_fold(e.ctypes.data, k, int(log2_out), e.ctypes.data)   # in place
    if rc:
        raise PatrolHipError(rc, "phip_digest_fold: log2_out above the digest's level")
    n = 1 << int(log2_out)
    return np.ascontiguousarray(e[:n, 0]), np.ascontiguousarray(e[:n, 1])


@dataclass
class BucketState:
    """A Bucket's replicated fields plus its local `created` (bucket.go:20-32)."""
    added: int      # float64 bits
    taken: int      # float64 bits
    elapsed: int    # ns
    created: int    # ns since the Unix epoch

    @property
    def added_f(self) -> float:
        return float(np.array([self.added], np.uint64).view(np.float64)[0])

    @property
    def taken_f(self) -> float:
        return float(np.array([self.taken], np.uint64).view(np.float64)[0])


class GPURepo:
    """A device-resident bucket map (the LocalRepo of repo.go:171-235)."""

    def __init__(self, device: int = 0, log2_slots: int = 20, arena_bytes: int = 1 << 24,
                 max_load_pct: int = 90, debug_tag_bits: int = 0, grow: bool = True,
                 small: bool = True, hash_seed: int | None = None, isolate: bool = False,
                 classify_first: bool = False, track_changes: bool = False,
                 track_usage: bool = False):
        """hash_seed: None = a random placement seed per handle (the default,
        as Go's map seeds its hash per process); an int pins it
        (PHIP_CFG_FIXED_SEED; 0 = the unseeded placement).  isolate: set every
        Receive batch's dirty buckets apart (PHIP_CFG_ISOLATE; by default only
        after a dirty batch).  classify_first: classify every decoded Receive
        batch before merging it instead of merging optimistically
        (PHIP_CFG_CLASSIFY_FIRST; same results).  track_changes: keep the change
        set export_changed drains (PHIP_CFG_TRACK_CHANGES).  track_usage: keep
        the usage baseline of usage_mark() and top(metric=1)
        (PHIP_CFG_TRACK_USAGE; 8 bytes a slot)."""
        self.L = _lib.load()
        flags = (0 if grow else _lib.CFG_NO_GROW) | (0 if small else _lib.CFG_NO_SMALL)
        if isolate:
            flags |= _lib.CFG_ISOLATE
        if classify_first:
            flags |= _lib.CFG_CLASSIFY_FIRST
        if track_changes:
            flags |= _lib.CFG_TRACK_CHANGES
        if track_usage:
            flags |= _lib.CFG_TRACK_USAGE
        if hash_seed is not None:
            flags |= _lib.CFG_FIXED_SEED
        cfg = phip_config(device, log2_slots, arena_bytes, max_load_pct, debug_tag_bits, flags, 0,
                          (hash_seed or 0) & (2**64 - 1))
        h = C.c_void_p()
        rc = self.L.phip_open(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise PatrolHipError(rc, "phip_open failed")
        self.h = h
        self.device = device
        self.owned = True

    @classmethod
    def wrap(cls, handle, device: int):
        """A GPURepo over a handle someone else owns (a GPUGroup member)."""
        r = cls.__new__(cls)
        r.L, r.h, r.device, r.owned = _lib.load(), C.c_void_p(handle), device, False
        return r

    # ------------------------------------------------------------ basics --
    def close(self):
        if getattr(self, "h", None) and getattr(self, "owned", True):
            self.L.phip_close(self.h)
        self.h = None
        self._queued = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.L.phip_len(self.h))

    @property
    def capacity(self) -> int:
        return int(self.L.phip_capacity(self.h))

    def _check(self, rc: int, allow=()):
        if rc < 0 and rc not in allow:
            raise PatrolHipError(rc, self.L.phip_last_error(self.h).decode(errors="replace"))
        return rc

    def flush(self):
        rc = self.L.phip_flush(self.h)
        self._queued = None   # the queued batch is finished (or failed)
        self._check(rc)

    def set_stream(self, stream=None):
        """Run the handle's work on `stream` (a torch.cuda.Stream, a raw
        hipStream_t int, or None for the handle's own stream).  Device-pointer
        calls whose inputs torch produces on that stream then need no
        synchronisation between the two."""
        raw = getattr(stream, "cuda_stream", stream)
        self._check(self.L.phip_set_stream(self.h, C.c_void_p(raw) if raw else None))

    def use_torch_stream(self):
        """set_stream(torch's current stream on this device).  torch's default
        stream has the handle 0, which means "the handle's own stream" here:
        make a dedicated torch stream current first (torch.cuda.set_stream)."""
        import torch
        s = torch.cuda.current_stream(self.device)
        if not s.cuda_stream:
            raise ValueError("torch's current stream is the default stream; set a torch.cuda.Stream first")
        self.set_stream(s)

    def set_timing(self, on, accumulate: bool = False):
        """Event timing per kernel; accumulate=True keeps every call's
        timings until timings() is read (for a timed loop)."""
        self.L.phip_set_timing(self.h, (2 if accumulate else 1) if on else 0)

    def last_stats(self):
        """(hot-directory entries, messages folded through it, misses) of the
        last fast-path Receive batch, the table's growths since open, and the
        batch's messages that went through the ordered path; then the undo-log
        entries of the last optimistic pass and its messages that found the
        log full; then the passes the batch's hot directory served before it
        (0: built for this batch) and whether its first optimistic kernel
        found its gate shut."""
        out = (C.c_uint64 * 9)()
        k = self.L.phip_last_stats(self.h, out, 9)
        return tuple(int(out[i]) for i in range(k))

    def table_stats(self):
        """dict(buckets, slots, max_probe, sum_probe): probe distances of the
        buckets from their home slots (phip_table_stats)."""
        out = (C.c_uint64 * 4)()
        k = self._check(self.L.phip_table_stats(self.h, out, 4))
        keys = ("buckets", "slots", "max_probe", "sum_probe")
        return {keys[i]: int(out[i]) for i in range(k)}

    def timings(self, max_entries: int = 1 << 14):
        names = (C.c_char_p * max_entries)()
        ms = (C.c_float * max_entries)()
        k = self.L.phip_last_timings(self.h, names, ms, max_entries)
        return [(names[i].decode(), float(ms[i])) for i in range(k)]

    # -------------------------------------------------------------- repo --
    def seed(self, names: Sequence[bytes], added, taken, elapsed, created):
        """NewLocalRepo(clock, bs...) (repo.go:179-185): buckets as given."""
        blob, offs = names_blob(names)
        n = len(names)
        st = np.zeros(max(n, 1), dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
        st["a"][:n], st["t"][:n] = np.asarray(added, np.uint64), np.asarray(taken, np.uint64)
        st["e"][:n], st["c"][:n] = np.asarray(elapsed, np.int64), np.asarray(created, np.int64)
        self._check(self.L.phip_seed(self.h, blob.ctypes.data, offs.ctypes.data, n,
                                     st.ctypes.data, 0))

    def seed_device(self, names, name_offs, states, n: int):
        """phip_seed with device pointers: names (uint8 CUDA tensor), name_offs
        (n+1 int32/uint32), states (n x 4 int64: added bits, taken bits,
        elapsed, created)."""
        self._check(self.L.phip_seed(self.h, _ptr(names), _ptr(name_offs), n, _ptr(states),
                                     DEVICE_PTRS))

    def get(self, name: bytes):
        """Lookup without creating (None when absent)."""
        s = phip_state()
        rc = self._check(self.L.phip_get(self.h, name, len(name), C.byref(s)))
        if rc == 0:
            return None
        return BucketState(s.added, s.taken, s.elapsed, s.created)

    def export_datagrams(self, names: Sequence[bytes]):
        """Egress batch: each named bucket's current state as its MarshalBinary
        datagram (bucket.go:51-68).  -> (list of datagrams, found uint8[n]);
        an absent bucket's datagram is zero bytes."""
        n = len(names)
        blob, offs = names_blob(names)
        out = np.zeros(25 * n + int(offs[-1]) + 1, np.uint8)
        found = np.zeros(max(n, 1), np.uint8)
        self._check(self.L.phip_export_datagrams(self.h, blob.ctypes.data, offs.ctypes.data, n,
                                                 out.ctypes.data, found.ctypes.data, 0))
        raw = out.tobytes()
        dgs = [raw[25 * i + int(offs[i]):25 * (i + 1) + int(offs[i + 1])] for i in range(n)]
        return dgs, found[:n]

    def export_states_device(self, names, name_offs, n: int):
        """phip_export_datagrams with device pointers (names uint8 CUDA tensor,
        name_offs int32[n+1]): each named bucket's MarshalBinary datagram
        (bucket.go:51-68) written on the device, then its three big-endian
        words read back as (added bits, taken bits, elapsed) int64 tensors and
        found (bool), all on the device.  An absent bucket reads as zeros."""
        import torch
        dev = names.device
        offs64 = name_offs.to(torch.int64)
        total = int(offs64[-1] - offs64[0])
        out = torch.zeros(_lib.BUCKET_FIXED_SIZE * max(n, 1) + total + 8, dtype=torch.uint8,
                          device=dev)
        found = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        self._check(self.L.phip_export_datagrams(self.h, _ptr(names), _ptr(name_offs), n,
                                                 _ptr(out), _ptr(found), DEVICE_PTRS))
        base = _lib.BUCKET_FIXED_SIZE * torch.arange(n, dtype=torch.int64, device=dev) + \
            (offs64[:-1] - offs64[0])
        words = out[base.unsqueeze(1) + torch.arange(24, device=dev).unsqueeze(0)]   # [n, 24]
        w = words.view(n, 3, 8).flip(2).contiguous().view(torch.int64).view(n, 3)   # big-endian
        return w[:, 0], w[:, 1], w[:, 2], found[:n].bool()

    def snapshot(self, path=None):
        """The table as a raw image (phip_snapshot); written to `path` if given,
        else returned as a uint8 array."""
        nb = int(self.L.phip_snapshot_bytes(self.h))
        if nb == 0:
            raise PatrolHipError(-1, "phip_snapshot_bytes failed")
        buf = np.empty(nb, np.uint8)
        self._check(self.L.phip_snapshot(self.h, buf.ctypes.data, nb))
        if path is None:
            return buf
        buf.tofile(path)
        return None

    def restore(self, src):
        """Load a snapshot (a path or a uint8 array) into this handle, which must
        have the snapshot's log2_slots (phip_restore)."""
        buf = np.fromfile(src, np.uint8) if isinstance(src, (str, bytes, os.PathLike)) else \
            np.ascontiguousarray(src, np.uint8)
        self._check(self.L.phip_restore(self.h, buf.ctypes.data, buf.size))

    def evict_idle(self, now: int, idle_ns: int, min_evict: int = 1, shrink: bool = False,
                   dry_run: bool = False) -> dict:
        """Evict every bucket idle for idle_ns or longer (phip_evict_idle):
        idle = now - (created + elapsed), exact, 0 when negative.  An evicted
        bucket is recreated by its next GetBucket (PHIP_ST_CREATED), as after
        a node restart in the reference (repo.go:96-106); keep idle_ns >= per
        of every rate served and its first Take answers as it would have.
        Fewer than min_evict idle buckets, or dry_run, only counts.  shrink
        also picks a smaller table.  -> dict(idle, evicted, buckets, slots,
        arena_used, arena_freed)."""
        st = _lib.phip_evict_stats()
        rc = self.L.phip_evict_idle(self.h, int(now), int(idle_ns), int(min_evict), C.byref(st),
                                    _evict_flags(shrink, dry_run))
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        return _evict_dict(st)

    # ------------------------------------------------------------- sweep --
    @staticmethod
    def _sweep_cursor(cursor):
        return _lib.phip_sweep_cursor(*(cursor or (0, 0)))

    @staticmethod
    def _sweep_dict(st) -> dict:
        return {k: int(getattr(st, k)) for k, _ in _lib.phip_sweep_stats._fields_}

    def _sweep_call(self, parts, cur, now, idle_ns, out, out_cap, offs, max_msgs, st, flags):
        """phip_export_sweep, or with parts = (log2_parts, mask uint64 words)
        phip_export_sweep_parts: only the buckets of the partitions whose bit
        is set (digest_diff's mask)."""
        if parts is None:
            return self.L.phip_export_sweep(self.h, C.byref(cur), int(now), int(idle_ns), out,
                                            out_cap, offs, max_msgs, C.byref(st), flags)
        k, mask = int(parts[0]), _part_mask(*parts)
        return self.L.phip_export_sweep_parts(self.h, C.byref(cur), int(now), int(idle_ns), k,
                                              mask.ctypes.data, out, out_cap, offs, max_msgs,
                                              C.byref(st), flags)

    def export_sweep(self, cursor=None, max_msgs: int = 1 << 16, out_cap: int | None = None,
                     now: int = 0, idle_ns: int = 0, parts=None):
        """One call of the anti-entropy sweep (phip_export_sweep): the next
        window of the table as MarshalBinary datagrams (bucket.go:51-68), at
        most max_msgs of them in at most out_cap bytes (default 256 each).
        Zero states are skipped; idle_ns > 0 also skips the buckets
        evict_idle(now, idle_ns) would evict; parts = (log2_parts, mask) keeps
        only the partitions digest_diff marked (phip_export_sweep_parts).
        cursor: None to start, then the one the last call returned.
        -> (datagrams, cursor, stats dict(n, bytes, slots_scanned, done,
        restarted)); loop until stats["done"]."""
        if out_cap is None:
            out_cap = _lib.PACKET_SIZE * max_msgs
        cur, st = self._sweep_cursor(cursor), _lib.phip_sweep_stats()
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        offs = np.zeros(int(max_msgs) + 1, np.uint64)
        rc = self._sweep_call(parts, cur, now, idle_ns, out.ctypes.data, int(out_cap),
                              offs.ctypes.data, int(max_msgs), st, 0)
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        raw = out[:int(st.bytes)].tobytes()
        dgs = [raw[int(offs[i]):int(offs[i + 1])] for i in range(int(st.n))]
        d = self._sweep_dict(st)
        d["offs"] = offs[:int(st.n) + 1]
        return dgs, (int(cur.slot), int(cur.layout)), d

    def export_sweep_device(self, out, offs, cursor, max_msgs: int, now: int = 0,
                            idle_ns: int = 0, parts=None):
        """phip_export_sweep with device pointers: out (uint8 CUDA tensor, 8-byte
        aligned, a multiple of 8 bytes; the byte budget is its size - 8), offs
        (int64[max_msgs + 1]).  Both can go unchanged into another repo's
        receive_datagrams_device.  parts as in export_sweep (the mask stays
        host memory).  -> (n, cursor, stats dict)."""
        cur, st = self._sweep_cursor(cursor), _lib.phip_sweep_stats()
        cap = int(out.numel() * out.element_size())
        rc = self._sweep_call(parts, cur, now, idle_ns, _ptr(out), cap, _ptr(offs), int(max_msgs),
                              st, DEVICE_PTRS)
        self._queued = None
        self._check(rc)
        return int(st.n), (int(cur.slot), int(cur.layout)), self._sweep_dict(st)

    def sweep_count(self, now: int = 0, idle_ns: int = 0, parts=None) -> dict:
        """What a whole sweep under this filter would write (PHIP_SWEEP_COUNT):
        dict(n, bytes, ...), to size buffers by."""
        cur, st = _lib.phip_sweep_cursor(), _lib.phip_sweep_stats()
        rc = self._sweep_call(parts, cur, now, idle_ns, None, 0, None, 0, st, _lib.SWEEP_COUNT)
        self._queued = None
        self._check(rc)
        return self._sweep_dict(st)

    def sweep(self, max_msgs: int = 1 << 16, out_cap: int | None = None, now: int = 0,
              idle_ns: int = 0, parts=None):
        """Generator over a whole sweep: yields (datagrams, stats) per call
        until the cursor reaches the end of the table (a rebuild in between
        starts it over, stats["restarted"])."""
        cursor = None
        while True:
            dgs, cursor, st = self.export_sweep(cursor, max_msgs, out_cap, now, idle_ns, parts)
            yield dgs, st
            if st["done"]:
                return

    # --------------------------------------------------------- throttled --
    def _throttled_call(self, rules, cur, now, min_wait_ns, out, st, flags):
        arr = _throttle_rules(rules)
        rc = self.L.phip_export_throttled(self.h, C.byref(cur), arr, len(arr), int(now),
                                          int(min_wait_ns), out, C.byref(st), flags)
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)

    def export_throttled(self, rules, now: int, min_wait_ns: int = 0, cursor=None,
                         max_entries: int = 1 << 16, names_cap: int | None = None) -> dict:
        """One call of the throttled sweep (phip_export_throttled): the buckets
        of the next window of the table that their rule's rate denies at `now`
        and still denies min_wait_ns later.  rules: a sequence of (prefix bytes
        of at most 16, freq, per, count); the first rule whose prefix a name
        starts with gives its query, and a bucket no rule matches is not
        reported.  At most max_entries entries and names_cap name bytes
        (default 231 each).  cursor: None to start, then the one the last call
        returned.  -> dict(names list[bytes], retry_at int64 (the least later
        clock reading that grants, or PEEK_NEVER), remaining uint64, rule
        uint8, cursor, n, bytes, slots_scanned, done, restarted); loop until
        done."""
        if names_cap is None:
            names_cap = _lib.MAX_NAME_LEN * max_entries
        cur, st = self._sweep_cursor(cursor), _lib.phip_sweep_stats()
        z = max(int(max_entries), 1)
        names = np.zeros(max(int(names_cap), 1), np.uint8)
        offs = np.zeros(z + 1, np.uint64)
        at, rem, rule = np.zeros(z, np.int64), np.zeros(z, np.uint64), np.zeros(z, np.uint8)
        out = _lib.phip_throttled_out(_ptr(names), int(names_cap), _ptr(offs), int(max_entries), 0,
                                      _ptr(at), _ptr(rem), _ptr(rule))
        self._throttled_call(rules, cur, now, min_wait_ns, C.byref(out), st, 0)
        n = int(st.n)
        raw = names[:int(st.bytes)].tobytes()
        d = self._sweep_dict(st)
        d.update(names=[raw[int(offs[i]):int(offs[i + 1])] for i in range(n)], retry_at=at[:n],
                 remaining=rem[:n], rule=rule[:n], cursor=(int(cur.slot), int(cur.layout)))
        return d

    def export_throttled_device(self, rules, now: int, names, offs, cursor, max_entries: int,
                                min_wait_ns: int = 0, retry_at=None, remaining=None, rule=None):
        """phip_export_throttled with device pointers: names (uint8 CUDA tensor,
        every byte of it is budget), offs (int64[max_entries + 1]) and the
        columns wanted (retry_at / remaining int64[max_entries], rule
        uint8[max_entries]); the rules stay host memory.
        -> (n, cursor, stats dict)."""
        cur, st = self._sweep_cursor(cursor), _lib.phip_sweep_stats()
        cap = int(names.numel() * names.element_size())
        out = _lib.phip_throttled_out(_ptr(names), cap, _ptr(offs), int(max_entries), 0,
                                      _ptr(retry_at), _ptr(remaining), _ptr(rule))
        self._throttled_call(rules, cur, now, min_wait_ns, C.byref(out), st, DEVICE_PTRS)
        return int(st.n), (int(cur.slot), int(cur.layout)), self._sweep_dict(st)

    def throttled_count(self, rules, now: int, min_wait_ns: int = 0) -> dict:
        """What a whole throttled sweep would report (PHIP_SWEEP_COUNT):
        dict(n, bytes (name bytes), ...), to size buffers by."""
        cur, st = _lib.phip_sweep_cursor(), _lib.phip_sweep_stats()
        self._throttled_call(rules, cur, now, min_wait_ns, None, st, _lib.SWEEP_COUNT)
        return self._sweep_dict(st)

    def throttled(self, rules, now: int, min_wait_ns: int = 0, max_entries: int = 1 << 16,
                  names_cap: int | None = None):
        """Generator over a whole throttled sweep: yields export_throttled's
        dict per call until the cursor reaches the end of the table (a rebuild
        in between starts it over, "restarted")."""
        cursor = None
        while True:
            d = self.export_throttled(rules, now, min_wait_ns, cursor, max_entries, names_cap)
            cursor = d["cursor"]
            yield d
            if d["done"]:
                return

    # -------------------------------------------------------- top talkers --
    def _top_call(self, k, prefix, now, idle_ns, out, flags, metric=0):
        prefix = bytes(prefix)
        q = _lib.phip_top_query()
        head = prefix[:_lib.THROTTLE_MAX_PREFIX]   # (a longer one keeps its length: refused)
        q.prefix[:len(head)] = list(head)
        q.prefix_len, q.metric, q.now, q.idle_ns, q.k = len(prefix), int(metric), int(now), \
            int(idle_ns), int(k)
        st = _lib.phip_top_stats()
        rc = self.L.phip_export_top(self.h, C.byref(q), out, C.byref(st), flags)
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        return {f: int(getattr(st, f)) for f, _ in _lib.phip_top_stats._fields_}

    def top(self, k: int, prefix: bytes = b"", now: int = 0, idle_ns: int = 0,
            names_cap: int | None = None, state: bool = False, metric: int = 0,
            mark: bool = False) -> dict:
        """phip_export_top: the k buckets with the largest `taken` among those
        whose name starts with `prefix` (at most 16 bytes) and, with idle_ns >
        0, that evict_idle's rule does not call idle at `now`; only positive
        `taken` (+Inf included) ranks.  By `taken` descending, equal values in
        slot order.  -> dict(names list[bytes], taken uint64 (float64 bits),
        state (None, or a structured array a/t/e/c), n, bytes, population (the
        buckets that qualified), passes (kernels that read the whole table),
        truncated (names_cap, default 231 * k, cut the list)).

        On a repo opened with track_usage=True: metric=1 (PHIP_TOP_SINCE_MARK)
        ranks by `taken` since the last usage mark, and the taken column then
        holds that difference (state["t"] stays the current total);
        mark=True (PHIP_TOP_MARK) marks the whole table behind the list, in
        the same call."""
        z = max(int(k), 1)
        if names_cap is None:
            names_cap = _lib.MAX_NAME_LEN * z
        names = np.zeros(max(int(names_cap), 1), np.uint8)
        offs = np.zeros(z + 1, np.uint64)
        taken = np.zeros(z, np.uint64)
        sta = np.zeros(z, dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")]) \
            if state else None
        out = _lib.phip_top_out(_ptr(names), int(names_cap), _ptr(offs), _ptr(taken), _ptr(sta))
        d = self._top_call(k, prefix, now, idle_ns, C.byref(out), _lib.TOP_MARK if mark else 0,
                           metric)
        n = d["n"]
        raw = names[:d["bytes"]].tobytes()
        d.update(names=[raw[int(offs[i]):int(offs[i + 1])] for i in range(n)], taken=taken[:n],
                 state=None if sta is None else sta[:n])
        return d

    def top_device(self, k: int, names, offs, taken=None, state=None, prefix: bytes = b"",
                   now: int = 0, idle_ns: int = 0, metric: int = 0, mark: bool = False) -> dict:
        """phip_export_top with device pointers: names (uint8 CUDA tensor, every
        byte of it is budget), offs (int64[k + 1]), taken (int64[k]) and state
        (int64[k, 4]) where wanted; metric and mark as in top().  -> the stats
        dict."""
        cap = int(names.numel() * names.element_size())
        out = _lib.phip_top_out(_ptr(names), cap, _ptr(offs), _ptr(taken), _ptr(state))
        return self._top_call(k, prefix, now, idle_ns, C.byref(out),
                              DEVICE_PTRS | (_lib.TOP_MARK if mark else 0), metric)

    def top_count(self, prefix: bytes = b"", now: int = 0, idle_ns: int = 0,
                  metric: int = 0) -> dict:
        """How many buckets qualify for top() (PHIP_SWEEP_COUNT): one pass,
        dict(population, passes, ...).  metric=1: the buckets active since the
        mark."""
        return self._top_call(1, prefix, now, idle_ns, None, _lib.SWEEP_COUNT, metric)

    def usage_mark(self, flags: int = 0) -> dict:
        """phip_usage_mark on a repo opened with track_usage=True: every
        bucket's `taken` becomes its baseline for top(metric=1).  ->
        dict(buckets, the published records baselined; active, of those the
        ones that took anything since the previous mark)."""
        st = _lib.phip_usage_stats()
        rc = self.L.phip_usage_mark(self.h, C.byref(st), int(flags))
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        return dict(buckets=int(st.buckets), active=int(st.active))

    # -------------------------------------------------------- change set --
    @staticmethod
    def _changes_dict(st) -> dict:
        return {k: int(getattr(st, k)) for k, _ in _lib.phip_changes_stats._fields_}

    def export_changed(self, max_msgs: int = 1 << 16, out_cap: int | None = None) -> dict:
        """One call of phip_export_changed on a repo opened with
        track_changes=True: the replication traffic of the buckets this repo's
        own TAKE / UPSERT ops touched since they were last exported, at most
        max_msgs datagrams in at most out_cap bytes (default 256 each), and
        their marks cleared.  -> dict(data uint8, offs uint64[n + 1], n,
        n_incast, bytes, pending, done): datagram i = data[offs[i]:offs[i+1]],
        the incast requests [0, n_incast) first, then one state datagram per
        bucket; loop until done (drain_changes)."""
        if out_cap is None:
            out_cap = _lib.PACKET_SIZE * max_msgs
        st = _lib.phip_changes_stats()
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        offs = np.zeros(int(max_msgs) + 1, np.uint64)
        rc = self.L.phip_export_changed(self.h, out.ctypes.data, int(out_cap), offs.ctypes.data,
                                        int(max_msgs), C.byref(st), 0)
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        d = self._changes_dict(st)
        d["data"], d["offs"] = out[:int(st.bytes)], offs[:int(st.n) + 1]
        return d

    def export_changed_device(self, out, offs, max_msgs: int) -> dict:
        """phip_export_changed with device pointers: out (uint8 CUDA tensor,
        8-byte aligned, a multiple of 8 bytes; the byte budget is its size - 8),
        offs (int64[max_msgs + 1]).  Both can go unchanged into another repo's
        receive_datagrams_device.  -> dict(n, n_incast, bytes, pending, done)."""
        st = _lib.phip_changes_stats()
        cap = int(out.numel() * out.element_size())
        rc = self.L.phip_export_changed(self.h, _ptr(out), cap, _ptr(offs), int(max_msgs),
                                        C.byref(st), DEVICE_PTRS)
        self._queued = None
        self._check(rc)
        return self._changes_dict(st)

    def changes_count(self) -> dict:
        """What a full drain would write now (PHIP_SWEEP_COUNT): dict(n,
        n_incast, bytes, pending, done); nothing is cleared."""
        st = _lib.phip_changes_stats()
        rc = self.L.phip_export_changed(self.h, None, 0, None, 0, C.byref(st), _lib.SWEEP_COUNT)
        self._queued = None
        self._check(rc)
        return self._changes_dict(st)

    def drain_changes(self, max_msgs: int = 1 << 16, out_cap: int | None = None):
        """Generator over a whole drain: yields export_changed's dict per call
        until nothing is pending."""
        while True:
            d = self.export_changed(max_msgs, out_cap)
            yield d
            if d["done"]:
                return

    # ------------------------------------------------------------ digest --
    def digest(self, log2_parts: int):
        """Partition digests of the table (phip_table_digest): per partition of
        the name space the sum of a hash of every bucket a sweep would export
        and their number.  -> (sum uint64[2^k], count uint64[2^k], stats
        dict(records, bytes, slots_scanned)).  Two replicas compare them with
        digest_diff and sweep only what differs (export_sweep(parts=...))."""
        k = int(log2_parts)
        out = np.zeros((1 << min(max(k, 0), _lib.DIGEST_MAX_LOG2_PARTS), 2), np.uint64)
        st = _lib.phip_digest_stats()
        rc = self.L.phip_table_digest(self.h, k, out.ctypes.data, C.byref(st), 0)
        self._queued = None   # a queued batch is finished (or failed)
        self._check(rc)
        return (np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1]),
                {f: int(getattr(st, f)) for f, _ in _lib.phip_digest_stats._fields_})

    def digest_device(self, out, log2_parts: int) -> dict:
        """phip_table_digest with device pointers: out, an int64 CUDA tensor of
        2^log2_parts (sum, count) pairs.  -> stats dict."""
        k = int(log2_parts)
        if out.numel() * out.element_size() < 16 << k:
            raise ValueError("digest_device: out holds fewer than 2^log2_parts entries")
        st = _lib.phip_digest_stats()
        rc = self.L.phip_table_digest(self.h, k, _ptr(out), C.byref(st), DEVICE_PTRS)
        self._queued = None
        self._check(rc)
        return {f: int(getattr(st, f)) for f, _ in _lib.phip_digest_stats._fields_}

    def dump_arrays(self):
        """Every bucket as arrays (unordered): (names uint8, offs uint64[n+1],
        added bits, taken bits, elapsed, created) -- for tables too large for
        a dict."""
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self.L.phip_dump(self.h, None, 0, None, None, 0, C.byref(n), C.byref(nb)))
        cnt = n.value
        names = np.zeros(max(nb.value, 1), np.uint8)
        offs = np.zeros(cnt + 1, np.uint64)
        st = np.zeros(max(cnt, 1), dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
        self._check(self.L.phip_dump(self.h, names.ctypes.data, names.size, offs.ctypes.data,
                                     st.ctypes.data, cnt, C.byref(n), C.byref(nb)))
        st = st[:n.value]
        return (names, offs[:n.value + 1], np.ascontiguousarray(st["a"]),
                np.ascontiguousarray(st["t"]), np.ascontiguousarray(st["e"]),
                np.ascontiguousarray(st["c"]))

    def dump(self):
        """{name: BucketState} of every bucket."""
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self.L.phip_dump(self.h, None, 0, None, None, 0, C.byref(n), C.byref(nb)))
        cnt = n.value
        names = np.zeros(max(nb.value, 1), np.uint8)
        offs = np.zeros(cnt + 1, np.uint64)
        st = np.zeros(max(cnt, 1), dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
        self._check(self.L.phip_dump(self.h, names.ctypes.data, names.size, offs.ctypes.data,
                                     st.ctypes.data, cnt, C.byref(n), C.byref(nb)))
        raw = names.tobytes()
        return {raw[int(offs[i]):int(offs[i + 1])]:
                BucketState(int(st["a"][i]), int(st["t"][i]), int(st["e"][i]), int(st["c"][i]))
                for i in range(n.value)}

    # ---------------------------------------------------------- hot path --
    @staticmethod
    def _results(n, want_remaining=False, want_reply=False):
        status = np.zeros(max(n, 1), np.uint8)
        rem = np.zeros(max(n, 1), np.uint64) if want_remaining else None
        have = np.zeros(max(n, 1), np.uint64) if want_remaining else None
        reply = (np.zeros(max(n, 1), dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
                 if want_reply else None)
        res = phip_results(status.ctypes.data, _ptr(rem), _ptr(have), _ptr(reply))
        return res, status, rem, have, reply

    def receive_datagrams(self, datagrams: Sequence[bytes], now: int):
        """ReplicatedRepo.Receive over raw datagrams (repo.go:54-92).

        Returns dict(status, reply, stop) — `stop` is the index of the first
        malformed datagram (the Go loop returns io.ErrShortBuffer there) or n.
        """
        n = len(datagrams)
        offs = np.zeros(n + 1, np.uint64)
        if n:
            offs[1:] = np.cumsum([len(d) for d in datagrams])
        blob = np.zeros(int(offs[-1]) + 8, np.uint8)
        if offs[-1]:
            blob[:offs[-1]] = np.frombuffer(b"".join(datagrams), np.uint8)
        res, status, _, _, reply = self._results(n, want_reply=True)
        stop = C.c_uint32()
        self._check(self.L.phip_receive_datagrams(self.h, blob.ctypes.data, offs.ctypes.data, n,
                                                  int(now), C.byref(res), C.byref(stop), 0),
                    allow=(-5,))
        return dict(status=status[:n], reply=reply[:n], stop=stop.value)

    def receive_datagrams_device(self, data, offs, n: int, now: int, status=None):
        """phip_receive_datagrams with device pointers: data (uint8 CUDA tensor
        of back-to-back datagrams, 8 bytes of slack), offs (int64[n+1]).
        Returns the index of the first malformed datagram (n if none)."""
        res = phip_results(_ptr(status), None, None, None)
        stop = C.c_uint32(0)
        rc = self.L.phip_receive_datagrams(self.h, _ptr(data), _ptr(offs), n, int(now),
                                           C.byref(res), C.byref(stop), DEVICE_PTRS)
        if rc not in (0, -5):
            self._check(rc)
        return stop.value

    def receive_soa(self, names, added, taken, elapsed, now: int, name_offs=None, n=None,
                    status=None, device=False, reply=None, queue=False, names_len=None):
        """Receive over decoded states.  With device=True every array is a torch
        CUDA tensor (names = uint8 blob, name_offs = int32/uint32 offsets;
        reply: an int64 [n, 4] tensor for the phip_state replies).
        queue=True (device only): PHIP_RECV_ASYNC, the batch is finished by
        the handle's next call or flush(); the binding holds the batch's
        tensors until the next receive or flush(), so that the caching
        allocator cannot hand their memory to another tensor meanwhile.
        names_len (device only): the blob length the device checks the name
        offsets against (phip_msgs.names_len); default the blob's size, 0 =
        unchecked."""
        fl = _lib.RECV_ASYNC if queue else 0
        if device:
            m = phip_msgs(n, _names_len(names, names_len), _ptr(names), _ptr(name_offs),
                          _ptr(added), _ptr(taken), _ptr(elapsed))
            res = phip_results(_ptr(status), None, None, _ptr(reply))
            rc = self.L.phip_receive_soa(self.h, C.byref(m), int(now), C.byref(res),
                                         DEVICE_PTRS | fl)
            self._queued = ((names, name_offs, added, taken, elapsed, status, reply)
                            if queue and rc == 0 else None)
            self._check(rc)
            return None
        n = len(names)
        blob, offs = names_blob(names)
        a, t, e = _np(added, np.uint64), _np(taken, np.uint64), _np(elapsed, np.int64)
        m = phip_msgs(n, 0, blob.ctypes.data, offs.ctypes.data, a.ctypes.data, t.ctypes.data,
                      e.ctypes.data)
        res, st, _, _, reply = self._results(n, want_reply=True)
        self._check(self.L.phip_receive_soa(self.h, C.byref(m), int(now), C.byref(res), fl))
        return dict(status=st[:n], reply=reply[:n])

    # -- incast reply egress (patrolhip.h "Incast reply egress") --
    @staticmethod
    def _reply_host(n, max_msgs, out_cap):
        """Host buffers of a phip_reply_egress for a batch of n messages (by
        default caps no batch's replies reach)."""
        max_msgs = max(n, 1) if max_msgs is None else int(max_msgs)
        out_cap = _lib.PACKET_SIZE * max(max_msgs, 1) if out_cap is None else int(out_cap)
        out = np.zeros(max(out_cap, 8), np.uint8)
        offs = np.zeros(max_msgs + 1, np.uint64)
        src = np.zeros(max(max_msgs, 1), np.uint32)
        rq = _lib.phip_reply_egress(out.ctypes.data, out_cap, offs.ctypes.data, src.ctypes.data,
                                    max_msgs, 0, 0, 0, 0)
        return rq, out, offs, src

    @staticmethod
    def _reply_dict(rq, status, out, offs, src, rc=0, **more):
        """dict(status, data, offs, src, n, replies, skipped, bytes[, stop]); host
        buffers are cut to what was written, device tensors returned whole."""
        k = int(rq.n)
        if not _is_torch(out):
            out, offs, src = out[:int(rq.bytes)], offs[:k + 1], src[:k]
        return dict(status=status, data=out, offs=offs, src=src, n=k, replies=int(rq.replies),
                    skipped=int(rq.skipped), bytes=int(rq.bytes), rc=rc, **more)

    def receive_soa_replies(self, names, added, taken, elapsed, now: int, max_msgs=None,
                            out_cap=None, want_status: bool = True, classify: bool = False):
        """phip_receive_soa_replies over host arrays: the batch is received as
        receive_soa receives it, and its incast replies come back as
        datagrams (`data` / `offs`) with the batch index each one answers
        (`src`).  No reply column is asked for; want_status=False asks for
        no column at all."""
        n = len(names)
        blob, noffs = names_blob(names)
        a, t, e = _np(added, np.uint64), _np(taken, np.uint64), _np(elapsed, np.int64)
        m = phip_msgs(n, 0, blob.ctypes.data, noffs.ctypes.data, a.ctypes.data, t.ctypes.data,
                      e.ctypes.data)
        res, st, _, _, _ = self._results(n)
        rq, out, offs, src = self._reply_host(n, max_msgs, out_cap)
        self._check(self.L.phip_receive_soa_replies(
            self.h, C.byref(m), int(now), C.byref(res) if want_status else None, C.byref(rq),
            _lib.RECV_CLASSIFY if classify else 0))
        return self._reply_dict(rq, st[:n] if want_status else None, out, offs, src)

    def receive_soa_replies_device(self, n: int, names, name_offs, added, taken, elapsed, now: int,
                                   out, offs, src, max_msgs: int, out_cap=None, status=None,
                                   reply=None, names_len=None, flags: int = 0, allow=()):
        """phip_receive_soa_replies with device pointers: the batch's columns
        as receive_soa(device=True) takes them; out (uint8, 8-byte aligned),
        offs (int64[max_msgs + 1]) and src (int32[max_msgs], or None) are CUDA
        tensors.  status / reply: optional result columns.  `allow`: return
        codes handed back in `rc` instead of raised (a stopped batch's)."""
        m = phip_msgs(n, _names_len(names, names_len), _ptr(names), _ptr(name_offs),
                      _ptr(added), _ptr(taken), _ptr(elapsed))
        res = phip_results(_ptr(status), None, None, _ptr(reply))
        cap = int(out.numel()) if out_cap is None else int(out_cap)
        rq = _lib.phip_reply_egress(_ptr(out), cap, _ptr(offs), _ptr(src), int(max_msgs), 0, 0, 0, 0)
        rc = self.L.phip_receive_soa_replies(
            self.h, C.byref(m), int(now),
            C.byref(res) if (status is not None or reply is not None) else None, C.byref(rq),
            DEVICE_PTRS | flags)
        self._check(rc, allow=allow)
        return self._reply_dict(rq, status, out, offs, src, rc=rc)

    def receive_datagrams_replies(self, datagrams: Sequence[bytes], now: int, max_msgs=None,
                                  out_cap=None, want_status: bool = True):
        """phip_receive_datagrams_replies over host datagrams -> the reply
        dict of receive_soa_replies plus `stop` (receive_datagrams)."""
        n = len(datagrams)
        doffs = np.zeros(n + 1, np.uint64)
        if n:
            doffs[1:] = np.cumsum([len(d) for d in datagrams])
        blob = np.zeros(int(doffs[-1]) + 8, np.uint8)
        if doffs[-1]:
            blob[:doffs[-1]] = np.frombuffer(b"".join(datagrams), np.uint8)
        res, st, _, _, _ = self._results(n)
        rq, out, offs, src = self._reply_host(n, max_msgs, out_cap)
        stop = C.c_uint32()
        rc = self.L.phip_receive_datagrams_replies(
            self.h, blob.ctypes.data, doffs.ctypes.data, n, int(now),
            C.byref(res) if want_status else None, C.byref(stop), C.byref(rq), 0)
        self._check(rc, allow=(-5,))
        return self._reply_dict(rq, st[:n] if want_status else None, out, offs, src, rc=rc,
                                stop=stop.value)

    def receive_datagrams_replies_device(self, data, doffs, n: int, now: int, out, offs, src,
                                         max_msgs: int, out_cap=None, status=None):
        """phip_receive_datagrams_replies with device pointers (data / doffs as
        receive_datagrams_device takes them; out / offs / src as
        receive_soa_replies_device)."""
        res = phip_results(_ptr(status), None, None, None)
        cap = int(out.numel()) if out_cap is None else int(out_cap)
        rq = _lib.phip_reply_egress(_ptr(out), cap, _ptr(offs), _ptr(src), int(max_msgs), 0, 0, 0, 0)
        stop = C.c_uint32(0)
        rc = self.L.phip_receive_datagrams_replies(
            self.h, _ptr(data), _ptr(doffs), n, int(now),
            C.byref(res) if status is not None else None, C.byref(stop), C.byref(rq), DEVICE_PTRS)
        self._check(rc, allow=(-5,))
        return self._reply_dict(rq, status, out, offs, src, rc=rc, stop=stop.value)

    # -- packed frames (patrolhip.h "Packed frames") --
    def _frames_check(self, rc: int, needed: int, allow=()):
        """_check for a frames call: the error carries the count the call
        needs (`needed`: *n_recs_out / *n_frames_out)."""
        try:
            self._check(rc, allow=allow)
        except PatrolHipError as e:
            e.needed = int(needed)
            raise

    def unframe(self, frames, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_recs=None):
        """The host form of phip_unframe (module function `unframe`)."""
        return unframe(frames, frame_bytes, max_recs)

    def unframe_device(self, data, foffs, n_frames: int, rec_offs, rec_frame=None,
                       frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_recs=None,
                       bytes_len=None) -> int:
        """phip_unframe with device pointers: data (uint8 CUDA tensor, 8-byte
        aligned, 8 bytes of slack), foffs (int64[n_frames + 1]); rec_offs
        (int64[max_recs + 1]) and rec_frame (int32[max_recs], optional) are
        written.  bytes_len: the length the frame offsets are checked against
        (default: data's size; 0 = trusted).  -> the record count; on error
        PatrolHipError carries `needed`."""
        max_recs = int(rec_offs.numel()) - 1 if max_recs is None else int(max_recs)
        lim = int(data.numel()) if bytes_len is None else int(bytes_len)
        n = C.c_uint32()
        rc = self.L.phip_unframe(self.h, _ptr(data), _ptr(foffs), int(n_frames), lim,
                                 int(frame_bytes), _ptr(rec_offs), _ptr(rec_frame), max_recs,
                                 C.byref(n), DEVICE_PTRS)
        self._frames_check(rc, n.value)
        return n.value

    def frame_cuts(self, offs, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_frames=None):
        """The host form of phip_frame_cuts (module function `frame_cuts`)."""
        return frame_cuts(offs, frame_bytes, max_frames)

    def frame_cuts_device(self, offs, n: int, frame_offs, frame_first=None,
                          frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_frames=None) -> int:
        """phip_frame_cuts with device pointers: offs (int64[n + 1]) is an
        export's offsets column; frame_offs (int64[max_frames + 1]) and
        frame_first (int32[max_frames], optional) are written.  -> the frame
        count; on error PatrolHipError carries `needed`."""
        max_frames = int(frame_offs.numel()) - 1 if max_frames is None else int(max_frames)
        k = C.c_uint32()
        rc = self.L.phip_frame_cuts(self.h, _ptr(offs), int(n), int(frame_bytes), _ptr(frame_offs),
                                    _ptr(frame_first), max_frames, C.byref(k), DEVICE_PTRS)
        self._frames_check(rc, k.value)
        return k.value

    def receive_frames(self, frames: Sequence[bytes], now: int,
                       frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_recs=None, replies=None):
        """phip_receive_frames over host frames (each a run of whole records):
        -> dict(status, reply, stop, n_recs, rec_frame) as receive_datagrams
        over the frames' records; `stop` is a record index, rec_frame[k] the
        frame of record k.  replies=dict(max_msgs=, out_cap=) (or {}):
        phip_receive_frames_replies -> the reply dict of
        receive_datagrams_replies plus n_recs and rec_frame; its src[] are
        record indices too."""
        blob, foffs = _frames_blob(frames)
        nf = len(frames)
        cap = _frame_bound(int(foffs[-1]), nf) if max_recs is None else int(max_recs)
        rec_frame = np.zeros(max(cap, 1), np.uint32)
        stop, nrec = C.c_uint32(), C.c_uint32()
        if replies is not None:
            res, st, _, _, _ = self._results(cap)
            rq, out, offs, src = self._reply_host(cap, replies.get("max_msgs"),
                                                  replies.get("out_cap"))
            rc = self.L.phip_receive_frames_replies(
                self.h, blob.ctypes.data, foffs.ctypes.data, nf, int(now), C.byref(res),
                C.byref(stop), C.byref(rq), int(frame_bytes), rec_frame.ctypes.data, cap,
                C.byref(nrec), 0)
            self._frames_check(rc, nrec.value, allow=(-5,))
            k = nrec.value
            return self._reply_dict(rq, st[:k], out, offs, src, rc=rc, stop=stop.value, n_recs=k,
                                    rec_frame=rec_frame[:k])
        res, status, _, _, reply = self._results(cap, want_reply=True)
        rc = self.L.phip_receive_frames(self.h, blob.ctypes.data, foffs.ctypes.data, nf, int(now),
                                        C.byref(res), C.byref(stop), int(frame_bytes),
                                        rec_frame.ctypes.data, cap, C.byref(nrec), 0)
        self._frames_check(rc, nrec.value, allow=(-5,))
        k = nrec.value
        return dict(status=status[:k], reply=reply[:k], stop=stop.value, n_recs=k,
                    rec_frame=rec_frame[:k], rc=rc)

    def receive_frames_device(self, data, foffs, n_frames: int, now: int, max_recs: int,
                              frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, status=None,
                              rec_frame=None, replies=None):
        """phip_receive_frames with device pointers (data / foffs as
        unframe_device takes them; status uint8[max_recs] and rec_frame
        int32[max_recs] optional CUDA tensors).  -> dict(stop, n_recs, rc).
        replies=dict(out=, offs=, src=, max_msgs=[, out_cap=]) of CUDA tensors:
        phip_receive_frames_replies -> the reply dict plus n_recs."""
        res = phip_results(_ptr(status), None, None, None)
        stop, nrec = C.c_uint32(0), C.c_uint32(0)
        if replies is not None:
            out = replies["out"]
            cap = int(out.numel()) if replies.get("out_cap") is None else int(replies["out_cap"])
            rq = _lib.phip_reply_egress(_ptr(out), cap, _ptr(replies["offs"]),
                                        _ptr(replies.get("src")), int(replies["max_msgs"]),
                                        0, 0, 0, 0)
            rc = self.L.phip_receive_frames_replies(
                self.h, _ptr(data), _ptr(foffs), int(n_frames), int(now),
                C.byref(res) if status is not None else None, C.byref(stop), C.byref(rq),
                int(frame_bytes), _ptr(rec_frame), int(max_recs), C.byref(nrec), DEVICE_PTRS)
            self._frames_check(rc, nrec.value, allow=(-5,))
            return self._reply_dict(rq, status, out, replies["offs"], replies.get("src"), rc=rc,
                                    stop=stop.value, n_recs=nrec.value)
        rc = self.L.phip_receive_frames(self.h, _ptr(data), _ptr(foffs), int(n_frames), int(now),
                                        C.byref(res), C.byref(stop), int(frame_bytes),
                                        _ptr(rec_frame), int(max_recs), C.byref(nrec), DEVICE_PTRS)
        self._frames_check(rc, nrec.value, allow=(-5,))
        return dict(stop=stop.value, n_recs=nrec.value, rc=rc)

    def upsert_soa(self, names, added, taken, elapsed, now: int):
        """LocalRepo.UpsertBucket for each state (repo.go:215-235)."""
        n = len(names)
        blob, offs = names_blob(names)
        a, t, e = _np(added, np.uint64), _np(taken, np.uint64), _np(elapsed, np.int64)
        m = phip_msgs(n, 0, blob.ctypes.data, offs.ctypes.data, a.ctypes.data, t.ctypes.data,
                      e.ctypes.data)
        res, st, _, _, _ = self._results(n)
        self._check(self.L.phip_upsert_soa(self.h, C.byref(m), int(now), C.byref(res), 0))
        return dict(status=st[:n])

    def egress_caps(self, n: int, name_bytes: int, device: bool = False):
        """phip_egress_caps: (max_msgs, out_cap) a batch of n ops and name_bytes
        of names needs for its coalesced egress."""
        m, c = C.c_uint32(), C.c_uint64()
        self._check(self.L.phip_egress_caps(n, int(name_bytes), DEVICE_PTRS if device else 0,
                                            C.byref(m), C.byref(c)))
        return m.value, c.value

    def apply_mixed(self, kind, names, now, freq=None, per=None, count=None, added=None,
                    taken=None, elapsed=None, egress=False, want_status=True):
        """Ordered TAKE/RECEIVE/UPSERT stream (api.go:67-74, repo.go:78-90, :215-235).
        egress=True: phip_apply_mixed_egress; the dict gains egress = dict(data,
        offs, n, n_incast): the batch's incast requests, then one state
        datagram per bucket its TAKE / UPSERT ops named (data uint8, datagram
        i = data[offs[i]:offs[i+1]]).  want_status=False (egress only) passes no
        status column."""
        n = len(names)
        blob, offs = names_blob(names)
        arrs = dict(kind=_np(kind, np.uint8), now=_np(now, np.int64), freq=_np(freq, np.int64),
                    per=_np(per, np.int64), count=_np(count, np.uint64),
                    added=_np(added, np.uint64), taken=_np(taken, np.uint64),
                    elapsed=_np(elapsed, np.int64))
        ops = phip_ops(n, 0, _ptr(arrs["kind"]), blob.ctypes.data, offs.ctypes.data,
                       _ptr(arrs["now"]), _ptr(arrs["freq"]), _ptr(arrs["per"]), _ptr(arrs["count"]),
                       _ptr(arrs["added"]), _ptr(arrs["taken"]), _ptr(arrs["elapsed"]))
        res, st, rem, have, reply = self._results(n, want_remaining=True, want_reply=True)
        if not egress:
            self._check(self.L.phip_apply_mixed(self.h, C.byref(ops), C.byref(res), 0))
            return dict(status=st[:n], remaining=rem[:n], have=have[:n], reply=reply[:n])
        if not want_status:
            res.status = None
        max_msgs, cap = self.egress_caps(n, int(offs[n]))
        data = np.zeros(max(cap, 1), np.uint8)
        eoffs = np.zeros(max_msgs + 1, np.uint64)
        eg = _lib.phip_egress(data.ctypes.data, cap, eoffs.ctypes.data, max_msgs, 0, 0, 0, 0)
        self._check(self.L.phip_apply_mixed_egress(self.h, C.byref(ops), C.byref(res), C.byref(eg), 0))
        return dict(status=st[:n], remaining=rem[:n], have=have[:n], reply=reply[:n],
                    egress=dict(data=data[:eg.bytes], offs=eoffs[:eg.n + 1], n=int(eg.n),
                                n_incast=int(eg.n_incast)))

    def apply_mixed_device(self, n, kind, names, name_offs, now, freq=None, per=None, count=None,
                           added=None, taken=None, elapsed=None, status=None, remaining=None,
                           have=None, names_len=None, reply=None):
        """apply_mixed with every array a torch CUDA tensor (PHIP_DEVICE_PTRS);
        names_len as receive_soa's; reply: an int64 [n, 4] tensor for the
        phip_state replies."""
        ops = phip_ops(n, _names_len(names, names_len), _ptr(kind), _ptr(names), _ptr(name_offs),
                       _ptr(now), _ptr(freq),
                       _ptr(per), _ptr(count), _ptr(added), _ptr(taken), _ptr(elapsed))
        res = phip_results(_ptr(status), _ptr(remaining), _ptr(have), _ptr(reply))
        self._check(self.L.phip_apply_mixed(self.h, C.byref(ops), C.byref(res), DEVICE_PTRS))

    def apply_mixed_egress_device(self, n, kind, names, name_offs, now, out, offs, max_msgs,
                                  freq=None, per=None, count=None, added=None, taken=None,
                                  elapsed=None, status=None, remaining=None, have=None,
                                  names_len=None, out_cap=None):
        """phip_apply_mixed_egress with every array a torch CUDA tensor
        (PHIP_DEVICE_PTRS): out (uint8, 8-byte aligned, egress_caps(...,
        device=True) bytes) and offs (int64[max_msgs + 1]) receive the
        datagrams and go unchanged into a peer's receive_datagrams_device.
        Returns dict(n, n_incast, bytes)."""
        ops = phip_ops(n, _names_len(names, names_len), _ptr(kind), _ptr(names), _ptr(name_offs),
                       _ptr(now), _ptr(freq),
                       _ptr(per), _ptr(count), _ptr(added), _ptr(taken), _ptr(elapsed))
        res = phip_results(_ptr(status), _ptr(remaining), _ptr(have), None)
        cap = int(out.numel()) if out_cap is None else int(out_cap)
        eg = _lib.phip_egress(_ptr(out), cap, _ptr(offs), int(max_msgs), 0, 0, 0, 0)
        self._check(self.L.phip_apply_mixed_egress(self.h, C.byref(ops), C.byref(res), C.byref(eg),
                                                   DEVICE_PTRS))
        return dict(n=int(eg.n), n_incast=int(eg.n_incast), bytes=int(eg.bytes))

    def route_pack_ops_device(self, n, world, kind, names, name_offs, now, freq=None, per=None,
                              count=None, added=None, taken=None, elapsed=None, names_len=None):
        """phip_route_pack_ops: the stable owner partition of an op stream given
        as torch CUDA tensors (a missing operand column reads as zeros) ->
        dict of CUDA tensors: names (uint8, packed back to back), lens, kind,
        now, x0, x1, x2 (the operand words by kind), src (op j of the send
        buffers is op src[j] of the batch), counts and name_bytes per owner.
        kind=None: the query pack of phip_group_peek (no kind column on either
        side: out["kind"] is None; x0, x1, x2 are freq, per, count)."""
        import torch
        dev = names.device
        nb = int(names.numel())
        z = max(n, 1)
        out = dict(names=torch.zeros(nb + 64, dtype=torch.uint8, device=dev),
                   lens=torch.zeros(z, dtype=torch.int32, device=dev),
                   kind=torch.zeros(z, dtype=torch.uint8, device=dev) if kind is not None else None,
                   now=torch.zeros(z, dtype=torch.int64, device=dev),
                   x0=torch.zeros(z, dtype=torch.int64, device=dev),
                   x1=torch.zeros(z, dtype=torch.int64, device=dev),
                   x2=torch.zeros(z, dtype=torch.int64, device=dev),
                   src=torch.zeros(z, dtype=torch.int32, device=dev),
                   counts=torch.zeros(max(world, 1), dtype=torch.int64, device=dev),
                   name_bytes=torch.zeros(max(world, 1), dtype=torch.int64, device=dev))
        ops = phip_ops(n, _names_len(names, names_len), _ptr(kind), _ptr(names), _ptr(name_offs),
                       _ptr(now), _ptr(freq), _ptr(per), _ptr(count), _ptr(added), _ptr(taken),
                       _ptr(elapsed))
        torch.cuda.synchronize(dev)
        self._check(self.L.phip_route_pack_ops(
            self.h, C.byref(ops), world, _ptr(out["names"]), _ptr(out["lens"]), _ptr(out["kind"]),
            _ptr(out["now"]), _ptr(out["x0"]), _ptr(out["x1"]), _ptr(out["x2"]), _ptr(out["src"]),
            _ptr(out["counts"]), _ptr(out["name_bytes"]), DEVICE_PTRS))
        return out

    def route_pack_datagrams_device(self, data, offs, n: int, world: int, combine: bool = False,
                                    bytes_len: int = 0):
        """phip_route_pack_datagrams: the stable owner partition of n raw
        datagrams read in place (data: uint8 CUDA tensor of back-to-back
        datagrams with 8 bytes of slack, offs: int64[n+1]) -> dict of CUDA
        tensors names (packed back to back), lens, added, taken, elapsed (bit
        patterns), counts and name_bytes per owner, and stop: the first
        malformed datagram (the Go loop stops there, repo.go:70-74; only the
        datagrams before it are packed) or n.  bytes_len != 0 has the offsets
        checked against it (a violation raises, code -1)."""
        import torch
        dev = data.device
        z = max(n, 1)
        out = dict(names=torch.zeros(int(data.numel()) + 64, dtype=torch.uint8, device=dev),
                   lens=torch.zeros(z, dtype=torch.int32, device=dev),
                   added=torch.zeros(z, dtype=torch.int64, device=dev),
                   taken=torch.zeros(z, dtype=torch.int64, device=dev),
                   elapsed=torch.zeros(z, dtype=torch.int64, device=dev),
                   counts=torch.zeros(max(world, 1), dtype=torch.int64, device=dev),
                   name_bytes=torch.zeros(max(world, 1), dtype=torch.int64, device=dev))
        w = phip_wire(n, 0, _ptr(data), _ptr(offs), int(bytes_len))
        stop = C.c_uint32(0)
        torch.cuda.synchronize(dev)
        self._check(self.L.phip_route_pack_datagrams(
            self.h, C.byref(w), world, _ptr(out["names"]), _ptr(out["lens"]), _ptr(out["added"]),
            _ptr(out["taken"]), _ptr(out["elapsed"]), _ptr(out["counts"]), _ptr(out["name_bytes"]),
            C.byref(stop), DEVICE_PTRS | (_lib.ROUTE_COMBINE if combine else 0)), allow=(-5,))
        out["stop"] = stop.value
        return out

    def take(self, names, now, freq, per, count):
        """Batched Bucket.Take via GetBucket (create) then Take: (remaining, ok)."""
        n = len(names)
        blob, offs = names_blob(names)
        now, freq, per = _np(now, np.int64), _np(freq, np.int64), _np(per, np.int64)
        count = _np(count, np.uint64)
        rem = np.zeros(max(n, 1), np.uint64)
        ok = np.zeros(max(n, 1), np.uint8)
        self._check(self.L.phip_take(self.h, blob.ctypes.data, offs.ctypes.data, n, now.ctypes.data,
                                     freq.ctypes.data, per.ctypes.data, count.ctypes.data,
                                     rem.ctypes.data, ok.ctypes.data, 0))
        return rem[:n], ok[:n].astype(bool)

    def api_take(self, name: bytes, rate: bytes, count: bytes, now: int):
        """API.takeBucket (api.go:51-86): (HTTP status, body)."""
        body = C.create_string_buffer(64)
        bl = C.c_uint32()
        code = self._check(self.L.phip_api_take(self.h, name, len(name), rate, len(rate), count,
                                                len(count), int(now), body, C.byref(bl)))
        return code, body.raw[:bl.value].decode()

    # -------------------------------------------------------------- peek --
    def peek(self, names, now, freq, per, count) -> dict:
        """phip_peek over host arrays: Bucket.Take evaluated on a copy of each
        named bucket's state; nothing is created or written.  -> dict(status
        (ST_TAKE_OK / ST_TAKE_DENIED, | ST_ABSENT), remaining, have (float64
        bits), retry_at (now when granted, the least later clock reading that
        grants, or PEEK_NEVER), state (a/t/e/c records: the state evaluated))."""
        n = len(names)
        blob, offs = names_blob(names)
        now, freq, per = _np(now, np.int64), _np(freq, np.int64), _np(per, np.int64)
        count = _np(count, np.uint64)
        z = max(n, 1)
        status, rem, have = np.zeros(z, np.uint8), np.zeros(z, np.uint64), np.zeros(z, np.uint64)
        at = np.zeros(z, np.int64)
        state = np.zeros(z, dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
        q = phip_ops(n, 0, None, blob.ctypes.data, offs.ctypes.data, _ptr(now), _ptr(freq),
                     _ptr(per), _ptr(count), None, None, None)
        res = _lib.phip_peek_results(_ptr(status), _ptr(rem), _ptr(have), _ptr(at), _ptr(state))
        self._check(self.L.phip_peek(self.h, C.byref(q), C.byref(res), 0))
        return dict(status=status[:n], remaining=rem[:n], have=have[:n], retry_at=at[:n],
                    state=state[:n])

    def peek_device(self, n, names, name_offs, now, freq=None, per=None, count=None, status=None,
                    remaining=None, have=None, retry_at=None, state=None, names_len=None):
        """phip_peek with every array a torch CUDA tensor (PHIP_DEVICE_PTRS):
        names (uint8 blob, 8 bytes of read slack), name_offs (int32[n+1]), the
        operand columns (int64), and the result columns wanted (status uint8,
        remaining / have / retry_at int64, state int64 [n, 4]); names_len as
        receive_soa's."""
        q = phip_ops(n, _names_len(names, names_len), None, _ptr(names), _ptr(name_offs),
                     _ptr(now), _ptr(freq), _ptr(per), _ptr(count), None, None, None)
        res = _lib.phip_peek_results(_ptr(status), _ptr(remaining), _ptr(have), _ptr(retry_at),
                                     _ptr(state))
        self._check(self.L.phip_peek(self.h, C.byref(q), C.byref(res), DEVICE_PTRS))

    def api_peek(self, name: bytes, rate: bytes, count: bytes, now: int):
        """API.takeBucket's request (api.go:51-86) answered without taking:
        (HTTP status, body, retry_after_ns: 0 with 200; with 429 the wait until
        the same request would pass, -1 for never; None with 400)."""
        body = C.create_string_buffer(64)
        bl = C.c_uint32()
        after = C.c_int64()
        code = self._check(self.L.phip_api_peek(self.h, name, len(name), rate, len(rate), count,
                                                len(count), int(now), body, C.byref(bl),
                                                C.byref(after)))
        return code, body.raw[:bl.value].decode(), (None if code == 400 else int(after.value))


def peek_eval(state, now: int, freq: int, per: int, count: int):
    """phip_peek_eval (host only, no handle, no GPU): phip_peek's evaluation of
    one query on a state the caller holds (a BucketState, an (added bits, taken
    bits, elapsed, created) tuple, or None for an absent bucket) ->
    (status, remaining, have bits, retry_at)."""
    s = None
    if state is not None:
        a, t, e, c = ((state.added, state.taken, state.elapsed, state.created)
                      if isinstance(state, BucketState) else state)
        s = C.byref(phip_state(int(a), int(t), int(e), int(c)))
    rem, have, at = C.c_uint64(), C.c_uint64(), C.c_int64()
    st = _lib.load().phip_peek_eval(s, int(now), int(freq), int(per), int(count), C.byref(rem),
                                    C.byref(have), C.byref(at))
    if st < 0:
        raise PatrolHipError(st, "phip_peek_eval")
    return st, int(rem.value), int(have.value), int(at.value)


def _throttle_rules(rules):
    """(prefix bytes, freq, per, count) rows -> a phip_throttle_rule array.  A
    prefix over 16 bytes keeps its length (the library refuses it) and its
    first 16 bytes."""
    arr = (_lib.phip_throttle_rule * len(rules))()
    for r, (prefix, freq, per, count) in zip(arr, rules):
        prefix = bytes(prefix)
        head = prefix[:_lib.THROTTLE_MAX_PREFIX]
        r.prefix[:len(head)] = list(head)
        r.prefix_len, r.freq, r.per, r.count = len(prefix), int(freq), int(per), int(count)
    return arr


def throttle_match(rules, name: bytes) -> int:
    """phip_throttle_match (host only, no handle, no GPU): the index of the
    first of the throttled sweep's rules ((prefix, freq, per, count) rows)
    whose prefix `name` starts with, or -1 -- the function the sweep's kernels
    call."""
    arr = _throttle_rules(rules)
    out = C.c_int32(-2)
    rc = _lib.load().phip_throttle_match(arr, len(arr), bytes(name), len(name), C.byref(out))
    if rc < 0:
        raise PatrolHipError(rc, "phip_throttle_match")
    return int(out.value)


_STATE_DT = [("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")]


def top_merge(lists, k: int, names_cap: int | None = None) -> dict:
    """phip_top_merge (host only, no handle, no GPU): the top k of several
    GPURepo.top() results (dicts with names, taken and, optionally, state) --
    a shard group's members, or replicas of different nodes.  By `taken`
    descending, equal values by list index and then position; a name present
    more than once is kept once, with the larger `taken` and that entry's
    state.  -> dict(names, taken, state (None unless every list carries one),
    n)."""
    lists = list(lists)
    n_l = len(lists)
    arr = (_lib.phip_top_out * max(n_l, 1))()
    ns = (C.c_uint64 * max(n_l, 1))()
    keep = []
    want_state = n_l > 0 and all(d.get("state") is not None for d in lists)
    total = 0
    for i, d in enumerate(lists):
        nm = d["names"]
        offs = np.zeros(len(nm) + 1, np.uint64)
        if nm:
            offs[1:] = np.cumsum(np.fromiter((len(x) for x in nm), np.int64, len(nm)))
        blob = np.frombuffer(b"".join(nm) + b"\0", np.uint8).copy()
        tk = _np(d["taken"], np.uint64)
        st = np.ascontiguousarray(d["state"], _STATE_DT) if d.get("state") is not None else None
        if st is not None and not st.size:
            st = np.zeros(1, _STATE_DT)
        keep.append((blob, offs, tk, st))
        arr[i] = _lib.phip_top_out(_ptr(blob), int(offs[-1]), _ptr(offs), _ptr(tk), _ptr(st))
        ns[i] = len(nm)
        total += int(offs[-1])
    z = max(int(k), 1)
    if names_cap is None:
        names_cap = total
    names = np.zeros(max(int(names_cap), 1), np.uint8)
    offs = np.zeros(z + 1, np.uint64)
    taken = np.zeros(z, np.uint64)
    sta = np.zeros(z, _STATE_DT) if want_state else None
    out = _lib.phip_top_out(_ptr(names), int(names_cap), _ptr(offs), _ptr(taken), _ptr(sta))
    n = C.c_uint64()
    rc = _lib.load().phip_top_merge(arr, ns, n_l, int(k), C.byref(out), C.byref(n))
    if rc < 0:
        raise PatrolHipError(rc, "phip_top_merge")
    n = int(n.value)
    raw = names[:int(offs[n])].tobytes()
    return dict(names=[raw[int(offs[i]):int(offs[i + 1])] for i in range(n)], taken=taken[:n],
                state=None if sta is None else sta[:n], n=n)


class GPUGroup:
    """A shard group over RCCL (phip_group_*, include/patrolhip.h): the
    buckets hash-sharded by name over several GPUs, owner-routed Receive and
    anti-entropy in the C library (no torch on the data path).

    open_all(devices): one process, every listed GPU (ncclCommInitAll);
    open_rank(repo, uid, nranks, rank): one process per GPU around `repo`
    (ncclCommInitRank), `uid` from unique_id() on rank 0."""

    def __init__(self, g, L, repos):
        self.g, self.L, self.repos = g, L, repos

    @staticmethod
    def unique_id() -> bytes:
        L = _lib.load()
        buf = C.create_string_buffer(_lib.GROUP_ID_BYTES)
        rc = L.phip_group_unique_id(buf)
        if rc != 0:
            raise PatrolHipError(rc, "phip_group_unique_id failed")
        return buf.raw

    @classmethod
    def open_all(cls, devices, log2_slots: int = 20, arena_bytes: int = 1 << 24,
                 max_load_pct: int = 90, track_changes: bool = False, track_usage: bool = False):
        """track_changes: every member keeps a change set (PHIP_CFG_TRACK_CHANGES):
        an owner marks the buckets it applied ops to, and repos[i].export_changed
        is that owner's egress.  track_usage: every member keeps a usage
        baseline (PHIP_CFG_TRACK_USAGE) for usage_mark() and top(metric=1)."""
        L = _lib.load()
        cfg = phip_config(0, log2_slots, arena_bytes, max_load_pct, 0,
                          (_lib.CFG_TRACK_CHANGES if track_changes else 0) |
                          (_lib.CFG_TRACK_USAGE if track_usage else 0), 0, 0)
        devs = (C.c_int32 * len(devices))(*devices)
        g = C.c_void_p()
        rc = L.phip_group_open_all(C.byref(cfg), devs, len(devices), C.byref(g))
        if rc != 0:
            raise PatrolHipError(rc, "phip_group_open_all failed")
        repos = [GPURepo.wrap(L.phip_group_handle(g, i), devices[i]) for i in range(len(devices))]
        return cls(g, L, repos)

    @classmethod
    def open_rank(cls, repo: "GPURepo", uid: bytes, nranks: int, rank: int):
        L = repo.L
        g = C.c_void_p()
        rc = L.phip_group_open_rank(repo.h, uid, nranks, rank, C.byref(g))
        if rc != 0:
            raise PatrolHipError(rc, "phip_group_open_rank failed")
        return cls(g, L, [repo])

    @property
    def world(self) -> int:
        return int(self.L.phip_group_world(self.g))

    def _check(self, rc):
        if rc != 0:
            raise PatrolHipError(rc, self.L.phip_group_last_error(self.g).decode(errors="replace"))

    def _group_rq(self, replies, host: bool = False):
        """One phip_reply_egress per local member from replies=dict(max_msgs=,
        out_cap=) -> (the ctypes array, the buffers per member): CUDA tensors on
        the member's GPU (out_cap: a multiple of 8, 8 bytes past the byte
        budget), or numpy arrays for the ring form."""
        k = len(self.repos)
        max_msgs = int(replies["max_msgs"])
        out_cap = int(replies.get("out_cap") or _lib.PACKET_SIZE * max(max_msgs, 1) + 8)
        rq = (_lib.phip_reply_egress * k)()
        bufs = []
        for i in range(k):
            if host:
                out = np.zeros(max(out_cap, 8), np.uint8)
                offs = np.zeros(max_msgs + 1, np.uint64)
                src = np.zeros(max(max_msgs, 1), np.uint32)
                ptrs = (out.ctypes.data, offs.ctypes.data, src.ctypes.data)
            else:
                import torch
                dev = torch.device("cuda", self.repos[i].device)
                out = torch.zeros(max(out_cap, 8), dtype=torch.uint8, device=dev)
                offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
                src = torch.zeros(max(max_msgs, 1), dtype=torch.int32, device=dev)
                torch.cuda.synchronize(dev)
                ptrs = (_ptr(out), _ptr(offs), _ptr(src))
            rq[i] = _lib.phip_reply_egress(ptrs[0], out_cap, ptrs[1], ptrs[2], max_msgs, 0, 0, 0, 0)
            bufs.append((out, offs, src))
        return rq, bufs

    @staticmethod
    def _group_replies(rq, bufs):
        """-> one dict(data, offs, src, n, replies, skipped, bytes) per member
        (the group form's counters: patrolhip.h "Group reply egress"); host
        buffers are cut to what was written, device tensors returned whole."""
        out = []
        for q, (data, offs, src) in zip(rq, bufs):
            n = int(q.n)
            if not _is_torch(data):
                data, offs, src = data[:int(q.bytes)], offs[:n + 1], src[:n]
            out.append(dict(data=data, offs=offs, src=src, n=n, replies=int(q.replies),
                            skipped=int(q.skipped), bytes=int(q.bytes)))
        return out

    def reply_stats(self, i: int = 0) -> dict:
        """phip_group_reply_stats of member i's last replies call."""
        v = (C.c_uint64 * 4)()
        k = self.L.phip_group_reply_stats(self.g, i, v, 4)
        names = ("rounds", "return_rounds", "bound", "written")
        return {nm: int(v[j]) for j, nm in enumerate(names[:k])}

    def receive(self, batches, now: int, combine: bool = True, rccl_self: bool = False,
                small_chunks: bool = False, replies=None):
        """batches: one (names uint8, name_offs int32[n+1], added, taken, elapsed)
        tuple of CUDA tensors per local member -> (sent, merged) lists.
        rccl_self (PHIP_GROUP_RCCL_SELF, testing): every segment, the
        member's own included, travels through ncclSend/ncclRecv.
        small_chunks (PHIP_GROUP_SMALL_CHUNKS, testing): the pipelined
        exchange runs in chunks of 4096 messages.

        The batches are checked (names_len = the names tensor's length):
        every local batch's name_offs column is verified in full before
        anything is packed.  A malformed entry in any of them raises
        PatrolHipError (code -1, PHIP_ERR_INVALID; the message names the
        member and the message index) and none of the batches is applied;
        the members still run the exchange with empty batches, so peer
        ranks are not left waiting.

        replies=dict(max_msgs=, out_cap=): phip_group_receive_replies; the
        result then ends with one reply dict per member (device tensors)."""
        k = len(batches)
        msgs = (phip_msgs * k)()
        for i, (names, offs, a, t, e) in enumerate(batches):
            msgs[i] = phip_msgs(offs.numel() - 1, _names_len(names), _ptr(names), _ptr(offs), _ptr(a), _ptr(t),
                                _ptr(e))
        sent, merged = (C.c_uint64 * k)(), (C.c_uint64 * k)()
        flags = DEVICE_PTRS | (_lib.ROUTE_COMBINE if combine else 0) | \
            (_lib.GROUP_RCCL_SELF if rccl_self else 0) | \
            (_lib.GROUP_SMALL_CHUNKS if small_chunks else 0)
        if replies is not None:
            rq, bufs = self._group_rq(replies)
            self._check(self.L.phip_group_receive_replies(self.g, msgs, int(now), sent, merged, rq,
                                                          flags))
            return [int(x) for x in sent], [int(x) for x in merged], self._group_replies(rq, bufs)
        self._check(self.L.phip_group_receive(self.g, msgs, int(now), sent, merged, flags))
        return [int(x) for x in sent], [int(x) for x in merged]

    def _wire_flags(self, combine, rccl_self, small_chunks):
        return DEVICE_PTRS | (_lib.ROUTE_COMBINE if combine else 0) | \
            (_lib.GROUP_RCCL_SELF if rccl_self else 0) | \
            (_lib.GROUP_SMALL_CHUNKS if small_chunks else 0)

    def _wire_call(self, rc, sent, merged, stopped):
        """A stop (PHIP_ERR_SHORT_BUFFER, the Go loop's io.ErrShortBuffer) does
        not raise: `stopped` tells where each member's batch ended."""
        if rc not in (0, -5):
            self._check(rc)
        self.last_rc = rc
        return [int(x) for x in sent], [int(x) for x in merged], [int(x) for x in stopped]

    def receive_datagrams(self, batches, now: int, combine: bool = True, rccl_self: bool = False,
                          small_chunks: bool = False, checked: bool = True, replies=None):
        """Owner-routed Receive straight from the wire
        (phip_group_receive_datagrams): batches holds, per local member, the
        raw datagrams that arrived there, as a (bytes uint8, offs int64[n+1])
        pair of CUDA tensors (8-byte aligned, 8 bytes of slack past the last
        datagram) or as a list of `bytes` objects that is packed and uploaded
        to the member's GPU.  -> (sent, merged, stopped) lists.

        Member i's datagrams before its first malformed one (repo.go:70-74)
        are routed and merged; stopped[i] is that index, or its n.  A stop
        does not raise: last_rc is then -5 (PHIP_ERR_SHORT_BUFFER), else 0.
        checked: the offsets are verified against the bytes tensor's length
        before anything is read through them; a violation raises
        PatrolHipError (code -1) and no batch is applied.  combine,
        rccl_self, small_chunks: as receive().

        replies=dict(max_msgs=, out_cap=): phip_group_receive_datagrams_replies;
        the result then ends with one reply dict per member (device tensors:
        the answers to the incast requests of that member's batch)."""
        import torch
        k = len(batches)
        ws = (phip_wire * k)()
        keep = []
        for i, b in enumerate(batches):
            if isinstance(b, (list, tuple)) and (len(b) != 2 or not _is_torch(b[0])):
                dev = torch.device("cuda", self.repos[i].device)
                offs = np.zeros(len(b) + 1, np.int64)
                if len(b):
                    offs[1:] = np.cumsum(np.fromiter((len(d) for d in b), np.int64, len(b)))
                blob = np.zeros((int(offs[-1]) + 15) // 8 * 8, np.uint8)
                blob[:int(offs[-1])] = np.frombuffer(b"".join(b), np.uint8)
                b = (torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev))
                torch.cuda.synchronize(dev)
            data, offs = b
            keep.append(b)
            ws[i] = phip_wire(offs.numel() - 1, 0, _ptr(data), _ptr(offs),
                              int(data.numel()) if checked else 0)
        sent, merged, stopped = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_uint32 * k)()
        flags = self._wire_flags(combine, rccl_self, small_chunks)
        if replies is not None:
            rq, bufs = self._group_rq(replies)
            rc = self.L.phip_group_receive_datagrams_replies(self.g, ws, int(now), sent, merged,
                                                             stopped, rq, flags)
            return self._wire_call(rc, sent, merged, stopped) + (self._group_replies(rq, bufs),)
        rc = self.L.phip_group_receive_datagrams(self.g, ws, int(now), sent, merged, stopped, flags)
        return self._wire_call(rc, sent, merged, stopped)

    def receive_frames(self, batches, now: int, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES,
                       replies=None, **kw):
        """receive_datagrams over packed frames (patrolhip.h "Packed frames"):
        batches holds, per local member, the frames that arrived there, as a
        (bytes uint8, foffs int64[n_frames+1]) pair of CUDA tensors or as a
        list of `bytes` frames.  Composition only: each member's
        unframe_device on its own handle, then receive_datagrams over the
        records; `stopped` and the replies' src[] are record indices, and
        last_rec_frame[i] (an int32 CUDA tensor) maps member i's records to
        its frames.  kw: receive_datagrams' other arguments."""
        import torch
        recs, self.last_rec_frame = [], []
        for i, b in enumerate(batches):
            repo = self.repos[i]
            dev = torch.device("cuda", repo.device)
            if isinstance(b, (list, tuple)) and (len(b) != 2 or not _is_torch(b[0])):
                blob, foffs = _frames_blob(b)
                pad = np.zeros((blob.size + 7) // 8 * 8, np.uint8)
                pad[:blob.size] = blob
                b = (torch.from_numpy(pad).to(dev), torch.from_numpy(foffs.astype(np.int64)).to(dev))
            data, foffs = b
            nf = int(foffs.numel()) - 1
            cap = _frame_bound(int(data.numel()), nf)
            rec_offs = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
            rec_frame = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
            n = repo.unframe_device(data, foffs, nf, rec_offs, rec_frame, frame_bytes=frame_bytes,
                                    max_recs=cap)
            recs.append((data, rec_offs[:n + 1]))
            self.last_rec_frame.append(rec_frame[:n])
        return self.receive_datagrams(recs, now, replies=replies, **kw)

    def ring_receive(self, rings, slots, now: int, combine: bool = True, rccl_self: bool = False,
                     small_chunks: bool = False, replies=None):
        """The socket edge (phip_group_ring_receive): rings[i] is a Ring over
        repos[i] (None: an empty batch for member i), slots[i] its next
        submitted slot.  -> (sent, merged, stopped) as receive_datagrams; the
        slots are free again when the call returns.  An out-of-order slot
        raises PatrolHipError (code -9, PHIP_ERR_BUSY) and a ring of another
        handle code -1; both leave every slot submitted.

        replies=dict(max_msgs=, out_cap=): phip_group_ring_receive_replies; the
        result then ends with one reply dict per member (numpy arrays, cut to
        what was written; reply_peers(peers_i, src) gives their peers)."""
        k = len(rings)
        rs = (C.c_void_p * k)(*[r.r.value if r is not None else None for r in rings])
        sl = (C.c_uint32 * k)(*[int(s) for s in slots])
        sent, merged, stopped = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_uint32 * k)()
        flags = self._wire_flags(combine, rccl_self, small_chunks)
        if replies is not None:
            rq, bufs = self._group_rq(replies, host=True)
            rc = self.L.phip_group_ring_receive_replies(self.g, rs, sl, int(now), sent, merged,
                                                        stopped, rq, flags)
            return self._wire_call(rc, sent, merged, stopped) + (self._group_replies(rq, bufs),)
        rc = self.L.phip_group_ring_receive(self.g, rs, sl, int(now), sent, merged, stopped, flags)
        return self._wire_call(rc, sent, merged, stopped)

    _OPS_KEYS = ("kind", "names", "name_offs", "now", "freq", "per", "count", "added", "taken",
                 "elapsed")

    def apply_mixed(self, batches, rccl_self: bool = False, small_chunks: bool = False,
                    want_reply: bool = True, results=None):
        """Owner-routed phip_apply_mixed (phip_group_apply_mixed): batches holds,
        per local member, the ops that arrived there as a dict (or a tuple in
        this order) of CUDA tensors: kind uint8, names uint8 blob, name_offs
        int32[n+1], now int64, and the operand columns freq, per, count
        (TAKE), added, taken, elapsed (RECEIVE / UPSERT), any of which may be
        None.  -> (results, sent, applied): results[i] is a dict of CUDA
        tensors status uint8[n], remaining / have int64[n] (uint64 bit
        patterns), reply int64[n, 4] (None without want_reply), entry j the
        result of op j of batches[i] as its owner applied it; sent[i] /
        applied[i] the ops member i sent and applied as an owner.

        Order: a bucket's ops take effect in (round, source rank, index)
        order, a round being 2^24 ops of every member's batch (4096 with
        small_chunks).  The batches are checked (names_len = the names
        tensor's length) as receive()'s are: a malformed name_offs entry
        raises PatrolHipError (code -1, naming the member and the op) and no
        batch is applied.

        results (optional): per member, a dict of the caller's own CUDA
        tensors for the columns (status, remaining, have, reply; a missing
        key or None leaves that column out, want_reply is then ignored), or
        None for that member's default columns.  They are handed to the
        library as they are and returned as results[i]."""
        import torch
        k = len(batches)
        ops = (phip_ops * k)()
        res = (phip_results * k)()
        out = []
        for i, b in enumerate(batches):
            if not isinstance(b, dict):
                b = dict(zip(self._OPS_KEYS, b))
            n = b["name_offs"].numel() - 1
            ops[i] = phip_ops(n, _names_len(b["names"]), *[_ptr(b.get(key)) for key in self._OPS_KEYS])
            if results is not None and results[i] is not None:
                r = {key: results[i].get(key) for key in ("status", "remaining", "have", "reply")}
                res[i] = phip_results(*[_ptr(v) for v in r.values()])
                out.append(r)
                continue
            dev, z = b["names"].device, max(n, 1)
            r = dict(status=torch.zeros(z, dtype=torch.uint8, device=dev),
                     remaining=torch.zeros(z, dtype=torch.int64, device=dev),
                     have=torch.zeros(z, dtype=torch.int64, device=dev),
                     reply=torch.zeros((z, 4), dtype=torch.int64, device=dev) if want_reply else None)
            res[i] = phip_results(_ptr(r["status"]), _ptr(r["remaining"]), _ptr(r["have"]),
                                  _ptr(r["reply"]))
            out.append({key: (v[:n] if v is not None else None) for key, v in r.items()})
        for r in self.repos:
            torch.cuda.synchronize(r.device)
        sent, applied = (C.c_uint64 * k)(), (C.c_uint64 * k)()
        flags = DEVICE_PTRS | (_lib.GROUP_RCCL_SELF if rccl_self else 0) | \
            (_lib.GROUP_SMALL_CHUNKS if small_chunks else 0)
        self._check(self.L.phip_group_apply_mixed(self.g, ops, res, sent, applied, flags))
        return out, [int(x) for x in sent], [int(x) for x in applied]

    _PEEK_KEYS = ("status", "remaining", "have", "retry_at", "state")

    def peek(self, batches, rccl_self: bool = False, small_chunks: bool = False,
             want_state: bool = False, results=None):
        """Owner-routed phip_peek (phip_group_peek): batches holds, per local
        member, the queries that arrived there as a dict of CUDA tensors:
        names uint8 blob, name_offs int32[n+1], now int64, and the operand
        columns freq, per, count (any of which may be None: zeros).  ->
        (results, sent, answered): results[i] is a dict of CUDA tensors status
        uint8[n] (ST_TAKE_OK / ST_TAKE_DENIED, | ST_ABSENT), remaining / have /
        retry_at int64[n], state int64[n, 4] (None without want_state), entry
        j what phip_peek reports for query j of batches[i] on the member that
        owns its name; sent[i] / answered[i] the queries member i sent and
        answered as an owner.  Nothing is written on any member.

        The batches are checked as apply_mixed()'s are.  want_state sets
        PHIP_GROUP_PEEK_STATE (the state column returns over the exchange).

        results (optional): per member, a dict of the caller's own CUDA
        tensors for the columns (a missing key or None leaves that column
        out), or None for that member's default columns.  They are handed to
        the library as they are and returned as results[i]."""
        import torch
        k = len(batches)
        ops = (phip_ops * k)()
        res = (_lib.phip_peek_results * k)()
        out = []
        for i, b in enumerate(batches):
            n = b["name_offs"].numel() - 1
            ops[i] = phip_ops(n, _names_len(b["names"]), None, _ptr(b["names"]),
                              _ptr(b["name_offs"]), _ptr(b.get("now")), _ptr(b.get("freq")),
                              _ptr(b.get("per")), _ptr(b.get("count")), None, None, None)
            if results is not None and results[i] is not None:
                r = {key: results[i].get(key) for key in self._PEEK_KEYS}
                res[i] = _lib.phip_peek_results(*[_ptr(v) for v in r.values()])
                out.append(r)
                continue
            dev, z = b["names"].device, max(n, 1)
            r = {key: torch.zeros(z, dtype=torch.int64, device=dev)
                 for key in ("remaining", "have", "retry_at")}
            r["status"] = torch.zeros(z, dtype=torch.uint8, device=dev)
            r["state"] = torch.zeros((z, 4), dtype=torch.int64, device=dev) if want_state else None
            res[i] = _lib.phip_peek_results(*[_ptr(r[key]) for key in self._PEEK_KEYS])
            out.append({key: (r[key][:n] if r[key] is not None else None)
                        for key in self._PEEK_KEYS})
        for r in self.repos:
            torch.cuda.synchronize(r.device)
        sent, answered = (C.c_uint64 * k)(), (C.c_uint64 * k)()
        flags = DEVICE_PTRS | (_lib.GROUP_RCCL_SELF if rccl_self else 0) | \
            (_lib.GROUP_SMALL_CHUNKS if small_chunks else 0) | \
            (_lib.GROUP_PEEK_STATE if want_state else 0)
        self._check(self.L.phip_group_peek(self.g, ops, res, sent, answered, flags))
        return out, [int(x) for x in sent], [int(x) for x in answered]

    def top(self, k: int, prefix: bytes = b"", now: int = 0, idle_ns: int = 0,
            state: bool = False, metric: int = 0, mark: bool = False) -> dict:
        """The group's top talkers: GPURepo.top of every local member (their
        tables are disjoint), then top_merge.  -> top_merge's dict, with
        population and passes summed over the members and `members`, their own
        results.  metric and mark go to every member as they are: each marks
        its own table behind its own list."""
        parts = [r.top(k, prefix, now, idle_ns, state=state, metric=metric, mark=mark)
                 for r in self.repos]
        d = top_merge(parts, k)
        d.update(bytes=sum(map(len, d["names"])), population=sum(p["population"] for p in parts),
                 passes=sum(p["passes"] for p in parts),
                 truncated=int(any(p["truncated"] for p in parts)), members=parts)
        return d

    def usage_mark(self) -> dict:
        """GPURepo.usage_mark of every local member, the stats summed."""
        parts = [r.usage_mark() for r in self.repos]
        return dict(buckets=sum(p["buckets"] for p in parts),
                    active=sum(p["active"] for p in parts), members=parts)

    def set_timing(self, on: bool = True):
        """phip_group_set_timing: per-stage event timing of later calls."""
        self._check(self.L.phip_group_set_timing(self.g, 1 if on else 0))

    def stage_ms(self, i: int = 0):
        """phip_group_stage_ms: member i's busy ms of the last call per stage
        -> dict(pack, exchange, merge) (anti-entropy: local join, all-reduce,
        apply)."""
        ms = (C.c_float * 3)()
        self._check(self.L.phip_group_stage_ms(self.g, i, ms))
        return dict(pack=float(ms[0]), exchange=float(ms[1]), merge=float(ms[2]))

    def rccl_info(self, i: int = 0):
        """phip_group_rccl_info: the RCCL member i runs on -> dict(version,
        comm_count, lib_path, mapped): `mapped` lists every librccl this
        process has mapped (/proc/self/maps), to show one copy is shared."""
        v, c = C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(4096)
        self._check(self.L.phip_group_rccl_info(self.g, i, C.byref(v), C.byref(c), buf, 4096))
        mapped = set()
        try:
            with open("/proc/self/maps") as f:
                for line in f:
                    p = line.split()[-1] if len(line.split()) >= 6 else ""
                    if "librccl" in p:
                        mapped.add(os.path.realpath(p))
        except OSError:
            pass
        return dict(version=int(v.value), comm_count=int(c.value),
                    lib_path=os.path.realpath(buf.value.decode()) if buf.value else None,
                    mapped=sorted(mapped))

    def anti_entropy(self, replicas):
        """replicas: one contiguous int64 CUDA tensor [R, 3, B] per local member."""
        R, three, B = replicas[0].shape
        ptrs = (C.c_void_p * len(replicas))(*[x.data_ptr() for x in replicas])
        self._check(self.L.phip_group_anti_entropy(self.g, ptrs, R, B, DEVICE_PTRS))

    def evict_idle(self, now: int, idle_ns: int, min_evict: int = 1, shrink: bool = False,
                   dry_run: bool = False) -> list:
        """GPURepo.evict_idle on every local member, concurrently
        (phip_group_evict_idle; eviction is local per shard) -> one dict per
        member."""
        st = (_lib.phip_evict_stats * len(self.repos))()
        self._check(self.L.phip_group_evict_idle(self.g, int(now), int(idle_ns), int(min_evict),
                                                 st, _evict_flags(shrink, dry_run)))
        return [_evict_dict(s) for s in st]

    def close(self):
        if getattr(self, "g", None):
            for r in self.repos:
                if not r.owned:
                    r.h = None
            self.L.phip_group_close(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TakeBatcher:
    """Request-coalescing Take batcher over a GPURepo (phip_batcher_*,
    include/patrolhip.h): the drop-in form of the POST /take handler
    (api.go:51-86) for one-request-per-thread callers.  take()/api_take()
    block until the request's batch ran; they release the GIL (ctypes), so
    many Python threads can wait at once.  egress_slots (None: no egress, 0:
    the library's default ring): phip_batcher_open_egress, each batch's
    coalesced replication traffic comes out of egress_next() and somebody has
    to drain it."""

    def __init__(self, repo: "GPURepo", window_us: int = 20, max_batch: int = 0,
                 egress_slots: int | None = None):
        self.repo, self.L = repo, repo.L
        b = C.c_void_p()
        cfg = _lib.phip_batcher_config(window_us, max_batch)
        if egress_slots is None:
            repo._check(self.L.phip_batcher_open(repo.h, C.byref(cfg), C.byref(b)))
        else:
            repo._check(self.L.phip_batcher_open_egress(repo.h, C.byref(cfg), int(egress_slots),
                                                        C.byref(b)))
        self.b = b
        # egress_next calls in flight: close() lets them leave before the
        # batcher is freed under them
        self._idle = threading.Condition()
        self._draining = 0
        self._closing = False

    def egress_next(self, timeout_ms: int = -1):
        """phip_batcher_egress_next: the next batch's datagrams, copied out of
        its slot, as dict(data, offs, n, n_incast, batch, first_seq, requests);
        None after timeout_ms without one or on a batcher being closed.  The
        slot stays handed out until egress_done(batch)."""
        e = _lib.phip_egress_batch()
        with self._idle:
            if self._closing or not self.b:
                return None
            self._draining += 1
        try:
            # (waited in slices, so that a close() from another thread is seen)
            left, rc = int(timeout_ms), 0
            while rc == 0 and not self._closing:
                step = 20 if left < 0 else min(left, 20)
                rc = self.L.phip_batcher_egress_next(self.b, step, C.byref(e))
                if left >= 0:
                    left -= step
                    if left <= 0:
                        break
        finally:
            with self._idle:
                self._draining -= 1
                self._idle.notify_all()
        if rc < 0:
            raise PatrolHipError(rc, "phip_batcher_egress_next failed")
        if rc == 0:
            return None
        offs = np.ctypeslib.as_array(C.cast(e.offs, C.POINTER(C.c_uint64)), (e.n + 1,)).copy()
        nb = int(offs[e.n])
        data = (np.ctypeslib.as_array(C.cast(e.bytes, C.POINTER(C.c_uint8)), (nb,)).copy()
                if nb else np.zeros(0, np.uint8))
        return dict(data=data, offs=offs, n=int(e.n), n_incast=int(e.n_incast), batch=int(e.batch),
                    first_seq=int(e.first_seq), requests=int(e.requests))

    def egress_done(self, batch: int):
        rc = self.L.phip_batcher_egress_done(self.b, int(batch))
        if rc != 0:
            raise PatrolHipError(rc, "phip_batcher_egress_done failed")

    def close(self):
        if getattr(self, "b", None):
            with self._idle:
                self._closing = True
                while self._draining:
                    self._idle.wait()
            self.L.phip_batcher_close(self.b)
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def take(self, name: bytes, now: int, freq: int, per: int, count: int):
        """-> (remaining, ok, arrival seq)."""
        rem, ok, seq = C.c_uint64(), C.c_uint8(), C.c_uint64()
        rc = self.L.phip_batcher_take(self.b, name, len(name), int(now), int(freq), int(per),
                                      int(count), C.byref(rem), C.byref(ok), C.byref(seq))
        if rc != 0:
            raise PatrolHipError(rc, "phip_batcher_take failed")
        return rem.value, bool(ok.value), seq.value

    def api_take(self, name: bytes, rate: bytes, count: bytes, now: int):
        """API.takeBucket through the batcher: (HTTP status, body)."""
        body = C.create_string_buffer(64)
        bl = C.c_uint32()
        code = self.L.phip_batcher_api_take(self.b, name, len(name), rate, len(rate), count,
                                            len(count), int(now), body, C.byref(bl))
        if code < 0:
            raise PatrolHipError(code, "phip_batcher_api_take failed")
        return code, body.raw[:bl.value].decode()

    @staticmethod
    def _reply(r):
        st = r.state
        return dict(remaining=int(r.remaining), ok=bool(r.ok), created=bool(r.created),
                    seq=int(r.seq), state=BucketState(st.added, st.taken, st.elapsed, st.created),
                    datagram=bytes(r.datagram[:r.datagram_len]))

    def take_reply(self, name: bytes, now: int, freq: int, per: int, count: int):
        """A Take with everything the handler replicates (phip_batcher_take_reply):
        dict(remaining, ok, created, seq, state, datagram)."""
        r = phip_take_reply()
        rc = self.L.phip_batcher_take_reply(self.b, name, len(name), int(now), int(freq), int(per),
                                            int(count), C.byref(r))
        if rc != 0:
            raise PatrolHipError(rc, "phip_batcher_take_reply failed")
        return self._reply(r)

    def api_take_reply(self, name: bytes, rate: bytes, count: bytes, now: int):
        """API.takeBucket plus its replication (phip_batcher_api_take_reply):
        (HTTP status, body, reply dict)."""
        body = C.create_string_buffer(64)
        bl = C.c_uint32()
        r = phip_take_reply()
        code = self.L.phip_batcher_api_take_reply(self.b, name, len(name), rate, len(rate), count,
                                                  len(count), int(now), body, C.byref(bl),
                                                  C.byref(r))
        if code < 0:
            raise PatrolHipError(code, "phip_batcher_api_take_reply failed")
        return code, body.raw[:bl.value].decode(), self._reply(r)

    def stats(self):
        """dict(batches, requests, max_batch, gpu_ns, errors, egress_batches,
        egress_datagrams, egress_wait_ns)."""
        out = (C.c_uint64 * 8)()
        k = self.L.phip_batcher_stats(self.b, out, 8)
        keys = ("batches", "requests", "max_batch", "gpu_ns", "errors", "egress_batches",
                "egress_datagrams", "egress_wait_ns")
        return {keys[i]: int(out[i]) for i in range(k)}


class Ring:
    """Pinned ingest ring over a GPURepo (phip_ring_*, include/patrolhip.h):
    the batched form of the Receive goroutine (repo.go:54-92).  Slots are
    filled in host memory (fill(), or recv() from a UDP socket), submitted
    (an async host->device copy on the ring's own stream) and received in
    order; submitting slot k+1 before receiving slot k overlaps its copy with
    slot k's merge."""

    def __init__(self, repo: "GPURepo", nslots: int = 3, max_msgs: int = 1 << 16,
                 max_bytes: int | None = None):
        self.repo, self.L = repo, repo.L
        self.max_msgs = max_msgs
        self.max_bytes = max_bytes if max_bytes is not None else 256 * max_msgs
        r = C.c_void_p()
        repo._check(self.L.phip_ring_open(repo.h, nslots, max_msgs, self.max_bytes, C.byref(r)))
        self.r = r
        self._views = {}

    def close(self):
        if getattr(self, "r", None):
            self.L.phip_ring_close(self.r)
            self.r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def acquire(self):
        """-> (slot, bytes view uint8[max_bytes], offs view uint64[max_msgs+1])."""
        slot, b, o = C.c_uint32(), C.c_void_p(), C.c_void_p()
        self.repo._check(self.L.phip_ring_acquire(self.r, C.byref(slot), C.byref(b), C.byref(o)))
        bv = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint8)), (self.max_bytes,))
        ov = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), (self.max_msgs + 1,))
        return slot.value, bv, ov

    def fill(self, datagrams: Sequence[bytes]):
        """Acquire a slot and pack `datagrams` into it -> (slot, n)."""
        slot, bv, ov = self.acquire()
        n = len(datagrams)
        if n > self.max_msgs:
            raise ValueError("batch larger than the ring's slots")
        ov[0] = 0
        if n:
            ov[1:n + 1] = np.cumsum([len(d) for d in datagrams])
            bv[:int(ov[n])] = np.frombuffer(b"".join(datagrams), np.uint8)
        return slot, n

    def recv(self, sock, timeout_ms: int = 3000, peers: bool = True):
        """Acquire a slot and fill it from a UDP socket (phip_udp_recv_batch)
        -> (slot, n, peers uint8[n, PEER_BYTES] or None)."""
        slot, bv, ov = self.acquire()
        pbuf = np.zeros((self.max_msgs, _lib.PEER_BYTES), np.uint8) if peers else None
        n = C.c_uint32()
        self.repo._check(self.L.phip_udp_recv_batch(sock.fileno(), bv.ctypes.data, self.max_bytes,
                                                    ov.ctypes.data, self.max_msgs, _ptr(pbuf),
                                                    int(timeout_ms), C.byref(n)))
        return slot, n.value, (pbuf[:n.value] if peers else None)

    def submit(self, slot: int, n: int):
        self.repo._check(self.L.phip_ring_submit(self.r, slot, n))

    def receive(self, slot: int, n: int, now: int, want_reply: bool = True,
                want_status: bool = True, status=None):
        """-> dict(status, reply, stop) as GPURepo.receive_datagrams.
        `status`: a caller uint8[>= n] array to fill instead of a new one."""
        if status is not None:
            res, reply = phip_results(status.ctypes.data, None, None, None), None
        elif want_status or want_reply:
            res, status, _, _, reply = GPURepo._results(n, want_reply=want_reply)
        else:
            res, reply = None, None
        stop = C.c_uint32()
        self.repo._check(self.L.phip_ring_receive(self.r, slot, int(now),
                                                  C.byref(res) if res is not None else None,
                                                  C.byref(stop)), allow=(-5,))
        return dict(status=status[:n] if status is not None else None,
                    reply=reply[:n] if reply is not None else None, stop=stop.value)

    def receive_replies(self, slot: int, n: int, now: int, max_msgs=None, out_cap=None,
                        want_status: bool = False):
        """phip_ring_receive_replies: receive the slot and return its incast
        replies as datagrams -> GPURepo.receive_datagrams_replies' dict.  By
        default no result column is asked for; reply_peers(peers, r["src"])
        gives the addresses to send r["data"] / r["offs"] to."""
        res, st, _, _, _ = GPURepo._results(n)
        rq, out, offs, src = GPURepo._reply_host(n, max_msgs, out_cap)
        stop = C.c_uint32()
        rc = self.L.phip_ring_receive_replies(self.r, slot, int(now),
                                              C.byref(res) if want_status else None,
                                              C.byref(stop), C.byref(rq))
        self.repo._check(rc, allow=(-5,))
        return GPURepo._reply_dict(rq, st[:n] if want_status else None, out, offs, src, rc=rc,
                                   stop=stop.value)


    # -- packed frames: a slot filled with frames (fill() / recv_frames()) --
    def recv_frames(self, sock, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES,
                    timeout_ms: int = 3000, peers: bool = True):
        """Acquire a slot and fill it with frames from a UDP socket
        (phip_udp_recv_frames) -> (slot, n_frames, peers by frame or None).
        The ring was opened with max_msgs = frames and max_bytes >=
        frame_bytes * frames."""
        slot, bv, ov = self.acquire()
        pbuf = np.zeros((self.max_msgs, _lib.PEER_BYTES), np.uint8) if peers else None
        n = C.c_uint32()
        self.repo._check(self.L.phip_udp_recv_frames(sock.fileno(), bv.ctypes.data, self.max_bytes,
                                                     ov.ctypes.data, self.max_msgs,
                                                     int(frame_bytes), _ptr(pbuf), int(timeout_ms),
                                                     C.byref(n)))
        return slot, n.value, (pbuf[:n.value] if peers else None)

    def receive_frames(self, slot: int, max_recs: int, now: int,
                       frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, want_reply: bool = False,
                       replies=None):
        """phip_ring_receive_frames over a submitted slot of frames -> the
        dict of GPURepo.receive_frames (max_recs: the capacity of the result
        columns); replies=dict(max_msgs=, out_cap=) (or {}):
        phip_ring_receive_frames_replies -> its reply dict."""
        cap = int(max_recs)
        rec_frame = np.zeros(max(cap, 1), np.uint32)
        stop, nrec = C.c_uint32(), C.c_uint32()
        if replies is not None:
            res, st, _, _, _ = GPURepo._results(cap)
            rq, out, offs, src = GPURepo._reply_host(cap, replies.get("max_msgs"),
                                                     replies.get("out_cap"))
            rc = self.L.phip_ring_receive_frames_replies(
                self.r, slot, int(now), C.byref(res), int(frame_bytes), rec_frame.ctypes.data, cap,
                C.byref(nrec), C.byref(stop), C.byref(rq))
            self.repo._frames_check(rc, nrec.value, allow=(-5,))
            k = nrec.value
            return GPURepo._reply_dict(rq, st[:k], out, offs, src, rc=rc, stop=stop.value,
                                       n_recs=k, rec_frame=rec_frame[:k])
        res, status, _, _, reply = GPURepo._results(cap, want_reply=want_reply)
        rc = self.L.phip_ring_receive_frames(self.r, slot, int(now), C.byref(res),
                                             int(frame_bytes), rec_frame.ctypes.data, cap,
                                             C.byref(nrec), C.byref(stop))
        self.repo._frames_check(rc, nrec.value, allow=(-5,))
        k = nrec.value
        return dict(status=status[:k], reply=reply[:k] if reply is not None else None,
                    stop=stop.value, n_recs=k, rec_frame=rec_frame[:k], rc=rc)


def udp_send_batch(sock, data: bytes | np.ndarray, offs: np.ndarray, peers=None,
                   peer_stride: int = 0) -> int:
    """sendmmsg of datagrams data[offs[i]:offs[i+1]] (phip_udp_send_batch)."""
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data
    offs = np.ascontiguousarray(offs, np.uint64)
    sent = C.c_uint32()
    rc = L.phip_udp_send_batch(sock.fileno(), buf.ctypes.data if buf.size else None,
                               offs.ctypes.data, len(offs) - 1, _ptr(peers), peer_stride,
                               C.byref(sent))
    if rc != 0:
        raise PatrolHipError(rc, "sendmmsg failed")
    return sent.value


def udp_recv_batch(sock, max_msgs: int, timeout_ms: int = 3000, cap: int | None = None):
    """recvmmsg into plain host arrays (phip_udp_recv_batch) ->
    (list of datagrams, peers uint8[n, PEER_BYTES])."""
    L = _lib.load()
    cap = cap if cap is not None else 256 * max_msgs
    buf = np.zeros(cap + 8, np.uint8)
    offs = np.zeros(max_msgs + 1, np.uint64)
    peers = np.zeros((max(max_msgs, 1), _lib.PEER_BYTES), np.uint8)
    n = C.c_uint32()
    rc = L.phip_udp_recv_batch(sock.fileno(), buf.ctypes.data, cap, offs.ctypes.data, max_msgs,
                               peers.ctypes.data, int(timeout_ms), C.byref(n))
    if rc != 0:
        raise PatrolHipError(rc, "recvmmsg failed")
    k = n.value
    return [bytes(buf[int(offs[i]):int(offs[i + 1])]) for i in range(k)], peers[:k]


def incast_replies(data: np.ndarray, offs: np.ndarray, status, reply, peers=None):
    """phip_incast_replies -> (packed replies uint8, offs uint64[m+1], peers or None)."""
    L = _lib.load()
    n = len(offs) - 1
    status = np.ascontiguousarray(status, np.uint8)
    cap = 256 * max(n, 1)
    out = np.zeros(cap, np.uint8)
    oo = np.zeros(n + 1, np.uint64)
    op = np.zeros((max(n, 1), _lib.PEER_BYTES), np.uint8) if peers is not None else None
    m = C.c_uint32()
    rc = L.phip_incast_replies(data.ctypes.data, offs.ctypes.data, n, status.ctypes.data,
                               reply.ctypes.data, _ptr(peers), out.ctypes.data, cap,
                               oo.ctypes.data, _ptr(op), C.byref(m))
    if rc != 0:
        raise PatrolHipError(rc, "incast replies")
    k = m.value
    return out[:int(oo[k])], oo[:k + 1], (op[:k] if op is not None else None)


def reply_peers(peers: np.ndarray, src) -> np.ndarray:
    """phip_reply_peers: peers[src[k]] for the datagrams of a *_replies call
    (uint8[n, PEER_BYTES], the batch's senders in reply order)."""
    L = _lib.load()
    src = np.ascontiguousarray(src, np.uint32)
    peers = np.ascontiguousarray(peers, np.uint8)
    out = np.zeros((max(len(src), 1), _lib.PEER_BYTES), np.uint8)
    rc = L.phip_reply_peers(peers.ctypes.data if peers.size else None,
                            src.ctypes.data if src.size else None, len(src), out.ctypes.data)
    if rc != 0:
        raise PatrolHipError(rc, "reply peers")
    return out[:len(src)]


def _frames_blob(frames: Sequence[bytes]):
    """list of frames -> (bytes uint8 with 8 bytes of slack, foffs uint64[n+1])."""
    n = len(frames)
    foffs = np.zeros(n + 1, np.uint64)
    if n:
        foffs[1:] = np.cumsum(np.fromiter((len(f) for f in frames), np.int64, n))
    blob = np.zeros(int(foffs[-1]) + 8, np.uint8)
    if foffs[-1]:
        blob[:int(foffs[-1])] = np.frombuffer(b"".join(frames), np.uint8)
    return blob, foffs


def _frame_bound(total_bytes: int, n_frames: int) -> int:
    """No more records than this come out of n_frames frames of total_bytes
    bytes: a frame of s bytes holds at most s // 25 whole records and a tail."""
    return total_bytes // _lib.BUCKET_FIXED_SIZE + n_frames


def _frames_error(rc: int, what: str, needed: int):
    e = PatrolHipError(rc, what)
    e.needed = int(needed)
    return e


def unframe(frames, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_recs=None, bytes_len=None):
    """phip_unframe on the host (no GPU, no handle): `frames` is a list of
    `bytes` frames or a (data uint8, foffs uint64[n+1]) pair of numpy arrays ->
    dict(rec_offs uint64[n+1], rec_frame uint32[n], n).  bytes_len: the length
    the entries are checked against (a pair's default: len(data); 0 = not
    checked).  On error PatrolHipError carries `needed`, the record count."""
    L = _lib.load()
    if isinstance(frames, tuple):
        data, foffs = frames
        data = np.ascontiguousarray(data, np.uint8)
        foffs = np.ascontiguousarray(foffs, np.uint64)
        lim = int(data.size) if bytes_len is None else int(bytes_len)
    else:
        data, foffs = _frames_blob(frames)
        lim = int(foffs[-1]) if bytes_len is None else int(bytes_len)
    nf = len(foffs) - 1
    if max_recs is None:
        max_recs = _frame_bound(int(data.size), nf)
    rec_offs = np.zeros(int(max_recs) + 1, np.uint64)
    rec_frame = np.zeros(max(int(max_recs), 1), np.uint32)
    n = C.c_uint32()
    rc = L.phip_unframe(None, data.ctypes.data, foffs.ctypes.data, nf, lim, int(frame_bytes),
                        rec_offs.ctypes.data, rec_frame.ctypes.data, int(max_recs), C.byref(n), 0)
    if rc != 0:
        raise _frames_error(rc, "unframe", n.value)
    return dict(rec_offs=rec_offs[:n.value + 1], rec_frame=rec_frame[:n.value], n=n.value)


def frame_cuts(offs, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES, max_frames=None):
    """phip_frame_cuts on the host (no GPU, no handle): offs is an export's
    offsets column (n + 1 entries) -> dict(frame_offs uint64[k+1], frame_first
    uint32[k], n=k); phip_udp_send_batch(fd, bytes, frame_offs, k, ...) sends
    the frames.  On error PatrolHipError carries `needed`, the frame count."""
    L = _lib.load()
    offs = np.ascontiguousarray(offs, np.uint64)
    n = len(offs) - 1
    if max_frames is None:
        max_frames = n
    frame_offs = np.zeros(int(max_frames) + 1, np.uint64)
    frame_first = np.zeros(max(int(max_frames), 1), np.uint32)
    k = C.c_uint32()
    rc = L.phip_frame_cuts(None, offs.ctypes.data, n, int(frame_bytes), frame_offs.ctypes.data,
                           frame_first.ctypes.data, int(max_frames), C.byref(k), 0)
    if rc != 0:
        raise _frames_error(rc, "frame cuts", k.value)
    return dict(frame_offs=frame_offs[:k.value + 1], frame_first=frame_first[:k.value], n=k.value)


def frame_reply_peers(peers: np.ndarray, rec_frame, src) -> np.ndarray:
    """phip_frame_reply_peers: peers[rec_frame[src[k]]] for the reply datagrams
    of a *_frames_replies call (peers by frame, uint8[n_frames, PEER_BYTES])."""
    L = _lib.load()
    src = np.ascontiguousarray(src, np.uint32)
    rec_frame = np.ascontiguousarray(rec_frame, np.uint32)
    peers = np.ascontiguousarray(peers, np.uint8)
    out = np.zeros((max(len(src), 1), _lib.PEER_BYTES), np.uint8)
    rc = L.phip_frame_reply_peers(peers.ctypes.data if peers.size else None,
                                  rec_frame.ctypes.data if rec_frame.size else None,
                                  src.ctypes.data if src.size else None, len(src), out.ctypes.data)
    if rc != 0:
        raise PatrolHipError(rc, "frame reply peers")
    return out[:len(src)]


def udp_recv_frames(sock, max_frames: int, frame_bytes: int = _lib.FRAME_DEFAULT_BYTES,
                    timeout_ms: int = 3000, cap: int | None = None):
    """recvmmsg of packed frames into plain host arrays (phip_udp_recv_frames)
    -> (list of frames, peers uint8[n, PEER_BYTES])."""
    L = _lib.load()
    cap = cap if cap is not None else int(frame_bytes) * max_frames
    buf = np.zeros(cap + 8, np.uint8)
    foffs = np.zeros(max_frames + 1, np.uint64)
    peers = np.zeros((max(max_frames, 1), _lib.PEER_BYTES), np.uint8)
    n = C.c_uint32()
    rc = L.phip_udp_recv_frames(sock.fileno(), buf.ctypes.data, cap, foffs.ctypes.data, max_frames,
                                int(frame_bytes), peers.ctypes.data, int(timeout_ms), C.byref(n))
    if rc != 0:
        raise PatrolHipError(rc, "recvmmsg of frames failed")
    k = n.value
    return [bytes(buf[int(foffs[i]):int(foffs[i + 1])]) for i in range(k)], peers[:k]


def parse_rate(s: bytes):
    """ParseRate (bucket.go:102-123): (freq, per_ns, ok) with Go's error values."""
    L = _lib.load()
    f, p = C.c_int64(), C.c_int64()
    rc = L.phip_parse_rate(s, len(s), C.byref(f), C.byref(p))
    return f.value, p.value, rc == 0


def marshal(name: bytes, state: BucketState) -> bytes:
    """Bucket.MarshalBinary (bucket.go:51-68)."""
    L = _lib.load()
    out = C.create_string_buffer(256)
    st = phip_state(state.added, state.taken, state.elapsed, state.created)
    n = L.phip_marshal(name, len(name), C.byref(st), out)
    if n < 0:
        raise PatrolHipError(n, "bucket name larger than 231")
    return out.raw[:n]
