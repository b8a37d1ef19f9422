"""Packed frames without a GPU (include/patrolhip.h "Packed frames"): the new
symbols and constants, the host forms of phip_unframe and phip_frame_cuts
against the pure-Python rules of tests/_frames_cases.py, their error cases,
the round trip, phip_udp_recv_frames over loopback, phip_frame_reply_peers,
and tools/frames_check.cpp -- the shared host functions as a stand-alone
program under ASan and UBSan.  No device calls; exact equality throughout."""
import ctypes as C
import os
import re
import shutil
import socket
import struct
import subprocess

import numpy as np
import pytest

import patrol_amd
from patrol_amd import _lib
from tests import _frames_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("phip_unframe", "phip_frame_cuts", "phip_receive_frames", "phip_receive_frames_replies",
       "phip_ring_receive_frames", "phip_ring_receive_frames_replies", "phip_udp_recv_frames",
       "phip_frame_reply_peers")


def header():
    return open(os.path.join(ROOT, "include", "patrolhip.h")).read()


def test_header_exports_constants_and_binding():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name, want in (("MIN_BYTES", 256), ("DEFAULT_BYTES", 1472), ("MAX_BYTES", 65507),
                       ("TILE", 4096)):
        assert re.search(r"#define PHIP_FRAME_%s\s+%d\b" % (name, want), src), name
        assert getattr(_lib, "FRAME_" + name) == want
    assert (FC.FRAME_MIN, FC.FRAME_DEFAULT, FC.FRAME_MAX, FC.FRAME_TILE) == (256, 1472, 65507, 4096)
    # the section stands behind the incast reply egress
    assert header().index("---- Incast reply egress ----") < header().index("---- Packed frames ----") \
        < header().index("---- shard layer ----")
    assert L.phip_abi_version() == 3
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", src)
    for f in ("unframe", "frame_cuts", "frame_reply_peers", "udp_recv_frames"):
        assert callable(getattr(patrol_amd, f)), f
    for m in ("unframe", "unframe_device", "frame_cuts", "frame_cuts_device", "receive_frames",
              "receive_frames_device"):
        assert callable(getattr(patrol_amd.GPURepo, m)), m
    assert callable(patrol_amd.Ring.receive_frames) and callable(patrol_amd.Ring.recv_frames)
    assert callable(patrol_amd.GPUGroup.receive_frames)


# ---------------------------------------------------------------- unframe --
@pytest.mark.parametrize("name", sorted(FC.unframe_cases()))
def test_host_unframe_equals_the_rule(name):
    frames = FC.unframe_cases()[name]
    want_offs, want_frame = FC.unframe_model(frames)
    got = patrol_amd.unframe(frames, FC.FRAME_DEFAULT)
    assert got["n"] == len(want_frame)
    assert got["rec_offs"].tolist() == want_offs
    assert got["rec_frame"].tolist() == want_frame
    # an exact capacity is enough
    again = patrol_amd.unframe(frames, FC.FRAME_DEFAULT, max_recs=len(want_frame))
    assert again["rec_offs"].tolist() == want_offs


def test_the_cases_hold_what_they_are_for():
    c = FC.unframe_cases()
    assert FC.split_frame(c["58_empty_names"][0]) == [25] * 58 and len(c["58_empty_names"][0]) == 1450
    assert FC.split_frame(c["58_empty_names_and_tail"][0]) == [25] * 58 + [22]
    assert FC.split_frame(c["name_lengths"][0]) == [25, 26, 255, 256]
    assert FC.split_frame(c["empty_frame"][1]) == [0]
    assert FC.split_frame(c["length_byte_overruns"][0]) == [27, 31]
    assert [len(c["frames_%d" % k]) for k in (0, 1, 63, 64, 65, 4096, 4097)] == \
        [0, 1, 63, 64, 65, 4096, 4097]
    assert all(len(f) <= FC.FRAME_DEFAULT for fr in c.values() for f in fr)


def test_unframe_refuses_a_long_frame_and_bad_frame_bytes():
    frames = [FC.record(b"a") * 3, FC.record(b"b" * 200) * 2]     # 78 and 450 bytes
    with pytest.raises(patrol_amd.PatrolHipError) as e:
        patrol_amd.unframe(frames, 256)
    assert e.value.code == FC.INVALID
    assert patrol_amd.unframe(frames, 450)["n"] == 5
    for fb in (255, 65508, 0):
        with pytest.raises(patrol_amd.PatrolHipError) as e:
            patrol_amd.unframe(frames[:1], fb)
        assert e.value.code == FC.INVALID
    assert patrol_amd.unframe(frames[:1], 256)["n"] == 3
    assert patrol_amd.unframe(frames[:1], 65507)["n"] == 3


def test_unframe_reads_nothing_at_a_bad_entry():
    """A checked batch: the bad offset points far outside the buffer, and the
    call returns PHIP_ERR_INVALID without walking anything."""
    data, foffs = FC.frames_blob([FC.record(b"a") * 2, FC.record(b"b"), FC.record(b"c")])
    far = 1 << 45
    dec = foffs.copy()
    dec[2] = dec[1] - 1                                  # a decreasing entry
    past = foffs.copy()
    past[3] = far                                        # one past bytes_len (and over frame_bytes)
    both = foffs.copy()
    both[1], both[2] = far, far + 30                     # in order, short enough, outside the buffer
    for bad in (dec, past, both):
        with pytest.raises(patrol_amd.PatrolHipError) as e:
            patrol_amd.unframe((data, bad), 1472)
        assert e.value.code == FC.INVALID and e.value.needed == 0
    # the last one is only caught by the bytes_len check
    past2 = foffs.copy()
    past2[3] = int(data.size) + 1
    with pytest.raises(patrol_amd.PatrolHipError):
        patrol_amd.unframe((data, past2), 1472)
    assert patrol_amd.unframe((data, foffs), 1472)["n"] == 4


def test_unframe_max_recs_one_short_returns_the_count():
    frames = FC.unframe_cases()["frames_65"]
    want = len(FC.unframe_model(frames)[1])
    with pytest.raises(patrol_amd.PatrolHipError) as e:
        patrol_amd.unframe(frames, 1472, max_recs=want - 1)
    assert e.value.code == FC.INVALID and e.value.needed == want


# ------------------------------------------------------------------- cuts --
@pytest.mark.parametrize("name", sorted(FC.cuts_cases()))
def test_host_frame_cuts_equal_the_rule(name):
    offs, fb = FC.cuts_cases()[name]
    n = len(offs) - 1
    want_offs, want_first = FC.cuts_model(offs.tolist(), fb)
    got = patrol_amd.frame_cuts(offs, fb)
    assert got["n"] == len(want_first)
    assert got["frame_offs"].tolist() == want_offs
    assert got["frame_first"].tolist() == want_first
    fo, ff = got["frame_offs"], got["frame_first"].astype(np.int64)
    assert int(fo[0]) == int(offs[0]) and int(fo[-1]) == int(offs[n])
    assert set(fo.tolist()) <= set(offs.tolist())
    if n:
        assert int(np.diff(fo.astype(np.int64)).max()) <= fb          # every frame fits
        last = np.append(ff[1:], n) - 1                                # a frame's last record
        assert np.array_equal(ff // FC.FRAME_TILE, last // FC.FRAME_TILE)   # no tile crossed
    # A condition, not a measurement: per-tile greedy is optimal per tile, and
    # an optimal global cut restricted to tiles adds at most one frame per boundary.
    ntiles = (n + FC.FRAME_TILE - 1) // FC.FRAME_TILE
    greedy = len(FC.cuts_model(offs.tolist(), fb, tile=None)[1])
    assert got["n"] <= greedy + max(ntiles - 1, 0)


def test_cuts_of_no_records():
    got = patrol_amd.frame_cuts(np.array([77], np.uint64), 1472)
    assert got["n"] == 0 and got["frame_offs"].tolist() == [77]


def test_cuts_refuse_a_record_longer_than_frame_bytes():
    offs = FC.offsets_of([100, 257, 100])
    with pytest.raises(patrol_amd.PatrolHipError) as e:
        patrol_amd.frame_cuts(offs, 256)
    assert e.value.code == FC.INVALID
    assert patrol_amd.frame_cuts(offs, 257)["n"] == 3
    for fb in (255, 65508):
        with pytest.raises(patrol_amd.PatrolHipError):
            patrol_amd.frame_cuts(FC.offsets_of([30, 30]), fb)
    with pytest.raises(patrol_amd.PatrolHipError) as e:     # max_frames one short
        patrol_amd.frame_cuts(offs, 257, max_frames=2)
    assert e.value.code == FC.INVALID and e.value.needed == 3


@pytest.mark.parametrize("n,fb", [(1, 256), (4097, 1472), (8193, 8972), (5000, 256)])
def test_round_trip(n, fb):
    """unframe(frame_cuts(offs)) returns offs, and rec_frame agrees with frame_first."""
    rng = np.random.default_rng(n)
    recs = [FC.record(FC.name_of(k, int(rng.integers(0, 232))), k, k + 1, k + 2) for k in range(n)]
    offs = FC.offsets_of([len(r) for r in recs])
    data = np.frombuffer(b"".join(recs) + bytes(8), np.uint8)
    cuts = patrol_amd.frame_cuts(offs, fb)
    back = patrol_amd.unframe((data, cuts["frame_offs"]), fb, bytes_len=int(offs[-1]))
    assert np.array_equal(back["rec_offs"], offs)
    first = np.searchsorted(cuts["frame_first"], np.arange(n), side="right") - 1
    assert np.array_equal(back["rec_frame"], first)


# ------------------------------------------------------------ socket edge --
def _pair():
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    rx.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
    rx.bind(("127.0.0.1", 0))
    tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tx.bind(("127.0.0.1", 0))
    return rx, tx


def _peer_addr(rec):
    assert struct.unpack_from("=H", rec, 0)[0] == socket.AF_INET
    return socket.inet_ntoa(bytes(rec[4:8])), struct.unpack_from(">H", rec, 2)[0]


def _drain(rx, want, **kw):
    got, peers = [], []
    while len(got) < want:
        fr, pr = patrol_amd.udp_recv_frames(rx, timeout_ms=2000, **kw)
        assert fr, "frames lost on loopback"
        got += fr
        peers += [_peer_addr(p) for p in pr]
    return got, peers


def test_recv_frames_windows_order_and_peers():
    rx, tx = _pair()
    tx2 = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tx2.bind(("127.0.0.1", 0))
    try:
        rng = np.random.default_rng(4)
        sent, who = [], []
        for i in range(90):
            size = (25, 1472, 1473)[i % 3] if i < 30 else int(rng.integers(1, 1473))
            d = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            s = tx2 if i % 7 == 3 else tx
            s.sendto(d, rx.getsockname())
            sent.append(d)
            who.append(s.getsockname())
        got, peers = _drain(rx, len(sent), max_frames=64, frame_bytes=1472)
        assert got == [d[:1472] for d in sent]          # a 1473-byte frame is cut to 1472
        assert peers == who
    finally:
        rx.close()
        tx.close()
        tx2.close()


def test_recv_frames_caps_and_timeout():
    rx, tx = _pair()
    try:
        fr, pr = patrol_amd.udp_recv_frames(rx, 8, 1472, timeout_ms=20)   # a timeout is not an error
        assert fr == [] and len(pr) == 0
        sent = [bytes([i]) * (300 + i) for i in range(30)]
        for d in sent:
            tx.sendto(d, rx.getsockname())
        fr, _ = patrol_amd.udp_recv_frames(rx, 8, 1472, timeout_ms=1000)         # max_frames
        assert fr == sent[:8]
        # cap: a frame is only read while a whole window of frame_bytes is free
        fr, _ = patrol_amd.udp_recv_frames(rx, 64, 1472, timeout_ms=1000, cap=4000)
        used = sum(len(d) for d in fr)
        assert fr == sent[8:8 + len(fr)] and 1 <= len(fr) < 22
        assert used <= 4000 and used + 1472 > 4000
        rest, _ = _drain(rx, 30 - 8 - len(fr), max_frames=64, frame_bytes=1472)
        assert rest == sent[8 + len(fr):]
        for fb in (255, 65508):
            with pytest.raises(patrol_amd.PatrolHipError) as e:
                patrol_amd.udp_recv_frames(rx, 8, fb, timeout_ms=0)
            assert e.value.code == FC.INVALID
    finally:
        rx.close()
        tx.close()


def test_frame_reply_peers_on_a_hand_made_map():
    peers = np.zeros((3, _lib.PEER_BYTES), np.uint8)
    for f in range(3):
        peers[f] = 10 * (f + 1)
    rec_frame = np.array([0, 0, 1, 1, 1, 2], np.uint32)
    src = np.array([5, 0, 3, 2], np.uint32)
    out = patrol_amd.frame_reply_peers(peers, rec_frame, src)
    assert out.shape == (4, _lib.PEER_BYTES)
    assert out[:, 0].tolist() == [30, 10, 20, 20] and np.array_equal(out, peers[[2, 0, 1, 1]])
    assert patrol_amd.frame_reply_peers(peers, rec_frame, np.zeros(0, np.uint32)).shape[0] == 0


# ------------------------------------------------------ the host sanitizers --
def test_frames_check_under_asan_and_ubsan(tmp_path):
    """tools/frames_check.cpp with patrol_amd/csrc/phip_udp.cpp, built for the
    CPU with -fsanitize=address,undefined: the functions the host forms and the
    kernels share, every buffer at its exact size."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    exe = str(tmp_path / "frames_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "patrol_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "frames_check.cpp"),
                    os.path.join(ROOT, "patrol_amd", "csrc", "phip_udp.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert re.search(r"\d+ cases clean", r.stdout), r.stdout
