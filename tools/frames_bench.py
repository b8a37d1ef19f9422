#!/usr/bin/env python3
"""What packed frames cost on the device (not the bench): one process, one
build, the forms alternating (include/patrolhip.h "Packed frames").

  (a) phip_receive_datagrams over 2^24 Zipf-1.1 records of the 10M-bucket
      table against phip_receive_frames over the same bytes cut into
      1472-byte frames, each on its own table, device pointers: kernel time
      (phip_last_timings, HIP events) and call time (a host clock round the
      call, which ends in a stream synchronise).  With --parent-lib the parent
      commit's library receives the same datagrams in the same run: the
      yardstick that shows the datagram path did not move.
  (b) The unframe kernels alone (k_frame_check, _count, _scan, _write) beside
      k_wire_scan over the same bytes, the one-pass pre-pass of
      phip_route_pack_datagrams.
  (c) The one-call export sweep of that table with and without
      phip_frame_cuts(PHIP_DEVICE_PTRS) behind it, and the bytes of offsets a
      host would read back each way.

Every figure is the median of --reps steps after --warmup, with min and max
beside it.  The socket side is not measured here.  Writes
profiles/frames_bench.json (--out) with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

UNFRAME_KERNELS = ("k_frame_check", "k_frame_count", "k_frame_scan", "k_frame_write")
CUT_KERNELS = ("k_frame_cut_count", "k_frame_scan", "k_frame_cut_write")
SWEEP_KERNELS = ("k_sweep_count", "k_sweep_scan", "k_sweep_write")


def stat(xs):
    return dict(ms=float(statistics.median(xs)), min_ms=float(min(xs)), max_ms=float(max(xs)))


def by_name(timings):
    tm = {}
    for nm, x in timings:
        tm[nm] = tm.get(nm, 0.0) + x
    return tm


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25)
    p.add_argument("--frame-bytes", type=int, default=1472)
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--route-world", type=int, default=8)
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "var", "libpatrolhip_parent.so"),
                   help="the parent commit's libpatrolhip.so ('' or missing: not measured)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    from patrol_amd.engine import GPURepo, phip_config, phip_wire
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(17)
    n, K, L, FB, W = args.records, args.buckets, args.log2_slots, args.frame_bytes, args.route_world
    total = args.warmup + args.reps
    lib = _lib.load()
    out = dict(tool="tools/frames_bench.py", build_id=_lib.build_id(), records=n, buckets=K, zipf=1.1,
               frame_bytes=FB, reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))

    ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
    blob, offs = bench.names_for_ids(torch, ids)
    del ids

    def open_repo(Lx, log2):
        r = GPURepo.__new__(GPURepo)
        r.L, r.device, r.owned = Lx, 0, True
        cfg = phip_config(0, log2, 1 << 20, 90, 0, 0, 0, 0)
        h = C.c_void_p()
        assert Lx.phip_open(C.byref(cfg), C.byref(h)) == 0
        r.h = h
        r._queued = None
        r.set_timing(True)
        return r

    handles = dict(datagrams=open_repo(lib, L), frames=open_repo(lib, L))
    if args.parent_lib and os.path.exists(args.parent_lib):
        cur, _lib._lib = _lib._lib, None
        try:
            Lp = _lib.load(args.parent_lib)
        finally:
            _lib._lib = cur
        out["parent_build_id"] = Lp.phip_build_id().decode()
        assert out["parent_build_id"] != out["build_id"], "--parent-lib is this build"
        handles["parent_datagrams"] = open_repo(Lp, L)
    small = patrol_amd.GPURepo(device=0, log2_slots=10)
    small.set_timing(True)

    frame_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rec_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rec_frame = torch.zeros(n, dtype=torch.int32, device=dev)
    s_names = torch.empty(int(offs[-1]) + 64, dtype=torch.uint8, device=dev)
    s_lens = torch.empty(n, dtype=torch.int32, device=dev)
    s_a, s_t, s_e = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    cw, bw = (torch.zeros(W, dtype=torch.int64, device=dev) for _ in range(2))
    send = [x.data_ptr() for x in (s_names, s_lens, s_a, s_t, s_e, cw, bw)]

    rows = {k: [] for k in list(handles) + ["unframe", "unframe_no_map", "wire_scan", "cuts"]}
    order = list(handles)
    nf = 0
    for j in range(total):
        a, t, e = bench.replica_states(torch, gen, n, j, dev)
        data, doffs = bench.datagrams(torch, blob, offs, a, t, e)
        nf = small.frame_cuts_device(doffs, n, frame_offs, None, frame_bytes=FB)
        rows["cuts"].append(by_name(small.timings()))
        # (b) the unframe kernels alone, and the pre-pass they are compared with
        for key, rf in (("unframe", rec_frame), ("unframe_no_map", None)):
            assert small.unframe_device(data, frame_offs, nf, rec_offs, rf, frame_bytes=FB,
                                        max_recs=n, bytes_len=0) == n
            rows[key].append(by_name(small.timings()))
        assert torch.equal(rec_offs, doffs)
        w = phip_wire(n, 0, data.data_ptr(), doffs.data_ptr(), 0)
        stop = C.c_uint32()
        assert lib.phip_route_pack_datagrams(small.h, C.byref(w), W, *send, C.byref(stop),
                                             _lib.DEVICE_PTRS) == 0 and stop.value == n
        rows["wire_scan"].append(by_name(small.timings()))
        # (a) the receive calls, each on its own table, none always first
        for key in order[j % len(order):] + order[:j % len(order)]:
            r = handles[key]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if key == "frames":
                got = r.receive_frames_device(data, frame_offs, nf, bench.T0 + j, n, frame_bytes=FB)
                assert got["stop"] == n and got["n_recs"] == n
            else:
                assert r.receive_datagrams_device(data, doffs, n, bench.T0 + j) == n
            wall = (time.perf_counter() - t0) * 1e3
            rows[key].append(dict(wall_ms=wall, kernels=by_name(r.timings())))
        del data, doffs, a, t, e

    def calls(rs):
        rs = rs[args.warmup:]
        names = sorted({nm for r in rs for nm in r["kernels"]})
        return dict(call=stat([r["wall_ms"] for r in rs]),
                    kernels=stat([sum(r["kernels"].values()) for r in rs]),
                    kernels_ms={nm: float(statistics.median([r["kernels"].get(nm, 0.0) for r in rs]))
                                for nm in names})

    def kernels(rs, names):
        rs = rs[args.warmup:]
        d = stat([sum(r.get(nm, 0.0) for nm in names) for r in rs])
        d["kernels_ms"] = {nm: float(statistics.median([r.get(nm, 0.0) for r in rs])) for nm in names}
        return d

    a_out = {k: calls(rows[k]) for k in handles}
    a_out["frames_over_datagrams_kernels"] = a_out["frames"]["kernels"]["ms"] / a_out["datagrams"]["kernels"]["ms"]
    a_out["frames_minus_datagrams_kernels_ms"] = a_out["frames"]["kernels"]["ms"] - a_out["datagrams"]["kernels"]["ms"]
    a_out["frames_minus_datagrams_call_ms"] = a_out["frames"]["call"]["ms"] - a_out["datagrams"]["call"]["ms"]
    if "parent_datagrams" in a_out:
        a_out["datagrams_over_parent_kernels"] = \
            a_out["datagrams"]["kernels"]["ms"] / a_out["parent_datagrams"]["kernels"]["ms"]
        a_out["datagrams_over_parent_call"] = \
            a_out["datagrams"]["call"]["ms"] / a_out["parent_datagrams"]["call"]["ms"]
    out["a_receive"] = dict(n_frames=nf, records_per_frame=n / max(nf, 1), **a_out)
    b_out = dict(unframe=kernels(rows["unframe"], UNFRAME_KERNELS),
                 unframe_no_rec_frame=kernels(rows["unframe_no_map"], UNFRAME_KERNELS),
                 k_wire_scan=kernels(rows["wire_scan"], ("k_wire_scan",)),
                 frame_cuts=kernels(rows["cuts"], CUT_KERNELS))
    b_out["unframe_over_wire_scan"] = b_out["unframe_no_rec_frame"]["ms"] / b_out["k_wire_scan"]["ms"]
    out["b_unframe_alone"] = b_out
    print(json.dumps(out["a_receive"]), flush=True)
    print(json.dumps(out["b_unframe_alone"]), flush=True)

    # (c) the export sweep of the table (a) left, with and without the cuts behind it
    del rec_offs, rec_frame, s_names, s_lens, s_a, s_t, s_e
    repo = handles["datagrams"]
    sw_msgs = 1 << (L - 1)
    cnt_all = repo.sweep_count()
    sw_out = torch.zeros((cnt_all["bytes"] + 15) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    sw_offs = torch.zeros(sw_msgs + 1, dtype=torch.int64, device=dev)
    c_rows = dict(plain=[], cuts=[])
    sw_frames = 0
    for j in range(2 * total):
        mode = "cuts" if j % 2 else "plain"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nrec, _, st = repo.export_sweep_device(sw_out, sw_offs, None, sw_msgs)
        km = by_name(repo.timings())
        if mode == "cuts":
            sw_frames = repo.frame_cuts_device(sw_offs, nrec, frame_offs, None, frame_bytes=FB)
            for nm, x in by_name(repo.timings()).items():
                km[nm] = km.get(nm, 0.0) + x
        wall = (time.perf_counter() - t0) * 1e3
        assert st["done"] and nrec == cnt_all["n"]
        c_rows[mode].append(dict(wall_ms=wall, kernels=km))
    out["c_sweep"] = dict(
        records=cnt_all["n"], bytes=cnt_all["bytes"], n_frames=sw_frames,
        plain=calls(c_rows["plain"]),
        with_cuts=calls(c_rows["cuts"]),
        offsets_bytes_per_record=8 * (cnt_all["n"] + 1), offsets_bytes_per_frame=8 * (sw_frames + 1))
    out["c_sweep"]["with_cuts_over_plain_kernels"] = \
        out["c_sweep"]["with_cuts"]["kernels"]["ms"] / out["c_sweep"]["plain"]["kernels"]["ms"]
    print(json.dumps(out["c_sweep"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
