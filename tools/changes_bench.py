#!/usr/bin/env python3
"""What the change set costs (not the bench): a handle opened with
PHIP_CFG_TRACK_CHANGES against one without, and phip_export_changed against
the sweep, in one process on one build.

The table is tools/export_sweep_bench.py's: 10M buckets b"b%d" seeded into
2^25 slots (opened at 2^20 with max_load_pct 45), half of them created long
ago; one untracked and one tracked handle hold a copy each.

  (a) mark cost.  C3's mix at one chunk -- 2^24 ops, 50 % Take at 100:1s and
      50 % received replica states, Zipf 1.1 over the 10M buckets, device
      pointers -- alternating the untracked and the tracked handle: the wall
      time of each call (it ends in a stream synchronise) and the marking
      kernels' own times from phip_last_timings (HIP events).
  (b) drain cost.  On the tracked handle: phip_export_changed with device
      pointers after TAKEs on 100 and on 10,000 buckets, and after one step of
      (a); kernel times and the call's wall time.  In the same run one
      phip_export_sweep over the whole table and one with half the buckets
      filtered as idle, both of which read every slot.
  (c) 1024 host ops of the same stream through the binding (the small path,
      one launch), untracked and tracked handles alternated, wall time.

Every figure is the median of --reps after --warmup.  Writes
profiles/changes_bench.json (--out) with the library's build id.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.evict_bench import make_names  # noqa: E402

SEC = 10**9
T0 = bench.T0
NOW = T0 + 1000 * SEC
IDLE_NS = 500 * SEC
MARK_KERNELS = ("k_egress_wants", "k_changes_mark")
DRAIN_KERNELS = ("k_changed_count", "k_egress_scan", "k_changed_write")
SWEEP_KERNELS = ("k_sweep_count", "k_sweep_scan", "k_sweep_write")


def med(xs):
    return float(statistics.median(xs)) if xs else None


def by_name(timings):
    tm = {}
    for nm, x in timings:
        tm[nm] = tm.get(nm, 0.0) + x
    return tm


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ops", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="the table the buckets end up in")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--pending", type=int, nargs="*", default=[100, 10000])
    p.add_argument("--host-ops", type=int, default=1024)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "changes_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    n, K, L = args.ops, args.buckets, args.log2_slots
    W, R = args.warmup, args.reps
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    total = 2 * (W + R)   # untracked and tracked steps alternate
    c3 = bench.c3_inputs(types.SimpleNamespace(ops=n, zipf=1.1, warmup=0, steps=total,
                                               c3_clock="above"), torch, dev, K, 0, gen)
    blob, offs, kind = c3["blob"], c3["offs"], c3["kind"]
    freq, per, cnt = c3["freq"], c3["per"], c3["cnt"]
    out = dict(tool="tools/changes_bench.py", build_id=_lib.build_id(), ops=n, buckets=K,
               log2_slots=L, zipf=1.1, take_frac=float((kind == 0).double().mean()), reps=R,
               warmup=W, device=torch.cuda.get_device_name(0))

    kb, ko = make_names(torch, K, 0.0, dev)
    st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
    st[:, 0] = 0x4024000000000000
    st[:, 1] = 0x4008000000000000
    st[:, 2] = torch.arange(K, dtype=torch.int64, device=dev)
    perm = torch.randperm(K, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    st[:, 3] = NOW
    st[perm[:K // 2], 3] = T0
    repos = {}
    for mode in ("untracked", "tracked"):
        r = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct,
                               track_changes=mode == "tracked")
        r.seed_device(kb, ko, st, K)
        assert len(r) == K and r.capacity == 1 << L
        r.set_timing(True)
        repos[mode] = r
    del st
    on = repos["tracked"]
    assert on.changes_count()["pending"] == 0   # a seed marks nothing

    # (a) device pointers, untracked and tracked steps alternating
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    rem, have = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(2))
    rows = dict(untracked=[], tracked=[])
    for j in range(total):
        now, a, t, e = c3["steps"][j]
        mode = "tracked" if j % 2 else "untracked"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        repos[mode].apply_mixed_device(n, kind, blob, offs, now, freq, per, cnt, a, t, e,
                                       status=status, remaining=rem, have=have)
        wall = (time.perf_counter() - t0) * 1e3
        rows[mode].append(dict(wall_ms=wall, kernels=by_name(repos[mode].timings())))
    keep = {m: v[W:] for m, v in rows.items()}
    mk = {k: med([r["kernels"].get(k, 0.0) for r in keep["tracked"]]) for k in MARK_KERNELS}
    out["c3_device"] = dict(
        untracked_wall_ms=med([r["wall_ms"] for r in keep["untracked"]]),
        tracked_wall_ms=med([r["wall_ms"] for r in keep["tracked"]]),
        untracked_wall_all=[round(r["wall_ms"], 4) for r in keep["untracked"]],
        tracked_wall_all=[round(r["wall_ms"], 4) for r in keep["tracked"]],
        mark_kernels_ms=mk, mark_kernels_total_ms=sum(mk.values()),
        untracked_kernel_names=sorted(keep["untracked"][-1]["kernels"]),
        tracked_kernel_names=sorted(keep["tracked"][-1]["kernels"]),
        last_tracked_step_kernels_ms=keep["tracked"][-1]["kernels"])
    print(json.dumps(out["c3_device"]), flush=True)
    repos["untracked"].close()

    # (b) drains of the tracked handle, then the sweeps over the same table
    full = on.changes_count()
    cap = (full["bytes"] + 15) // 8 * 8 + 8
    dr_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    dr_offs = torch.zeros(full["n"] + 2, dtype=torch.int64, device=dev)
    max_msgs = full["n"] + 1

    def drain_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = on.export_changed_device(dr_out, dr_offs, max_msgs)
        wall = (time.perf_counter() - t0) * 1e3
        assert d["done"], d
        return dict(wall_ms=wall, kernels=by_name(on.timings()), **d)

    def summarise(rs):
        ks = {k: med([r["kernels"].get(k, 0.0) for r in rs]) for k in DRAIN_KERNELS}
        return dict(kernels_ms=ks, kernels_total_ms=sum(ks.values()),
                    wall_ms=med([r["wall_ms"] for r in rs]), datagrams=med([r["n"] for r in rs]),
                    requests=med([r["n_incast"] for r in rs]), bytes=med([r["bytes"] for r in rs]))

    drains = {}
    rs = []
    for j in range(W + R):
        if j:   # (the first drain takes what (a) left: the same buckets as one step's)
            now, a, t, e = c3["steps"][2 * j + 1]
            on.apply_mixed_device(n, kind, blob, offs, now + 2000 * SEC, freq, per, cnt, a, t, e,
                                  status=status, remaining=rem, have=have)
        rs.append(drain_once())
    drains["one_batch_of_%d_ops" % n] = summarise(rs[W:])
    for P in args.pending:
        ids = torch.randperm(K, device=dev, generator=gen)[:P]
        pb, po = bench.names_for_ids(torch, ids)
        pk = torch.zeros(P, dtype=torch.uint8, device=dev)
        pf = torch.full((P,), 100, dtype=torch.int64, device=dev)
        pp = torch.full((P,), SEC, dtype=torch.int64, device=dev)
        pc = torch.ones(P, dtype=torch.int64, device=dev)
        rs = []
        for j in range(W + R):
            pn = torch.full((P,), NOW + (3000 + j) * SEC, dtype=torch.int64, device=dev)
            on.apply_mixed_device(P, pk, pb, po.to(torch.int32), pn, pf, pp, pc)
            rs.append(drain_once())
            assert rs[-1]["n"] == P and rs[-1]["n_incast"] == 0, rs[-1]
        drains["%d_pending" % P] = summarise(rs[W:])
    out["drain"] = drains
    print(json.dumps(drains), flush=True)
    del dr_out, dr_offs

    cnt_all = on.sweep_count()
    sw_out = torch.zeros((cnt_all["bytes"] + 15) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    sw_offs = torch.zeros(K + 2, dtype=torch.int64, device=dev)
    sweeps = {}
    for name, idle_ns in (("sweep_one_call", 0), ("sweep_idle_filtered", IDLE_NS)):
        rs = []
        for _ in range(W + R):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nrec, _, s = on.export_sweep_device(sw_out, sw_offs, None, K + 1, NOW, idle_ns)
            wall = (time.perf_counter() - t0) * 1e3
            assert s["done"], s
            rs.append(dict(wall_ms=wall, kernels=by_name(on.timings()), n=nrec))
        rs = rs[W:]
        ks = {k: med([r["kernels"].get(k, 0.0) for r in rs]) for k in SWEEP_KERNELS}
        sweeps[name] = dict(kernels_ms=ks, kernels_total_ms=sum(ks.values()),
                            wall_ms=med([r["wall_ms"] for r in rs]), records=rs[-1]["n"])
    out["sweep"] = sweeps
    full_ms = sweeps["sweep_one_call"]["kernels_total_ms"]
    out["ratios"] = {k + "_over_full_sweep_kernels": v["kernels_total_ms"] / full_ms
                     for k, v in drains.items()}
    out["ratios"].update({k + "_over_full_sweep_wall": v["wall_ms"] / sweeps["sweep_one_call"]["wall_ms"]
                          for k, v in drains.items()})
    print(json.dumps(dict(sweep=sweeps, ratios=out["ratios"])), flush=True)
    on.close()
    del sw_out, sw_offs

    # (c) host batches: the stream's first ops, untracked against tracked
    m = args.host_ops
    h_offs = offs[:m + 1].cpu().numpy()
    h_blob = blob[:int(h_offs[-1])].cpu().numpy().tobytes()
    names = [h_blob[int(h_offs[i]):int(h_offs[i + 1])] for i in range(m)]
    cols = [x[:m].cpu().numpy() for x in (kind, freq, per, cnt)]
    hrepos = dict(untracked=patrol_amd.GPURepo(device=0, log2_slots=20),
                  tracked=patrol_amd.GPURepo(device=0, log2_slots=20, track_changes=True))
    ms = dict(untracked=[], tracked=[])
    for j in range(W + R):
        now, a, t, e = (x[:m].cpu().numpy() for x in c3["steps"][j])
        for mode, rp in hrepos.items():
            t0 = time.perf_counter()
            rp.apply_mixed(cols[0], names, now, cols[1], cols[2], cols[3].astype(np.uint64),
                           a.view(np.uint64), t.view(np.uint64), e)
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    pend = hrepos["tracked"].changes_count()
    out["host"] = {str(m): dict(
        untracked_ms=med(ms["untracked"][W:]), tracked_ms=med(ms["tracked"][W:]),
        untracked_all=[round(x, 4) for x in ms["untracked"][W:]],
        tracked_all=[round(x, 4) for x in ms["tracked"][W:]], pending_after=pend["pending"],
        note="host clock around the binding's call, numpy staging included on both sides")}
    print(json.dumps(out["host"]), flush=True)
    for rp in hrepos.values():
        rp.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"], ratios=out["ratios"])))


if __name__ == "__main__":
    main()
