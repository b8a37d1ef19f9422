#!/usr/bin/env python3
"""What the coalesced egress costs (not the bench): phip_apply_mixed against
phip_apply_mixed_egress in one process, on one build.

  (a) C3's mix at one chunk -- 2^24 ops, 50 % Take at 100:1s and 50 % received
      replica states, Zipf 1.1 over 10M buckets, device pointers -- alternating
      a plain step and an egress step on the same table (every step applies
      the stream one second later with fresh replica states): the wall time of
      each call (it ends in a stream synchronise), the egress kernels' own
      times from phip_last_timings (HIP events), and the datagrams an egress
      step wrote against what per-op replication sends (one per TAKE, plus one
      request per bucket a TAKE created).
  (b) The yardstick, in the same run: one phip_export_sweep over the table
      those steps left (k_sweep_count + k_sweep_scan + k_sweep_write), per
      exported record, beside the egress kernels' time per datagram.
  (c) Host batches of 1024 ops (the small path, one launch) and 65,536 ops of
      the same stream, plain against egress, wall time.

Every figure is the median of --reps steps after --warmup.  Writes
profiles/egress_bench.json (--out) with the library's build id.
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

EGRESS_KERNELS = ("k_egress_wants", "k_egress_count", "k_egress_scan", "k_egress_write")
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
    p.add_argument("--log2-slots", type=int, default=25)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--host-sizes", type=int, nargs="*", default=[1024, 65536])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "egress_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    n, K, L = args.ops, args.buckets, args.log2_slots
    total = 2 * (args.warmup + args.reps)   # plain and egress steps alternate
    c3 = bench.c3_inputs(types.SimpleNamespace(ops=n, zipf=1.1, warmup=0, steps=total,
                                               c3_clock="above"), torch, dev, K, 0, gen)
    blob, offs, kind = c3["blob"], c3["offs"], c3["kind"]
    freq, per, cnt = c3["freq"], c3["per"], c3["cnt"]
    out = dict(tool="tools/egress_bench.py", build_id=_lib.build_id(), ops=n, buckets=K, zipf=1.1,
               take_frac=float((kind == 0).double().mean()), reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))

    # (a) device pointers, the same table, plain and egress steps alternating
    repo = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20)
    repo.set_timing(True)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    rem, have = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(2))
    max_msgs, cap = repo.egress_caps(n, int(blob.numel()), device=True)
    eg_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    eg_offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
    rows = dict(plain=[], egress=[])
    takes = int((kind == 0).sum())
    for j in range(total):
        now, a, t, e = c3["steps"][j]
        mode = "egress" if j % 2 else "plain"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "plain":
            repo.apply_mixed_device(n, kind, blob, offs, now, freq, per, cnt, a, t, e,
                                    status=status, remaining=rem, have=have)
            r = None
        else:
            r = repo.apply_mixed_egress_device(n, kind, blob, offs, now, eg_out, eg_offs, max_msgs,
                                               freq=freq, per=per, count=cnt, added=a, taken=t,
                                               elapsed=e, status=status, remaining=rem, have=have)
        wall = (time.perf_counter() - t0) * 1e3
        row = dict(wall_ms=wall, kernels=by_name(repo.timings()))
        if r:
            created = int(((status & 0x80) != 0)[kind == 0].sum())
            row.update(r, per_op=takes + created)
        rows[mode].append(row)
    keep = {m: v[args.warmup:] for m, v in rows.items()}
    eg_rows = keep["egress"]
    eg_k = {k: med([r["kernels"].get(k, 0.0) for r in eg_rows]) for k in EGRESS_KERNELS}
    eg_ms = sum(eg_k.values())
    last = eg_rows[-1]
    out["c3_device"] = dict(
        plain_wall_ms=med([r["wall_ms"] for r in keep["plain"]]),
        egress_wall_ms=med([r["wall_ms"] for r in eg_rows]),
        plain_wall_all=[round(r["wall_ms"], 4) for r in keep["plain"]],
        egress_wall_all=[round(r["wall_ms"], 4) for r in eg_rows],
        egress_kernels_ms=eg_k, egress_kernels_total_ms=eg_ms,
        datagrams=med([r["n"] for r in eg_rows]), requests=med([r["n_incast"] for r in eg_rows]),
        bytes=med([r["bytes"] for r in eg_rows]), per_op_datagrams=med([r["per_op"] for r in eg_rows]),
        egress_ns_per_datagram=1e6 * eg_ms / max(1, med([r["n"] for r in eg_rows])),
        last_step_kernels_ms=last["kernels"], buckets=len(repo))
    print(json.dumps(out["c3_device"]), flush=True)

    # (b) the sweep over the same table, one call covering every slot
    sw_msgs = 1 << (L - 1)
    cnt_all = repo.sweep_count()
    sw_out = torch.zeros((cnt_all["bytes"] + 15) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    sw_offs = torch.zeros(sw_msgs + 1, dtype=torch.int64, device=dev)
    sw_rows = []
    for _ in range(args.warmup + args.reps):
        nrec, _, st = repo.export_sweep_device(sw_out, sw_offs, None, sw_msgs)
        assert st["done"] and nrec == cnt_all["n"], (st, cnt_all)
        sw_rows.append(by_name(repo.timings()))
    sw_k = {k: med([r.get(k, 0.0) for r in sw_rows[args.warmup:]]) for k in SWEEP_KERNELS}
    out["sweep_yardstick"] = dict(records=cnt_all["n"], bytes=cnt_all["bytes"], kernels_ms=sw_k,
                                  total_ms=sum(sw_k.values()),
                                  ns_per_record=1e6 * sum(sw_k.values()) / max(1, cnt_all["n"]))
    print(json.dumps(out["sweep_yardstick"]), flush=True)
    repo.close()
    del eg_out, eg_offs, sw_out, sw_offs

    # (c) host batches: the stream's first ops, plain against egress
    h_offs = offs[:max(args.host_sizes) + 1].cpu().numpy()
    h_blob = blob[:int(h_offs[-1])].cpu().numpy().tobytes()
    out["host"] = {}
    for m in args.host_sizes:
        names = [h_blob[int(h_offs[i]):int(h_offs[i + 1])] for i in range(m)]
        cols = [x[:m].cpu().numpy() for x in (kind, freq, per, cnt)]
        repos = dict(plain=patrol_amd.GPURepo(device=0, log2_slots=20),
                     egress=patrol_amd.GPURepo(device=0, log2_slots=20))
        ms = dict(plain=[], egress=[])
        n_dg = []
        for j in range(args.warmup + args.reps):
            now, a, t, e = (x[:m].cpu().numpy() for x in c3["steps"][j])
            for mode, rp in repos.items():
                t0 = time.perf_counter()
                r = rp.apply_mixed(cols[0], names, now, cols[1], cols[2], cols[3].astype(np.uint64),
                                   a.view(np.uint64), t.view(np.uint64), e, egress=mode == "egress")
                ms[mode].append((time.perf_counter() - t0) * 1e3)
                if mode == "egress":
                    n_dg.append(r["egress"]["n"])
        out["host"][str(m)] = dict(
            plain_ms=med(ms["plain"][args.warmup:]), egress_ms=med(ms["egress"][args.warmup:]),
            datagrams=med(n_dg[args.warmup:]), per_op_datagrams_at_least=int((cols[0] == 0).sum()),
            note="host clock around the binding's call, numpy staging included on both sides")
        print(json.dumps({m: out["host"][str(m)]}), flush=True)
        for rp in repos.values():
            rp.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
