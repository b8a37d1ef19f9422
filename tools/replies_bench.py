#!/usr/bin/env python3
"""What a batch's incast replies cost (not the bench): three ways to receive
the same batch, in one process, on twin handles over the C2 table (10M
buckets), Zipf 1.1 batches of 2^24 and 2^16 messages holding 0, 64 and 4096
incast requests to existing buckets, device pointers.

  (a) phip_receive_soa, statuses only (what bench.py times; no replies);
  (b) phip_receive_soa with the full status and reply columns, both copied to
      pinned host memory, and the host phip_incast_replies over them;
  (c) phip_receive_soa_replies with no result column at all.

Per form: the kernels' own time (phip_last_timings, HIP events, summed over
the call's launches) and the call's wall time (a host clock around work that
ends in a stream synchronise; (b) includes its two copies and the host loop).
The three forms alternate inside every repetition; every figure is the median
of --reps after --warmup.  (c)'s datagrams are compared with (b)'s once per
shape, and with no request (c)'s launches are compared with (a)'s by name.
Writes profiles/replies_bench.json (--out) with the library's build id.
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
from tools.evict_bench import make_names  # noqa: E402

SEC = 10**9
T0 = bench.T0
REPLY_KERNELS = ("k_reply_select", "k_reply_write", "k_reply_count", "k_reply_scan", "k_reply_place")


def med(xs):
    return float(statistics.median(xs)) if xs else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="the table the buckets end up in")
    p.add_argument("--sizes", type=int, nargs="*", default=[1 << 24, 1 << 16])
    p.add_argument("--requests", type=int, nargs="*", default=[0, 64, 4096])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "replies_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    K, L, W, R = args.buckets, args.log2_slots, args.warmup, args.reps
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    out = dict(tool="tools/replies_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               zipf=1.1, reps=R, warmup=W, isolate=True, device=torch.cuda.get_device_name(0),
               forms=dict(a="phip_receive_soa, status only",
                          b="phip_receive_soa, status + reply columns, copied to pinned host "
                            "memory, phip_incast_replies on the host",
                          c="phip_receive_soa_replies, no result column"))

    kb, ko = make_names(torch, K, 0.0, dev)
    st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
    st[:, 0] = 0x4024000000000000            # added 10.0
    st[:, 1] = 0x4008000000000000            # taken 3.0
    st[:, 2] = torch.arange(K, dtype=torch.int64, device=dev)
    st[:, 3] = T0
    repos = {}
    for f in "abc":   # twins: one placement seed, the dirty buckets of every batch set apart
        g = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct,
                               hash_seed=7, isolate=True)
        g.seed_device(kb, ko, st, K)
        assert len(g) == K and g.capacity == 1 << L
        g.set_timing(True)
        repos[f] = g
    del st, kb, ko
    Lc = repos["a"].L
    max_msgs = max(max(args.requests), 1)
    rq_out = torch.zeros(256 * max_msgs + 8, dtype=torch.uint8, device=dev)
    rq_offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
    rq_src = torch.zeros(max_msgs, dtype=torch.int32, device=dev)
    h_out = np.zeros(256 * max_msgs + 8, np.uint8)
    h_offs = np.zeros(max_msgs + 1, np.uint64)

    shapes = {}
    step = 0
    for n in args.sizes:
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        reply = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        h_status = torch.zeros(n, dtype=torch.uint8).pin_memory()
        h_reply = torch.zeros((n, 4), dtype=torch.int64).pin_memory()
        for q in args.requests:
            step += 1
            ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
            blob, offs = bench.names_for_ids(torch, ids)
            a, t, e = bench.replica_states(torch, gen, n, step, dev)
            if q:
                pos = torch.randperm(n, device=dev, generator=gen)[:q]
                a[pos], t[pos], e[pos] = 0, 0, 0
            now = T0 + step * SEC
            # the wire form of the batch on the host, for (b)'s phip_incast_replies (names)
            wb, wo = bench.datagrams(torch, blob, offs, a, t, e)
            h_wb, h_wo = wb.cpu().numpy(), wo.cpu().numpy().astype(np.uint64)
            del wb, wo, ids
            rows = {f: [] for f in "abc"}
            m = C.c_uint32()
            for _ in range(W + R):
                for f in "abc":
                    g = repos[f]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if f == "a":
                        g.receive_soa(blob, a, t, e, now, name_offs=offs, n=n, status=status,
                                      device=True)
                        r = None
                    elif f == "b":
                        g.receive_soa(blob, a, t, e, now, name_offs=offs, n=n, status=status,
                                      device=True, reply=reply)
                        tm = g.timings()
                        h_status.copy_(status, non_blocking=True)
                        h_reply.copy_(reply, non_blocking=True)
                        torch.cuda.synchronize()
                        rc = Lc.phip_incast_replies(h_wb.ctypes.data, h_wo.ctypes.data, n,
                                                    h_status.data_ptr(), h_reply.data_ptr(), None,
                                                    h_out.ctypes.data, h_out.size - 8,
                                                    h_offs.ctypes.data, None, C.byref(m))
                        assert rc == 0, rc
                        r = dict(n=m.value, bytes=int(h_offs[m.value]))
                    else:
                        r = g.receive_soa_replies_device(n, blob, offs, a, t, e, now, rq_out,
                                                         rq_offs, rq_src, max_msgs)
                    wall = (time.perf_counter() - t0) * 1e3
                    if f != "b":
                        tm = g.timings()
                    rows[f].append(dict(wall_ms=wall, kernel_ms=sum(x for _, x in tm),
                                        launches=sorted(nm for nm, _ in tm),
                                        reply_kernels_ms=sum(x for nm, x in tm if nm in REPLY_KERNELS),
                                        ordered=g.last_stats()[4], r=r))
            rb, rc_ = rows["b"][-1]["r"], rows["c"][-1]["r"]
            assert (rc_["n"], rc_["bytes"]) == (rb["n"], rb["bytes"]) and rc_["replies"] == rb["n"], \
                (rb, {k: rc_[k] for k in ("n", "bytes", "replies", "skipped")})
            nb = rb["bytes"]
            assert bytes(rq_out[:nb].cpu().numpy()) == bytes(h_out[:nb]), "datagrams differ"
            keep = {f: v[W:] for f, v in rows.items()}
            row = dict(messages=n, requests=q, replies=rb["n"], reply_bytes=nb,
                       ordered_messages=keep["c"][-1]["ordered"])
            for f in "abc":
                row[f] = dict(kernel_ms=med([x["kernel_ms"] for x in keep[f]]),
                              call_ms=med([x["wall_ms"] for x in keep[f]]),
                              kernel_all=[round(x["kernel_ms"], 4) for x in keep[f]],
                              call_all=[round(x["wall_ms"], 4) for x in keep[f]])
            row["c"]["reply_kernels_ms"] = med([x["reply_kernels_ms"] for x in keep["c"]])
            row["c"]["launches"] = keep["c"][-1]["launches"]
            row["c_launches_equal_a"] = all(x["launches"] == y["launches"]
                                            for x, y in zip(keep["a"], keep["c"]))
            for k in ("kernel_ms", "call_ms"):
                row["c_over_a_" + k] = row["c"][k] / row["a"][k]
                row["c_over_b_" + k] = row["c"][k] / row["b"][k]
            shapes["%d_%d" % (n, q)] = row
            print(json.dumps({"%d_%d" % (n, q): {k: v for k, v in row.items() if k not in "abc"}}),
                  flush=True)
            del blob, offs, a, t, e, h_wb, h_wo
        del status, reply, h_status, h_reply
    out["shapes"] = shapes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
