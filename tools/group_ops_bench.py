#!/usr/bin/env python3
"""Owner-routed ops over the shard group, timed (not the bench): C3's mix at
one chunk -- 2^24 ops, 50 % Take at 100:1s and 50 % received replica states,
Zipf 1.1 over 10M buckets -- through

  (a) phip_apply_mixed on one handle: the yardstick, what a single table does;
  (b) GPUGroup.apply_mixed at world 1 with PHIP_GROUP_RCCL_SELF: the pack, the
      RCCL exchange to itself, the owner's apply, the results' way back;
  (c) GPUGroup.apply_mixed over two shards on one GPU (device copies), each
      member submitting half of the stream.

Every step applies the same op stream one second later with fresh replica
states, to the table the earlier steps left, in all three.  A step's time is
a host clock around the call, which ends in a stream synchronise; (b) and (c)
also report phip_group_stage_ms of the last step (pack / both exchanges /
apply + results scatter).  Every figure is the median of --reps steps after
--warmup.  Beside them the pack alone for 8 owners: phip_route_pack_ops'
kernels and phip_route_pack's (without the combine) over the same names, from
phip_last_timings (HIP events).

Writes profiles/group_ops_bench.json (--out) with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def med(xs):
    return float(statistics.median(xs)) if xs else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ops", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="one table holding every bucket")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--route-world", type=int, default=8)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_ops_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    from patrol_amd.engine import phip_msgs
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    n, K, L = args.ops, args.buckets, args.log2_slots
    total = args.warmup + args.reps
    c3 = bench.c3_inputs(types.SimpleNamespace(ops=n, zipf=1.1, warmup=args.warmup, steps=args.reps,
                                               c3_clock="above"), torch, dev, K, 0, gen)
    blob, offs, kind = c3["blob"], c3["offs"], c3["kind"]
    freq, per, cnt = c3["freq"], c3["per"], c3["cnt"]
    out = dict(tool="tools/group_ops_bench.py", build_id=_lib.build_id(), ops=n, buckets=K,
               zipf=1.1, take_frac=float((kind == 0).double().mean()), reps=args.reps,
               warmup=args.warmup, device=torch.cuda.get_device_name(0))

    def batch(j, lo=0, hi=n):
        now, a, t, e = c3["steps"][j]
        o = offs[lo:hi + 1]
        return dict(kind=kind[lo:hi], names=blob, name_offs=o, now=now[lo:hi], freq=freq[lo:hi],
                    per=per[lo:hi], count=cnt[lo:hi], added=a[lo:hi], taken=t[lo:hi],
                    elapsed=e[lo:hi])

    # (a) one handle
    repo = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    rem, have = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(2))
    ms = []
    for j in range(total):
        b = batch(j)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        repo.apply_mixed_device(n, b["kind"], blob, offs, b["now"], freq, per, cnt, b["added"],
                                b["taken"], b["elapsed"], status=status, remaining=rem, have=have)
        ms.append((time.perf_counter() - t0) * 1e3)
    assert bool(status.all())
    want_status = status.clone()
    out["apply_mixed_one_handle"] = dict(ms=med(ms[args.warmup:]), min_ms=min(ms[args.warmup:]),
                                         buckets=len(repo))
    print(json.dumps(out["apply_mixed_one_handle"]), flush=True)
    nb = len(repo)
    repo.close()

    # (b) world 1 through the RCCL self-exchange, (c) two shards on one GPU
    for key, devices, log2 in (("group_world1_rccl_self", [0], L), ("group_shared_world2", [0, 0], L - 1)):
        W = len(devices)
        g = patrol_amd.GPUGroup.open_all(devices, log2_slots=log2, arena_bytes=1 << 20)
        g.set_timing(True)
        cut = [n * i // W for i in range(W + 1)]
        ms = []
        for j in range(total):
            bs = [batch(j, cut[i], cut[i + 1]) for i in range(W)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, sent, applied = g.apply_mixed(bs, rccl_self=W == 1, want_reply=False)
            ms.append((time.perf_counter() - t0) * 1e3)
        assert sum(sent) == n and sum(applied) == n and sum(len(r) for r in g.repos) == nb
        if W == 1:   # one source: the same order as (a), so the same results
            assert torch.equal(res[0]["status"], want_status)
        out[key] = dict(ms=med(ms[args.warmup:]), min_ms=min(ms[args.warmup:]), sent=sent,
                        applied=applied, stage_ms=[g.stage_ms(i) for i in range(W)])
        print(json.dumps(out[key]), flush=True)
        del res
        g.close()

    # the pack alone, 8 owners: the ops pack and the message pack over the same names
    W = args.route_world
    repo = patrol_amd.GPURepo(device=0, log2_slots=10)
    repo.set_timing(True)
    lib = _lib.load()
    now, a, t, e = c3["steps"][0]
    s_names = torch.empty(blob.numel() + 64, dtype=torch.uint8, device=dev)
    s_lens = torch.empty(n, dtype=torch.int32, device=dev)
    s_a, s_t, s_e = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    cw, bw = (torch.zeros(W, dtype=torch.int64, device=dev) for _ in range(2))
    m = phip_msgs(n, 0, blob.data_ptr(), offs.data_ptr(), a.data_ptr(), t.data_ptr(), e.data_ptr())
    ops_ms, msg_ms = [], []
    for _ in range(total):
        b = batch(0)
        repo.route_pack_ops_device(n, W, names_len=0, **b)
        tm = dict()
        for nm, x in repo.timings():
            tm[nm] = tm.get(nm, 0.0) + x
        ops_ms.append(tm)
        torch.cuda.synchronize()
        rc = lib.phip_route_pack(repo.h, C.byref(m), W, s_names.data_ptr(), s_lens.data_ptr(),
                                 s_a.data_ptr(), s_t.data_ptr(), s_e.data_ptr(), cw.data_ptr(),
                                 bw.data_ptr(), _lib.DEVICE_PTRS)
        assert rc == 0 and int(cw.sum()) == n
        tm = dict()
        for nm, x in repo.timings():
            tm[nm] = tm.get(nm, 0.0) + x
        msg_ms.append(tm)

    def kernels(rows):
        return {nm: med([r[nm] for r in rows[args.warmup:]]) for nm in rows[-1]}
    ko, km = kernels(ops_ms), kernels(msg_ms)
    out["route_pack_8_owners"] = dict(
        world=W, phip_route_pack_ops=dict(kernels_ms=ko, total_ms=sum(ko.values())),
        phip_route_pack_no_combine=dict(kernels_ms=km, total_ms=sum(km.values())))
    print(json.dumps(out["route_pack_8_owners"]), flush=True)
    repo.close()
    out["note"] = ("one MI355X; the RCCL exchange at world > 1 (one GPU per rank) has not run on "
                   "hardware")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
