#!/usr/bin/env python3
"""Group receive from the wire, timed (not the bench): 2^24 datagrams, Zipf 1.1
over 10M names, C2's name mix (b"b%d"), through

  (a) phip_route_pack of the pre-decoded messages, 8 owners, with and without
      PHIP_ROUTE_COMBINE;
  (a') the same call in the parent commit's library (--parent-lib, loaded
      beside the new one through _lib.load(path), the PATROLHIP_LIB variant
      hook's loader), alternating with (a) step by step, each first in turn:
      the decoded pack must not move;
  (b) phip_route_pack_datagrams of the same messages as wire datagrams;
  (c) one extra streaming pass over the datagrams: the k_classify time of a
      classify_first handle's phip_receive_datagrams of the same batch;
  (d) phip_group_receive (decoded) and (e) phip_group_receive_datagrams at
      world 1 with PHIP_GROUP_RCCL_SELF and over two shards on one GPU, each
      member holding half of the batch, alternating step by step.

(a), (a'), (b), (c) are sums of HIP-event kernel times (phip_last_timings);
(d), (e) are a host clock around the call ending in a device synchronise, with
phip_group_stage_ms (pack / exchange / merge) beside it.  Every step brings
fresh replica states.  All forms alternate in one process; every figure is the
median of --reps steps after --warmup, with min and max as the spread.

Yardstick: if (b) exceeds (a) + (c), decoding first would have been no worse.

Writes profiles/group_wire_bench.json (--out) with the libraries' build ids.
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


def stat(xs):
    return dict(ms=float(statistics.median(xs)), min_ms=float(min(xs)), max_ms=float(max(xs)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--messages", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="one table holding every bucket")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--route-world", type=int, default=8)
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "var", "libpatrolhip_parent.so"),
                   help="the parent commit's libpatrolhip.so ('' or missing: (a') is not measured)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_wire_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    from patrol_amd.engine import GPURepo, phip_config, phip_msgs, phip_wire
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(13)
    n, K, L, W = args.messages, args.buckets, args.log2_slots, args.route_world
    total = args.warmup + args.reps
    lib = _lib.load()
    out = dict(tool="tools/group_wire_bench.py", build_id=_lib.build_id(), messages=n, buckets=K,
               zipf=1.1, reps=args.reps, warmup=args.warmup, route_world=W,
               device=torch.cuda.get_device_name(0))

    ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
    blob, offs = bench.names_for_ids(torch, ids)
    del ids
    name_bytes = int(offs[-1])

    def states(j):
        return bench.replica_states(torch, gen, n, j, dev)

    # the parent's library beside the new one (same process, own handle)
    parent = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        cur, _lib._lib = _lib._lib, None
        try:
            Lp = _lib.load(args.parent_lib)
        finally:
            _lib._lib = cur
        parent = GPURepo.__new__(GPURepo)
        parent.L, parent.device, parent.owned = Lp, 0, True
        cfg = phip_config(0, 10, 1 << 24, 90, 0, 0, 0, 0)
        h = C.c_void_p()
        assert Lp.phip_open(C.byref(cfg), C.byref(h)) == 0
        parent.h = h
        parent.set_timing(True)
        out["parent_build_id"] = Lp.phip_build_id().decode()
        assert out["parent_build_id"] != out["build_id"], "--parent-lib is this build"

    # ---- the pack alone: (a), (a'), (b), and (c) -------------------------
    repo = patrol_amd.GPURepo(device=0, log2_slots=10)
    repo.set_timing(True)
    cls = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20, classify_first=True)
    cls.set_timing(True)
    s_names = torch.empty(name_bytes + 64, dtype=torch.uint8, device=dev)
    s_lens = torch.empty(n, dtype=torch.int32, device=dev)
    s_a, s_t, s_e = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    cw, bw = (torch.zeros(W, dtype=torch.int64, device=dev) for _ in range(2))
    send = [x.data_ptr() for x in (s_names, s_lens, s_a, s_t, s_e, cw, bw)]

    def kernel_ms(r):
        tm = {}
        for nm, x in r.timings():
            tm[nm] = tm.get(nm, 0.0) + x
        return tm

    rows = {k: [] for k in ("a", "a_combine", "parent_a", "parent_a_combine", "b", "b_combine", "c")}
    sent = {}
    for j in range(total):
        a, t, e = states(j)
        data, doffs = bench.datagrams(torch, blob, offs, a, t, e)
        m = phip_msgs(n, 0, blob.data_ptr(), offs.data_ptr(), a.data_ptr(), t.data_ptr(), e.data_ptr())
        w = phip_wire(n, 0, data.data_ptr(), doffs.data_ptr(), 0)
        torch.cuda.synchronize()
        for comb in (0, _lib.ROUTE_COMBINE):
            sfx = "_combine" if comb else ""
            flags = _lib.DEVICE_PTRS | comb
            pair = (("a", repo), ("parent_a", parent))
            for key, r in (pair if j % 2 == 0 else pair[::-1]):   # neither always runs first
                if r is None:
                    continue
                assert r.L.phip_route_pack(r.h, C.byref(m), W, *send, flags) == 0
                rows[key + sfx].append(kernel_ms(r))
                sent[key + sfx] = int(cw.sum())
            stop = C.c_uint32()
            assert lib.phip_route_pack_datagrams(repo.h, C.byref(w), W, *send, C.byref(stop), flags) == 0
            rows["b" + sfx].append(kernel_ms(repo))
            sent["b" + sfx] = int(cw.sum())
            assert stop.value == n and sent["b" + sfx] == sent["a" + sfx]
        assert cls.receive_datagrams_device(data, doffs, n, bench.T0 + j) == n
        rows["c"].append(kernel_ms(cls))
        del data, doffs, a, t, e
    cls.close()

    def summary(rs):
        rs = rs[args.warmup:]
        tot = stat([sum(r.values()) for r in rs])
        tot["kernels_ms"] = {nm: float(statistics.median([r.get(nm, 0.0) for r in rs])) for nm in rs[-1]}
        return tot
    pack = {k: summary(v) for k, v in rows.items() if v and k != "c"}
    for k in pack:
        pack[k]["sent"] = sent[k]
    out["route_pack"] = pack
    kc = [r.get("k_classify") for r in rows["c"][args.warmup:]]
    out["wire_classify_pass"] = stat(kc) if all(x is not None for x in kc) else None
    c_ms = out["wire_classify_pass"]["ms"] if out["wire_classify_pass"] else None
    for sfx in ("", "_combine"):
        a_, b_ = pack["a" + sfx], pack["b" + sfx]
        r = dict(b_over_a=b_["ms"] / a_["ms"])
        if c_ms is not None:
            r.update(a_plus_c_ms=a_["ms"] + c_ms, b_exceeds_a_plus_c=b_["ms"] > a_["ms"] + c_ms)
        if parent is not None:
            pa_ = pack["parent_a" + sfx]
            spread = max(a_["max_ms"] - a_["min_ms"], pa_["max_ms"] - pa_["min_ms"])
            r.update(a_minus_parent_ms=a_["ms"] - pa_["ms"], run_spread_ms=spread,
                     a_inside_spread=abs(a_["ms"] - pa_["ms"]) <= spread)
        out["pack_ratios" + sfx] = r
    print(json.dumps(dict(route_pack={k: v["ms"] for k, v in pack.items()}, c=c_ms,
                          ratios=out["pack_ratios"], ratios_combine=out["pack_ratios_combine"])),
          flush=True)
    repo.close()
    if parent is not None:
        parent.L.phip_close(parent.h)
        parent.h = None
    del s_names, s_lens, s_a, s_t, s_e

    # ---- the group: (d) decoded vs (e) wire ---------------------------------
    for key, devices, log2 in (("group_world1_rccl_self", [0], L), ("group_shared_world2", [0, 0], L - 1)):
        Wg = len(devices)
        gd = patrol_amd.GPUGroup.open_all(devices, log2_slots=log2, arena_bytes=1 << 20)
        ge = patrol_amd.GPUGroup.open_all(devices, log2_slots=log2, arena_bytes=1 << 20)
        gd.set_timing(True)
        ge.set_timing(True)
        cut = [n * i // Wg for i in range(Wg + 1)]
        d_ms, e_ms, d_st, e_st = [], [], [], []
        for j in range(total):
            a, t, e = states(100 + j)
            data, doffs = bench.datagrams(torch, blob, offs, a, t, e)
            dec = [(blob, offs[cut[i]:cut[i + 1] + 1], a[cut[i]:cut[i + 1]], t[cut[i]:cut[i + 1]],
                    e[cut[i]:cut[i + 1]]) for i in range(Wg)]
            wire = [(data, doffs[cut[i]:cut[i + 1] + 1]) for i in range(Wg)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sd, md = gd.receive(dec, bench.T0 + j, combine=True, rccl_self=Wg == 1)
            torch.cuda.synchronize()
            d_ms.append((time.perf_counter() - t0) * 1e3)
            d_st.append([gd.stage_ms(i) for i in range(Wg)])
            t0 = time.perf_counter()
            se, me, stopped = ge.receive_datagrams(wire, bench.T0 + j, combine=True, rccl_self=Wg == 1,
                                                   checked=False)
            torch.cuda.synchronize()
            e_ms.append((time.perf_counter() - t0) * 1e3)
            e_st.append([ge.stage_ms(i) for i in range(Wg)])
            assert stopped == [cut[i + 1] - cut[i] for i in range(Wg)]
            assert sum(sd) == sum(md) and sum(se) == sum(me)
            del data, doffs, a, t, e, dec, wire
        assert sum(len(r) for r in gd.repos) == sum(len(r) for r in ge.repos)

        def stages(rows):
            rows = rows[args.warmup:]
            return [{s: float(statistics.median([r[i][s] for r in rows]))
                     for s in ("pack", "exchange", "merge")} for i in range(Wg)]
        d, e_ = stat(d_ms[args.warmup:]), stat(e_ms[args.warmup:])
        d.update(stage_ms=stages(d_st), sent=sd, merged=md)
        e_.update(stage_ms=stages(e_st), sent=se, merged=me)
        out[key] = dict(decoded=d, wire=e_, e_over_d=e_["ms"] / d["ms"],
                        pack_stage_e_over_d=sum(x["pack"] for x in e_["stage_ms"]) /
                        max(sum(x["pack"] for x in d["stage_ms"]), 1e-9), buckets=sum(len(r) for r in ge.repos))
        print(json.dumps({key: dict(d=d["ms"], e=e_["ms"], e_over_d=out[key]["e_over_d"],
                                    d_stage=d["stage_ms"], e_stage=e_["stage_ms"])}), flush=True)
        gd.close()
        ge.close()
    out["note"] = ("one MI355X; the RCCL exchange at world > 1 (one GPU per rank) has not run on "
                   "hardware and remains unmeasured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
