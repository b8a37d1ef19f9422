#!/usr/bin/env python3
"""What a peek costs (not the bench): phip_peek beside the lookup-only kernel
of phip_export_datagrams and beside phip_get, in one process on one build.

The table is C2's: 10M buckets b"b%d" in 2^25 slots (opened at 2^20 with
max_load_pct 45), each holding 7 tokens of a 100:1s rate.  Names are drawn as
C3 draws them: Zipf 1.1 over the 10M buckets.

  (a) one name, host pointers: phip_peek against phip_get, the host clock
      around the C call (structs prebuilt, no numpy in the loop).
  (b) 1024 queries, host pointers: phip_peek against phip_export_datagrams over
      the same names; wall time and the kernel's own time.
  (c) 2^20 and 2^24 queries, device pointers, all granted (count 1) and all
      denied with a later answer (count 50: every lane bisects), each run
      alternating with phip_export_datagrams over the same names.

Kernel times are HIP events around the launch (phip_last_timings), the median
of --reps after --warmup.  Writes profiles/peek_bench.json (--out) with the
library's build id and the peek / export ratios.
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
NOW = T0 + 1000 * SEC


def med(xs):
    return float(statistics.median(xs)) if xs else None


def kernel_ms(repo, name):
    return sum(ms for nm, ms in repo.timings() if nm == name)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="the table the buckets end up in")
    p.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 1 << 24])
    p.add_argument("--host-batch", type=int, default=1024)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "peek_bench.json"))
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
    out = dict(tool="tools/peek_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               zipf=1.1, reps=R, warmup=W, device=torch.cuda.get_device_name(0))

    kb, ko = make_names(torch, K, 0.0, dev)
    st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
    st[:, 0] = 0x4024000000000000            # added 10.0
    st[:, 1] = 0x4008000000000000            # taken 3.0
    st[:, 2] = torch.arange(K, dtype=torch.int64, device=dev)
    st[:, 3] = T0
    g = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct)
    g.seed_device(kb, ko, st, K)
    assert len(g) == K and g.capacity == 1 << L
    del st, kb, ko
    g.set_timing(True)
    L_ = g.L
    # every `last` lies in [T0, T0 + 10 ms): at this reading a bucket holds at
    # most 8 of its 100 tokens, so count 1 is granted and count 50 is denied
    # with an answer about 0.4 s later
    now_q = T0 + 10_000_001

    # (c) device batches
    device = {}
    for n in args.sizes:
        ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
        blob, offs = bench.names_for_ids(torch, ids)
        nb = int(offs[-1])
        now = torch.full((n,), now_q, dtype=torch.int64, device=dev)
        freq = torch.full((n,), 100, dtype=torch.int64, device=dev)
        per = torch.full((n,), SEC, dtype=torch.int64, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        rem, have, at = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
        ex_out = torch.zeros(25 * n + nb + 8, dtype=torch.uint8, device=dev)
        found = torch.zeros(n, dtype=torch.uint8, device=dev)
        row = {}
        for label, c in (("all_ok", 1), ("all_denied", 50)):
            cnt = torch.full((n,), c, dtype=torch.int64, device=dev)
            pk, ex, wall = [], [], []
            for _ in range(W + R):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.peek_device(n, blob, offs, now, freq, per, cnt, status=status, remaining=rem,
                              have=have, retry_at=at, names_len=0)
                wall.append((time.perf_counter() - t0) * 1e3)
                pk.append(kernel_ms(g, "k_peek"))
                g._check(L_.phip_export_datagrams(g.h, blob.data_ptr(), offs.data_ptr(), n,
                                                  ex_out.data_ptr(), found.data_ptr(),
                                                  _lib.DEVICE_PTRS))
                ex.append(kernel_ms(g, "k_export"))
            want = _lib.ST_TAKE_OK if c == 1 else _lib.ST_TAKE_DENIED
            assert bool((status == want).all()) and bool(found.all())
            assert bool((at == now_q).all()) if c == 1 else bool((at > now_q).all())
            row[label] = dict(k_peek_ms=med(pk[W:]), k_export_ms=med(ex[W:]),
                              peek_call_wall_ms=med(wall[W:]),
                              peek_over_export=med(pk[W:]) / med(ex[W:]),
                              k_peek_all=[round(x, 4) for x in pk[W:]],
                              k_export_all=[round(x, 4) for x in ex[W:]])
        row["denied_over_ok"] = row["all_denied"]["k_peek_ms"] / row["all_ok"]["k_peek_ms"]
        device[str(n)] = row
        print(json.dumps({str(n): row}), flush=True)
        del ids, blob, offs, now, freq, per, status, rem, have, at, ex_out, found
    out["device"] = device

    # (a), (b) host pointers: structs built once, the C call alone timed
    def host_batch(m):
        ids = bench.zipf_ids(torch, gen, m, K, 1.1, dev).cpu().numpy()
        names = [b"b%d" % int(i) for i in ids]
        blob, offs = patrol_amd.names_blob(names)
        cols = dict(now=np.full(m, now_q, np.int64), freq=np.full(m, 100, np.int64),
                    per=np.full(m, SEC, np.int64), count=np.ones(m, np.uint64))
        res = dict(status=np.zeros(m, np.uint8), remaining=np.zeros(m, np.uint64),
                   have=np.zeros(m, np.uint64), retry_at=np.zeros(m, np.int64))
        q = _lib.phip_ops(m, 0, None, blob.ctypes.data, offs.ctypes.data, cols["now"].ctypes.data,
                          cols["freq"].ctypes.data, cols["per"].ctypes.data,
                          cols["count"].ctypes.data, None, None, None)
        r = _lib.phip_peek_results(res["status"].ctypes.data, res["remaining"].ctypes.data,
                                   res["have"].ctypes.data, res["retry_at"].ctypes.data, None)
        keep = (blob, offs, cols, res)
        return names, blob, offs, q, r, res, keep

    host = {}
    names, blob, offs, q, r, res, keep = host_batch(1)
    state = _lib.phip_state()
    pw, gw = [], []
    for _ in range(50 * (W + R)):
        t0 = time.perf_counter()
        rc = L_.phip_peek(g.h, C.byref(q), C.byref(r), 0)
        pw.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0 and res["status"][0] == _lib.ST_TAKE_OK
        t0 = time.perf_counter()
        rc = L_.phip_get(g.h, names[0], len(names[0]), C.byref(state))
        gw.append((time.perf_counter() - t0) * 1e6)
        assert rc == 1
    host["1"] = dict(phip_peek_us=med(pw[50 * W:]), phip_get_us=med(gw[50 * W:]),
                     peek_over_get=med(pw[50 * W:]) / med(gw[50 * W:]))
    m = args.host_batch
    names, blob, offs, q, r, res, keep = host_batch(m)
    ex_out = np.zeros(25 * m + int(offs[-1]) + 8, np.uint8)
    found = np.zeros(m, np.uint8)
    pw, ew, pk, ek = [], [], [], []
    for _ in range(5 * (W + R)):
        t0 = time.perf_counter()
        rc = L_.phip_peek(g.h, C.byref(q), C.byref(r), 0)
        pw.append((time.perf_counter() - t0) * 1e6)
        pk.append(kernel_ms(g, "k_peek") * 1e3)
        assert rc == 0 and bool((res["status"] == _lib.ST_TAKE_OK).all())
        t0 = time.perf_counter()
        rc = L_.phip_export_datagrams(g.h, blob.ctypes.data, offs.ctypes.data, m,
                                      ex_out.ctypes.data, found.ctypes.data, 0)
        ew.append((time.perf_counter() - t0) * 1e6)
        ek.append(kernel_ms(g, "k_export") * 1e3)
        assert rc == 0 and bool(found.all())
    host[str(m)] = dict(phip_peek_us=med(pw[5 * W:]), phip_export_datagrams_us=med(ew[5 * W:]),
                        k_peek_us=med(pk[5 * W:]), k_export_us=med(ek[5 * W:]),
                        peek_over_export_wall=med(pw[5 * W:]) / med(ew[5 * W:]))
    host["note"] = "host clock around the C call; four result columns copied back by the peek"
    out["host"] = host
    print(json.dumps(host), flush=True)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
