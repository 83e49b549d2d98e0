"""The token ring's two device entries against their yardsticks, timed with
HIP events in alternating rounds, answers compared first.

1. cb_ring_route_fixed of 1M 16-byte device keys over a 3x8 ring (searched in
   LDS) and a 64x256 ring (searched in global memory behind its bucket table),
   against
     * cb_set_probe_fixed of the same keys on a 32-slot m = 1024 set: the
       project's other one-hash-per-key kernel, the floor. Timed twice: as the
       library runs it (1M keys on a 4 KiB set count as a dense batch, so it
       takes the region-partitioned probe) and with cb_set_dense(-1), which is
       k_set_probe, one lane per key like the route; cb_last_path of each is
       recorded;
     * a single-thread host loop of cb_ring_replicas over the same keys: what a
       caller does today. It is a Python loop over ctypes calls, so it carries
       the binding's per-call cost; it is timed by the wall clock, a few rounds.
2. cb_tables_compact_ring for one node of a 3-node ring with rf = 1 and rf = 3
   against cb_tables_compact of the same tables, at the two shapes of
   tools/ubench_lww.py (300 x 1024 lines; 4 x 512K lines). The keys have no
   namespace, so the rules are the one empty prefix with npk = 0.

Per measurement: the times, the ratio per round (median, min, max) beside the
yardstick's own spread, and for the compactions the launch lists of both
entries (cb_profile_read): two more launches are expected.

Prints one JSON line per measurement (also appended to --out). Diagnostic only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ubench_lww import KERNELS, launch_list, make_tables, rounds_ms, stats  # noqa: E402

RING_KERNELS = ["k_ring_route", "k_ring_keep"]


def ratio(a, b):
    r = np.array(a) / np.array(b)
    return {"median": round(float(np.median(r)), 3), "min": round(float(r.min()), 3), "max": round(float(r.max()), 3)}


def route_part(mods, args, dev):
    lsmt_amd, workload, L = mods
    from lsmt_amd import ring
    n = 1 << 20
    keys = np.ascontiguousarray(workload.key_range(4242, n))
    dkeys = torch.from_numpy(keys).to(dev)
    rings = {"3x8": ring.Ring([b"http://n%d" % i for i in range(3)], 8, 2),
             "64x256": ring.Ring([b"http://n%d" % i for i in range(64)], 256, 3)}
    assert rings["3x8"].positions <= ring.LDS_POSITIONS < rings["64x256"].positions
    filters = []
    for f in range(32):
        bf = lsmt_amd.BloomFilter(1024, device=0)
        bf.insert_batch(workload.key_range(100 + f, 64))
        filters.append(bf)
    fset = lsmt_amd.FilterSet.from_filters(filters)
    s = torch.cuda.Stream(dev)
    hits = torch.zeros((32, n // 64), dtype=torch.int64, device=dev)
    out = {k: (torch.zeros(n, dtype=torch.uint32, device=dev), torch.zeros((n, r.rf), dtype=torch.int32, device=dev))
           for k, r in rings.items()}

    def route(name):
        r, (tok, rep) = rings[name], out[name]
        return lambda: lsmt_amd._lib.check(L.cb_ring_route_fixed(r._h, dkeys.data_ptr(), 16, n, 0, 0, 0, tok.data_ptr(),
                                                                 rep.data_ptr(), s.cuda_stream))

    def host_loop(r, count):
        tok, rep = ctypes.c_uint32(), (ctypes.c_int32 * r.rf)()
        ptr, fn, h = keys.ctypes.data, L.cb_ring_replicas, r._h
        toks, reps = np.zeros(count, np.uint32), np.zeros((count, r.rf), np.int32)
        t0 = time.perf_counter()
        for i in range(count):
            fn(h, ptr + 16 * i, 16, 0, 0, ctypes.byref(tok), rep)
            toks[i] = tok.value
            reps[i] = rep
        return (time.perf_counter() - t0) * 1e3, toks, reps

    # answers first: the device's against the host entry's, every key
    rows = []
    host_ms = {}
    for name, r in rings.items():
        route(name)()
        s.synchronize()
        ms, toks, reps = host_loop(r, n)
        host_ms[name] = [ms] + [host_loop(r, n)[0] for _ in range(args.host_reps - 1)]
        assert np.array_equal(out[name][0].cpu().numpy(), toks) and np.array_equal(out[name][1].cpu().numpy(), reps), name
    probe = lambda: fset.probe(lsmt_amd.DeviceKeys(dkeys), out=hits, stream=s.cuda_stream)  # noqa: E731

    def probe_plain():  # k_set_probe whatever the batch's density (the library's own choice here is the dense probe)
        lsmt_amd.set_dense(-1)
        try:
            return probe()
        finally:
            lsmt_amd.set_dense(0)

    paths = {}
    for name, fn in (("set_probe", probe), ("set_probe_plain", probe_plain)):
        fn()
        paths[name] = lsmt_amd.last_path()
    fns = {"set_probe": probe, "set_probe_plain": probe_plain, "route_3x8": route("3x8"),
           "route_64x256": route("64x256")}
    ms = rounds_ms(fns, s, args.reps, args.warmup)
    for name in rings:
        t = ms["route_" + name]
        rows.append({"measure": "cb_ring_route_fixed", "ring": name, "keys": n, "key_len": 16,
                     "positions": rings[name].positions, "rf": rings[name].rf,
                     "search": "LDS" if rings[name].positions <= ring.LDS_POSITIONS else "global, bucket table",
                     "answers_equal_host": True, "route": stats(t), "set_probe_32x1024": stats(ms["set_probe"]),
                     "ratio_route_over_set_probe": ratio(t, ms["set_probe"]),
                     "set_probe_32x1024_plain_kernel": stats(ms["set_probe_plain"]),
                     "ratio_route_over_set_probe_plain_kernel": ratio(t, ms["set_probe_plain"]),
                     "set_probe_cb_last_path": paths,
                     "host_loop_cb_ring_replicas": stats(host_ms[name]),
                     "host_loop_over_route_median": round(float(np.median(host_ms[name]) / np.median(t)), 1),
                     "mkeys_per_s": round(n / np.median(t) / 1e3, 1)})
    return rows


def table_keys16(t):
    """uint8[nlines, 16]: the keys of a table whose keys are all 16 bytes."""
    st, kl, _ = t.lines()
    assert (kl == 16).all()
    raw = np.frombuffer(t.data(), np.uint8)
    return raw[st.astype(np.int64)[:, None] + np.arange(16)]


def compact_part(mods, name, nt, per, pool_n, args, dev):
    lsmt_amd, workload, L = mods
    from lsmt_amd import ring
    tables, keys, _ = make_tables(lsmt_amd, workload, nt, per, pool_n, nt, False)
    s = torch.cuda.Stream(dev)
    rules = {b"": 0}  # every key is partitioned, whole
    rows = []
    plain = lsmt_amd.compact(tables, m=1024)[0]
    for rf in (1, 3):
        r = ring.Ring([b"http://n%d" % i for i in range(3)], 8, rf)
        mine = [ring.compact_ring(tables, r, node, rules=rules)[0] for node in range(3)]
        res = {"measure": "cb_tables_compact_ring", "shape": name, "tables": nt, "lines_in": int(len(keys)), "rf": rf,
               "lines_out_compact": plain.nlines, "lines_out_per_node": [t.nlines for t in mine]}
        if rf == 1:  # every key has one owner: node 0's file holds exactly the keys whose primary it is
            assert sum(t.nlines for t in mine) == plain.nlines
            all_keys = table_keys16(plain)
            primary = r.route(all_keys)[1][:, 0]
            assert [r.replicas(k.tobytes())[1][0] for k in all_keys[:5000]] == primary[:5000].tolist()
            assert np.array_equal(table_keys16(mine[0]), all_keys[primary == 0])
        else:  # three nodes, three replicas: every node keeps everything
            assert all(t.data() == plain.data() for t in mine)
        res["answers_checked"] = True
        fns = {"compact": lambda: lsmt_amd.compact(tables, m=1024, stream=s.cuda_stream),
               "compact_ring": lambda: ring.compact_ring(tables, r, 0, rules=rules, stream=s.cuda_stream)}
        ms = rounds_ms(fns, s, args.reps, args.warmup)
        res["compact"], res["compact_ring"] = stats(ms["compact"]), stats(ms["compact_ring"])
        res["ratio_ring_over_compact"] = ratio(ms["compact_ring"], ms["compact"])
        KERNELS[:] = [k for k in KERNELS if k not in RING_KERNELS] + RING_KERNELS
        res["launches_compact"] = launch_list(L, fns["compact"])
        res["launches_compact_ring"] = launch_list(L, fns["compact_ring"])
        count = lambda d: sum(v["launches"] for v in d.values())  # noqa: E731
        res["launch_count"] = {"compact": count(res["launches_compact"]), "compact_ring": count(res["launches_compact_ring"])}
        rows.append(res)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--host-reps", type=int, default=2)
    p.add_argument("--out", default=None)
    p.add_argument("--skip-large", action="store_true", help="leave out the 4 x 512K shape")
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import lsmt_amd
    from lsmt_amd import workload
    from lsmt_amd._lib import load
    mods = (lsmt_amd, workload, load())
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    def emit(rows):  # (as they come: a long run shows where it is)
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")

    emit(route_part(mods, args, dev))
    shapes = [("300 x 1024 lines, 16-byte keys", 300, 1024, 120_000), ("4 x 512K lines, 16-byte keys", 4, 1 << 19, 1_500_000)]
    for name, nt, per, pool_n in shapes[:1 if args.skip_large else 2]:
        emit(compact_part(mods, name, nt, per, pool_n, args, dev))


if __name__ == "__main__":
    main()
