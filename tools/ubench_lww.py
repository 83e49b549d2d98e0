"""cb_tables_compact_lww against cb_tables_compact on the device, timed with
HIP events in the same alternating rounds: the two shapes of
tools/ubench_compact.py (300 tables of 1024 lines; 4 tables of 512K lines),
each with two sets of timestamps over the same keys:

  * in table order (a newer table's rows carry greater timestamps): the two
    rules choose the same lines, and the files must be byte-equal;
  * shuffled per key: the LWW file is checked against the per-key maximum
    computed on the host (the winners' timestamps through cb_scan_ts).

Answers are compared first, then timed. Per shape and timestamp set: both
entries' times, the ratio per round (median, min, max) and the launch list of
each (cb_profile_read), so the extra launches of the LWW select are visible
and the plain entry's list can be held against another build's.

--plain-only times the newest-wins entries alone (cb_tables_compact and
cb_tables_scan_many of the 300-table shape's first 16 tables) with their
launch lists; --tree DIR imports lsmt_amd from another checkout's build, so
the same script measures a parent commit's library next to this one's.

Prints one JSON line per measurement (also appended to --out). Diagnostic only.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

KERNELS = ["k_compact_klen", "k_scan_reduce", "k_tile_scan", "k_scan_apply", "k_compact_gather", "k_entry_sort",
           "k_bin_count", "k_bin_offsets", "k_bin_scatter", "k_bin_sort", "k_compact_select", "k_compact_select_live",
           "k_compact_ts", "k_compact_lww_runs", "k_compact_lww_runs_live", "k_compact_lww_tiles", "k_compact_format",
           "k_insert_lds", "k_insert_direct", "k_build_part", "k_build_tile", "k_pfx_masks", "k_table_dir",
           "k_scan_bounds", "k_scan_sources", "k_scan_emit", "k_scan_range_off", "k_scan_count", "k_scan_ts",
           "k_b64_decode", "k_decode_scan"]


def offsets16(n):
    return np.arange(0, 16 * (n + 1), 16, dtype=np.uint64)


def stamped_values(keys, ts):
    """16-byte values: the 8-byte big-endian timestamp, then 8 bytes of the key."""
    v = np.empty((len(keys), 16), np.uint8)
    v[:, :8] = ts.astype(">u8").view(np.uint8).reshape(-1, 8)
    v[:, 8:] = keys[:, :8]
    return v


def make_tables(lsmt_amd, workload, nt, per, pool_n, seed, shuffled):
    """nt tables of ~per lines whose keys come from one pool, newest first.
    In table order table t's rows carry timestamp 10^6 - t; shuffled, every
    line gets a random 40-bit one. Returns (tables, all keys, all timestamps)."""
    rng = np.random.default_rng(seed)
    pool = workload.key_range(4242, pool_n)
    tables, keys, stamps = [], [], []
    for t in range(nt):
        idx = np.unique(rng.choice(len(pool), per, replace=False))
        ks = np.ascontiguousarray(pool[idx])
        ts = rng.integers(1, 1 << 40, len(idx), dtype=np.uint64) if shuffled else np.full(len(idx), 10 ** 6 - t, np.uint64)
        vs = stamped_values(ks, ts)
        kb = lsmt_amd.KeyBatch(n=len(idx), data=ks.reshape(-1), offsets=offsets16(len(idx)))
        vb = lsmt_amd.KeyBatch(n=len(idx), data=vs.reshape(-1), offsets=offsets16(len(idx)))
        tables.append(lsmt_amd.sstable_create((kb, vb), m=1024)[0])
        keys.append(ks)
        stamps.append(ts)
    return tables, np.concatenate(keys), np.concatenate(stamps)


def rounds_ms(fns, stream, reps, warm):
    """Device time per call of every fn, one after the other in each round
    (so all see the same clocks and neighbours): {name: [ms per round]}."""
    out = {k: [] for k in fns}
    with torch.cuda.stream(stream):
        for i in range(warm + reps):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                keep = fn()
                e1.record(stream)
                e1.synchronize()
                del keep
                if i >= warm:
                    out[name].append(e0.elapsed_time(e1))
    return out


def stats(xs):
    return {"min_ms": round(float(np.min(xs)), 4), "median_ms": round(float(np.median(xs)), 4),
            "max_ms": round(float(np.max(xs)), 4), "reps": len(xs)}


def launch_list(L, fn, reps=3):
    L.cb_profile_enable(1)
    L.cb_profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        if L.cb_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value:
            out[name] = {"us_per_call": round(ms.value * 1e3 / reps, 2), "launches": int(n.value // reps)}
    L.cb_profile_enable(0)
    return out


def lww_shape(mods, name, nt, per, pool_n, shuffled, args, dev):
    lsmt_amd, workload, L = mods
    tables, keys, stamps = make_tables(lsmt_amd, workload, nt, per, pool_n, nt, shuffled)
    s = torch.cuda.Stream(dev)
    res = {"shape": name, "timestamps": "shuffled per key" if shuffled else "in table order", "tables": nt,
           "lines_in": int(len(keys))}
    # answers first
    plain = lsmt_amd.compact(tables, m=1024)[0]
    lww = lsmt_amd.compact_lww(tables, m=1024)[0]
    res["lines_out"] = lww.nlines
    if not shuffled:
        res["files_byte_equal"] = bool(plain.data() == lww.data())
        assert res["files_byte_equal"], "timestamps in table order: the two files differ"
    else:
        # per key the greatest timestamp: sort by (key, ts) and take each key's last
        k2 = np.ascontiguousarray(keys).view([("a", ">u8"), ("b", ">u8")]).reshape(-1)
        order = np.lexsort((stamps, k2["b"], k2["a"]))
        ks, ts = k2[order], stamps[order]
        last = np.ones(len(ks), bool)
        last[:-1] = ks[1:] != ks[:-1]
        r = lsmt_amd.scan([lww])
        res["winners_equal_host_maximum"] = bool(r.count == int(last.sum()) and np.array_equal(r.ts(), ts[last]))
        res["lines_that_differ_from_newest_wins"] = int((lsmt_amd.scan([plain]).ts() != r.ts()).sum())
        assert res["winners_equal_host_maximum"] and lww.nlines == plain.nlines
    fns = {"compact": lambda: lsmt_amd.compact(tables, m=1024, stream=s.cuda_stream),
           "compact_lww": lambda: lsmt_amd.compact_lww(tables, m=1024, stream=s.cuda_stream)}
    ms = rounds_ms(fns, s, args.reps, args.warmup)
    res["compact"], res["compact_lww"] = stats(ms["compact"]), stats(ms["compact_lww"])
    ratio = np.array(ms["compact_lww"]) / np.array(ms["compact"])
    res["ratio_lww_over_compact"] = {"median": round(float(np.median(ratio)), 3), "min": round(float(ratio.min()), 3),
                                     "max": round(float(ratio.max()), 3)}
    res["launches_compact"] = launch_list(L, fns["compact"])
    res["launches_compact_lww"] = launch_list(L, fns["compact_lww"])
    return res


def plain_shape(mods, name, nt, per, pool_n, args, dev, tree):
    lsmt_amd, workload, L = mods
    tables, _, _ = make_tables(lsmt_amd, workload, nt, per, pool_n, nt, False)
    s = torch.cuda.Stream(dev)
    prefixes = [b"%x" % i for i in range(16)]
    fns = {"compact": lambda: lsmt_amd.compact(tables, m=1024, stream=s.cuda_stream),
           "scan_many": lambda: lsmt_amd.scan_many(tables[:16], prefixes=prefixes, stream=s.cuda_stream)}
    ms = rounds_ms(fns, s, args.reps, args.warmup)
    return {"plain_only": True, "tree": tree, "shape": name, "compact": stats(ms["compact"]),
            "scan_many_16_tables": stats(ms["scan_many"]), "launches_compact": launch_list(L, fns["compact"]),
            "launches_scan_many": launch_list(L, fns["scan_many"])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--plain-only", action="store_true")
    p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import lsmt_amd
    from lsmt_amd import workload
    from lsmt_amd._lib import load
    mods = (lsmt_amd, workload, load())
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    shapes = [("300 x 1024 lines, 16-byte keys", 300, 1024, 120_000), ("4 x 512K lines, 16-byte keys", 4, 1 << 19, 1_500_000)]
    rows = []
    for name, nt, per, pool_n in shapes:
        if args.plain_only:
            rows.append(plain_shape(mods, name, nt, per, pool_n, args, dev, os.path.abspath(args.tree)))
        else:
            rows += [lww_shape(mods, name, nt, per, pool_n, shuffled, args, dev) for shuffled in (False, True)]
    for r in rows:
        line = json.dumps(r)
        print(line)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
