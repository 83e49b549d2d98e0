"""cb_tables_compact on the device, timed with HIP events: two shapes (the
wide fan-out's 300 tables of 1024 lines; 4 tables of 512K lines), each after
a warm-up, on two lanes (streams) reported apart. Per shape:

  * time per compaction, against its yardstick in the same run:
    cb_sstable_create of the same number of unsorted entries;
  * the per-kernel split (cb_profile_read), in a pass of its own;
  * for the 300-table shape, the reason for the feature: get_many of 1M keys
    over the 300 tables through their wide FilterSet against the same keys
    over the one compacted table through its filter, the answers compared.

Prints one JSON line per shape (also appended to --out). Diagnostic only.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsmt_amd  # noqa: E402
from lsmt_amd import workload  # noqa: E402
from lsmt_amd._lib import load as _L  # noqa: E402

KERNELS = ["k_compact_klen", "k_scan_reduce", "k_tile_scan", "k_scan_apply", "k_compact_gather", "k_entry_sort",
           "k_bin_count", "k_bin_offsets", "k_bin_scatter", "k_bin_sort", "k_compact_select", "k_compact_format",
           "k_insert_lds", "k_insert_direct", "k_build_part", "k_build_tile", "k_line_count", "k_line_emit",
           "k_line_finish", "k_line_keys", "k_pfx_masks", "k_table_dir"]


def offsets16(n):
    return np.arange(0, 16 * (n + 1), 16, dtype=np.uint64)


def make_tables(nt, per, pool_n, seed):
    """nt tables of ~per lines whose keys come from one pool (later tables
    rewrite keys), as bench.py's wide fan-out builds them. Oldest first."""
    rng = np.random.default_rng(seed)
    pool = workload.key_range(4242, pool_n)
    tables, blooms, zones = [], [], []
    for t in range(nt):
        idx = np.unique(rng.choice(len(pool), per, replace=False))
        ks = np.ascontiguousarray(pool[idx])
        vs = np.ascontiguousarray(workload.table_value(ks, t))
        kb = lsmt_amd.KeyBatch(n=len(idx), data=ks.reshape(-1), offsets=offsets16(len(idx)))
        vb = lsmt_amd.KeyBatch(n=len(idx), data=vs.reshape(-1), offsets=offsets16(len(idx)))
        tb, bloom, zone = lsmt_amd.sstable_create((kb, vb), m=1024)
        tables.append(tb)
        blooms.append(bloom)
        zones.append(zone)
    return pool, tables, blooms, zones


def event_ms(fn, stream, reps, warm):
    """Device time of fn() per call on `stream`: an event pair around each call."""
    out = []
    with torch.cuda.stream(stream):
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            keep = fn()
            e1.record(stream)
            e1.synchronize()
            del keep
            if i >= warm:
                out.append(e0.elapsed_time(e1))
    return out


def stats(xs):
    return {"min_ms": round(float(np.min(xs)), 4), "median_ms": round(float(np.median(xs)), 4),
            "max_ms": round(float(np.max(xs)), 4), "reps": len(xs)}


def kernel_split(fn, reps):
    L = _L()
    L.cb_profile_enable(1)
    L.cb_profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        if L.cb_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value:
            out[name] = {"us_per_compaction": round(ms.value * 1e3 / reps, 2), "launches": int(n.value // reps)}
    L.cb_profile_enable(0)
    return out


def shape(name, nt, per, pool_n, args, dev, reads):
    pool, tables, blooms, zones = make_tables(nt, per, pool_n, seed=nt)
    newest_first = tables[::-1]
    lines = sum(t.nlines for t in tables)
    lanes = [torch.cuda.default_stream(dev), torch.cuda.Stream(dev)]
    res = {"shape": name, "tables": nt, "lines_in": lines}

    def compact(stream):
        return lambda: lsmt_amd.compact(newest_first, m=1024, stream=stream.cuda_stream)

    merged, mbloom, mzone = lsmt_amd.compact(newest_first, m=1024)
    res["lines_out"] = merged.nlines
    res["bytes_out"] = merged.nbytes
    res["compact"] = [dict(lane=i, **stats(event_ms(compact(s), s, args.reps, args.warmup))) for i, s in enumerate(lanes)]
    # the yardstick: SsTable::create of as many unsorted entries, device-resident
    rng = np.random.default_rng(1)
    uk = np.ascontiguousarray(workload.key_range(77, lines)[rng.permutation(lines)])
    uv = np.ascontiguousarray(workload.table_value(uk, 1))
    kd = torch.from_numpy(uk.reshape(-1)).to(dev)
    vd = torch.from_numpy(uv.reshape(-1)).to(dev)
    od = torch.from_numpy(offsets16(lines).astype(np.int64)).to(dev)
    kb = lsmt_amd.KeyBatch(n=lines, data=kd, offsets=od)
    vb = lsmt_amd.KeyBatch(n=lines, data=vd, offsets=od)

    def create(stream):
        def run():
            t, b, _ = lsmt_amd.sstable_create((kb, vb), m=1024, stream=stream.cuda_stream, wait=False)
            return t, b
        return run

    res["create_unsorted"] = [dict(lane=i, **stats(event_ms(create(s), s, args.reps, args.warmup)))
                              for i, s in enumerate(lanes)]
    res["ratio_compact_over_create"] = round(res["compact"][0]["median_ms"] / res["create_unsorted"][0]["median_ms"], 2)
    res["kernels"] = kernel_split(compact(lanes[0]), 5)
    if reads:
        n = 1 << 20
        present = pool[rng.integers(0, len(pool), 3 * n // 4)]
        look = np.concatenate([present, workload.key_range(4343, n - len(present))])[rng.permutation(n)]
        keys = lsmt_amd.DeviceKeys(torch.from_numpy(look).to(dev))
        wide = lsmt_amd.FilterSet(1024, width=(nt + 63) // 64 * 64)
        for t in range(nt):
            wide.assign(t, blooms[t])
            wide.set_zone(t, zones[t])
        one = lsmt_amd.FilterSet.from_filters([mbloom])
        one.set_zone(0, mzone)
        slots = np.arange(nt, dtype=np.uint32)[::-1].copy()
        outs = [(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
                 torch.empty(n * 16, dtype=torch.uint8, device=dev)) for _ in range(2)]
        s0 = lanes[0]
        merged_list = [merged]

        def read_wide():
            lsmt_amd.get_many(newest_first, keys, filterset=wide, hit_rows=slots, out=outs[0], stream=s0.cuda_stream,
                              wait=False)

        def read_one():
            lsmt_amd.get_many(merged_list, keys, filterset=one, out=outs[1], stream=s0.cuda_stream, wait=False)

        w = stats(event_ms(read_wide, s0, args.reps, args.warmup))
        o = stats(event_ms(read_one, s0, args.reps, args.warmup))
        torch.cuda.synchronize()
        tot = int(outs[0][1][n].item())
        equal = (torch.equal(outs[0][0] >= 0, outs[1][0] >= 0) and torch.equal(outs[0][1], outs[1][1]) and
                 torch.equal(outs[0][2][:tot], outs[1][2][:tot]))
        res["get_many_1M"] = {"wide_300_tables": dict(w, gets_per_s=round(n / (w["median_ms"] * 1e-3), 1)),
                              "compacted_table": dict(o, gets_per_s=round(n / (o["median_ms"] * 1e-3), 1)),
                              "found": int((outs[0][0] >= 0).sum().item()), "answers_equal": bool(equal)}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    rows = [shape("300 x 1024 lines, 16-byte keys", 300, 1024, 120_000, args, dev, reads=True),
            shape("4 x 512K lines, 16-byte keys", 4, 1 << 19, 1_500_000, args, dev, reads=False)]
    for r in rows:
        line = json.dumps(r)
        print(line)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
