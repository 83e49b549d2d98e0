"""Database::get over the store a compaction leaves, timed with HIP events:
one table of ~110K lines behind a filter of m = 2^20 (300 flushes of 1024
lines merged by cb_tables_compact, as tools/ubench_compact.py builds them)
and, in front of it, 8 fresh tables of 1024 lines behind m = 1024 filters,
listed newest first; 1M lookups of 16-byte keys, everything on the device.

  (a) cb_tiers_get_many_fixed: one launch over both FilterSets;
  (b) the path without it: one cb_set_probe_gated_fixed per set into a shared
      row buffer, then cb_get_many_fixed with hits and hit_rows.

Both are checked to return identical `which`, offsets and values before
anything is timed. The two are timed alternately, warm, one event pair per
--inner back-to-back calls (per-call time = elapsed / inner). Prints one JSON
line (also appended to --out). Diagnostic only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsmt_amd  # noqa: E402
from lsmt_amd import workload  # noqa: E402


def offsets16(n):
    return np.arange(0, 16 * (n + 1), 16, dtype=np.uint64)


def flush(ks, t, m):
    ks = np.ascontiguousarray(ks)
    vs = np.ascontiguousarray(workload.table_value(ks, t))
    kb = lsmt_amd.KeyBatch(n=len(ks), data=ks.reshape(-1), offsets=offsets16(len(ks)))
    vb = lsmt_amd.KeyBatch(n=len(ks), data=vs.reshape(-1), offsets=offsets16(len(ks)))
    return lsmt_amd.sstable_create((kb, vb), m=m)


def stats(xs):
    return {"min_ms": round(float(np.min(xs)), 4), "median_ms": round(float(np.median(xs)), 4),
            "max_ms": round(float(np.max(xs)), 4), "samples": len(xs)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--inner", type=int, default=10, help="calls per event pair")
    p.add_argument("--keys", type=int, default=1 << 20)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(300)
    pool = workload.key_range(4242, 120_000)
    # the compacted table: 300 flushes of 1024 lines out of one pool, merged behind an m = 2^20 filter
    old = [flush(pool[np.unique(rng.choice(len(pool), 1024, replace=False))], t, 1024)[0] for t in range(300)]
    merged, mbloom, mzone = lsmt_amd.compact(old[::-1], m=1 << 20)
    for t in old:
        t.close()
    # 8 fresh flushes in front of it: half rewrites of pool keys, half new keys
    fresh = []
    for i in range(8):
        ks = np.concatenate([pool[rng.choice(len(pool), 512, replace=False)], workload.key_range(5000 + i, 512)])
        fresh.append(flush(np.unique(ks, axis=0), 1000 + i, 1024))
    small = lsmt_amd.FilterSet(1024, width=32)
    for i, (_, bloom, zone) in enumerate(fresh):
        small.assign(i, bloom)
        small.set_zone(i, zone)
    large = lsmt_amd.FilterSet(1 << 20, width=32)
    large.assign(0, mbloom)
    large.set_zone(0, mzone)
    tables = [fresh[i][0] for i in range(7, -1, -1)] + [merged]  # newest first
    tiers = np.array([0] * 8 + [1], np.uint32)
    slots = np.array(list(range(7, -1, -1)) + [0], np.uint32)
    rows = np.array(list(range(7, -1, -1)) + [8], np.uint32)  # (b)'s shared row buffer: the small set's 8 rows, then the large set's

    n = args.keys
    present = pool[rng.integers(0, len(pool), 3 * n // 4)]
    look = np.concatenate([present, workload.key_range(4343, n - len(present))])[rng.permutation(n)]
    keys = lsmt_amd.DeviceKeys(torch.from_numpy(np.ascontiguousarray(look)).to(dev))
    words = (n + 63) // 64
    outs = [(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
             torch.empty(n * 16, dtype=torch.uint8, device=dev)) for _ in range(2)]
    rowbuf = torch.zeros((9, words), dtype=torch.int64, device=dev)
    stream = torch.cuda.default_stream(dev)
    sh = stream.cuda_stream
    sets = [small, large]

    def tiered():
        lsmt_amd.get_many_tiers(tables, sets, tiers, slots, keys, out=outs[0], stream=sh, wait=False)

    def two_step():
        small.probe(keys, out=rowbuf[0:8], stream=sh, gated=True)
        large.probe(keys, out=rowbuf[8:9], stream=sh, gated=True)
        lsmt_amd.get_many(tables, keys, hits=rowbuf, hit_rows=rows, out=outs[1], stream=sh, wait=False)

    tiered()
    two_step()
    torch.cuda.synchronize()
    tot = int(outs[0][1][n].item())
    assert torch.equal(outs[0][0], outs[1][0]), "which differs between the tiered call and the two-step path"
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2][:tot], outs[1][2][:tot]), "values differ"
    found = int((outs[0][0] >= 0).sum().item())
    per_table = np.bincount(outs[0][0][outs[0][0] >= 0].cpu().numpy(), minlength=9).tolist()

    times = {"tiered": [], "two_step": []}
    with torch.cuda.stream(stream):
        for i in range(args.warmup + args.reps):
            for name, fn in (("tiered", tiered), ("two_step", two_step)):  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.inner):  # back to back: the queue stays full, host enqueue time hides
                    fn()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) / args.inner)
    a, b = stats(times["tiered"]), stats(times["two_step"])
    res = {"shape": "1 table of %d lines (m = 2^20) behind 8 x ~1024 lines (m = 1024), %d lookups of 16-byte keys"
                    % (merged.nlines, n),
           "found": found, "found_per_table": per_table, "answers_equal": True,
           "tiers_get_many": dict(a, gets_per_s=round(n / (a["median_ms"] * 1e-3), 1)),
           "probe_per_set_then_get_many": dict(b, gets_per_s=round(n / (b["median_ms"] * 1e-3), 1)),
           "ratio_two_step_over_tiered": round(b["median_ms"] / a["median_ms"], 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
