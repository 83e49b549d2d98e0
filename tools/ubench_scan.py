"""cb_tables_scan on the device, timed with HIP events, against the only other
route to the same answer: cb_tables_compact of all the tables. Two shapes
(ubench_compact.py's: 300 tables of 1024 lines; 4 tables of 512K lines), each
after a warm-up, four legs per shape taken in one process in alternating
order (a round runs them forwards, the next one backwards):

  * compact      cb_tables_compact of the tables (m = 1024 filter);
  * scan_full    the full-range scan: the same gather, sort and select, fewer
                 bytes written, no line index, directory or filter;
  * scan_1pct    a range of about 1 % of the key space (keys are 16 hex
                 characters: ["400", "429"));
  * scan_prefix  one two-character prefix (1/256 of the key space), the shape
                 of a one-namespace scan_ns.

Per leg: min / median / max per call; the compaction leg's spread is the
margin for "no slower than"; ratios of the medians; the per-kernel split
(cb_profile_read) of the scan legs in a pass of their own. The full scan's
count and key bytes are checked against the compacted table's lines.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmt_amd  # noqa: E402
from lsmt_amd._lib import load as _L  # noqa: E402
from ubench_compact import make_tables, stats  # noqa: E402

KERNELS = ["k_scan_bounds", "k_scan_sources", "k_compact_klen", "k_scan_reduce", "k_tile_scan", "k_scan_apply",
           "k_compact_gather", "k_entry_sort", "k_bin_count", "k_bin_offsets", "k_bin_scatter", "k_bin_sort",
           "k_compact_select", "k_scan_emit", "k_b64_decode", "k_compact_format", "k_insert_lds", "k_insert_direct",
           "k_build_part", "k_build_tile", "k_pfx_masks", "k_table_dir"]
LO_1PCT, HI_1PCT = b"400", b"429"  # 0x29 / 0x1000 = 1.0 % of 16-hex-character keys
PREFIX = b"7f"


def alternating(legs, stream, reps, warm):
    """{name: [ms per call]}: every round times each leg once (an event pair
    around the call, which waits for its own stream inside), odd rounds in
    reverse order."""
    out = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        for i in range(warm + reps):
            for name, fn in (legs if i % 2 == 0 else legs[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                keep = fn()
                e1.record(stream)
                e1.synchronize()
                del keep
                if i >= warm:
                    out[name].append(e0.elapsed_time(e1))
    return out


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
            out[name] = {"us_per_call": round(ms.value * 1e3 / reps, 2), "launches": int(n.value // reps)}
    L.cb_profile_enable(0)
    return out


def shape(name, nt, per, pool_n, args, dev):
    pool, tables, blooms, zones = make_tables(nt, per, pool_n, seed=nt)
    newest_first = tables[::-1]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    res = {"shape": name, "tables": nt, "lines_in": sum(t.nlines for t in tables)}
    legs = [("compact", lambda: lsmt_amd.compact(newest_first, m=1024, stream=s)),
            ("scan_full", lambda: lsmt_amd.scan(newest_first, stream=s)),
            ("scan_1pct", lambda: lsmt_amd.scan(newest_first, lo=LO_1PCT, hi=HI_1PCT, stream=s)),
            ("scan_prefix", lambda: lsmt_amd.scan(newest_first, prefix=PREFIX, stream=s))]
    # what each leg returns, and the full scan against the compacted table
    merged, _, _ = lsmt_amd.compact(newest_first, m=1024)
    full = lsmt_amd.scan(newest_first)
    res["lines_out"] = merged.nlines
    _, kl, ll = merged.lines()
    res["full_scan_matches_compaction"] = bool(
        full.count == merged.nlines and full.key_bytes == int(kl.sum()) and
        full.keys() == [ln.split(b"\t", 1)[0] for ln in merged.data().split(b"\n") if ln])
    for leg, fn in legs[1:]:
        r = fn()
        res[leg + "_entries"] = {"count": r.count, "key_bytes": r.key_bytes, "val_bytes": r.val_bytes}
    ms = alternating(legs, stream, args.reps, args.warmup)
    for leg, xs in ms.items():
        res[leg] = stats(xs)
    c = res["compact"]
    res["compact_spread_over_median"] = round((c["max_ms"] - c["min_ms"]) / c["median_ms"], 3)
    for leg in ("scan_full", "scan_1pct", "scan_prefix"):
        res["ratio_" + leg + "_over_compact"] = round(res[leg]["median_ms"] / c["median_ms"], 3)
    res["kernels"] = {leg: kernel_split(fn, 5) for leg, fn in legs}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    rows = [shape("300 x 1024 lines, 16-byte keys", 300, 1024, 120_000, args, dev),
            shape("4 x 512K lines, 16-byte keys", 4, 1 << 19, 1_500_000, args, dev)]
    for r in rows:
        line = json.dumps(r)
        print(line)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
