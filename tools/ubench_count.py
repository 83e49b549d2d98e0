"""The live-row entries on the device, timed with HIP events against the routes
that existed before them. ubench_scan_many.py's two shapes (300 tables of
1024 lines; 4 tables of 512K lines; keys are 16 hex characters) and its
method: one process, after a warm-up every round runs all legs once, odd
rounds in reverse order, an event pair around each leg on one stream.

The tables are ubench_compact.py's with a share of the values replaced by
tombstones (the 8-byte timestamp alone, exec_delete's value,
src/query.rs:240-261): one set at 10 %, one at 0 %.

Legs, for R in {1, 16, 64} two-character prefixes over the 10 % set:

  * count_R     cb_tables_count of the R prefixes (entries and live), given as
                ranges built before the timed rounds (the entry takes ranges;
                64 prefix_end calls from Python would be timed as device idle);
  * scanpfx_R   cb_tables_scan_prefixes of the same prefixes, the counts taken
                from its offsets: the yardstick, the only route to the number
                without cb_tables_count (and it still counts tombstones);

and for both sets (T = 0 and 10):

  * compact_live_T  cb_tables_compact_live of the tables (m = 1024 filter);
  * compact_T       cb_tables_compact of the same tables: the yardstick.

Before anything is timed the answers are compared: count's entries with the
batched scan's offsets, its live with cb_tables_scan_live's offsets, and at
0 % the two compactions' files byte for byte. Per leg: min / median / max and
(max - min) / median; per pair the ratio of the medians next to the
yardstick's spread. The per-kernel split (cb_profile_read) of the count, the
batched scan and the two compactions in a pass of their own, with the launch
counts.

Prints one JSON line per shape (also appended to --out). Diagnostic only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmt_amd  # noqa: E402
from lsmt_amd import workload  # noqa: E402
from ubench_compact import offsets16, stats  # noqa: E402
from ubench_scan import KERNELS, alternating, kernel_split  # noqa: E402
from ubench_scan_many import prefixes_for  # noqa: E402  (adds k_scan_range_off to KERNELS)

RS = [1, 16, 64]
KERNELS.insert(KERNELS.index("k_compact_select") + 1, "k_compact_select_live")  # (kernel_split reads this list)
KERNELS.insert(KERNELS.index("k_scan_emit"), "k_scan_count")


def make_tables(nt, per, pool_n, seed, dead_share):
    """ubench_compact.make_tables with dead_share of every table's values cut
    to their 8-byte timestamp. Oldest first."""
    rng = np.random.default_rng(seed)
    pool = workload.key_range(4242, pool_n)
    tables = []
    for t in range(nt):
        idx = np.unique(rng.choice(len(pool), per, replace=False))
        ks = np.ascontiguousarray(pool[idx])
        vs = np.ascontiguousarray(workload.table_value(ks, t))
        dead = rng.random(len(idx)) < dead_share
        keep = np.ones(vs.shape, bool)
        keep[:, 8:] = ~dead[:, None]
        voff = np.zeros(len(idx) + 1, np.uint64)
        np.cumsum(np.where(dead, 8, 16), out=voff[1:])
        kb = lsmt_amd.KeyBatch(n=len(idx), data=ks.reshape(-1), offsets=offsets16(len(idx)))
        vb = lsmt_amd.KeyBatch(n=len(idx), data=np.ascontiguousarray(vs[keep]), offsets=voff)
        tables.append(lsmt_amd.sstable_create((kb, vb), m=1024)[0])
    return tables


def spread(st):
    return round((st["max_ms"] - st["min_ms"]) / st["median_ms"], 3)


def shape(name, nt, per, pool_n, args, dev):
    sets = {0: make_tables(nt, per, pool_n, nt, 0.0)[::-1], 10: make_tables(nt, per, pool_n, nt, 0.10)[::-1]}
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    res = {"shape": name, "tables": nt, "lines_in": sum(t.nlines for t in sets[10])}
    legs = []
    tabs = sets[10]
    for r in RS:
        ps = prefixes_for(r)
        # the C entry takes ranges: built once, outside the timed window, as a store builds its bounds
        rs = [(p, lsmt_amd.prefix_end(p)) for p in ps]
        entries, live = lsmt_amd.count(tabs, prefixes=ps)
        by_ranges = lsmt_amd.count(tabs, ranges=rs)
        assert entries.tolist() == by_ranges[0].tolist() and live.tolist() == by_ranges[1].tolist()
        many = lsmt_amd.scan_many(tabs, prefixes=ps)
        lv = lsmt_amd.scan_live(tabs, prefixes=ps)
        equal = bool(entries.tolist() == np.diff(many.range_off()).tolist() and
                     live.tolist() == np.diff(lv.range_off()).tolist())
        res[f"R{r}"] = {"prefixes": [ps[0].decode(), ps[-1].decode()], "entries": int(entries.sum()),
                        "live": int(live.sum()), "cuts": r * nt, "answers_equal": equal}
        assert equal, f"{name}: R={r}: the counts differ from the scans' offsets"
        legs.append((f"count_{r}", lambda rs=rs: lsmt_amd.count(tabs, ranges=rs, stream=s)))
        legs.append((f"scanpfx_{r}", lambda ps=ps: np.diff(lsmt_amd.scan_many(tabs, prefixes=ps, stream=s).range_off())))
    for share, ts in sets.items():
        plain, _, _ = lsmt_amd.compact(ts, m=1024)
        lively, _, _ = lsmt_amd.compact_live(ts, m=1024)
        res[f"compaction_{share}"] = {"lines_out": plain.nlines, "lines_out_live": lively.nlines}
        if share == 0:
            assert plain.data() == lively.data(), f"{name}: without tombstones the two compactions differ"
        else:
            assert lively.nlines < plain.nlines
        legs.append((f"compact_live_{share}", lambda ts=ts: lsmt_amd.compact_live(ts, m=1024, stream=s)))
        legs.append((f"compact_{share}", lambda ts=ts: lsmt_amd.compact(ts, m=1024, stream=s)))
    ms = alternating(legs, stream, args.reps, args.warmup)
    for leg, xs in ms.items():
        st = stats(xs)
        st["spread_over_median"] = spread(st)
        res[leg] = st
    for r in RS:
        res[f"R{r}"]["count_over_scanpfx"] = round(res[f"count_{r}"]["median_ms"] / res[f"scanpfx_{r}"]["median_ms"], 3)
        res[f"R{r}"]["yardstick_spread"] = res[f"scanpfx_{r}"]["spread_over_median"]
    for share in sets:
        c = res[f"compaction_{share}"]
        c["live_over_plain"] = round(res[f"compact_live_{share}"]["median_ms"] / res[f"compact_{share}"]["median_ms"], 3)
        c["yardstick_spread"] = res[f"compact_{share}"]["spread_over_median"]
    fns = dict(legs)
    res["kernels"] = {leg: kernel_split(fns[leg], 5) for leg in
                      ("count_1", "scanpfx_1", "count_64", "scanpfx_64", "compact_live_0", "compact_0",
                       "compact_live_10", "compact_10")}
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
