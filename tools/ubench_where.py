"""cb_tables_count_where on the device, timed with HIP events against what a
caller had before it. ubench_count.py's two shapes (300 tables of 1024 lines;
4 tables of 512K lines; keys are 16 hex characters) and its method: one
process, after a warm-up every round runs all legs once, odd rounds in reverse
order, an event pair around each leg on one stream.

The rows are the reference's: an 8-byte timestamp, then a JSON object of three
short columns, {"a":"NN","b":"N","c":"NNNN"} (a: 00..99, b: 0 or 1). Legs, for
R in {1, 16} two-character prefixes (skip = 2, no key column):

  * where_R_1    cb_tables_count_where with a = "07": about 1 % of the rows;
  * where_R_50   the same with b = "1": about 50 %;
  * count_R      cb_tables_count of the same ranges: the floor, the same cuts,
                 merge and select with no row read;
  * scanlive_R   cb_tables_scan_live of the same ranges and the copy of its
                 value offsets and bytes to the host: a lower bound on what a
                 caller pays today, before it parses anything.

Before anything is timed the answers are compared: live with cb_tables_count's,
matched with the rows counted on the host from the scan's values (the rows are
fixed-width, so numpy compares the columns' bytes) and with ScanResult.match.
Per leg: min / median / max and (max - min) / median; per where leg its ratio
to both yardsticks next to their spreads. The per-kernel split
(cb_profile_read) of one count and one count_where in a pass of their own, with
the launch counts: k_scan_count_where's own time and its share of the call.

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
from ubench_scan_many import prefixes_for  # noqa: E402

RS = [1, 16]
KERNELS.insert(KERNELS.index("k_scan_emit"), "k_scan_count")  # (kernel_split reads this list)
KERNELS.insert(KERNELS.index("k_scan_emit"), "k_scan_count_where")
TEMPLATE = b'\0\0\0\0\0\0\0\0{"a":"00","b":"0","c":"0000"}'
A_AT, B_AT, C_AT = TEMPLATE.index(b'"a":"') + 5, TEMPLATE.index(b'"b":"') + 5, TEMPLATE.index(b'"c":"') + 5
WHERES = {1: {"a": "07"}, 50: {"b": "1"}}


def make_tables(nt, per, pool_n, seed):
    """nt tables of ~per lines whose keys come from one pool, every value a
    timestamp and the three-column row. Oldest first."""
    rng = np.random.default_rng(seed)
    pool = workload.key_range(4242, pool_n)
    w = len(TEMPLATE)
    tables = []
    for t in range(nt):
        idx = np.unique(rng.choice(len(pool), per, replace=False))
        n = len(idx)
        vs = np.tile(np.frombuffer(TEMPLATE, np.uint8), (n, 1))
        vs[:, 7] = t % 250 + 1
        a, c = rng.integers(0, 100, n), rng.integers(0, 10000, n)
        vs[:, A_AT], vs[:, A_AT + 1] = 48 + a // 10, 48 + a % 10
        vs[:, B_AT] = 48 + rng.integers(0, 2, n)
        for j in range(4):
            vs[:, C_AT + j] = 48 + c // 10 ** (3 - j) % 10
        kb = lsmt_amd.KeyBatch(n=n, data=np.ascontiguousarray(pool[idx]).reshape(-1), offsets=offsets16(n))
        vb = lsmt_amd.KeyBatch(n=n, data=np.ascontiguousarray(vs).reshape(-1),
                               offsets=np.arange(0, w * (n + 1), w, dtype=np.uint64))
        tables.append(lsmt_amd.sstable_create((kb, vb), m=1024)[0])
    return tables


def spread(st):
    return round((st["max_ms"] - st["min_ms"]) / st["median_ms"], 3)


def host_matched(r, sel):
    """Per range, the rows of a live scan that hold WHERES[sel], counted from
    the values' bytes on the host."""
    _, _, vo, vb = r.raw()
    rows = vb.reshape(-1, len(TEMPLATE))
    assert np.array_equal(vo, np.arange(0, len(TEMPLATE) * (r.count + 1), len(TEMPLATE), dtype=np.uint64))
    hit = (rows[:, A_AT] == 48) & (rows[:, A_AT + 1] == 55) if sel == 1 else rows[:, B_AT] == 49
    off = r.range_off().tolist()
    return [int(hit[off[i]:off[i + 1]].sum()) for i in range(len(off) - 1)]


def shape(name, nt, per, pool_n, args, dev):
    tabs = make_tables(nt, per, pool_n, nt)[::-1]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    res = {"shape": name, "tables": nt, "lines_in": sum(t.nlines for t in tabs), "row_bytes": len(TEMPLATE)}
    legs = []
    for r in RS:
        ps = prefixes_for(r)
        rs = [(p, lsmt_amd.prefix_end(p)) for p in ps]  # built once, outside the timed window
        _, live0 = lsmt_amd.count(tabs, ranges=rs)
        lv = lsmt_amd.scan_live(tabs, ranges=rs)
        res[f"R{r}"] = {"prefixes": [ps[0].decode(), ps[-1].decode()], "live": int(live0.sum()), "cuts": r * nt}
        for sel, where in WHERES.items():
            live, matched = lsmt_amd.count_where(tabs, where, ranges=rs, skip=2)
            flags, off = lv.match(where, skip=2), lv.range_off().tolist()
            equal = bool(live.tolist() == live0.tolist() and matched.tolist() == host_matched(lv, sel) and
                         matched.tolist() == [int(flags[off[i]:off[i + 1]].sum()) for i in range(r)])
            assert equal, f"{name}: R={r}, {where}: count_where differs from the host's count"
            res[f"R{r}"][f"matched_{sel}"] = int(matched.sum())
            legs.append((f"where_{r}_{sel}", lambda rs=rs, where=where: lsmt_amd.count_where(tabs, where, ranges=rs, skip=2,
                                                                                            stream=s)))
        legs.append((f"count_{r}", lambda rs=rs: lsmt_amd.count(tabs, ranges=rs, stream=s)))
        vo, vb = np.zeros(lv.count + 1, np.uint64), np.zeros(max(lv.val_bytes, 1), np.uint8)

        def scan_and_copy(rs=rs, vo=vo, vb=vb):
            got = lsmt_amd.scan_live(tabs, ranges=rs, stream=s)
            got.copy_values(vo, vb)
            return got
        legs.append((f"scanlive_{r}", scan_and_copy))
    ms = alternating(legs, stream, args.reps, args.warmup)
    for leg, xs in ms.items():
        st = stats(xs)
        st["spread_over_median"] = spread(st)
        res[leg] = st
    for r in RS:
        for sel in WHERES:
            m = res[f"where_{r}_{sel}"]["median_ms"]
            res[f"R{r}"][f"where_{sel}_over_count"] = round(m / res[f"count_{r}"]["median_ms"], 3)
            res[f"R{r}"][f"where_{sel}_over_scanlive"] = round(m / res[f"scanlive_{r}"]["median_ms"], 3)
        res[f"R{r}"]["count_spread"] = res[f"count_{r}"]["spread_over_median"]
        res[f"R{r}"]["scanlive_spread"] = res[f"scanlive_{r}"]["spread_over_median"]
    fns = dict(legs)
    res["kernels"] = {leg: kernel_split(fns[leg], 5) for leg in
                      ("count_1", "where_1_1", "where_1_50", "count_16", "where_16_1", "where_16_50")}
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
