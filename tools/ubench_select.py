"""cb_scan_select on the device, timed against what a caller had before it.
ubench_where.py's two shapes (300 tables of 1024 lines; 4 tables of 512K lines;
keys are 16 hex characters), its rows (an 8-byte timestamp, then
{"a":"NN","b":"N","c":"NNNN"}) and its method: one process, after a warm-up
every round runs all legs once, odd rounds in reverse order, an event pair
around each leg (every leg waits for its own work, so the pair spans the call).

For R in {1, 16} two-character prefixes (skip = 2, no key column) one live scan
result is made outside the timed window; the legs run over it:

  * select_R_{1,3}_{json,meta}  ScanResult.select of one column (a) or all
                  three, as the client's JSON array or the coordinator's lines;
                  the response stays in device memory, as the values did;
  * match_R       ScanResult.match(a = "07") over the same result: the floor,
                  the same parse with nothing written (flags to the host);
  * copy_R        the result's values and keys copied to the host
                  (cb_scan_values + cb_scan_keys): what a caller pays today
                  before it parses, projects or encodes anything.

Before anything is timed the answers are compared with the response built on
the host from the scan's keys and values (the rows are fixed-width and hold
nothing that needs an escape). Per leg: min / median / max and (max - min) /
median; per select leg its ratio to both yardsticks next to their spreads. The
per-kernel split (cb_profile_read) of every select leg in a pass of its own,
with the launch counts.

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
from ubench_compact import stats  # noqa: E402
from ubench_scan import KERNELS, alternating, kernel_split  # noqa: E402
from ubench_scan_many import prefixes_for  # noqa: E402
from ubench_where import TEMPLATE, make_tables, spread  # noqa: E402

RS = [1, 16]
for k in ("k_scan_match", "k_select_size", "k_select_write"):
    if k not in KERNELS:
        KERNELS.append(k)  # (kernel_split reads this list)
COLS = {1: ["a"], 3: ["a", "b", "c"]}


def host_response(r, ncols, meta):
    """The response of a live scan's rows, built on the host."""
    ko, kb, vo, vb = r.raw()
    w = len(TEMPLATE)
    assert np.array_equal(vo, np.arange(0, w * (r.count + 1), w, dtype=np.uint64))
    rows, keys = vb.reshape(-1, w), kb.tobytes()
    ko = ko.tolist()
    objs = [bytes(x) for x in (rows[:, 8:] if ncols == 3 else np.concatenate(
        [rows[:, 8:8 + len(b'{"a":"00"')], np.full((r.count, 1), ord("}"), np.uint8)], axis=1))]
    if not meta:
        return b"[" + b",".join(objs) + b"]"
    ts = [int.from_bytes(bytes(x), "big") for x in rows[:, :8]]
    return b"\n".join(keys[ko[i] + 2:ko[i + 1]] + b"\t%d\t" % ts[i] + objs[i] for i in range(r.count))


def shape(name, nt, per, pool_n, args, dev):
    tabs = make_tables(nt, per, pool_n, nt)[::-1]
    stream = torch.cuda.Stream(dev)
    res = {"shape": name, "tables": nt, "lines_in": sum(t.nlines for t in tabs), "row_bytes": len(TEMPLATE)}
    legs, keep = [], []
    for r in RS:
        ps = prefixes_for(r)
        lv = lsmt_amd.scan_live(tabs, ranges=[(p, lsmt_amd.prefix_end(p)) for p in ps])
        keep.append(lv)
        res[f"R{r}"] = {"prefixes": [ps[0].decode(), ps[-1].decode()], "rows": lv.count, "val_bytes": lv.val_bytes}
        for nc, cols in COLS.items():
            for meta in (False, True):
                got = lv.select(cols, skip=2, meta=meta)
                want = host_response(lv, nc, meta)
                assert got.text() == want, f"{name}: R={r}, {cols}, meta={meta}: select differs from the host's response"
                assert got.with_text == lv.count and set(got.flags().tolist()) <= {1 if nc == 3 else 17}
                form = "meta" if meta else "json"
                res[f"R{r}"][f"bytes_{nc}_{form}"] = got.bytes
                legs.append((f"select_{r}_{nc}_{form}", lambda lv=lv, cols=cols, meta=meta: lv.select(cols, skip=2, meta=meta)))
        legs.append((f"match_{r}", lambda lv=lv: lv.match({"a": "07"}, skip=2)))
        ko, kb = np.zeros(lv.count + 1, np.uint64), np.zeros(max(lv.key_bytes, 1), np.uint8)
        vo, vb = np.zeros(lv.count + 1, np.uint64), np.zeros(max(lv.val_bytes, 1), np.uint8)

        def copy(lv=lv, ko=ko, kb=kb, vo=vo, vb=vb):
            lv.copy_values(vo, vb)
            lv.copy_keys(ko, kb)
        legs.append((f"copy_{r}", copy))
    ms = alternating(legs, stream, args.reps, args.warmup)
    for leg, xs in ms.items():
        st = stats(xs)
        st["spread_over_median"] = spread(st)
        res[leg] = st
    for r in RS:
        for leg in [n for n, _ in legs if n.startswith(f"select_{r}_")]:
            m = res[leg]["median_ms"]
            res[f"R{r}"][leg + "_over_match"] = round(m / res[f"match_{r}"]["median_ms"], 3)
            res[f"R{r}"][leg + "_over_copy"] = round(m / res[f"copy_{r}"]["median_ms"], 3)
        res[f"R{r}"]["match_spread"] = res[f"match_{r}"]["spread_over_median"]
        res[f"R{r}"]["copy_spread"] = res[f"copy_{r}"]["spread_over_median"]
    fns = dict(legs)
    res["kernels"] = {leg: kernel_split(fns[leg], 5) for leg in fns if leg.startswith(("select_", "match_"))}
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
