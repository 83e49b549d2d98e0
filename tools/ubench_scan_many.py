"""cb_tables_scan_prefixes (R prefixes from one merge) on the device, timed with
HIP events, against the only other route to the same answer: R
cb_tables_scan_prefix calls back to back. ubench_scan.py's two shapes (300
tables of 1024 lines; 4 tables of 512K lines; keys are 16 hex characters) and
its method: after a warm-up every round runs all legs once, odd rounds in
reverse order, an event pair around each leg on one stream.

Prefixes are distinct two-character strings (each 1/256 of the key space),
ascending and spread over the key space. Legs, for R in {1, 16, 64}:

  * many_R     one cb_tables_scan_prefixes of the R prefixes;
  * singles_R  the same R prefixes as R cb_tables_scan_prefix calls (the
               yardstick: the code of the single scan).

Before anything is timed the two answers are compared for equality (keys,
values, sources, and the ranges' offsets against the singles' counts). Per
leg: min / median / max and (max - min) / median; per R the ratio of the
medians. For R = 64 the per-kernel split (cb_profile_read) of many_R in a pass
of its own: k_scan_bounds and the one-block k_scan_sources at 64 x the
tables' cuts.

Prints one JSON line per shape (also appended to --out). Diagnostic only.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmt_amd  # noqa: E402
from ubench_compact import make_tables, stats  # noqa: E402
from ubench_scan import KERNELS, alternating, kernel_split  # noqa: E402

RS = [1, 16, 64]
KERNELS.insert(KERNELS.index("k_scan_emit") + 1, "k_scan_range_off")  # (kernel_split reads this list)


def prefixes_for(r):
    """r distinct two-hex-character prefixes, ascending, evenly spread."""
    return [b"%02x" % (i * (256 // r) + (256 // r) // 2) for i in range(r)]


def same_answer(many, singles):
    off = [0]
    for s in singles:
        off.append(off[-1] + s.count)
    return bool(many.range_off().tolist() == off and many.nranges == len(singles) and
                many.keys() == [k for s in singles for k in s.keys()] and
                many.values() == [v for s in singles for v in s.values()] and
                many.which().tolist() == [w for s in singles for w in s.which().tolist()])


def shape(name, nt, per, pool_n, args, dev):
    pool, tables, blooms, zones = make_tables(nt, per, pool_n, seed=nt)
    newest_first = tables[::-1]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    res = {"shape": name, "tables": nt, "lines_in": sum(t.nlines for t in tables)}
    legs = []
    for r in RS:
        ps = prefixes_for(r)
        many = lsmt_amd.scan_many(newest_first, prefixes=ps)
        singles = [lsmt_amd.scan(newest_first, prefix=p) for p in ps]
        res[f"R{r}"] = {"prefixes": [ps[0].decode(), ps[-1].decode()], "entries": many.count,
                        "key_bytes": many.key_bytes, "val_bytes": many.val_bytes,
                        "cuts": r * nt, "answers_equal": same_answer(many, singles)}
        assert res[f"R{r}"]["answers_equal"], f"{name}: R={r}: the batched answer differs from the single scans'"
        legs.append((f"many_{r}", lambda ps=ps: lsmt_amd.scan_many(newest_first, prefixes=ps, stream=s)))
        legs.append((f"singles_{r}", lambda ps=ps: [lsmt_amd.scan(newest_first, prefix=p, stream=s) for p in ps]))
    ms = alternating(legs, stream, args.reps, args.warmup)
    for leg, xs in ms.items():
        st = stats(xs)
        st["spread_over_median"] = round((st["max_ms"] - st["min_ms"]) / st["median_ms"], 3)
        res[leg] = st
    for r in RS:
        a, b = res[f"many_{r}"], res[f"singles_{r}"]
        res[f"R{r}"]["singles_over_many"] = round(b["median_ms"] / a["median_ms"], 2)
        res[f"R{r}"]["singles_ms_per_prefix"] = round(b["median_ms"] / r, 4)
    res["kernels_many_64"] = kernel_split(dict(legs)["many_64"], 5)
    res["kernels_many_1"] = kernel_split(dict(legs)["many_1"], 5)
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
