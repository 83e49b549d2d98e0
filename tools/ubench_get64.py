"""Host time of a small get: 64 device-resident 16-byte keys, device outputs,
over (a) 32 tables of 1024 lines with cb_get_many_fixed (no gate) and (b) 300
tables of ~1024 lines behind one wide FilterSet with cb_set_get_many_fixed.
At this size a call is all host work and launch latency, so it shows what a
change to the C entry points' host code costs. Per shape: the host time of an
enqueue-only call (wait=False, K calls back to back, then one sync) and the
wall time of a waited call (wait=True), microseconds, medians over --reps
rounds. Prints one JSON line (also appended to --out). Diagnostic only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsmt_amd  # noqa: E402
from lsmt_amd import workload  # noqa: E402


def flush(ks, t):
    ks = np.ascontiguousarray(ks)
    vs = np.ascontiguousarray(workload.table_value(ks, t))
    off = np.arange(0, 16 * (len(ks) + 1), 16, dtype=np.uint64)
    kb = lsmt_amd.KeyBatch(n=len(ks), data=ks.reshape(-1), offsets=off)
    vb = lsmt_amd.KeyBatch(n=len(ks), data=vs.reshape(-1), offsets=off)
    return lsmt_amd.sstable_create((kb, vb), m=1024)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--calls", type=int, default=200, help="calls per round")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    pool = workload.key_range(4242, 120_000)
    made = [flush(pool[np.unique(rng.choice(len(pool), 1024, replace=False))], t) for t in range(300)]
    tables = [m[0] for m in made][::-1]  # newest first
    fset = lsmt_amd.FilterSet(1024, width=320)
    for t, (_, bloom, zone) in enumerate(made):
        fset.assign(t, bloom)
        fset.set_zone(t, zone)
    slots = np.arange(300, dtype=np.uint32)[::-1].copy()
    n = 64
    look = np.concatenate([pool[rng.integers(0, len(pool), 48)], workload.key_range(4343, 16)])
    keys = lsmt_amd.DeviceKeys(torch.from_numpy(np.ascontiguousarray(look)).to(dev))
    out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
           torch.empty(n * 16, dtype=torch.uint8, device=dev))
    sh = torch.cuda.current_stream(dev).cuda_stream
    few = tables[:32]
    shapes = {
        "get_many_32_tables": lambda wait: lsmt_amd.get_many(few, keys, out=out, stream=sh, wait=wait),
        "set_get_many_300_tables_wide": lambda wait: lsmt_amd.get_many(tables, keys, filterset=fset, hit_rows=slots,
                                                                       out=out, stream=sh, wait=wait),
    }
    res = {"keys": n, "calls_per_round": args.calls, "rounds": args.reps}
    for name, call in shapes.items():
        for _ in range(50):
            call(False)
        torch.cuda.synchronize(dev)
        enq, waited = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(False)
            enq.append((time.perf_counter() - t0) / args.calls * 1e6)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(True)
            waited.append((time.perf_counter() - t0) / args.calls * 1e6)
        res[name] = {"enqueue_us": round(float(np.median(enq)), 2), "waited_us": round(float(np.median(waited)), 2),
                     "found": int((out[0] >= 0).sum().item())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
