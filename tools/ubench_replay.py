"""cb_log_replay against the two ways the same records reach a table today,
timed with HIP events in the same alternating rounds, on logs of 1024 lines
(the reference's log never exceeds max_memtable_size = 1024 records: a flush
clears it) and of 1M lines, with 0 % and 50 % repeated keys:

  replay   cb_log_replay of the log's bytes in device memory (and, as a third
           row, of the same bytes in pageable host memory);
  (a)      cb_sstable_create from device arrays that are already parsed and
           deduplicated, unsorted: the floor, what the store enqueues today
           AFTER the host has split the log, checked UTF-8, decoded every value
           and deduplicated the keys; the host's parse is not counted;
  (b)      cb_tables_compact over the same records pre-flushed as sorted tables
           of 1024 records each (the making of those tables is not counted).

Answers are compared first: the replayed file must equal the host restatement
(split, a dict in log order, the sorted lines), (a)'s file and (b)'s file.
Then the rounds, then each entry's launch list (cb_profile_read).

Prints one JSON line per shape (also appended to --out). Diagnostic only.
"""
import argparse
import base64
import ctypes
import json
import os
import sys

import numpy as np
import torch

KERNELS = ["k_line_count", "k_scan_reduce", "k_tile_scan", "k_scan_apply", "k_line_emit", "k_line_finish", "k_log_mark",
           "k_log_gather", "k_compact_klen", "k_compact_gather", "k_sorted_check", "k_entry_sort", "k_bin_count",
           "k_bin_offsets", "k_bin_scatter", "k_bin_sort", "k_compact_select", "k_compact_format", "k_format",
           "k_insert_lds", "k_insert_direct", "k_build_part", "k_build_tile", "k_pfx_masks", "k_table_dir",
           "k_zone_bounds"]


def make_records(n, repeated, seed):
    """n records (key, value) in log order: 16-hex-digit keys, 16-byte values
    (an 8-byte timestamp, 8 bytes of payload); `repeated` of 0.5: half as many
    distinct keys, each written twice at random places."""
    rng = np.random.default_rng(seed)
    distinct = n - int(n * repeated)
    raw = rng.integers(0, 256, (distinct, 8), dtype=np.uint8)
    keys = np.unique(raw.view(">u8").reshape(-1))
    assert len(keys) == distinct, "key collision: pick another seed"
    keys = rng.permutation(keys)
    which = rng.permutation(np.concatenate([np.arange(distinct), rng.choice(distinct, n - distinct, replace=False)]))
    ks = [b"%016x" % int(k) for k in keys]
    return [(ks[w], int(i).to_bytes(8, "big") + ks[w][:8]) for i, w in enumerate(which)]


def rounds_ms(fns, stream, reps, warm):
    """Device time per call of every fn, one after the other in each round."""
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


def ratio(a, b):
    r = np.array(a) / np.array(b)
    return {"median": round(float(np.median(r)), 3), "min": round(float(r.min()), 3), "max": round(float(r.max()), 3)}


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


def device_batch(lsmt_amd, items):
    offs = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(x) for x in items], out=offs[1:])
    data = np.frombuffer(b"".join(items), np.uint8).copy()
    return lsmt_amd.KeyBatch(n=len(items), data=torch.from_numpy(data).cuda(),
                             offsets=torch.from_numpy(offs.view(np.int64)).cuda())


def shape(mods, n, repeated, args, dev):
    lsmt_amd, L = mods
    recs = make_records(n, repeated, 1000 + n % 997 + int(repeated * 10))
    log = lsmt_amd.wal_bytes(recs)
    res = {"lines": n, "repeated_keys": repeated, "log_bytes": len(log)}
    # the host restatement: split, a dict in log order, the sorted lines
    rows = {}
    for piece in log.split(b"\n"):
        if piece and b"\t" in piece:
            k, text = piece.split(b"\t", 1)
            rows[k] = text
    want = b"".join(k + b"\t" + rows[k] + b"\n" for k in sorted(rows))
    dlog = torch.from_numpy(np.frombuffer(log, np.uint8).copy()).cuda()
    t, _, _, st = lsmt_amd.replay_log(dlog, m=1024)
    res["keys"] = int(st.keys)
    res["replay_equals_host_restatement"] = bool(t.data() == want)
    assert res["replay_equals_host_restatement"] and st.entries == n and st.keys == len(rows)
    # (a): parsed and deduplicated on the host (not counted), unsorted, in device arrays
    last = {k: base64.b64decode(v) for k, v in rows.items()}  # (a dict in order of each key's first write: unsorted)
    kb, vb = device_batch(lsmt_amd, list(last)), device_batch(lsmt_amd, list(last.values()))
    res["create_equals_replay"] = bool(lsmt_amd.sstable_create((kb, vb), m=1024)[0].data() == want)
    # (b): the same records pre-flushed as sorted tables of 1024 records, newest first
    tables = []
    for i in range(0, n, 1024):
        chunk = dict(recs[i:i + 1024])
        tables.insert(0, lsmt_amd.sstable_create(sorted(chunk.items()), m=1024)[0])
    res["tables_b"] = len(tables)
    res["compact_equals_replay"] = bool(lsmt_amd.compact(tables, m=1024)[0].data() == want)
    assert res["create_equals_replay"] and res["compact_equals_replay"]
    s = torch.cuda.Stream(dev)
    fns = {"replay": lambda: lsmt_amd.replay_log(dlog, m=1024, stream=s.cuda_stream),
           "replay_host_log": lambda: lsmt_amd.replay_log(log, m=1024, stream=s.cuda_stream),
           "a_sstable_create": lambda: lsmt_amd.sstable_create((kb, vb), m=1024, stream=s.cuda_stream),
           "b_compact": lambda: lsmt_amd.compact(tables, m=1024, stream=s.cuda_stream)}
    ms = rounds_ms(fns, s, args.reps, args.warmup)
    for name in fns:
        res[name] = stats(ms[name])
    res["ratio_replay_over_a"] = ratio(ms["replay"], ms["a_sstable_create"])
    res["ratio_replay_over_b"] = ratio(ms["replay"], ms["b_compact"])
    for name in ("replay", "a_sstable_create", "b_compact"):
        res["launches_" + name] = launch_list(L, fns[name])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--lines", type=int, nargs="*", default=[1024, 1 << 20])
    p.add_argument("--out", default=None)
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import lsmt_amd
    from lsmt_amd._lib import load
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    for n in args.lines:
        for repeated in (0.0, 0.5):
            line = json.dumps(shape((lsmt_amd, load()), n, repeated, args, dev))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
