"""cb_rows_write on the device, timed against its yardsticks in alternating
rounds of one process on one MI355X.

Rows: a timestamp, two key parts (16 hex characters and 4 digits) and three
short columns, {"a":"NN","b":"N","c":"NNNN"}: ubench_select.py's rows, written
instead of read. Sizes: 1024 rows and 2^20 rows, and a few small counts for the
crossover.

  insert        cb_rows_write(INSERT), cells, offsets in device memory;
  insert_host_cells  the same cells in pageable host memory (staged by the call);
  update        cb_rows_write(UPDATE) of column a over the INSERT's values as old
                rows, b and c kept;
  (a) select    cb_rows_select of all columns over the same rows: the
                parse-and-re-encode floor (one walk of a payload, one text out);
  (b) host      a loop of cb_row_write over the same rows, through ctypes, by the
                host's clock (over at most 65536 rows, scaled to the batch);
  (c) flush     cb_sstable_create of the written arrays, finalised: what share of
                a flush the encoding is.

Answers are compared first: the device's keys, values and records equal the
host twin's for INSERT and UPDATE (the first 1024 rows), and the select of the
written values returns the cells. Every device leg is timed by an event pair
around the call (it waits for its own stream inside) and by the host's clock.
Then the launch list (cb_profile_read) in a pass of its own.

Writes one JSON document (--out). Diagnostic only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmt_amd  # noqa: E402
from lsmt_amd import _lib, write as wr  # noqa: E402
from ubench_fold import rounds, stats  # noqa: E402

KERNELS = ["k_write_size", "k_scan_reduce", "k_tile_scan", "k_scan_apply", "k_write_emit"]
WAITS = ["the three totals and the two counts", "the end (the result is complete)"]
COLS, KC = ["a", "b", "c"], ("pk", "ck")
WIDTHS = [16, 4, 2, 1, 4]


def cells_of(n, widths):
    """(data uint8, offsets int64) of n rows of fixed-width cells: pk, ck, a, b, c."""
    rows = [b"%016x%04d%02d%d%04d" % (i * 0x9E3779B97F4A7C15 % 2 ** 64, i % 10 ** 4, i % 100, i % 10, i * 7 % 10 ** 4)
            for i in range(n)]
    full = np.frombuffer(b"".join(rows), np.uint8).reshape(n, sum(WIDTHS))
    data = np.ascontiguousarray(full[:, :sum(widths)]).reshape(-1)
    off = np.concatenate([[0], np.cumsum(np.tile(widths, n))]).astype(np.int64)
    return data, off, rows


def host_loop(stmt, data, off, width, n, ts, olds=None):
    """(seconds, [key | value | record per row]) of cb_row_write over n rows."""
    L = _lib.load()
    base, obase = data.ctypes.data, off.ctypes.data
    kl, vl, rl, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint8()
    refs = (ctypes.byref(kl), ctypes.byref(vl), ctypes.byref(rl), ctypes.byref(f))
    out = ctypes.create_string_buffer(512)
    got = []
    t0 = time.perf_counter()
    for i in range(n):
        old = olds[i] if olds is not None else None
        rc = L.cb_row_write(stmt.ref(), base, obase + 8 * width * i, ts, old, len(old) if old else 0, int(old is not None),
                            out, 512, *refs)
        assert rc == 0
        got.append(out.raw[:kl.value + vl.value + rl.value])
    return time.perf_counter() - t0, got


def launch_list(fn, reps=3):
    L = _lib.load()
    L.cb_profile_enable(1)
    L.cb_profile_reset()
    for _ in range(reps):
        fn().close()
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        if L.cb_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value:
            out[name] = {"us_per_call": round(ms.value * 1e3 / reps, 2), "launches": int(n.value // reps)}
    L.cb_profile_enable(0)
    return out


def joined(w):
    return [k + v + r for k, v, r in zip(w.keys(), w.values(), w.records())]


def shape(n, args, dev, full):
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    data, off, _ = cells_of(n, WIDTHS)
    udata, uoff, _ = cells_of(n, WIDTHS[:3])
    ddata, doff = torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda()
    dudata, duoff = torch.from_numpy(udata).cuda(), torch.from_numpy(uoff).cuda()
    ins = lambda cells: wr.write_rows("ns", cells, 2, COLS, ts=5, stream=s)  # noqa: E731
    w = ins((ddata, doff))
    res = {"rows": n, "key_bytes": w.key_bytes, "val_bytes": w.val_bytes, "log_bytes": w.log_bytes}
    # the old rows of the UPDATE and the rows of the select: the INSERT's values, in tensors
    vals = torch.empty(w.val_bytes + 64, dtype=torch.uint8, device="cuda")
    voff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    keys = torch.empty(w.key_bytes + 64, dtype=torch.uint8, device="cuda")
    koff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    w.copy(keys=keys, key_off=koff, vals=vals, val_off=voff)
    which = torch.zeros(n, dtype=torch.int32, device="cuda")
    upd = lambda: wr.write_rows("ns", (dudata, duoff), 2, ["a"], ["b", "c"], "update", ts=6, old=(which, voff, vals),  # noqa: E731
                                stream=s)
    batch = lsmt_amd.KeyBatch(n=n, data=keys, offsets=koff)
    sel = lambda: lsmt_amd.select_rows(batch, None, voff, vals, COLS + list(KC), KC, skip=3, stream=s)  # noqa: E731
    # answers first
    m = min(n, 1024)
    si, su = wr._Write("ns", 2, COLS), wr._Write("ns", 2, ["a"], ["b", "c"], "update")
    head = joined(w)[:m] if n <= 4096 else None
    t_ins, got = host_loop(si, data, off, 5, min(n, 65536), 5)
    if head is not None:
        assert got[:m] == head, "the device INSERT differs from the host twin"
    olds = w.values()[:m] if n <= 4096 else None
    if olds is not None:
        u = upd()
        assert joined(u)[:m] == host_loop(su, udata, uoff, 3, m, 6, olds)[1], "the device UPDATE differs from the host twin"
        assert u.flagged == 0
        u.close()
        r = sel()
        rows = json.loads(r.text().decode())
        want = [dict(zip(["pk", "ck"] + COLS, [bytes(data[27 * i + a:27 * i + b]).decode() for a, b in
                                               zip(np.cumsum([0] + WIDTHS[:-1]), np.cumsum(WIDTHS))])) for i in range(m)]
        assert rows[:m] == want, "the select of the written rows does not return the cells"
        r.close()
    res["answers_equal"] = head is not None
    res["b_host_loop"] = {"rows_timed": min(n, 65536), "us_per_row": round(t_ins / min(n, 65536) * 1e6, 3),
                          "ms_for_the_batch": round(t_ins / min(n, 65536) * n * 1e3, 4)}
    legs = [("insert", lambda: ins((ddata, doff))), ("insert_host_cells", lambda: ins((data, off))), ("update", upd)]
    if full:
        legs += [("a_select", sel), ("c_flush", lambda: w.to_table(stream=s)[0])]
    ms = rounds(legs, stream, args.reps, args.warmup)
    for leg, (ev, wall) in ms.items():
        res[leg] = {"event": stats(ev), "wall": stats(wall)}
    med = lambda leg, kind="event": res[leg][kind]["median_ms"]  # noqa: E731
    res["host_loop_over_device_wall"] = round(res["b_host_loop"]["ms_for_the_batch"] / med("insert_host_cells", "wall"), 3)
    if full:
        res["insert_over_a"] = round(med("insert") / med("a_select"), 3)
        res["update_over_a"] = round(med("update") / med("a_select"), 3)
        res["insert_over_c"] = round(med("insert") / med("c_flush"), 3)
        res["launches_insert"] = launch_list(lambda: ins((ddata, doff)))
        res["launches_update"] = launch_list(upd)
        res["launch_count"] = sum(v["launches"] for v in res["launches_insert"].values())
        res["waits"] = WAITS
    w.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    rows = [shape(n, args, dev, False) for n in (1, 16, 64, 256)] + [shape(1024, args, dev, True), shape(1 << 20, args, dev, True)]
    cross = next((r["rows"] for r in rows if r["host_loop_over_device_wall"] >= 1.0), None)
    doc = {"what": "cb_rows_write (INSERT, and UPDATE of one column over old rows) against (a) cb_rows_select of all "
                   "columns over the same rows, (b) a host loop of cb_row_write and (c) cb_sstable_create of the written arrays",
           "method": "tools/ubench_write.py on one MI355X: answers compared first (device == host twin for INSERT and "
                     "UPDATE, the select returns the cells; batches up to 4096 rows), then %d rounds after %d, all legs "
                     "alternating in one process, an event pair and the host's clock around each call (waits included); the "
                     "host loop goes through ctypes, by the host's clock; the launch list from cb_profile_read in a run of "
                     "its own; spread = (max - min) / median" % (args.reps, args.warmup),
           "device": torch.cuda.get_device_name(0), "rows": rows,
           "crossover_rows": cross,
           "crossover": "the smallest measured batch at which the host loop takes as long as the device call with host "
                        "cells, by the host's clock; below it cb_row_write is the call to make"}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
