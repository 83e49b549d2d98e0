"""cb_replies_fold on the device, timed against the same answer computed other
ways, in alternating rounds of one process on one MI355X.

Shapes: 3 replicas whose tables hold 300 x 1024 rows in all, and 3 replicas of
about 1.2M rows in all; ubench_select.py's rows (16-hex-character keys, an
8-byte timestamp, then {"a":"NN","b":"N","c":"NNNN"}), the replicas' keys drawn
from one pool, so most keys are on two or three of them. Each replica's reply is
what ScanResult.select(meta=True) writes over a scan of its table alone.

  fold        cb_replies_fold of the three replies, joined in device memory;
  fold_host_bytes  the same replies in pageable host memory (staged by the call);
  (a) lww_select   cb_tables_scan_lww + cb_scan_select(JSON) over the same
              replicas held as tables on the device: the same answer when no
              network lies between;
  (b) replay  cb_log_replay of a log of as many lines: the same chain shape
              (line index, mark, gather, sort, select, format);
  (c) host    cb_replies_fold with device = -1 (bytes in host memory), here and
              at 3 x 1 row and 3 x 1024 rows next to the device fold of the same
              replies: the crossover a caller needs to choose between the two.

Answers are compared first: the fold's response must equal (a)'s response and
the host fold's, byte for byte, and the two folds' stats and rows must agree.
Every leg is timed by an event pair around the call (it waits for its own
stream inside) and by the host's clock; the host fold by the host's clock
alone. Then the fold's launch list (cb_profile_read) in a pass of its own.

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
from lsmt_amd import _lib, replies as rp  # noqa: E402
from ubench_where import make_tables  # noqa: E402

KERNELS = ["k_line_count", "k_scan_reduce", "k_tile_scan", "k_scan_apply", "k_line_emit", "k_line_finish",
           "k_reply_mark", "k_reply_gather", "k_sorted_check", "k_entry_sort", "k_bin_count", "k_bin_offsets",
           "k_bin_scatter", "k_bin_sort", "k_compact_ts", "k_compact_lww_runs", "k_compact_lww_tiles", "k_fold_size",
           "k_fold_write"]
WAITS = ["the pieces' count", "the entries' counts and the first bad piece", "the winners' totals",
         "the end (the result is complete)"]
COLS = ["a", "b", "c"]


def fold_joined(buf, off, device, stream):
    """cb_replies_fold over replies already joined in one buffer."""
    h = ctypes.c_void_p()
    ptr = buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data
    _lib.check(_lib.load().cb_replies_fold(ptr, off.ctypes.data, len(off) - 1, device,
                                           None if stream is None else stream.cuda_stream, ctypes.byref(h), None))
    return rp.FoldResult(h.value, device)


def rounds(legs, stream, reps, warm):
    """{name: ([event ms], [wall ms])}: every round runs each leg once, odd
    rounds in reverse order. A host leg (name ends in _host) has no events."""
    out = {name: ([], []) for name, _ in legs}
    with torch.cuda.stream(stream):
        for i in range(warm + reps):
            for name, fn in (legs if i % 2 == 0 else legs[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                host = name.endswith("_host")
                if not host:
                    e0.record(stream)
                t0 = time.perf_counter()
                keep = fn()
                t1 = time.perf_counter()
                if not host:
                    e1.record(stream)
                    e1.synchronize()
                if hasattr(keep, "close"):
                    keep.close()
                del keep
                if i >= warm:
                    out[name][1].append((t1 - t0) * 1e3)
                    if not host:
                        out[name][0].append(e0.elapsed_time(e1))
    return out


def stats(xs):
    if not xs:
        return None
    mn, med, mx = float(np.min(xs)), float(np.median(xs)), float(np.max(xs))
    return {"min_ms": round(mn, 4), "median_ms": round(med, 4), "max_ms": round(mx, 4),
            "spread_over_median": round((mx - mn) / med, 3), "reps": len(xs)}


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


def replies_of(tables):
    """Each replica's META reply in device memory, joined, with the offsets."""
    metas = [lsmt_amd.scan([t]).select(COLS, meta=True) for t in tables]
    parts = []
    for m in metas:
        t = torch.empty(max(m.bytes, 1), dtype=torch.uint8, device="cuda")
        m.copy(text=t)
        parts.append(t[:m.bytes])
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([int(p.numel()) for p in parts], out=off[1:])
    return torch.cat(parts).contiguous(), off


def shape(name, per, pool_n, args, dev, with_yardsticks):
    tables = make_tables(3, per, pool_n, 3)  # (table t stamps t + 1: the last replica's rows are the newest)
    stream = torch.cuda.Stream(dev)
    dbuf, off = replies_of(tables)
    hbuf = dbuf.cpu().numpy()
    res = {"shape": name, "replicas": 3, "lines": int(sum(t.nlines for t in tables)), "reply_bytes": int(off[-1])}
    f, h = fold_joined(dbuf, off, 0, stream), fold_joined(hbuf, off, -1, None)
    st = {n: int(getattr(f.stats, n)) for n, _ in f.stats._fields_}
    assert st == {n: int(getattr(h.stats, n)) for n, _ in h.stats._fields_} and st["host_rows"] == 0
    assert f.text() == h.text() and f.rows() == h.rows()
    lww = lsmt_amd.scan_lww(tables, ranges=[(b"", None)])
    assert f.text() == lww.select(COLS, meta=False).text(), f"{name}: the fold differs from scan_lww + select"
    res["stats"] = st
    res["answers_equal"] = True
    f.close()
    h.close()
    legs = [("fold", lambda: fold_joined(dbuf, off, 0, stream)),
            ("fold_host_bytes", lambda: fold_joined(hbuf, off, 0, stream)),
            ("c_fold_host", lambda: fold_joined(hbuf, off, -1, None))]
    if with_yardsticks:
        n = res["lines"]
        recs = [(b"%016x" % (i * 0x9E3779B97F4A7C15 % 2 ** 64), b"\0\0\0\0\0\0\0\1" + b"%08d" % (i % 10 ** 8))
                for i in range(n)]
        dlog = torch.from_numpy(np.frombuffer(lsmt_amd.wal_bytes(recs), np.uint8).copy()).cuda()
        res["log_bytes"] = int(dlog.numel())
        legs += [("a_lww_select", lambda: lsmt_amd.scan_lww(tables, ranges=[(b"", None)],
                                                            stream=stream.cuda_stream).select(COLS)),
                 ("b_replay", lambda: lsmt_amd.replay_log(dlog, m=1024, stream=stream.cuda_stream)[0])]
    ms = rounds(legs, stream, args.reps, args.warmup)
    for leg, (ev, wall) in ms.items():
        res[leg] = {"event": stats(ev), "wall": stats(wall)}
    med = lambda leg, kind="event": res[leg][kind]["median_ms"]  # noqa: E731
    res["host_over_device_wall"] = round(med("c_fold_host", "wall") / med("fold_host_bytes", "wall"), 3)
    if with_yardsticks:
        res["fold_over_a"] = round(med("fold") / med("a_lww_select"), 3)
        res["fold_over_b"] = round(med("fold") / med("b_replay"), 3)
    res["launches_fold"] = launch_list(lambda: fold_joined(dbuf, off, 0, stream))
    res["launch_count"] = sum(v["launches"] for v in res["launches_fold"].values())
    res["waits"] = WAITS
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    assert lsmt_amd.device_count() > 0, "no GPU visible"
    rows = [shape("3 replies of 1 row", 1, 64, args, dev, False),
            shape("3 replies of 1024 rows", 1024, 2048, args, dev, False),
            shape("3 replies, 300 x 1024 rows in all", 102_400, 160_000, args, dev, True),
            shape("3 replies, 1.2M rows in all", 400_000, 650_000, args, dev, True)]
    doc = {"what": "cb_replies_fold against (a) cb_tables_scan_lww + cb_scan_select(JSON) over the replicas as tables, "
                   "(b) cb_log_replay of a log of as many lines and (c) the host fold (device -1)",
           "method": "tools/ubench_fold.py on one MI355X: answers compared first (fold == host fold == (a)'s response), "
                     "then %d rounds after %d, all legs alternating in one process, an event pair and the host's clock "
                     "around each call (waits included); the launch list from cb_profile_read in a run of its own; "
                     "spread = (max - min) / median" % (args.reps, args.warmup),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
