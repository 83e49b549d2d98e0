"""cb_rows_write on the device (lsmt_amd.write.write_rows) against the plain
restatement in tests/rowwrite_ref.py: every case compares the keys, the values,
the log records, the log as one string and the flags byte for byte, and the
result's totals with them. The shapes are the smallest at which the kernels can
go wrong: row counts around one block of write.hip (kSelectBlock), empty
dimensions, every base64 padding, the escaper's whole table, the timestamp's
ends, one long row among short ones, and every kind of old row an UPDATE meets.
"""
import numpy as np
import pytest

import rowwrite_ref as ref
from test_fold_gpu import launch_list

pytestmark = pytest.mark.gpu

BLOCK = 256  # select.hpp kSelectBlock: the rows of one block of both kernels
HOST, BADOLD, KEYCTL = ref.HOST, ref.BADOLD, ref.KEYCTL
TS = (5).to_bytes(8, "big")


def old_arrays(old):
    """(which, val_off, vals) as a get leaves them: which < 0 where there is no row."""
    which = np.array([-1 if o is None else 0 for o in old], np.int32)
    off = np.zeros(len(old) + 1, np.uint64)
    np.cumsum([len(o or b"") for o in old], out=off[1:])
    return which, off, np.frombuffer(b"".join(o or b"" for o in old) or b"\0", np.uint8)


def check(rows, nk, columns=(), keep=(), op=ref.INSERT, ts=0, old=None, ns=b"ns", stream=None, to_device=False):
    """write_rows of the batch equals the restatement; returns the flags."""
    import torch

    import lsmt_amd.write as wr
    columns, keep = [c if isinstance(c, bytes) else c.encode() for c in columns], [c.encode() for c in keep]
    rows = [[c if isinstance(c, bytes) else c.encode() for c in row] for row in rows]
    keys, vals, recs, flags = ref.write_batch(ns, rows, nk, columns, keep, op, ts, old)
    arg, ts_arg, old_arg = rows, ts, None if old is None else old_arrays(old)
    if nk + len(columns) == 0:
        arg = len(rows)  # (rows without cells: their count)
    elif to_device:  # the cells, their offsets and the timestamps already in device memory (the ABI's order)
        w = wr._Write(ns, nk, columns, keep, op)
        flat = [c for row in rows for c in w.row_cells(row)]
        off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(c) for c in flat], out=off[1:])
        arg = (torch.from_numpy(np.frombuffer(b"".join(flat) or b"\0", np.uint8).copy()).cuda(), torch.from_numpy(off).cuda())
        columns = sorted(columns)
    if to_device and not isinstance(ts, int):
        ts_arg = torch.from_numpy(np.array(ts, np.uint64).view(np.int64)).cuda()
    if to_device:
        torch.cuda.synchronize()
    r = wr.write_rows(ns, arg, nk, columns, keep, op, ts_arg, old_arg, stream=stream)
    assert r.count == len(rows)
    assert r.keys() == keys
    assert r.values() == vals
    assert r.records() == recs
    assert r.log() == b"".join(recs)
    assert r.flags().tolist() == flags
    assert (r.key_bytes, r.val_bytes, r.log_bytes, r.flagged) == (sum(map(len, keys)), sum(map(len, vals)),
                                                                  sum(map(len, recs)), sum(f != 0 for f in flags))
    a = r.arrays()
    assert all(a.values()) and len(set(a.values())) == 7
    r.close()
    return flags


def short_rows(n):
    """n rows of two key parts and three short columns, lengths varying row by row."""
    return [[b"p%d" % (i * 7919 % 1000), b"c" * (i % 4), b"v%d" % i, b"x" * (i % 7), b"\n" if i % 5 == 0 else b"z"] for i in range(n)]


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_row_counts_around_one_block(gpu, n):
    rows = short_rows(n)
    ts = [(i * 0x9E3779B97F4A7C15) % 2 ** 64 for i in range(n)]
    assert set(check(rows, 2, ["b", "a", "c"], ts=ts)) == {0}
    assert set(check(rows, 2, ["b", "a", "c"], ts=ts, to_device=True)) == {0}
    assert set(check([r[:2] for r in rows], 2, op=ref.DELETE, ts=ts)) == {0}


def test_empty_dimensions(gpu):
    """No key column, no namespace, empty cells, an empty name; no payload
    column gives {} for an INSERT, a live row, and no payload for a DELETE."""
    n = BLOCK + 3
    check([[]] * n, 0, ns=b"", ts=9)                       # `:` and {}
    check([[]] * n, 0, ns=b"", op=ref.DELETE, ts=9)        # `:` and the timestamp alone
    check([[]] * n, 0, ns=b"", op=ref.UPDATE, ts=9)        # an UPDATE of nothing over no old row: {}
    check([[b""]] * n, 1, ns=b"")                          # `:` again, from one empty key cell
    check([[b"", b"", b""]] * n, 3)                        # ns:||
    check([[b"k%d" % i, b"", b""] for i in range(n)], 1, ["a", ""])   # empty cells under an empty name
    check([[b"", b"v"]] * 3, 1, ["a"], ns=b"")
    check([[b"v%d" % i] for i in range(n)], 0, ["a"])      # no key column, one payload column


def test_base64_padding_and_whole_quads(gpu):
    """Values of every length mod 3, from the shortest (a DELETE's 8 bytes, an
    INSERT's 8 + 2) on; the record's base64 is compared with Python's."""
    rows = [[b"k", b"x" * i] for i in range(40)]
    check(rows, 1, ["a"])
    check(rows, 1, ["a"], to_device=True)
    check([[b"k" * i] for i in range(40)], 1, op=ref.DELETE)
    vals = ref.write_batch(b"ns", rows, 1, [b"a"])[1]
    assert {len(v) % 3 for v in vals} == {0, 1, 2}


def test_every_escape(gpu):
    """A cell, a key cell, a namespace and a name holding every byte from 0x00
    to 0x7F and multibyte UTF-8; \\t and \\n in a key are flagged, not refused."""
    every = bytes(range(0x80)) + "é€😀".encode()
    flags = check([[b"k", every, every[::-1]], [every, b"", b"v"], [b"k2", b"\\", b'"']], 1, ["a", every])
    assert flags == [0, KEYCTL, 0]
    assert set(check([[b"k", b"v"]] * 3, 1, ["a"], ns=every)) == {KEYCTL}
    assert check([[b"a\tb"], [b"a\nb"], [b"a\rb|"], [b"ab"]], 1, op=ref.DELETE) == [KEYCTL, KEYCTL, 0, 0]


def test_timestamps(gpu):
    rows = short_rows(BLOCK + 1)
    for ts in (0, 2 ** 64 - 1, 0x0102030405060708):
        check(rows, 2, ["a", "b", "c"], ts=ts)
    per_row = [0, 2 ** 64 - 1] + [2 ** 63 + i for i in range(BLOCK - 1)]
    check(rows, 2, ["a", "b", "c"], ts=per_row)
    check(rows, 2, ["a", "b", "c"], ts=per_row, to_device=True)
    check(rows, 2, ["a", "b", "c"], ts=[7] * len(rows))  # per-row timestamps that equal ts_all's answer
    assert ref.write_batch(b"ns", rows, 2, [b"a", b"b", b"c"], ts=[7] * len(rows)) == ref.write_batch(b"ns", rows, 2, [b"a", b"b", b"c"], ts=7)


def test_one_long_row_among_short_ones(gpu):
    rows = short_rows(BLOCK + 9)
    rows[BLOCK + 1][3] = bytes(i * 31 % 256 for i in range(70000)).replace(b"\xff", b"\x00")
    check(rows, 2, ["a", "b", "c"])
    rows[0][0] = b"K" * 70001
    check(rows, 2, ["a", "b", "c"], to_device=True)


OLD = [
    None,                                                      # no old row
    TS,                                                        # a tombstone
    b"",                                                       # an empty value
    TS + b"not json",
    TS + b'{"a":"1","b":"2"',                                  # cut off
    TS + b'{"a":"1"}x',                                        # a byte behind the map
    b"{}",                                                     # a value that is its own payload
    TS + b'{"a":"old","b":"kept","d":"also"}',
    TS + b'{"b":"first","a":"x","b":"last"}',                  # a duplicated name: the last wins
    TS + b' { "b" : "q\\"\\\\\\/\\b\\f\\n\\r\\t\\u0041\\u00e9\\u20ac\\ud83d\\ude00\\u0000\\u001f" } ',
    TS + b'{"\\u0062":"through an escaped name"}',
    TS + '{"b":"é€😀","d":""}'.encode(),
    TS + b'{"b":"v","zz":"an extra name"}',                    # flagged: the caller's row
    TS + b'{"zz":"x","zz":"y","b":"v"}',
    TS + b'{"b":"\\ud83d"}',                                   # a lone surrogate: no valid map
    TS + b'{"b":"\xff"}',                                      # not UTF-8: no valid map
    TS + b"{}",
]


def test_update_over_every_kind_of_old_row(gpu):
    """a is set, b and d are kept: old rows absent, tombstoned, bad, with a
    duplicated name, with \\u escapes, with an extra name (flagged, lengths 0,
    and the neighbours' offsets still right)."""
    n = 2 * BLOCK + 5
    old = [OLD[i % len(OLD)] for i in range(n)]
    rows = [[b"k%d" % i, b"new%d" % i] for i in range(n)]
    flags = check(rows, 1, ["a"], ["b", "d"], ref.UPDATE, ts=11, old=old)
    assert [flags[i] for i in range(len(OLD))] == [0, 0, 0, BADOLD, BADOLD, BADOLD, 0, 0, 0, 0, 0, 0, HOST, HOST, BADOLD,
                                                   BADOLD, 0]
    check(rows, 1, ["a"], ["b", "d"], ref.UPDATE, ts=11, old=old, to_device=True)
    # nothing set: the old rows written again under a new timestamp
    check([r[:1] for r in rows], 1, [], ["a", "b", "d"], ref.UPDATE, ts=12, old=old)
    # old arrays given, and no row has one
    assert set(check(rows, 1, ["a"], ["b", "d"], ref.UPDATE, old=[None] * n)) == {0}
    # a flagged row meets a key with a tab
    assert check([[b"k\t", b"v"]], 1, ["a"], [], ref.UPDATE, old=[OLD[12]]) == [HOST | KEYCTL]


@pytest.mark.parametrize("where", ["first", "last", "alone", "all", "block edges"])
def test_flagged_rows_leave_their_neighbours_offsets_right(gpu, where):
    n = 1 if where == "alone" else 2 * BLOCK + 1
    at = {"first": [0], "last": [n - 1], "alone": [0], "all": range(n), "block edges": [BLOCK - 1, BLOCK, 2 * BLOCK]}[where]
    old = [TS + b'{"b":"row %d"}' % i for i in range(n)]
    for i in at:
        old[i] = TS + b'{"b":"v","extra":"%d"}' % i
    flags = check([[b"k%d" % i, b"v"] for i in range(n)], 1, ["a"], ["b"], ref.UPDATE, ts=3, old=old)
    assert [i for i, f in enumerate(flags) if f] == list(at) and {flags[i] for i in at} == {HOST}


def test_host_and_device_inputs_on_a_side_stream(gpu):
    import torch
    rows = short_rows(BLOCK + 2)
    old = [OLD[i % len(OLD)] for i in range(len(rows))]
    s = torch.cuda.Stream()
    ts = list(range(len(rows)))
    for to_device in (False, True):
        check([r[:4] for r in rows], 2, ["c", "a"], ["b", "d"], ref.UPDATE, ts=ts, old=old, stream=s, to_device=to_device)
        check(rows, 2, ["a", "b", "c"], ts=5, stream=s, to_device=to_device)


def test_a_written_batch_with_host_rows_makes_no_table(gpu):
    import lsmt_amd.write as wr
    r = wr.write_rows("ns", [["k", "v"]], 1, ["a"], op="update", old=old_arrays([OLD[12]]))
    assert r.flags().tolist() == [HOST] and (r.val_bytes, r.log_bytes) == (0, 0)
    with pytest.raises(ValueError):
        r.to_table()
    with pytest.raises(ValueError):
        r.replay()
    r.close()


WRITE_1024 = {"k_write_size": 1, "k_scan_reduce": 3, "k_tile_scan": 3, "k_scan_apply": 3, "k_write_emit": 1}


def test_launch_list(gpu):
    """cb_rows_write's own launches, which DESIGN.md 6.16 records: the size
    pass, three scans of three launches each, the emit."""
    import lsmt_amd.write as wr
    rows = short_rows(1024)
    old = old_arrays([OLD[7]] * 1024)
    got = launch_list(gpu, lambda: wr.write_rows("ns", rows, 2, ["a", "b", "c"]).close())
    assert got == WRITE_1024 and sum(got.values()) == 11
    got = launch_list(gpu, lambda: wr.write_rows("ns", [r[:3] for r in rows], 2, ["a"], ["b", "d"], "update", old=old).close())
    assert got == WRITE_1024
