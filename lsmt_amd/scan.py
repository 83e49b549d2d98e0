"""Range and prefix scans and counts over SSTables, merged on the device
(cb_tables_scan*, cb_tables_count*), and a scan's result in device memory."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._ffi import _Handle, _key_bytes, _L, _pack, _ptr_of, _raise, _stream
from ._lib import check
from .rows import RowsResult, _per_range, _Select, _Where
from .table import Table, _table_list


def prefix_end(prefix) -> "bytes | None":
    """The exclusive upper bound of "starts with prefix" in byte order
    (cb_key_prefix_end, host only): the prefix without its trailing 0xFF
    bytes, its last remaining byte incremented; None when nothing remains (an
    empty prefix, or all 0xFF), i.e. unbounded above."""
    p = _key_bytes(prefix)
    out = ctypes.create_string_buffer(max(len(p), 1))
    n, has = ctypes.c_uint64(), ctypes.c_int()
    check(_L().cb_key_prefix_end(p, len(p), out, ctypes.byref(n), ctypes.byref(has)))
    return out.raw[:n.value] if has.value else None


class ScanResult(_Handle):
    """A scan's entries in device memory (cb_scan_*): sorted by key, each with
    its decoded value and the index in the scanned table list of the table
    that supplied it. Complete when scan() returns; the scanned tables may be
    closed while it lives."""
    _destroy = "cb_scan_destroy"

    def __init__(self, handle: int, device: int):
        self._h = ctypes.c_void_p(handle)
        self.device = device
        n, kb, vb, tr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        check(_L().cb_scan_info(self._h, ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb), ctypes.byref(tr)))
        self.count, self.key_bytes, self.val_bytes = int(n.value), int(kb.value), int(vb.value)
        self.truncated = bool(tr.value)
        nr = ctypes.c_uint64()
        check(_L().cb_scan_ranges(self._h, ctypes.byref(nr), None))
        self.nranges = int(nr.value)

    def __len__(self) -> int:
        return self.count

    def copy_keys(self, key_off=None, keys=None) -> None:
        """key_off (uint64[count + 1]) and / or keys (uint8[key_bytes]) into
        numpy arrays or device tensors."""
        check(_L().cb_scan_keys(self._h, _ptr_of(key_off)[0], _ptr_of(keys)[0]))

    def copy_values(self, val_off=None, vals=None) -> None:
        check(_L().cb_scan_values(self._h, _ptr_of(val_off)[0], _ptr_of(vals)[0]))

    def copy_which(self, which) -> None:
        check(_L().cb_scan_which(self._h, _ptr_of(which)[0]))

    def raw(self):
        """(key_off uint64[count + 1], keys uint8[key_bytes], val_off
        uint64[count + 1], vals uint8[val_bytes]) as numpy arrays."""
        ko, vo = np.zeros(self.count + 1, np.uint64), np.zeros(self.count + 1, np.uint64)
        kb, vb = np.zeros(max(self.key_bytes, 1), np.uint8), np.zeros(max(self.val_bytes, 1), np.uint8)
        self.copy_keys(ko, kb)
        self.copy_values(vo, vb)
        return ko, kb[:self.key_bytes], vo, vb[:self.val_bytes]

    @staticmethod
    def _split(off, data) -> "list[bytes]":
        raw, o = data.tobytes(), off.tolist()
        return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]

    def keys(self) -> "list[bytes]":
        ko = np.zeros(self.count + 1, np.uint64)
        kb = np.zeros(max(self.key_bytes, 1), np.uint8)
        self.copy_keys(ko, kb)
        return self._split(ko, kb)

    def values(self) -> "list[bytes]":
        vo = np.zeros(self.count + 1, np.uint64)
        vb = np.zeros(max(self.val_bytes, 1), np.uint8)
        self.copy_values(vo, vb)
        return self._split(vo, vb)

    def which(self) -> np.ndarray:
        w = np.zeros(max(self.count, 1), np.int32)
        self.copy_which(w)
        return w[:self.count]

    def copy_ts(self, ts) -> None:
        check(_L().cb_scan_ts(self._h, _ptr_of(ts)[0]))

    def ts(self) -> np.ndarray:
        """uint64[count]: every entry's write timestamp, the first 8 bytes of
        its value as a big-endian integer, 0 for a value below 8 bytes
        (cb_scan_ts; the reference's split_ts, src/query.rs:21-27)."""
        t = np.zeros(max(self.count, 1), np.uint64)
        self.copy_ts(t)
        return t[:self.count]

    def copy_match(self, flags, where, key_columns=(), skip=None) -> None:
        """match()'s verdicts as bytes (0 / 1) into a numpy array or device
        tensor of `count` uint8."""
        w = _Where(where, key_columns)
        sk = None if skip is None else np.ascontiguousarray(_per_range(skip, self.nranges), np.uint32)
        check(_L().cb_scan_match(self._h, _ptr_of(sk)[0], w.ref(), _ptr_of(flags)[0]))

    def match(self, where, key_columns=(), skip=None) -> np.ndarray:
        """bool[count]: which entries are rows that match `where` (count_where's
        rule, cb_scan_match): a filtered select over a result that is already
        on the device. Dead entries are False. skip: the bytes of each key
        before its `|`-separated parts, one number for all ranges or one per
        range (default 0)."""
        f = np.zeros(max(self.count, 1), np.uint8)
        self.copy_match(f, where, key_columns, skip)
        return f[:self.count].astype(bool)

    def select(self, columns, key_columns=(), casts=None, skip=None, meta=False) -> RowsResult:
        """SELECT columns over this result's entries, on the device
        (cb_scan_select): the response bytes of the reference's
        exec_select_schema, projected, cast and re-encoded per row by the rule of
        lsmt_amd/csrc/rowselect.hpp. columns in any order; casts: a mapping name
        -> 0 / 1 or one per column (1: integer). skip as in match(). meta: the
        coordinator's `key \\t ts \\t val` lines in place of the JSON array."""
        q = _Select(columns, key_columns, casts)
        sk = None if skip is None else np.ascontiguousarray(_per_range(skip, self.nranges) + [0], np.uint32)
        h = ctypes.c_void_p()
        _raise(_L().cb_scan_select(self._h, _ptr_of(sk)[0], q.ref(), int(bool(meta)), ctypes.byref(h)))
        return RowsResult(h.value, self.device)

    def items(self) -> "list[tuple[bytes, bytes]]":
        return list(zip(self.keys(), self.values()))

    def range_off(self) -> np.ndarray:
        """uint64[nranges + 1]: range r's entries are [range_off[r],
        range_off[r + 1]) (cb_scan_ranges; {0, count} for a scan of one range)."""
        off = np.zeros(self.nranges + 1, np.uint64)
        check(_L().cb_scan_ranges(self._h, None, _ptr_of(off)[0]))
        return off


def scan(tables: Sequence[Table], lo=b"", hi=None, prefix=None, limit: int = 0, stream=None) -> ScanResult:
    """Every live entry of well-formed tables (tables[0] newest, as get_many
    takes them) whose key lies in [lo, hi), or starts with prefix, merged on
    the device (cb_tables_scan): sorted by key bytes, each key with the value
    Database::get (src/lib.rs:128-134) returns for it over these tables — the
    newest line whose value decodes; a key whose value decodes nowhere is
    absent. hi=None: unbounded above. limit > 0: the first `limit` entries,
    ScanResult.truncated saying whether more qualified. The reference's
    Database::scan / scan_ns (src/lib.rs:144-146, 178-186) read the memtable
    alone; a store merges that over this result, as it does for get.
    scan_ns(ns) is prefix = ns + ":". The tables are not modified and may be
    closed as soon as the call returns."""
    if prefix is not None and (hi is not None or _key_bytes(lo)):
        raise ValueError("prefix excludes lo and hi")
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    if prefix is not None:
        p = _key_bytes(prefix)
        _raise(_L().cb_tables_scan_prefix(arr, len(tables), p, len(p), int(limit), _stream(stream), ctypes.byref(h)))
    else:
        lo_b = _key_bytes(lo)
        hi_b = _key_bytes(hi) if hi is not None else None
        _raise(_L().cb_tables_scan(arr, len(tables), lo_b, len(lo_b), hi_b, len(hi_b) if hi_b is not None else 0,
                                   int(hi_b is not None), int(limit), _stream(stream), ctypes.byref(h)))
    return ScanResult(h.value, dev)


def scan_many(tables: Sequence[Table], ranges=None, prefixes=None, stream=None) -> ScanResult:
    """Many scans from one merge (cb_tables_scan_many / _prefixes): the entries
    of scan(tables, lo, hi) for every (lo, hi) of `ranges`, or of scan(tables,
    prefix=p) for every p of `prefixes`, one after the other in one
    ScanResult, whose range_off() says where each begins (so len of range r,
    COUNT(*) per namespace, is a difference of two offsets). The ranges must
    ascend and be pairwise disjoint (each lo and hi <= the next lo; touching
    is fine, empty ranges are fine); overlapping, descending or nested ones
    ("a:" with "a:b:") are refused (CB_EINVAL): sort them, split them at
    overlaps, or fall back to single scans. hi=None (unbounded above) is
    allowed on the last range only, as is a prefix without an end (empty, all
    0xFF). There is no limit in this form. scan_ns over many namespaces is
    prefixes=[ns + ":" for ns in sorted(names)]."""
    if (ranges is None) == (prefixes is None):
        raise ValueError("exactly one of ranges and prefixes")
    if prefixes is None:
        ranges = list(ranges)
        if any(hi is None for _, hi in ranges[:-1]):
            raise ValueError("hi=None is allowed on the last range only")
        return _scan_ranges(_L().cb_tables_scan_many, tables, ranges, None, stream)
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    data, off = _pack([_key_bytes(p) for p in prefixes])  # (the library turns them into ranges itself)
    _raise(_L().cb_tables_scan_prefixes(arr, len(tables), data, _ptr_of(off)[0], len(off) - 1, _stream(stream),
                                        ctypes.byref(h)))
    return ScanResult(h.value, dev)


def _range_list(ranges, prefixes):
    """(bounds bytes, bound_off uint64[2 nr + 1], nr, last_unbounded) of a
    list of (lo, hi) ranges, or of prefixes turned into ranges with
    prefix_end: cb_tables_scan_many's list format."""
    if (ranges is None) == (prefixes is None):
        raise ValueError("exactly one of ranges and prefixes")
    if prefixes is not None:
        ranges = [(p, prefix_end(p)) for p in map(_key_bytes, prefixes)]
    pairs = [(_key_bytes(lo), hi) for lo, hi in ranges]
    if any(hi is None for _, hi in pairs[:-1]):
        raise ValueError("hi=None (or a prefix without an end) is allowed on the last range only")
    last_unbounded = int(bool(pairs) and pairs[-1][1] is None)
    data, off = _pack([b for lo, hi in pairs for b in (lo, _key_bytes(hi) if hi is not None else b"")])
    return data, off, len(pairs), last_unbounded


def _scan_ranges(entry, tables: Sequence[Table], ranges, prefixes, stream, *args) -> ScanResult:
    """One scan entry over a range list: entry(tables, nt, bounds, bound_off,
    nr, last_unbounded, *args, stream, &result)."""
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    _raise(entry(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, *args, _stream(stream),
                 ctypes.byref(h)))
    return ScanResult(h.value, dev)


def _count_ranges(entry, tables: Sequence[Table], range_list, stream, *args):
    """One count entry over _range_list's tuple: entry(tables, nt, bounds,
    bound_off, nr, last_unbounded, *args, stream, first, second); the two
    uint64[nr] arrays it filled."""
    data, off, nr, last_unbounded = range_list
    arr, _ = _table_list(tables)
    first, second = np.zeros(max(nr, 1), np.uint64), np.zeros(max(nr, 1), np.uint64)
    _raise(entry(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, *args, _stream(stream),
                 _ptr_of(first)[0], _ptr_of(second)[0]))
    return first[:nr], second[:nr]


def count(tables: Sequence[Table], ranges=None, prefixes=None, stream=None):
    """Per range, how many entries scan_many(tables, ...) would return and how
    many of them are live rows, without building a result (cb_tables_count):
    (entries, live), two uint64 arrays. A value is dead when the reference's
    split_ts (src/query.rs:21-27) leaves no payload, the tombstone exec_delete
    writes (src/query.rs:240-261); a key whose newest decodable line is dead
    counts in entries and not in live, whatever older tables hold. SELECT
    COUNT(*) per namespace (src/query.rs:341-357) is live for
    prefixes=[ns + ":" for ns in sorted(names)]. Ranges as scan_many takes
    them; prefixes become ranges through prefix_end."""
    return _count_ranges(_L().cb_tables_count, tables, _range_list(ranges, prefixes), stream)


def scan_live(tables: Sequence[Table], ranges=None, prefixes=None, limit: int = 0, stream=None) -> ScanResult:
    """scan_many without the dead entries (cb_tables_scan_live): deleted rows
    (count's rule) are left out on the device, and range_off() counts live
    entries. A tombstone shadows before it is dropped: a key whose newest
    decodable line is dead is absent even when an older table holds a live
    value. limit > 0 takes exactly one range: the first `limit` live entries,
    ScanResult.truncated saying whether more live entries qualified."""
    return _scan_ranges(_L().cb_tables_scan_live, tables, ranges, prefixes, stream, int(limit))


def scan_lww(tables: Sequence[Table], ranges=None, prefixes=None, limit: int = 0, drop_dead: bool = False,
             stream=None) -> ScanResult:
    """scan_many under compact_lww's rule (cb_tables_scan_lww): every key's
    entry is its winner by timestamp, which() its table's index in `tables`
    and ts() its timestamp. drop_dead leaves out the winners that are
    tombstones. limit > 0 takes exactly one range, as in scan_live."""
    return _scan_ranges(_L().cb_tables_scan_lww, tables, ranges, prefixes, stream, int(bool(drop_dead)), int(limit))


def count_lww(tables: Sequence[Table], ranges=None, prefixes=None, stream=None):
    """count() under compact_lww's rule (cb_tables_count_lww): (entries, live),
    per range the winners and the winners that are not tombstones, i.e. the
    sizes of scan_lww's ranges with drop_dead False and True."""
    return _count_ranges(_L().cb_tables_count_lww, tables, _range_list(ranges, prefixes), stream)


def count_where(tables: Sequence[Table], where, key_columns=(), ranges=None, prefixes=None, skip=None,
                lww: bool = False, stream=None):
    """Per range, the live rows (count()'s live, or count_lww()'s with lww)
    and how many of them match `where`, without building a result
    (cb_tables_count_where): (live, matched), two uint64 arrays. `where` is a
    mapping or a list of (column, value), all ANDed; a column named in
    `key_columns` is compared with that `|`-separated part of the key after
    its first `skip` bytes, every other one with the row's JSON payload, the
    value after its 8-byte timestamp, parsed as the reference's decode_row
    parses it (src/schema.rs:42-44; any error: no columns). SELECT COUNT(*)
    FROM ns WHERE ... (src/query.rs:309-362) is prefixes=[ns + ":"], whose
    skip defaults to the prefix's length; with ranges it defaults to 0. skip
    may be one number or one per range."""
    range_list = _range_list(ranges, prefixes)
    w = _Where(where, key_columns)
    if skip is None:
        skip = [len(_key_bytes(p)) for p in prefixes] if prefixes is not None else 0
    sk = np.ascontiguousarray(_per_range(skip, range_list[2]) + [0], np.uint32)
    return _count_ranges(_L().cb_tables_count_where, tables, range_list, stream, _ptr_of(sk)[0], w.ref(),
                         int(bool(lww)))
