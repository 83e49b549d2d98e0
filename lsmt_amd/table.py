"""SSTable data files in HBM (src/sstable.rs:51-87, 133-179): ``Table``, the
flush (``sstable_create``) and the three compactions."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._ffi import (KeyBatch, _call_keys, _Handle, _host_bytes, _L, _ptr_of, _raise, _raise_text, _size_then_fill,
                   _stream, _to_var, as_batch)
from ._lib import check
from .bloom import BloomFilter
from .zone import ZoneMap


class Table(_Handle):
    """One SSTable data file (``key \t base64(value) \n`` lines, sorted;
    src/sstable.rs:57-72) resident in HBM with its line index, built on the
    device. ``data``: bytes, a uint8 numpy array, or a uint8 device tensor."""
    _destroy = "cb_table_destroy"

    def __init__(self, data, device: int = 0, stream=None):
        self._h = ctypes.c_void_p()
        buf, n = _host_bytes(data)
        ptr, keep = _ptr_of(buf)
        _raise(_L().cb_table_create(ptr, n, int(device), _stream(stream), ctypes.byref(self._h)))
        self.device = int(device)

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def wait(self) -> None:
        """Finalise a table from sstable_create(wait=False): wait for its
        enqueued work, take its results (raises its deferred error, if any)."""
        _raise(_L().cb_table_wait(self._h))
        self.__dict__.pop("_inputs", None)

    @property
    def nlines(self) -> int:
        n = ctypes.c_uint64()
        check(_L().cb_table_info(self._h, ctypes.byref(n), None))
        return int(n.value)

    @property
    def nbytes(self) -> int:
        n = ctypes.c_uint64()
        check(_L().cb_table_info(self._h, None, ctypes.byref(n)))
        return int(n.value)

    def data(self) -> bytes:
        """The data file's bytes (what storage.put writes, src/sstable.rs:73)."""
        n = self.nbytes
        out = np.zeros(max(n, 1), np.uint8)
        check(_L().cb_table_copy(self._h, 0, n, out.ctypes.data))
        return out[:n].tobytes()

    @classmethod
    def _adopt(cls, handle: int, device: int) -> "Table":
        t = cls.__new__(cls)
        t._h = ctypes.c_void_p(handle)
        t.device = device
        return t

    def _zone(self, which: int) -> bytes:
        """ZoneMap bound kept by cb_sstable_create: 0 = min, 1 = max (host copy)."""
        return _size_then_fill(lambda out, cap, n: check(_L().cb_table_zone(self._h, int(which), out, cap, n)))

    def rebuild(self, m: int = 1024, stream=None) -> "tuple[BloomFilter, ZoneMap]":
        """SsTable::load's rebuild from the data file when `.meta` is missing or
        undecodable (src/sstable.rs:109-120), on the device: (bloom, zone_map)
        over the keys of the lines that have a TAB. A key that is not UTF-8
        raises UnicodeDecodeError, as the reference's load returns Err."""
        h = ctypes.c_void_p()
        lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
        _raise_text(_L().cb_table_rebuild(self._h, int(m), _stream(stream), ctypes.byref(h), ctypes.byref(lo),
                                          ctypes.byref(hi)))
        z = ZoneMap()
        if lo.value != 0xFFFFFFFFFFFFFFFF:
            st, kl, _ = self.lines()
            raw = self.data()
            for li in (lo.value, hi.value):
                z.update(raw[int(st[li]):int(st[li]) + int(kl[li])])
        return BloomFilter(0, _handle=h.value), z

    @property
    def well_formed(self) -> bool:
        """A TAB on every line and strictly increasing keys (what SsTable::create
        writes): searched through the prefix/fence index."""
        v = ctypes.c_int()
        check(_L().cb_table_well_formed(self._h, ctypes.byref(v)))
        return bool(v.value)

    @staticmethod
    def force_exact(on: bool) -> None:
        """Tables created while on always replay the reference's exact
        (lo+hi)/2 search trajectory (tests / bench)."""
        check(_L().cb_table_force_exact(int(bool(on))))

    @staticmethod
    def bucket_limit(max_bytes: int) -> None:
        """The most device bytes one table's read-path key buckets may take
        (0: none for tables read from now on; default 1 GiB, and never over a
        quarter of the free device memory). Tables past it are searched
        without buckets: same answers, slower reads."""
        check(_L().cb_table_bucket_limit(int(max_bytes)))

    def lines(self):
        """(start uint64[n], key_len uint32[n] (0xFFFFFFFF = no TAB), line_len uint32[n])."""
        n = self.nlines
        st = np.zeros(max(n, 1), np.uint64)
        kl = np.zeros(max(n, 1), np.uint32)
        ll = np.zeros(max(n, 1), np.uint32)
        check(_L().cb_table_lines(self._h, st.ctypes.data, kl.ctypes.data, ll.ctypes.data))
        return st[:n], kl[:n], ll[:n]

    def search(self, keys, out=None, stream=None) -> np.ndarray:
        """SsTable::binary_search per key: int64 line index or -1."""
        b = as_batch(keys)
        if out is None:
            out = np.zeros(max(b.n, 1), np.int64)
            res = out[: b.n]
        else:
            res = out
        op, keep = _ptr_of(out)
        L = _L()
        _call_keys(L.cb_table_search_fixed, L.cb_table_search_var, (self._h,), b, (op, _stream(stream)))
        return res


def sstable_create(entries, m: int = 1024, device: int = 0, stream=None, wait: bool = True):
    """SsTable::create (src/sstable.rs:51-87) on the device. entries: a list of
    (key, value) pairs (str/bytes), or a (keys, values) pair of ragged
    KeyBatches. Returns (Table, BloomFilter of m bits, ZoneMap).

    The C call only enqueues (cb_sstable_create_bounded: device offsets are
    sized by their data buffers, no host round trip); the table finalises on
    first use. wait=False returns (Table, BloomFilter, None) without waiting
    for the zone bounds (Table.wait() or any read of the table finalises it);
    the key and value buffers must then stay alive until it has."""
    if isinstance(entries, tuple) and len(entries) == 2 and isinstance(entries[0], KeyBatch):
        kb, vb = entries
    else:
        kb = as_batch([k for k, _ in entries])
        vb = as_batch([v for _, v in entries])
    if not kb.is_var:
        kb = _to_var(kb)
    if not vb.is_var:
        vb = _to_var(vb)
    if kb.n != vb.n:
        raise ValueError("keys and values differ in count")
    th, fh = ctypes.c_void_p(), ctypes.c_void_p()
    kd, k1 = _ptr_of(kb.data)
    ko, k2 = _ptr_of(kb.offsets)
    vd, k3 = _ptr_of(vb.data)
    vo, k4 = _ptr_of(vb.offsets)

    def nbytes(x):
        return int(x.numel() * x.element_size()) if hasattr(x, "numel") else int(np.asarray(x).nbytes)
    if kb.n and hasattr(kb.offsets, "is_cuda") and kb.offsets.is_cuda:
        # device offsets: their data buffers bound the byte totals
        _raise(_L().cb_sstable_create_bounded(kd, ko, nbytes(kb.data), vd, vo, nbytes(vb.data), kb.n, int(m),
                                              int(device), _stream(stream), ctypes.byref(th), ctypes.byref(fh)))
    else:
        _raise(_L().cb_sstable_create(kd, ko, vd, vo, kb.n, int(m), int(device), _stream(stream), ctypes.byref(th),
                                      ctypes.byref(fh), None, None))
    table = Table._adopt(th.value, device)
    if not wait:
        table._inputs = (kb, vb)  # the enqueued work (and a fallback sort) reads them until finalised
    bloom = BloomFilter(0, device=device, _handle=fh.value)
    if not wait:
        return table, bloom, None
    zone = ZoneMap()
    if kb.n:
        zone = ZoneMap(table._zone(0), table._zone(1))
    return table, bloom, zone


def _table_list(tables: Sequence[Table]):
    if not tables:
        return None, 0
    return ctypes.cast((ctypes.c_void_p * len(tables))(*[t._h.value for t in tables]), ctypes.c_void_p), tables[0].device


def _adopt_compaction(th, fh, dev: int):
    """(Table, BloomFilter, ZoneMap) of the handles a compaction entry returned."""
    table = Table._adopt(th.value, dev)
    bloom = BloomFilter(0, device=dev, _handle=fh.value)
    zone = ZoneMap()
    if table.nlines:
        zone = ZoneMap(table._zone(0), table._zone(1))
    return table, bloom, zone


def _compact(entry, tables: Sequence[Table], stream, *args):
    """One compaction entry: entry(tables, nt, *args, stream, &table, &bloom)."""
    arr, dev = _table_list(tables)
    th, fh = ctypes.c_void_p(), ctypes.c_void_p()
    _raise(entry(arr, len(tables), *args, _stream(stream), ctypes.byref(th), ctypes.byref(fh)))
    return _adopt_compaction(th, fh, dev)


def compact(tables: Sequence[Table], m: int = 1024, stream=None):
    """Newest-wins merge of well-formed tables (tables[0] newest, as get_many
    takes them) into one, on the device (cb_tables_compact). The reference has
    no compaction; the result is SsTable::create (src/sstable.rs:51-87) of
    every key of the inputs with the value Database::get (src/lib.rs:128-134)
    returns for it over them: a key keeps its newest line whose value decodes,
    and a key whose value decodes nowhere is dropped. Returns (Table,
    BloomFilter of m bits, ZoneMap), as sstable_create does. The inputs are
    not modified and may be closed as soon as the call returns."""
    return _compact(_L().cb_tables_compact, tables, stream, int(m))


def compact_live(tables: Sequence[Table], m: int = 1024, stream=None):
    """compact() that also drops deleted rows (cb_tables_compact_live): the
    merged table holds every key whose newest decodable line is not a
    tombstone (count's rule), and the Bloom filter and zone map are of those
    keys. Correct only for a full compaction: with an older table of the store
    left out of `tables`, a dropped tombstone no longer shadows that table's
    line and the deleted row comes back. Returns (Table, BloomFilter, ZoneMap)
    as compact does."""
    return _compact(_L().cb_tables_compact_live, tables, stream, int(m))


def compact_lww(tables: Sequence[Table], m: int = 1024, drop_dead: bool = False, stream=None):
    """compact() with last-write-wins by row timestamp in place of newest-wins
    (cb_tables_compact_lww): table r stands for replica r, and a key keeps its
    decodable line with the greatest timestamp (the first 8 value bytes,
    big-endian; 0 below 8 bytes), the lowest table index among equal
    timestamps: the fold the reference's coordinator runs over its replicas'
    rows (src/cluster.rs:405-416). Use it where table order is not write
    order: tables of several replicas (repair, bootstrap), or forwarded writes
    that arrived out of order. A tombstone that loses to a row with a newer
    timestamp deletes nothing, whichever table is newer (compact_live would
    drop that row). drop_dead: winners that are tombstones are then left out
    (src/cluster.rs:454-459); correct only when no table or replica of the
    store stays outside `tables`. Returns (Table, BloomFilter, ZoneMap) as
    compact does."""
    return _compact(_L().cb_tables_compact_lww, tables, stream, int(m), int(bool(drop_dead)))
