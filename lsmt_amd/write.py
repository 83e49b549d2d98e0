"""Writes: a batch of INSERT, UPDATE or DELETE rows turned into the store's
keys, values and log records on the device (cb_rows_write; src/query.rs:162-261,
716-731, src/schema.rs:37-39, src/lib.rs:96-116, 154-157), the result in device
memory, and the one-row rule on the host (cb_row_write). Reached as
``lsmt_amd.write``."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._ffi import _Handle, _key_bytes, _L, _pack, _ptr_of, _raise, _raise_text, _stream
from ._lib import (WRITE_DELETE, WRITE_INSERT, WRITE_UPDATE, WRITTEN_BADOLD, WRITTEN_HOST,  # noqa: F401
                   WRITTEN_KEYCTL, check)
from .bloom import BloomFilter
from .rows import _on_device, _text_buffer
from .table import Table, _adopt_compaction
from .zone import ZoneMap

INSERT, UPDATE, DELETE = WRITE_INSERT, WRITE_UPDATE, WRITE_DELETE
_OPS = {"insert": INSERT, "update": UPDATE, "delete": DELETE}


class _CbWrite(ctypes.Structure):
    """cb_write (include/cassbloom.h)."""
    _fields_ = [("ns", ctypes.c_void_p), ("ns_len", ctypes.c_uint64), ("nk", ctypes.c_uint32),
                ("cols", ctypes.c_void_p), ("col_off", ctypes.c_void_p), ("set", ctypes.c_void_p),
                ("nc", ctypes.c_uint32), ("op", ctypes.c_int)]


class _Write:
    """A cb_write built from the statement's parts: `columns` are the payload
    columns the statement sets, in the caller's order (the order of a row's
    cells behind its nk key cells), `keep` the ones an UPDATE takes from the old
    row. The names are sorted bytewise, as the C ABI wants them; `order` says
    where each sorted set column's cell stands in the caller's row. Keeps its
    arrays alive."""

    def __init__(self, ns, nk: int, columns=(), keep=(), op=INSERT):
        self.op = _OPS[op.lower()] if isinstance(op, str) else int(op)
        given = [_key_bytes(c) for c in columns]
        kept = [_key_bytes(c) for c in keep]
        if len(set(given)) != len(given) or len(set(kept)) != len(kept) or set(given) & set(kept):
            raise ValueError("a column is named twice")
        self.names = sorted(given + kept)
        self.nk = int(nk)
        self.order = [self.nk + given.index(c) for c in self.names if c in given]
        self.width = self.nk + len(given)
        self.ns = _text_buffer(_key_bytes(ns))
        joined, self.col_off = _pack(self.names)
        self.cols = _text_buffer(joined)
        self.set = np.array([c in given for c in self.names] + [0], np.uint8)
        self.c = _CbWrite(ctypes.addressof(self.ns), len(_key_bytes(ns)), self.nk, ctypes.addressof(self.cols),
                          self.col_off.ctypes.data, self.set.ctypes.data, len(self.names), self.op)

    def ref(self):
        return ctypes.addressof(self.c)

    def row_cells(self, row) -> "list[bytes]":
        """A caller's row (key cells, then `columns`' cells) in the ABI's order."""
        cells = [_key_bytes(x) for x in row]
        if len(cells) != self.width:
            raise ValueError("a row has %d cells, the statement %d" % (len(cells), self.width))
        return cells[:self.nk] + [cells[j] for j in self.order]


def _split(raw: bytes, off: np.ndarray) -> "list[bytes]":
    o = off.tolist()
    return [raw[a:b] for a, b in zip(o[:-1], o[1:])]


class Written(_Handle):
    """A written batch in device memory (cb_written_*): per row the key, the
    value (timestamp + payload) and the log record, with its flags
    (_lib.WRITTEN_*). Complete when the call that made it returns."""
    _destroy = "cb_written_destroy"

    def __init__(self, handle: int, device: int):
        self._h = ctypes.c_void_p(handle)
        self.device = device
        v = [ctypes.c_uint64() for _ in range(5)]
        check(_L().cb_written_info(self._h, *[ctypes.byref(x) for x in v]))
        self.count, self.key_bytes, self.val_bytes, self.log_bytes, self.flagged = [int(x.value) for x in v]

    def __len__(self) -> int:
        return self.count

    def copy(self, keys=None, key_off=None, vals=None, val_off=None, log=None, log_off=None, flags=None) -> None:
        """Any of the arrays into numpy arrays or device tensors: keys, vals,
        log (uint8[*_bytes]), the offsets (uint64[count + 1]), flags
        (uint8[count])."""
        check(_L().cb_written_copy(self._h, *[_ptr_of(x)[0] for x in (keys, key_off, vals, val_off, log, log_off,
                                                                      flags)]))

    def _ragged(self, which: str, nbytes: int) -> "list[bytes]":
        raw, off = np.zeros(max(nbytes, 1), np.uint8), np.zeros(self.count + 1, np.uint64)
        self.copy(**{which: raw, which[:-1] + "_off" if which != "log" else "log_off": off})
        return _split(raw[:nbytes].tobytes(), off)

    def keys(self) -> "list[bytes]":
        return self._ragged("keys", self.key_bytes)

    def values(self) -> "list[bytes]":
        """Every row's value, b"" for a row flagged WRITTEN_HOST."""
        return self._ragged("vals", self.val_bytes)

    def records(self) -> "list[bytes]":
        """Every row's log record, b"" for a row flagged WRITTEN_HOST."""
        return self._ragged("log", self.log_bytes)

    def log(self) -> bytes:
        """The records in row order: what insert_internal appends to the log."""
        raw = np.zeros(max(self.log_bytes, 1), np.uint8)
        self.copy(log=raw)
        return raw[:self.log_bytes].tobytes()

    def flags(self) -> np.ndarray:
        f = np.zeros(max(self.count, 1), np.uint8)
        self.copy(flags=f)
        return f[:self.count]

    def arrays(self) -> dict:
        """The device addresses of keys, key_off, vals, val_off, log, log_off
        and flags (0 all for a batch of no rows), valid until close()."""
        p = [ctypes.c_void_p() for _ in range(7)]
        check(_L().cb_written_arrays(self._h, *[ctypes.byref(x) for x in p]))
        return dict(zip(("keys", "key_off", "vals", "val_off", "log", "log_off", "flags"),
                        [int(x.value or 0) for x in p]))

    def _no_host_rows(self) -> None:
        if self.flagged and (self.flags() & WRITTEN_HOST).any():
            raise ValueError("rows flagged WRITTEN_HOST have no value: write them on the host first")

    def to_table(self, m: int = 1024, stream=None, wait: bool = True):
        """SsTable::create of the batch from its device arrays
        (cb_sstable_create): (Table, BloomFilter of m bits, ZoneMap). The table
        keeps this batch alive until it is finalised; with wait=False the zone
        map is None, as sstable_create returns it."""
        self._no_host_rows()
        a = self.arrays()
        th, fh = ctypes.c_void_p(), ctypes.c_void_p()
        _raise(_L().cb_sstable_create(a["keys"] or None, a["key_off"] or None, a["vals"] or None, a["val_off"] or None,
                                      self.count, int(m), int(self.device), _stream(stream), ctypes.byref(th),
                                      ctypes.byref(fh), None, None))
        table = Table._adopt(th.value, self.device)
        table._inputs = self  # (device inputs must outlive the enqueued work: Table.wait() drops this)
        bloom = BloomFilter(0, device=self.device, _handle=fh.value)
        if not wait:
            return table, bloom, None
        table.wait()
        return table, bloom, (ZoneMap(table._zone(0), table._zone(1)) if self.count else ZoneMap())

    def replay(self, m: int = 1024, stream=None):
        """replay_log of the batch's log where it lies (cb_log_replay):
        (Table, BloomFilter, ZoneMap or None, LogStats)."""
        self._no_host_rows()
        th, fh, st = ctypes.c_void_p(), ctypes.c_void_p(), _lib.LogStats()
        _raise_text(_L().cb_log_replay(self.arrays()["log"] or None, self.log_bytes, int(m), int(self.device),
                                       _stream(stream), ctypes.byref(th), ctypes.byref(fh), ctypes.byref(st)), stats=st)
        table, bloom, zone = _adopt_compaction(th, fh, int(self.device))
        return table, bloom, (zone if table.nlines else None), st


def _cells(w: _Write, rows):
    """(data, offsets, n) of the caller's rows: a (data, offsets) pair of
    arrays or tensors already in the ABI's order, or a list of rows."""
    if isinstance(rows, tuple) and len(rows) == 2 and not isinstance(rows[0], (bytes, str, list, tuple)):
        data, off = rows
        nof = int(off.numel()) if hasattr(off, "numel") else int(len(off))
        if w.order != list(range(w.nk, w.width)):
            raise ValueError("packed cells need the set columns in ascending name order")
        if w.width == 0 or (nof - 1) % w.width:
            raise ValueError("the offsets do not hold whole rows")
        return data, off, (nof - 1) // w.width
    flat = [c for row in rows for c in w.row_cells(row)]
    joined, off = _pack(flat)
    return np.frombuffer(joined or b"\0", np.uint8), off, len(rows)


def write_rows(ns, rows, nk: int, columns=(), keep=(), op=INSERT, ts=0, old=None, device=None, stream=None) -> Written:
    """The keys, values and log records of one statement's rows on the device
    (cb_rows_write). ns: the namespace; rows: a list of rows, each nk key cells
    (INSERT: in the statement's column order; UPDATE, DELETE: in the schema's
    key_columns() order) followed by one cell per name in `columns`, or a
    (data, offsets) pair of arrays or device tensors holding the same cells
    row-major (then `columns` must ascend); keep: the payload columns an UPDATE
    takes from the old row; op: INSERT, UPDATE, DELETE or their names; ts: one
    timestamp, or one per row (array or device tensor); old: None or (which,
    val_off, vals) as get_many wrote them, e.g. with wait=False on the same
    stream (host arrays are copied to the device). A DELETE's rows are key
    cells only. Returns a finished Written."""
    w = _Write(ns, nk, columns, keep, op)
    if w.width == 0:
        n = int(rows) if isinstance(rows, (int, np.integer)) else len(rows)
        data, off = None, None
    else:
        data, off, n = _cells(w, rows)
    if device is None:
        device = next((int(x.device.index or 0) for x in (data, off) + tuple(old or ()) if hasattr(x, "is_cuda") and
                       x.is_cuda), 0)
    if isinstance(ts, (int, np.integer)):
        ts_arr, ts_all = None, int(ts)
    else:
        ts_arr, ts_all = (ts if hasattr(ts, "data_ptr") else np.ascontiguousarray(ts, np.uint64)), 0
        if (int(ts_arr.numel()) if hasattr(ts_arr, "numel") else len(ts_arr)) != n:
            raise ValueError("one timestamp per row")
    h = ctypes.c_void_p()
    if n == 0:
        _raise(_L().cb_rows_write(w.ref(), None, None, None, ts_all, None, None, None, 0, int(device), _stream(stream),
                                  ctypes.byref(h)))
        return Written(h.value, int(device))
    wh = vo = vd = None
    if old is not None:
        which, val_off, vals = old
        wh, vo, vd = (_on_device(which, np.int32, device), _on_device(val_off, np.uint64, device),
                      _on_device(vals, np.uint8, device))
    _raise(_L().cb_rows_write(w.ref(), _ptr_of(data)[0], _ptr_of(off)[0], _ptr_of(ts_arr)[0], ts_all, _ptr_of(wh)[0],
                              _ptr_of(vd)[0], _ptr_of(vo)[0], n, int(device), _stream(stream), ctypes.byref(h)))
    return Written(h.value, int(device))


def row_write(ns, row, nk: int, columns=(), keep=(), op=INSERT, ts: int = 0, old=None):
    """The rule for one row on the host (cb_row_write; no device), e.g. a write
    into the memtable: (key, value, record, flags); value and record are None
    for a row flagged WRITTEN_HOST. old: the old value's bytes, or None."""
    w = _Write(ns, nk, columns, keep, op)
    cells = w.row_cells(row)
    joined, off = _pack(cells)
    data = _text_buffer(joined)
    ov = None if old is None else _key_bytes(old)
    kl, vl, rl, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint8()

    def call(out, cap):
        check(_L().cb_row_write(w.ref(), ctypes.addressof(data), off.ctypes.data, int(ts), ov, len(ov or b""),
                                int(ov is not None), out, cap, ctypes.byref(kl), ctypes.byref(vl), ctypes.byref(rl),
                                ctypes.byref(f)))
    call(None, 0)
    total = kl.value + vl.value + rl.value
    out = ctypes.create_string_buffer(max(total, 1))
    call(out, total)
    raw, k, v = out.raw, kl.value, vl.value
    if f.value & WRITTEN_HOST:
        return raw[:k], None, None, int(f.value)
    return raw[:k], raw[k:k + v], raw[k + v:total], int(f.value)
