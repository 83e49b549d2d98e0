"""Rows: the WHERE and SELECT structures of the C ABI (cb_where, cb_select),
a selection's result in device memory, and the one-row rules on the host
(src/query.rs:309-432, src/schema.rs:27-44)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._ffi import (KeyBatch, _Handle, _key_bytes, _key_parts, _L, _pack, _ptr_of, _raise, _size_then_fill, _stream,
                   as_batch)
from ._lib import check


class _CbWhere(ctypes.Structure):
    """cb_where (include/cassbloom.h)."""
    _fields_ = [("cols", ctypes.c_void_p), ("col_off", ctypes.c_void_p), ("vals", ctypes.c_void_p),
                ("val_off", ctypes.c_void_p), ("part", ctypes.c_void_p), ("nc", ctypes.c_uint32)]


def _text_buffer(joined: bytes):
    return ctypes.create_string_buffer(joined, max(len(joined), 1))


class _Where:
    """A cb_where built from a mapping or a list of (column, value), with
    `key_columns` (the schema's key_columns(), src/schema.rs:27-33) giving each
    condition its key part; keeps the arrays it points into alive."""

    def __init__(self, where, key_columns=()):
        pairs = list(where.items()) if hasattr(where, "items") else list(where)
        cols = [_key_bytes(c) for c, _ in pairs]
        joined, self.col_off = _pack(cols)
        self.cols = _text_buffer(joined)
        joined, self.val_off = _pack([_key_bytes(v) for _, v in pairs])
        self.vals = _text_buffer(joined)
        self.part = _key_parts(cols, key_columns)
        self.c = _CbWhere(ctypes.addressof(self.cols), self.col_off.ctypes.data, ctypes.addressof(self.vals),
                          self.val_off.ctypes.data, self.part.ctypes.data, len(pairs))

    def ref(self):
        return ctypes.addressof(self.c)


def _per_range(skip, nr: int) -> "list[int]":
    if isinstance(skip, (int, np.integer)):
        return [int(skip)] * nr
    skip = [int(x) for x in skip]
    if len(skip) != nr:
        raise ValueError("one skip per range")
    return skip


def row_matches(key, value, where, key_columns=(), skip: int = 0) -> bool:
    """count_where's rule for one row on the host (cb_row_matches; no device):
    e.g. a memtable row, which a store merges over the tables' answer."""
    k, v = _key_bytes(key), _key_bytes(value)
    w = _Where(where, key_columns)
    out = ctypes.c_int()
    check(_L().cb_row_matches(k, len(k), int(skip), v, len(v), w.ref(), ctypes.byref(out)))
    return bool(out.value)


class _CbSelect(ctypes.Structure):
    """cb_select (include/cassbloom.h)."""
    _fields_ = [("cols", ctypes.c_void_p), ("col_off", ctypes.c_void_p), ("part", ctypes.c_void_p),
                ("cast", ctypes.c_void_p), ("nc", ctypes.c_uint32)]


class _Select:
    """A cb_select built from column names in any order: sorted bytewise and
    de-duplicated (of a repeated name the last cast wins, as the reference's
    sel_map.insert does), `key_columns` giving each column its key part as in
    _Where. casts: None, a mapping name -> cast, or one cast per column; a
    cast is 0 / False (none) or 1 / True (integer). Keeps its arrays alive."""

    def __init__(self, columns, key_columns=(), casts=None):
        names = [_key_bytes(c) for c in columns]
        if casts is None:
            given = [0] * len(names)
        elif hasattr(casts, "items"):
            by_name = {_key_bytes(c): int(v) for c, v in casts.items()}
            given = [by_name.get(c, 0) for c in names]
        else:
            given = [int(v) for v in casts]
            if len(given) != len(names):
                raise ValueError("one cast per column")
        chosen = dict(zip(names, given))  # (a later pair replaces an earlier one)
        self.names = sorted(chosen)
        joined, self.col_off = _pack(self.names)
        self.cols = _text_buffer(joined)
        self.part = _key_parts(self.names, key_columns)
        self.cast = np.array([chosen[c] for c in self.names] + [0], np.int64)
        if ((self.cast < 0) | (self.cast > 255)).any():
            raise ValueError("a cast is 0 or 1")
        self.cast = self.cast.astype(np.uint8)
        self.c = _CbSelect(ctypes.addressof(self.cols), self.col_off.ctypes.data, self.part.ctypes.data,
                           self.cast.ctypes.data, len(self.names))

    def ref(self):
        return ctypes.addressof(self.c)


class RowsResult(_Handle):
    """A selection's response in device memory (cb_rows_*): the bytes the
    reference's exec_select_schema returns (src/query.rs:365-432) and, per row,
    where its text lies in them and its flags (_lib.ROW_*). Complete when the
    call that made it returns."""
    _destroy = "cb_rows_destroy"

    def __init__(self, handle: int, device: int):
        self._h = ctypes.c_void_p(handle)
        self.device = device
        n, wt, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(_L().cb_rows_info(self._h, ctypes.byref(n), ctypes.byref(wt), ctypes.byref(nb)))
        self.count, self.with_text, self.bytes = int(n.value), int(wt.value), int(nb.value)

    def __len__(self) -> int:
        return self.count

    def copy(self, text=None, row_at=None, row_len=None, flags=None) -> None:
        """Any of text (uint8[bytes]), row_at, row_len (uint64[count]) and
        flags (uint8[count]) into numpy arrays or device tensors."""
        check(_L().cb_rows_text(self._h, _ptr_of(text)[0], _ptr_of(row_at)[0], _ptr_of(row_len)[0],
                                _ptr_of(flags)[0]))

    def text(self) -> bytes:
        """The response: a JSON array, or with meta the `key \\t ts \\t val`
        lines (empty without any: the reference's Ok(None))."""
        t = np.zeros(max(self.bytes, 1), np.uint8)
        self.copy(text=t)
        return t[:self.bytes].tobytes()

    def spans(self):
        """(row_at, row_len): uint64[count] each; row_len is 0 without text."""
        at, ln = np.zeros(max(self.count, 1), np.uint64), np.zeros(max(self.count, 1), np.uint64)
        self.copy(row_at=at, row_len=ln)
        return at[:self.count], ln[:self.count]

    def rows(self) -> "list[bytes]":
        """Every row's own text, b"" where it has none."""
        raw = self.text()
        at, ln = self.spans()
        return [raw[a:a + n] for a, n in zip(at.tolist(), ln.tolist())]

    def flags(self) -> np.ndarray:
        f = np.zeros(max(self.count, 1), np.uint8)
        self.copy(flags=f)
        return f[:self.count]


def _on_device(x, dtype, device: int):
    """x as a contiguous device tensor (a host array is copied there)."""
    import torch
    if hasattr(x, "data_ptr"):
        if x.numel() == 0:  # (no storage: the C ABI takes no NULL array beside a count)
            return torch.zeros(1, dtype=x.dtype, device=f"cuda:{device}")
        return x if x.is_cuda else x.to(f"cuda:{device}")
    a = np.ascontiguousarray(x, dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    if not a.flags.writeable:
        a = a.copy()  # (torch takes no read-only array)
    if dtype == np.uint64:  # (torch has no arithmetic on uint64, but it moves the bytes)
        return torch.from_numpy(a.view(np.int64)).to(f"cuda:{device}")
    return torch.from_numpy(a).to(f"cuda:{device}")


def select_rows(keys, which, val_off, vals, columns, key_columns=(), casts=None, skip=0, meta=False, device=None,
                stream=None) -> RowsResult:
    """ScanResult.select over rows that a get left in device memory
    (cb_rows_select): keys as get_many takes them, and the which, val_off and
    vals it wrote, e.g. with wait=False on the same stream; which=None: every
    row is present. Host arrays are copied to the device first. The work is
    enqueued on stream; the call returns a finished result."""
    b = as_batch(keys)
    if not b.is_var:
        data = b.keys.reshape(-1) if b.n and b.key_len else np.zeros(1, np.uint8)
        b = KeyBatch(n=b.n, data=data, offsets=np.arange(b.n + 1, dtype=np.uint64) * np.uint64(b.key_len))
    if device is None:
        device = next((int(x.device.index or 0) for x in (vals, val_off, b.data) if hasattr(x, "data_ptr") and
                       x.is_cuda), 0)
    q = _Select(columns, key_columns, casts)
    h = ctypes.c_void_p()
    if b.n == 0:
        _raise(_L().cb_rows_select(None, None, None, None, None, 0, int(skip), q.ref(), int(bool(meta)), int(device),
                                   _stream(stream), ctypes.byref(h)))
        return RowsResult(h.value, int(device))
    kd, ko = _on_device(b.data, np.uint8, device), _on_device(b.offsets, np.uint64, device)
    wh = None if which is None else _on_device(which, np.int32, device)
    vo, vd = _on_device(val_off, np.uint64, device), _on_device(vals, np.uint8, device)
    _raise(_L().cb_rows_select(_ptr_of(kd)[0], _ptr_of(ko)[0], _ptr_of(wh)[0], _ptr_of(vd)[0], _ptr_of(vo)[0], b.n,
                               int(skip), q.ref(), int(bool(meta)), int(device), _stream(stream), ctypes.byref(h)))
    return RowsResult(h.value, int(device))


def row_select(key, value, columns, key_columns=(), casts=None, skip=0, meta=False):
    """The selection's rule for one row on the host (cb_row_select; no
    device), e.g. a memtable row: (text, flags), text None when the row has
    none (a deleted row without meta)."""
    k, v = _key_bytes(key), _key_bytes(value)
    q = _Select(columns, key_columns, casts)
    f = ctypes.c_uint8()
    text = _size_then_fill(
        lambda out, cap, n: check(_L().cb_row_select(k, len(k), int(skip), v, len(v), q.ref(), int(bool(meta)), out,
                                                     cap, n, ctypes.byref(f))),
        wanted=lambda: f.value & _lib.ROW_TEXT)
    return text, int(f.value)
