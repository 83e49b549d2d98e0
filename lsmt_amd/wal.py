"""The write-ahead log (src/wal.rs:14-31, src/lib.rs:30-39, 96-102): its
writer on the host and its replay to a table on the device."""
from __future__ import annotations

import ctypes

from . import _lib
from ._ffi import _host_bytes, _key_bytes, _L, _ptr_of, _raise, _raise_text, _stream
from .table import _adopt_compaction

LogStats = _lib.LogStats


def wal_bytes(entries) -> bytes:
    """The log insert_internal writes for [(key, value)] (src/lib.rs:96-102 and
    Wal::append, src/wal.rs:63-72): ``key \t STANDARD.encode(value) \n`` per
    entry, in order. Host only: the writer the tests and tools replay."""
    import base64
    return b"".join(_key_bytes(k) + b"\t" + base64.b64encode(_key_bytes(v)) + b"\n" for k, v in entries)


def log_line(piece):
    """The verdict of one piece of a log (cb_log_line; parse_entries' loop body,
    src/wal.rs:17-28), on the host: (kind, key_len, value_len) with kind 0 for a
    skipped piece (no TAB), 1 for an entry, CB_EUTF8 or CB_EBASE64 for the
    error the piece is; the lengths are the key's and the decoded value's."""
    piece = bytes(piece)
    kind, kl, vl = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    _raise(_L().cb_log_line(piece, len(piece), ctypes.byref(kind), ctypes.byref(kl), ctypes.byref(vl)))
    return int(kind.value), int(kl.value), int(vl.value)


def replay_log(log, m: int = 1024, device: int = 0, stream=None):
    """Database::new's replay of the write-ahead log followed by the flush of
    the replayed memtable (src/lib.rs:30-39, src/sstable.rs:51-87), on the
    device (cb_log_replay): one line per distinct key holding its LAST record,
    sorted by key. ``log``: bytes, a uint8 numpy array or a uint8 device
    tensor. Returns (Table, BloomFilter of m bits, ZoneMap or None for a log
    without an entry, LogStats). A key that is not UTF-8 raises
    UnicodeDecodeError as Table.rebuild does, a value that is not STANDARD
    base64 ValueError, both with the bad line in the message and the call's
    LogStats as ``.stats``: Wal::new returns Err (src/wal.rs:21-26)."""
    buf, n = _host_bytes(log)
    ptr, keep = _ptr_of(buf)
    th, fh, st = ctypes.c_void_p(), ctypes.c_void_p(), LogStats()
    _raise_text(_L().cb_log_replay(ptr, n, int(m), int(device), _stream(stream), ctypes.byref(th), ctypes.byref(fh),
                                   ctypes.byref(st)), stats=st)
    table, bloom, zone = _adopt_compaction(th, fh, int(device))
    return table, bloom, (zone if table.nlines else None), st
