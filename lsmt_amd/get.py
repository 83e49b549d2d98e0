"""The batched read path: Database::get's newest-first walk over SSTables
for a key batch (src/lib.rs:128-134), gated by hit rows, by a FilterSet or by
tiered sets inside the search kernel."""
from __future__ import annotations

import ctypes
import operator
from typing import Sequence

import numpy as np

from ._ffi import _call_keys, _L, _ptr_of, _stream, as_batch
from .filterset import FilterSet, _tier_args
from .table import Table

_TABLE_ARRAYS: dict = {}  # id(sequence) -> (the tables' handle objects, their C array)
_HANDLE = operator.attrgetter("_h")


def _table_array(tables: Sequence[Table]):
    """The tables' handles as one C array, kept per sequence object while it
    holds the same open tables in the same order. A store passes its table
    list batch after batch (Database::get walks self.sstables, src/lib.rs:
    129-134), and converting 300 handles into a fresh ctypes array took ~70 us
    of host time per call, more than half the wide fan-out's device step.
    The check is one identity test per table against the handle objects
    stored here: Table.close() replaces a table's handle object, so a closed
    or different table never reuses a stored array (and holding the handle
    objects keeps no table alive)."""
    hs = list(map(_HANDLE, tables))
    hit = _TABLE_ARRAYS.get(id(tables))
    if hit is not None and hit[0] == hs:  # (ctypes handles compare by identity)
        return hit[1]
    arr = (ctypes.c_void_p * max(len(hs), 1))(*[h.value for h in hs])
    if len(_TABLE_ARRAYS) >= 8:
        _TABLE_ARRAYS.clear()  # (one call, so safe against another thread's insert)
    _TABLE_ARRAYS[id(tables)] = (hs, arr)
    return arr


def get_many(tables: Sequence[Table], keys, hits=None, hit_rows=None, stream=None, out=None, wait=True,
             filterset=None):
    """Database::get's newest-first walk for a key batch (tables[0] newest).
    hits: optional per-table gate bitmaps (e.g. FilterSet.probe(gated=True));
    table t uses row hit_rows[t] (default t). Returns (which int32[n]: table
    index or -1, val_off uint64[n+1], vals bytes).

    out=(which, val_off, vals) with preallocated (e.g. device) buffers runs
    one pass and returns (which, val_off, total); values are written only if
    vals is large enough for total. With wait=False (out, keys and hits on the
    device) the call only enqueues the work on stream and returns total None:
    val_off[n] holds it once the stream has run.

    filterset=FilterSet: Database::get in one launch (cb_set_get_many_*): each
    table's gate (its slot's ZoneMap and Bloom bits, as
    FilterSet.probe(gated=True)) is computed inside the search kernel, so no
    hit rows exist; hit_rows then names each table's slot (default t) and
    hits must be None. At most the set's width tables (a wide set: up to 4096
    in one launch)."""
    if filterset is not None and hits is not None:
        raise ValueError("filterset= computes the gate itself: pass hits=None")
    nt = len(tables)
    arr = ctypes.cast(_table_array(tables), ctypes.c_void_p)
    hp, hk = _ptr_of(hits) if hits is not None else (None, None)
    rows = None
    if hit_rows is not None:
        rows = np.ascontiguousarray(hit_rows, dtype=np.uint32)
    rp = rows.ctypes.data if rows is not None else None
    L = _L()
    if filterset is not None:
        return _get_many_run(L.cb_set_get_many_fixed, L.cb_set_get_many_var, (filterset._h, arr, nt, rp),
                             keys, stream, out, wait)
    return _get_many_run(L.cb_get_many_fixed, L.cb_get_many_var, (arr, nt, hp, rp), keys, stream, out, wait)


def _get_many_run(fixed_fn, var_fn, head, keys, stream, out, wait):
    """The cb_*get_many_* families share their argument tail (keys, n, which,
    val_off, vals, cap, total, stream) and their return forms (get_many's
    docstring); head holds the arguments before the keys."""
    b = as_batch(keys)
    total = ctypes.c_uint64()
    if not wait and out is None:
        raise ValueError("wait=False needs out= device buffers")
    tref = ctypes.byref(total) if wait else None
    s = _stream(stream)
    if out is not None:
        which, voff, vals = out
        cap = int(vals.numel()) if hasattr(vals, "numel") else int(vals.nbytes)
    else:
        which = np.zeros(max(b.n, 1), np.int32)
        voff = np.zeros(b.n + 1, np.uint64)
    wp, k3 = _ptr_of(which)
    vo, k4 = _ptr_of(voff)

    def call(vp, cap):
        _call_keys(fixed_fn, var_fn, head, b, (wp, vo, vp, cap, tref, s))
    if out is not None:
        call(_ptr_of(vals)[0], cap)
        return which, voff, (int(total.value) if wait else None)
    call(None, 0)
    vals = np.zeros(max(int(total.value), 1), np.uint8)
    call(vals.ctypes.data, int(total.value))
    return which[: b.n], voff, vals[: int(total.value)].tobytes()


def get_many_tiers(tables: Sequence[Table], sets: Sequence[FilterSet], tiers, slots, keys, stream=None, out=None,
                   wait=True):
    """Database::get in one launch over tiered filter sets
    (cb_tiers_get_many_*): get_many's walk with table t's gate taken from
    slot slots[t] of sets[tiers[t]] inside the search kernel, the key hashed
    once for every tier. The store after a compaction: a large table behind
    a large filter and fresh tables behind m = 1024 ones. Same return forms as
    get_many (out=, wait=)."""
    arr, ns, t, sl = _tier_args(sets, tiers, slots)
    if len(tables) != int(t.shape[0]):
        raise ValueError("tiers and slots need one entry per table")
    L = _L()
    head = (ctypes.cast(arr, ctypes.c_void_p), ns, ctypes.cast(_table_array(tables), ctypes.c_void_p), len(tables),
            t.ctypes.data, sl.ctypes.data)
    return _get_many_run(L.cb_tiers_get_many_fixed, L.cb_tiers_get_many_var, head, keys, stream, out, wait)
