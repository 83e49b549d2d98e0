"""Bit-sliced filter sets for the read-path fan-out (Database::get,
src/lib.rs:129-134): ``FilterSet``, and the tiered probe over several sets of
different filter sizes."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._ffi import _call_keys, _Handle, _hit_rows, _host_bytes, _L, _ptr_of, _raise, _stream, as_batch
from ._lib import check
from .bloom import BloomFilter
from .zone import ZoneMap, _bound


def set_dense(mode: int) -> None:
    """FilterSet probes of dense batches: 0 by density (default), 1 the
    region-partitioned probe whenever the set allows it, -1 never
    (cb_set_dense; last_path() is 6 after a dense probe)."""
    check(_L().cb_set_dense(int(mode)))


class FilterSet(_Handle):
    """Up to ``width`` filters of one size m, bit-sliced in HBM for the
    read-path fan-out (Database::get, src/lib.rs:129-134): one probe call
    answers may_contain for every slot with two word (or row) reads per key.
    width 32 or 64, or a wide set of any multiple of 64 up to 4096 slots
    (rows of width/64 uint64 words: the reference's real shape of hundreds of
    m = 1024 tables, src/sstable.rs:44,59, src/lib.rs:72,105). A derived copy —
    the BloomFilter handles remain the source of truth."""
    _destroy = "cb_set_destroy"

    def __init__(self, m: int, width: int = 32, device: int = 0):
        self._h = ctypes.c_void_p()
        _raise(_L().cb_set_create(int(m), int(width), int(device), ctypes.byref(self._h)))
        self.m, self.width, self.device = int(m), int(width), int(device)

    @classmethod
    def from_filters(cls, filters: Sequence[BloomFilter], width: int | None = None,
                     stream=None) -> "FilterSet":
        if not filters:
            raise ValueError("need at least one filter")
        width = width or (32 if len(filters) <= 32 else 64 if len(filters) <= 64 else
                          (len(filters) + 63) // 64 * 64)
        s = cls(filters[0].m, width, device=filters[0].device)
        s.assign_all(filters, stream=stream)
        return s

    @property
    def used(self) -> int:
        u = ctypes.c_uint32()
        check(_L().cb_set_info(self._h, None, None, ctypes.byref(u)))
        return int(u.value)

    def assign(self, slot: int, f: BloomFilter, stream=None) -> None:
        f.flush(stream)
        _raise(_L().cb_set_assign(self._h, int(slot), f.handle, _stream(stream)))

    def assign_all(self, filters: Sequence[BloomFilter], stream=None) -> None:
        for f in filters:
            f.flush(stream)
        arr = (ctypes.c_void_p * max(len(filters), 1))(*[f.handle.value for f in filters])
        _raise(_L().cb_set_assign_all(self._h, ctypes.cast(arr, ctypes.c_void_p), len(filters),
                                      _stream(stream)))

    def clear_slot(self, slot: int, stream=None) -> None:
        _raise(_L().cb_set_clear_slot(self._h, int(slot), _stream(stream)))

    def set_zone(self, slot: int, zone: "ZoneMap | tuple", stream=None) -> None:
        """Slot's zone map := zone (ZoneMap or (min, max) bytes/str/None)."""
        lo, hi = map(_bound, (zone.min, zone.max) if isinstance(zone, ZoneMap) else zone)
        lb = np.frombuffer(lo, np.uint8) if lo else np.zeros(1, np.uint8)
        hb = np.frombuffer(hi, np.uint8) if hi else np.zeros(1, np.uint8)
        _raise(_L().cb_set_zone(self._h, int(slot), lb.ctypes.data_as(ctypes.c_void_p), len(lo or b""),
                                lo is not None, hb.ctypes.data_as(ctypes.c_void_p), len(hi or b""),
                                hi is not None, _stream(stream)))

    def zone(self, slot: int) -> ZoneMap:
        ll, hl = ctypes.c_uint64(), ctypes.c_uint64()
        hasl, hash_ = ctypes.c_int(), ctypes.c_int()
        check(_L().cb_set_zone_get(self._h, int(slot), None, 0, ctypes.byref(ll), ctypes.byref(hasl), None, 0,
                                   ctypes.byref(hl), ctypes.byref(hash_)))
        lb = np.zeros(max(ll.value, 1), np.uint8)
        hb = np.zeros(max(hl.value, 1), np.uint8)
        check(_L().cb_set_zone_get(self._h, int(slot), lb.ctypes.data_as(ctypes.c_void_p), lb.size, ctypes.byref(ll),
                                   ctypes.byref(hasl), hb.ctypes.data_as(ctypes.c_void_p), hb.size,
                                   ctypes.byref(hl), ctypes.byref(hash_)))
        return ZoneMap(lb[: ll.value].tobytes() if hasl.value else None,
                       hb[: hl.value].tobytes() if hash_.value else None)

    def load_meta(self, slot: int, data: bytes, stream=None) -> None:
        """Decode one table's ``.meta`` (TableMeta) straight into ``slot``:
        filter bits and zone map (the restart path, src/sstable.rs:96-108)."""
        buf, n = _host_bytes(data)
        _raise(_L().cb_set_load_meta(self._h, int(slot), buf.ctypes.data, n, _stream(stream)))

    def zone_from_keys(self, slot: int, keys, stream=None) -> None:
        """ZoneMap::update over a key batch, on the device (src/sstable.rs:62-65)."""
        L = _L()
        _call_keys(L.cb_set_zone_from_keys_fixed, L.cb_set_zone_from_keys_var, (self._h, int(slot)), as_batch(keys),
                   (_stream(stream),))

    def probe_pack(self, keys, hits, pack, cap: int, gated: bool = False, stream=None) -> None:
        """The probe writing the exchange pack too (cb_set_probe_pack_fixed):
        keys uint8[n, key_len], hits int64[used][ceil(n/64)] and pack int32
        [pack_words(n, cap)], all device tensors."""
        n = int(keys.shape[0])
        kp, k1 = _ptr_of(keys)
        hp, k2 = _ptr_of(hits)
        pp, k3 = _ptr_of(pack)
        _raise(_L().cb_set_probe_pack_fixed(self._h, kp, int(keys.shape[1]), n, int(bool(gated)), hp, pp, int(cap),
                                            _stream(stream)))

    @staticmethod
    def pack_words(n: int, cap: int) -> int:
        out = ctypes.c_uint64()
        check(_L().cb_set_pack_words(int(n), int(cap), ctypes.byref(out)))
        return int(out.value)

    def probe(self, keys, out=None, stream=None, gated: bool = False) -> np.ndarray:
        """uint64[used, ceil(n/64)]: row s = slot s's may_contain bits; with
        gated=True, SsTable::get's full gate zone.contains && may_contain
        (src/sstable.rs:138)."""
        b = as_batch(keys)
        out, result = _hit_rows(self.used, b.n, out)
        op, keep = _ptr_of(out)
        L = _L()
        if gated:
            _call_keys(L.cb_set_probe_gated_fixed, L.cb_set_probe_gated_var, (self._h,), b, (op, _stream(stream)))
        else:
            _call_keys(L.cb_set_probe_fixed, L.cb_set_probe_var, (self._h,), b, (op, _stream(stream)))
        return result


def _tier_args(sets: Sequence[FilterSet], tiers, slots):
    """(set handle array, ns, tiers uint32[nt], slots uint32[nt]) of a tiered call."""
    hs = [st._h.value for st in sets]
    arr = (ctypes.c_void_p * max(len(hs), 1))(*hs)
    t = np.ascontiguousarray(tiers, dtype=np.uint32)
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    if t.ndim != 1 or t.shape != sl.shape:
        raise ValueError("tiers and slots are parallel 1-d arrays, one entry per table")
    return arr, len(hs), t, sl


def probe_tiers(sets: Sequence[FilterSet], tiers, slots, keys, gated: bool = True, out=None, stream=None):
    """The gate rows of an ordered table list whose filters live in several
    FilterSets of different m (cb_tiers_probe_*): table t's filter and zone
    are slot slots[t] of sets[tiers[t]]. Returns uint64[nt, ceil(n/64)], row
    t = table t: what sets[tiers[t]].probe(keys, gated=gated) reports for slot
    slots[t] (src/sstable.rs:138), with the key hashed once for every tier.
    Up to 8 sets of width 32 or 64 and up to 64 tables."""
    b = as_batch(keys)
    arr, ns, t, sl = _tier_args(sets, tiers, slots)
    nt = int(t.shape[0])
    out, result = _hit_rows(nt, b.n, out)
    op, keep = _ptr_of(out)
    L = _L()
    _call_keys(L.cb_tiers_probe_fixed, L.cb_tiers_probe_var,
               (ctypes.cast(arr, ctypes.c_void_p), ns, t.ctypes.data, sl.ctypes.data, nt), b,
               (int(bool(gated)), op, _stream(stream)))
    return result
