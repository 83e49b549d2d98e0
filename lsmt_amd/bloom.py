"""Host-side mirror of the reference's ``BloomFilter`` over the gfx950 C ABI.

Same surface as /root/reference/src/bloom.rs so the reference's callers and
tests read the same:

    BloomFilter.new(size)          src/bloom.rs:17-21
    f.insert(item)                 src/bloom.rs:40-44
    f.may_contain(item) -> bool    src/bloom.rs:48-51
    f.to_proto() / from_proto(p)   src/bloom.rs:54-63
    f.to_bytes() / from_bytes(b)   src/bloom.rs:66-77

The filter bits live in HBM. Per-key ``insert`` calls are queued on the host
and flushed as ONE batched build launch before the filter is next read: this
is how SsTable::create's per-key loop (src/sstable.rs:62-65) turns into a
single GPU build without changing the caller. ``may_contain`` on one key is a
synchronous single-key probe; the read-path fan-out over many tables
(src/lib.rs:129-134) uses the batched :func:`probe`.

Errors follow the reference's panics: inserting into or probing an m == 0
filter raises ZeroDivisionError (``h % 0``, src/bloom.rs:36); malformed proto
bytes raise ValueError (``decode(..).unwrap()``, src/bloom.rs:75).

There is no CPU fallback: every operation goes through libcassbloom.so.
"""
from __future__ import annotations

import ctypes
import operator
from dataclasses import dataclass, field
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import CassBloomError, check

__all__ = ["BloomFilter", "BloomProto", "FilterSet", "probe", "insert_many", "set_path",
           "last_path", "device_count", "DeviceKeys", "KeyBatch", "ZoneMap", "zone_bounds", "TableMeta", "Table", "get_many", "sstable_create"]


def _L():
    return _lib.load()


def _raise(rc: int) -> None:
    if rc == _lib.CB_EZEROM:
        raise ZeroDivisionError("attempt to calculate the remainder with a divisor of zero")
    if rc == _lib.CB_EDECODE:
        msg = _L().cb_last_error()
        raise ValueError(msg.decode() if msg else "BloomProto decode error")
    check(rc)


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = _L().cb_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def set_path(path: int) -> None:
    """0 auto, 1 direct (per-key atomics/gathers), 2 tiled (LDS tiles)."""
    check(_L().cb_set_path(path))


def last_path() -> int:
    return int(_L().cb_last_path())


def set_dense(mode: int) -> None:
    """FilterSet probes of dense batches: 0 by density (default), 1 the
    region-partitioned probe whenever the set allows it, -1 never
    (cb_set_dense; last_path() is 6 after a dense probe)."""
    check(_L().cb_set_dense(int(mode)))


# ---- key batches ---------------------------------------------------------------

def _ptr_of(x):
    """(address, keepalive) for numpy arrays, torch tensors, or raw ints."""
    if x is None:
        return None, None
    if isinstance(x, int):
        return x, None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            x = np.ascontiguousarray(x)
        return x.ctypes.data, x
    if hasattr(x, "data_ptr"):  # torch tensor (device or host)
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr(), x
    raise TypeError(f"unsupported buffer type {type(x)!r}")


@dataclass
class KeyBatch:
    """A batch of keys as the C ABI takes them: fixed-length rows
    (``keys``: uint8[n, key_len]) or ragged (``data`` + ``offsets[n+1]``).
    Buffers may be numpy (host) or device tensors."""
    n: int
    key_len: int = 0
    keys: object = None
    data: object = None
    offsets: object = None

    @property
    def is_var(self) -> bool:
        return self.offsets is not None


def DeviceKeys(tensor) -> KeyBatch:
    """Fixed-length keys already resident in HBM (torch uint8 [n, key_len])."""
    n, kl = tensor.shape
    return KeyBatch(n=int(n), key_len=int(kl), keys=tensor)


def as_batch(keys) -> KeyBatch:
    if isinstance(keys, KeyBatch):
        return keys
    if isinstance(keys, np.ndarray):
        if keys.dtype != np.uint8 or keys.ndim != 2:
            raise TypeError("fixed-length keys must be a uint8 array of shape [n, key_len]")
        return KeyBatch(n=keys.shape[0], key_len=keys.shape[1], keys=np.ascontiguousarray(keys))
    if hasattr(keys, "data_ptr") and getattr(keys, "ndim", 0) == 2:
        return DeviceKeys(keys)
    items = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
    offs = np.zeros(len(items) + 1, np.uint64)
    if items:
        np.cumsum([len(k) for k in items], out=offs[1:])
    data = np.frombuffer(b"".join(items), np.uint8) if offs[-1] else np.zeros(1, np.uint8)
    return KeyBatch(n=len(items), data=np.ascontiguousarray(data), offsets=offs)


def _stream(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)  # torch.cuda.Stream


# ---- proto mirror ----------------------------------------------------------------

@dataclass
class BloomProto:
    """Mirror of ``BloomProto { repeated bool bits = 1; }`` (src/bloom.rs:9-13)."""
    bits: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


@dataclass
class ZoneMap:
    """Mirror of ``ZoneMap { min, max: Option<String> }`` (src/zonemap.rs:3-8).

    Bounds are bytes, ordered as Rust orders ``str`` (byte-wise, a proper
    prefix first). This host object only carries a table's bounds; the
    per-key gate runs on the device (``FilterSet.probe(..., gated=True)``)."""
    min: bytes | None = None
    max: bytes | None = None

    def update(self, key) -> None:
        """zonemap.rs:21-32."""
        k = key.encode() if isinstance(key, str) else bytes(key)
        if self.min is None or k < self.min:
            self.min = k
        if self.max is None or k > self.max:
            self.max = k

    def contains(self, key) -> bool:
        """zonemap.rs:37-42: min <= key <= max, true if a bound is missing."""
        if self.min is None or self.max is None:
            return True
        k = key.encode() if isinstance(key, str) else bytes(key)
        return self.min <= k <= self.max


@dataclass
class TableMeta:
    """Mirror of ``TableMeta { bloom: Option<BloomProto>, zone_map:
    Option<ZoneMapProto> }`` (src/sstable.rs:31-37), the SSTable ``.meta``
    file. Encoding and decoding run through the C ABI; the filter's bits are
    expanded / packed on the device."""
    bloom: "BloomFilter | None" = None
    zone_map: ZoneMap | None = None

    def encode(self) -> bytes:
        """TableMeta.encode (SsTable::create, src/sstable.rs:74-81)."""
        zb, keep = _zone_struct(self.zone_map)
        fh = self.bloom.handle if self.bloom is not None else None
        if self.bloom is not None:
            self.bloom.flush()
        n = ctypes.c_uint64()
        zp = ctypes.byref(zb) if zb is not None else None
        _raise(_L().cb_meta_encode(fh, zp, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint8)
        _raise(_L().cb_meta_encode(fh, zp, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[: n.value].tobytes()

    @classmethod
    def decode(cls, data: bytes, device: int = 0) -> "TableMeta":
        """TableMeta::decode; raises ValueError (CB_EDECODE) on malformed bytes.
        A missing field decodes to None, as in the proto."""
        bloom, info, buf = _meta_decode(data, device)
        return cls(bloom if info.has_bloom else None, _zone_from_info(info, buf) if info.has_zone else None)

    @staticmethod
    def load(data: bytes, device: int = 0) -> "tuple[BloomFilter, ZoneMap]":
        """The metadata half of SsTable::load (src/sstable.rs:96-108): a missing
        bloom is BloomFilter::new(1024), a missing zone map ZoneMap::default()."""
        bloom, info, buf = _meta_decode(data, device)
        return bloom, (_zone_from_info(info, buf) if info.has_zone else ZoneMap())


def _zone_struct(z: "ZoneMap | None"):
    if z is None:
        return None, None
    lo = z.min.encode() if isinstance(z.min, str) else z.min
    hi = z.max.encode() if isinstance(z.max, str) else z.max
    lb = ctypes.create_string_buffer(lo or b"", max(len(lo or b""), 1))
    hb = ctypes.create_string_buffer(hi or b"", max(len(hi or b""), 1))
    zb = _lib.ZoneBounds(ctypes.cast(lb, ctypes.c_void_p), len(lo or b""), lo is not None,
                         ctypes.cast(hb, ctypes.c_void_p), len(hi or b""), hi is not None)
    return zb, (lb, hb)


def _meta_decode(data: bytes, device: int):
    buf = np.frombuffer(bytes(data), np.uint8).copy() if data else np.zeros(1, np.uint8)
    h = ctypes.c_void_p()
    info = _lib.MetaInfo()
    _raise(_L().cb_meta_decode(buf.ctypes.data, len(data), int(device), ctypes.byref(h), ctypes.byref(info)))
    return BloomFilter(0, device=device, _handle=h.value), info, buf


def _zone_from_info(info, buf: np.ndarray) -> ZoneMap:
    base = buf.ctypes.data
    z = info.zone

    def span(p, n, has):
        if not has:
            return None
        return buf[p - base: p - base + n].tobytes() if n else b""
    return ZoneMap(span(z.min or 0, z.min_len, z.has_min), span(z.max or 0, z.max_len, z.has_max))


def zone_bounds(keys, device: int = 0, stream=None) -> tuple[int, int] | None:
    """(index of first smallest key, index of first largest key), computed on
    the device; None for an empty batch."""
    b = as_batch(keys)
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    s = _stream(stream)
    if b.is_var:
        dp, k1 = _ptr_of(b.data)
        offp, k2 = _ptr_of(b.offsets)
        _raise(_L().cb_zone_bounds_var(dp, offp, b.n, int(device), ctypes.byref(lo), ctypes.byref(hi), s))
    else:
        kp, k1 = _ptr_of(b.keys)
        _raise(_L().cb_zone_bounds_fixed(kp, b.key_len, b.n, int(device), ctypes.byref(lo),
                                         ctypes.byref(hi), s))
    if b.n == 0:
        return None
    return int(lo.value), int(hi.value)


# ---- the filter --------------------------------------------------------------------

class BloomFilter:
    """A Bloom filter of ``size`` bits resident in HBM (src/bloom.rs:4-7)."""

    def __init__(self, size: int, device: int = 0, _handle: int | None = None):
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = ctypes.c_void_p(_handle)
        else:
            _raise(_L().cb_filter_create(int(size), int(device), ctypes.byref(self._h)))
        m = ctypes.c_uint64()
        check(_L().cb_filter_bits(self._h, ctypes.byref(m)))
        self._m = int(m.value)
        d = ctypes.c_int()
        check(_L().cb_filter_device(self._h, ctypes.byref(d)))
        self._device = int(d.value)
        self._pending: list[bytes] = []

    # src/bloom.rs:17-21
    @classmethod
    def new(cls, size: int, device: int = 0) -> "BloomFilter":
        return cls(size, device)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _L().cb_filter_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def m(self) -> int:
        return self._m

    @property
    def device(self) -> int:
        return self._device

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def __len__(self) -> int:
        return self._m

    # ---- build -------------------------------------------------------------
    def insert(self, item) -> None:
        """src/bloom.rs:40-44. Queued; flushed as one batched launch."""
        if self._m == 0:
            raise ZeroDivisionError("attempt to calculate the remainder with a divisor of zero")
        self._pending.append(item.encode() if isinstance(item, str) else bytes(item))

    def flush(self, stream=None) -> None:
        if self._pending:
            batch, self._pending = self._pending, []
            self.insert_batch(batch, stream=stream)

    def insert_batch(self, keys, stream=None) -> None:
        """Batched insert of every key (the flush build, src/sstable.rs:62-65)."""
        b = as_batch(keys)
        if self._pending:
            pend, self._pending = self._pending, []
            self.insert_batch(pend, stream=stream)
        s = _stream(stream)
        if b.is_var:
            dp, k1 = _ptr_of(b.data)
            op, k2 = _ptr_of(b.offsets)
            _raise(_L().cb_filter_insert_var(self._h, dp, op, b.n, s))
        else:
            kp, k1 = _ptr_of(b.keys)
            _raise(_L().cb_filter_insert_fixed(self._h, kp, b.key_len, b.n, s))

    def clear(self, stream=None) -> None:
        self._pending = []
        check(_L().cb_filter_clear(self._h, _stream(stream)))

    # ---- probe -------------------------------------------------------------
    def may_contain(self, item) -> bool:
        """src/bloom.rs:48-51 for one key (synchronous; answered from the
        host mirror of the words when it is on, see host_mirror)."""
        self.flush()
        key = item.encode() if isinstance(item, str) else bytes(item)
        buf = ctypes.create_string_buffer(key, max(len(key), 1))
        out = ctypes.c_int(0)
        _raise(_L().cb_may_contain(self._h, ctypes.cast(buf, ctypes.c_void_p), len(key), ctypes.byref(out)))
        return bool(out.value)

    def host_mirror(self, mode: int = 1) -> None:
        """Single-key may_contain source (cb_filter_host_mirror): 1 the host
        mirror of the words (refreshed by one copy after each write), 0 a
        one-key GPU probe per call, -1 auto (mirror when m <= 2^24)."""
        check(_L().cb_filter_host_mirror(self._h, int(mode)))

    def host_mirror_info(self) -> tuple[bool, bool]:
        """(mirror on, mirror holds the latest write)."""
        on, cur = ctypes.c_int(), ctypes.c_int()
        check(_L().cb_filter_host_mirror_info(self._h, ctypes.byref(on), ctypes.byref(cur)))
        return bool(on.value), bool(cur.value)

    def may_contain_batch(self, keys, stream=None) -> np.ndarray:
        hits = probe([self], keys, stream=stream)
        n = as_batch(keys).n
        return unpack_hits(hits, n)[0]

    # ---- persistence -------------------------------------------------------
    def bools(self, stream=None) -> np.ndarray:
        """The Vec<bool> contents as uint8 0/1 (to_proto's bits)."""
        self.flush(stream)
        out = np.zeros(max(self._m, 1), np.uint8)
        _raise(_L().cb_filter_export_bools(self._h, out.ctypes.data, _stream(stream)))
        return out[: self._m]

    def packed(self, stream=None) -> np.ndarray:
        self.flush(stream)
        nw = (self._m + 31) // 32
        out = np.zeros(max(nw, 1), np.uint32)
        _raise(_L().cb_filter_export_packed(self._h, out.ctypes.data, _stream(stream)))
        return out[:nw]

    def load_packed(self, words: np.ndarray, stream=None) -> None:
        self._pending = []
        w = np.ascontiguousarray(words, dtype=np.uint32)
        _raise(_L().cb_filter_import_packed(self._h, w.ctypes.data if w.size else None, w.size, _stream(stream)))

    def to_proto(self) -> BloomProto:  # src/bloom.rs:54-58
        return BloomProto(bits=self.bools().astype(bool))

    @classmethod
    def from_proto(cls, proto: BloomProto, device: int = 0) -> "BloomFilter":  # src/bloom.rs:61-63
        bits = np.ascontiguousarray(np.asarray(proto.bits, dtype=bool).view(np.uint8))
        f = cls(bits.shape[0], device)
        if bits.shape[0]:
            _raise(_L().cb_filter_import_bools(f._h, bits.ctypes.data, bits.shape[0], None))
        return f

    def to_bytes(self) -> bytes:  # src/bloom.rs:66-70
        self.flush()
        n = ctypes.c_uint64()
        _raise(_L().cb_filter_to_bytes(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(int(n.value), 1), np.uint8)
        _raise(_L().cb_filter_to_bytes(self._h, out.ctypes.data, int(n.value), ctypes.byref(n)))
        return out[: int(n.value)].tobytes()

    @classmethod
    def from_bytes(cls, data: bytes, device: int = 0) -> "BloomFilter":  # src/bloom.rs:74-77
        buf = np.frombuffer(bytes(data), np.uint8) if data else np.zeros(1, np.uint8)
        h = ctypes.c_void_p()
        _raise(_L().cb_filter_from_bytes(buf.ctypes.data, len(data), device, ctypes.byref(h)))
        return cls(0, _handle=h.value)


# ---- batched multi-filter build (concurrent flushes) ---------------------------------

def insert_many(filters: Sequence["BloomFilter"], keys_per_filter, stream=None) -> None:
    """filters[i].insert of every row of keys_per_filter[i] (uint8 [n_i, L]
    arrays or device tensors, one key length L), all built together."""
    nf = len(filters)
    if nf == 0:
        return
    for f in filters:
        f.flush(stream)
    batches = [as_batch(k) for k in keys_per_filter]
    if len(batches) != nf or any(b.is_var for b in batches):
        raise ValueError("one fixed-length key array per filter")
    kl = {b.key_len for b in batches if b.n}
    if len(kl) > 1:
        raise ValueError("all key arrays must share one key length")
    key_len = kl.pop() if kl else 0
    keep = []
    ptrs = (ctypes.c_void_p * nf)()
    ns = (ctypes.c_uint64 * nf)()
    for i, b in enumerate(batches):
        p, k = _ptr_of(b.keys) if b.n else (None, None)
        keep.append(k)
        ptrs[i] = p
        ns[i] = b.n
    hs = (ctypes.c_void_p * nf)(*[f.handle.value for f in filters])
    _raise(_L().cb_filter_insert_fixed_many(ctypes.cast(hs, ctypes.c_void_p), nf,
                                            ctypes.cast(ptrs, ctypes.c_void_p), key_len,
                                            ctypes.cast(ns, ctypes.c_void_p), _stream(stream)))


# ---- batched multi-filter probe ------------------------------------------------------

def probe(filters: Sequence[BloomFilter], keys, out=None, stream=None) -> np.ndarray:
    """may_contain of every key against every filter (Database::get's fan-out,
    src/lib.rs:129-134). Returns (or fills ``out``) uint64[nf, ceil(n/64)]:
    bit k%64 of word [f][k/64] = filters[f].may_contain(key k)."""
    b = as_batch(keys)
    nf = len(filters)
    for f in filters:
        f.flush(stream)
    words = (b.n + 63) // 64
    if out is None:
        out = np.zeros((nf, max(words, 1)), np.uint64)
        result = out[:, :words]
    else:
        result = out
    arr = (ctypes.c_void_p * max(nf, 1))(*[f.handle.value for f in filters])
    op, keep = _ptr_of(out)
    s = _stream(stream)
    if b.is_var:
        dp, k1 = _ptr_of(b.data)
        offp, k2 = _ptr_of(b.offsets)
        _raise(_L().cb_probe_var(ctypes.cast(arr, ctypes.c_void_p), nf, dp, offp, b.n, op, s))
    else:
        kp, k1 = _ptr_of(b.keys)
        _raise(_L().cb_probe_fixed(ctypes.cast(arr, ctypes.c_void_p), nf, kp, b.key_len, b.n, op, s))
    return result


class FilterSet:
    """Up to ``width`` filters of one size m, bit-sliced in HBM for the
    read-path fan-out (Database::get, src/lib.rs:129-134): one probe call
    answers may_contain for every slot with two word (or row) reads per key.
    width 32 or 64, or a wide set of any multiple of 64 up to 4096 slots
    (rows of width/64 uint64 words: the reference's real shape of hundreds of
    m = 1024 tables, src/sstable.rs:44,59, src/lib.rs:72,105). A derived copy —
    the BloomFilter handles remain the source of truth."""

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

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _L().cb_set_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        lo, hi = (zone.min, zone.max) if isinstance(zone, ZoneMap) else zone
        lo = lo.encode() if isinstance(lo, str) else lo
        hi = hi.encode() if isinstance(hi, str) else hi
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
        buf = np.frombuffer(bytes(data), np.uint8).copy() if data else np.zeros(1, np.uint8)
        _raise(_L().cb_set_load_meta(self._h, int(slot), buf.ctypes.data, len(data), _stream(stream)))

    def zone_from_keys(self, slot: int, keys, stream=None) -> None:
        """ZoneMap::update over a key batch, on the device (src/sstable.rs:62-65)."""
        b = as_batch(keys)
        s = _stream(stream)
        if b.is_var:
            dp, k1 = _ptr_of(b.data)
            offp, k2 = _ptr_of(b.offsets)
            _raise(_L().cb_set_zone_from_keys_var(self._h, int(slot), dp, offp, b.n, s))
        else:
            kp, k1 = _ptr_of(b.keys)
            _raise(_L().cb_set_zone_from_keys_fixed(self._h, int(slot), kp, b.key_len, b.n, s))

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
        used = self.used
        words = (b.n + 63) // 64
        if out is None:
            out = np.zeros((max(used, 1), max(words, 1)), np.uint64)
            result = out[:used, :words]
        else:
            result = out
        op, keep = _ptr_of(out)
        s = _stream(stream)
        if b.is_var:
            dp, k1 = _ptr_of(b.data)
            offp, k2 = _ptr_of(b.offsets)
            fn = _L().cb_set_probe_gated_var if gated else _L().cb_set_probe_var
            _raise(fn(self._h, dp, offp, b.n, op, s))
        else:
            kp, k1 = _ptr_of(b.keys)
            fn = _L().cb_set_probe_gated_fixed if gated else _L().cb_set_probe_fixed
            _raise(fn(self._h, kp, b.key_len, b.n, op, s))
        return result


# ---- SSTable data files and the batched read path (src/sstable.rs:133-179, src/lib.rs:128-134)

class Table:
    """One SSTable data file (``key \t base64(value) \n`` lines, sorted;
    src/sstable.rs:57-72) resident in HBM with its line index, built on the
    device. ``data``: bytes, a uint8 numpy array, or a uint8 device tensor."""

    def __init__(self, data, device: int = 0, stream=None):
        self._h = ctypes.c_void_p()
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(bytes(data), np.uint8)
        n = int(data.numel()) if hasattr(data, "numel") else int(len(data))
        ptr, keep = _ptr_of(data if n else np.zeros(1, np.uint8))
        _raise(_L().cb_table_create(ptr, n, int(device), _stream(stream), ctypes.byref(self._h)))
        self.device = int(device)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _L().cb_table_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        n = ctypes.c_uint64()
        check(_L().cb_table_zone(self._h, int(which), None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(int(n.value), 1))
        check(_L().cb_table_zone(self._h, int(which), buf, n.value, ctypes.byref(n)))
        return buf.raw[:n.value]

    def rebuild(self, m: int = 1024, stream=None) -> "tuple[BloomFilter, ZoneMap]":
        """SsTable::load's rebuild from the data file when `.meta` is missing or
        undecodable (src/sstable.rs:109-120), on the device: (bloom, zone_map)
        over the keys of the lines that have a TAB. A key that is not UTF-8
        raises UnicodeDecodeError, as the reference's load returns Err."""
        h = ctypes.c_void_p()
        lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
        rc = _L().cb_table_rebuild(self._h, int(m), _stream(stream), ctypes.byref(h), ctypes.byref(lo),
                                   ctypes.byref(hi))
        if rc == _lib.CB_EUTF8:
            msg = _L().cb_last_error().decode()
            raise UnicodeDecodeError("utf-8", b"", 0, 1, msg)
        _raise(rc)
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
        s = _stream(stream)
        if b.is_var:
            dp, k1 = _ptr_of(b.data)
            offp, k2 = _ptr_of(b.offsets)
            _raise(_L().cb_table_search_var(self._h, dp, offp, b.n, op, s))
        else:
            kp, k1 = _ptr_of(b.keys)
            _raise(_L().cb_table_search_fixed(self._h, kp, b.key_len, b.n, op, s))
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


def compact(tables: Sequence[Table], m: int = 1024, stream=None):
    """Newest-wins merge of well-formed tables (tables[0] newest, as get_many
    takes them) into one, on the device (cb_tables_compact). The reference has
    no compaction; the result is SsTable::create (src/sstable.rs:51-87) of
    every key of the inputs with the value Database::get (src/lib.rs:128-134)
    returns for it over them: a key keeps its newest line whose value decodes,
    and a key whose value decodes nowhere is dropped. Returns (Table,
    BloomFilter of m bits, ZoneMap), as sstable_create does. The inputs are
    not modified and may be closed as soon as the call returns."""
    arr, dev = _table_list(tables)
    th, fh = ctypes.c_void_p(), ctypes.c_void_p()
    _raise(_L().cb_tables_compact(arr, len(tables), int(m), _stream(stream), ctypes.byref(th), ctypes.byref(fh)))
    return _adopt_compaction(th, fh, dev)


# ---- the write-ahead log (src/wal.rs:14-31, src/lib.rs:30-39, 96-102)

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
    if isinstance(log, (bytes, bytearray, memoryview)):
        log = np.frombuffer(bytes(log), np.uint8)
    n = int(log.numel()) if hasattr(log, "numel") else int(len(log))
    ptr, keep = _ptr_of(log if n else np.zeros(1, np.uint8))
    th, fh, st = ctypes.c_void_p(), ctypes.c_void_p(), LogStats()
    rc = _L().cb_log_replay(ptr, n, int(m), int(device), _stream(stream), ctypes.byref(th), ctypes.byref(fh),
                            ctypes.byref(st))
    if rc in (_lib.CB_EUTF8, _lib.CB_EBASE64):
        msg = _L().cb_last_error().decode()
        err = UnicodeDecodeError("utf-8", b"", 0, 1, msg) if rc == _lib.CB_EUTF8 else ValueError(msg)
        err.code, err.stats = rc, st
        raise err
    _raise(rc)
    table, bloom, zone = _adopt_compaction(th, fh, int(device))
    return table, bloom, (zone if table.nlines else None), st


def _key_bytes(k) -> bytes:
    return k.encode() if isinstance(k, str) else bytes(k)


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


class ScanResult:
    """A scan's entries in device memory (cb_scan_*): sorted by key, each with
    its decoded value and the index in the scanned table list of the table
    that supplied it. Complete when scan() returns; the scanned tables may be
    closed while it lives."""

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

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _L().cb_scan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    if prefixes is not None:  # (the library turns them into ranges itself)
        parts = [_key_bytes(p) for p in prefixes]
        off = np.zeros(len(parts) + 1, np.uint64)
        np.cumsum([len(b) for b in parts], out=off[1:])
        _raise(_L().cb_tables_scan_prefixes(arr, len(tables), b"".join(parts), _ptr_of(off)[0], len(parts),
                                            _stream(stream), ctypes.byref(h)))
    else:
        ranges = list(ranges)
        if any(hi is None for _, hi in ranges[:-1]):
            raise ValueError("hi=None is allowed on the last range only")
        data, off, nr, last_unbounded = _range_list(ranges, None)
        _raise(_L().cb_tables_scan_many(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, _stream(stream),
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
    parts = [b for lo, hi in pairs for b in (lo, _key_bytes(hi) if hi is not None else b"")]
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(b) for b in parts], out=off[1:])
    return b"".join(parts), off, len(pairs), last_unbounded


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
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, _ = _table_list(tables)
    entries, live = np.zeros(max(nr, 1), np.uint64), np.zeros(max(nr, 1), np.uint64)
    _raise(_L().cb_tables_count(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, _stream(stream),
                                _ptr_of(entries)[0], _ptr_of(live)[0]))
    return entries[:nr], live[:nr]


def scan_live(tables: Sequence[Table], ranges=None, prefixes=None, limit: int = 0, stream=None) -> ScanResult:
    """scan_many without the dead entries (cb_tables_scan_live): deleted rows
    (count's rule) are left out on the device, and range_off() counts live
    entries. A tombstone shadows before it is dropped: a key whose newest
    decodable line is dead is absent even when an older table holds a live
    value. limit > 0 takes exactly one range: the first `limit` live entries,
    ScanResult.truncated saying whether more live entries qualified."""
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    _raise(_L().cb_tables_scan_live(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, int(limit),
                                    _stream(stream), ctypes.byref(h)))
    return ScanResult(h.value, dev)


def compact_live(tables: Sequence[Table], m: int = 1024, stream=None):
    """compact() that also drops deleted rows (cb_tables_compact_live): the
    merged table holds every key whose newest decodable line is not a
    tombstone (count's rule), and the Bloom filter and zone map are of those
    keys. Correct only for a full compaction: with an older table of the store
    left out of `tables`, a dropped tombstone no longer shadows that table's
    line and the deleted row comes back. Returns (Table, BloomFilter, ZoneMap)
    as compact does."""
    arr, dev = _table_list(tables)
    th, fh = ctypes.c_void_p(), ctypes.c_void_p()
    _raise(_L().cb_tables_compact_live(arr, len(tables), int(m), _stream(stream), ctypes.byref(th), ctypes.byref(fh)))
    return _adopt_compaction(th, fh, dev)


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
    arr, dev = _table_list(tables)
    th, fh = ctypes.c_void_p(), ctypes.c_void_p()
    _raise(_L().cb_tables_compact_lww(arr, len(tables), int(m), int(bool(drop_dead)), _stream(stream),
                                      ctypes.byref(th), ctypes.byref(fh)))
    return _adopt_compaction(th, fh, dev)


def scan_lww(tables: Sequence[Table], ranges=None, prefixes=None, limit: int = 0, drop_dead: bool = False,
             stream=None) -> ScanResult:
    """scan_many under compact_lww's rule (cb_tables_scan_lww): every key's
    entry is its winner by timestamp, which() its table's index in `tables`
    and ts() its timestamp. drop_dead leaves out the winners that are
    tombstones. limit > 0 takes exactly one range, as in scan_live."""
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, dev = _table_list(tables)
    h = ctypes.c_void_p()
    _raise(_L().cb_tables_scan_lww(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, int(bool(drop_dead)),
                                   int(limit), _stream(stream), ctypes.byref(h)))
    return ScanResult(h.value, dev)


def count_lww(tables: Sequence[Table], ranges=None, prefixes=None, stream=None):
    """count() under compact_lww's rule (cb_tables_count_lww): (entries, live),
    per range the winners and the winners that are not tombstones, i.e. the
    sizes of scan_lww's ranges with drop_dead False and True."""
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, _ = _table_list(tables)
    entries, live = np.zeros(max(nr, 1), np.uint64), np.zeros(max(nr, 1), np.uint64)
    _raise(_L().cb_tables_count_lww(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, _stream(stream),
                                    _ptr_of(entries)[0], _ptr_of(live)[0]))
    return entries[:nr], live[:nr]


class _CbWhere(ctypes.Structure):
    """cb_where (include/cassbloom.h)."""
    _fields_ = [("cols", ctypes.c_void_p), ("col_off", ctypes.c_void_p), ("vals", ctypes.c_void_p),
                ("val_off", ctypes.c_void_p), ("part", ctypes.c_void_p), ("nc", ctypes.c_uint32)]


class _Where:
    """A cb_where built from a mapping or a list of (column, value), with
    `key_columns` (the schema's key_columns(), src/schema.rs:27-33) giving each
    condition its key part; keeps the arrays it points into alive."""

    def __init__(self, where, key_columns=()):
        pairs = list(where.items()) if hasattr(where, "items") else list(where)
        cols = [_key_bytes(c) for c, _ in pairs]
        vals = [_key_bytes(v) for _, v in pairs]
        kc = [_key_bytes(c) for c in key_columns]
        self.col_off = np.zeros(len(pairs) + 1, np.uint64)
        self.val_off = np.zeros(len(pairs) + 1, np.uint64)
        np.cumsum([len(c) for c in cols], out=self.col_off[1:])
        np.cumsum([len(v) for v in vals], out=self.val_off[1:])
        self.cols = ctypes.create_string_buffer(b"".join(cols), max(int(self.col_off[-1]), 1))
        self.vals = ctypes.create_string_buffer(b"".join(vals), max(int(self.val_off[-1]), 1))
        self.part = np.array([kc.index(c) if c in kc else -1 for c in cols] + [0], np.int32)
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
    data, off, nr, last_unbounded = _range_list(ranges, prefixes)
    arr, _ = _table_list(tables)
    w = _Where(where, key_columns)
    if skip is None:
        skip = [len(_key_bytes(p)) for p in prefixes] if prefixes is not None else 0
    sk = np.ascontiguousarray(_per_range(skip, nr) + [0], np.uint32)
    live, matched = np.zeros(max(nr, 1), np.uint64), np.zeros(max(nr, 1), np.uint64)
    _raise(_L().cb_tables_count_where(arr, len(tables), data, _ptr_of(off)[0], nr, last_unbounded, _ptr_of(sk)[0],
                                      w.ref(), int(bool(lww)), _stream(stream), _ptr_of(live)[0],
                                      _ptr_of(matched)[0]))
    return live[:nr], matched[:nr]


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
        kc = [_key_bytes(c) for c in key_columns]
        self.col_off = np.zeros(len(self.names) + 1, np.uint64)
        np.cumsum([len(c) for c in self.names], out=self.col_off[1:])
        self.cols = ctypes.create_string_buffer(b"".join(self.names), max(int(self.col_off[-1]), 1))
        self.part = np.array([kc.index(c) if c in kc else -1 for c in self.names] + [0], np.int32)
        self.cast = np.array([chosen[c] for c in self.names] + [0], np.int64)
        if ((self.cast < 0) | (self.cast > 255)).any():
            raise ValueError("a cast is 0 or 1")
        self.cast = self.cast.astype(np.uint8)
        self.c = _CbSelect(ctypes.addressof(self.cols), self.col_off.ctypes.data, self.part.ctypes.data,
                           self.cast.ctypes.data, len(self.names))

    def ref(self):
        return ctypes.addressof(self.c)


class RowsResult:
    """A selection's response in device memory (cb_rows_*): the bytes the
    reference's exec_select_schema returns (src/query.rs:365-432) and, per row,
    where its text lies in them and its flags (_lib.ROW_*). Complete when the
    call that made it returns."""

    def __init__(self, handle: int, device: int):
        self._h = ctypes.c_void_p(handle)
        self.device = device
        n, wt, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(_L().cb_rows_info(self._h, ctypes.byref(n), ctypes.byref(wt), ctypes.byref(nb)))
        self.count, self.with_text, self.bytes = int(n.value), int(wt.value), int(nb.value)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _L().cb_rows_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
    n, f = ctypes.c_uint64(), ctypes.c_uint8()
    check(_L().cb_row_select(k, len(k), int(skip), v, len(v), q.ref(), int(bool(meta)), None, 0, ctypes.byref(n),
                             ctypes.byref(f)))
    if not f.value & _lib.ROW_TEXT:
        return None, int(f.value)
    out = ctypes.create_string_buffer(max(int(n.value), 1))
    check(_L().cb_row_select(k, len(k), int(skip), v, len(v), q.ref(), int(bool(meta)), out, int(n.value),
                             ctypes.byref(n), ctypes.byref(f)))
    return out.raw[:n.value], int(f.value)


def _to_var(b: KeyBatch) -> KeyBatch:
    keys = np.ascontiguousarray(b.keys)
    offs = (np.arange(0, b.key_len * (b.n + 1), b.key_len, dtype=np.uint64) if b.key_len
            else np.zeros(b.n + 1, np.uint64))
    data = keys.reshape(-1) if keys.size else np.zeros(1, np.uint8)
    return KeyBatch(n=b.n, data=data, offsets=offs)


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
    if b.is_var:
        dp, k1 = _ptr_of(b.data)
        offp, k2 = _ptr_of(b.offsets)

        def call(vp, cap):
            _raise(var_fn(*head, dp, offp, b.n, wp, vo, vp, cap, tref, s))
    else:
        kp, k1 = _ptr_of(b.keys)

        def call(vp, cap):
            _raise(fixed_fn(*head, kp, b.key_len, b.n, wp, vo, vp, cap, tref, s))
    if out is not None:
        call(_ptr_of(vals)[0], cap)
        return which, voff, (int(total.value) if wait else None)
    call(None, 0)
    vals = np.zeros(max(int(total.value), 1), np.uint8)
    call(vals.ctypes.data, int(total.value))
    return which[: b.n], voff, vals[: int(total.value)].tobytes()


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
    words = (b.n + 63) // 64
    if out is None:
        out = np.zeros((max(nt, 1), max(words, 1)), np.uint64)
        result = out[:nt, :words]
    else:
        result = out
    op, keep = _ptr_of(out)
    s = _stream(stream)
    ap = ctypes.cast(arr, ctypes.c_void_p)
    if b.is_var:
        dp, k1 = _ptr_of(b.data)
        offp, k2 = _ptr_of(b.offsets)
        _raise(_L().cb_tiers_probe_var(ap, ns, t.ctypes.data, sl.ctypes.data, nt, dp, offp, b.n, int(bool(gated)),
                                       op, s))
    else:
        kp, k1 = _ptr_of(b.keys)
        _raise(_L().cb_tiers_probe_fixed(ap, ns, t.ctypes.data, sl.ctypes.data, nt, kp, b.key_len, b.n,
                                         int(bool(gated)), op, s))
    return result


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


def unpack_hits(hits: np.ndarray, n: int) -> np.ndarray:
    """uint64[nf, words] -> bool[nf, n]."""
    h = np.ascontiguousarray(hits, dtype="<u8")
    bits = np.unpackbits(h.view(np.uint8).reshape(h.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


# ---- multi-GPU exchange (lsmt_amd/shard.py) ---------------------

def _pack_blocks(nw: int) -> int:
    from .shard import PACK_BLOCK_WORDS
    return -(-int(nw) // PACK_BLOCK_WORDS)


def hits_compress(hits, pack, cap: int, stream=None) -> None:
    """pack (int32 device tensor) := {count, 0, set-bit positions[cap],
    directory} of hits ([rows][words] int64 device tensor): cb_hits_compress.
    cap is required: packs that are all-gathered share one stride (the
    largest shard's, cb_hits_pack_words), so every rank must pass the same cap
    and no rank may derive it from its own pack size."""
    rows, words = hits.shape
    cap = int(cap)
    if cap < 0 or int(pack.numel()) < 2 + cap + 2 * _pack_blocks(rows * words):
        raise ValueError("pack too small for cap positions and the directory")
    hp, k1 = _ptr_of(hits)
    pp, k2 = _ptr_of(pack)
    _raise(_L().cb_hits_compress(hp, rows, words, pp, cap, _stream(stream)))


def hits_expand(packs, world: int, row_off, full, cap: int, ok=None, stream=None) -> None:
    """full ([total_rows][words] int64 device tensor) := the OR of every
    rank's positions (packs: the all-gathered int32 [world * stride], stride
    = cb_hits_pack_words of the largest shard, every pack compressed with this
    same cap). ok: optional int32 device tensor, cleared to 0 when some rank's
    count exceeds cap (that rank's rows are then zeros in full)."""
    total_rows, words = full.shape
    bounds = [int(x) for x in row_off] + [int(total_rows)]
    max_rows = max(bounds[r + 1] - bounds[r] for r in range(world))
    if int(packs.numel()) < world * (2 + int(cap) + 2 * _pack_blocks(max_rows * words)):
        raise ValueError("packs too small for world packs of the largest shard's stride")
    off = (ctypes.c_uint64 * world)(*bounds[:world])
    pp, k1 = _ptr_of(packs)
    fp, k2 = _ptr_of(full)
    op, k3 = _ptr_of(ok)
    _raise(_L().cb_hits_expand(pp, world, int(cap), off, words, total_rows, fp, op, _stream(stream)))


def hits_expand_set(packs, world: int, row_off, n: int, full, cap: int, ok=None, stream=None) -> None:
    """full ([total_rows][ceil(n/64)] int64 device tensor) := every rank's
    rows from packs written by FilterSet.probe_pack (all-gathered int32,
    world x FilterSet.pack_words(n, cap)): cb_hits_expand_set."""
    total_rows = int(full.shape[0])
    off = (ctypes.c_uint64 * world)(*[int(x) for x in row_off])
    pp, k1 = _ptr_of(packs)
    fp, k2 = _ptr_of(full)
    op, k3 = _ptr_of(ok)
    _raise(_L().cb_hits_expand_set(pp, world, int(cap), off, int(n), total_rows, fp, op, _stream(stream)))
