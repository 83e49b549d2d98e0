"""Zone maps and the SSTable ``.meta`` file (src/zonemap.rs, src/sstable.rs:
31-37): the host mirrors of ``ZoneMap`` and ``TableMeta``, and the bounds of
a key batch computed on the device."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._ffi import _call_keys, _host_bytes, _key_bytes, _L, _raise, _size_then_fill, _stream, as_batch
from .bloom import BloomFilter


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
        k = _key_bytes(key)
        if self.min is None or k < self.min:
            self.min = k
        if self.max is None or k > self.max:
            self.max = k

    def contains(self, key) -> bool:
        """zonemap.rs:37-42: min <= key <= max, true if a bound is missing."""
        if self.min is None or self.max is None:
            return True
        return self.min <= _key_bytes(key) <= self.max


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
        zp = ctypes.byref(zb) if zb is not None else None
        return _size_then_fill(lambda out, cap, n: _raise(_L().cb_meta_encode(fh, zp, out, cap, n)))

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


def _bound(b) -> "bytes | None":
    return None if b is None else _key_bytes(b)


def _zone_struct(z: "ZoneMap | None"):
    if z is None:
        return None, None
    lo, hi = _bound(z.min), _bound(z.max)
    lb = ctypes.create_string_buffer(lo or b"", max(len(lo or b""), 1))
    hb = ctypes.create_string_buffer(hi or b"", max(len(hi or b""), 1))
    zb = _lib.ZoneBounds(ctypes.cast(lb, ctypes.c_void_p), len(lo or b""), lo is not None,
                         ctypes.cast(hb, ctypes.c_void_p), len(hi or b""), hi is not None)
    return zb, (lb, hb)


def _meta_decode(data: bytes, device: int):
    buf, n = _host_bytes(data)
    h = ctypes.c_void_p()
    info = _lib.MetaInfo()
    _raise(_L().cb_meta_decode(buf.ctypes.data, n, int(device), ctypes.byref(h), ctypes.byref(info)))
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
    L = _L()
    _call_keys(L.cb_zone_bounds_fixed, L.cb_zone_bounds_var, (), b,
               (int(device), ctypes.byref(lo), ctypes.byref(hi), _stream(stream)))
    if b.n == 0:
        return None
    return int(lo.value), int(hi.value)
