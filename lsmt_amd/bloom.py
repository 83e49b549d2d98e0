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
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from ._ffi import (_call_keys, _Handle, _hit_rows, _host_bytes, _key_bytes, _L, _ptr_of, _raise, _size_then_fill,
                   _stream, as_batch)
from ._lib import check


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = _L().cb_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def set_path(path: int) -> None:
    """0 auto, 1 direct (per-key atomics/gathers), 2 tiled (LDS tiles)."""
    check(_L().cb_set_path(path))


def last_path() -> int:
    return int(_L().cb_last_path())


@dataclass
class BloomProto:
    """Mirror of ``BloomProto { repeated bool bits = 1; }`` (src/bloom.rs:9-13)."""
    bits: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


class BloomFilter(_Handle):
    """A Bloom filter of ``size`` bits resident in HBM (src/bloom.rs:4-7)."""
    _destroy = "cb_filter_destroy"

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
        self._pending.append(_key_bytes(item))

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
        L = _L()
        _call_keys(L.cb_filter_insert_fixed, L.cb_filter_insert_var, (self._h,), b, (_stream(stream),))

    def clear(self, stream=None) -> None:
        self._pending = []
        check(_L().cb_filter_clear(self._h, _stream(stream)))

    # ---- probe -------------------------------------------------------------
    def may_contain(self, item) -> bool:
        """src/bloom.rs:48-51 for one key (synchronous; answered from the
        host mirror of the words when it is on, see host_mirror)."""
        self.flush()
        key = _key_bytes(item)
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
        return _size_then_fill(lambda out, cap, n: _raise(_L().cb_filter_to_bytes(self._h, out, cap, n)))

    @classmethod
    def from_bytes(cls, data: bytes, device: int = 0) -> "BloomFilter":  # src/bloom.rs:74-77
        buf, n = _host_bytes(data)
        h = ctypes.c_void_p()
        _raise(_L().cb_filter_from_bytes(_ptr_of(buf)[0], n, device, ctypes.byref(h)))
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
    out, result = _hit_rows(nf, b.n, out)
    arr = (ctypes.c_void_p * max(nf, 1))(*[f.handle.value for f in filters])
    op, keep = _ptr_of(out)
    L = _L()
    _call_keys(L.cb_probe_fixed, L.cb_probe_var, (ctypes.cast(arr, ctypes.c_void_p), nf), b, (op, _stream(stream)))
    return result


def unpack_hits(hits: np.ndarray, n: int) -> np.ndarray:
    """uint64[nf, words] -> bool[nf, n]."""
    h = np.ascontiguousarray(hits, dtype="<u8")
    bits = np.unpackbits(h.view(np.uint8).reshape(h.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)
