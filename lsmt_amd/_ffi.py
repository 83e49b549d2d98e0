"""The base of the ctypes binding: the loaded library, error mapping, buffer
and key-batch conversion, and one body for each step that the subject
modules (bloom, zone, filterset, table, wal, rows, scan, get, exchange) and
shard.py repeat. It imports none of them.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check


def _L():
    return _lib.load()


def _raise(rc: int) -> None:
    if rc == _lib.CB_EZEROM:
        raise ZeroDivisionError("attempt to calculate the remainder with a divisor of zero")
    if rc == _lib.CB_EDECODE:
        msg = _L().cb_last_error()
        raise ValueError(msg.decode() if msg else "BloomProto decode error")
    check(rc)


def _raise_text(rc: int, stats=None) -> None:
    """_raise, with the two errors a line's text can be: a key that is not
    UTF-8 (CB_EUTF8) raises UnicodeDecodeError, a value that is not STANDARD
    base64 (CB_EBASE64) ValueError, both with the library's message. With
    `stats` the error carries the code and them as ``.code`` and ``.stats``."""
    if rc in (_lib.CB_EUTF8, _lib.CB_EBASE64):
        msg = _L().cb_last_error().decode()
        err = UnicodeDecodeError("utf-8", b"", 0, 1, msg) if rc == _lib.CB_EUTF8 else ValueError(msg)
        if stats is not None:
            err.code, err.stats = rc, stats
        raise err
    _raise(rc)


class _Handle:
    """Owner of one C handle, ``_h``. A subclass names the entry that frees
    it in ``_destroy``. close() is idempotent, safe on an object whose
    constructor raised before ``_h`` existed, and REPLACES the handle object
    with a fresh null one: get's cached handle arrays compare handle objects
    by identity to notice closed tables."""
    _destroy = ""

    def _free(self, h) -> None:
        getattr(_L(), self._destroy)(h)

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h and h.value:
            self._free(h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- buffers -------------------------------------------------------------------

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


def _stream(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)  # torch.cuda.Stream


def _key_bytes(k) -> bytes:
    return k.encode() if isinstance(k, str) else bytes(k)


def _host_bytes(data):
    """(buffer, length) of a file's bytes: bytes, a uint8 numpy array or a
    uint8 device tensor. The buffer is never empty (the C ABI takes no NULL
    beside a length); the length is the true one."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(bytes(data), np.uint8)
    n = int(data.numel()) if hasattr(data, "numel") else int(len(data))
    return (data if n else np.zeros(1, np.uint8)), n


def _pack(parts) -> "tuple[bytes, np.ndarray]":
    """Ragged byte strings as the C ABI takes them: (the parts joined,
    offsets uint64[n + 1])."""
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return b"".join(parts), off


def _key_parts(names, key_columns) -> np.ndarray:
    """int32[n + 1]: for each column name its index among `key_columns` (the
    schema's key_columns(), src/schema.rs:27-33) or -1, then a 0."""
    kc = [_key_bytes(c) for c in key_columns]
    return np.array([kc.index(c) if c in kc else -1 for c in names] + [0], np.int32)


def _size_then_fill(call, wanted=None) -> "bytes | None":
    """The two-call idiom of the entries that write bytes of a length only
    they know: call(None, 0, n) asks the size, call(buffer, size, n) fills a
    buffer of at least one byte. `call` checks its own status. `wanted`, if
    given, is asked after the first call; on False the result is None."""
    n = ctypes.c_uint64()
    call(None, 0, ctypes.byref(n))
    if wanted is not None and not wanted():
        return None
    out = ctypes.create_string_buffer(max(int(n.value), 1))
    call(out, int(n.value), ctypes.byref(n))
    return out.raw[:n.value]


def _hit_rows(rows: int, n: int, out):
    """(buffer, result) for hit rows of n keys: the caller's `out` as both, or
    a fresh uint64[rows, ceil(n/64)] padded to at least 1 x 1 for the C ABI
    and the view of it to return."""
    if out is not None:
        return out, out
    words = (n + 63) // 64
    buf = np.zeros((max(rows, 1), max(words, 1)), np.uint64)
    return buf, buf[:rows, :words]


# ---- key batches ---------------------------------------------------------------

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
    joined, offs = _pack([_key_bytes(k) for k in keys])
    data = np.frombuffer(joined, np.uint8) if joined else np.zeros(1, np.uint8)
    return KeyBatch(n=len(offs) - 1, data=data, offsets=offs)


def _to_var(b: KeyBatch) -> KeyBatch:
    keys = np.ascontiguousarray(b.keys)
    offs = (np.arange(0, b.key_len * (b.n + 1), b.key_len, dtype=np.uint64) if b.key_len
            else np.zeros(b.n + 1, np.uint64))
    data = keys.reshape(-1) if keys.size else np.zeros(1, np.uint8)
    return KeyBatch(n=b.n, data=data, offsets=offs)


def _call_keys(fixed, var, head, b: KeyBatch, tail) -> None:
    """One call of a cb_*_fixed / cb_*_var pair, chosen by the batch's form:
    fixed(*head, keys, key_len, n, *tail) or var(*head, data, offsets, n,
    *tail). The batch's buffers stay alive until the call has returned."""
    if b.offsets is None:
        kp, k1 = _ptr_of(b.keys)
        rc = fixed(*head, kp, b.key_len, b.n, *tail)
    else:
        dp, k1 = _ptr_of(b.data)
        op, k2 = _ptr_of(b.offsets)
        rc = var(*head, dp, op, b.n, *tail)
    if rc:
        _raise(rc)
