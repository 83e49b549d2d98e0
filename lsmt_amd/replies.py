"""The coordinator's read merge (cb_replies_fold, cb_reply_line): the
replicas' ``key \\t ts \\t val`` replies folded by timestamp into the response
the client gets.

The reference does this at the end of Cluster::execute
(src/cluster.rs:394-473); what goes in is what ScanResult.select(meta=True)
writes on every replica. The rule's text is lsmt_amd/csrc/replyline.hpp's.
Reached as ``lsmt_amd.replies``: nothing here is exported from the package
itself.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from ._ffi import _Handle, _key_bytes, _L, _ptr_of, _raise_text, _stream
from ._lib import check
from .rows import RowsResult

FOLD_TEXT, FOLD_DEAD, FOLD_HOST = 1, 2, 4
MAX_REPLIES = 4096  # replyline.hpp kFoldMaxReplies

FoldRow = namedtuple("FoldRow", "key_at key_len ts val_at val_len reply flags")
ReplyLine = namedtuple("ReplyLine", "kind key_len ts val_at val_len val_flags")


class FoldResult(_Handle):
    """A fold's result (cb_fold_*): the response bytes, the winners in key
    order as places in the folded bytes, and what the fold saw (``stats``, a
    FoldStats). Complete when the call that made it returns; it keeps no copy
    of the replies."""
    _destroy = "cb_fold_destroy"

    def __init__(self, handle: int, device: int):
        self._h = ctypes.c_void_p(handle)
        self.device = device
        self.stats = _lib.FoldStats()
        check(_L().cb_fold_info(self._h, ctypes.byref(self.stats)))

    def copy(self, text=None, key_at=None, key_len=None, ts=None, val_at=None, val_len=None, reply=None,
             flags=None) -> None:
        """Any of text (uint8[stats.bytes]) and the winners' columns (uint64[keys],
        reply uint32[keys], flags uint8[keys]) into numpy arrays or device
        tensors."""
        if text is not None:
            check(_L().cb_fold_text(self._h, _ptr_of(text)[0]))
        cols = (key_at, key_len, ts, val_at, val_len, reply, flags)
        if any(c is not None for c in cols):
            check(_L().cb_fold_rows(self._h, *(_ptr_of(c)[0] for c in cols)))

    def text(self) -> bytes:
        """The response: a JSON array, or the least other line where no reply
        held a row."""
        t = np.zeros(max(int(self.stats.bytes), 1), np.uint8)
        self.copy(text=t)
        return t[:int(self.stats.bytes)].tobytes()

    def rows(self) -> "list[FoldRow]":
        """The winners in key order; offsets point into the folded bytes (the
        replies joined in order)."""
        n = int(self.stats.keys)
        u64 = [np.zeros(max(n, 1), np.uint64) for _ in range(5)]
        rp, fl = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
        self.copy(None, *u64, rp, fl)
        return [FoldRow(*(int(c[i]) for c in u64), int(rp[i]), int(fl[i])) for i in range(n)]

    def other(self):
        """(at, len) of the least other line where it is the response, else None."""
        at, ln = ctypes.c_uint64(), ctypes.c_uint64()
        check(_L().cb_fold_other(self._h, ctypes.byref(at), ctypes.byref(ln)))
        return None if at.value == 0xFFFFFFFFFFFFFFFF else (int(at.value), int(ln.value))


def _joined(replies, device: int):
    """(buffer, offsets uint64[n + 1]) of the replies joined in order: host
    bytes as one numpy array; with any device tensor or RowsResult among them,
    one device tensor."""
    parts = list(replies)
    on_device = any(isinstance(p, RowsResult) or hasattr(p, "data_ptr") for p in parts)
    if not on_device:
        raw = [_key_bytes(p) for p in parts]
        off = np.zeros(len(raw) + 1, np.uint64)
        np.cumsum([len(p) for p in raw], out=off[1:])
        joined = b"".join(raw)
        return (np.frombuffer(joined, np.uint8) if joined else np.zeros(1, np.uint8)), off
    import torch
    dev = f"cuda:{device}"
    tensors = []
    for p in parts:
        if isinstance(p, RowsResult):
            t = torch.empty(max(p.bytes, 1), dtype=torch.uint8, device=dev)
            p.copy(text=t)
            tensors.append(t[:p.bytes])
        elif hasattr(p, "data_ptr"):
            tensors.append(p.reshape(-1).to(dev))
        else:
            b = _key_bytes(p)
            tensors.append(torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev) if b else
                           torch.empty(0, dtype=torch.uint8, device=dev))
    off = np.zeros(len(tensors) + 1, np.uint64)
    np.cumsum([int(t.numel()) for t in tensors], out=off[1:])
    joined = torch.cat(tensors) if tensors and int(off[-1]) else torch.zeros(1, dtype=torch.uint8, device=dev)
    joined = joined.contiguous()
    torch.cuda.current_stream(joined.device).synchronize()  # (joined on torch's stream; the fold may run on another)
    return joined, off


def fold_replies(replies, device: int = 0, stream=None) -> FoldResult:
    """The read's fold over `replies`, in their order (cb_replies_fold): each a
    bytes object, a RowsResult (its text is taken on the device) or a uint8
    device tensor. device=-1 folds on the host by the same rule (host bytes
    only; no device is touched), which is what a point read of a few replicas
    wants. A reply that is not UTF-8 raises UnicodeDecodeError with ``.code``
    and ``.stats``."""
    buf, off = _joined(replies, int(device))
    if device == -1 and hasattr(buf, "data_ptr"):
        raise ValueError("the host fold takes host bytes")
    h, st = ctypes.c_void_p(), _lib.FoldStats()
    rc = _L().cb_replies_fold(_ptr_of(buf)[0], _ptr_of(off)[0], len(off) - 1, int(device), _stream(stream),
                              ctypes.byref(h), ctypes.byref(st))
    if rc:
        _raise_text(rc, st)
    return FoldResult(h.value, int(device))


def reply_line(piece, terminated: bool = True) -> ReplyLine:
    """The rule's verdict of one piece of a reply on the host (cb_reply_line):
    kind 0 ignored, 1 an entry, 2 an other, or CB_EUTF8."""
    p = _key_bytes(piece)
    kind, fl = ctypes.c_int(), ctypes.c_uint8()
    kl, ts, va, vl = (ctypes.c_uint64() for _ in range(4))
    check(_L().cb_reply_line(p, len(p), int(bool(terminated)), ctypes.byref(kind), ctypes.byref(kl), ctypes.byref(ts),
                             ctypes.byref(va), ctypes.byref(vl), ctypes.byref(fl)))
    return ReplyLine(int(kind.value), int(kl.value), int(ts.value), int(va.value), int(vl.value), int(fl.value))
