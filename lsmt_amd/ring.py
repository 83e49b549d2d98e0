"""The token ring on the device (cb_ring_*, cb_scan_route,
cb_tables_compact_ring): which node holds which row.

The reference places rows with a murmur3 token ring (Cluster::new,
src/cluster.rs:46-54) and asks it with replicas_for (src/cluster.rs:102-123)
about the partition keys of a statement (src/query.rs:448-528, 697-713,
734-760). The rule's text is lsmt_amd/csrc/ring.hpp's. Reached as
``lsmt_amd.ring``: nothing here is exported from the package itself.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _lib
from ._ffi import KeyBatch, _call_keys, _Handle, _key_bytes, _L, _pack, _ptr_of, _raise, _stream, as_batch
from ._lib import check
from .rows import _per_range, _text_buffer
from .table import Table, _compact

LDS_POSITIONS = 2048  # ring.hpp kRingLdsPositions: a larger ring is searched in global memory


class Ring(_Handle):
    """An immutable token ring over `nodes` (names, in Cluster::new's order:
    the own node last), `vnodes` positions a node and `rf` replicas a token
    (each acts as 1 when 0). Nodes are known by their index in `nodes`."""
    _destroy = "cb_ring_destroy"

    def __init__(self, nodes, vnodes: int = 8, rf: int = 1, _handle=None):
        if _handle is None:
            names = [_key_bytes(x) for x in nodes]
            joined, off = _pack(names)
            buf = _text_buffer(joined)
            h = ctypes.c_void_p()
            _raise(_L().cb_ring_create(ctypes.addressof(buf), _ptr_of(off)[0], len(names), int(vnodes), int(rf),
                                       ctypes.byref(h)))
            _handle = h.value
        self._h = ctypes.c_void_p(_handle)
        nn, r, w, pos = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        check(_L().cb_ring_info(self._h, ctypes.byref(nn), ctypes.byref(r), ctypes.byref(pos), ctypes.byref(w)))
        self._info = (int(nn.value), int(r.value), int(w.value), int(pos.value))

    @classmethod
    def from_tokens(cls, tokens, owners, nnodes: int, rf: int = 1) -> "Ring":
        """The ring of explicit (token, owner) pairs, inserted in order: a later
        pair replaces an earlier one of the same token."""
        t = np.ascontiguousarray(np.asarray(tokens, np.uint64).astype(np.uint32))
        o = np.ascontiguousarray(np.asarray(owners, np.uint64).astype(np.uint32))
        if t.shape != o.shape or t.ndim != 1:
            raise ValueError("one owner per token")
        t1, o1 = (t, o) if len(t) else (np.zeros(1, np.uint32), np.zeros(1, np.uint32))
        h = ctypes.c_void_p()
        _raise(_L().cb_ring_create_tokens(_ptr_of(t1)[0], _ptr_of(o1)[0], len(t), int(nnodes), int(rf),
                                          ctypes.byref(h)))
        return cls(None, _handle=h.value)

    nnodes = property(lambda self: self._info[0])
    rf = property(lambda self: self._info[1])
    width = property(lambda self: self._info[2], doc="min(rf, the nodes that hold a position): a list's entries")
    positions = property(lambda self: self._info[3], doc="the ring's distinct tokens")

    def tokens(self):
        """(tokens uint32[positions], owners uint32[positions]), ascending by token."""
        t, o = np.zeros(self.positions, np.uint32), np.zeros(self.positions, np.uint32)
        check(_L().cb_ring_tokens(self._h, _ptr_of(t)[0], _ptr_of(o)[0]))
        return t, o

    def replicas(self, key, skip: int = 0, npk: int = 0):
        """(token, [node, ...]) of one key on the host (cb_ring_replicas):
        replicas_for of its partition key, the primary first, `width` nodes."""
        k = _key_bytes(key)
        tok, reps = ctypes.c_uint32(), np.zeros(self.rf, np.int32)
        check(_L().cb_ring_replicas(self._h, k, len(k), int(skip), int(npk), ctypes.byref(tok), _ptr_of(reps)[0]))
        return int(tok.value), [int(x) for x in reps[:self.width]]

    def route(self, keys, skip: int = 0, npk: int = 0, stream=None):
        """The batched replicas() on the device (cb_ring_route_*): (tokens
        uint32[n], replicas int32[n, rf], -1 past `width`). Keys as the probes
        take them. Host keys give numpy arrays and the call waits; a batch of
        device tensors gives device tensors, filled asynchronously on
        `stream`."""
        return _route(self, as_batch(keys), skip, npk, stream, True, True)


def _route(ring: Ring, b: KeyBatch, skip, npk, stream, want_tokens: bool, want_replicas: bool):
    """route() with either output left out (None in its place)."""
    src = b.keys if b.offsets is None else b.data
    device = 0
    if hasattr(src, "is_cuda") and src.is_cuda:
        import torch
        device = src.device.index or 0
        tok = torch.empty(max(b.n, 1), dtype=torch.uint32, device=src.device) if want_tokens else None
        rep = torch.empty((max(b.n, 1), ring.rf), dtype=torch.int32, device=src.device) if want_replicas else None
    else:
        tok = np.zeros(max(b.n, 1), np.uint32) if want_tokens else None
        rep = np.full((max(b.n, 1), ring.rf), -1, np.int32) if want_replicas else None
    _call_keys(_L().cb_ring_route_fixed, _L().cb_ring_route_var, (ring._h,), b,
               (int(skip), int(npk), device, _ptr_of(tok)[0], _ptr_of(rep)[0], _stream(stream)))
    return (tok[:b.n] if want_tokens else None), (rep[:b.n] if want_replicas else None)


def route_scan(result, ring: Ring, skip=None, npk=None):
    """route() over a ScanResult's keys on its device (cb_scan_route): (tokens
    uint32[count], replicas int32[count, rf]) as numpy arrays. skip and npk:
    one number for all ranges of the result or one per range (default 0)."""
    per = lambda x: None if x is None else np.ascontiguousarray(_per_range(x, result.nranges) + [0], np.uint32)  # noqa: E731
    sk, pk = per(skip), per(npk)
    tok, rep = np.zeros(max(result.count, 1), np.uint32), np.full((max(result.count, 1), ring.rf), -1, np.int32)
    check(_L().cb_scan_route(result._h, ring._h, _ptr_of(sk)[0], _ptr_of(pk)[0], _ptr_of(tok)[0], _ptr_of(rep)[0]))
    return tok[:result.count], rep[:result.count]


class _Rules:
    """A cb_key_rules built from (prefix, npk) pairs, sorted by prefix; keeps
    the arrays it points into alive."""

    def __init__(self, rules):
        pairs = sorted((_key_bytes(p), int(n)) for p, n in (rules.items() if hasattr(rules, "items") else rules))
        joined, self.off = _pack([p for p, _ in pairs])
        self.prefixes = _text_buffer(joined)
        self.npk = np.array([n for _, n in pairs] + [0], np.uint32)
        self.c = _lib.KeyRules(ctypes.addressof(self.prefixes), self.off.ctypes.data, self.npk.ctypes.data, len(pairs))

    def ref(self):
        return ctypes.addressof(self.c)


def compact_ring(tables: Sequence[Table], ring: Ring, node: int, rules=(), m: int = 1024, ranks: int = 0,
                 lww: bool = False, drop_dead: bool = False, stream=None):
    """compact() (or, with lww, compact_lww()) cut down to what `node` owns
    (cb_tables_compact_ring): the compaction a node runs after the ring
    changed, or to cut what a joining node must receive. `rules` maps a key
    prefix (a namespace and its separator) to the number of key columns that
    make its partition key; a key under prefix p is kept when `node` is among
    the first `ranks` of its replicas (0: all rf), its partition key taken
    after len(p) bytes; a key under no prefix, such as a catalog row, is kept
    by every node. drop_dead as in compact_live / compact_lww, with their
    caller's rule. Returns (Table, BloomFilter, ZoneMap) as compact does."""
    r = _Rules(rules)
    return _compact(_L().cb_tables_compact_ring, tables, stream, int(m), ring._h, int(node), int(ranks), r.ref(),
                    int(bool(lww)), int(bool(drop_dead)))
