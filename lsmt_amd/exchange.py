"""The sparse hit exchange between GPUs (lsmt_amd/shard.py):
hit rows compressed to packs of set-bit positions and expanded back."""
from __future__ import annotations

import ctypes

from ._ffi import _L, _ptr_of, _raise, _stream
from .shard import PACK_BLOCK_WORDS


def _pack_blocks(nw: int) -> int:
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
