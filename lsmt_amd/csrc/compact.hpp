// compact.hpp — newest-wins merge of well-formed tables into one data file
// (compact.hip; the C ABI's cb_tables_compact).
//
// The reference never merges its tables, so the result is defined through
// the two functions it must be indistinguishable from: for tables T[0..nt),
// T[0] newest, the file is SsTable::create (src/sstable.rs:51-87) of
// { (k, Database::get(k)) : k a key of any line, get(k) is Some }, with
// Database::get (src/lib.rs:128-134) taken over T alone. get keeps the first
// Ok(Some) of the newest-first walk, so a key keeps the line of the newest
// table whose value decodes (vdl != kBadValue), and a key whose value decodes
// nowhere is dropped. A kept line's text is what STANDARD.encode would write
// again, so lines are copied, never re-encoded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flush.hpp"
#include "sstable.hpp"

namespace cb {

// One input table (non-empty, well-formed) and the number of lines before it
// in newest-first order: global line g belongs to the last source whose base
// is <= g.
struct CompactSrc {
  const uint8_t* data;
  const LineRec* rec;
  const uint32_t* llen;
  uint64_t base;
};

// The last i in [0, n) with at(i) <= x (at is non-decreasing, at(0) <= x).
template <class At>
__device__ __forceinline__ uint32_t last_le(uint32_t n, uint64_t x, At at) {
  uint32_t lo = 0, hi = n;  // at(lo) <= x < at(hi) (at(n) = past every x)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (at(mid) <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The source of global line g: the last one whose base is <= g (no two
// sources share a base: every source has lines).
__device__ __forceinline__ uint32_t src_of(const CompactSrc* __restrict__ src, uint32_t nsrc, uint64_t g) {
  return last_le(nsrc, g, [&](uint32_t i) { return src[i].base; });
}

constexpr uint32_t kCompactTile = 256;  // records per select / format block

// The bytes of one tile of survivors written by its whole block (kCompactTile
// lanes, after the barrier behind s_off): o[0 .. tl) where survivor i of nsv
// owns bytes s_off[i] .. s_off[i + 1) (s_off[nsv] = tl; a survivor may own
// none) and byte_at(i, j) is byte j of the tile, which survivor i owns. Bytes
// up to the first 4-aligned address, then aligned dwords assembled across the
// survivors, then the tail. (threadIdx.x is written out at each use: held in
// a local, k_compact_format's allocation grew by two VGPRs.)
template <class ByteAt>
__device__ __forceinline__ void copy_tile_bytes(uint8_t* o, uint64_t tl, uint32_t nsv, const uint64_t* s_off,
                                                ByteAt byte_at) {
  // byte j's survivor: the last with s_off[i] <= j (of equal offsets the last
  // is the one that owns a byte)
  auto owner = [&](uint64_t j) { return last_le(nsv, j, [&](uint32_t i) { return s_off[i]; }); };
  const uint64_t mis = (4 - ((uintptr_t)o & 3)) & 3;
  const uint64_t head = mis < tl ? mis : tl;
  if (threadIdx.x < head) o[threadIdx.x] = (uint8_t)byte_at(owner(threadIdx.x), threadIdx.x);
  const uint64_t body = (tl - head) / 4;
  uint32_t* ow = reinterpret_cast<uint32_t*>(o + head);
  for (uint64_t w = threadIdx.x; w < body; w += kCompactTile) {
    const uint64_t j0 = head + 4 * w;
    uint32_t i = owner(j0), x = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      while (j0 + k >= s_off[i + 1]) ++i;  // (j0 + k < tl = s_off[nsv]: stops at a survivor)
      x |= byte_at(i, j0 + k) << (8 * k);
    }
    ow[w] = x;
  }
  const uint64_t tail0 = head + 4 * body;
  if (tail0 + threadIdx.x < tl) o[tail0 + threadIdx.x] = (uint8_t)byte_at(owner(tail0 + threadIdx.x), tail0 + threadIdx.x);
}

// What the later passes need of input line g once the sort has moved its
// record: where `key \t text` starts, its length (the line without '\n'), the
// key's length and the value's decoded length.
struct CompactSide {
  const uint8_t* src;
  uint32_t llen, klen, vdl, pad;
};

inline uint64_t compact_tiles(uint64_t n) { return n ? (n + kCompactTile - 1) / kCompactTile : 1; }

// klen[g] = the key length of global line g (the scan of these is ko).
hipError_t launch_compact_klen(const CompactSrc* src, uint32_t nsrc, uint64_t n, uint64_t* klen, hipStream_t s);
// The keys of all lines as one ragged batch (kb, ko) in newest-first order
// (a smaller index is a newer line), and side[g]; dmask[kDirPos][4] |= the
// prefix bytes of kDirSample evenly spaced lines (the bin sort's map; the
// caller zeroes it).
hipError_t launch_compact_gather(const CompactSrc* src, uint32_t nsrc, uint64_t n, const uint64_t* ko, uint8_t* kb,
                                 CompactSide* side, uint64_t* dmask, hipStream_t s);
// Over the sorted records (equal keys adjacent, newest first): slen[p] = the
// output line's length (with its '\n') when record p is its key's newest line
// with a decodable value, else 0; per tile of kCompactTile records the number
// of survivors, their line bytes and their key bytes. drop_dead (the live-row
// entries; a compile-time variant of the kernel): such a record survives only
// when its own value is not a tombstone (liverow.hpp) either. A tombstone
// shadows and is then dropped: it still defeats every older line of its key,
// so no older value comes back for a deleted row.
hipError_t launch_compact_select(const SortKey* order, const CompactSide* side, const uint8_t* kb, const uint64_t* ko,
                                 uint64_t n, bool drop_dead, uint64_t* slen, uint64_t* tcnt, uint64_t* tbytes,
                                 uint64_t* tkeys, hipStream_t s);

// Which line of a key a merge keeps. newest: the rule above, by table order
// alone. lww (the LWW entries): the tables stand for replicas, and the
// decodable line with the greatest timestamp wins, the lowest table index
// among equal timestamps (rowts.hpp: the fold of src/cluster.rs:405-416).
// drop_dead: the winner, whichever order chose it, is then dropped when its
// value is a tombstone (liverow.hpp); it has defeated the other lines first.
enum class MergeOrder : uint8_t { newest, lww };
struct MergeRule {
  MergeOrder order;
  bool drop_dead;
};

// ts[g] = the timestamp of gathered line g (rowts.hpp, from the first 11
// characters of its value's text); 0 for a line whose value does not decode
// (never compared). For LWW merges only.
hipError_t launch_compact_ts(const CompactSide* side, uint64_t n, uint64_t* ts, hipStream_t s);
// launch_compact_select's outputs under the LWW order, in two launches: per
// run of equal keys (adjacent in the sorted order, ascending by table index)
// the one decodable record that lww_beats every other decodable one survives
// (drop_dead: unless its own value is a tombstone), every other record of the
// run gets slen 0; then the tile sums of slen.
hipError_t launch_compact_select_lww(const SortKey* order, const CompactSide* side, const uint64_t* ts,
                                     const uint8_t* kb, const uint64_t* ko, uint64_t n, bool drop_dead,
                                     uint64_t* slen, uint64_t* tcnt, uint64_t* tbytes, uint64_t* tkeys,
                                     hipStream_t s);
// The LWW select's second launch alone: the tile sums of slen as it stands,
// for a caller that has cleared survivors behind a select (the ring's
// ownership filter, capi_ring.cpp).
hipError_t launch_compact_tiles(const SortKey* order, const CompactSide* side, const uint64_t* slen, uint64_t n,
                                uint64_t* tcnt, uint64_t* tbytes, uint64_t* tkeys, hipStream_t s);
// From the scanned tile sums: the file (out: the survivors' lines `key \t
// text \n` back to back), its line index without re-reading it (sstable.hpp
// layout: survivor l is line l of nl; vdl carried over from the input's
// index; the directory is built from pfx afterwards), and the survivors' keys
// as a ragged batch (kb2, ko2). totals = {survivors, file bytes, key bytes}
// (device); nl = the survivors (host: read back to size the output).
hipError_t launch_compact_format(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                                 const uint64_t* tcnt, const uint64_t* tbytes, const uint64_t* tkeys,
                                 const uint64_t* totals, uint64_t n, uint64_t nl, uint8_t* out, LineRec* rec,
                                 uint64_t* pfx, uint64_t* fence, uint32_t* llen, uint8_t* kb2, uint64_t* ko2,
                                 hipStream_t s);

}  // namespace cb
