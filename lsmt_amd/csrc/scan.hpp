// scan.hpp — range and prefix scans over well-formed tables (scan.hip; the C
// ABI's cb_tables_scan).
//
// The reference scans its memtable alone (Database::scan / scan_ns,
// src/lib.rs:144-146, 178-186), so the scan of the tables is defined the way
// compaction is (compact.hpp): for tables T[0..nt), T[0] newest, and a byte
// range [lo, hi) it is, sorted by key bytes,
//   { (k, Database::get(k)) : k a key of any line, lo <= k < hi, get(k) is Some }
// with Database::get (src/lib.rs:128-134) taken over T alone and the values
// decoded. It is compaction's merge over the tables cut to the range: each
// table's lower bounds of lo and hi first (k_scan_bounds), the cut tables as
// compaction's sources (k_scan_sources), then compaction's own gather, sort
// and select, and an emit pass (k_scan_emit) that writes keys, sources and
// the value spans the read path's decode (b64decode.hip) takes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact.hpp"
#include "flush.hpp"
#include "sstable.hpp"

namespace cb {

// One input table (non-empty, well-formed): its file and line index, and its
// position in the caller's table list.
struct ScanTable {
  const uint8_t* data;
  const LineRec* rec;
  const uint64_t* pfx;
  const uint64_t* fence;
  const uint32_t* llen;
  uint64_t nlines, len;
  uint32_t index, pad;
};

// The range's bounds in device memory: lo's bytes at bytes[0 .. lo_len), hi's
// at bytes[hi_at .. hi_at + hi_len). lo_len == 0: from the first key;
// !has_hi: unbounded above.
struct ScanRange {
  const uint8_t* bytes;
  uint64_t lo_len, hi_at, hi_len;
  uint32_t has_hi, pad;
};

// A table cut to the range: lines [first, last) (last >= first), and the byte
// span of those lines in the file, which bounds their keys' bytes.
struct ScanCut {
  uint64_t first, last, bytes;
};

// cut[t] for tables tab[0..nt): the lower bounds (the first line whose key is
// >= the bound) of lo and of hi, every table and both bounds in one launch.
// Sixteen lanes share one search: they read one run of at most 16 entries per
// fence level together, then settle the lines that share the bound's 8-byte
// prefix by record compares (pfx2, klen, and the file's bytes past 16).
hipError_t launch_scan_bounds(const ScanTable* tab, uint32_t nt, const ScanRange& range, ScanCut* cut, hipStream_t s);
// The cut tables as compaction's sources (compact.hpp): tables whose cut is
// empty are dropped, so no two sources share a base; src_tab[i] = the index
// in the caller's list of source i's table. totals = {lines in the range,
// their byte spans' sum, sources}.
hipError_t launch_scan_sources(const ScanTable* tab, const ScanCut* cut, uint32_t nt, CompactSrc* src,
                               uint32_t* src_tab, uint64_t* totals, hipStream_t s);
// Over the sorted records and launch_compact_select's scanned tile sums
// (tcnt, tkeys; totals = {survivors, line bytes, key bytes}): survivor r <
// count (count <= the survivors: the scan's limit) gets its key at keys +
// key_off[r] (key_off[count] = the end), which[r] = its table's index in the
// caller's list, and vsrc[r] / dlen[r] = its value's base64 text and decoded
// length; vsum[r / kDecodeTile] += dlen[r] (the caller zeroes vsum):
// launch_b64_decode's inputs.
hipError_t launch_scan_emit(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                            const uint64_t* tcnt, const uint64_t* tkeys, const uint64_t* totals,
                            const CompactSrc* src, const uint32_t* src_tab, uint32_t nsrc, uint64_t n, uint64_t count,
                            uint8_t* keys, uint64_t* key_off, int32_t* which, uint64_t* vsrc, uint64_t* dlen,
                            uint64_t* vsum, hipStream_t s);

}  // namespace cb
