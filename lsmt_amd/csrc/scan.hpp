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
// the value spans the read path's decode (b64decode.hip) takes. A batched
// scan (cb_tables_scan_many) is the same chain over the cuts of many pairwise
// disjoint, ascending ranges at once: the sorted survivors fall into the
// ranges in order, and k_scan_range_off finds where each range's begin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact.hpp"
#include "flush.hpp"
#include "rowjson.hpp"
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

// One range of a scan (cb_tables_scan_many takes many): its bounds lie in one
// block of bytes staged in device memory (with 16 bytes of padding after the
// last), lo's at [lo_at, lo_at + lo_len), hi's at [hi_at, hi_at + hi_len).
// lo_len == 0: from the first key; !has_hi: unbounded above.
struct ScanRange {
  uint64_t lo_at, lo_len, hi_at, hi_len;
  uint32_t has_hi, pad;
};

// A table cut to the range: lines [first, last) (last >= first), and the byte
// span of those lines in the file, which bounds their keys' bytes.
struct ScanCut {
  uint64_t first, last, bytes;
};

// cut[r * nt + t] for ranges rng[0..nr) (device; offsets into bytes) and
// tables tab[0..nt): the lower bounds (the first line whose key is >= the
// bound) of lo_r and of hi_r, every range, table and bound in one launch.
// Sixteen lanes share one search: they read one run of at most 16 entries per
// fence level together, then settle the lines that share the bound's 8-byte
// prefix by record compares (pfx2, klen, and the file's bytes past 16).
hipError_t launch_scan_bounds(const ScanTable* tab, uint32_t nt, const ScanRange* rng, uint32_t nr,
                              const uint8_t* bytes, ScanCut* cut, hipStream_t s);
// The nr * nt cuts as compaction's sources (compact.hpp), in the cuts' order
// (range-major, the tables newest first inside a range): empty cuts are
// dropped, so no two sources share a base; src_tab[i] = the index in the
// caller's list of source i's table, src_rng[i] = its range. The ranges are
// pairwise disjoint and ascend (keyrange.hpp's ordering rule), so a table's
// cuts share no line, a key's lines all lie in one range, and the sort's
// "input index last" leaves them newest first. totals = {lines in the ranges,
// their byte spans' sum, sources}.
hipError_t launch_scan_sources(const ScanTable* tab, const ScanCut* cut, uint32_t nt, uint32_t nr, CompactSrc* src,
                               uint32_t* src_tab, uint32_t* src_rng, uint64_t* totals, hipStream_t s);
// Over the sorted records and launch_compact_select's scanned tile sums
// (tcnt, tkeys; totals = {survivors, line bytes, key bytes}): survivor r <
// count (count <= the survivors: the scan's limit) gets its key at keys +
// key_off[r] (key_off[count] = the end), which[r] = its table's index in the
// caller's list, and vsrc[r] / dlen[r] = its value's base64 text and decoded
// length; vsum[r / kDecodeTile] += dlen[r] (the caller zeroes vsum):
// launch_b64_decode's inputs. rid (nullable: a scan of one range has no use
// for it): rid[r] = the range of survivor r's source, non-decreasing in r.
hipError_t launch_scan_emit(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                            const uint64_t* tcnt, const uint64_t* tkeys, const uint64_t* totals,
                            const CompactSrc* src, const uint32_t* src_tab, const uint32_t* src_rng, uint32_t nsrc,
                            uint64_t n, uint64_t count, uint8_t* keys, uint64_t* key_off, int32_t* which,
                            uint32_t* rid, uint64_t* vsrc, uint64_t* dlen, uint64_t* vsum, hipStream_t s);
// range_off[r] for r in [0, nr]: the first entry whose range is >= r (the
// lower bound of r in the non-decreasing rid[0..count)), so range r's entries
// are [range_off[r], range_off[r + 1]), range_off[0] = 0, range_off[nr] = count.
hipError_t launch_scan_range_off(const uint32_t* rid, uint64_t count, uint32_t nr, uint64_t* range_off, hipStream_t s);
// Counts without a result (cb_tables_count), over the sorted records and the
// plain launch_compact_select's slen: cnt[2 r] += the survivors whose source
// lies in range r (the entries a scan of r returns), cnt[2 r + 1] += those of
// them whose value is not dead (liverow.hpp). The caller zeroes cnt (2 nr
// words). src_rng as launch_scan_sources left it (not read when nr == 1).
hipError_t launch_scan_count(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                             const CompactSrc* src, const uint32_t* src_rng, uint32_t nsrc, uint64_t n, uint32_t nr,
                             uint64_t* cnt, hipStream_t s);
// ts[i] = the timestamp (rowts.hpp: split_ts's first half) of entry i of a
// finished result, from its decoded value vals[val_off[i] .. val_off[i + 1]):
// 0 below 8 bytes (cb_scan_ts).
hipError_t launch_scan_ts(const uint64_t* val_off, const uint8_t* vals, uint64_t count, uint64_t* ts, hipStream_t s);
// launch_scan_count with a predicate (cb_tables_count_where): cnt[3 r] and
// cnt[3 r + 1] as launch_scan_count's two, cnt[3 r + 2] += the live ones whose
// row matches w (rowjson.hpp), the key's parts taken after skip[r] bytes
// (skip nullable: zeros). The caller zeroes cnt (3 nr words). A live
// survivor's value text is read in place, at side[g].src + klen + 1.
hipError_t launch_scan_count_where(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                                   const CompactSrc* src, const uint32_t* src_rng, uint32_t nsrc, uint64_t n,
                                   uint32_t nr, const WherePred* w, const uint32_t* skip, uint64_t* cnt,
                                   hipStream_t s);
// flags[i] = whether entry i of a finished result matches w (cb_scan_match),
// 0 for a dead entry. skip (nullable: zeros) is per range, and range_off
// (nr + 1 offsets, device; read only with skip) says which range an entry is of.
hipError_t launch_scan_match(const uint64_t* key_off, const uint8_t* keys, const uint64_t* val_off,
                             const uint8_t* vals, uint64_t count, const uint64_t* range_off, const uint32_t* skip,
                             uint32_t nr, const WherePred* w, uint8_t* flags, hipStream_t s);

}  // namespace cb
