// replay.hpp — the write-ahead log's records as the newest-wins merge's input
// (replay.hip; the C ABI's cb_log_replay).
//
// Database::new inserts the log's records into the memtable in log order
// (src/lib.rs:35-39), so of a key's records the last stands, and the flush
// that follows writes SsTable::create of the memtable's sorted scan
// (src/sstable.rs:51-87). A record is a table line already (logline.hpp), so
// a replay is a compaction of one unsorted file with duplicates: the entries'
// keys are gathered newest first (the last record gets index 0), the stable
// key sort leaves a key's records adjacent in that order, compaction's select
// keeps the first of each run and its format copies the lines (compact.hpp).
// What is new is the validation in front: the first piece in log order whose
// key is not UTF-8 or whose text is not base64 fails the whole log.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact.hpp"
#include "sstable.hpp"

namespace cb {

// The first bad piece as one word an atomicMin orders: the piece's index among
// the non-empty pieces, then the kind (key before value, though a piece has
// one verdict). All-ones: none.
constexpr uint64_t kLogNoBad = ~0ull;
__host__ __device__ inline uint64_t log_bad_pack(uint64_t piece, bool value) { return piece << 1 | (value ? 1 : 0); }
inline uint64_t log_bad_piece(uint64_t w) { return w >> 1; }
inline bool log_bad_is_value(uint64_t w) { return w & 1; }

// Per piece l of nl (rec / llen as launch_line_finish left them; *err its
// 4-GiB flag: nothing is read when it is up): has[l] = the piece is an entry
// by logline.hpp's verdict (a piece with a TAB that fails it counts too: the
// call fails anyway), klen[l] = its key's bytes, vdl[l] = its value's decoded
// length (kBadValue otherwise); *bad = min(*bad, log_bad_pack of a failing
// piece) (the caller sets it to kLogNoBad).
hipError_t launch_log_mark(const uint8_t* data, const LineRec* rec, const uint32_t* llen, uint64_t nl,
                           const uint32_t* err, uint64_t* has, uint64_t* klen, uint32_t* vdl, uint64_t* bad,
                           hipStream_t s);
// From the exclusive scans of has / klen (nl + 1 entries each; E entries with
// K key bytes): the entries' keys as a ragged batch (kb, ko) in reverse log
// order (entry e of E is key E-1-e, so a smaller index is a later record),
// side[E-1-e] as launch_compact_gather writes it, and dmask |= the prefix
// bytes of kDirSample evenly spaced pieces (the bin sort's map; the caller
// zeroes it; a piece that is no entry samples as the empty key).
hipError_t launch_log_gather(const uint8_t* data, const LineRec* rec, const uint32_t* llen, const uint32_t* vdl,
                             uint64_t nl, const uint64_t* has_scan, const uint64_t* len_scan, uint8_t* kb,
                             uint64_t* ko, CompactSide* side, uint64_t* dmask, hipStream_t s);

}  // namespace cb
