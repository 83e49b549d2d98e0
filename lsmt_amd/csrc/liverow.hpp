// liverow.hpp — which decoded values are deleted rows (host and device).
//
// The reference deletes a row by writing a tombstone: exec_delete inserts the
// 8-byte timestamp with an empty payload (src/query.rs:240-261), and every
// reader of a scan splits the timestamp off and skips a value without payload
// (split_ts and its callers, src/query.rs:21-27, 343-346, 395-398). split_ts
// returns the bytes themselves below 8 and strips 8 from there on, so the
// payload is empty at exactly two lengths.
//
// This is the rule's one home in the library: the live-row entries
// (cb_tables_count, cb_tables_scan_live, cb_tables_compact_live) ask here and
// nothing restates it. It looks at a line's own length only; which line
// decides a key's fate (its newest decodable one, dead or not) is the merge's
// select (compact.hpp).
#pragma once
#include <stdint.h>

namespace cb {

// Whether a value of decoded length vdl is dead: split_ts leaves no payload.
// The index's mark for a value that does not decode (kBadValue, sstable.hpp)
// is neither dead nor live (such a line is no entry at all) and callers test
// it first; here it is simply not dead.
constexpr bool value_dead(uint32_t vdl) { return vdl == 0 || vdl == 8; }

}  // namespace cb
