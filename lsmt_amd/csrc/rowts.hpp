// rowts.hpp — a row's write timestamp and the last-write-wins rule over it
// (host and device).
//
// Every value the reference stores begins with the 8-byte big-endian
// timestamp its coordinator stamped (insert_ns_ts, src/lib.rs:154-158);
// split_ts (src/query.rs:21-27) takes it off again: 0 below 8 bytes, else the
// first 8 as an unsigned big-endian u64. The cluster's read folds its
// replicas' rows with "keep the current row if cur_ts >= ts, else replace"
// (src/cluster.rs:405-416), replica 0 first: the greatest timestamp wins and,
// among equal ones, the replica asked first.
//
// This is the rule's one home in the library: the LWW entries
// (cb_tables_compact_lww, cb_tables_scan_lww, cb_tables_count_lww,
// cb_scan_ts) ask here and nothing restates it. Which lines take part (the
// decodable ones) and what happens to a winner without payload (liverow.hpp)
// is the merge's select (compact.hpp).
#pragma once
#include <stdint.h>

namespace cb {

// The 6 bits of one character of the STANDARD alphabet (A-Z a-z 0-9 + /).
constexpr uint64_t b64_sextet(uint8_t c) {
  return c >= 'a' ? c - 'a' + 26u : c >= 'A' ? c - 'A' + 0u : c >= '0' ? c - '0' + 52u : c == '+' ? 62u : 63u;
}

// Its inverse: the character of 6 bits v < 64 (what STANDARD.encode writes;
// rowwrite.hpp's log records. The flush keeps its own in flush.hip.)
constexpr uint8_t b64_char(uint32_t v) {
  return (uint8_t)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/');
}

// split_ts(value).0 of decoded bytes p[0..len).
constexpr uint64_t decoded_ts(const uint8_t* p, uint64_t len) {
  if (len < 8) return 0;
  uint64_t v = 0;
  for (uint32_t j = 0; j < 8; ++j) v = v << 8 | p[j];
  return v;
}

// The same through a byte source over the decoded value (rowjson.hpp's
// sources: size(), seek(), next()), which is left at the payload's first byte:
// split_ts's second half begins there.
template <class Src>
constexpr uint64_t source_ts(Src& value) {
  const bool has = value.size() >= 8;
  value.seek(0);
  uint64_t v = 0;
  for (uint32_t j = 0; has && j < 8; ++j) v = v << 8 | value.next();
  return v;
}

// The same from a value's base64 text, vdl its decoded length (the line
// index's; not kBadValue: callers test that first). Such a text is valid
// STANDARD base64 and holds at least 12 characters when vdl >= 8, so its
// first 11 are alphabet characters, no padding: 66 bits, of which the top 64
// are the timestamp. Nothing is read when vdl < 8.
constexpr uint64_t value_ts(const uint8_t* text, uint32_t vdl) {
  if (vdl < 8) return 0;
  uint64_t v = 0;
  for (uint32_t j = 0; j < 10; ++j) v = v << 6 | b64_sextet(text[j]);
  return v << 4 | b64_sextet(text[10]) >> 2;
}

// Whether line a (timestamp ts_a, at place idx_a of the replica order: a
// smaller place is asked earlier) wins against line b, idx_a != idx_b:
// src/cluster.rs:405-416's fold keeps the greater timestamp, and of equal
// ones the row it met first.
constexpr bool lww_beats(uint64_t ts_a, uint64_t idx_a, uint64_t ts_b, uint64_t idx_b) {
  return ts_a != ts_b ? ts_a > ts_b : idx_a < idx_b;
}

// The same fold taken one row at a time, as src/cluster.rs:405-416 runs it:
// whether the row met now (ts, at place idx) replaces the row kept so far.
// The host fold of the replicas' replies (replyfold.hpp) asks here.
constexpr bool lww_replaces(uint64_t kept_ts, uint64_t kept_idx, uint64_t ts, uint64_t idx) {
  return lww_beats(ts, idx, kept_ts, kept_idx);
}

}  // namespace cb
