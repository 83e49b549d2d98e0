// logline.hpp — what one piece of the write-ahead log is (host and device).
//
// The reference replays its log in Wal::new (src/wal.rs:14-31, parse_entries):
// the bytes are split on '\n', an empty piece is skipped, a piece without a
// TAB is skipped without being looked at, and of any other piece the bytes
// before the first TAB must be UTF-8 (std::str::from_utf8, the key) and the
// bytes after it, to the piece's end, must be accepted by base64 0.21.7
// STANDARD.decode (the value; a second TAB is one more character of that text
// and fails it). The key is checked before the value (the `?` order of
// src/wal.rs:21-26), and the first failing piece in log order is the error of
// the whole log: Database::new returns Err (src/lib.rs:35,
// tests/wal_error_test.rs:19). '\r' is a byte like any other. The writer is
// insert_internal (src/lib.rs:96-102): `key \t STANDARD.encode(value)`, which
// Wal::append ends with '\n', so a record is byte for byte a table line.
//
// This is the rule's one home in the library: cb_log_replay's k_log_mark
// (replay.hip), cb_log_line and SsTable::load's key check (sstable.hip, which
// shares utf8_valid) ask here and nothing restates it. The value's verdict is
// the one LineRec::vdl records for a table line (tablebytes.hpp b64_len, which
// reads a table's padded buffer eight bytes at a time); here it is stated
// over a byte source, any p with p[i], so the host can ask it of a piece in a
// block of exactly its size.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CB_LOG_HD __host__ __device__
#else
#define CB_LOG_HD
#endif

namespace cb {

// A piece's kind: skipped (no TAB), an entry, or the error it is.
constexpr int kLogSkipped = 0, kLogEntry = 1, kLogBadKey = -7 /* CB_EUTF8 */, kLogBadValue = -8 /* CB_EBASE64 */;

// Rust's str::from_utf8 acceptance (Unicode well-formed sequences: no
// overlongs, no surrogates, nothing above U+10FFFF).
template <class Src>
CB_LOG_HD inline bool utf8_valid(Src p, uint64_t n) {
  uint64_t i = 0;
  while (i < n) {
    const uint32_t c = p[i];
    if (c < 0x80) {
      ++i;
      continue;
    }
    uint32_t len, lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) len = 2;
    else if (c == 0xE0) { len = 3; lo = 0xA0; }
    else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) len = 3;
    else if (c == 0xED) { len = 3; hi = 0x9F; }
    else if (c == 0xF0) { len = 4; lo = 0x90; }
    else if (c >= 0xF1 && c <= 0xF3) len = 4;
    else if (c == 0xF4) { len = 4; hi = 0x8F; }
    else return false;
    if (n - i < len) return false;
    if (p[i + 1] < lo || p[i + 1] > hi) return false;
    for (uint32_t k = 2; k < len; ++k)
      if (p[i + k] < 0x80 || p[i + k] > 0xBF) return false;
    i += len;
  }
  return true;
}

// The STANDARD alphabet's value of a character, -1 outside it.
CB_LOG_HD inline int log_b64_value(uint32_t c) {
  if (c - 'A' < 26u) return (int)(c - 'A');
  if (c - 'a' < 26u) return (int)(c - 'a') + 26;
  if (c - '0' < 10u) return (int)(c - '0') + 52;
  return c == '+' ? 62 : c == '/' ? 63 : -1;
}

// base64 0.21.7 STANDARD.decode of text[0..len): the decoded length, or -1
// where it returns Err. Whole quads only (padding is required, so a length
// that is no multiple of 4 fails whatever it holds), at most two '=' and only
// at the very end, and the bits the last quad does not use must be zero.
template <class Src>
CB_LOG_HD inline int64_t b64_text_len(Src text, uint64_t len) {
  if (len & 3) return -1;
  if (!len) return 0;
  const uint32_t pad = text[len - 1] == '=' ? (text[len - 2] == '=' ? 2 : 1) : 0;
  const uint64_t body = len - pad;
  int last = 0;
  for (uint64_t i = 0; i < body; ++i) {
    last = log_b64_value(text[i]);
    if (last < 0) return -1;
  }
  if (pad == 2 && (last & 0x0F)) return -1;
  if (pad == 1 && (last & 0x03)) return -1;
  return (int64_t)(len / 4 * 3 - pad);
}

// One non-empty piece: kind, and for an entry the key's length and the value's
// decoded length (tab = klen, the first TAB's place; both 0 otherwise).
struct LogLine {
  int kind;
  uint64_t klen, vdl;
};

// The verdict of a piece whose first TAB is known (tab == len: it has none).
template <class Src>
CB_LOG_HD inline LogLine log_line_at(Src p, uint64_t len, uint64_t tab) {
  if (tab >= len) return LogLine{kLogSkipped, 0, 0};
  if (!utf8_valid(p, tab)) return LogLine{kLogBadKey, 0, 0};
  const int64_t d = b64_text_len(p + (tab + 1), len - tab - 1);
  if (d < 0) return LogLine{kLogBadValue, 0, 0};
  return LogLine{kLogEntry, tab, (uint64_t)d};
}

// The verdict of piece p[0..len) (no '\n' inside: the caller split the log).
template <class Src>
CB_LOG_HD inline LogLine log_line(Src p, uint64_t len) {
  uint64_t tab = 0;
  while (tab < len && p[tab] != '\t') ++tab;
  return log_line_at(p, len, tab);
}

}  // namespace cb
