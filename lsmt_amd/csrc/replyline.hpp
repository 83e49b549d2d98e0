// replyline.hpp — what one line of a replica's reply is to the coordinator of
// a read, and what the winning row's text becomes in the response (host and
// device, no HIP dependency).
//
// The reference's cluster read ends in Cluster::execute (src/cluster.rs:394-473,
// is_write false): every replica's reply is taken as text
// (String::from_utf8_lossy), split with str::lines(), each line cut with
// splitn(3, '\t') into key, timestamp and val, the timestamp read with
// str::parse::<u64>().unwrap_or(0), and per key the row with the greatest
// timestamp kept, of equal ones the row met first (rowts.hpp lww_beats is that
// fold). The winners are walked in key order (a BTreeMap<String, _>), a winner
// with an empty val is a deleted row and left out, every other val goes
// through serde_json::from_str::<Value> and the values that parse are written
// as one JSON array. A line with fewer than two TABs goes into a BTreeSet of
// others; when no line had two TABs the least of them is the response (a
// forwarded COUNT(*) travels so), and `[]` when there is none either.
//
// This is the rule's one home in the library: k_reply_mark and k_fold_size
// (fold.hip), cb_replies_fold's host fold, cb_reply_line and the stand-alone
// driver (tests/cpp/replyline_driver.cpp) ask here and nothing restates it.
// Like rowjson.hpp it is a restatement of Rust's and serde_json's documented
// behaviour, checked against an independent Python restatement
// (tests/fold_ref.py), and NOT run against the reference itself.
//
// Replies: in the caller's order (the reference's is a HashSet's, so the
// caller's order is the order). A reply must be UTF-8 by utf8_valid
// (logline.hpp); the lossy replacement is left to the host, and the first
// reply in order with an invalid piece fails the fold ('\n' and '\t' are
// ASCII, so checking per piece is checking the reply).
//
// Lines: str::lines() of each reply by itself. The reply is split at '\n'; a
// piece that ended at a '\n' loses one trailing '\r'; the last piece of a
// reply without a final '\n' keeps its '\r' (current std behaviour: only the
// "\r\n" pair is a line ending); nothing is yielded after a final '\n'.
// Replies are never joined. A line that is empty after the strip is ignored.
//
// Entry: a line with at least two TABs. key = the bytes before the first (it
// may be empty), the timestamp's text lies between the first and the second,
// val is everything behind the second, further TABs included.
// ts: an optional single '+', then one or more ASCII digits and nothing else,
// any number of leading zeros, at most 2^64 - 1; everything else (empty, '+'
// alone, '-', spaces, other digits, 0x..., a greater value) is 0.
// Other: a non-empty line with fewer than two TABs.
//
// A winner's val: empty is a deleted row (kFoldDead). A val in canonical form
// is copied byte for byte (kFoldText): for it from_str::<Value> followed by
// to_vec is the identity. Canonical: an object of strings by rowjson.hpp's
// grammar, no whitespace anywhere, names strictly ascending bytewise as
// unescaped (serde_json's Map is a BTreeMap without preserve_order), every
// string written as rowselect.hpp (4) says serde_json writes it: of the
// escapes only \" \\ \b \f \n \r \t and \u00xx in lower-case hex, and only for
// the bytes that need them. `{}` is canonical. Every other non-empty val is kFoldHost: it
// may be invalid JSON, which the reference drops, or valid JSON that
// serialises differently; the device does not decide it.
#pragma once
#include <stdint.h>

#include "logline.hpp"
#include "rowts.hpp"

namespace cb {

constexpr int kReplyIgnored = 0, kReplyEntry = 1, kReplyOther = 2, kReplyBadUtf8 = -7 /* CB_EUTF8 */;
constexpr uint8_t kFoldText = 1, kFoldDead = 2, kFoldHost = 4;  // CB_FOLD_*
constexpr uint32_t kFoldMaxReplies = 4096;

// str::lines()'s strip of a piece of `len` bytes: its length as a line.
template <class Src>
CB_LOG_HD inline uint64_t reply_strip(Src p, uint64_t len, bool terminated) {
  return terminated && len && p[len - 1] == '\r' ? len - 1 : len;
}

// str::parse::<u64>().unwrap_or(0) of text[0..n).
template <class Src>
CB_LOG_HD inline uint64_t reply_ts(Src text, uint64_t n) {
  uint64_t i = n && text[0] == '+' ? 1 : 0, v = 0;
  if (i == n) return 0;
  for (; i < n; ++i) {
    const uint64_t d = (uint64_t)text[i] - '0';
    if (text[i] < '0' || text[i] > '9' || v > (~0ull - d) / 10) return 0;  // (v * 10 + d > 2^64 - 1)
    v = v * 10 + d;
  }
  return v;
}

// One piece of a reply: its kind, its length as a line and, for an entry,
// where its two TABs are and its timestamp (val = line[tab2 + 1 .. len)).
struct ReplyLine {
  int kind;
  uint64_t len, tab1, tab2, ts;
};

// The verdict of piece p[0..n) (no '\n' inside) whose first TAB is known
// (tab >= n: it has none); terminated: a '\n' of its own reply followed it.
template <class Src>
CB_LOG_HD inline ReplyLine reply_line_at(Src p, uint64_t n, bool terminated, uint64_t tab) {
  if (!utf8_valid(p, n)) return ReplyLine{kReplyBadUtf8, 0, 0, 0, 0};
  const uint64_t len = reply_strip(p, n, terminated);
  if (!len) return ReplyLine{kReplyIgnored, 0, 0, 0, 0};
  if (tab >= len) return ReplyLine{kReplyOther, len, 0, 0, 0};
  uint64_t tab2 = tab + 1;
  while (tab2 < len && p[tab2] != '\t') ++tab2;
  if (tab2 >= len) return ReplyLine{kReplyOther, len, 0, 0, 0};
  return ReplyLine{kReplyEntry, len, tab, tab2, reply_ts(p + (tab + 1), tab2 - tab - 1)};
}

template <class Src>
CB_LOG_HD inline ReplyLine reply_line(Src p, uint64_t n, bool terminated) {
  uint64_t tab = 0;
  while (tab < n && p[tab] != '\t') ++tab;
  return reply_line_at(p, n, terminated, tab);
}

// ---- the canonical form of a val ----

// The string whose opening quote is v[at - 1], as serde_json writes one: the
// place behind its closing quote, or 0 when it is not in that form.
template <class Src>
CB_LOG_HD inline uint64_t canon_string_end(Src v, uint64_t n, uint64_t at) {
  while (at < n) {
    const uint32_t c = v[at++];
    if (c == '"') return at;
    if (c < 0x20) return 0;
    if (c != '\\') continue;  // (0x7F, '/' and non-ASCII bytes stand as they are)
    if (at >= n) return 0;
    const uint32_t e = v[at++];
    if (e == '"' || e == '\\' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't') continue;
    if (e != 'u' || n - at < 4 || v[at] != '0' || v[at + 1] != '0') return 0;
    const uint32_t h = v[at + 2], l = v[at + 3];
    if (h != '0' && h != '1') return 0;
    if (!((l >= '0' && l <= '9') || (l >= 'a' && l <= 'f'))) return 0;
    const uint32_t b = (h - '0') * 16 + (l <= '9' ? l - '0' : l - 'a' + 10);
    if (b == 8 || b == 9 || b == 10 || b == 12 || b == 13) return 0;  // (these have a short form)
    at += 4;
  }
  return 0;
}

// The next unescaped byte of a string in that form (*at inside it), or -1 at
// its closing quote.
template <class Src>
CB_LOG_HD inline int canon_next(Src v, uint64_t* at) {
  const uint32_t c = v[(*at)++];
  if (c == '"') return -1;
  if (c != '\\') return (int)c;
  const uint32_t e = v[(*at)++];
  if (e == 'u') {
    const uint32_t h = v[*at + 2], l = v[*at + 3];
    *at += 4;
    return (int)((h - '0') * 16 + (l <= '9' ? l - '0' : l - 'a' + 10));
  }
  return e == 'b' ? 8 : e == 'f' ? 12 : e == 'n' ? 10 : e == 'r' ? 13 : e == 't' ? 9 : (int)e;
}

// Whether the name at a is bytewise below the name at b, both in that form.
template <class Src>
CB_LOG_HD inline bool canon_name_less(Src v, uint64_t a, uint64_t b) {
  for (;;) {
    const int x = canon_next(v, &a), y = canon_next(v, &b);
    if (x != y) return x < y;  // (-1, the shorter name's end, is below every byte)
    if (x < 0) return false;
  }
}

// A winner's verdict: kFoldDead, kFoldText or kFoldHost.
template <class Src>
CB_LOG_HD inline uint8_t reply_val_flags(Src v, uint64_t n) {
  if (!n) return kFoldDead;
  if (n < 2 || v[0] != '{' || v[n - 1] != '}') return kFoldHost;
  if (n == 2) return kFoldText;
  uint64_t at = 1, prev = 0;
  for (;;) {
    if (at >= n || v[at] != '"') return kFoldHost;
    const uint64_t name = at + 1;
    at = canon_string_end(v, n, name);
    if (!at) return kFoldHost;
    if (prev && !canon_name_less(v, prev, name)) return kFoldHost;
    prev = name;
    if (n - at < 2 || v[at] != ':' || v[at + 1] != '"') return kFoldHost;
    at = canon_string_end(v, n, at + 2);
    if (!at || at >= n) return kFoldHost;
    if (v[at] == '}') return at + 1 == n ? kFoldText : kFoldHost;
    if (v[at] != ',') return kFoldHost;
    ++at;
  }
}

}  // namespace cb
