// rowjson.hpp — which rows a `WHERE col = value AND ...` keeps (host and
// device): the row's JSON payload, its key's parts and the equality
// conditions over both.
//
// The reference answers SELECT COUNT(*) ... WHERE by scanning the namespace
// (src/query.rs:309-362): per row it takes the timestamp off the value
// (split_ts, src/query.rs:21-27), skips a row without payload
// (src/query.rs:344-346), parses the payload with
//   serde_json::from_slice::<BTreeMap<String, String>>(payload).unwrap_or_default()
// (decode_row, src/schema.rs:42-44), inserts the key's `|`-separated parts as
// the key columns (key_columns(), src/schema.rs:27-33, zipped with the parts)
// and compares every condition (src/query.rs:341-357).
//
// This is the rule's one home in the library: cb_tables_count_where,
// cb_scan_match and cb_row_matches ask here and nothing restates it. No Rust
// toolchain and no serde_json were available when this was written, so the
// rules below are a restatement of serde_json's documented behaviour, checked
// against an independent Python restatement (tests/rowjson_ref.py) and
// Python's json module, and NOT run against the reference itself.
//
// Payload: the value itself below 8 decoded bytes, else the value from byte 8
// on. An empty payload is a deleted row (liverow.hpp says the same of the
// length alone): it never matches and nothing else is looked at.
//
// Map: the document is  ws { ws }  or  ws { ws string ws : ws string ws
// (, ws string ws : ws string ws)* } ws  and then the end of the input; ws is
// any run of space, \t, \n, \r. No trailing comma, no BOM. A key or value
// that is no string, a top level that is no object and any byte after the
// closing ws fail the document. Inside a string a raw byte below 0x20 is an
// error; the escapes are \" \\ \/ \b \f \n \r \t \uXXXX (hex digits of either
// case); a \u high surrogate must be followed at once by a \u low surrogate
// and the two form one code point; a lone surrogate of either kind is an
// error; \u0000 is legal; the unescaped bytes must be UTF-8 by Rust's rules
// (no overlong forms, no encoded surrogates, nothing above U+10FFFF). Of
// duplicate keys the last pair wins. ANY error ANYWHERE gives the empty map,
// not the pairs read so far: a match is decided only at the document's end,
// so a scanner must not stop at the first matching pair.
//
// Conditions: nc triples (col_i, val_i, part_i), ANDed; col and val are
// bytes, part_i the index of the key column col_i names, or -1.
// Key parts: the key without its first min(skip, len) bytes, split at every
// '|' (an empty rest is one empty part, as Rust's split gives).
// Match, per condition i of a row that is not deleted:
//   0 <= part_i < nparts: parts[part_i] == val_i bytewise; the JSON is not
//       consulted (the reference's insert of the key part overrides the map);
//   else (part_i >= nparts included: the reference's zip stops, and the key
//       column falls back to the JSON): the map has col_i and its last value
//       equals val_i bytewise, after unescaping.
// Two consequences: with nc == 0 every row that is not deleted matches; and a
// row whose conditions are all answered by its key matches even when its
// payload is not JSON at all.
//
// The rule reads a value through a byte source, so the same code runs over
// decoded bytes (DecodedBytes) and over base64 text decoded on the fly
// (B64Bytes, whose Text policy says how four characters are fetched).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rowts.hpp"

#if defined(__HIPCC__)
#define CB_ROW_HD __host__ __device__
#else
#define CB_ROW_HD
#endif

namespace cb {

constexpr uint32_t kWhereMaxConds = 16;    // conditions of one predicate
constexpr uint32_t kWhereMaxBytes = 4096;  // names and values together
constexpr int32_t kWhereMaxPart = 255;     // the largest key part index

// A checked predicate in one block (what travels to the device): condition
// i's name is bytes[col_at[i] .. col_at[i + 1]), its value bytes[val_at[i] ..
// val_at[i + 1]).
struct WherePred {
  uint32_t nc;
  int32_t part[kWhereMaxConds];
  uint16_t col_at[kWhereMaxConds + 1], val_at[kWhereMaxConds + 1];
  uint8_t bytes[kWhereMaxBytes];
};

// Why a predicate is refused, or nullptr (host arithmetic; no byte is read).
inline const char* where_check(const uint8_t* cols, const uint64_t* col_off, const uint8_t* vals,
                               const uint64_t* val_off, const int32_t* part, uint32_t nc) {
  if (nc > kWhereMaxConds) return "too many conditions (at most 16)";
  if (!nc) return nullptr;
  if (!col_off || !val_off || !part) return "null condition offsets or parts with a non-zero count";
  for (uint32_t i = 0; i < nc; ++i)
    if (col_off[i + 1] < col_off[i] || val_off[i + 1] < val_off[i]) return "condition offsets decrease";
  const uint64_t cb = col_off[nc] - col_off[0], vb = val_off[nc] - val_off[0];
  if (cb > kWhereMaxBytes || vb > kWhereMaxBytes || cb + vb > kWhereMaxBytes)
    return "too many bytes of names and values (at most 4096)";
  if ((cb && !cols) || (vb && !vals)) return "null names or values with a non-zero total";
  for (uint32_t i = 0; i < nc; ++i)
    if (part[i] < -1 || part[i] > kWhereMaxPart) return "a key part index outside -1..255";
  return nullptr;
}

// The checked predicate packed into *w (every byte of *w is written).
inline void where_pack(const uint8_t* cols, const uint64_t* col_off, const uint8_t* vals, const uint64_t* val_off,
                       const int32_t* part, uint32_t nc, WherePred* w) {
  *w = WherePred{};
  w->nc = nc;
  uint32_t at = 0;
  for (uint32_t i = 0; i < nc; ++i) {
    w->part[i] = part[i];
    w->col_at[i] = (uint16_t)at;
    for (uint64_t j = col_off[i]; j < col_off[i + 1]; ++j) w->bytes[at++] = cols[j];
  }
  for (uint32_t i = nc; i <= kWhereMaxConds; ++i) w->col_at[i] = (uint16_t)at;
  for (uint32_t i = 0; i < nc; ++i) {
    w->val_at[i] = (uint16_t)at;
    for (uint64_t j = val_off[i]; j < val_off[i + 1]; ++j) w->bytes[at++] = vals[j];
  }
  for (uint32_t i = nc; i <= kWhereMaxConds; ++i) w->val_at[i] = (uint16_t)at;
}

// ---- byte sources: size(), seek(i <= size()), tell(), more(), next() ----

// Decoded bytes p[0..n).
struct DecodedBytes {
  const uint8_t* p;
  uint64_t n, i;
  CB_ROW_HD DecodedBytes(const uint8_t* p_, uint64_t n_) : p(p_), n(n_), i(0) {}
  CB_ROW_HD uint64_t size() const { return n; }
  CB_ROW_HD void seek(uint64_t at) { i = at; }
  CB_ROW_HD uint64_t tell() const { return i; }
  CB_ROW_HD bool more() const { return i < n; }
  CB_ROW_HD uint8_t next() { return p[i++]; }
};

// Four characters of a text by byte loads: quad(q) = characters 4q .. 4q + 3,
// the first in the low byte. Reads nothing outside the text.
struct TextByBytes {
  const uint8_t* t;
  CB_ROW_HD uint32_t quad(uint64_t q) {
    const uint8_t* c = t + 4 * q;
    return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
  }
};

// The n bytes a valid STANDARD base64 text decodes to (4 ceil(n / 3)
// characters, '=' padding in the last quantum when n is no multiple of 3),
// one quantum of four characters at a time; seek() may land inside a quantum
// (byte 8 is the third byte of quantum 2). A padding character's bits are
// never handed out: next() is called for bytes below n only.
template <class Text>
struct B64Bytes {
  Text text;
  uint64_t n, i, q;
  uint32_t r, buf;  // the next byte is byte r of quantum q, whose 24 bits are buf (r == 3: not loaded yet)
  CB_ROW_HD B64Bytes(Text t, uint64_t n_) : text(t), n(n_), i(0), q(0), r(3), buf(0) {}
  CB_ROW_HD uint64_t size() const { return n; }
  CB_ROW_HD void load() {
    const uint32_t x = text.quad(q);
    buf = (uint32_t)(b64_sextet((uint8_t)x) & 63) << 18 | (uint32_t)(b64_sextet((uint8_t)(x >> 8)) & 63) << 12 |
          (uint32_t)(b64_sextet((uint8_t)(x >> 16)) & 63) << 6 | (uint32_t)(b64_sextet((uint8_t)(x >> 24)) & 63);
  }
  CB_ROW_HD void seek(uint64_t at) {
    i = at;
    q = at / 3;
    r = (uint32_t)(at % 3);
    if (at < n) load();
    else r = 3;
  }
  CB_ROW_HD uint64_t tell() const { return i; }
  CB_ROW_HD bool more() const { return i < n; }
  CB_ROW_HD uint8_t next() {
    if (r == 3) {
      q = i / 3;  // (i is a multiple of 3 here)
      r = 0;
      load();
    }
    const uint8_t b = (uint8_t)(buf >> (16 - 8 * r));
    ++r;
    ++i;
    return b;
  }
};

// ---- the key's parts ----

// What stands between two parts: build_row's and build_single_key's join
// (src/query.rs:730) writes it (rowwrite.hpp), the functions below split at it.
constexpr uint8_t kKeyPartSep = '|';

// How many parts the key's rest[0..n) has: one more than its separators (an
// empty rest is one empty part).
CB_ROW_HD inline uint64_t key_part_count(const uint8_t* rest, uint64_t n) {
  uint64_t nparts = 1;
  for (uint64_t j = 0; j < n; ++j) nparts += rest[j] == '|';
  return nparts;
}

// Where part p < key_part_count(rest, n) begins in rest, and *len its length.
CB_ROW_HD inline uint64_t key_part_at(const uint8_t* rest, uint64_t n, uint32_t p, uint64_t* len) {
  uint64_t a = 0;  // part p begins after its p-th separator (there are at least p)
  for (uint32_t k = 0; k < p; ++k) {
    while (rest[a] != '|') ++a;
    ++a;
  }
  uint64_t e = a;
  while (e < n && rest[e] != '|') ++e;
  *len = e - a;
  return a;
}

// ---- the grammar ----

// The one reader of the map's grammar (the header's "Map" paragraph): the
// document src.next()... is walked once, and what it holds goes to a sink:
//   sink.begin(value, at)  a string begins: a name, or (value) a name's value;
//                          `at` is the source's place after the opening quote
//   sink.byte(b)           one byte of the string, unescaped
//   sink.end(value)        the string is complete (it is valid so far)
//   sink.done(valid)       the input is at its end, or failed: whether the
//                          document is a valid map. An error ANYWHERE makes
//                          everything handed out before void.
// Returns `valid`. With one_string the source stands after an opening quote
// (an `at` of an earlier walk of a valid document): that string alone is read,
// sink.byte() for its bytes, and nothing else is called.
template <class Src, class Sink>
CB_ROW_HD inline bool json_walk(Src& src, Sink& sink, bool one_string = false) {
  enum : uint32_t {
    kOpen,       // ws, then {
    kFirstKey,   // ws, then " or }
    kKey,        // (after a comma) ws, then "
    kColon,      // ws, then :
    kValue,      // ws, then "
    kNext,       // ws, then , or }
    kEnd,        // ws to the end of the input
    kStr,        // inside a string
    kEsc,        // after a backslash
    kHex,        // the four digits of \u
    kLowSlash,   // after a high surrogate: a backslash
    kLowU,       // ... and its u
    kFail
  };
  uint32_t st = one_string ? kStr : kOpen;
  uint32_t need = 0, lo = 0x80, hi = 0xBF;  // continuation bytes still due, and the next one's bounds
  uint32_t cp = 0, hexn = 0, high = 0;
  bool val = false;
  uint32_t out = 0, nout = 0;  // the string's bytes that an input byte completes: nout of them, the first in out's low byte
  auto emit_cp = [&](uint32_t c) {  // a code point from an escape, as UTF-8
    if (c < 0x80) {
      out = c;
      nout = 1;
    } else if (c < 0x800) {
      out = (0xC0 | c >> 6) | (0x80 | (c & 63)) << 8;
      nout = 2;
    } else if (c < 0x10000) {
      out = (0xE0 | c >> 12) | (0x80 | (c >> 6 & 63)) << 8 | (0x80 | (c & 63)) << 16;
      nout = 3;
    } else {
      out = (0xF0 | c >> 18) | (0x80 | (c >> 12 & 63)) << 8 | (0x80 | (c >> 6 & 63)) << 16 | (0x80 | (c & 63)) << 24;
      nout = 4;
    }
  };
  auto emit = [&](uint32_t b) {
    out = b;
    nout = 1;
  };
  auto begin = [&](bool value) {
    val = value;
    sink.begin(value, src.tell());
    st = kStr;
  };
  auto is_ws = [](uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; };
  while (st != kFail && src.more()) {
    const uint32_t c = src.next();
    switch (st) {
      case kOpen:
        if (!is_ws(c)) st = c == '{' ? kFirstKey : kFail;
        break;
      case kFirstKey:
      case kKey:
        if (is_ws(c)) break;
        if (c == '"') begin(false);
        else st = c == '}' && st == kFirstKey ? kEnd : kFail;
        break;
      case kColon:
        if (!is_ws(c)) st = c == ':' ? kValue : kFail;
        break;
      case kValue:
        if (is_ws(c)) break;
        if (c == '"') begin(true);
        else st = kFail;
        break;
      case kNext:
        if (!is_ws(c)) st = c == ',' ? kKey : c == '}' ? kEnd : kFail;
        break;
      case kEnd:
        if (!is_ws(c)) st = kFail;
        break;
      case kStr:
        if (need) {  // inside a multi-byte sequence: nothing but its next byte is legal
          if (c < lo || c > hi) {
            st = kFail;
            break;
          }
          --need;
          lo = 0x80;
          hi = 0xBF;
          emit(c);
        } else if (c == '"') {
          if (one_string) return true;
          sink.end(val);
          st = val ? kNext : kColon;
        } else if (c == '\\') {
          st = kEsc;
        } else if (c < 0x20) {
          st = kFail;
        } else if (c < 0x80) {
          emit(c);
        } else {  // a lead byte, by Rust's str::from_utf8
          if (c >= 0xC2 && c <= 0xDF) {
            need = 1;
          } else if (c >= 0xE0 && c <= 0xEF) {
            need = 2;
            if (c == 0xE0) lo = 0xA0;  // no overlong form
            if (c == 0xED) hi = 0x9F;  // no encoded surrogate
          } else if (c >= 0xF0 && c <= 0xF4) {
            need = 3;
            if (c == 0xF0) lo = 0x90;  // no overlong form
            if (c == 0xF4) hi = 0x8F;  // nothing above U+10FFFF
          } else {
            st = kFail;
            break;
          }
          emit(c);
        }
        break;
      case kEsc: {
        const uint32_t e = c == '"' || c == '\\' || c == '/' ? c
                           : c == 'b'                        ? 8u
                           : c == 'f'                        ? 12u
                           : c == 'n'                        ? 10u
                           : c == 'r'                        ? 13u
                           : c == 't'                        ? 9u
                                                             : 0xFFFFu;
        if (e != 0xFFFFu) {
          emit(e);
          st = kStr;
        } else if (c == 'u') {
          cp = 0;
          hexn = 0;
          st = kHex;
        } else {
          st = kFail;
        }
        break;
      }
      case kHex: {
        const uint32_t d = c >= '0' && c <= '9'   ? c - '0'
                           : c >= 'a' && c <= 'f' ? c - 'a' + 10
                           : c >= 'A' && c <= 'F' ? c - 'A' + 10
                                                  : 0xFFu;
        if (d == 0xFFu) {
          st = kFail;
          break;
        }
        cp = cp << 4 | d;
        if (++hexn < 4) break;
        st = kStr;
        if (high) {  // the second half of a pair
          if (cp < 0xDC00 || cp > 0xDFFF) st = kFail;
          else emit_cp(0x10000 + ((high - 0xD800) << 10) + (cp - 0xDC00));
          high = 0;
        } else if (cp >= 0xD800 && cp <= 0xDBFF) {
          high = cp;
          st = kLowSlash;
        } else if (cp >= 0xDC00 && cp <= 0xDFFF) {
          st = kFail;  // a lone low surrogate
        } else {
          emit_cp(cp);
        }
        break;
      }
      case kLowSlash:
        st = c == '\\' ? kLowU : kFail;
        break;
      case kLowU:
        cp = 0;
        hexn = 0;
        st = c == 'u' ? kHex : kFail;
        break;
      default:
        st = kFail;
    }
    for (; nout; --nout, out >>= 8) sink.byte(out & 0xFF);  // (the one place a sink gets bytes)
  }
  if (one_string) return false;  // (an `at` that is none: the string never closed)
  sink.done(st == kEnd);
  return st == kEnd;
}

// ---- the rule ----

// The conditions the key answers (*answered) and, returned, those of them it
// satisfies, for the key's parts after `skip` bytes.
CB_ROW_HD inline uint32_t where_key_conditions(const WherePred& w, const uint8_t* key, uint64_t klen, uint32_t skip,
                                               uint32_t* answered) {
  const uint64_t s = skip < klen ? skip : klen;
  const uint8_t* rest = key + s;
  const uint64_t n = klen - s;
  uint32_t ans = 0, sat = 0;
  bool counted = false;
  uint64_t nparts = 1;
  for (uint32_t i = 0; i < w.nc; ++i) {
    const int32_t p = w.part[i];
    if (p < 0) continue;
    if (!counted) {
      nparts = key_part_count(rest, n);
      counted = true;
    }
    if ((uint64_t)p >= nparts) continue;
    ans |= 1u << i;
    uint64_t plen = 0;
    const uint64_t a = key_part_at(rest, n, (uint32_t)p, &plen);
    const uint32_t vat = w.val_at[i], vlen = w.val_at[i + 1] - vat;
    uint64_t j = 0;
    while (j < plen && j < vlen && rest[a + j] == w.bytes[vat + j]) ++j;
    if (j == vlen && j == plen) sat |= 1u << i;
  }
  *answered = ans;
  return sat;
}

// json_walk's sink for the conditions: the pairs are compared as they are
// read; per string, `alive` holds the conditions whose name (or value) equals
// the unescaped bytes so far.
struct WhereSink {
  const WherePred& w;
  uint32_t ask, alive, keyhit, ok, pos;
  bool val;
  CB_ROW_HD WhereSink(const WherePred& w_, uint32_t ask_) : w(w_), ask(ask_), alive(0), keyhit(0), ok(0), pos(0), val(false) {}
  CB_ROW_HD void begin(bool value, uint64_t) {
    val = value;
    alive = value ? keyhit : ask;
    pos = 0;
  }
  CB_ROW_HD void byte(uint32_t b) {
    for (uint32_t m = alive; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__builtin_ctz(m);
      const uint32_t at = val ? w.val_at[i] : w.col_at[i], len = (val ? w.val_at[i + 1] : w.col_at[i + 1]) - at;
      if (pos >= len || w.bytes[at + pos] != b) alive &= ~(1u << i);
    }
    ++pos;
  }
  CB_ROW_HD void end(bool) {  // the conditions of exactly this length stay
    for (uint32_t m = alive; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__builtin_ctz(m);
      const uint32_t len = val ? w.val_at[i + 1] - w.val_at[i] : w.col_at[i + 1] - w.col_at[i];
      if (len != pos) alive &= ~(1u << i);
    }
    if (val) ok = (ok & ~keyhit) | alive;  // the last pair of a name wins
    else keyhit = alive;
  }
  CB_ROW_HD void done(bool valid) {
    if (!valid) ok = 0;
  }
};

// The conditions of `ask` (a mask over w's conditions) that the map of the
// document src.next()... satisfies; 0 for a document with an error.
template <class Src>
CB_ROW_HD inline uint32_t where_json_conditions(const WherePred& w, uint32_t ask, Src& src) {
  WhereSink sink(w, ask);
  json_walk(src, sink);
  return sink.ok;
}

// Whether the row (key, value) matches w, the key's parts taken after `skip`
// bytes. value: a byte source over the whole decoded value.
template <class Src>
CB_ROW_HD inline bool row_matches(const WherePred& w, const uint8_t* key, uint64_t klen, uint32_t skip, Src& value) {
  const uint64_t n = value.size(), start = n < 8 ? 0 : 8;  // split_ts
  if (n == start) return false;                             // no payload: a deleted row
  const uint32_t all = (1u << w.nc) - 1;                    // (nc <= 16)
  uint32_t answered = 0;
  const uint32_t sat = where_key_conditions(w, key, klen, skip, &answered);
  if (sat != answered) return false;
  const uint32_t ask = all & ~answered;
  if (!ask) return true;  // the key answered everything: the payload is not parsed
  value.seek(start);
  return where_json_conditions(w, ask, value) == ask;
}

}  // namespace cb
