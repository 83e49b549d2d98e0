// rowselect.hpp — the bytes a `SELECT a, b FROM t WHERE pk IN (...)` returns
// for a row (host and device): the row's columns projected, cast and written
// out again as JSON.
//
// The reference's exec_select_schema (src/query.rs:365-432) does, per key it
// got a value for: split_ts (src/query.rs:21-27); a row without payload is a
// deleted row (src/query.rs:396-400); decode_row (src/schema.rs:42-44); the
// key's `|`-separated parts laid over the map as the key columns
// (src/query.rs:402-405); project_row with cast_simple (src/query.rs:641-662,
// 817-827); encode_row (src/schema.rs:37-39); and the rows joined into the
// response, a JSON array for a client (src/query.rs:411-431) or `key\tts\tval`
// lines for a coordinator, which folds them by timestamp
// (src/cluster.rs:404-421).
//
// This is the rule's one home in the library: cb_scan_select, cb_rows_select
// and cb_row_select ask here. What a payload's map is comes from rowjson.hpp
// (json_walk, the grammar's one reader, and the key-part locator), the
// timestamp from rowts.hpp. Like rowjson.hpp it is a restatement of
// serde_json's and Rust's documented behaviour, checked against an independent
// Python restatement (tests/rowselect_ref.py) and Python's json module, and
// NOT run against the reference itself.
//
// Selection: nc <= 16 columns, each a name (bytes; empty is legal), `part`
// (the index of the key column the name is, or -1) and `cast` (0 none, 1
// integer). The names ascend strictly bytewise, which is a BTreeMap's order:
// the object's pairs are written in selection order and nothing is sorted per
// row. kWhereMaxBytes bounds the names' bytes, kWhereMaxPart the parts.
//
// Per row (key, value), the key's parts taken after min(skip, len) bytes:
//   1. ts, payload = split_ts(value). An empty payload is a deleted row.
//   2. Column c's value: if 0 <= part_c < nparts it is key part part_c and the
//      payload is not consulted for it; else (part_c >= nparts included) the
//      LAST pair of that name in the payload's map, unescaped. Without such a
//      pair, or with an error anywhere in the document (the empty map), the
//      column is left out.
//   3. cast 1: Rust's str::parse::<i64> takes an optional single + or -, then
//      one or more ASCII digits and nothing else, of a value that fits i64;
//      the value becomes i64::to_string of it (no +, no leading zeros, -0 is
//      0). Any failure leaves the value as it was. (Text, Varchar and Char
//      casts change nothing: cast 0.)
//   4. The row's object: {"name":"value",...} over the columns that have a
//      value, in selection order, no spaces; names and values escaped as
//      serde_json writes strings: " and \ behind a backslash, 0x08 0x0C 0x0A
//      0x0D 0x09 as \b \f \n \r \t, every other byte below 0x20 as \u00xx in
//      lower-case hex, every other byte (0x7F, non-ASCII and / included) as it
//      is. No column with a value: {}.
//   5. Flags: kRowText (the row has text), kRowDead, kRowAbsent (no row at
//      all: the caller's which < 0; nothing else is looked at), kRowBadJson
//      (the payload is no valid map), kRowExtra (a valid map holds a name
//      that is not in the selection). EVERY live row's payload is parsed,
//      whether a column needs it or not, so the last two are defined for every
//      live row. kRowExtra is what makes SELECT * exact without a sort on the
//      device: the caller passes all of the schema's columns, and a row
//      without kRowExtra is the reference's wildcard row; the rows with it are
//      done again from their values (cb_scan_values). A true wildcard is not
//      offered.
// Text, by mode:
//   kSelectJson: a live row's text is its object; dead and absent rows have
//      none. The response is [ + the texts joined by , + ] ([] without any).
//   kSelectMeta: a live row's text is the key after skip, \t, ts in decimal,
//      \t, the object; a dead row's is key \t ts \t and nothing else; absent
//      rows have none. The response is the texts joined by \n, no trailing
//      newline, and no byte at all without any (the reference's Ok(None)).
//
// Two passes, so that a row's text can be written where an exclusive scan of
// the lengths puts it: select_size walks the payload once and leaves, per
// column, where the winning value's string begins and how long it is once
// cast and escaped (Slots: the caller's storage, one place per column);
// select_write reads each winning string again from that place through
// json_walk's unescaper. No unescaped copy is kept.
#pragma once
#include "rowjson.hpp"

namespace cb {

constexpr uint32_t kSelectMaxCols = kWhereMaxConds;

constexpr uint8_t kRowText = 1, kRowDead = 2, kRowAbsent = 4, kRowBadJson = 8, kRowExtra = 16;
constexpr int kSelectJson = 0, kSelectMeta = 1;

// A checked selection in one block (what travels to the device): column c's
// name is bytes[col_at[c] .. col_at[c + 1]), name_esc[c] its length escaped.
struct SelectCols {
  uint32_t nc;
  int32_t part[kSelectMaxCols];
  uint8_t cast[kSelectMaxCols];
  uint16_t name_esc[kSelectMaxCols];
  uint16_t col_at[kSelectMaxCols + 1];
  uint8_t bytes[kWhereMaxBytes];
};

// ---- the writer ----

struct CountOut {  // how many bytes a text takes
  uint64_t n = 0;
  CB_ROW_HD void put(uint32_t) { ++n; }
};
struct ByteOut {  // the text itself
  uint8_t* p;
  CB_ROW_HD void put(uint32_t b) { *p++ = (uint8_t)b; }
};

// One byte of a string as serde_json writes it.
template <class Out>
CB_ROW_HD inline void esc_put(Out& out, uint32_t b) {
  if (b == '"' || b == '\\') {
    out.put('\\');
    out.put(b);
  } else if (b >= 0x20) {
    out.put(b);
  } else {
    const uint32_t e = b == 8 ? 'b' : b == 12 ? 'f' : b == 10 ? 'n' : b == 13 ? 'r' : b == 9 ? 't' : 0u;
    out.put('\\');
    if (e) {
      out.put(e);
    } else {
      out.put('u');
      out.put('0');
      out.put('0');
      out.put('0' + (b >> 4));  // (below 0x20: 0 or 1)
      out.put((b & 15) < 10 ? '0' + (b & 15) : 'a' + (b & 15) - 10);
    }
  }
}

// v in decimal: `digits` = dec_digits(v) bytes.
CB_ROW_HD inline uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}
CB_ROW_HD inline void dec_put(ByteOut& out, uint64_t v, uint32_t digits) {
  for (uint32_t k = digits; k-- > 0; v /= 10) out.p[k] = (uint8_t)('0' + v % 10);
  out.p += digits;
}

// str::parse::<i64> over a value's bytes, one at a time.
struct CastScan {
  uint32_t st = 0;   // 0 nothing yet, 1 a sign, 2 digits, 3 no integer
  uint32_t sig = 0;  // digits from the first that is not 0
  bool neg = false;
  uint64_t mag = 0;
  CB_ROW_HD void byte(uint32_t b) {
    if (st == 3) return;
    if (st == 0 && (b == '+' || b == '-')) {
      neg = b == '-';
      st = 1;
      return;
    }
    const uint64_t d = (uint64_t)b - '0', lim = 0x7FFFFFFFFFFFFFFFull + (neg ? 1 : 0);
    if (b < '0' || b > '9' || mag > (lim - d) / 10) {  // (mag * 10 + d > lim)
      st = 3;
      return;
    }
    mag = mag * 10 + d;
    if (mag) ++sig;
    st = 2;
  }
  CB_ROW_HD bool ok() const { return st == 2; }
  CB_ROW_HD bool minus() const { return neg && mag; }
  CB_ROW_HD uint32_t digits() const { return sig ? sig : 1; }
  CB_ROW_HD uint64_t len() const { return digits() + (minus() ? 1 : 0); }  // of i64::to_string
  CB_ROW_HD void put(ByteOut& out) const {
    if (minus()) out.put('-');
    dec_put(out, mag, digits());
  }
};

// ---- the selection ----

// Why a selection is refused, or nullptr (host arithmetic and the names' bytes).
inline const char* select_check(const uint8_t* cols, const uint64_t* col_off, const int32_t* part, const uint8_t* cast,
                                uint32_t nc) {
  if (nc > kSelectMaxCols) return "too many columns (at most 16)";
  if (!nc) return nullptr;
  if (!col_off || !part) return "null column offsets or parts with a non-zero count";
  for (uint32_t i = 0; i < nc; ++i)
    if (col_off[i + 1] < col_off[i]) return "column offsets decrease";
  const uint64_t nb = col_off[nc] - col_off[0];
  if (nb > kWhereMaxBytes) return "too many bytes of names (at most 4096)";
  if (nb && !cols) return "null names with a non-zero total";
  for (uint32_t i = 0; i < nc; ++i) {
    if (part[i] < -1 || part[i] > kWhereMaxPart) return "a key part index outside -1..255";
    if (cast && cast[i] > 1) return "a cast that is neither 0 nor 1";
  }
  for (uint32_t i = 0; i + 1 < nc; ++i) {  // name i < name i + 1, bytewise
    const uint8_t *a = cols + col_off[i], *b = cols + col_off[i + 1];
    const uint64_t la = col_off[i + 1] - col_off[i], lb = col_off[i + 2] - col_off[i + 1];
    uint64_t j = 0;
    while (j < la && j < lb && a[j] == b[j]) ++j;
    if (j == lb || (j < la && a[j] > b[j])) return "the names are not strictly ascending";
  }
  return nullptr;
}

// The checked selection packed into *sel (every byte of *sel is written).
inline void select_pack(const uint8_t* cols, const uint64_t* col_off, const int32_t* part, const uint8_t* cast,
                        uint32_t nc, SelectCols* sel) {
  *sel = SelectCols{};
  sel->nc = nc;
  uint32_t at = 0;
  for (uint32_t i = 0; i < nc; ++i) {
    sel->part[i] = part[i];
    sel->cast[i] = cast ? cast[i] : 0;
    sel->col_at[i] = (uint16_t)at;
    CountOut esc;
    for (uint64_t j = col_off[i]; j < col_off[i + 1]; ++j) {
      sel->bytes[at++] = cols[j];
      esc_put(esc, cols[j]);
    }
    sel->name_esc[i] = (uint16_t)esc.n;  // (at most 6 x 4096)
  }
  for (uint32_t i = nc; i <= kSelectMaxCols; ++i) sel->col_at[i] = (uint16_t)at;
}

// What select_size leaves per column for select_write, in the caller's Slots
// (set(c, at, len), get(c, &at, &len)): where the value begins (in the value
// for a payload's string, in the key's rest for a key part) and its length
// as written, with two marks.
constexpr uint64_t kSlotNone = ~0ull;       // the column is left out
constexpr uint64_t kSlotCast = 1ull << 63;  // the length is i64::to_string's: the cast took
constexpr uint64_t kSlotKey = 1ull << 62;   // a key part
constexpr uint64_t kSlotLen = kSlotKey - 1;

// Slots in plain arrays: the host's form.
struct ArraySlots {
  uint64_t at[kSelectMaxCols], len[kSelectMaxCols];
  CB_ROW_HD void set(uint32_t c, uint64_t a, uint64_t l) {
    at[c] = a;
    len[c] = l;
  }
  CB_ROW_HD void get(uint32_t c, uint64_t* a, uint64_t* l) const {
    *a = at[c];
    *l = len[c];
  }
};

// A value's length as written, from its unescaped bytes one at a time.
struct ValueMeasure {
  CountOut esc;
  CastScan num;
  CB_ROW_HD void byte(uint32_t b) {
    esc_put(esc, b);
    num.byte(b);
  }
  CB_ROW_HD uint64_t len(bool cast) const { return cast && num.ok() ? num.len() | kSlotCast : esc.n; }
};

// json_walk's sink of the first pass: a name is compared with the selection's
// as it is read (the names differ, so at most one stays), a value of a
// selected column that the key does not answer is measured and put in its
// slot; a later pair of the same name overwrites it.
template <class Slots>
struct SelectSizeSink {
  const SelectCols& sel;
  Slots& slots;
  uint32_t from_key;  // the columns the key answers
  uint32_t alive = 0, hit = 0, pos = 0;
  bool val = false, extra = false;
  uint64_t at = 0;
  ValueMeasure m;
  CB_ROW_HD SelectSizeSink(const SelectCols& sel_, Slots& slots_, uint32_t from_key_)
      : sel(sel_), slots(slots_), from_key(from_key_) {}
  CB_ROW_HD void begin(bool value, uint64_t at_) {
    val = value;
    if (value) {
      at = at_;
      m = ValueMeasure{};
    } else {
      alive = (1u << sel.nc) - 1;  // (nc <= 16)
      pos = 0;
    }
  }
  CB_ROW_HD void byte(uint32_t b) {
    if (val) {
      if (hit) m.byte(b);
      return;
    }
    for (uint32_t k = alive; k; k &= k - 1) {
      const uint32_t c = (uint32_t)__builtin_ctz(k);
      const uint32_t a = sel.col_at[c], len = sel.col_at[c + 1] - a;
      if (pos >= len || sel.bytes[a + pos] != b) alive &= ~(1u << c);
    }
    ++pos;
  }
  CB_ROW_HD void end(bool) {
    if (val) {
      if (hit) {
        const uint32_t c = (uint32_t)__builtin_ctz(hit);
        slots.set(c, at, m.len(sel.cast[c] != 0));
      }
      return;
    }
    for (uint32_t k = alive; k; k &= k - 1) {
      const uint32_t c = (uint32_t)__builtin_ctz(k);
      if ((uint32_t)(sel.col_at[c + 1] - sel.col_at[c]) != pos) alive &= ~(1u << c);
    }
    if (!alive) extra = true;
    hit = alive & ~from_key;
  }
  CB_ROW_HD void done(bool) {}
};

// The first pass: *flags, the slots of a live row, and, returned, the length
// of the row's text (0 without kRowText). value: a byte source over the whole
// decoded value; absent: the caller has no row here.
template <class Src, class Slots>
CB_ROW_HD inline uint64_t select_size(const SelectCols& sel, const uint8_t* key, uint64_t klen, uint32_t skip,
                                      bool absent, Src& value, int mode, Slots& slots, uint8_t* flags) {
  if (absent) {
    *flags = kRowAbsent;
    return 0;
  }
  const uint64_t n = value.size(), start = n < 8 ? 0 : 8;  // split_ts
  const uint64_t s = skip < klen ? skip : klen, rn = klen - s;
  const uint8_t* rest = key + s;
  const uint64_t ts = source_ts(value);
  const uint64_t head = mode == kSelectMeta ? rn + 1 + dec_digits(ts) + 1 : 0;
  if (n == start) {  // no payload: a deleted row
    *flags = mode == kSelectMeta ? kRowDead | kRowText : kRowDead;
    return head;
  }
  uint32_t from_key = 0;
  uint64_t nparts = 0;
  for (uint32_t c = 0; c < sel.nc; ++c) {
    slots.set(c, 0, kSlotNone);
    if (sel.part[c] < 0) continue;
    if (!nparts) nparts = key_part_count(rest, rn);
    if ((uint64_t)sel.part[c] < nparts) from_key |= 1u << c;
  }
  value.seek(start);
  SelectSizeSink<Slots> sink(sel, slots, from_key);
  const bool valid = json_walk(value, sink);
  *flags = kRowText | (!valid ? kRowBadJson : sink.extra ? kRowExtra : 0);
  uint64_t obj = 2, pairs = 0;
  for (uint32_t c = 0; c < sel.nc; ++c) {
    uint64_t at = 0, len = kSlotNone;
    if (from_key >> c & 1) {
      uint64_t plen = 0;
      at = key_part_at(rest, rn, (uint32_t)sel.part[c], &plen);
      ValueMeasure m;
      for (uint64_t j = 0; j < plen; ++j) m.byte(rest[at + j]);
      len = m.len(sel.cast[c] != 0) | kSlotKey;
      slots.set(c, at, len);
    } else if (valid) {
      slots.get(c, &at, &len);
    } else {
      slots.set(c, 0, kSlotNone);  // (an error anywhere: what the walk put here is void)
    }
    if (len == kSlotNone) continue;
    obj += (pairs ? 1 : 0) + 1 + sel.name_esc[c] + 3 + (len & kSlotLen) + 1;  // , "name":"value"
    ++pairs;
  }
  return head + obj;
}

// json_walk's sinks of the second pass, over one string: its bytes escaped
// into the text, or taken as an integer.
struct EscSink {
  ByteOut& out;
  CB_ROW_HD void begin(bool, uint64_t) {}
  CB_ROW_HD void byte(uint32_t b) { esc_put(out, b); }
  CB_ROW_HD void end(bool) {}
  CB_ROW_HD void done(bool) {}
};
struct CastSink {
  CastScan num;
  CB_ROW_HD void begin(bool, uint64_t) {}
  CB_ROW_HD void byte(uint32_t b) { num.byte(b); }
  CB_ROW_HD void end(bool) {}
  CB_ROW_HD void done(bool) {}
};

// The second pass: the text of a row whose flags hold kRowText, select_size's
// return value bytes long, at out; flags and slots as select_size left them.
template <class Src, class Slots>
CB_ROW_HD inline void select_write(const SelectCols& sel, const uint8_t* key, uint64_t klen, uint32_t skip, Src& value,
                                   int mode, uint8_t flags, const Slots& slots, uint8_t* out_at) {
  ByteOut out{out_at};
  const uint64_t s = skip < klen ? skip : klen, rn = klen - s;
  const uint8_t* rest = key + s;
  if (mode == kSelectMeta) {
    for (uint64_t j = 0; j < rn; ++j) out.put(rest[j]);
    out.put('\t');
    const uint64_t ts = source_ts(value);
    dec_put(out, ts, dec_digits(ts));
    out.put('\t');
    if (flags & kRowDead) return;
  }
  out.put('{');
  bool first = true;
  for (uint32_t c = 0; c < sel.nc; ++c) {
    uint64_t at = 0, len = kSlotNone;
    slots.get(c, &at, &len);
    if (len == kSlotNone) continue;
    if (!first) out.put(',');
    first = false;
    out.put('"');
    for (uint32_t j = sel.col_at[c]; j < sel.col_at[c + 1]; ++j) esc_put(out, sel.bytes[j]);
    out.put('"');
    out.put(':');
    out.put('"');
    if (len & kSlotKey) {
      uint64_t plen = 0;
      (void)key_part_at(rest + at, rn - at, 0, &plen);  // (the part that begins at `at`: to its end)
      if (len & kSlotCast) {
        CastScan num;
        for (uint64_t j = 0; j < plen; ++j) num.byte(rest[at + j]);
        num.put(out);
      } else {
        for (uint64_t j = 0; j < plen; ++j) esc_put(out, rest[at + j]);
      }
    } else {
      value.seek(at);
      if (len & kSlotCast) {
        CastSink sink;
        json_walk(value, sink, true);
        sink.num.put(out);
      } else {
        EscSink sink{out};
        json_walk(value, sink, true);
      }
    }
    out.put('"');
  }
  out.put('}');
}

}  // namespace cb
