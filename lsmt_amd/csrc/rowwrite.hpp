// rowwrite.hpp — the bytes an INSERT, UPDATE or DELETE stores for a row (host
// and device): the row's key, its value (timestamp + JSON payload) and its
// record in the write-ahead log.
//
// The reference's write statements end in one call each:
//   exec_insert + build_row (src/query.rs:162-198, 716-731): the key columns'
//       values joined by `|` in the statement's column order, every other
//       column into a BTreeMap, encode_row (src/schema.rs:37-39) of the map;
//   exec_update (src/query.rs:201-237): the key from the WHERE clause in the
//       schema's key_columns() order, the old row's map (split_ts, decode_row
//       with unwrap_or_default; no old row: the empty map), the assignments
//       laid over it, encode_row;
//   exec_delete (src/query.rs:240-261): the key, and an empty payload;
// then insert_ns_ts / insert_ts (src/lib.rs:154-157): the key prefixed with
// `ns:`, the value prefixed with the 8 big-endian bytes of the timestamp, and
// insert_internal (src/lib.rs:96-116), which appends `key \t
// STANDARD.encode(value) \n` to the log before the memtable takes the pair.
//
// This is the rule's one home in the library: cb_rows_write (write.hip) and
// cb_row_write ask here. What a payload's map is comes from rowjson.hpp
// (json_walk), how a string is written from rowselect.hpp (esc_put), whose
// first-pass sink also finds the old row's values. Like them it is a
// restatement of serde_json's and Rust's documented behaviour, checked against
// an independent Python restatement (tests/rowwrite_ref.py) and Python's json
// and base64 modules, and NOT run against the reference itself. The SQL
// parser stays outside: a batch is the cells of one prepared statement.
//
// Batch: a namespace ns (bytes, may be empty); nk <= 16 key columns in the
// caller's order; nc <= 16 payload column names, strictly ascending bytewise
// (a BTreeMap's order; select_check's rules and its 4096-byte bound); per
// payload column set[c], 1 the statement gives the value, 0 keep the old
// row's; an op. kWriteInsert: every set[c] is 1 and there are no old rows.
// kWriteDelete: nc is 0 and there are no old rows. With w = nk + the number
// of set columns, row i's cells are w byte strings: the key cells, then the
// set columns' in name order.
//
// Per row:
//   1. Key: ns ':' then the key cells joined by '|'; `ns:` with nk == 0.
//   2. Old map (kWriteUpdate with an old value only): split_ts of the old
//      value, its payload walked by json_walk. An error anywhere gives the
//      empty map (kWrittenBadOld); so does an empty payload, a tombstone,
//      which is no error of the store's and is not flagged. Of a duplicated
//      name the last pair wins.
//   3. Payload: none for kWriteDelete. Else {"name":"value",...} over the
//      columns that have a value, in name order, no spaces: a set column has
//      its cell (which may be empty: ""), a kept column the old map's value,
//      unescaped and escaped again, a kept column without one is left out.
//      Names and values go through esc_put. No column with a value: {}, a
//      live row.
//   4. Value: the timestamp as 8 big-endian bytes, then the payload.
//   5. Log record: key \t STANDARD.encode(value) \n.
//   6. Flags: kWrittenHost, the old payload is a valid map that holds a name
//      outside the nc columns: nothing is sorted per row, so the row is the
//      caller's to do (as kRowExtra's rows are); its key is written, its value
//      and its record have length 0. kWrittenBadOld, see 2. kWrittenKeyCtl, the
//      key holds \t or \n: its record will not replay to the same key
//      (cb_log_replay cuts at both); the row is written all the same.
// Cell bytes are the caller's Rust Strings: UTF-8 is NOT checked here, and a
// cell that is not UTF-8 gives a payload no reader accepts.
//
// Two passes, as in rowselect.hpp: write_size leaves the three lengths and,
// per kept column, where the old value's string begins and its escaped length
// (the caller's Slots); write_emit writes the three byte strings, each kept
// string read again from its place.
#pragma once
#include "rowselect.hpp"

namespace cb {

constexpr int kWriteInsert = 0, kWriteUpdate = 1, kWriteDelete = 2;
constexpr uint8_t kWrittenHost = 1, kWrittenBadOld = 2, kWrittenKeyCtl = 4;
constexpr uint32_t kWriteMaxKeyCols = 16;
constexpr uint64_t kWriteMaxRecord = 1ull << 32;  // a record this long or longer is refused: cb_log_replay's limit

// A checked statement in one block (what travels to the device): the payload
// columns as a selection without key parts or casts, which of them are set
// (setmask) and, for those, which cell of the row holds the value.
struct WriteCols {
  SelectCols sel;
  uint32_t nk, op, width, setmask;  // width: cells per row
  uint8_t cell_of[kSelectMaxCols];
};

// Why a statement is refused, or nullptr (host arithmetic and the names' bytes).
inline const char* write_check(const uint8_t* ns, uint64_t ns_len, uint32_t nk, const uint8_t* cols,
                               const uint64_t* col_off, const uint8_t* set, uint32_t nc, int op) {
  static const int32_t no_part[kSelectMaxCols] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
  if (op != kWriteInsert && op != kWriteUpdate && op != kWriteDelete) return "an op that is none of insert, update and delete";
  if (nk > kWriteMaxKeyCols) return "too many key columns (at most 16)";
  if (ns_len && !ns) return "null namespace with a length";
  if (const char* why = select_check(cols, col_off, no_part, nullptr, nc)) return why;
  if (op == kWriteDelete && nc) return "a delete with payload columns";
  if (nc && !set) return "null set flags with a non-zero count";
  for (uint32_t c = 0; c < nc; ++c) {
    if (set[c] > 1) return "a set flag that is neither 0 nor 1";
    if (op == kWriteInsert && !set[c]) return "an insert that keeps a column";
  }
  return nullptr;
}

// The checked statement packed into *w (every byte of *w is written).
inline void write_pack(uint32_t nk, const uint8_t* cols, const uint64_t* col_off, const uint8_t* set, uint32_t nc,
                       int op, WriteCols* w) {
  int32_t no_part[kSelectMaxCols];
  for (uint32_t c = 0; c < kSelectMaxCols; ++c) no_part[c] = -1;
  select_pack(cols, col_off, no_part, nullptr, nc, &w->sel);
  w->nk = nk;
  w->op = (uint32_t)op;
  w->setmask = 0;
  uint32_t at = nk;
  for (uint32_t c = 0; c < kSelectMaxCols; ++c) {
    const bool s = c < nc && set[c];
    w->cell_of[c] = (uint8_t)(s ? at : 0);
    if (s) {
      w->setmask |= 1u << c;
      ++at;
    }
  }
  w->width = at;
}

// Whether a record cut at these bytes comes back as another key.
CB_ROW_HD inline bool key_ctl(const uint8_t* p, uint64_t n) {
  bool ctl = false;
  for (uint64_t j = 0; j < n; ++j) ctl |= p[j] == '\t' || p[j] == '\n';
  return ctl;
}

// 4 ceil(n / 3): STANDARD.encode's length.
CB_ROW_HD inline uint64_t b64_text_len(uint64_t n) { return (n + 2) / 3 * 4; }

// The first pass over row i: off = its width + 1 cell offsets into cells (not
// read with a width of 0); has_old: old is a byte source over the old value.
// *flags, the key's, the value's and the record's lengths, and the kept
// columns' slots.
template <class Src, class Slots>
CB_ROW_HD inline void write_size(const WriteCols& w, uint64_t ns_len, bool ns_ctl, const uint8_t* cells,
                                 const uint64_t* off, bool has_old, Src& old, Slots& slots, uint8_t* flags,
                                 uint64_t* klen, uint64_t* vlen, uint64_t* rlen) {
  const uint32_t nk = w.nk, nc = w.sel.nc;
  uint64_t kl = ns_len + 1;
  uint8_t f = 0;
  if (nk) {
    kl += off[nk] - off[0] + (nk - 1);
    if (key_ctl(cells + off[0], off[nk] - off[0])) f |= kWrittenKeyCtl;
  }
  if (ns_ctl) f |= kWrittenKeyCtl;
  uint64_t payload = 0;
  if (w.op != kWriteDelete) {
    for (uint32_t c = 0; c < nc; ++c) slots.set(c, 0, kSlotNone);
    if (has_old) {
      const uint64_t n = old.size(), start = n < 8 ? 0 : 8;  // split_ts
      if (n != start) {
        old.seek(start);
        SelectSizeSink<Slots> sink(w.sel, slots, w.setmask);  // (a set column's old value is not measured)
        if (!json_walk(old, sink)) {
          f |= kWrittenBadOld;
          for (uint32_t c = 0; c < nc; ++c) slots.set(c, 0, kSlotNone);  // (what the walk put here is void)
        } else if (sink.extra) {
          f |= kWrittenHost;
        }
      }
    }
    payload = 2;
    uint32_t pairs = 0;
    for (uint32_t c = 0; c < nc; ++c) {
      uint64_t len = 0;
      if (w.setmask >> c & 1) {
        const uint32_t j = w.cell_of[c];
        CountOut esc;
        for (uint64_t b = off[j]; b < off[j + 1]; ++b) esc_put(esc, cells[b]);
        len = esc.n;
      } else {
        uint64_t at = 0;
        slots.get(c, &at, &len);
        if (len == kSlotNone) continue;
      }
      payload += (pairs ? 1 : 0) + 1 + w.sel.name_esc[c] + 3 + len + 1;  // , "name":"value"
      ++pairs;
    }
  }
  *flags = f;
  *klen = kl;
  *vlen = f & kWrittenHost ? 0 : 8 + payload;
  *rlen = f & kWrittenHost ? 0 : kl + 1 + b64_text_len(8 + payload) + 1;
}

// The value's bytes on their way out: each goes to the value and, three at a
// time, as one quad of base64 into the record.
struct ValueOut {
  uint8_t *v, *r;
  uint32_t buf = 0, have = 0;
  CB_ROW_HD ValueOut(uint8_t* v_, uint8_t* r_) : v(v_), r(r_) {}
  CB_ROW_HD void quad(uint32_t x, uint32_t m) {  // m of x's three bytes are the value's
    r[0] = b64_char(x >> 18);
    r[1] = b64_char(x >> 12 & 63);
    r[2] = m > 1 ? b64_char(x >> 6 & 63) : (uint8_t)'=';
    r[3] = m > 2 ? b64_char(x & 63) : (uint8_t)'=';
    r += 4;
  }
  CB_ROW_HD void put(uint32_t b) {
    *v++ = (uint8_t)b;
    buf = buf << 8 | (b & 0xFF);
    if (++have == 3) {
      quad(buf, 3);
      buf = 0;
      have = 0;
    }
  }
  CB_ROW_HD void finish() {
    if (have) quad(buf << (8 * (3 - have)), have);
  }
};

// json_walk's sink of the second pass: one string's bytes escaped into Out.
template <class Out>
struct EscTo {
  Out& out;
  CB_ROW_HD void begin(bool, uint64_t) {}
  CB_ROW_HD void byte(uint32_t b) { esc_put(out, b); }
  CB_ROW_HD void end(bool) {}
  CB_ROW_HD void done(bool) {}
};

// The second pass: the key (klen bytes at key_out), and for a row without
// kWrittenHost the value (vlen bytes at val_out) and the record (rlen bytes at
// rec_out); flags and slots as write_size left them.
template <class Src, class Slots>
CB_ROW_HD inline void write_emit(const WriteCols& w, const uint8_t* ns, uint64_t ns_len, const uint8_t* cells,
                                 const uint64_t* off, uint64_t ts, Src& old, uint8_t flags, const Slots& slots,
                                 uint8_t* key_out, uint8_t* val_out, uint8_t* rec_out) {
  const bool whole = !(flags & kWrittenHost);
  uint64_t k = 0;
  auto key_put = [&](uint8_t b) {
    key_out[k] = b;
    if (whole) rec_out[k] = b;
    ++k;
  };
  for (uint64_t j = 0; j < ns_len; ++j) key_put(ns[j]);
  key_put(':');
  for (uint32_t p = 0; p < w.nk; ++p) {
    if (p) key_put(kKeyPartSep);
    for (uint64_t b = off[p]; b < off[p + 1]; ++b) key_put(cells[b]);
  }
  if (!whole) return;
  rec_out[k] = '\t';
  ValueOut out(val_out, rec_out + k + 1);
  for (uint32_t j = 0; j < 8; ++j) out.put((uint32_t)(ts >> (56 - 8 * j)) & 0xFF);
  if (w.op != kWriteDelete) {
    out.put('{');
    bool first = true;
    for (uint32_t c = 0; c < w.sel.nc; ++c) {
      const bool set = w.setmask >> c & 1;
      uint64_t at = 0, len = kSlotNone;
      if (!set) {
        slots.get(c, &at, &len);
        if (len == kSlotNone) continue;
      }
      if (!first) out.put(',');
      first = false;
      out.put('"');
      for (uint32_t j = w.sel.col_at[c]; j < w.sel.col_at[c + 1]; ++j) esc_put(out, w.sel.bytes[j]);
      out.put('"');
      out.put(':');
      out.put('"');
      if (set) {
        const uint32_t j = w.cell_of[c];
        for (uint64_t b = off[j]; b < off[j + 1]; ++b) esc_put(out, cells[b]);
      } else {
        old.seek(at);
        EscTo<ValueOut> sink{out};
        json_walk(old, sink, true);
      }
      out.put('"');
    }
    out.put('}');
  }
  out.finish();
  *out.r = '\n';
}

}  // namespace cb
