// rowjson_driver.cpp — prints cb::row_matches (lsmt_amd/csrc/rowjson.hpp, the
// row rule behind cb_tables_count_where, cb_scan_match and cb_row_matches)
// without a device, through both of its readers: the decoded bytes and the
// value's base64 text decoded on the fly. Built by tests/test_where_cpu.py
// under the address and undefined-behaviour sanitizers and run as a child
// process.
//
// stdin, one request per line ("-" stands for an empty string, HEX is lower
// case):
//   M SKIP KEY VALUE TEXT NC (COL VAL PART){NC}
//       KEY, VALUE, COL, VAL in hex; TEXT = VALUE's STANDARD base64 text
// stdout, one line per request: "d t" (the verdicts over VALUE and over TEXT,
// 1 or 0), or "E" when where_check refuses the predicate. Every input is
// copied into a heap block of exactly its size first, so a read past it is
// the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rowjson.hpp"

namespace {

using Block = std::unique_ptr<uint8_t[]>;

Block exact(const std::string& bytes) {
  Block b(new uint8_t[bytes.size() ? bytes.size() : 1]);
  if (!bytes.empty()) std::memcpy(b.get(), bytes.data(), bytes.size());
  return b;
}

int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

bool unhex(const std::string& h, std::string* out) {
  out->clear();
  if (h == "-") return true;
  if (h.size() % 2) return false;
  for (size_t i = 0; i < h.size(); i += 2) {
    const int a = hex(h[i]), b = hex(h[i + 1]);
    if (a < 0 || b < 0) return false;
    out->push_back((char)(a << 4 | b));
  }
  return true;
}

}  // namespace

int main() {
  std::string line;
  auto pred = std::make_unique<cb::WherePred>();
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, key_h, value_h, text;
    uint64_t skip = 0, nc = 0;
    if (!(in >> op >> skip >> key_h >> value_h >> text >> nc) || op != "M" || skip > 0xFFFFFFFFull || nc > 64) return 2;
    std::string key, value;
    if (!unhex(key_h, &key) || !unhex(value_h, &value)) return 2;
    if (text == "-") text.clear();
    if (text.size() != (value.size() + 2) / 3 * 4) return 2;  // B64Bytes' precondition
    std::string cols, vals;
    std::vector<uint64_t> col_off{0}, val_off{0};
    std::vector<int32_t> part;
    for (uint64_t i = 0; i < nc; ++i) {
      std::string ch, vh, c, v;
      long long p;
      if (!(in >> ch >> vh >> p) || !unhex(ch, &c) || !unhex(vh, &v)) return 2;
      cols += c;
      vals += v;
      col_off.push_back(cols.size());
      val_off.push_back(vals.size());
      part.push_back((int32_t)p);
    }
    const Block cb_ = exact(cols), vb = exact(vals), kb = exact(key), db = exact(value), tb = exact(text);
    std::unique_ptr<uint64_t[]> co(new uint64_t[nc + 1]), vo(new uint64_t[nc + 1]);
    std::unique_ptr<int32_t[]> pa(new int32_t[nc ? nc : 1]);
    std::memcpy(co.get(), col_off.data(), (nc + 1) * 8);
    std::memcpy(vo.get(), val_off.data(), (nc + 1) * 8);
    if (nc) std::memcpy(pa.get(), part.data(), nc * 4);
    if (cb::where_check(cb_.get(), co.get(), vb.get(), vo.get(), pa.get(), (uint32_t)nc)) {
      std::puts("E");
      continue;
    }
    cb::where_pack(cb_.get(), co.get(), vb.get(), vo.get(), pa.get(), (uint32_t)nc, pred.get());
    cb::DecodedBytes d(db.get(), value.size());
    cb::B64Bytes<cb::TextByBytes> t(cb::TextByBytes{tb.get()}, value.size());
    const bool md = cb::row_matches(*pred, kb.get(), key.size(), (uint32_t)skip, d);
    const bool mt = cb::row_matches(*pred, kb.get(), key.size(), (uint32_t)skip, t);
    std::printf("%d %d\n", md ? 1 : 0, mt ? 1 : 0);
  }
  return std::cin.eof() ? 0 : 2;
}
