// rowselect_driver.cpp — prints cb::select_size / cb::select_write
// (lsmt_amd/csrc/rowselect.hpp, the rule behind cb_scan_select, cb_rows_select
// and cb_row_select) without a device. Built by tests/test_select_cpu.py under
// the address and undefined-behaviour sanitizers and run as a child process.
//
// stdin, one request per line ("-" stands for an empty string, HEX is lower
// case):
//   S MODE SKIP ABSENT KEY VALUE NC (COL PART CAST){NC}
//       KEY, VALUE, COL in hex; MODE 0 or 1; ABSENT 0 or 1
// stdout, one line per request: "FLAGS LEN TEXT" (TEXT in hex, "-" when the
// row has none), or "E" when select_check refuses the selection. Every input
// is copied into a heap block of exactly its size first and the text is
// written into a block of exactly LEN bytes, so a read or a write past either
// is the sanitizer's; a text shorter than LEN shows as its filler.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rowselect.hpp"

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
  auto sel = std::make_unique<cb::SelectCols>();
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, key_h, value_h;
    uint64_t skip = 0, nc = 0;
    int mode = 0, absent = 0;
    if (!(in >> op >> mode >> skip >> absent >> key_h >> value_h >> nc) || op != "S" || skip > 0xFFFFFFFFull || nc > 64)
      return 2;
    std::string key, value;
    if (!unhex(key_h, &key) || !unhex(value_h, &value)) return 2;
    std::string cols;
    std::vector<uint64_t> col_off{0};
    std::vector<int32_t> part;
    std::vector<uint8_t> cast;
    for (uint64_t i = 0; i < nc; ++i) {
      std::string ch, c;
      long long p, k;
      if (!(in >> ch >> p >> k) || !unhex(ch, &c)) return 2;
      cols += c;
      col_off.push_back(cols.size());
      part.push_back((int32_t)p);
      cast.push_back((uint8_t)k);
    }
    const Block cb_ = exact(cols), kb = exact(key), db = exact(value);
    std::unique_ptr<uint64_t[]> co(new uint64_t[nc + 1]);
    std::unique_ptr<int32_t[]> pa(new int32_t[nc ? nc : 1]);
    std::unique_ptr<uint8_t[]> ca(new uint8_t[nc ? nc : 1]);
    std::memcpy(co.get(), col_off.data(), (nc + 1) * 8);
    if (nc) std::memcpy(pa.get(), part.data(), nc * 4);
    if (nc) std::memcpy(ca.get(), cast.data(), nc);
    if (cb::select_check(cb_.get(), co.get(), pa.get(), ca.get(), (uint32_t)nc)) {
      std::puts("E");
      continue;
    }
    cb::select_pack(cb_.get(), co.get(), pa.get(), ca.get(), (uint32_t)nc, sel.get());
    cb::DecodedBytes v(db.get(), value.size());
    cb::ArraySlots slots;
    uint8_t flags = 0;
    const uint64_t len = cb::select_size(*sel, kb.get(), key.size(), (uint32_t)skip, absent != 0, v, mode, slots, &flags);
    std::printf("%u %llu ", (unsigned)flags, (unsigned long long)len);
    if (!(flags & cb::kRowText)) {
      std::puts("-");
      continue;
    }
    Block text(new uint8_t[len ? len : 1]);
    std::memset(text.get(), 0xAA, len ? len : 1);
    cb::select_write(*sel, kb.get(), key.size(), (uint32_t)skip, v, mode, flags, slots, text.get());
    for (uint64_t i = 0; i < len; ++i) std::printf("%02x", text[i]);
    std::puts(len ? "" : "-");
  }
  return std::cin.eof() ? 0 : 2;
}
