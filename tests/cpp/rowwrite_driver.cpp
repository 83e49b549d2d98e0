// rowwrite_driver.cpp — prints cb::write_size / cb::write_emit
// (lsmt_amd/csrc/rowwrite.hpp, the rule behind cb_rows_write and cb_row_write)
// without a device. Built by tests/test_write_cpu.py under the address and
// undefined-behaviour sanitizers and run as a child process.
//
// stdin, one request per line ("-" stands for an empty string, HEX is lower
// case):
//   W OP NK TS HASOLD NS OLD NC (COL SET){NC} NCELLS (CELL){NCELLS}
//       NS, OLD, COL, CELL in hex; OP 0 insert, 1 update, 2 delete
// stdout, one line per request: "FLAGS KEY VALUE RECORD" (hex, "-" for an empty
// string), or "E" when write_check refuses the statement or the cells do not
// make a row. Every input is copied into a heap block of exactly its size first
// and the three outputs are written into blocks of exactly their lengths, so a
// read or a write past either is the sanitizer's; an output shorter than its
// length shows as its filler.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rowwrite.hpp"

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

void print_hex(const uint8_t* p, uint64_t n) {
  if (!n) std::fputs("-", stdout);
  for (uint64_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}

}  // namespace

int main() {
  std::string line;
  auto w = std::make_unique<cb::WriteCols>();
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string tag, ns_h, old_h, ns, old;
    int op = 0, has_old = 0;
    uint64_t nk = 0, ts = 0, nc = 0, ncells = 0;
    if (!(in >> tag >> op >> nk >> ts >> has_old >> ns_h >> old_h >> nc) || tag != "W" || nc > 64 || nk > 64) return 2;
    if (!unhex(ns_h, &ns) || !unhex(old_h, &old)) return 2;
    std::string cols, cells;
    std::vector<uint64_t> col_off{0}, cell_off{0};
    std::vector<uint8_t> set;
    for (uint64_t i = 0; i < nc; ++i) {
      std::string ch, c;
      int s;
      if (!(in >> ch >> s) || !unhex(ch, &c)) return 2;
      cols += c;
      col_off.push_back(cols.size());
      set.push_back((uint8_t)s);
    }
    if (!(in >> ncells) || ncells > 128) return 2;
    for (uint64_t i = 0; i < ncells; ++i) {
      std::string ch, c;
      if (!(in >> ch) || !unhex(ch, &c)) return 2;
      cells += c;
      cell_off.push_back(cells.size());
    }
    const Block nb = exact(ns), ob = exact(old), cb_ = exact(cols), db = exact(cells);
    std::unique_ptr<uint64_t[]> co(new uint64_t[nc + 1]), ce(new uint64_t[ncells + 1]);
    std::unique_ptr<uint8_t[]> se(new uint8_t[nc ? nc : 1]);
    std::memcpy(co.get(), col_off.data(), (nc + 1) * 8);
    std::memcpy(ce.get(), cell_off.data(), (ncells + 1) * 8);
    if (nc) std::memcpy(se.get(), set.data(), nc);
    if (cb::write_check(nb.get(), ns.size(), (uint32_t)nk, cb_.get(), co.get(), se.get(), (uint32_t)nc, op) ||
        (has_old && op != cb::kWriteUpdate)) {
      std::puts("E");
      continue;
    }
    cb::write_pack((uint32_t)nk, cb_.get(), co.get(), se.get(), (uint32_t)nc, op, w.get());
    if (w->width != ncells) {
      std::puts("E");
      continue;
    }
    cb::DecodedBytes o(ob.get(), has_old ? old.size() : 0);
    cb::ArraySlots slots;
    uint8_t flags = 0;
    uint64_t kl = 0, vl = 0, rl = 0;
    cb::write_size(*w, ns.size(), cb::key_ctl(nb.get(), ns.size()), db.get(), ce.get(), has_old != 0, o, slots, &flags,
                   &kl, &vl, &rl);
    Block key(new uint8_t[kl ? kl : 1]), val(new uint8_t[vl ? vl : 1]), rec(new uint8_t[rl ? rl : 1]);
    std::memset(key.get(), 0xAA, kl ? kl : 1);
    std::memset(val.get(), 0xAA, vl ? vl : 1);
    std::memset(rec.get(), 0xAA, rl ? rl : 1);
    cb::write_emit(*w, nb.get(), ns.size(), db.get(), ce.get(), ts, o, flags, slots, key.get(), val.get(), rec.get());
    std::printf("%u ", (unsigned)flags);
    print_hex(key.get(), kl);
    std::fputs(" ", stdout);
    print_hex(val.get(), vl);
    std::fputs(" ", stdout);
    print_hex(rec.get(), rl);
    std::puts("");
  }
  return std::cin.eof() ? 0 : 2;
}
