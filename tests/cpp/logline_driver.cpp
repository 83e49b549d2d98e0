// logline_driver.cpp — prints cb::log_line (lsmt_amd/csrc/logline.hpp, the
// rule behind cb_log_replay and cb_log_line) without a device. Built by
// tests/test_replay_cpu.py under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin, one request per line: "L HEX", the piece in lower-case hex ("-" is
// the empty piece). stdout, one line per request: "KIND KEYLEN VALUELEN".
// Every piece is copied into a heap block of exactly its size first, so a
// read past either end is the sanitizer's. The verdict is taken twice, by
// log_line and by log_line_at with the TAB found here, and must agree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include "logline.hpp"

namespace {

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
  std::string line, piece;
  while (std::getline(std::cin, line)) {
    if (line.size() < 3 || line[0] != 'L' || line[1] != ' ' || !unhex(line.substr(2), &piece)) return 2;
    const size_t n = piece.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(block.get(), piece.data(), n);
    const uint8_t* p = block.get();
    const cb::LogLine v = cb::log_line(p, n);
    const void* t = n ? std::memchr(p, '\t', n) : nullptr;
    const cb::LogLine w = cb::log_line_at(p, n, t ? (uint64_t)((const uint8_t*)t - p) : (uint64_t)n);
    if (v.kind != w.kind || v.klen != w.klen || v.vdl != w.vdl) return 3;
    std::printf("%d %llu %llu\n", v.kind, (unsigned long long)v.klen, (unsigned long long)v.vdl);
  }
  return std::cin.eof() ? 0 : 2;
}
