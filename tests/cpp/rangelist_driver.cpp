// rangelist_driver.cpp — prints the answers of cb::range_list_first_bad and
// cb::prefix_list_to_ranges (lsmt_amd/csrc/keyrange.hpp, the checks behind
// cb_tables_scan_many and cb_tables_scan_prefixes) without a device. Built by
// tests/test_scan_many_cpu.py under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin, one list per line ("-" is the empty string, U is last_unbounded):
//   r U N HEX*2N        N ranges as lo, hi pairs
//   o U N HEX OFF*2N+1  N ranges as raw bytes and raw offsets
//   p N HEX*N           N prefixes
//   q N HEX OFF*N+1     N prefixes as raw bytes and raw offsets
// stdout, one line per input line:
//   r / o:  "r IDX"                       (range_list_first_bad)
//   p / q:  "p BAD"                       (prefix_list_to_ranges refused BAD), or
//           "p -1 U IDX HEX OFF*2N+1"     (its lists, and their first bad range)
// Every input buffer is a heap block of exactly the length in use, so a byte
// read past it is the sanitizer's to report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "keyrange.hpp"

namespace {

bool unhex(const char* s, std::vector<uint8_t>& out) {
  const size_t len = std::strcmp(s, "-") ? std::strlen(s) : 0;
  if (len & 1) return false;
  for (size_t i = 0; i < len / 2; ++i) {
    unsigned v;
    if (std::sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}

// Exactly-sized heap copies (a vector's capacity may hide an overrun).
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

void put_hex(const std::vector<uint8_t>& b) {
  if (b.empty()) std::printf("-");
  for (uint8_t x : b) std::printf("%02x", x);
}

}  // namespace

int main() {
  char kind, tok[4200];
  while (std::scanf(" %c", &kind) == 1) {
    const bool ranges = kind == 'r' || kind == 'o', raw = kind == 'o' || kind == 'q';
    if (!ranges && kind != 'p' && kind != 'q') return 2;
    unsigned unb = 0;
    uint64_t n = 0;
    if (ranges && std::scanf(" %u", &unb) != 1) return 2;
    if (std::scanf(" %" SCNu64, &n) != 1 || n > 4096) return 2;
    const uint64_t parts = ranges ? 2 * n : n;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    if (raw) {
      if (std::scanf(" %4100s", tok) != 1 || !unhex(tok, bytes)) return 2;
      for (uint64_t i = 0; i <= parts; ++i) {
        uint64_t o;
        if (std::scanf(" %" SCNu64, &o) != 1) return 2;
        off.push_back(o);
      }
    } else {
      off.push_back(0);
      for (uint64_t i = 0; i < parts; ++i) {
        if (std::scanf(" %4100s", tok) != 1 || !unhex(tok, bytes)) return 2;
        off.push_back(bytes.size());
      }
    }
    const std::unique_ptr<uint8_t[]> b = exact(bytes);
    const std::unique_ptr<uint64_t[]> o = exact(off);
    if (ranges) {
      std::printf("r %" PRId64 "\n", cb::range_list_first_bad(b.get(), o.get(), n, unb != 0));
      continue;
    }
    std::vector<uint8_t> rb(7, 0xAA);  // (stale contents: the function clears them)
    std::vector<uint64_t> ro(3, 99);
    bool last_unbounded = true;
    const int64_t bad = cb::prefix_list_to_ranges(b.get(), o.get(), n, rb, ro, &last_unbounded);
    if (bad >= 0) {
      std::printf("p %" PRId64 "\n", bad);
      continue;
    }
    if (ro.size() != 2 * n + 1 || ro.back() != rb.size()) return 3;
    const std::unique_ptr<uint8_t[]> eb = exact(rb);
    const std::unique_ptr<uint64_t[]> eo = exact(ro);
    std::printf("p -1 %d %" PRId64 " ", (int)last_unbounded, cb::range_list_first_bad(eb.get(), eo.get(), n, last_unbounded));
    put_hex(rb);
    for (uint64_t x : ro) std::printf(" %" PRIu64, x);
    std::printf("\n");
  }
  return std::feof(stdin) ? 0 : 2;
}
