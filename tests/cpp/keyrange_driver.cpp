// keyrange_driver.cpp — prints cb::key_prefix_end's answers
// (lsmt_amd/csrc/keyrange.hpp, the code behind cb_key_prefix_end) without a
// device. Built by tests/test_scan_cpu.py under the address and
// undefined-behaviour sanitizers and run as a child process.
//
// stdin: lines "e HEX" (the end of prefix HEX; "-" is the empty string) or
// "c HEXP HEXK" (is P <= K < end(P)?).
// stdout, one line per input line: "e 0" / "e 1 HEX", or "c 0" / "c 1".
// Every buffer is a heap block of exactly the length in use, so a byte read
// or written past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "keyrange.hpp"

namespace {

bool unhex(const char* s, std::unique_ptr<uint8_t[]>& out, uint64_t& n) {
  const size_t len = std::strcmp(s, "-") ? std::strlen(s) : 0;
  if (len & 1) return false;
  n = len / 2;
  out.reset(new uint8_t[n ? n : 1]);
  for (uint64_t i = 0; i < n; ++i) {
    unsigned v;
    if (std::sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

}  // namespace

int main() {
  char kind, a[4200], b[4200];
  while (std::scanf(" %c %4100s", &kind, a) == 2) {
    std::unique_ptr<uint8_t[]> p, k;
    uint64_t pn = 0, kn = 0, en = 0;
    if (!unhex(a, p, pn)) return 2;
    std::unique_ptr<uint8_t[]> end(new uint8_t[pn ? pn : 1]);
    const bool has = cb::key_prefix_end(p.get(), pn, end.get(), &en);
    if (kind == 'e') {
      std::printf("e %d", (int)has);
      if (has) {
        std::printf(" ");
        for (uint64_t i = 0; i < en; ++i) std::printf("%02x", end[i]);
      }
      std::printf("\n");
    } else if (kind == 'c') {
      if (std::scanf(" %4100s", b) != 1 || !unhex(b, k, kn)) return 2;
      const bool in = cb::key_cmp(p.get(), pn, k.get(), kn) <= 0 && (!has || cb::key_cmp(k.get(), kn, end.get(), en) < 0);
      std::printf("c %d\n", (int)in);
    } else {
      return 2;
    }
  }
  return std::feof(stdin) ? 0 : 2;
}
