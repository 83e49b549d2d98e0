// rowts_driver.cpp — prints cb::value_ts, cb::decoded_ts and cb::lww_beats
// (lsmt_amd/csrc/rowts.hpp, the timestamp rule behind cb_tables_compact_lww,
// cb_tables_scan_lww, cb_tables_count_lww and cb_scan_ts) without a device.
// Built by tests/test_lww_cpu.py under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin, one request per line ("-" stands for an empty string):
//   T VDL TEXT         -> value_ts of the base64 text TEXT, decoded length VDL
//   D HEX              -> decoded_ts of the bytes HEX spells
//   B TSA IDXA TSB IDXB -> lww_beats, "1" or "0"
// stdout: one decimal result per request. Every input is copied into a heap
// block of exactly its size first, so a read past it is the sanitizer's.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "rowts.hpp"

// (the rule is usable in constant expressions)
static_assert(cb::lww_beats(2, 5, 1, 0) && !cb::lww_beats(1, 0, 2, 5) && cb::lww_beats(7, 2, 7, 5) &&
                  !cb::lww_beats(7, 5, 7, 2),
              "rowts.hpp");
static_assert(cb::b64_sextet('A') == 0 && cb::b64_sextet('Z') == 25 && cb::b64_sextet('a') == 26 &&
                  cb::b64_sextet('z') == 51 && cb::b64_sextet('0') == 52 && cb::b64_sextet('9') == 61 &&
                  cb::b64_sextet('+') == 62 && cb::b64_sextet('/') == 63,
              "rowts.hpp");

namespace {

std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

}  // namespace

int main() {
  static char line[1 << 16], arg[1 << 16];
  while (std::fgets(line, sizeof line, stdin)) {
    uint64_t a, ia, b, ib;
    if (std::sscanf(line, "T %" SCNu64 " %65535s", &a, arg) == 2) {
      if (a > 0xFFFFFFFFull) return 2;
      const size_t n = std::strcmp(arg, "-") ? std::strlen(arg) : 0;
      if (a >= 8 && n < 12) return 2;  // rowts.hpp's precondition
      const auto t = exact((const uint8_t*)arg, n);
      std::printf("%" PRIu64 "\n", cb::value_ts(t.get(), (uint32_t)a));
    } else if (std::sscanf(line, "D %65535s", arg) == 1) {
      const size_t n = std::strcmp(arg, "-") ? std::strlen(arg) / 2 : 0;
      std::unique_ptr<uint8_t[]> raw(new uint8_t[n ? n : 1]);
      for (size_t i = 0; i < n; ++i) {
        const int h = hex(arg[2 * i]), l = hex(arg[2 * i + 1]);
        if (h < 0 || l < 0) return 2;
        raw[i] = (uint8_t)(h << 4 | l);
      }
      const auto t = exact(raw.get(), n);
      std::printf("%" PRIu64 "\n", cb::decoded_ts(t.get(), n));
    } else if (std::sscanf(line, "B %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &ia, &b, &ib) == 4) {
      std::printf("%d\n", cb::lww_beats(a, ia, b, ib) ? 1 : 0);
    } else {
      return 2;
    }
  }
  return std::feof(stdin) ? 0 : 2;
}
