// liverow_driver.cpp — prints cb::value_dead (lsmt_amd/csrc/liverow.hpp, the
// dead-row rule behind cb_tables_count, cb_tables_scan_live and
// cb_tables_compact_live) without a device. Built by tests/test_live_cpu.py
// under the address and undefined-behaviour sanitizers and run as a child
// process.
//
// stdin: decoded value lengths (the line index's vdl), one per line, decimal.
// stdout, one line per input line: "LEN 1" when a value of that length is
// dead, else "LEN 0".
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "liverow.hpp"

// (the rule is usable in constant expressions, as a kernel's template
// argument or static_assert would use it)
static_assert(cb::value_dead(0) && cb::value_dead(8) && !cb::value_dead(7) && !cb::value_dead(9), "liverow.hpp");

int main() {
  uint64_t v;
  while (std::scanf(" %" SCNu64, &v) == 1) {
    if (v > 0xFFFFFFFFull) return 2;
    std::printf("%" PRIu64 " %d\n", v, cb::value_dead((uint32_t)v) ? 1 : 0);
  }
  return std::feof(stdin) ? 0 : 2;
}
