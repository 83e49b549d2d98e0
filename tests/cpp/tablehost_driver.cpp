// tablehost_driver.cpp — prints the answers of the host-only code behind the
// SSTable entries (lsmt_amd/csrc/tablehost.hpp) without a device. Built by
// tests/test_tablehost_cpu.py under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin, one request per line (numbers in decimal):
//   g NT S0 .. S(NT-1)   the wide walk's groups of NT tables in these slots
//   i NT                 the same with no slot list (table t is slot t)
//   c K B0 .. B(K-1)     a carver taking K parts of these sizes
//   s COUNT KB VB        a scan result's layout
//   f N K V              the flush's file bound
//   l MASK B0 B1 B2 B3   the flush's staged block; bit i of MASK: input i is host memory
// stdout, one line per request:
//   g/i: "g NEED NG" then "KIND LO GN PAD" per group
//   c:   "c" the K offsets, then the total
//   s:   "s" the five offsets, then the total
//   f:   "f BOUND"
//   l:   "l" the four offsets ("-" for a device input), then the total
// Every array is a heap block of exactly the length in use, so a read or
// write past it is the sanitizer's to report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <memory>

#include "tablehost.hpp"

namespace {

bool read_u64(uint64_t* v) { return std::scanf(" %" SCNu64, v) == 1; }

bool groups(bool with_slots) {
  uint64_t nt = 0;
  if (!read_u64(&nt) || nt > (1u << 20)) return false;
  std::unique_ptr<uint32_t[]> slots;
  if (with_slots) {
    slots.reset(new uint32_t[nt]);
    for (uint64_t i = 0; i < nt; ++i) {
      uint64_t v;
      if (!read_u64(&v)) return false;
      slots[i] = (uint32_t)v;
    }
  }
  const uint32_t ng = cb::wide_group_count((uint32_t)nt);
  std::unique_ptr<cb::WideGroup[]> g(new cb::WideGroup[ng]);
  const bool need = cb::wide_groups(slots.get(), (uint32_t)nt, g.get());
  std::printf("g %d %u", (int)need, ng);
  for (uint32_t i = 0; i < ng; ++i) std::printf(" %u %u %u %u", g[i].kind, g[i].lo, g[i].gn, g[i].pad);
  std::printf("\n");
  return true;
}

bool carve() {
  uint64_t k = 0;
  if (!read_u64(&k) || k > 4096) return false;
  cb::Carver c;
  std::printf("c");
  for (uint64_t i = 0; i < k; ++i) {
    uint64_t b;
    if (!read_u64(&b)) return false;
    std::printf(" %zu", c.take(b));
  }
  std::printf(" %zu\n", c.total());
  return true;
}

bool scan() {
  uint64_t count, kb, vb;
  if (!read_u64(&count) || !read_u64(&kb) || !read_u64(&vb)) return false;
  size_t o[5];
  const size_t total = cb::scan_layout(count, kb, vb, o);
  std::printf("s %zu %zu %zu %zu %zu %zu\n", o[0], o[1], o[2], o[3], o[4], total);
  return true;
}

bool bound() {
  uint64_t n, k, v;
  if (!read_u64(&n) || !read_u64(&k) || !read_u64(&v)) return false;
  std::printf("f %" PRIu64 "\n", cb::flush_file_bound(n, k, v));
  return true;
}

bool stage() {
  uint64_t mask, b[4];
  if (!read_u64(&mask)) return false;
  for (uint64_t& x : b)
    if (!read_u64(&x)) return false;
  const bool host[4] = {(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0};
  const uint64_t bytes[4] = {b[0], b[1], b[2], b[3]};
  const cb::FlushStage st = cb::flush_stage_layout(host, bytes);
  std::printf("l");
  for (int i = 0; i < 4; ++i) {
    if (host[i])
      std::printf(" %zu", st.off[i]);
    else
      std::printf(" -");
  }
  std::printf(" %zu\n", st.total);
  return true;
}

}  // namespace

int main() {
  static_assert(sizeof(cb::WideGroup) == 16, "the wide walk reads 16-byte groups");
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    bool ok = false;
    switch (kind) {
      case 'g': ok = groups(true); break;
      case 'i': ok = groups(false); break;
      case 'c': ok = carve(); break;
      case 's': ok = scan(); break;
      case 'f': ok = bound(); break;
      case 'l': ok = stage(); break;
    }
    if (!ok) return 2;
  }
  return std::feof(stdin) ? 0 : 2;
}
