// codec_driver.cpp — runs the host codec (lsmt_amd/csrc/codec.cpp) over
// untrusted TableMeta bytes without a device. Built by tests/test_codec_cpu.py
// together with codec.cpp under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin: records of a little-endian u32 length and that many bytes.
// stdout, one line per record:
//   rc has_bloom m set-bits has_zone min max
// set-bits is a comma-separated list, min / max are hex; "-" stands for an
// empty list, "none" for an absent bound, "" is written as "empty".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "codec.hpp"

namespace {

std::string hex_or(bool has, const uint8_t* p, uint64_t n) {
  if (!has) return "none";
  if (!n) return "empty";
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint64_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

}  // namespace

int main() {
  for (;;) {
    uint8_t lb[4];
    const size_t got = fread(lb, 1, 4, stdin);
    if (got == 0) break;
    if (got != 4) return 2;
    const uint32_t len = lb[0] | lb[1] << 8 | lb[2] << 16 | (uint32_t)lb[3] << 24;
    // an allocation of exactly len bytes: a read past the input is a report
    std::unique_ptr<uint8_t[]> in(new uint8_t[len]);
    if (len && fread(in.get(), 1, len, stdin) != len) return 2;
    cbx::codec::MetaParse mp;
    std::string err;
    const int rc = cbx::codec::parse_meta(in.get(), len, mp, err);
    if (rc) {
      if (err.empty()) return 3;  // every refusal carries its message
      printf("%d 0 0 - 0 none none\n", rc);
      continue;
    }
    const cbx::codec::MetaScan& ms = mp.scan;
    std::string bits;
    for (uint64_t i = 0; mp.has_bloom() && i < mp.bloom.m; ++i)
      if (mp.bloom.src[i]) bits += (bits.empty() ? "" : ",") + std::to_string(i);
    printf("0 %d %llu %s %d %s %s\n", (int)mp.has_bloom(), (unsigned long long)(mp.has_bloom() ? mp.bloom.m : 0),
           bits.empty() ? "-" : bits.c_str(), (int)ms.has_zone, hex_or(ms.has_min, ms.min, ms.min_len).c_str(),
           hex_or(ms.has_max, ms.max, ms.max_len).c_str());
  }
  return 0;
}
