// keyrange.hpp — host-only arithmetic on key ranges (no device code: tested
// on the CPU under sanitizers, tests/cpp/keyrange_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cb {

// The exclusive upper bound of "starts with prefix" in byte order: the prefix
// without its trailing 0xFF bytes, its last remaining byte incremented
// (p <= k < end iff k starts with p). out receives at most len bytes; returns
// false, with *out_len = 0, when nothing remains (an empty prefix, or all
// 0xFF): every key from the prefix on starts with it. out may alias prefix.
inline bool key_prefix_end(const uint8_t* prefix, uint64_t len, uint8_t* out, uint64_t* out_len) {
  uint64_t n = len;
  while (n && prefix[n - 1] == 0xFF) --n;
  *out_len = n;
  if (!n) return false;
  for (uint64_t i = 0; i + 1 < n; ++i) out[i] = prefix[i];
  out[n - 1] = (uint8_t)(prefix[n - 1] + 1);
  return true;
}

// Rust's `Ord for [u8]`: byte-wise, then length.
inline int key_cmp(const uint8_t* a, uint64_t al, const uint8_t* b, uint64_t bl) {
  const uint64_t n = al < bl ? al : bl;
  for (uint64_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

}  // namespace cb
