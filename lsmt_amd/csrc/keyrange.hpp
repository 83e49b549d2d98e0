// keyrange.hpp — host-only arithmetic on key ranges (no device code: tested
// on the CPU under sanitizers, tests/cpp/keyrange_driver.cpp and
// tests/cpp/rangelist_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

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

// A list of nr ranges for one batched scan (cb_tables_scan_many): range r =
// [lo_r, hi_r) with lo_r = bounds[bound_off[2r] .. bound_off[2r+1]) and hi_r =
// bounds[bound_off[2r+1] .. bound_off[2r+2]); with last_unbounded the last
// range has no hi (its hi bytes are not read). The ordering rule, which makes
// every table's cuts disjoint runs of lines in ascending order:
//   bound_off[2r] <= bound_off[2r+1] <= bound_off[2r+2]          for every r,
//   lo_r <= lo_{r+1} and hi_r <= lo_{r+1} (key_cmp)              for r < nr-1.
// An empty range (lo_r >= hi_r) and touching ranges (hi_r == lo_{r+1}) are
// legal. Returns the first r that breaks the rule, or -1: r's own offsets
// decrease, or its successor starts below lo_r or hi_r; a successor whose lo
// offsets decrease (its bytes cannot be read) is itself the one reported. No
// byte is read through an offset pair that decreases.
inline int64_t range_list_first_bad(const uint8_t* bounds, const uint64_t* bound_off, uint64_t nr,
                                    bool last_unbounded) {
  (void)last_unbounded;  // only the last range may lack a hi, and no rule reads the last hi
  for (uint64_t r = 0; r < nr; ++r) {
    const uint64_t* o = bound_off + 2 * r;
    if (o[0] > o[1] || o[1] > o[2]) return (int64_t)r;
    if (r + 1 == nr) break;
    if (o[2] > o[3]) return (int64_t)(r + 1);
    const uint8_t* nlo = bounds + o[2];
    const uint64_t nlo_len = o[3] - o[2];
    if (key_cmp(bounds + o[0], o[1] - o[0], nlo, nlo_len) > 0) return (int64_t)r;
    if (key_cmp(bounds + o[1], o[2] - o[1], nlo, nlo_len) > 0) return (int64_t)r;
  }
  return -1;
}

// A list of np prefixes (prefix r = prefixes[prefix_off[r] .. prefix_off[r+1]))
// as a range list: range r = [p_r, key_prefix_end(p_r)), its two bounds
// appended to bounds and their three offsets to bound_off (2 np + 1 entries;
// both vectors are cleared first). A prefix without an end (empty, all 0xFF)
// may only be the last: *last_unbounded says whether it is. Returns -1, or
// the first prefix that cannot be taken: its offsets decrease, or it has no
// end and is not the last (the lists are then incomplete).
inline int64_t prefix_list_to_ranges(const uint8_t* prefixes, const uint64_t* prefix_off, uint64_t np,
                                     std::vector<uint8_t>& bounds, std::vector<uint64_t>& bound_off,
                                     bool* last_unbounded) {
  bounds.clear();
  bound_off.assign(1, 0);
  *last_unbounded = false;
  for (uint64_t r = 0; r < np; ++r) {
    if (prefix_off[r] > prefix_off[r + 1]) return (int64_t)r;
    const uint8_t* p = prefixes + prefix_off[r];
    const uint64_t len = prefix_off[r + 1] - prefix_off[r];
    if (len) bounds.insert(bounds.end(), p, p + len);
    bound_off.push_back(bounds.size());
    const size_t at = bounds.size();
    bounds.resize(at + len);
    uint64_t end_len = 0;
    const bool has_end = key_prefix_end(p, len, bounds.data() + at, &end_len);
    bounds.resize(at + end_len);
    bound_off.push_back(bounds.size());
    if (!has_end) {
      if (r + 1 != np) return (int64_t)r;
      *last_unbounded = true;
    }
  }
  return -1;
}

}  // namespace cb
