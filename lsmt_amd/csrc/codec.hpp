// codec.hpp — the prost wire format of BloomProto, ZoneMapProto and TableMeta
// (DESIGN.md "Persistence") on the host alone: sizes, headers and the parser
// of untrusted bytes. Nothing here touches a device, so all of it also runs
// (and is tested) on a machine without one. A failed parse returns CB_EDECODE
// and leaves the message for cb_last_error in `err`; the C entry points
// (capi_filter.cpp) report it and do the device work.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "cassbloom.h"

namespace cbx {
namespace codec {

uint64_t varint_len(uint64_t v);
// 0x0A varint(m): the BloomProto header written before m 0/1 bytes.
size_t put_bloom_header(uint8_t* p, uint64_t m);
// Bytes of an encoded BloomProto of m bits (an empty packed field is omitted).
inline uint64_t bloom_len(uint64_t m) { return m ? 1 + varint_len(m) + m : 0; }

// Rust's str::from_utf8 acceptance.
bool utf8_ok(const uint8_t* p, uint64_t n);

// A decoded BloomProto: m bytes of 0 / 1 at src. A message that is exactly
// one packed run of single-byte 0/1 varints (what to_bytes writes) is not
// copied: src points into the input; anything else is gathered in `bits`.
struct BloomBits {
  const uint8_t* src = nullptr;
  uint64_t m = 0;
  std::vector<uint8_t> bits;
};
int parse_bloom(const uint8_t* in, uint64_t len, BloomBits& out, std::string& err);

// One pass over a TableMeta message: the spans of every `bloom` (field 1)
// occurrence, and the last `min` / `max` of every `zone_map` (field 2)
// occurrence — prost's merge of a repeated singular message field is the
// decode of the concatenated payloads, so bloom spans are concatenated and
// zone strings are last-wins.
struct MetaScan {
  std::vector<std::pair<const uint8_t*, uint64_t>> bloom;
  bool has_zone = false, has_min = false, has_max = false;
  const uint8_t *min = nullptr, *max = nullptr;
  uint64_t min_len = 0, max_len = 0;
};
int scan_meta(const uint8_t* in, uint64_t len, MetaScan& ms, std::string& err);

// A whole TableMeta: the scan, and the bits of its bloom when it has one
// (several occurrences are parsed from `cat`, their concatenation).
struct MetaParse {
  MetaScan scan;
  BloomBits bloom;
  std::vector<uint8_t> cat;
  bool has_bloom() const { return !scan.bloom.empty(); }
};
int parse_meta(const uint8_t* in, uint64_t len, MetaParse& out, std::string& err);

// TableMeta{bloom, zone_map}.encode without the bloom's m 0/1 bytes (those
// come from the device): `head` is everything before them, `zone` everything
// after, total the whole message's length.
struct MetaFrame {
  uint8_t head[32];
  size_t head_len = 0;
  std::vector<uint8_t> zone;
  uint64_t total = 0;
};
void meta_frame(bool has_bloom, uint64_t m, const cb_zone_bounds* zone, MetaFrame& out);

}  // namespace codec
}  // namespace cbx
