// codec.cpp — the prost codec's host side (codec.hpp; product side, see
// DESIGN.md "Persistence"). The parser takes untrusted bytes: every read is
// bounded by the span it was given.
#include "codec.hpp"

namespace cbx {
namespace codec {

namespace {

int bad(std::string& err, const char* what) {
  err = what;
  return CB_EDECODE;
}

bool skip_field(const uint8_t*& p, const uint8_t* end, uint32_t wt, uint64_t field, int depth);

bool get_varint(const uint8_t*& p, const uint8_t* end, uint64_t& v) {
  uint64_t r = 0;
  for (int i = 0; i < 10; ++i) {
    if (p >= end) return false;
    const uint8_t b = *p++;
    if (i == 9 && b > 1) return false;  // prost: overflowing varint
    r |= (uint64_t)(b & 0x7F) << (7 * i);
    if (!(b & 0x80)) {
      v = r;
      return true;
    }
  }
  return false;
}

bool skip_group(const uint8_t*& p, const uint8_t* end, uint64_t field, int depth) {
  if (depth > 100) return false;
  for (;;) {
    uint64_t key;
    if (!get_varint(p, end, key) || key > 0xFFFFFFFFull) return false;
    const uint32_t wt = (uint32_t)(key & 7);
    const uint64_t fn = key >> 3;
    if (fn == 0) return false;
    if (wt == 4) return fn == field;
    if (!skip_field(p, end, wt, fn, depth + 1)) return false;
  }
}

bool skip_field(const uint8_t*& p, const uint8_t* end, uint32_t wt, uint64_t field, int depth) {
  uint64_t v;
  switch (wt) {
    case 0: return get_varint(p, end, v);
    case 1:
      if (end - p < 8) return false;
      p += 8;
      return true;
    case 2:
      if (!get_varint(p, end, v) || v > (uint64_t)(end - p)) return false;
      p += v;
      return true;
    case 3: return skip_group(p, end, field, depth);
    case 5:
      if (end - p < 4) return false;
      p += 4;
      return true;
    default: return false;
  }
}

size_t put_varint_buf(uint8_t* p, uint64_t v) {
  size_t n = 0;
  while (v >= 0x80) {
    p[n++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  p[n++] = (uint8_t)v;
  return n;
}

}  // namespace

uint64_t varint_len(uint64_t v) {
  uint64_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

// 0x0A varint(m): the BloomProto header written before m 0/1 bytes.
size_t put_bloom_header(uint8_t* p, uint64_t m) {
  p[0] = 0x0A;  // field 1 (bits), wire type 2 (packed)
  return 1 + put_varint_buf(p + 1, m);
}

// Rust's str::from_utf8 acceptance (prost rejects a `string` field that is
// not well-formed UTF-8). Classifies each lead byte by its range and checks
// the tightened second-byte window that rules out overlongs, surrogates and
// code points above U+10FFFF.
bool utf8_ok(const uint8_t* p, uint64_t n) {
  const uint8_t* end = p + n;
  while (p < end) {
    const uint8_t c = *p;
    if (c < 0x80) {
      ++p;
      continue;
    }
    int need;
    uint8_t lo = 0x80, hi = 0xBF;
    switch (c >> 4) {
      case 0xC:
      case 0xD:
        if (c < 0xC2) return false;
        need = 1;
        break;
      case 0xE:
        need = 2;
        if (c == 0xE0) lo = 0xA0;
        if (c == 0xED) hi = 0x9F;
        break;
      case 0xF:
        if (c > 0xF4) return false;
        need = 3;
        if (c == 0xF0) lo = 0x90;
        if (c == 0xF4) hi = 0x8F;
        break;
      default:
        return false;  // stray continuation byte
    }
    if (end - p <= need) return false;
    if (p[1] < lo || p[1] > hi) return false;
    for (int k = 2; k <= need; ++k)
      if ((p[k] & 0xC0) != 0x80) return false;
    p += need + 1;
  }
  return true;
}

int parse_bloom(const uint8_t* in, uint64_t len, BloomBits& out, std::string& err) {
  const uint8_t* p = in;
  const uint8_t* end = in + len;
  // Fast path: exactly one packed field-1 run of single-byte 0/1 varints (what
  // to_bytes writes) is imported straight from the input buffer.
  std::vector<uint8_t>& bits = out.bits;
  bits.clear();
  const uint8_t* direct = nullptr;
  uint64_t direct_len = 0;
  int runs = 0;
  while (p < end) {
    uint64_t key;
    if (!get_varint(p, end, key) || key > 0xFFFFFFFFull) return bad(err, "BloomProto decode: invalid key");
    const uint32_t wt = (uint32_t)(key & 7);
    const uint64_t fn = key >> 3;
    if (fn == 0) return bad(err, "BloomProto decode: invalid tag value 0");
    if (fn == 1 && wt == 2) {
      uint64_t l;
      if (!get_varint(p, end, l) || l > (uint64_t)(end - p)) return bad(err, "BloomProto decode: bad length");
      const uint8_t* lim = p + l;
      bool simple = true;
      for (const uint8_t* q = p; q < lim; ++q)
        if (*q > 1) {
          simple = false;
          break;
        }
      if (simple && runs == 0 && bits.empty()) {
        direct = p;
        direct_len = l;
        p = lim;
        ++runs;
        continue;
      }
      if (direct) {
        bits.assign(direct, direct + direct_len);
        direct = nullptr;
      }
      while (p < lim) {
        uint64_t v;
        if (!get_varint(p, lim, v)) return bad(err, "BloomProto decode: bad varint");
        bits.push_back(v != 0);
      }
      ++runs;
    } else if (fn == 1 && wt == 0) {
      uint64_t v;
      if (!get_varint(p, end, v)) return bad(err, "BloomProto decode: bad varint");
      if (direct) {
        bits.assign(direct, direct + direct_len);
        direct = nullptr;
      }
      bits.push_back(v != 0);
      ++runs;
    } else if (fn == 1) {
      return bad(err, "BloomProto decode: invalid wire type for field 1");
    } else if (!skip_field(p, end, wt, fn, 0)) {
      return bad(err, "BloomProto decode: malformed unknown field");
    }
  }
  out.src = direct ? direct : bits.data();
  out.m = direct ? direct_len : bits.size();
  return CB_OK;
}

namespace {

int scan_zone(const uint8_t* p, const uint8_t* end, MetaScan& ms, std::string& err) {
  while (p < end) {
    uint64_t key, l;
    if (!get_varint(p, end, key) || key > 0xFFFFFFFFull) return bad(err, "ZoneMapProto decode: invalid key");
    const uint32_t wt = (uint32_t)(key & 7);
    const uint64_t fn = key >> 3;
    if (fn == 0) return bad(err, "ZoneMapProto decode: invalid tag value 0");
    if (fn == 1 || fn == 2) {
      if (wt != 2) return bad(err, "ZoneMapProto decode: invalid wire type");
      if (!get_varint(p, end, l) || l > (uint64_t)(end - p)) return bad(err, "ZoneMapProto decode: bad length");
      if (!utf8_ok(p, l))
        return bad(err, "ZoneMapProto decode: invalid string value: data is not UTF-8 encoded");
      if (fn == 1) {
        ms.min = p;
        ms.min_len = l;
        ms.has_min = true;
      } else {
        ms.max = p;
        ms.max_len = l;
        ms.has_max = true;
      }
      p += l;
    } else if (!skip_field(p, end, wt, fn, 0)) {
      return bad(err, "ZoneMapProto decode: malformed unknown field");
    }
  }
  return CB_OK;
}

}  // namespace

int scan_meta(const uint8_t* in, uint64_t len, MetaScan& ms, std::string& err) {
  const uint8_t* p = in;
  const uint8_t* end = in + len;
  while (p < end) {
    uint64_t key, l;
    if (!get_varint(p, end, key) || key > 0xFFFFFFFFull) return bad(err, "TableMeta decode: invalid key");
    const uint32_t wt = (uint32_t)(key & 7);
    const uint64_t fn = key >> 3;
    if (fn == 0) return bad(err, "TableMeta decode: invalid tag value 0");
    if (fn == 1 || fn == 2) {
      if (wt != 2) return bad(err, "TableMeta decode: invalid wire type");
      if (!get_varint(p, end, l) || l > (uint64_t)(end - p)) return bad(err, "TableMeta decode: bad length");
      if (fn == 1) {
        ms.bloom.emplace_back(p, l);
      } else {
        ms.has_zone = true;
        int rc = scan_zone(p, p + l, ms, err);
        if (rc) return rc;
      }
      p += l;
    } else if (!skip_field(p, end, wt, fn, 0)) {
      return bad(err, "TableMeta decode: malformed unknown field");
    }
  }
  return CB_OK;
}

int parse_meta(const uint8_t* in, uint64_t len, MetaParse& out, std::string& err) {
  int rc = scan_meta(in, len, out.scan, err);
  if (rc || !out.has_bloom()) return rc;
  const auto& spans = out.scan.bloom;
  if (spans.size() == 1) {
    rc = parse_bloom(spans[0].first, spans[0].second, out.bloom, err);
  } else {
    out.cat.clear();
    for (auto& sp : spans) out.cat.insert(out.cat.end(), sp.first, sp.first + sp.second);
    rc = parse_bloom(out.cat.data(), out.cat.size(), out.bloom, err);
  }
  if (rc) err = "TableMeta decode: " + err;
  return rc;
}

void meta_frame(bool has_bloom, uint64_t m, const cb_zone_bounds* zone, MetaFrame& out) {
  // [0x0A len(bloom) [0x0A varint(m) m x 0/1]] [0x12 len(zone) [0x0A min] [0x12 max]]
  const uint64_t bl = has_bloom ? bloom_len(m) : 0;
  uint64_t zl = 0;
  out.total = 0;
  out.head_len = 0;
  out.zone.clear();
  if (has_bloom) {
    size_t h = 0;
    out.head[h++] = 0x0A;
    h += put_varint_buf(out.head + h, bl);
    if (m) h += put_bloom_header(out.head + h, m);
    out.head_len = h;
    out.total += 1 + varint_len(bl) + bl;
  }
  if (zone) {
    if (zone->has_min) zl += 1 + varint_len(zone->min_len) + zone->min_len;
    if (zone->has_max) zl += 1 + varint_len(zone->max_len) + zone->max_len;
    out.total += 1 + varint_len(zl) + zl;
    std::vector<uint8_t>& z = out.zone;
    z.reserve(zl + 11);
    uint8_t v[11];
    z.push_back(0x12);
    z.insert(z.end(), v, v + put_varint_buf(v, zl));
    if (zone->has_min) {
      z.push_back(0x0A);
      z.insert(z.end(), v, v + put_varint_buf(v, zone->min_len));
      z.insert(z.end(), zone->min, zone->min + zone->min_len);
    }
    if (zone->has_max) {
      z.push_back(0x12);
      z.insert(z.end(), v, v + put_varint_buf(v, zone->max_len));
      z.insert(z.end(), zone->max, zone->max + zone->max_len);
    }
  }
}

}  // namespace codec
}  // namespace cbx
