// ring_driver.cpp — prints what lsmt_amd/csrc/ring.hpp computes (the token,
// the partition key, the ring build, the replica lists and the rule a key is
// under: the rule behind cb_ring_*, cb_scan_route and cb_tables_compact_ring)
// without a device. Built by tests/test_ring_cpu.py under the address and
// undefined-behaviour sanitizers and run as a child process.
//
// stdin, one request per line (bytes travel as hex, "-" for none):
//   H HEX                      -> the token of the bytes
//   P SKIP NPK HEX             -> "start len" of the key's partition key
//   N VNODES RF HEX...         -> the ring of the named nodes becomes current:
//                                 "width npos token:owner ..." or "ERR why"
//   X NNODES RF TOKEN:OWNER... -> the same from explicit pairs
//   R TOKEN                    -> the current ring's replica list of the token,
//                                 "a,b,c": the precomputed row, which must
//                                 equal the walk of replicas_for's two loops
//   U HEX HEX:NPK...           -> the index of the rule the first HEX (a key) is
//                                 under, among the prefixes that follow; -1
// stdout: one line per request. Every byte string is copied into a heap block
// of exactly its size first, so a read past it is the sanitizer's.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "ring.hpp"

namespace {

std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[v.size() ? v.size() : 1]);
  if (!v.empty()) std::memcpy(b.get(), v.data(), v.size());
  return b;
}

int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

bool unhex(const std::string& s, std::vector<uint8_t>* out) {
  out->clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    const int h = hex(s[i]), l = hex(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((uint8_t)(h << 4 | l));
  }
  return true;
}

void print_ring(const char* why, const cb::RingHost& r) {
  if (why) {
    std::printf("ERR %s\n", why);
    return;
  }
  std::printf("%u %zu", r.width, r.tokens.size());
  for (size_t i = 0; i < r.tokens.size(); ++i) std::printf(" %u:%u", r.tokens[i], r.owners[i]);
  std::printf("\n");
}

}  // namespace

int main() {
  cb::RingHost ring;
  bool have = false;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, word;
    std::vector<uint8_t> bytes;
    in >> op;
    if (op == "H") {
      if (!(in >> word) || !unhex(word, &bytes)) return 2;
      const auto b = exact(bytes);
      std::printf("%u\n", cb::murmur3_32(b.get(), bytes.size()));
    } else if (op == "P") {
      uint32_t skip, npk;
      if (!(in >> skip >> npk >> word) || !unhex(word, &bytes)) return 2;
      const auto b = exact(bytes);
      const uint64_t len = bytes.size(), s = skip < len ? skip : len;
      std::printf("%" PRIu64 " %" PRIu64 "\n", s, cb::partition_key_len(b.get() + s, len - s, npk));
    } else if (op == "N") {
      uint32_t vnodes, rf;
      if (!(in >> vnodes >> rf)) return 2;
      std::vector<uint8_t> names;
      std::vector<uint64_t> off{0};
      while (in >> word) {
        if (!unhex(word, &bytes)) return 2;
        names.insert(names.end(), bytes.begin(), bytes.end());
        off.push_back(names.size());
      }
      const auto b = exact(names);
      cb::RingHost r;
      const char* why = cb::ring_build_names(b.get(), off.data(), (uint32_t)(off.size() - 1), vnodes, rf, &r);
      print_ring(why, r);
      if (!why) ring = std::move(r), have = true;
    } else if (op == "X") {
      uint32_t nnodes, rf;
      if (!(in >> nnodes >> rf)) return 2;
      std::vector<uint32_t> tokens, owners;
      while (in >> word) {
        uint32_t t, o;
        if (std::sscanf(word.c_str(), "%" SCNu32 ":%" SCNu32, &t, &o) != 2) return 2;
        tokens.push_back(t);
        owners.push_back(o);
      }
      // (exact-size blocks; an empty list keeps one unread word)
      std::unique_ptr<uint32_t[]> tb(new uint32_t[tokens.size() ? tokens.size() : 1]),
          ob(new uint32_t[tokens.size() ? tokens.size() : 1]);
      for (size_t i = 0; i < tokens.size(); ++i) tb[i] = tokens[i], ob[i] = owners[i];
      cb::RingHost r;
      const char* why = cb::ring_build_tokens(tb.get(), ob.get(), tokens.size(), nnodes, rf, &r);
      print_ring(why, r);
      if (!why) ring = std::move(r), have = true;
    } else if (op == "R") {
      uint32_t t;
      if (!have || !(in >> t)) return 2;
      const uint64_t p = cb::ring_position(ring, t);
      const int32_t* row = &ring.rows[p * ring.rf];
      std::vector<int32_t> walk(ring.rf);
      const uint32_t got = cb::ring_walk(ring, p, walk.data());
      if (got != ring.width) return 3;
      for (uint32_t i = 0; i < ring.rf; ++i)
        if (row[i] != walk[i]) return 3;
      if (!cb::ring_row_holds(row, ring.width, (uint32_t)row[0]) || cb::ring_row_holds(row, 0, (uint32_t)row[0]))
        return 3;
      for (uint32_t i = 0; i < ring.rf; ++i) std::printf("%s%d", i ? "," : "", row[i]);
      std::printf("\n");
    } else if (op == "U") {
      std::vector<uint8_t> key;
      if (!(in >> word) || !unhex(word, &key)) return 2;
      auto kr = std::make_unique<cb::KeyRules>();
      uint32_t at = 0;
      while (in >> word) {
        const size_t colon = word.find(':');
        if (colon == std::string::npos || !unhex(word.substr(0, colon), &bytes)) return 2;
        if (kr->np >= cb::kRingMaxPrefixes || at + bytes.size() > cb::kRingMaxPrefixBytes) return 2;
        kr->npk[kr->np] = (uint32_t)std::stoul(word.substr(colon + 1));
        kr->at[kr->np++] = (uint16_t)at;
        for (uint8_t c : bytes) kr->bytes[at++] = c;
      }
      for (uint32_t i = kr->np; i <= cb::kRingMaxPrefixes; ++i) kr->at[i] = (uint16_t)at;
      const auto b = exact(key);
      std::printf("%d\n", cb::key_rule_of(*kr, b.get(), key.size()));
    } else {
      return 2;
    }
  }
  return 0;
}
