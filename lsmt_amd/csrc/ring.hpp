// ring.hpp — which node holds which row (host and device): the token of a
// byte string, the partition key of a stored key, the token ring and the
// replicas of a token.
//
// The reference places rows with a murmur3 token ring: Cluster::new
// (src/cluster.rs:46-54) inserts, for each node in order and each v in
// 0 .. max(vnodes, 1), the position (murmur3_32("{node}-{v}"), node) into a
// BTreeMap by token (a later insert replaces an earlier one of the same
// token), and replicas_for (src/cluster.rs:102-123) walks the positions with
// token >= t ascending, then the whole ring from its first position, and
// collects the nodes it has not collected yet until it holds rf of them. The
// keys it is asked about are the partition keys that SqlEngine::partition_keys
// cuts out of a statement (src/query.rs:448-528, 697-713, 734-760): the first
// npk key columns joined by the key's separator.
//
// This is the rule's one home in the library: the host entries (cb_ring_*),
// k_ring_route and k_ring_keep (ring.hip) ask here and nothing restates it.
//
// Token: MurmurHash3 x86_32 with seed 0 over the bytes, what
// murmur3_32(&mut Cursor, 0) of the murmur3 crate (0.5.2) computes. The
// crate's source was not available when this was written, so the hash below
// is a restatement of the published algorithm, pinned by the vectors of
// tests/test_ring_cpu.py, and NOT run against the reference itself. Bytes are
// unsigned; the tail's bytes enter the low end of the last block.
//
// Partition key of a stored key: rest = the key without its first
// min(skip, len) bytes (the namespace prefix, as rowjson.hpp's conditions take
// it off). With npk == 0, or when rest has at most npk parts, it is all of
// rest; otherwise rest up to, not including, its npk-th separator: the first
// npk parts joined again. Parts are rowjson.hpp's (key_part_count,
// key_part_at): a separator inside a column value is the key format's own
// ambiguity.
//
// Ring: nodes 0 .. nnodes - 1 in the caller's order (Cluster::new pushes the
// own node last); rf = max(rf, 1); the positions sorted by token. The replicas
// of t are an ordered list, the primary first, of width = min(rf, nodes that
// hold a position) entries for every t: lists are rf wide, -1 past width.
// What the device holds is the sorted tokens and, per position, its
// precomputed list: a key costs one hash, one search for the first position
// with token >= t (none: position 0) and one row read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "rowjson.hpp"

#if defined(__HIPCC__)
#define CB_RING_HD __host__ __device__
#else
#define CB_RING_HD
#endif

namespace cb {

constexpr uint32_t kRingMaxNodes = 4096;       // nodes of one ring
constexpr uint32_t kRingMaxVnodes = 4096;      // positions a node asks for
constexpr uint32_t kRingMaxRf = 16;            // replicas of one token
constexpr uint64_t kRingMaxPositions = 1ull << 20;
constexpr uint32_t kRingMaxPrefixes = 256;     // prefixes of one cb_key_rules
constexpr uint32_t kRingMaxPrefixBytes = 4096;

// ---- the token ----

// MurmurHash3 x86_32, seed 0, of n bytes handed out four at a time: next() is
// called ceil(n / 4) times and returns bytes 4i .. 4i + 3 of the input, the
// first in the low byte; what it returns past byte n - 1 is masked off here.
template <class Next>
CB_RING_HD inline uint32_t murmur3_32_blocks(uint64_t n, Next next) {
  constexpr uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
  auto rotl = [](uint32_t x, uint32_t r) { return x << r | x >> (32 - r); };
  uint32_t h = 0;
  for (uint64_t i = 0; i < n / 4; ++i) {
    uint32_t k = next();
    k *= c1;
    k = rotl(k, 15);
    k *= c2;
    h ^= k;
    h = rotl(h, 13);
    h = h * 5 + 0xe6546b64u;
  }
  const uint32_t tail = (uint32_t)(n & 3);
  if (tail) {
    uint32_t k = next() & ((1u << (8 * tail)) - 1);
    k *= c1;
    k = rotl(k, 15);
    k *= c2;
    h ^= k;
  }
  h ^= (uint32_t)n;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// The token of p[0..n) by byte loads: reads nothing outside the bytes.
CB_RING_HD inline uint32_t murmur3_32(const uint8_t* p, uint64_t n) {
  uint64_t at = 0;
  return murmur3_32_blocks(n, [&]() {
    uint32_t k = 0;
    for (uint32_t j = 0; j < 4 && at + j < n; ++j) k |= (uint32_t)p[at + j] << (8 * j);
    at += 4;
    return k;
  });
}

// ---- the partition key ----

// The length of the partition key of rest[0..n) (the key after its skipped
// bytes): it begins where rest does.
CB_RING_HD inline uint64_t partition_key_len(const uint8_t* rest, uint64_t n, uint32_t npk) {
  if (!npk || key_part_count(rest, n) <= npk) return n;
  uint64_t len = 0;
  const uint64_t a = key_part_at(rest, n, npk - 1, &len);
  return a + len;  // the npk-th separator stands here
}

// ---- the search ----

// The first position of tokens[0..npos) (ascending) with token >= t, in
// [lo, hi]; npos when there is none (the caller wraps to position 0).
CB_RING_HD inline uint32_t ring_first_ge(const uint32_t* tokens, uint32_t lo, uint32_t hi, uint32_t t) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tokens[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Whether `node` is among the first `ranks` entries of a replica list (ranks
// <= the list's width; entries past the width are -1 and never equal a node).
CB_RING_HD inline bool ring_row_holds(const int32_t* row, uint32_t ranks, uint32_t node) {
  for (uint32_t i = 0; i < ranks; ++i)
    if (row[i] == (int32_t)node) return true;
  return false;
}

// ---- the ring (host) ----

// A built ring: the positions ascending by token and, per position p, the
// replica list of every token whose first position is p (rows[p * rf ..], rf
// wide, -1 past width).
struct RingHost {
  uint32_t nnodes = 0, rf = 0, width = 0;
  std::vector<uint32_t> tokens, owners;
  std::vector<int32_t> rows;
};

// replicas_for's two loops (src/cluster.rs:106-121) from position p on: the
// positions p .. end, then the whole ring from its first position; out is rf
// wide, -1 past what was collected. Returns how many were collected.
inline uint32_t ring_walk(const RingHost& r, uint64_t p, int32_t* out) {
  const uint64_t npos = r.tokens.size();
  uint32_t got = 0;
  for (uint32_t i = 0; i < r.rf; ++i) out[i] = -1;
  auto take = [&](uint64_t q) {
    const int32_t node = (int32_t)r.owners[q];
    for (uint32_t i = 0; i < got; ++i)
      if (out[i] == node) return;
    out[got++] = node;
  };
  for (uint64_t q = p; q < npos && got < r.rf; ++q) take(q);
  for (uint64_t q = 0; q < npos && got < r.rf; ++q) take(q);
  return got;
}

// The position a token starts its walk at: the first with token >= t, or 0.
inline uint64_t ring_position(const RingHost& r, uint32_t t) {
  const uint32_t npos = (uint32_t)r.tokens.size();
  const uint32_t p = ring_first_ge(r.tokens.data(), 0, npos, t);
  return p == npos ? 0 : p;
}

// The ring of explicit (token, owner) pairs inserted in order, a later pair
// replacing an earlier one of the same token. Why it is refused, or nullptr.
inline const char* ring_build_tokens(const uint32_t* tokens, const uint32_t* owners, uint64_t npos, uint32_t nnodes,
                                     uint32_t rf, RingHost* out) {
  if (!nnodes || nnodes > kRingMaxNodes) return "a ring has 1 to 4096 nodes";
  if (rf > kRingMaxRf) return "rf is at most 16";
  if (!npos) return "a ring has at least one position";
  if (npos > kRingMaxPositions) return "too many positions (at most 2^20)";
  for (uint64_t i = 0; i < npos; ++i)
    if (owners[i] >= nnodes) return "a position's owner is not a node of the ring";
  std::map<uint32_t, uint32_t> ring;
  for (uint64_t i = 0; i < npos; ++i) ring[tokens[i]] = owners[i];  // BTreeMap::insert
  RingHost r;
  r.nnodes = nnodes;
  r.rf = rf ? rf : 1;
  for (const auto& kv : ring) {
    r.tokens.push_back(kv.first);
    r.owners.push_back(kv.second);
  }
  std::vector<uint8_t> holds(nnodes, 0);
  uint32_t holders = 0;
  for (uint32_t o : r.owners)
    if (!holds[o]) holds[o] = 1, ++holders;
  r.width = r.rf < holders ? r.rf : holders;
  // The lists, from the last position down: the walk from p is p's owner and
  // then the walk from p + 1 without that owner, so list(p) follows from
  // list(p + 1) in rf steps. The last position's own walk wraps to the first.
  const uint64_t n = r.tokens.size();
  r.rows.assign(n * r.rf, -1);
  (void)ring_walk(r, n - 1, &r.rows[(n - 1) * r.rf]);
  for (uint64_t p = n - 1; p-- > 0;) {
    int32_t* row = &r.rows[p * r.rf];
    const int32_t* nxt = &r.rows[(p + 1) * r.rf];
    uint32_t got = 0;
    row[got++] = (int32_t)r.owners[p];
    for (uint32_t i = 0; i < r.width && got < r.width; ++i)
      if (nxt[i] != row[0]) row[got++] = nxt[i];
  }
  *out = std::move(r);
  return nullptr;
}

// Cluster::new's ring (src/cluster.rs:46-54): node i's name is
// names[name_off[i] .. name_off[i + 1]). Why it is refused, or nullptr.
inline const char* ring_build_names(const uint8_t* names, const uint64_t* name_off, uint32_t nnodes, uint32_t vnodes,
                                    uint32_t rf, RingHost* out) {
  if (!nnodes || nnodes > kRingMaxNodes) return "a ring has 1 to 4096 nodes";
  if (vnodes > kRingMaxVnodes) return "vnodes is at most 4096";
  if (rf > kRingMaxRf) return "rf is at most 16";
  const uint32_t per = vnodes ? vnodes : 1;
  if ((uint64_t)nnodes * per > kRingMaxPositions) return "too many positions (at most 2^20)";
  for (uint32_t i = 0; i < nnodes; ++i) {
    if (name_off[i + 1] < name_off[i]) return "node name offsets decrease";
    if (name_off[i + 1] == name_off[i]) return "an empty node name";
  }
  std::map<std::vector<uint8_t>, uint32_t> seen;  // replicas_for compares names: the caller deduplicates
  for (uint32_t i = 0; i < nnodes; ++i)
    if (!seen.emplace(std::vector<uint8_t>(names + name_off[i], names + name_off[i + 1]), i).second)
      return "two nodes share a name";
  std::vector<uint32_t> tokens, owners;
  std::vector<uint8_t> key;
  for (uint32_t i = 0; i < nnodes; ++i)
    for (uint32_t v = 0; v < per; ++v) {
      key.assign(names + name_off[i], names + name_off[i + 1]);  // format!("{}-{}", node, v)
      key.push_back('-');
      char digits[12];
      int nd = 0;
      for (uint32_t x = v; nd == 0 || x; x /= 10) digits[nd++] = (char)('0' + x % 10);
      while (nd) key.push_back((uint8_t)digits[--nd]);
      tokens.push_back(murmur3_32(key.data(), key.size()));
      owners.push_back(i);
    }
  return ring_build_tokens(tokens.data(), owners.data(), tokens.size(), nnodes, rf, out);
}

// ---- what travels to the device ----

// A ring in device memory: the tokens, the rows and, for a ring too large for
// LDS, first[b] = the first position whose token's top `bits` bits are >= b
// (2^bits + 1 entries: the last is npos), so a token's search is one read of
// first[] and a walk inside its bucket.
struct RingView {
  const uint32_t* tokens;
  const int32_t* rows;
  const uint32_t* first;  // nullptr: search the tokens (the LDS path)
  uint32_t npos, rf, bits;
};

// A ring of up to this many positions is searched in LDS (k_ring_route keeps
// its tokens there: 8 KiB a block); a larger one through first[].
constexpr uint32_t kRingLdsPositions = 2048;
// The bits of first[] for a ring of npos positions: one bucket per position
// or more, so a bucket holds about one.
inline uint32_t ring_bucket_bits(uint64_t npos) {
  uint32_t bits = 1;
  while (bits < 20 && (1ull << bits) < npos) ++bits;
  return bits;
}

// The keys of a route: fixed-length rows, or (offsets != nullptr) a ragged
// batch of n + 1 offsets.
struct RouteKeys {
  const uint8_t* bytes;
  const uint64_t* offsets;
  uint32_t key_len;
};
// What is taken off a key before it is hashed: skip and npk for every key, or
// (roff != nullptr) per range of the keys: key k lies in the last range r of
// nr with roff[r] <= k, and rskip / rnpk (each nullable: zeros) hold its two.
struct RouteRule {
  uint32_t skip, npk;
  const uint64_t* roff;
  const uint32_t *rskip, *rnpk;
  uint32_t nr;
};

// The rules of a cb_key_rules, checked and packed: prefix r is bytes[at[r] ..
// at[r + 1]).
struct KeyRules {
  uint32_t np;
  uint32_t npk[kRingMaxPrefixes];
  uint16_t at[kRingMaxPrefixes + 1];
  uint8_t bytes[kRingMaxPrefixBytes];
};

// The rule a key is under: the last prefix that is <= the key bytewise is the
// only one the key can start with (the prefixes ascend and none starts with
// another). -1: under no prefix.
CB_RING_HD inline int32_t key_rule_of(const KeyRules& kr, const uint8_t* key, uint64_t klen) {
  uint32_t lo = 0, hi = kr.np;  // prefixes below lo are <= key, from hi on > key
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint8_t* p = kr.bytes + kr.at[mid];
    const uint64_t pl = (uint64_t)kr.at[mid + 1] - kr.at[mid], m = pl < klen ? pl : klen;
    uint64_t j = 0;
    while (j < m && p[j] == key[j]) ++j;
    const bool le = j == m ? pl <= klen : p[j] < key[j];
    if (le) lo = mid + 1;
    else hi = mid;
  }
  if (!lo) return -1;
  const uint8_t* p = kr.bytes + kr.at[lo - 1];
  const uint64_t pl = (uint64_t)kr.at[lo] - kr.at[lo - 1];
  if (pl > klen) return -1;
  for (uint64_t j = 0; j < pl; ++j)
    if (p[j] != key[j]) return -1;
  return (int32_t)(lo - 1);
}

// ---- ring.hip's launchers (a hipError_t as int, the stream as the C ABI
// passes it: this header names nothing of the runtime) ----

struct SortKey;
struct CompactSide;

// k_ring_route: tokens[k] (nullable) = the token of key k's partition key,
// replicas[k * rf ..] (nullable) = its replica list, for n keys.
int launch_ring_route(const RingView& rv, const RouteKeys& ks, const RouteRule& rule, uint64_t n, uint32_t* tokens,
                      int32_t* replicas, void* stream);
// k_ring_keep, behind a merge's select: slen[p] = 0 for every sorted record p
// of n that survives (slen[p] != 0), lies under a prefix of kr (device) and
// does not have `node` among the first `ranks` entries of its replica list.
// The tile sums are stale afterwards (compact.hpp launch_compact_tiles).
int launch_ring_keep(const RingView& rv, const KeyRules* kr, uint32_t node, uint32_t ranks, const SortKey* order,
                     const CompactSide* side, uint64_t n, uint64_t* slen, void* stream);

}  // namespace cb
