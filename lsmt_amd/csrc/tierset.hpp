// tierset.hpp — tiered filter sets: one gate over FilterSets of different m.
//
// cb_tables_compact leaves a store with one or a few large tables behind
// large filters and a handful of fresh 1024-entry tables behind m = 1024
// filters, so the filters of one table list live in several FilterSets
// ("tiers"), one per filter size. Table t's Bloom filter and zone map are
// slot slots[t] of sets[tiers[t]]; its gate bit is that set's own gate for
// that slot (zone_map.contains && bloom.may_contain,
// /root/reference/src/sstable.rs:138). The key is hashed once for every tier
// (tiermask.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hash.hpp"
#include "zone.hpp"

namespace cb {

constexpr uint32_t kMaxTiers = 8;     // sets per launch
constexpr uint32_t kTierTables = 64;  // tables per launch (one candidate word per key)

// One tier as the kernels see it. A tier no table names (and the entries past
// ns) is a copy of a named tier with live = 0: its loads stay in bounds and
// the unnamed set's memory is never read.
struct TierDesc {
  const void* words;  // the set's words (uint32 / uint64 per position)
  ModP mp;
  ZoneView zv;    // gated: the zone-gated slots among `live` (0 in an ungated launch)
  uint64_t live;  // the slots this launch's tables name
  // Kept as operands, not as cases: a branch on a tier's kind between the
  // tiers' loads makes the compiler wait for each load before the next.
  uint64_t generic;  // all-ones: m is no power of two (positions by fastmod); 0: by mask
  uint32_t half;     // 1: a 32-slot set (two positions per 8-byte word); 0: 64 slots
  uint32_t pad;
};

// A launch's tiers and its table -> (tier, slot) mapping, passed by value.
struct TierArgs {
  TierDesc tier[kMaxTiers];
  uint64_t tgated;               // bit t: table t's slot is zone-gated in this launch
  uint32_t ns, nt;
  uint32_t all32;                // every named tier is MOD_POW2_32: the 32-bit hash state serves them all
  uint32_t pad;
  uint16_t tbl[kTierTables];     // table t: tier << 8 | slot
  uint16_t srt[kTierTables];     // the tables grouped by tier: table << 8 | slot
  uint8_t start[kMaxTiers + 8];  // tier i's tables are srt[start[i] .. start[i + 1])
  // table t's bound prefixes (lower, upper) in its tier's zone table; null: not gated
  const BoundPrefix* zpre[kTierTables];
};
static_assert(sizeof(TierArgs) <= 2048, "TierArgs travels as a kernel argument");

// hits[t][ceil(n/64)] for tables 0..ta.nt-1 (row t = table t, not slot
// order): the gate of cb_set_probe_gated_* (or, ungated, cb_set_probe_*) on
// table t's own tier and slot.
hipError_t launch_tier_probe(int keyk, const TierArgs& ta, const KeySrc& ks, uint64_t n, uint64_t* hits,
                             uint64_t hwords, hipStream_t s);

}  // namespace cb
