// tileplan.hpp — the host-only planner of the tiled passes: how a build or a
// probe over filters of m bits is cut into tiles and partition blocks, the
// workspace and LDS bytes each pass needs, and the limits the callers chunk
// by. Nothing here needs HIP: tileplan.cpp compiles alone and is tested on
// the CPU (tests/test_tileplan_cpu.py). The kernels that run the plans are in
// tilebuild.hip and tileprobe.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cb {

constexpr uint32_t kFiltersPerGroup = 32;   // one uint32 result mask per key
constexpr uint32_t kMaxTiles = 4096;        // LDS histogram bound in the partition pass
constexpr uint32_t kMaxTileBits = 19;       // build: 64 KiB LDS tiles at most
constexpr uint32_t kMaxBuildBlocks = 4096;  // partition blocks per launch, build and probe (the host chunks keys)
constexpr uint32_t kMinTileBits = 12;       // build: 512 B tiles at least
constexpr uint32_t kMinProbeTileBits = 16;  // probe kernel instantiations: 2^16..2^18
constexpr uint32_t kMaxProbeTileBits = 18;
// Filter allocations are padded to whole tiles of the largest tile size a pass
// may use, so no tiled pass reads or writes past the allocation.
constexpr uint64_t kTileAlignBits = 1ull << kMaxTileBits;
constexpr uint64_t kSmallAlignBits = 1ull << kMinProbeTileBits;

// Threads per block of the passes the plans size, and the most keys a thread
// of a partition block takes.
constexpr uint32_t kBuildNT = 1024;          // k_build_part, k_build_tile
constexpr uint32_t kPartThreads = 256;       // k_part_probe
constexpr uint32_t kTileProbeThreads = 512;  // k_tile_probe
constexpr uint32_t kBuildMaxKpt = 4;
constexpr uint32_t kProbeMaxKpt = 8;

// Geometry of one tiled pass (build or probe) over filters of m bits.
struct TilePlan {
  uint32_t tb;    // log2(tile bits)
  uint32_t T;     // number of tiles = ceil(m / 2^tb)
  uint32_t kpt;   // keys per thread in the partition pass
  uint32_t C;     // keys per partition block = threads * kpt
  uint32_t nblk;  // partition blocks = ceil(n / C)
  uint32_t sub;   // build only: 0, or log2 of the 2^16-bit sub-tiles per tile (16-bit entries)
};

// nb: filters built together in one launch pair (insert_fixed_many batches).
TilePlan plan_build(uint64_t m, uint64_t n, uint32_t nb = 1);
TilePlan plan_probe(uint64_t m, uint64_t n);
bool plan_ok(const TilePlan& p);  // tile count fits the partition histogram

// Workspace bytes a tiled pass needs.
size_t build_seg_bytes(const TilePlan& p);
size_t build_ent_bytes(const TilePlan& p);
size_t probe_seg_bytes(const TilePlan& p);
size_t probe_ent_bytes(const TilePlan& p);
size_t probe_lkey_bytes(const TilePlan& p);

// Long runs: a partition block of C keys leaves 2 C / T entries per tile on
// average (tiles of one filter); past ~3/4 of a wave the build's tile pass
// takes two rounds of run loads, and batched builds 16-bit entries.
constexpr bool long_runs(uint32_t C, uint64_t T) { return 2ull * C > 48ull * T; }

// Keys per chunk of a tiled pass: kMaxBuildBlocks partition blocks of the
// largest C the plan can return.
constexpr uint64_t build_chunk_keys() { return (uint64_t)kMaxBuildBlocks * kBuildNT * kBuildMaxKpt; }
constexpr uint64_t probe_chunk_keys() { return (uint64_t)kMaxBuildBlocks * kPartThreads * kProbeMaxKpt; }
static_assert(build_chunk_keys() == 1ull << 24 && probe_chunk_keys() == 1ull << 23, "chunk sizes");
// A probe entry packs (offset in the tile) | (key index in the block << tb)
// into 32 bits: log2 of the probe's largest C.
constexpr uint32_t kProbeLocalBits = 11;
static_assert((1u << kProbeLocalBits) == kPartThreads * kProbeMaxKpt, "block-local key index");

// Dynamic LDS of each tiled pass, in the order the kernel carves it up.
//
// A partition histogram over `bins` bins: bins + 1 counts (then run starts and
// the total), zero-padded to a multiple of 4 words.
constexpr uint32_t part_hist_words(uint32_t bins) { return (bins + 4) & ~3u; }
// k_build_part (part_phases): hist [part_hist_words(bins)], 4 words of which
// the first takes the discards, stage [2 C entries of 4 or 2 bytes].
constexpr size_t build_part_lds(const TilePlan& p) {
  return (size_t)(part_hist_words(p.T << p.sub) + 4) * 4 + (size_t)2 * p.C * (p.sub ? 2 : 4);
}
// k_build_tile, k_build_tile_sub: the tile [2^tb bits].
constexpr size_t build_tile_lds(const TilePlan& p) { return (size_t)(1u << (p.tb - 5)) * 4; }
// k_part_probe: hist [part_hist_words(T)], stage [C uint2], lstage [C
// uint16], wsum [8 words].
constexpr size_t probe_part_lds(const TilePlan& p) {
  return ((size_t)part_hist_words(p.T) + 2 * p.C + p.C / 2 + 8) * 4;
}
// k_tile_probe: buf [2 tiles], P and S [nblk padded to 4 words each], wsum
// [a word per wave], fw [kFiltersPerGroup pointers].
constexpr size_t probe_tile_lds(const TilePlan& p) {
  return ((size_t)2 * (1u << (p.tb - 5)) + 2 * ((p.nblk + 3) & ~3u) + kTileProbeThreads / 64) * 4 +
         kFiltersPerGroup * 8;
}

}  // namespace cb
