// tileplan.cpp — plan_build / plan_probe and the workspace sizes of their
// passes (tileplan.hpp). Host code only.
#include "tileplan.hpp"

#include "knobs.hpp"

namespace cb {

static uint32_t ilog2_floor(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }

static int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Raise tb (up to hi) until the tile count fits the partition histogram.
static uint32_t fit_tiles(uint64_t m, int64_t tb, int64_t hi) {
  while (tb < hi && ((m + (1ull << tb) - 1) >> tb) > kMaxTiles) ++tb;
  return (uint32_t)tb;
}

// Tuning overrides (knobs.hpp; the shipped library always takes the
// defaults): CB_PROBE_TB / CB_BUILD_TB fix the tile bits, CB_PROBE_KPT /
// CB_BUILD_KPT the partition keys per thread.

TilePlan plan_build(uint64_t m, uint64_t n, uint32_t nb) {
  // ~256 tiles per launch over the whole batch, each as large as the 64 KiB
  // LDS tile allows (fewer tiles = longer runs per partition block);
  // 1024-thread partition blocks of up to 4096 keys, fewer keys per thread
  // only while that leaves under 256 blocks in the launch.
  TilePlan p{};
  static const int env_tb = knob_int("CB_BUILD_TB", 0);
  static const int env_kpt = knob_int("CB_BUILD_KPT", 0);
  if (nb < 1) nb = 1;
  const uint64_t want_tiles = nb >= 256 ? 1 : 256 / nb;
  int64_t tb = clamp64((int64_t)ilog2_floor(m > want_tiles ? m / want_tiles : 1), kMinTileBits,
                       kMaxTileBits);
  if (env_tb) tb = clamp64(env_tb, kMinTileBits, kMaxTileBits);
  p.tb = fit_tiles(m, tb, kMaxTileBits);
  p.T = (uint32_t)((m + (1ull << p.tb) - 1) >> p.tb);
  p.kpt = kBuildMaxKpt;
  while (p.kpt > 1 && nb * ((n + kBuildNT * p.kpt - 1) / (kBuildNT * p.kpt)) < 256) p.kpt /= 2;
  if (env_kpt == 1 || env_kpt == 2 || env_kpt == 4) p.kpt = env_kpt;
  p.C = kBuildNT * p.kpt;
  p.nblk = (uint32_t)((n + p.C - 1) / p.C);
  // Batched builds of long runs (C4: 32 filters of 2^18 keys into 2^25 bits,
  // ~128 entries per run) move 16-bit entries in 2^16-bit sub-tiles: the
  // passes are bandwidth-bound there, and the entries are a third of the
  // bytes. Single builds keep 32-bit entries (their tile pass is bound by its
  // dependent loads, where the sub-tile arithmetic cost more than the bytes
  // saved: HISTORY.md, round 3 build notes).
  // Their tiles are 2^18 bits (4 sub-tiles) worked by 512-thread
  // workgroups, four per CU instead of two 1024-thread ones on 2^19-bit
  // tiles: C4 141 -> 128-131 us per step on one lane, 147-151 -> 139-141 on
  // three (profiles/c4_sub_r04.json).
  static const int env_sub = knob_int("CB_BUILD_SUB", -1);
  p.sub = 0;
  // (CB_BUILD_SUB=1, experiment builds: every build of tb >= 17 takes them)
  if (env_sub != 0 && p.tb >= 17 && ((nb >= 8 && long_runs(p.C, p.T)) || env_sub == 1)) {
    // (runs still long over twice the tiles: halve the tile)
    if (p.tb == 19 && !env_tb && (long_runs(p.C, 2ull * p.T) || env_sub == 1) && ((uint64_t)p.T << 3) <= kMaxTiles) {
      p.tb = 18;
      p.T = (uint32_t)((m + (1ull << 18) - 1) >> 18);
    }
    if (((uint64_t)p.T << (p.tb - 16)) <= kMaxTiles) p.sub = p.tb - 16;
  }
  return p;
}

TilePlan plan_probe(uint64_t m, uint64_t n) {
  TilePlan p{};
  // The probe kernel is instantiated for tiles of 2^16..2^18 bits. Aim for
  // ~512 tiles and <= ~4096 entries per tile.
  int64_t tb1 = (int64_t)ilog2_floor(m > 512 ? m / 512 : 1);
  const uint64_t want = n ? (m * 4096ull) / n : m;
  int64_t tb2 = (int64_t)ilog2_floor(want ? want : 1);
  int64_t tb = clamp64(tb1 < tb2 ? tb1 : tb2, kMinProbeTileBits, kMaxProbeTileBits);
  static const int env_tb = knob_int("CB_PROBE_TB", 0);
  if (env_tb) tb = clamp64(env_tb, kMinProbeTileBits, kMaxProbeTileBits);
  p.tb = fit_tiles(m, tb, kMaxProbeTileBits);
  p.T = (uint32_t)((m + (1ull << p.tb) - 1) >> p.tb);
  // Longer runs per (block, tile) with C = 2048 once that still leaves >= 512
  // partition blocks; never more than 4096 blocks (the host chunks keys).
  p.kpt = n >= 512ull * 2048 ? kProbeMaxKpt : 4;
  static const int env_kpt = knob_int("CB_PROBE_KPT", 0);
  if (env_kpt == 4 || env_kpt == 8) p.kpt = env_kpt;
  p.C = kPartThreads * p.kpt;
  p.nblk = (uint32_t)((n + p.C - 1) / p.C);
  return p;
}

bool plan_ok(const TilePlan& p) { return p.T <= kMaxTiles; }

size_t build_seg_bytes(const TilePlan& p) { return ((size_t)(p.T << p.sub) + 1) * p.nblk * 4; }
size_t build_ent_bytes(const TilePlan& p) { return (size_t)p.nblk * 2 * p.C * (p.sub ? 2 : 4); }
size_t probe_seg_bytes(const TilePlan& p) { return (size_t)(p.T + 1) * p.nblk * 4; }
size_t probe_ent_bytes(const TilePlan& p) { return (size_t)p.nblk * p.C * 8; }
size_t probe_lkey_bytes(const TilePlan& p) { return (size_t)p.nblk * p.C * 2; }

}  // namespace cb
