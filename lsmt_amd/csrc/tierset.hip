// tierset.hip — the gate of an ordered table list whose filters live in
// several FilterSets of different m (tierset.hpp), in one launch.
//
// After a compaction (cb_tables_compact) a store holds large tables behind
// large filters next to fresh m = 1024 ones, so Database::get's walk
// (/root/reference/src/lib.rs:128-134) crosses filter sizes. Per key and
// table the bit is SsTable::get's gate (src/sstable.rs:138) from that table's
// own tier; the key is hashed once for all tiers (tiermask.hpp).
#include <hip/hip_runtime.h>

#include "filterset.hpp"
#include "profile.hpp"
#include "setmask.hpp"
#include "tiermask.hpp"
#include "tierset.hpp"

namespace cb {
namespace {

constexpr uint32_t kTierProbeThreads = 64 * kSetWords;  // one 64-key hit word per wave

// k_set_probe's shape: one key per lane, one 64-key hit word per wave, 16
// waves per block. The per-key table masks are balloted into one hit word per
// table row, staged in LDS so every row leaves as a contiguous 128-byte
// segment.
template <int KEYK, bool ALL32, int NS>
__global__ __launch_bounds__(kTierProbeThreads) void k_tier_probe(TierArgs ta, KeySrc ks, uint64_t n,
                                                                  uint64_t* __restrict__ hits, uint64_t hwords) {
  __shared__ uint64_t hb[kTierTables][kSetWords];
  __shared__ BoundPrefix zp[2 * kTierTables];  // gated 16-byte keys: the tables' bound prefixes
  __shared__ uint16_t stbl[kTierTables], ssrt[kTierTables];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  stage_tier_lists(ta, stbl, ssrt);
  stage_tier_prefixes<KEYK>(ta, zp, kTierProbeThreads);  // issued alongside the key loads
  const uint64_t wbase = (uint64_t)blockIdx.x * kSetWords;
  const uint64_t k = (wbase + wave) * 64 + lane;
  const uint64_t mask = tier_key_mask<KEYK, ALL32, NS, true>(ta, stbl, ssrt, ks, k, k < n, zp);
  const uint64_t mine = slot_words<(int)kTierTables>(mask, ta.nt, lane);
  if (lane < ta.nt) hb[lane][wave] = mine;
  __syncthreads();
  const uint64_t nw = (n + 63) / 64;
  for (uint32_t i = threadIdx.x; i < ta.nt * kSetWords; i += kTierProbeThreads) {
    const uint32_t f = i / kSetWords, w = i % kSetWords;
    if (wbase + w < nw) hits[(uint64_t)f * hwords + wbase + w] = hb[f][w];
  }
}

template <int KK, bool AA, int NN>
void tier_probe(const TierArgs& ta, const KeySrc& ks, uint64_t n, uint64_t* hits, uint64_t hwords, uint32_t grid,
                hipStream_t s) {
  hipLaunchKernelGGL((k_tier_probe<KK, AA, NN>), dim3(grid), dim3(kTierProbeThreads), 0, s, ta, ks, n, hits, hwords);
}

}  // namespace

hipError_t launch_tier_probe(int keyk, const TierArgs& ta, const KeySrc& ks, uint64_t n, uint64_t* hits,
                             uint64_t hwords, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!ta.nt || ta.nt > kTierTables || !ta.ns || ta.ns > kMaxTiers) return hipErrorInvalidValue;
  const uint32_t grid = (uint32_t)set_probe_blocks(n);
  ProfScope ps(ta.tgated ? "k_tier_probe_gated" : "k_tier_probe", s);
  CB_TIER_DISPATCH(keyk, ta.all32, ta.ns, (tier_probe<KK, AA, NN>(ta, ks, n, hits, hwords, grid, s)));
  return hipGetLastError();
}

}  // namespace cb
