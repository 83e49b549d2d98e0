// tiermask.hpp — one key's gate over tiered filter sets (device code shared
// by the tier probe, tierset.hip, and the fused read path, getmany.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hash.hpp"
#include "tierset.hpp"
#include "zone.hpp"

namespace cb {

// Position h % m in one tier from the shared hash state. ALL32: h is the
// 32-bit state, exact for every m = 2^k <= 2^32 (hash.hpp). Otherwise h is the
// u64 state: its low bits are exact for a power-of-two m of any size
// (mp.mask), and any other m takes the tier's fastmod (mp.mask = 0 there);
// the two are blended by d.generic, with no branch on the tier's kind.
template <bool ALL32>
__device__ __forceinline__ uint64_t tier_pos(uint64_t h, const TierDesc& d) {
  if constexpr (ALL32)
    return (uint32_t)h & (uint32_t)d.mp.mask;
  else
    return (h & d.mp.mask) | (fastmod(h, d.mp) & d.generic);
}

// The aligned 8 bytes that hold word p of a tier, and word p out of them
// among the slots in `keep` (at most the set's width). One load for either
// width and no branch on it: a 32-slot set reads the pair of words that holds
// word p (the set's words are allocated in multiples of 32) and shifts its
// half down. Load and pick are apart so that every tier's load can issue
// before the first pick waits for one.
__device__ __forceinline__ uint64_t tier_load(const TierDesc& d, uint64_t p) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) u32x2* gptr;
  const u32x2 v = *(gptr)((const uint8_t*)d.words + ((p >> d.half) << 3));
  return (uint64_t)v.y << 32 | v.x;
}
__device__ __forceinline__ uint64_t tier_pick(const TierDesc& d, uint64_t raw, uint64_t p, uint64_t keep) {
  return (raw >> (((uint32_t)p & d.half) << 5)) & keep;
}

// One key's answer for every table of a tiered launch: bit t of the result =
// table t's gate, i.e. what set_key_mask reports for slot (tbl[t] & 63) of
// tier (tbl[t] >> 8). The key is hashed once: the 32-bit state (dot4 fold for
// 16-byte keys) when every tier is MOD_POW2_32, else the 64-bit state, and
// each tier takes its positions from that state (tier_pos), so the key bytes
// are walked once however many tiers there are.
//
// Every tier's set[a] load is issued before any is consumed; a tier's set[b]
// is read only where its a word has a bit among the slots this launch names
// (the reference's `&&`, src/bloom.rs:50). Slot bits become table bits through
// the tables grouped by tier (ssrt, LDS). The zone gate (src/sstable.rs:138)
// runs only for candidates that survive the Bloom test: 16-byte keys against
// the bounds' prefixes staged per table (zp[2t], zp[2t+1]; stage_tier_prefixes),
// other keys against the tier's own table (zone_contains).
// NS: the tiers walked (ta.ns <= NS; the entries past ns are copies with no
// live slot). SYNC: the block barrier that publishes stbl, ssrt and zp is taken
// here, after the key's loads have issued (every thread calls this once).
template <int KEYK, bool ALL32, int NS, bool SYNC>
__device__ __forceinline__ uint64_t tier_key_mask(const TierArgs& ta, const uint16_t* stbl, const uint16_t* ssrt,
                                                  const KeySrc& ks, uint64_t k, bool ok, const BoundPrefix* zp) {
  constexpr int HM = ALL32 ? MOD_POW2_32 : MOD_POW2_64;
  const ModP whole{0, ~0ull, 0};  // the state itself: h & ~0
  uint64_t h1 = 0, h2 = 0;        // (a key past the batch probes position 0 and is masked off)
  uint4 kv = make_uint4(0, 0, 0, 0);
  if (ok) {
    if constexpr (KEYK == KEY_FIXED16) {
      kv = reinterpret_cast<const uint4*>(ks.bytes)[k];
      key_positions_u4<HM>(kv, whole, h1, h2);
    } else {
      key_positions<KEYK, HM>(ks, k, whole, h1, h2);
    }
  }
  uint64_t va[NS], vb[NS];
  uint32_t lo[NS];  // a position's low bits (its half of a 32-slot pair)
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const uint64_t pa = tier_pos<ALL32>(h1, ta.tier[i]);
    lo[i] = (uint32_t)pa;
    va[i] = tier_load(ta.tier[i], pa);
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    va[i] = tier_pick(ta.tier[i], va[i], lo[i], ok ? ta.tier[i].live : 0ull);
    const uint64_t pb = tier_pos<ALL32>(h2, ta.tier[i]);
    lo[i] = (uint32_t)pb;
    vb[i] = va[i] ? tier_load(ta.tier[i], pb) : 0ull;  // only the load is conditional
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) vb[i] = tier_pick(ta.tier[i], vb[i], lo[i], ta.tier[i].live);
  if constexpr (SYNC) __syncthreads();
  uint64_t mask = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const uint64_t m = va[i] & vb[i];
    if (m) {
      const uint32_t j1 = ta.start[i + 1];
      for (uint32_t j = ta.start[i]; j < j1; ++j) {
        const uint32_t e = ssrt[j];
        mask |= ((m >> (e & 63u)) & 1ull) << (e >> 8);
      }
    }
  }
  uint64_t c = mask & ta.tgated;
  if (c) {
    if constexpr (KEYK == KEY_FIXED16) {
      const uint32_t kw[4] = {be32(kv.x), be32(kv.y), be32(kv.z), be32(kv.w)};
      while (c) {
        const uint32_t t = (uint32_t)__builtin_ctzll(c);
        c &= c - 1;
        if (cmp16(kw, zp[2 * t]) < 0 || cmp16(kw, zp[2 * t + 1]) > 0) mask &= ~(1ull << t);
      }
    } else {
      const uint8_t* kp;
      uint64_t kl;
      key_span<KEYK>(ks, k, kp, kl);
      while (c) {
        const uint32_t t = (uint32_t)__builtin_ctzll(c);
        c &= c - 1;
        const uint32_t e = stbl[t];
        if (!zone_contains(ta.tier[e >> 8].zv, e & 63u, kp, kl)) mask &= ~(1ull << t);
      }
    }
  }
  return mask;
}

// The launch's table lists into LDS (tier_key_mask's stbl and ssrt).
__device__ __forceinline__ void stage_tier_lists(const TierArgs& ta, uint16_t* stbl, uint16_t* ssrt) {
  if (threadIdx.x < ta.nt) {
    stbl[threadIdx.x] = ta.tbl[threadIdx.x];
    ssrt[threadIdx.x] = ta.srt[threadIdx.x];
  }
}

// The gated tables' bound prefixes into LDS (16-byte keys; tier_key_mask's
// zp): table t's pair from its tier's live zone table (ta.zpre[t], resolved
// on the host so a lane's bytes are its pointer and one load away), 2 x nt
// BoundPrefix (at most 4 KiB) where staging every slot of every tier would
// take 32 KiB. Gathered per block from device memory, never cached on the
// host: cb_set_zone rewrites the table.
template <int KEYK>
__device__ __forceinline__ void stage_tier_prefixes(const TierArgs& ta, BoundPrefix* zp, uint32_t nthreads) {
  if constexpr (KEYK == KEY_FIXED16) {
    if (ta.tgated) {  // uniform
      typedef const __attribute__((address_space(1))) uint32_t* gptr;
      constexpr uint32_t kPairDw = 2 * sizeof(BoundPrefix) / 4;
      uint32_t* dst = reinterpret_cast<uint32_t*>(zp);
      for (uint32_t i = threadIdx.x; i < ta.nt * kPairDw; i += nthreads) {
        const BoundPrefix* p = ta.zpre[i / kPairDw];
        if (p) dst[i] = ((gptr)p)[i % kPairDw];
      }
    }
  }
}

// Every (key kind, hash state, tier count) instantiation, by runtime values.
#define CB_TIER_DISPATCH(keyk, all32, ns, CALL)                                                \
  switch (((keyk) * 2 + ((all32) ? 1 : 0)) * 2 + ((ns) > 2)) {                                \
    case 0: { constexpr int KK = KEY_FIXED16, NN = 2; constexpr bool AA = false; CALL; } break; \
    case 1: { constexpr int KK = KEY_FIXED16, NN = 8; constexpr bool AA = false; CALL; } break; \
    case 2: { constexpr int KK = KEY_FIXED16, NN = 2; constexpr bool AA = true; CALL; } break;  \
    case 3: { constexpr int KK = KEY_FIXED16, NN = 8; constexpr bool AA = true; CALL; } break;  \
    case 4: { constexpr int KK = KEY_FIXED, NN = 2; constexpr bool AA = false; CALL; } break;   \
    case 5: { constexpr int KK = KEY_FIXED, NN = 8; constexpr bool AA = false; CALL; } break;   \
    case 6: { constexpr int KK = KEY_FIXED, NN = 2; constexpr bool AA = true; CALL; } break;    \
    case 7: { constexpr int KK = KEY_FIXED, NN = 8; constexpr bool AA = true; CALL; } break;    \
    case 8: { constexpr int KK = KEY_VAR, NN = 2; constexpr bool AA = false; CALL; } break;     \
    case 9: { constexpr int KK = KEY_VAR, NN = 8; constexpr bool AA = false; CALL; } break;     \
    case 10: { constexpr int KK = KEY_VAR, NN = 2; constexpr bool AA = true; CALL; } break;     \
    case 11: { constexpr int KK = KEY_VAR, NN = 8; constexpr bool AA = true; CALL; } break;     \
    default: return hipErrorInvalidValue;                                                     \
  }

}  // namespace cb
