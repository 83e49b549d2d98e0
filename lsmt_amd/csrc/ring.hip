// ring.hip — the kernels of the token ring (ring.hpp): the batched
// replicas_for and the ownership filter of a compaction.
//
//   k_ring_route — one lane per key, a block over kRouteBlockKeys keys: the
//       partition key (a byte walk, only when npk != 0), its token, the first
//       position with token >= it and that position's replica row. The hash
//       eats 4-byte blocks, and a ragged key starts at any byte, so the key is
//       read as the ALIGNED dwords that contain it and each block is funnelled
//       out of two neighbours: one dword load per 4 bytes whatever the
//       alignment (byte loads would be four, and a dword load at an odd
//       address is not legal in every address space). A dword that holds a key
//       byte lies in that byte's page, so nothing unmapped is touched, and no
//       dword without a key byte is loaded. A ring of up to kRingLdsPositions
//       positions is copied into LDS once per block and searched there (the
//       block's keys pay for the copy: 2048 keys over at most 2048 tokens); a
//       larger one is searched in global memory behind first[], the table over
//       the token's top bits: one read gives the bucket, which holds about one
//       position, in place of 20 dependent steps through a megabyte.
//   k_ring_keep — behind the merge's select, one lane per sorted record: a
//       survivor that lies under a prefix of the rules and whose replica list
//       does not name the node within its first `ranks` entries gets slen 0.
//       It reads the key where the select read it (the input file), searches
//       global memory (one lane per record leaves nothing to share), and leaves
//       the tile sums to k_compact_lww_tiles (compact.hip).
#include <hip/hip_runtime.h>

#include "compact.hpp"
#include "launch.hpp"
#include "profile.hpp"
#include "ring.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;
constexpr uint32_t kRouteKeysPerLane = 8;
constexpr uint32_t kRouteBlockKeys = kNT * kRouteKeysPerLane;

// The token of p[0..n) from the aligned dwords that contain it.
__device__ __forceinline__ uint32_t token_of(const uint8_t* p, uint64_t n) {
  const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(p - mis);
  const uint64_t nd = n ? (mis + n + 3) / 4 : 0;  // the dwords that hold a key byte
  uint32_t lo = nd ? a[0] : 0;
  uint64_t j = 1;
  return murmur3_32_blocks(n, [&]() {
    const uint32_t hi = j < nd ? a[j] : 0;
    ++j;
    const uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * mis));
    lo = hi;
    return w;
  });
}

// The position a token's walk starts at, from global memory.
__device__ __forceinline__ uint32_t position_of(const RingView& rv, uint32_t t) {
  uint32_t lo = 0, hi = rv.npos;
  if (rv.first) {
    const uint32_t b = t >> (32 - rv.bits);
    lo = rv.first[b];
    hi = rv.first[b + 1];
  }
  const uint32_t p = ring_first_ge(rv.tokens, lo, hi, t);
  return p == rv.npos ? 0 : p;
}

template <bool Lds>
__global__ __launch_bounds__(kNT) void k_ring_route(RingView rv, RouteKeys ks, RouteRule rule, uint64_t n,
                                                    uint32_t* __restrict__ tokens, int32_t* __restrict__ replicas) {
  __shared__ uint32_t s_tok[Lds ? kRingLdsPositions : 1];
  if (Lds) {
    for (uint32_t i = threadIdx.x; i < rv.npos; i += kNT) s_tok[i] = rv.tokens[i];
    __syncthreads();
  }
  const uint64_t k0 = (uint64_t)blockIdx.x * kRouteBlockKeys;
  for (uint32_t it = 0; it < kRouteKeysPerLane; ++it) {
    const uint64_t k = k0 + (uint64_t)it * kNT + threadIdx.x;
    if (k >= n) break;
    const uint64_t at = ks.offsets ? ks.offsets[k] : k * ks.key_len;
    const uint64_t len = ks.offsets ? ks.offsets[k + 1] - at : ks.key_len;
    uint32_t skip = rule.skip, npk = rule.npk;
    if (rule.roff) {
      const uint32_t r = last_le(rule.nr, k, [&](uint32_t i) { return rule.roff[i]; });
      skip = rule.rskip ? rule.rskip[r] : 0;
      npk = rule.rnpk ? rule.rnpk[r] : 0;
    }
    const uint64_t s = skip < len ? skip : len;
    const uint8_t* rest = ks.bytes + at + s;
    const uint32_t t = token_of(rest, partition_key_len(rest, len - s, npk));
    if (tokens) tokens[k] = t;
    if (replicas) {
      uint32_t p;
      if (Lds) {
        p = ring_first_ge(s_tok, 0, rv.npos, t);
        if (p == rv.npos) p = 0;
      } else {
        p = position_of(rv, t);
      }
      const int32_t* row = rv.rows + (uint64_t)p * rv.rf;
      int32_t* out = replicas + k * rv.rf;
      for (uint32_t i = 0; i < rv.rf; ++i) out[i] = row[i];
    }
  }
}

__global__ __launch_bounds__(kNT) void k_ring_keep(RingView rv, const KeyRules* __restrict__ kr, uint32_t node,
                                                   uint32_t ranks, const SortKey* __restrict__ order,
                                                   const CompactSide* __restrict__ side, uint64_t n,
                                                   uint64_t* __restrict__ slen) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (p >= n || !slen[p]) return;
  const CompactSide sd = side[order[p].idx];
  const int32_t r = key_rule_of(*kr, sd.src, sd.klen);
  if (r < 0) return;  // under no prefix: every node's
  const uint32_t skip = (uint32_t)kr->at[r + 1] - kr->at[r];  // (the key starts with the prefix: skip <= klen)
  const uint8_t* rest = sd.src + skip;
  const uint32_t t = token_of(rest, partition_key_len(rest, sd.klen - skip, kr->npk[r]));
  const int32_t* row = rv.rows + (uint64_t)position_of(rv, t) * rv.rf;
  if (!ring_row_holds(row, ranks, node)) slen[p] = 0;
}

}  // namespace

int launch_ring_route(const RingView& rv, const RouteKeys& ks, const RouteRule& rule, uint64_t n, uint32_t* tokens,
                      int32_t* replicas, void* stream) {
  if (!n) return (int)hipSuccess;
  if (!rv.first && rv.npos > kRingLdsPositions) return (int)hipErrorInvalidValue;  // (the LDS copy's bound)
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("k_ring_route", s);
  const auto k = rv.first ? k_ring_route<false> : k_ring_route<true>;
  hipLaunchKernelGGL(k, dim3(blocks_for(n, kRouteBlockKeys)), dim3(kNT), 0, s, rv, ks, rule, n, tokens, replicas);
  return (int)hipGetLastError();
}

int launch_ring_keep(const RingView& rv, const KeyRules* kr, uint32_t node, uint32_t ranks, const SortKey* order,
                     const CompactSide* side, uint64_t n, uint64_t* slen, void* stream) {
  if (!n) return (int)hipSuccess;
  if (ranks > rv.rf) return (int)hipErrorInvalidValue;  // (a row is rf wide)
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("k_ring_keep", s);
  hipLaunchKernelGGL(k_ring_keep, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, rv, kr, node, ranks, order, side, n,
                     slen);
  return (int)hipGetLastError();
}

}  // namespace cb
