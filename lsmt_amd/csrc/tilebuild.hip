// tilebuild.hip — the tiled build of one filter, or of a batch of filters of
// one size, in two passes (the plan: tileplan.hpp
// plan_build).
//
// Reference semantics: /root/reference/src/bloom.rs:26-44 (hashes / insert).
// Filter layout in HBM: packed uint32 words, bit p at word p>>5, bit p&31
// (LSB-first).
//
// Partition layout: partition block b (C keys) writes its entries sorted by
// tile into ent[b*estride ...] and, in seg[b*(T+1) + t], the start of tile
// t's run inside that region (seg[b*(T+1) + T] = the block's total). Tile t's
// entries are therefore the runs [seg[b][t], seg[b][t+1]) of every block b.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "devutil.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "launch.hpp"
#include "profile.hpp"

// Phase stamps for diagnostics (tools/ubench_build.hip defines CB_STAMPS and
// provides g_stamps): wall-clock s_memrealtime at phase boundaries, one row of
// 8 per workgroup. Compiled out of the library.
#ifdef CB_STAMPS
__device__ uint64_t* g_stamps;
#define CB_STAMP(i)                                                                   \
  do {                                                                                \
    if (threadIdx.x == 0 && g_stamps)                                                 \
      g_stamps[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] =             \
          __builtin_amdgcn_s_memrealtime();                                           \
  } while (0)
#else
#define CB_STAMP(i) \
  do {              \
  } while (0)
#endif

namespace cb {
namespace {

// Two passes. Every key contributes two entries (bit a, bit b), bucketed by
// the filter tile they fall in; then one workgroup per tile ORs its entries
// into the tile in LDS and writes the tile back once. At C2 size a pass over
// 16 MiB is ~3 us of bandwidth, so the dependent steps, not the bytes, set the
// time (tools/ubench_build.hip stamps the phases):
//   k_build_part — 1024-thread blocks of KPT keys per thread (C = 1024*KPT).
//                  All key loads issue before any LDS work; ranks from LDS
//                  atomics; the block's entries leave tile-sorted as one
//                  contiguous region, its run starts as one row of seg.
//   k_build_tile — one 1024-thread workgroup per tile of up to 2^19 bits
//                  (64 KiB of LDS). Wave w reads whole runs (lane i = entry i
//                  of the run, one coalesced load per run), 8 runs in flight
//                  per wave, so the 128-B lines of a run are fetched by one
//                  instruction instead of by 64 lanes' scattered loads.
// Fewer, larger tiles (~256 for C2) and larger blocks make the average run
// ~32 entries = one 128-B line.
//
// Store cache policy of the build's two outputs: bit 0 write-through
// partition entries, bit 1 non-temporal tile write-back.
constexpr uint32_t kBuildStores = CB_BUILD_STORES;

// A 16-byte key's two positions packed as partition entries ((bin << 20) |
// offset in the bin, bins of 2^tb bits), 0xFFFFFFFF for both when !live.
// 32-bit arithmetic where the positions are (MOD_POW2_32).
template <int MODE>
__device__ __forceinline__ void pack_positions(const uint4& kv, bool live, const ModP& mp, uint32_t tb, uint32_t& qa,
                                               uint32_t& qb) {
  const uint32_t tmask = (1u << tb) - 1u;
  uint32_t a32, b32, ah, bh;
  if constexpr (MODE == MOD_POW2_32) {
    uint32_t h1, h2;
    hash16_u32(kv, h1, h2);
    const uint32_t mask = static_cast<uint32_t>(mp.mask);
    a32 = h1 & mask;
    b32 = h2 & mask;
    ah = a32 >> tb;
    bh = b32 >> tb;
  } else {
    uint64_t a, b;
    key_positions_u4<MODE>(kv, mp, a, b);
    a32 = (uint32_t)a;
    b32 = (uint32_t)b;
    ah = (uint32_t)(a >> tb);
    bh = (uint32_t)(b >> tb);
  }
  qa = live ? (ah << 20) | (a32 & tmask) : 0xFFFFFFFFu;
  qb = live ? (bh << 20) | (b32 & tmask) : 0xFFFFFFFFu;
}

// A partition block's LDS phases once its entries are in registers (q: packed
// (bin << 20) | offset, 0xFFFFFFFF for none): ranks from LDS atomics, the bin
// scan, the seg row (run starts and the total), the tile-sorted entries into
// LDS and out to `out` as one contiguous region. Barriers inside; the block's
// LDS is free again when it returns except for the final store's reads of
// `stage` (the caller's next LDS write must follow a barrier).
template <int KPT, typename E>
__device__ __forceinline__ void part_phases(const uint32_t (&q)[2 * KPT], uint32_t T, uint32_t* smem,
                                            uint32_t* __restrict__ srow, E* __restrict__ out) {
  constexpr uint32_t NT = kBuildNT, C = NT * KPT;
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  const uint32_t Tp = part_hist_words(T);  // the layout and its bytes: build_part_lds (tileplan.hpp)
  // hist: T + 1 entries (counts, then run starts and the total), zero to Tp,
  // then a discard word at Tp for the lanes without an entry
  uint32_t* hist = smem;
  E* stage = reinterpret_cast<E*>(smem + Tp + 4);
  const uint32_t tid = threadIdx.x;
  uint32_t er[2 * KPT];
  for (uint32_t i = tid; i < Tp; i += NT) hist[i] = 0;
  __syncthreads();
  CB_STAMP(1);
  // every lane adds (no branch per entry, whose merges cost more VALU than
  // the rare discards on the last block's padding)
#pragma unroll
  for (int e = 0; e < 2 * KPT; ++e) er[e] = atomicAdd(&hist[q[e] != kNone ? q[e] >> 20 : Tp], 1u);
  __syncthreads();
  CB_STAMP(2);
  wave0_exclusive_scan4(hist, Tp);  // Tp >= T + 1: hist[T] = the total
  __syncthreads();
  CB_STAMP(3);
  const uint32_t total = hist[T];
  for (uint32_t t = tid; t <= T; t += NT) srow[t] = hist[t];
#pragma unroll
  for (int e = 0; e < 2 * KPT; ++e)
    if (q[e] != kNone) stage[hist[q[e] >> 20] + er[e]] = (E)(q[e] & 0xFFFFFu);
  __syncthreads();
  CB_STAMP(4);
  constexpr uint32_t PER = 16 / sizeof(E);  // entries per 16-B store (out and stage 16-B aligned)
  const uint32_t n4 = total / PER;
  // write-through (sc1): the entries go on to the memory side at once, so the
  // kernel's end has no dirty L2 lines to write back, and the tile pass (on
  // other XCDs) still finds them there; C2 on four lanes 101 -> 105-107 G
  // keys/s (non-temporal stores instead made the tile pass's reads slower)
  if constexpr (kBuildStores & 1u) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(out, 0, 2 * C * sizeof(E), 0x00020000);
    for (uint32_t i = tid; i < n4; i += NT) store16_wt(r, i * 16, reinterpret_cast<const uint4*>(stage)[i]);
  } else {
    for (uint32_t i = tid; i < n4; i += NT)
      reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(stage)[i];
  }
  if (tid < total - PER * n4) out[PER * n4 + tid] = stage[PER * n4 + tid];  // the < PER left over
  CB_STAMP(5);
}

// E: the entry type — uint32_t (offsets in tiles of up to 2^20 bits) or
// uint16_t (bins of 2^16 bits, tb = 16 here: the sub-tiles of
// k_build_tile_sub's tiles).
template <int KEYK, int MODE, int KPT, typename E = uint32_t>
__global__ __launch_bounds__(kBuildNT) void k_build_part(BuildBatch bb, ModP mp, uint32_t tb,
                                                         uint32_t T,
                                                         uint32_t* __restrict__ seg_all,
                                                         void* __restrict__ ent_all) {
  constexpr uint32_t NT = kBuildNT, C = NT * KPT;
  static_assert(sizeof(E) == 4 || sizeof(E) == 2, "entry type");
  const KeySrc ks = bb.ks[blockIdx.y];
  const uint64_t n = bb.n[blockIdx.y];
  uint32_t* seg = seg_all + (size_t)blockIdx.y * gridDim.x * (T + 1);
  E* ent = reinterpret_cast<E*>(ent_all) + (size_t)blockIdx.y * gridDim.x * (2 * C);
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t tid = threadIdx.x;
  const uint64_t kbase = (uint64_t)blockIdx.x * C;
  CB_STAMP(0);

  // positions first: every key load of the thread is in flight together.
  // Each entry is kept packed as (tile << 20) | offset in the tile (tiles <
  // kMaxTiles = 2^12, offsets < 2^kMaxTileBits <= 2^20), 0xFFFFFFFF for none:
  // one register per entry instead of a 64-bit position and a tile.
  static_assert(kMaxTiles <= 4096 && kMaxTileBits <= 20, "packed entry");
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  uint32_t q[2 * KPT];
  if constexpr (KEYK == KEY_FIXED16) {
    // every lane loads all its keys first (indices clamped to the last key,
    // so no per-key branch serialises the loads behind each other's waits)
    uint4 kv[KPT] = {};  // (a block past this filter's keys hashes zeros, all discarded)
    if (kbase < n) {  // uniform
      const uint4* keys = reinterpret_cast<const uint4*>(ks.bytes);
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const uint64_t k = kbase + (uint64_t)j * NT + tid;
        kv[j] = keys[k < n ? k : n - 1];
      }
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const uint64_t k = kbase + (uint64_t)j * NT + tid;
      pack_positions<MODE>(kv[j], k < n, mp, tb, q[2 * j], q[2 * j + 1]);
    }
  } else {
    const uint32_t tmask = (1u << tb) - 1u;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const uint64_t k = kbase + (uint64_t)j * NT + tid;
      q[2 * j] = q[2 * j + 1] = kNone;
      if (k < n) {
        uint64_t a, b;
        key_positions<KEYK, MODE>(ks, k, mp, a, b);
        q[2 * j] = ((uint32_t)(a >> tb) << 20) | ((uint32_t)a & tmask);
        q[2 * j + 1] = ((uint32_t)(b >> tb) << 20) | ((uint32_t)b & tmask);
      }
    }
  }
  part_phases<KPT, E>(q, T, smem, seg + (size_t)blockIdx.x * (T + 1), ent + (size_t)blockIdx.x * (2 * C));
}

// The two tile kernels' shared ends (LDS: build_tile_lds, tileplan.hpp; the
// tile alone). Prologue: the tile of tw words zeroed (a fresh filter) or loaded
// into LDS, called with the first group's run bounds already in flight; the
// barrier that publishes it is inside.
template <uint32_t NT>
__device__ __forceinline__ void tile_to_lds(uint4* lt, const uint4* gt, uint32_t tw, bool fresh) {
  for (uint32_t i = threadIdx.x; i < tw / 4; i += NT) lt[i] = fresh ? make_uint4(0, 0, 0, 0) : gt[i];
  __syncthreads();
}

// Epilogue: the tile written back (after the caller's barrier). Non-temporal:
// the filter is written once and read by other launches, so no L2 lines to
// write back at the kernel's end (tile pass alone 8.8 -> 7.5 us, C2 on four
// lanes 97.8 -> 101 G keys/s; write-through measured the same here).
template <uint32_t NT>
__device__ __forceinline__ void tile_from_lds(uint4* gt, const uint4* lt, uint32_t tw) {
  if constexpr (kBuildStores & 2u)
    for (uint32_t i = threadIdx.x; i < tw / 4; i += NT) store16_nt(gt + i, lt[i]);
  else
    for (uint32_t i = threadIdx.x; i < tw / 4; i += NT) gt[i] = lt[i];
}

// Wave w owns partition blocks b = w + NW*u. Per group of 16: lanes 0..15
// load the 16 blocks' run bounds (seg[b][t], seg[b][t+1]), shuffles hand each
// run's start and length to the whole wave, and the wave issues the 16 run
// loads back to back (lane i = entry i): two dependent memory round trips per
// group and no LDS run table or barrier before the ORs.
template <int G, int R>
__global__ __launch_bounds__(kBuildNT) void k_build_tile(BuildBatch bb, uint32_t tb, uint32_t T,
                                                         const uint32_t* __restrict__ seg_all,
                                                         uint32_t nblk,
                                                         const uint32_t* __restrict__ ent_all,
                                                         uint32_t estride) {
  constexpr uint32_t NT = kBuildNT, NW = NT / 64;
  static_assert(G <= 64, "one lane per run bound");
  uint32_t* __restrict__ words = bb.words[blockIdx.y];
  const bool fresh = (bb.fresh >> blockIdx.y) & 1ull;
  const uint32_t* __restrict__ seg = seg_all + (size_t)blockIdx.y * nblk * (T + 1);
  const uint32_t* __restrict__ ent = ent_all + (size_t)blockIdx.y * nblk * estride;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t tw = 1u << (tb - 5);
  uint32_t* tile = smem;
  const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const uint32_t t = xcd_order(blockIdx.x, T);
  CB_STAMP(0);

  // first group's run bounds in flight while the tile is cleared / loaded
  uint32_t s0 = 0, s1 = 0;
  {
    const uint32_t b = w + NW * lane;
    if (lane < (uint32_t)G && b < nblk) {
      const uint32_t* row = seg + (size_t)b * (T + 1) + t;
      s0 = row[0];
      s1 = row[1];
    }
  }
  uint4* gt = reinterpret_cast<uint4*>(words + (size_t)t * tw);
  uint4* lt = reinterpret_cast<uint4*>(tile);
  tile_to_lds<NT>(lt, gt, tw, fresh);
  CB_STAMP(1);

  for (uint32_t g0 = 0; w + NW * g0 < nblk; g0 += G) {
    if (g0) {
      s0 = s1 = 0;
      const uint32_t b = w + NW * (g0 + lane);
      if (lane < (uint32_t)G && b < nblk) {
        const uint32_t* row = seg + (size_t)b * (T + 1) + t;
        s0 = row[0];
        s1 = row[1];
      }
    }
    // R rounds of run loads (lane i = entry i + 64 r): every load of the G
    // runs goes out before any OR. R = 2 for long runs (C4's 64 tiles per
    // filter give ~128 entries per run) with G = 8, so a lane holds G * R =
    // 16 entries either way (62 VGPRs, 8 waves per SIMD: two 16-wave tiles per
    // CU; 32 entries per lane took 80 VGPRs and one tile per CU)
    uint32_t o[R][G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const uint32_t st = __shfl(s0, u, 64), len = __shfl(s1, u, 64) - st;
      const uint32_t b = w + NW * (g0 + u);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        o[q][u] = 0xFFFFFFFFu;
        if (64 * q + lane < len) o[q][u] = ent[(size_t)b * estride + st + 64 * q + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int q = 0; q < R; ++q)
        if (o[q][u] != 0xFFFFFFFFu) atomicOr(&tile[o[q][u] >> 5], 1u << (o[q][u] & 31));
    // runs longer than R waves (skewed inputs, few partition blocks)
    if (__ballot(lane < (uint32_t)G && s1 - s0 > 64u * R)) {
#pragma unroll 1
      for (int u = 0; u < G; ++u) {
        const uint32_t st = __shfl(s0, u, 64), len = __shfl(s1, u, 64) - st;
        const uint32_t* run = ent + (size_t)(w + NW * (g0 + u)) * estride + st;
        for (uint32_t i = 64 * R + lane; i < len; i += 64) {
          const uint32_t v = run[i];
          atomicOr(&tile[v >> 5], 1u << (v & 31));
        }
      }
    }
  }
  CB_STAMP(2);
  __syncthreads();
  CB_STAMP(3);
  tile_from_lds<NT>(gt, lt, tw);
  CB_STAMP(4);
}

// The tile pass over 16-bit entries (batched builds of long runs, C4): the
// partition binned by sub-tiles of 2^16 bits (S = 2^SUB per tile), so block
// b's entries for tile t are one contiguous super-run [seg[b][S t],
// seg[b][S (t+1)]) and sub-tile j's part of it starts at seg[b][S t + j].
// Lanes 0 .. G (S+1) - 1 load the G blocks' S + 1 bounds; an entry's
// sub-tile is the number of interior bounds at or below its index (uniform
// values taken by readlane, S - 1 compares), its bit (j << 16) | entry. Half
// the entry bytes of k_build_tile for S - 1 compares per entry.
template <int G, int R, int SUB, uint32_t NT = kBuildNT>
__global__ __launch_bounds__(NT) void k_build_tile_sub(BuildBatch bb, uint32_t tb, uint32_t T,
                                                       const uint32_t* __restrict__ seg_all,
                                                       uint32_t nblk,
                                                       const uint16_t* __restrict__ ent_all,
                                                       uint32_t estride) {
  constexpr uint32_t NW = NT / 64, S = 1u << SUB, NB = S + 1;
  static_assert(G * NB <= 64, "one lane per bound");
  uint32_t* __restrict__ words = bb.words[blockIdx.y];
  const bool fresh = (bb.fresh >> blockIdx.y) & 1ull;
  const uint32_t TS = T << SUB;  // bins per filter
  const uint32_t* __restrict__ seg = seg_all + (size_t)blockIdx.y * nblk * (TS + 1);
  const uint16_t* __restrict__ ent = ent_all + (size_t)blockIdx.y * nblk * estride;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t tw = 1u << (tb - 5);
  uint32_t* tile = smem;
  const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const uint32_t t = xcd_order(blockIdx.x, T);
  const uint32_t lu = lane / NB, lk = lane - lu * NB;  // this lane's bound: block lu, bound lk

  uint32_t sb = 0;  // first group's bounds in flight while the tile is cleared / loaded
  {
    const uint32_t b = w + NW * lu;
    if (lane < G * NB && b < nblk) sb = seg[(size_t)b * (TS + 1) + (t << SUB) + lk];
  }
  uint4* gt = reinterpret_cast<uint4*>(words + (size_t)t * tw);
  uint4* lt = reinterpret_cast<uint4*>(tile);
  tile_to_lds<NT>(lt, gt, tw, fresh);

  for (uint32_t g0 = 0; w + NW * g0 < nblk; g0 += G) {
    if (g0) {
      sb = 0;
      const uint32_t b = w + NW * (g0 + lu);
      if (lane < G * NB && b < nblk) sb = seg[(size_t)b * (TS + 1) + (t << SUB) + lk];
    }
    uint32_t o[R][G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const uint32_t st = __builtin_amdgcn_readlane(sb, u * NB);
      const uint32_t len = __builtin_amdgcn_readlane(sb, u * NB + S) - st;
      const uint32_t b = w + NW * (g0 + u);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        o[q][u] = 0;
        if (64 * q + lane < len) o[q][u] = ent[(size_t)b * estride + st + 64 * q + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const uint32_t st = __builtin_amdgcn_readlane(sb, u * NB);
      const uint32_t len = __builtin_amdgcn_readlane(sb, u * NB + S) - st;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const uint32_t i = 64 * q + lane;
        if (i < len) {
          uint32_t j = 0;
#pragma unroll
          for (uint32_t k = 1; k < S; ++k) j += (st + i >= __builtin_amdgcn_readlane(sb, u * NB + k)) ? 1u : 0u;
          const uint32_t v = (j << 16) | o[q][u];
          atomicOr(&tile[v >> 5], 1u << (v & 31));
        }
      }
    }
    // super-runs longer than R waves (skewed inputs)
    bool longrun = false;
#pragma unroll
    for (int u = 0; u < G; ++u)
      longrun |= __builtin_amdgcn_readlane(sb, u * NB + S) - __builtin_amdgcn_readlane(sb, u * NB) > 64u * R;
    if (longrun) {
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const uint32_t st = __builtin_amdgcn_readlane(sb, u * NB);
        const uint32_t len = __builtin_amdgcn_readlane(sb, u * NB + S) - st;
        const uint16_t* run = ent + (size_t)(w + NW * (g0 + u)) * estride + st;
        for (uint32_t i = 64 * R + lane; i < len; i += 64) {
          uint32_t j = 0;
#pragma unroll
          for (uint32_t k = 1; k < S; ++k) j += (st + i >= __builtin_amdgcn_readlane(sb, u * NB + k)) ? 1u : 0u;
          const uint32_t v = (j << 16) | run[i];
          atomicOr(&tile[v >> 5], 1u << (v & 31));
        }
      }
    }
  }
  __syncthreads();
  tile_from_lds<NT>(gt, lt, tw);
}

// The launches as steps, each behind one call (tools/ubench_build.hip times
// them one by one).

// What the two passes can run: the bins fit the partition histogram, the
// batch the kernel arguments, and 16-bit entries go with tiles of 2^(16 + sub) bits.
bool build_plan_ok(const TilePlan& p, uint32_t nb) {
  if (!plan_ok(p) || nb > kMaxBuildBatch || p.nblk > kMaxBuildBlocks) return false;
  return !p.sub || (p.sub <= 3 && p.tb == 16 + p.sub && ((uint64_t)p.T << p.sub) <= kMaxTiles);
}

template <int KK, int MM, int KPT>
void build_part(const TilePlan& p, const BuildBatch& bb, uint32_t nb, const ModP& mp, uint32_t* seg, uint32_t* ent,
                hipStream_t s) {
  const size_t lds = build_part_lds(p);
  if (p.sub) {  // 16-bit entries binned by 2^16-bit sub-tile
    allow_lds(k_build_part<KK, MM, KPT, uint16_t>, lds);
    hipLaunchKernelGGL((k_build_part<KK, MM, KPT, uint16_t>), dim3(p.nblk, nb), dim3(kBuildNT), lds, s, bb, mp,
                       16u, p.T << p.sub, seg, ent);
    return;
  }
  allow_lds(k_build_part<KK, MM, KPT>, lds);
  hipLaunchKernelGGL((k_build_part<KK, MM, KPT>), dim3(p.nblk, nb), dim3(kBuildNT), lds, s, bb, mp,
                     p.tb, p.T, seg, ent);
}

// The partition pass: k_build_part for the plan's keys per thread and entry type.
hipError_t build_partition(int keyk, int mode, const BuildBatch& bb, uint32_t nb, const ModP& mp, const TilePlan& p,
                           uint32_t* seg, uint32_t* ent, hipStream_t s) {
  {
    ProfScope ps("k_build_part", s);
    if (p.kpt == 1) {
      CB_KEY_MODE_DISPATCH(keyk, mode, (build_part<KK, MM, 1>(p, bb, nb, mp, seg, ent, s)));
    } else if (p.kpt == 2) {
      CB_KEY_MODE_DISPATCH(keyk, mode, (build_part<KK, MM, 2>(p, bb, nb, mp, seg, ent, s)));
    } else {
      CB_KEY_MODE_DISPATCH(keyk, mode, (build_part<KK, MM, 4>(p, bb, nb, mp, seg, ent, s)));
    }
  }
  return hipGetLastError();
}

template <class K, class E>
void build_tile(K kernel, uint32_t threads, const BuildBatch& bb, uint32_t nb, const TilePlan& p, const uint32_t* seg,
                const E* ent, hipStream_t s) {
  const size_t lds = build_tile_lds(p);
  allow_lds(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3(p.T, nb), dim3(threads), lds, s, bb, p.tb, p.T, seg, p.nblk, ent, 2 * p.C);
}

// The tile pass: k_build_tile_sub over 16-bit entries, else k_build_tile with
// two rounds of run loads for long runs and one otherwise.
hipError_t build_tiles(const BuildBatch& bb, uint32_t nb, const TilePlan& p, const uint32_t* seg, const uint32_t* ent,
                       hipStream_t s) {
  ProfScope ps("k_build_tile", s);
  if (p.sub) {
    const uint16_t* e16 = reinterpret_cast<const uint16_t*>(ent);
    if (p.sub == 2)  // 2^18-bit tiles: 512-thread workgroups, four per CU
      build_tile(k_build_tile_sub<8, 2, 2, 512>, 512, bb, nb, p, seg, e16, s);
    else if (p.sub == 1)
      build_tile(k_build_tile_sub<4, 2, 1>, kBuildNT, bb, nb, p, seg, e16, s);
    else
      build_tile(k_build_tile_sub<4, 2, 3>, kBuildNT, bb, nb, p, seg, e16, s);
  } else if (long_runs(p.C, p.T)) {
    build_tile(k_build_tile<8, 2>, kBuildNT, bb, nb, p, seg, ent, s);
  } else {
    build_tile(k_build_tile<16, 1>, kBuildNT, bb, nb, p, seg, ent, s);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_build_batch(int keyk, int mode, const BuildBatch& bb, uint32_t nb,
                              const ModP& mp, const TilePlan& p, uint32_t* seg, uint32_t* ent,
                              hipStream_t s) {
  if (!nb) return hipSuccess;
  if (!build_plan_ok(p, nb)) return hipErrorInvalidValue;
  const hipError_t e = build_partition(keyk, mode, bb, nb, mp, p, seg, ent, s);
  if (e != hipSuccess) return e;
  return build_tiles(bb, nb, p, seg, ent, s);
}

hipError_t launch_build_tiled(int keyk, int mode, uint32_t* words, bool fresh, const KeySrc& ks,
                              uint64_t n, const ModP& mp, const TilePlan& p, uint32_t* seg,
                              uint32_t* ent, hipStream_t s) {
  if (!n) return hipSuccess;
  BuildBatch bb{};
  bb.ks[0] = ks;
  bb.n[0] = n;
  bb.words[0] = words;
  bb.fresh = fresh ? 1u : 0u;
  return launch_build_batch(keyk, mode, bb, 1, mp, p, seg, ent, s);
}

}  // namespace cb
