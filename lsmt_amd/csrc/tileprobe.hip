// tileprobe.hip — the tiled probe of a key batch against filters of one size,
// in three passes (the plan: tileplan.hpp plan_probe).
//
// Reference semantics: /root/reference/src/bloom.rs:26-37,48-51 (hashes /
// may_contain). Filter layout in HBM: packed uint32 words, bit p at word p>>5,
// bit p&31 (LSB-first).
//
//   k_part_probe    partitions the batch by the filter tile of bit a;
//   k_tile_probe    one workgroup per tile streams each filter's tile through
//                   LDS, tests bit a from LDS, and reads bit b from HBM only
//                   when bit a is set (the reference's `&&` short-circuit,
//                   src/bloom.rs:50);
//   k_masks_to_hits un-permutes the result masks and transposes them into
//                   the hit bitmaps by wave64 ballots.
//
// Partition layout (as the build's, tilebuild.hip): partition block b (C keys)
// writes its entries sorted by tile into ent[b*C ...] and, in
// seg[b*(T+1) + t], the start of tile t's run inside that region
// (seg[b*(T+1) + T] = the block's total). Tile t's entries are therefore the
// runs [seg[b][t], seg[b][t+1]) of every block b.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "devutil.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "profile.hpp"

namespace cb {
namespace {

// Last b with P[b] <= j (P: exclusive prefix of the runs' lengths, P[0] = 0).
__device__ __forceinline__ uint32_t seg_find(const uint32_t* P, uint32_t nblk, uint32_t j) {
  uint32_t lo = 0, hi = nblk;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (P[mid] <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;
}

// Loads tile t's run table into LDS: S[b] = run start in block b's region,
// P[b] = exclusive prefix of run lengths. Returns the tile's entry count.
template <uint32_t NT>
__device__ uint32_t load_runs(const uint32_t* __restrict__ seg, uint32_t nblk, uint32_t T,
                              uint32_t t, uint32_t* S, uint32_t* P, uint32_t* wsum) {
  for (uint32_t b = threadIdx.x; b < nblk; b += NT) {
    const uint32_t* row = seg + (size_t)b * (T + 1) + t;
    const uint32_t s0 = row[0], s1 = row[1];
    S[b] = s0;
    P[b] = s1 - s0;
  }
  __syncthreads();
  return block_exclusive_scan<NT>(P, nblk, wsum);
}

// Partition for probe: one 8-byte entry per key, bucketed by the tile of bit
// a: x = (offset of a in its tile) | (key index within the block << tb),
// y = b. Requires tb + log2(C) <= 32 and m <= 2^32 (checked on the host).
// lkey[b*C + i] = the block-local key index of region slot i: k_tile_probe
// writes each key's result mask at its entry's slot, and k_masks_to_hits
// reads a block's region back in order and un-permutes it in LDS.
template <int KEYK, int MODE, int KPT>
__global__ __launch_bounds__(kPartThreads) void k_part_probe(KeySrc ks, uint64_t n, ModP mp,
                                                             uint32_t tb, uint32_t T,
                                                             uint32_t* __restrict__ seg,
                                                             uint2* __restrict__ ent,
                                                             uint16_t* __restrict__ lkey) {
  constexpr uint32_t C = kPartThreads * KPT;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t Tp = part_hist_words(T);  // the layout and its bytes: probe_part_lds (tileplan.hpp)
  uint32_t* hist = smem;
  uint2* stage = reinterpret_cast<uint2*>(smem + Tp);
  uint16_t* lstage = reinterpret_cast<uint16_t*>(stage + C);
  uint32_t* wsum = reinterpret_cast<uint32_t*>(lstage + C);
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < Tp; i += kPartThreads) hist[i] = 0;
  __syncthreads();

  const uint64_t kbase = (uint64_t)blockIdx.x * C;
  const uint32_t tmask = (1u << tb) - 1u;
  uint32_t et[KPT], er[KPT];
  uint2 rec[KPT];
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const uint32_t local = (uint32_t)j * kPartThreads + tid;
    const uint64_t k = kbase + local;
    et[j] = 0xFFFFFFFFu;
    if (k < n) {
      uint64_t a, b;
      key_positions<KEYK, MODE>(ks, k, mp, a, b);
      et[j] = (uint32_t)(a >> tb);
      er[j] = atomicAdd(&hist[et[j]], 1u);
      rec[j] = make_uint2(((uint32_t)a & tmask) | (local << tb), (uint32_t)b);
    }
  }
  __syncthreads();
  const uint32_t total = block_exclusive_scan<kPartThreads>(hist, T, wsum);
  if (tid == 0) hist[T] = total;
  __syncthreads();
  uint32_t* srow = seg + (size_t)blockIdx.x * (T + 1);
  for (uint32_t t = tid; t <= T; t += kPartThreads) srow[t] = hist[t];
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (et[j] != 0xFFFFFFFFu) {
      const uint32_t slot = hist[et[j]] + er[j];
      stage[slot] = rec[j];
      lstage[slot] = (uint16_t)(j * kPartThreads + tid);
    }
  }
  __syncthreads();
  uint2* out = ent + (size_t)blockIdx.x * C;
  uint16_t* lout = lkey + (size_t)blockIdx.x * C;
  for (uint32_t i = tid; i < total; i += kPartThreads) {
    out[i] = stage[i];
    lout[i] = lstage[i];
  }
}

// Probe one tile against up to 32 filters (group blockIdx.y). Each filter's
// tile is streamed HBM -> registers -> LDS through a D-deep register ring, so
// D tiles are in flight while the current one is tested. Bit a is tested in
// LDS; bit b is gathered from HBM only for (key, filter) pairs whose bit a was
// set. Output: masks[g*n + key] = per-filter result bits.
// RPT = uint4 per thread per tile (tile bits = RPT * 16 * 8 * NT).
template <int EPT, int RPT, int D>
__global__ __launch_bounds__(kTileProbeThreads) void k_tile_probe(
    FilterPtrs fp, uint32_t nf, uint32_t tb, uint32_t T, const uint32_t* __restrict__ seg,
    uint32_t nblk, const uint2* __restrict__ ent, uint32_t C, uint64_t n,
    uint32_t* __restrict__ masks) {
  constexpr uint32_t NT = kTileProbeThreads;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t tw = 1u << (tb - 5);  // == RPT * 4 * NT
  const uint32_t nbp = (nblk + 3) & ~3u;
  // the layout and its bytes: probe_tile_lds (tileplan.hpp)
  uint32_t* buf = smem;  // 2 * tw
  uint32_t* P = buf + 2 * tw;
  uint32_t* S = P + nbp;
  uint32_t* wsum = S + nbp;                                                  // NT/64 words
  const uint32_t** fw = reinterpret_cast<const uint32_t**>(wsum + NT / 64);  // 32 pointers
  const uint32_t tid = threadIdx.x;
  const uint32_t t = xcd_order(blockIdx.x, T), g = blockIdx.y;
  const uint32_t f0 = g * kFiltersPerGroup;
  const uint32_t nfg = min(kFiltersPerGroup, nf - f0);
  const uint32_t tmask = (1u << tb) - 1u;
  if (tid < nfg) fw[tid] = fp.w[f0 + tid];

  // Register ring: slot s holds filter fb+s's tile. Each slot is its own
  // named array so every index is static (no scratch); a slot is refilled
  // right after it is committed to LDS, keeping D tiles in flight. Loads go
  // through address-space-1 pointers (global_load, counted vmcnt waits).
  u32x4 r0[RPT], r1[RPT], r2[RPT], r3[RPT];
#define TP_FETCH(R, F)                                                        \
  {                                                                           \
    const gptr_u4 src = (gptr_u4)(fp.w[f0 + (F)] + (size_t)t * tw);           \
    _Pragma("unroll") for (int q = 0; q < RPT; ++q) R[q] = src[tid + q * NT]; \
  }
#define TP_FETCH_FIRST()                  \
  {                                       \
    TP_FETCH(r0, 0);                      \
    if (1 < nfg) TP_FETCH(r1, 1);         \
    if constexpr (D == 4) {               \
      if (2 < nfg) TP_FETCH(r2, 2);       \
      if (3 < nfg) TP_FETCH(r3, 3);       \
    }                                     \
  }
  // The first D tiles are requested before the run table and entries are
  // read, so their HBM latency overlaps the prologue.
  TP_FETCH_FIRST();

  const uint32_t E = load_runs<NT>(seg, nblk, T, t, S, P, wsum);
  uint32_t* mg = masks + (size_t)g * n;  // results go to each entry's region slot

  for (uint32_t cbase = 0; cbase < E; cbase += NT * EPT) {
    if (cbase) TP_FETCH_FIRST();  // rare extra chunk: stream the tiles again
    const uint32_t cn = min(E - cbase, NT * EPT);
    const uint32_t per = (cn + NT - 1) / NT;
    const uint32_t j0 = cbase + min(tid * per, cn);
    const uint32_t cnt = cbase + min(tid * per + per, cn) - j0;
    uint32_t off[EPT], pb[EPT], am[EPT], slot[EPT];
    {
      uint32_t b = cnt ? seg_find(P, nblk, j0) : 0;
      uint32_t pnext = (b + 1 < nblk) ? P[b + 1] : E;
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        am[i] = 0;
        off[i] = 0;  // unused slots test bit 0 (branch-free LDS reads) and are dropped
        if ((uint32_t)i < cnt) {
          const uint32_t j = j0 + i;
          while (j >= pnext) {
            ++b;
            pnext = (b + 1 < nblk) ? P[b + 1] : E;
          }
          slot[i] = b * C + S[b] + (j - P[b]);
          const uint2 r = ent[slot[i]];
          off[i] = r.x & tmask;
          pb[i] = r.y;
        }
      }
    }

#define TP_STAGE(R, F)                                                                     \
  {                                                                                        \
    const uint32_t f_ = (F);                                                               \
    u32x4* dst = reinterpret_cast<u32x4*>(buf + (f_ & 1) * tw);                            \
    _Pragma("unroll") for (int q = 0; q < RPT; ++q) dst[tid + q * NT] = R[q];              \
    __syncthreads();                                                                       \
    if (f_ + D < nfg) TP_FETCH(R, f_ + D);                                                 \
    const uint32_t* lb = buf + (f_ & 1) * tw;                                              \
    _Pragma("unroll") for (int i = 0; i < EPT; ++i) am[i] |=                               \
        ((lb[off[i] >> 5] >> (off[i] & 31)) & 1u) << f_;                                   \
  }
    for (uint32_t fb = 0; fb < nfg; fb += D) {
      TP_STAGE(r0, fb);
      if (fb + 1 < nfg) TP_STAGE(r1, fb + 1);
      if constexpr (D == 4) {
        if (fb + 2 < nfg) TP_STAGE(r2, fb + 2);
        if (fb + 3 < nfg) TP_STAGE(r3, fb + 3);
      }
    }
#undef TP_STAGE
    __syncthreads();  // the LDS buffers are rewritten by the next chunk

    // Bit b of every (entry, filter) pair whose bit a was set, gathered from
    // HBM in rounds: each round issues one independent load per entry.
    uint32_t mask[EPT], x[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      mask[i] = 0;
      x[i] = (uint32_t)i < cnt ? am[i] : 0u;
    }
    for (;;) {
      uint32_t any = 0, v[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        any |= x[i];
        v[i] = x[i] ? ((gptr_u32)fw[__builtin_ctz(x[i])])[pb[i] >> 5] : 0u;
      }
      if (!any) break;
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        if (x[i]) {
          const uint32_t f = __builtin_ctz(x[i]);
          mask[i] |= ((v[i] >> (pb[i] & 31)) & 1u) << f;
          x[i] &= x[i] - 1;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i)
      if ((uint32_t)i < cnt) mg[slot[i]] = mask[i];
  }
#undef TP_FETCH_FIRST
#undef TP_FETCH
}

constexpr uint32_t kHitsThreads = 512;

// Un-permute one partition block's results and transpose them into the
// [filter][n/64] hit bitmaps. Block b reads its region's masks and local key
// indices in order (coalesced), scatters the masks into LDS by key, then each
// wave turns 64 keys into one word per filter with wave64 ballots; the words
// are staged in LDS so every filter row leaves as whole contiguous segments.
template <int KPT>
__global__ __launch_bounds__(kHitsThreads) void k_masks_to_hits(
    const uint32_t* __restrict__ masks, const uint16_t* __restrict__ lkey, FilterPtrs fp,
    uint32_t nf, uint64_t n, uint64_t* __restrict__ hits, uint64_t hwords) {
  constexpr uint32_t C = kPartThreads * KPT;  // keys per partition block
  constexpr uint32_t W = C / 64;              // hit words per filter row
  constexpr uint32_t G = kMaxFiltersPerLaunch / kFiltersPerGroup;
  __shared__ uint32_t km[G][C];
  __shared__ uint64_t hb[kMaxFiltersPerLaunch][W];
  __shared__ uint32_t rows[kMaxFiltersPerLaunch];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t ng = (nf + kFiltersPerGroup - 1) / kFiltersPerGroup;
  const uint64_t kbase = (uint64_t)blockIdx.x * C;
  const uint32_t cnt = (uint32_t)min((uint64_t)C, n - kbase);
  if (tid < nf) rows[tid] = fp.row[tid];
  for (uint32_t i = tid; i < cnt; i += kHitsThreads) {
    const uint32_t lk = lkey[kbase + i];
    km[0][lk] = masks[kbase + i];
    if (ng > 1) km[1][lk] = masks[n + kbase + i];
  }
  __syncthreads();
  for (uint32_t w = wave; w < W; w += kHitsThreads / 64) {
    const uint32_t kl = w * 64 + lane;
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) {
      if (g < ng) {
        const uint32_t m = kl < cnt ? km[g][kl] : 0u;
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t f = 0; f < kFiltersPerGroup; ++f) {
          const uint64_t bal = __ballot((m >> f) & 1u);
          mine = (lane == f) ? bal : mine;
        }
        if (lane < min(kFiltersPerGroup, nf - g * kFiltersPerGroup))
          hb[g * kFiltersPerGroup + lane][w] = mine;
      }
    }
  }
  __syncthreads();
  const uint64_t wbase = kbase / 64, nw = (n + 63) / 64;
  for (uint32_t i = tid; i < nf * W; i += kHitsThreads) {
    const uint32_t f = i / W, w = i % W;
    if (wbase + w < nw) hits[(uint64_t)rows[f] * hwords + wbase + w] = hb[f][w];
  }
}

}  // namespace

template <int KK, int MM, int KPT>
static void part_probe(const TilePlan& p, const KeySrc& ks, uint64_t n, const ModP& mp,
                       uint32_t* seg, uint2* ent, uint16_t* lkey, size_t lds, hipStream_t s) {
  allow_lds(k_part_probe<KK, MM, KPT>, lds);
  hipLaunchKernelGGL((k_part_probe<KK, MM, KPT>), dim3(p.nblk), dim3(kPartThreads), lds, s, ks, n,
                     mp, p.tb, p.T, seg, ent, lkey);
}

hipError_t launch_probe_partition(int keyk, int mode, const KeySrc& ks, uint64_t n,
                                  const ModP& mp, const TilePlan& p, uint32_t* seg, uint2* ent,
                                  uint16_t* lkey, hipStream_t s) {
  if (!n) return hipSuccess;
  // an entry's 32 bits hold tb + kProbeLocalBits; the bit to spare stays, so that what is refused does not change
  if (!plan_ok(p) || p.tb + kProbeLocalBits + 1 > 32) return hipErrorInvalidValue;
  const size_t lds = probe_part_lds(p);
  ProfScope ps("k_part_probe", s);
  if (p.kpt == 4) {
    CB_KEY_MODE_DISPATCH(keyk, mode, (part_probe<KK, MM, 4>(p, ks, n, mp, seg, ent, lkey, lds, s)));
  } else {
    CB_KEY_MODE_DISPATCH(keyk, mode, (part_probe<KK, MM, 8>(p, ks, n, mp, seg, ent, lkey, lds, s)));
  }
  return hipGetLastError();
}

template <int RPT>
static hipError_t tile_probe(const FilterPtrs& fp, uint32_t nf, uint64_t n, const TilePlan& p,
                             const uint32_t* seg, const uint2* ent, uint32_t* masks, size_t lds,
                             uint32_t G, hipStream_t s) {
  // The instantiation must cover the tile exactly: RPT uint4 per thread.
  if ((1u << (p.tb - 5)) != (uint32_t)RPT * 4u * kTileProbeThreads) return hipErrorInvalidValue;
  constexpr int D = RPT >= 4 ? 2 : 4;  // 32-64 KiB of tiles in flight per workgroup
  allow_lds(k_tile_probe<8, RPT, D>, lds);
  hipLaunchKernelGGL((k_tile_probe<8, RPT, D>), dim3(p.T, G), dim3(kTileProbeThreads), lds, s, fp,
                     nf, p.tb, p.T, seg, p.nblk, ent, p.C, n, masks);
  return hipGetLastError();
}

hipError_t launch_probe_tiles(const FilterPtrs& fp, uint32_t nf, uint64_t n, const TilePlan& p,
                              const uint32_t* seg, const uint2* ent, const uint16_t* lkey,
                              uint32_t* masks, uint64_t* hits, uint64_t hwords, hipStream_t s) {
  if (!n || !nf) return hipSuccess;
  const size_t lds = probe_tile_lds(p);
  const uint32_t G = (nf + kFiltersPerGroup - 1) / kFiltersPerGroup;
  hipError_t e;
  {
    ProfScope ps("k_tile_probe", s);
    // tile bits = RPT * 16 B * 8 * 512 threads = RPT * 2^16
    switch (p.tb) {
      case 16: e = tile_probe<1>(fp, nf, n, p, seg, ent, masks, lds, G, s); break;
      case 17: e = tile_probe<2>(fp, nf, n, p, seg, ent, masks, lds, G, s); break;
      case 18: e = tile_probe<4>(fp, nf, n, p, seg, ent, masks, lds, G, s); break;
      default: e = hipErrorInvalidValue;
    }
  }
  if (e != hipSuccess) return e;
  ProfScope ps("k_masks_to_hits", s);
  if (p.kpt == 4)
    hipLaunchKernelGGL((k_masks_to_hits<4>), dim3(p.nblk), dim3(kHitsThreads), 0, s, masks, lkey,
                       fp, nf, n, hits, hwords);
  else
    hipLaunchKernelGGL((k_masks_to_hits<8>), dim3(p.nblk), dim3(kHitsThreads), 0, s, masks, lkey,
                       fp, nf, n, hits, hwords);
  return hipGetLastError();
}

}  // namespace cb
