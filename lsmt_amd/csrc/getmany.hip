// getmany.hip — Database::get's newest-first walk over many tables, batched
// (see sstable.hpp for the reference mapping): the gate from hit rows
// (k_get_many), from a FilterSet (k_set_get_many), from tiered sets
// (k_tier_get_many) or from a wide set (k_wide_get_many).
//
// Resolution is latency-bound random access: one lane per key. Each lane
// gathers its candidate tables first and then searches its own next
// candidate, so a wave's lanes search different tables concurrently. The
// kernels differ in how a key's candidate word is made; the staging of views
// and maps, the walk and the epilogue are shared.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "knobs.hpp"
#include "launch.hpp"
#include "profile.hpp"
#include "setmask.hpp"
#include "sstable.hpp"
#include "tablesearch.hpp"
#include "tiermask.hpp"
#include "wideset.hpp"
#include "zone.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;

}  // namespace

namespace {

// Up to 64 tables' views (tv[0 .. nt): a group's, from its base table on),
// staged once per workgroup of NT threads into LDS: loaded into registers
// first (the narrow kernels issue these with the key and gate loads, so their
// round trip overlaps those), then stored after the gate. The caller's
// barrier publishes them.
constexpr uint32_t kViewDw = sizeof(TableView) / 4;
static_assert(sizeof(TableView) % 4 == 0, "dword copy");
template <uint32_t NT>
struct ViewRegs {
  static constexpr uint32_t kPer = (64 * kViewDw + NT - 1) / NT;
  uint32_t w[kPer];
};
template <uint32_t NT>
__device__ __forceinline__ ViewRegs<NT> load_views(const TableView* tv, uint32_t nt) {
  ViewRegs<NT> v;
  const uint32_t nd = (nt < 64 ? nt : 64) * kViewDw;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tv);
#pragma unroll
  for (uint32_t i = 0; i < ViewRegs<NT>::kPer; ++i) {
    const uint32_t d = threadIdx.x + i * NT;
    v.w[i] = d < nd ? src[d] : 0u;
  }
  return v;
}
template <uint32_t NT>
__device__ __forceinline__ void store_views(const ViewRegs<NT>& v, uint32_t nt, TableView* stv) {
  const uint32_t nd = (nt < 64 ? nt : 64) * kViewDw;
  uint32_t* dst = reinterpret_cast<uint32_t*>(stv);
#pragma unroll
  for (uint32_t i = 0; i < ViewRegs<NT>::kPer; ++i) {
    const uint32_t d = threadIdx.x + i * NT;
    if (d < nd) dst[d] = v.w[i];
  }
}

// The DirMaps of up to 64 tables (their views already in LDS) into LDS, 16 B
// per thread and step; barrier at the end. The search computes its bucket
// from these words (sstable.hpp dir_bucket) without a memory round trip.
constexpr uint32_t kMapWords = sizeof(DirMap) / 16;
template <uint32_t NT>
__device__ __forceinline__ void stage_maps(const TableView* stv, uint32_t nt, DirMap* sdm) {
  const uint32_t nm = (nt < 64 ? nt : 64) * kMapWords;
  for (uint32_t i = threadIdx.x; i < nm; i += NT) {
    const uint32_t t = i / kMapWords, k = i - t * kMapWords;
    const DirMap* g = stv[t].dmap;
    if (g) reinterpret_cast<uint4*>(sdm + t)[k] = reinterpret_cast<const uint4*>(g)[k];
  }
  __syncthreads();
}

// SsTable::get of table v (table t of the list; dm: its DirMap) for Database::
// get's `if let Ok(Some(v))`: true when the table holds the key with a value
// that decodes; then w = t, src = the value's base64 bytes, d = their decoded
// length.
__device__ __forceinline__ bool table_answers(const TableView& v, const DirMap* dm, uint32_t t, const Query& q,
                                              int32_t& w, uint64_t& src, uint64_t& d) {
  LineRec r;
  if (search(v, q, r, dm) < 0) return false;  // Ok(None)
  if (r.vdl == kBadValue) return false;       // Err(..) is skipped by `if let Ok(Some(v))`
  w = (int32_t)t;
  src = (uint64_t)(uintptr_t)(v.data + r.start + r.klen + 1);
  d = r.vdl;
  return true;
}

// The end of every get kernel, in two steps. put_answer: key k's answer (w /
// src / d, d = 0 when none) into which / vsrc / dlen; the narrow kernels call
// it inside the branch that searched. (One step that also takes the liveness
// check, called after that branch, was measured: the compiler keeps the two
// branches apart, and every narrow kernel's code and SGPR count moved.)
__device__ __forceinline__ void put_answer(uint64_t k, int32_t w, uint64_t src, uint64_t d, int32_t* which,
                                           uint64_t* vsrc, uint64_t* dlen) {
  which[k] = w;
  vsrc[k] = src;
  dlen[k] = d;
}
// tile_sums, by every thread of the workgroup of NT: its value bytes per
// 256-key tile, for k_b64_decode's offsets (get_tiles). A workgroup of one
// tile writes its total; a larger one takes its tiles' sums from the scan's
// prefixes at their bounds (bnd: NT / 256 + 1 words of LDS).
template <uint32_t NT>
__device__ __forceinline__ void tile_sums(uint64_t d, uint64_t n, uint64_t* tsum, uint64_t* bnd = nullptr) {
  uint64_t total;
  const uint64_t pre = block_scan<NT>(d, &total);
  if constexpr (NT == kNT) {
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
  } else {
    constexpr uint32_t T = NT / kNT;
    if (threadIdx.x % kNT == 0) bnd[threadIdx.x / kNT] = pre;
    if (threadIdx.x == 0) bnd[T] = total;
    __syncthreads();
    const uint64_t t0 = (uint64_t)T * blockIdx.x;
    if (threadIdx.x < T && (t0 + threadIdx.x) * kNT < n) tsum[t0 + threadIdx.x] = bnd[threadIdx.x + 1] - bnd[threadIdx.x];
  }
}

// One group of up to 64 tables (t0 .. t0 + 63): every candidate in cand,
// newest first, until a table answers Ok(Some). Returns whether one did.
// LDS_VIEWS (every table among the first 64): the search reads its table's
// view fields from LDS where it uses them instead of copying the 56-byte view
// into registers (88 -> 80 VGPRs: 6 waves per SIMD instead of 5).
template <bool LDS_VIEWS = false>
__device__ __forceinline__ bool resolve_group(const TableView* stv, const TableView* __restrict__ tv,
                                              const DirMap* sdm, uint32_t t0, uint64_t cand, const Query& q,
                                              int32_t& w, uint64_t& src, uint64_t& d) {
  while (cand) {
    const uint32_t t = t0 + (uint32_t)__builtin_ctzll(cand);
    cand &= cand - 1;
    if constexpr (LDS_VIEWS) {
      const TableView& v = stv[t];
      if (table_answers(v, t < 64 ? &sdm[t] : v.dmap, t, q, w, src, d)) return true;
    } else {
      const TableView v = t < 64 ? stv[t] : tv[t];
      if (table_answers(v, t < 64 ? &sdm[t] : v.dmap, t, q, w, src, d)) return true;
    }
  }
  return false;
}

// Database::get's walk for one key (src/lib.rs:129-134): tables in groups
// of 64, newest first (tables.iter().rev()). Each lane holds its candidate
// tables of the group as a bit mask (cand0 for the first 64; past them, from
// the hit rows), then every lane searches its OWN next candidate in the same
// iteration, so lanes whose keys live in different tables search concurrently
// instead of the wave stepping through the tables one by one. w / src / d:
// the first table whose SsTable::get returns Ok(Some), the value's base64
// bytes and their decoded length.
template <bool LDS_VIEWS>
__device__ __forceinline__ void resolve_key(const TableView* stv, const TableView* __restrict__ tv,
                                            const DirMap* sdm, uint32_t nt, uint64_t cand0,
                                            const uint64_t* __restrict__ hits,
                                            const uint32_t* __restrict__ rows, uint64_t hwords, uint64_t k,
                                            const Query& q, int32_t& w, uint64_t& src, uint64_t& d) {
  for (uint32_t t0 = 0; t0 < nt; t0 += 64) {
    const uint32_t gn = nt - t0 < 64 ? nt - t0 : 64;
    uint64_t cand = gn == 64 ? ~0ull : ((1ull << gn) - 1);
    if (t0 == 0) {
      cand = cand0;
    } else if (hits) {  // tables past the first 64: one broadcast load per table
      cand = 0;
      for (uint32_t i = 0; i < gn; ++i) {
        const uint64_t row = rows ? rows[t0 + i] : t0 + i;
        cand |= ((hits[row * hwords + (k >> 6)] >> (k & 63)) & 1) << i;  // the gate
      }
    }
    if (resolve_group<LDS_VIEWS>(stv, tv, sdm, t0, cand, q, w, src, d)) return;
  }
}

// LDS_VIEWS: nt <= 64 (every view staged in LDS; see resolve_group).
template <int KEYK, bool LDS_VIEWS>
__global__ __launch_bounds__(kNT, 6) void k_get_many(const TableView* __restrict__ tv, uint32_t nt,
                                                  const uint64_t* __restrict__ hits,
                                                  const uint32_t* __restrict__ rows,
                                                  uint64_t hwords, KeySrc ks, uint64_t n,
                                                  int32_t* __restrict__ which,
                                                  uint64_t* __restrict__ vsrc,
                                                  uint64_t* __restrict__ dlen,
                                                  uint64_t* __restrict__ tsum) {
  const uint64_t k = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  // The gate for the first 64 tables, with every lane of the wave active: a
  // wave's 64 keys share one hit word per table row, so lane i loads row i's
  // word (one load instruction for the wave, not one per table) and every
  // lane takes its bit of each row from lane i by a uniform shuffle.
  const ViewRegs<kNT> vr = load_views<kNT>(tv, nt);
  const uint32_t gn0 = nt < 64 ? nt : 64;
  uint64_t cand0 = gn0 == 64 ? ~0ull : ((1ull << gn0) - 1);
  // the key's loads go out with the gate's (independent of it)
  const Query q = make_query<KEYK>(ks, k < n ? k : 0);
  if (hits) {
    const uint64_t wi = ((uint64_t)blockIdx.x * kNT + (threadIdx.x & ~63u)) >> 6;
    uint64_t hw = 0;
    if (lane < gn0 && wi < hwords) hw = hits[(uint64_t)(rows ? rows[lane] : lane) * hwords + wi];
    cand0 = 0;
    for (uint32_t i = 0; i < gn0; ++i) cand0 |= ((__shfl(hw, (int)i, 64) >> lane) & 1ull) << i;
  }
  // the first 64 tables' views, staged once per block: each lane's search
  // reads its table's view from LDS instead of a divergent global gather
  __shared__ TableView stv[64];
  __shared__ DirMap sdm[64];
  store_views(vr, nt, stv);
  __syncthreads();
  stage_maps<kNT>(stv, nt, sdm);
  uint64_t d = 0;
  if (k < n) {
    int32_t w = -1;
    uint64_t src = 0;
    if constexpr (LDS_VIEWS)
      (void)resolve_group<true>(stv, tv, sdm, 0, cand0, q, w, src, d);  // one group
    else
      resolve_key<false>(stv, tv, sdm, nt, cand0, hits, rows, hwords, k, q, w, src, d);
    put_answer(k, w, src, d, which, vsrc, dlen);
  }
  tile_sums<kNT>(d, n, tsum);
}

}  // namespace

hipError_t launch_get_many(int keyk, const TableView* tv, uint32_t nt, const uint64_t* hits,
                           const uint32_t* rows, uint64_t hwords, const KeySrc& ks, uint64_t n,
                           int32_t* which, uint64_t* vsrc, uint64_t* dlen, uint64_t* tsum,
                           hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_get_many", s);
  const dim3 g(blocks_for(n, kNT));
  CB_KEY_DISPATCH(
      keyk,
      if (nt <= 64) hipLaunchKernelGGL((k_get_many<KK, true>), g, dim3(kNT), 0, s, tv, nt, hits, rows, hwords, ks, n,
                                       which, vsrc, dlen, tsum);
      else hipLaunchKernelGGL((k_get_many<KK, false>), g, dim3(kNT), 0, s, tv, nt, hits, rows, hwords, ks, n, which,
                              vsrc, dlen, tsum));
  return hipGetLastError();
}

namespace {

// Database::get in one launch (src/lib.rs:129-134 with SsTable::get's gate,
// src/sstable.rs:138): k_get_many with the gate computed per key from the
// FilterSet (set_key_mask: set[a] & set[b] over every slot, the zone check
// for gated slots) instead of read from hit rows, so no rows are written or
// read and the set's random reads overlap the searches' in one kernel. Table
// t is slot slots[t] (slots NULL: slot t); nt <= W.
template <int KEYK, int MODE, int W>
__global__ __launch_bounds__(kNT, 6) void k_set_get_many(const void* __restrict__ set, ModP mp, ZoneView zv,
                                                      const TableView* __restrict__ tv, uint32_t nt,
                                                      const uint32_t* __restrict__ slots, KeySrc ks, uint64_t n,
                                                      int32_t* __restrict__ which, uint64_t* __restrict__ vsrc,
                                                      uint64_t* __restrict__ dlen, uint64_t* __restrict__ tsum) {
  const uint64_t k = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const ViewRegs<kNT> vr = load_views<kNT>(tv, nt);
  __shared__ BoundPrefix zp[2 * W];
  __shared__ uint32_t sslot[64];
  __shared__ TableView stv[64];
  __shared__ DirMap sdm[64];
  stage_zone_prefixes<KEYK, W>(zv, zp, kNT);
  if (slots && threadIdx.x < nt) sslot[threadIdx.x] = slots[threadIdx.x];
  // the key's loads go out before the barrier (after it, the compiler kept
  // the whole search's state live across the gate: 256 VGPRs, 1 wave/SIMD)
  const Query q = make_query<KEYK>(ks, k < n ? k : 0);
  store_views(vr, nt, stv);
  __syncthreads();  // views, slots and zone prefixes staged
  const auto mask = set_key_mask<KEYK, MODE, W, true, false>(set, ks, k, k < n, mp, zv, zp);
  uint64_t cand0 = 0;
  if (slots) {
    for (uint32_t i = 0; i < nt; ++i) cand0 |= (((uint64_t)mask >> sslot[i]) & 1ull) << i;
  } else {
    cand0 = (uint64_t)mask & (nt == 64 ? ~0ull : ((1ull << nt) - 1));
  }
  stage_maps<kNT>(stv, nt, sdm);
  uint64_t d = 0;
  if (k < n) {
    int32_t w = -1;
    uint64_t src = 0;
    (void)resolve_group<true>(stv, tv, sdm, 0, cand0, q, w, src, d);  // nt <= 64: one group
    put_answer(k, w, src, d, which, vsrc, dlen);
  }
  tile_sums<kNT>(d, n, tsum);
}

}  // namespace

template <int KK, int MM, int WW>
static void set_get_many(const void* set, const ModP& mp, const ZoneView& zv, const TableView* tv, uint32_t nt,
                         const uint32_t* slots, const KeySrc& ks, uint64_t n, int32_t* which, uint64_t* vsrc,
                         uint64_t* dlen, uint64_t* tsum, hipStream_t s) {
  // Measured and not kept (one lane, us per 1M keys): forcing 6 or 7 waves
  // per SIMD (80 / 72 VGPRs with spills) 112-115 / 131 against 108-110 at the
  // natural 90 VGPRs and 5 waves; set[b] read without the short-circuit
  // 111-113; the first two records of each bucket loaded with its prefixes
  // 107-109; gathering and decoding values of <= 18 bytes here (so
  // k_b64_decode reads them coalesced: 27 -> 14 us) 132, the value load being
  // one more dependent step at the end of every found key's chain;
  // compacting the searches (the gate for 2 or 3 keys per lane, the keys
  // with a candidate queued in LDS, then one queue entry per lane, so search
  // waves run full) 243-249: the wave count, not lane occupancy, bounds it.
  hipLaunchKernelGGL((k_set_get_many<KK, MM, WW>), dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, set, mp, zv, tv, nt,
                     slots, ks, n, which, vsrc, dlen, tsum);
}

hipError_t launch_set_get_many(int keyk, int mode, uint32_t width, const void* set, const ModP& mp,
                               const ZoneView* zones, const TableView* tv, uint32_t nt, const uint32_t* slots,
                               const KeySrc& ks, uint64_t n, int32_t* which, uint64_t* vsrc, uint64_t* dlen,
                               uint64_t* tsum, hipStream_t s) {
  if (!n) return hipSuccess;
  if (nt > width || (width != 32 && width != 64)) return hipErrorInvalidValue;
  const ZoneView zv = zones ? *zones : ZoneView{nullptr, nullptr, nullptr, 0};
  ProfScope ps("k_set_get_many", s);
  CB_SET_DISPATCH(keyk, mode, width,
                  (set_get_many<KK, MM, WW>(set, mp, zv, tv, nt, slots, ks, n, which, vsrc, dlen, tsum, s)));
  return hipGetLastError();
}

namespace {

// Database::get in one launch over tiered filter sets (tierset.hpp): the
// store after a compaction, whose tables' filters live in FilterSets of
// different m. k_set_get_many with tier_key_mask in place of set_key_mask:
// the key is hashed once for every tier and the result is already in table
// order, so it is the candidate word. nt <= 64: one group.
template <int KEYK, bool ALL32, int NS>
__global__ __launch_bounds__(kNT, 6) void k_tier_get_many(TierArgs ta, const TableView* __restrict__ tv, KeySrc ks,
                                                          uint64_t n, int32_t* __restrict__ which,
                                                          uint64_t* __restrict__ vsrc, uint64_t* __restrict__ dlen,
                                                          uint64_t* __restrict__ tsum) {
  const uint64_t k = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const uint32_t nt = ta.nt;
  const ViewRegs<kNT> vr = load_views<kNT>(tv, nt);
  __shared__ BoundPrefix zp[2 * kTierTables];
  __shared__ uint16_t stbl[kTierTables], ssrt[kTierTables];
  __shared__ TableView stv[64];
  __shared__ DirMap sdm[64];
  stage_tier_lists(ta, stbl, ssrt);
  stage_tier_prefixes<KEYK>(ta, zp, kNT);
  // the key's loads go out before the barrier (k_set_get_many: after it, the
  // compiler kept the whole search's state live across the gate)
  const Query q = make_query<KEYK>(ks, k < n ? k : 0);
  store_views(vr, nt, stv);
  __syncthreads();  // views, table lists and zone prefixes staged
  const uint64_t cand0 = tier_key_mask<KEYK, ALL32, NS, false>(ta, stbl, ssrt, ks, k, k < n, zp);
  stage_maps<kNT>(stv, nt, sdm);
  uint64_t d = 0;
  if (k < n) {
    int32_t w = -1;
    uint64_t src = 0;
    (void)resolve_group<true>(stv, tv, sdm, 0, cand0, q, w, src, d);
    put_answer(k, w, src, d, which, vsrc, dlen);
  }
  tile_sums<kNT>(d, n, tsum);
}

}  // namespace

template <int KK, bool AA, int NN>
static void tier_get_many(const TierArgs& ta, const TableView* tv, const KeySrc& ks, uint64_t n, int32_t* which,
                          uint64_t* vsrc, uint64_t* dlen, uint64_t* tsum, hipStream_t s) {
  hipLaunchKernelGGL((k_tier_get_many<KK, AA, NN>), dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, ta, tv, ks, n, which,
                     vsrc, dlen, tsum);
}

hipError_t launch_tier_get_many(int keyk, const TierArgs& ta, const TableView* tv, const KeySrc& ks, uint64_t n,
                                int32_t* which, uint64_t* vsrc, uint64_t* dlen, uint64_t* tsum, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!ta.nt || ta.nt > kTierTables || !ta.ns || ta.ns > kMaxTiers) return hipErrorInvalidValue;
  ProfScope ps("k_tier_get_many", s);
  CB_TIER_DISPATCH(keyk, ta.all32, ta.ns, (tier_get_many<KK, AA, NN>(ta, tv, ks, n, which, vsrc, dlen, tsum, s)));
  return hipGetLastError();
}

namespace {

// The wide walk's screen (wideset.hpp WideScreen): bit (B, h, slot) is clear
// only when the table in that slot has a complete key bucket B none of whose
// stored fingerprints falls in bin h (fp & (H - 1)). One thread per (table,
// bucket); bits are ORed in (tables share screen words). Tables whose
// buckets the screen cannot speak for (none yet, not well-formed, another
// bucket count) set every bin: they always pass.
__global__ __launch_bounds__(kNT) void k_wide_screen(const TableView* __restrict__ tv, const uint32_t* __restrict__ slots,
                                                     uint32_t nt, uint32_t R, uint32_t bits, uint32_t hbits,
                                                     uint64_t* __restrict__ scr) {
  const uint64_t nb = 1ull << bits, H = 1ull << hbits;
  const uint64_t idx = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (idx >= nb * nt) return;
  const uint32_t i = (uint32_t)(idx >> bits);
  const uint64_t B = idx & (nb - 1);
  const uint32_t slot = slots ? slots[i] : i;
  const TableView v = tv[i];
  unsigned long long* row = reinterpret_cast<unsigned long long*>(scr) + B * H * R + (slot >> 6);
  const unsigned long long bit = 1ull << (slot & 63u);
  if (v.bkt && v.fast() && v.bkbits() == bits) {
    const uint64_t sw = v.bkt[nb * kBktWords + B];
    const uint32_t nst = (uint32_t)(sw & 15u);
    if (nst <= kBktSlots) {  // the bins of the stored fingerprints
      for (uint32_t s = 0; s < nst; ++s) atomicOr(row + ((sw >> (4 + 15 * s)) & (H - 1)) * R, bit);
      return;
    }
  }
  for (uint64_t h = 0; h < H; ++h) atomicOr(row + h * R, bit);  // no proof: every bin
}

}  // namespace

hipError_t launch_wide_screen(const TableView* tv, const uint32_t* slots, uint32_t nt, uint32_t R, uint32_t bits,
                              uint32_t hbits, uint64_t* scr, hipStream_t s) {
  if (!nt || bits > 24 || hbits > 8) return hipErrorInvalidValue;
  ProfScope ps("k_wide_screen", s);
  const hipError_t e = hipMemsetAsync(scr, 0, wide_screen_bytes(R, bits, hbits), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_wide_screen, dim3(blocks_for(((uint64_t)nt) << bits, kNT)), dim3(kNT), 0, s, tv, slots, nt, R,
                     bits, hbits, scr);
  return hipGetLastError();
}

// The tables' DirMaps copied into one contiguous array (a table without a
// directory: zeros), so the walk stages a group's maps with plain loads in
// the same pass as its views (k_wide_get_many). One lane per 16 B.
__global__ __launch_bounds__(kNT) void k_gather_maps(const TableView* __restrict__ tv, uint32_t nt,
                                                     DirMap* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (i >= (uint64_t)nt * kMapWords) return;
  const uint32_t t = (uint32_t)(i / kMapWords), j = (uint32_t)(i - (uint64_t)t * kMapWords);
  const DirMap* g = tv[t].dmap;
  reinterpret_cast<uint4*>(out + t)[j] = g ? reinterpret_cast<const uint4*>(g)[j] : make_uint4(0, 0, 0, 0);
}

hipError_t launch_gather_maps(const TableView* tv, uint32_t nt, DirMap* out, hipStream_t s) {
  if (!nt) return hipSuccess;
  hipLaunchKernelGGL(k_gather_maps, dim3(blocks_for((uint64_t)nt * kMapWords, kNT)), dim3(kNT), 0, s, tv, nt, out);
  return hipGetLastError();
}

namespace {

// Database::get in one launch over a wide set (wideset.hpp): k_set_get_many
// for more than 64 tables. Per key: rows a and b of the set (h1 % m, h2 % m,
// src/bloom.rs:26-37); then the tables in groups of 64, newest first
// (tables.iter().rev(), src/lib.rs:130): the group's candidate bits are a
// 64-bit window of row a AND the same window of row b, the latter read only
// when the former is non-zero (src/bloom.rs:50), reordered to table order
// (groups[g].kind); then the candidates newest first: each one's bucket
// summary word, the zone gate for gated tables (src/sstable.rs:138), the
// search, and the first Ok(Some) ends the walk. The group's views and maps
// are staged in LDS.
// The wide walk's summary words loaded together: 4 / 8 / 16 at once measured
// 671-679 / 792-809 / 816-820 M gets/s against 517-519 one at a time (300
// tables of m = 1024); 16 doubles the scratch spill (36 -> 72 B per lane).
// With the screen (round 5) the batch no longer matters: 8 / 4 / 2 at once
// measured 2.145 / 2.140 / 2.139 G gets/s, the same VGPRs (experiment builds).
constexpr uint32_t kScreen = CB_WIDE_SCREEN_BATCH;
// (Round 4, before the screen: five waves per SIMD at its natural 96 VGPRs;
// forcing six, 80 VGPRs with 112 B of scratch per lane, measured 606-617
// against 782-804 M gets/s.)
// Four waves per SIMD, 109 VGPRs and no spill (round 5, with the screen):
// 1.81-1.84 against 1.63 G gets/s for five waves at 96 VGPRs and 56 B of
// spill per lane (experiment r05_wide4, HISTORY.md, alternating on one box).
// The walk's workgroup: kWideNT keys (two 256-key tiles of the value scan);
// a group's views and maps are staged once per workgroup, so 512 keys per
// workgroup halve the staging's L2 requests per lookup against 256.
constexpr uint32_t kWideNT = CB_WIDE_THREADS;
static_assert(kWideNT % kNT == 0 && kWideNT / kNT <= 4, "up to four value tiles per workgroup");
template <int KEYK, int MODE>
__global__ __launch_bounds__(kWideNT, 4) void k_wide_get_many(const uint64_t* __restrict__ set, uint32_t R, ModP mp,
                                                       WideZone z, const TableView* __restrict__ tv, uint32_t nt,
                                                       const WideGroup* __restrict__ groups,
                                                       const uint32_t* __restrict__ slots, KeySrc ks, uint64_t n,
                                                       int32_t* __restrict__ which, uint64_t* __restrict__ vsrc,
                                                       uint64_t* __restrict__ dlen, uint64_t* __restrict__ tsum,
                                                       WideScreen ws, const DirMap* __restrict__ maps) {
  const uint64_t k = (uint64_t)blockIdx.x * kWideNT + threadIdx.x;
  const bool live = k < n;
  const Query q = make_query<KEYK>(ks, live ? k : 0);
  uint64_t pa = 0, pb = 0;
  if (live) key_positions<KEYK, MODE>(ks, k, mp, pa, pb);
  const uint64_t* ra = set + pa * R;
  const uint64_t* rb = set + pb * R;
  // the screen row of this key's bucket and fingerprint bin: one R-word row
  // says, for every slot at once, whether the summary word could pass
  const uint64_t* rs = ws.scr ? ws.scr + ((bkt_index(q.w0, ws.bits) << ws.hbits) +
                                          (bkt_fp(q.w0) & ((1u << ws.hbits) - 1u))) * R
                              : nullptr;
  const uint32_t kw[4] = {(uint32_t)(q.w0 >> 32), (uint32_t)q.w0, (uint32_t)(q.w1 >> 32), (uint32_t)q.w1};
  // The block walks the groups together: each group's 64 views and DirMaps
  // are staged in LDS once for the block (every search then reads its
  // table's view and map from LDS, not 56 + 320 B from global memory per
  // search), and the walk ends when no lane of the block is still looking.
  // The maps come from the table list's contiguous copy (maps, round 6) in
  // the same pass as the views, one barrier per group; without it each map
  // is found through its view (a second pass after the views' barrier).
  __shared__ TableView stv[64];
  __shared__ DirMap sdm[64];
  __shared__ WideGroup sg[kWideMax / 64];
  const uint32_t ng = (nt + 63) / 64;
  for (uint32_t i = threadIdx.x; i < ng; i += kWideNT) sg[i] = groups[i];
  __syncthreads();
  int32_t w = -1;
  uint64_t src = 0, d = 0;
  bool active = live;
  for (uint32_t g = 0; g < ng; ++g) {
    if (!__syncthreads_or(active)) break;  // (also: the previous group's stage is consumed)
    const uint32_t t0 = 64 * g, gn = nt - t0 < 64 ? nt - t0 : 64;
    // the group's views through registers, like the narrow kernels' (a
    // thread's two dwords in flight together: k_wide_get_many 83.7-84.4
    // against 88.0-88.8 us for a load-and-store loop, 300 tables of m = 1024,
    // alternating on one box)
    store_views(load_views<kWideNT>(tv + t0, gn), gn, stv);
    if (maps) {
      const uint4* ms = reinterpret_cast<const uint4*>(maps + t0);
      uint4* md = reinterpret_cast<uint4*>(sdm);
      for (uint32_t i = threadIdx.x; i < gn * kMapWords; i += kWideNT) md[i] = ms[i];
      __syncthreads();
    } else {
      __syncthreads();
      stage_maps<kWideNT>(stv, gn, sdm);
    }
    if (!active) continue;
    const WideGroup gd = sg[g];
    const uint64_t gmask = gd.gn >= 64 ? ~0ull : ((1ull << gd.gn) - 1);
    // The group's row windows one after another, each only when it can
    // matter: row b where row a's window has bits (src/bloom.rs:50's &&),
    // the screen where both do. Loading the three together, with the next
    // group's in flight during this group's walk, measured slower (round 6:
    // 93.9-94.2 against 92.1-92.3 us one lane, 3.07 against 3.29 G gets/s
    // on three lanes) and cost ~2 more L2 requests per lookup: a lane found
    // in this group had already loaded the next group's three windows.
    uint64_t ca = 0, cb = 0, cs = ~0ull;
    if (gd.kind != 2) {
      ca = wide_window(ra, R, gd.lo) & gmask;
      cb = ca ? wide_window(rb, R, gd.lo) : 0ull;
      cs = (ca & cb) && rs ? wide_window(rs, R, gd.lo) : ~0ull;
    }
    uint64_t cand = 0;
    if (gd.kind == 2) {  // scattered slots: one bit per table
      for (uint32_t i = 0; i < gd.gn; ++i) {
        const uint32_t s = slots[t0 + i];
        if ((ra[s >> 6] >> (s & 63)) & 1ull) cand |= ((rb[s >> 6] >> (s & 63)) & 1ull) << i;
      }
    } else {
      const uint64_t a = ca & gmask;
      cand = a ? (a & cb) : 0ull;  // src/bloom.rs:50's &&
      cand &= cs;                  // the screen (slot order, like the rows; all ones without one)
      if (gd.kind == 1 && cand) cand = __builtin_bitreverse64(cand) >> (64 - gd.gn);  // bit gn-1-i -> i
    }
    if (gd.kind == 2 && cand && rs) {
      uint64_t sc = 0;
      for (uint32_t i = 0; i < gd.gn; ++i) {
        const uint32_t s = slots[t0 + i];
        sc |= ((rs[s >> 6] >> (s & 63)) & 1ull) << i;
      }
      cand &= sc;
    }
    // the candidates newest first, the group's views and maps from LDS. At
    // the product's m = 1024 most candidates are false positives (~3/4 of
    // the tables pass the Bloom gate); each is settled by its key bucket's
    // 8-byte summary word (sstable.hpp bkt_fp), which stays in the L2s,
    // before any bucket line is read (a complete bucket without the key's
    // fingerprint: Ok(None)). Loading the words of 2 or 4 candidates at once
    // measured the same (profiles/wide_summary_r04.json).
    // The zone gate (src/sstable.rs:138) is checked after the summary word:
    // both only answer Ok(None), so their order leaves the walk's result as
    // it is, and the summary word settles nearly every candidate first.
    const uint32_t kfp = bkt_fp(q.w0);
    while (cand) {
      // screen the next kScreen candidates by their summary words, the
      // loads in flight together (one L2 round trip per kScreen candidates,
      // not per candidate); ~0: no summary word, no proof
      uint64_t taken = 0, keep = 0;
      {
        uint32_t ii[kScreen];
        uint64_t sw[kScreen];
        uint64_t c = cand;
#pragma unroll
        for (uint32_t j = 0; j < kScreen; ++j) {
          ii[j] = c ? (uint32_t)__builtin_ctzll(c) : 64u;
          c &= c - 1;
        }
#pragma unroll
        for (uint32_t j = 0; j < kScreen; ++j) {
          sw[j] = ~0ull;
          if (ii[j] < 64u) {
            const TableView& v = stv[ii[j]];
            if (v.bkt && v.fast()) {
              const uint32_t bits = v.bkbits();
              sw[j] = g64(v.bkt, (1ull << bits) * kBktWords + bkt_index(q.w0, bits));
            }
          }
        }
#pragma unroll
        for (uint32_t j = 0; j < kScreen; ++j) {
          if (ii[j] >= 64u) continue;
          taken |= 1ull << ii[j];
          const uint32_t nst = (uint32_t)(sw[j] & 15u);
          bool pass = nst > kBktSlots;  // not complete: the search decides
#pragma unroll
          for (uint32_t s = 0; s < kBktSlots; ++s)
            pass |= s < nst && (uint32_t)((sw[j] >> (4 + 15 * s)) & 0x7FFFu) == kfp;
          if (pass) keep |= 1ull << ii[j];  // else Ok(None)
        }
      }
      cand &= ~taken;
      bool found = false;
      while (keep) {  // the survivors, newest first
        const uint32_t i = (uint32_t)__builtin_ctzll(keep);
        keep &= keep - 1;
        if (z.any) {
          const uint32_t s = gd.kind == 2 ? slots[t0 + i] : gd.kind == 1 ? gd.lo + gd.gn - 1 - i : gd.lo + i;
          if (!wide_zone_ok<KEYK>(z, s, kw, q.p, q.len)) continue;  // Ok(None)
        }
        if (!table_answers(stv[i], &sdm[i], t0 + i, q, w, src, d)) continue;
        found = true;
        break;
      }
      if (found) {
        active = false;
        break;
      }
    }
  }
  constexpr uint32_t T = kWideNT / kNT;  // 256-key tiles per workgroup
  __shared__ uint64_t bnd[T + 1];
  if (live) put_answer(k, w, src, d, which, vsrc, dlen);
  tile_sums<kWideNT>(d, n, tsum, bnd);
}

}  // namespace

hipError_t launch_wide_get_many(int keyk, int mode, uint32_t R, const uint64_t* set, const ModP& mp,
                                const WideZone* zones, const TableView* tv, uint32_t nt, const WideGroup* groups,
                                const uint32_t* slots, const KeySrc& ks, uint64_t n, int32_t* which,
                                uint64_t* vsrc, uint64_t* dlen, uint64_t* tsum, hipStream_t s,
                                const WideScreen* screen, const DirMap* maps) {
  if (!n) return hipSuccess;
  if (!nt || nt > 64 * R || R > kWideMax / 64) return hipErrorInvalidValue;
  const WideZone z = zones ? *zones : WideZone{nullptr, nullptr, nullptr, nullptr, 0};
  const WideScreen sc = screen ? *screen : WideScreen{nullptr, 0, 0, 0};
  const dim3 g(blocks_for(n, kWideNT));
  ProfScope ps("k_wide_get_many", s);
  CB_KEY_MODE_DISPATCH(keyk, mode,
                       hipLaunchKernelGGL((k_wide_get_many<KK, MM>), g, dim3(kWideNT), 0, s, set, R, mp, z, tv, nt,
                                          groups, slots, ks, n, which, vsrc, dlen, tsum, sc, maps));
  return hipGetLastError();
}

}  // namespace cb
