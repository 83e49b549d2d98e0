// scan.hip — the kernels of cb_tables_scan (scan.hpp): cut every table to
// the range, hand the cuts to compaction's merge as its sources, and emit the
// survivors' keys, sources and value spans.
//
//   k_scan_bounds — sixteen lanes per (range, table, bound): the lower bound
//       of the bound's zero-padded 8-byte prefix down the table's fence levels, each
//       level one run of at most 16 entries read by the sixteen lanes at once
//       (one 128-B line, one round trip per level where a bisection takes
//       four), then the lines that share the prefix by record compares, again
//       sixteen probes a round. A lower-bound search: it never asks whether
//       the bound is a key of the table. Each search is a short chain of
//       dependent loads and all run side by side (two per table and range),
//       so the kernel is as long as one table's descent.
//   k_scan_sources — one block: the scan of the cuts' lengths, the non-empty
//       cuts packed as CompactSrc entries (rec + first, llen + first), each
//       with its table's place in the caller's list and its range.
//   k_scan_emit — one block per tile of sorted records, as k_compact_format:
//       the survivors' ranks and key offsets from the scanned tile sums and a
//       block scan, the tile's key bytes assembled into aligned dwords
//       (compaction's copier, copy_tile_bytes of compact.hpp), and
//       per survivor its key offset, source and value span. A tile's
//       survivors lie in at most two of the decode's tiles, so the block adds
//       two partial sums of their decoded lengths. For a scan of many ranges
//       it also writes each survivor's range.
//   k_scan_range_off — one lane per range: where its entries begin, the lower
//       bound of its number in the survivors' ranges (they ascend with the keys).
//   k_scan_count — cb_tables_count's tail, in place of the emit and all after
//       it: one block per tile of sorted records, the survivors and the live
//       ones (liverow.hpp) summed per run of equal ranges and added to the
//       ranges' counters (count_runs, the tail it shares with
//       k_scan_count_where). No key is copied and no value read.
//   k_scan_ts — cb_scan_ts: one lane per entry of a finished result, its
//       timestamp from its decoded value's first 8 bytes (rowts.hpp).
//   k_scan_count_where — cb_tables_count_where's tail, k_scan_count's shape
//       with a third sum: a lane whose record is a live survivor runs the row
//       rule (rowjson.hpp) over its line, the key in place and the value's
//       base64 text decoded on the fly, one aligned dword per three bytes.
//       One lane per row: a tile takes as long as its longest payload.
//   k_scan_match — cb_scan_match: one lane per entry of a finished result,
//       the same rule over its key and its decoded value.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "launch.hpp"
#include "liverow.hpp"
#include "profile.hpp"
#include "rowjson.hpp"
#include "rowts.hpp"
#include "scan.hpp"
#include "tablesearch.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;
constexpr uint32_t kGroup = 16;  // lanes per search
static_assert(kGroup == kFanout, "a group reads one run of a fence level at once");
static_assert(kCompactTile == kNT && kDecodeTile == kNT, "k_scan_emit's tiles");

// How many lanes of this lane's group hold pred (every lane of the group
// calls it together; other groups of the wave may be elsewhere).
__device__ __forceinline__ uint32_t group_count(bool pred) {
  const uint64_t b = __ballot(pred);
  return (uint32_t)__builtin_popcount((uint32_t)(b >> (threadIdx.x & 48u)) & 0xFFFFu);
}

// The first i in [lo, hi) for which below(i) is false, or hi (below is true
// on a prefix of the range): sixteen evenly spaced probes a round, so a run of
// at most 16 takes one round.
template <class Below>
__device__ __forceinline__ uint64_t group_lower_bound(uint64_t lo, uint64_t hi, uint32_t sub, Below below) {
  while (lo < hi) {  // (the same for every lane of the group)
    const uint64_t step = (hi - lo + kGroup - 1) / kGroup;
    const uint64_t p = lo + sub * step;
    const uint32_t c = group_count(p < hi && below(p));
    if (!c) break;
    // probes 0..c-1 are below, probe c is not (or lies past hi)
    const uint64_t nhi = lo + c * step < hi ? lo + c * step : hi;
    lo += (c - 1) * step + 1;
    hi = nhi;
  }
  return lo;
}

// The first entry of level 0 (pfx) that is >= x (strict) or > x, down the levels.
__device__ __forceinline__ uint64_t group_descend(const TableView& v, uint64_t x, bool strict, uint32_t sub) {
  uint32_t j = v.nlev();
  uint64_t lo = 0, hi = level_count(v.nlines(), j);
  for (;; --j) {
    const uint64_t* a = level_array(v, j);
    const uint64_t i = group_lower_bound(lo, hi, sub, [&](uint64_t p) {
      const uint64_t e = g64(a, p);
      return strict ? e < x : e <= x;
    });
    if (!j) return i;
    level_down(v, j, i, lo, hi);
  }
}

// The first line of v whose key is >= q.
__device__ __forceinline__ uint64_t group_bound(const TableView& v, const Query& q, uint32_t sub) {
  const uint64_t nl = v.nlines();
  const uint64_t i0 = group_descend(v, q.w0, true, sub);
  // the lines from i0 on that share q's prefix: the next 16 prefixes, and a
  // second descent only when they all do
  const uint32_t c = group_count(i0 + sub < nl && g64(v.pfx, i0 + sub) == q.w0);
  if (!c) return i0;
  uint64_t e = i0 + c;
  if (c == kGroup && e < nl) e = group_descend(v, q.w0, false, sub);
  return group_lower_bound(i0, e, sub, [&](uint64_t l) { return rec_cmp(v, grec(v.rec, l), q) < 0; });
}

__global__ __launch_bounds__(kNT) void k_scan_bounds(const ScanTable* __restrict__ tab, uint32_t nt,
                                                     const ScanRange* __restrict__ rng, uint32_t nr,
                                                     const uint8_t* __restrict__ bytes, ScanCut* __restrict__ cut) {
  const uint32_t sub = threadIdx.x & (kGroup - 1);
  // search 2 c: cut c's lo, 2 c + 1: its hi (adjacent groups of one wave);
  // cut c = r * nt + t: range r of table t
  const uint64_t nq = 2ull * nt * nr;
  uint64_t g = ((uint64_t)blockIdx.x * kNT + threadIdx.x) / kGroup;
  const bool live = g < nq;
  if (!live) g = nq - 1;  // (the last groups repeat the last search: every lane stays in step)
  const uint64_t c_at = g >> 1;
  const uint32_t t = (uint32_t)(c_at % nt);
  const bool upper = g & 1;
  const ScanTable st = tab[t];
  const ScanRange range = rng[c_at / nt];
  const TableView v =
      make_view(st.data, st.rec, st.pfx, st.fence, st.nlines, fence_levels(st.nlines), true, nullptr, nullptr);
  Query q;
  q.p = bytes + (upper ? range.hi_at : range.lo_at);
  q.len = upper ? range.hi_len : range.lo_len;
  q.w0 = be_chunk(q.p, q.len < 8 ? q.len : 8);
  q.w1 = q.len > 8 ? be_chunk(q.p + 8, q.len - 8 < 8 ? q.len - 8 : 8) : 0;
  unsigned long long b = st.nlines;
  if (!upper || range.has_hi) b = group_bound(v, q, sub);
  const unsigned long long hi_b = __shfl_down(b, kGroup, 64);  // the table's hi search: the next group
  if (live && !upper && sub == 0) {
    ScanCut c;
    c.first = b;
    c.last = hi_b > b ? hi_b : b;  // lo >= hi: an empty cut
    const uint64_t end = c.last < st.nlines ? grec(st.rec, c.last).start : st.len;
    c.bytes = c.last > c.first ? end - grec(st.rec, c.first).start : 0;
    cut[c_at] = c;
  }
}

__global__ __launch_bounds__(kNT) void k_scan_sources(const ScanTable* __restrict__ tab,
                                                      const ScanCut* __restrict__ cut, uint32_t nt, uint32_t nr,
                                                      CompactSrc* __restrict__ src, uint32_t* __restrict__ src_tab,
                                                      uint32_t* __restrict__ src_rng,
                                                      uint64_t* __restrict__ totals) {
  const uint32_t ncut = nt * nr;  // (the host caps the cuts of a call)
  uint64_t base = 0, bytes = 0, ns = 0;
  for (uint32_t c0 = 0; c0 < ncut; c0 += kNT) {
    const uint32_t ci = c0 + threadIdx.x;
    ScanCut c{0, 0, 0};
    if (ci < ncut) c = cut[ci];
    const uint64_t len = c.last - c.first;
    uint64_t tl, tn, tb, unused;
    const uint64_t off = block_scan<(int)kNT>(len, &tl);
    const uint64_t si = block_scan_sum2<(int)kNT>(len ? 1 : 0, c.bytes, 0, &tn, &tb, &unused);
    if (len) {
      const ScanTable st = tab[ci % nt];
      src[ns + si] = CompactSrc{st.data, st.rec + c.first, st.llen + c.first, base + off};
      src_tab[ns + si] = st.index;
      src_rng[ns + si] = ci / nt;
    }
    base += tl;
    bytes += tb;
    ns += tn;
  }
  if (threadIdx.x == 0) {
    totals[0] = base;
    totals[1] = bytes;
    totals[2] = ns;
  }
}

__global__ __launch_bounds__(kNT) void k_scan_emit(const SortKey* __restrict__ order,
                                                   const CompactSide* __restrict__ side,
                                                   const uint64_t* __restrict__ slen,
                                                   const uint64_t* __restrict__ tcnt,
                                                   const uint64_t* __restrict__ tkeys,
                                                   const uint64_t* __restrict__ totals,
                                                   const CompactSrc* __restrict__ src,
                                                   const uint32_t* __restrict__ src_tab,
                                                   const uint32_t* __restrict__ src_rng, uint32_t nsrc, uint64_t n,
                                                   uint64_t count, uint8_t* __restrict__ keys,
                                                   uint64_t* __restrict__ key_off, int32_t* __restrict__ which,
                                                   uint32_t* __restrict__ rid, uint64_t* __restrict__ vsrc,
                                                   uint64_t* __restrict__ dlen,
                                                   uint64_t* __restrict__ vsum) {
  __shared__ uint64_t s_off[kNT + 1];    // survivor i's first key byte in the tile
  __shared__ const uint8_t* s_src[kNT];  // its key
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const bool live = p < n && slen[p] != 0;
  CompactSide sd{};
  uint32_t g = 0;
  if (live) {
    g = order[p].idx;
    sd = side[g];
  }
  const uint64_t r0 = tcnt[blockIdx.x];  // the tile's first rank
  uint64_t tc, tk;
  const uint64_t ci = block_scan<(int)kNT>(live ? 1 : 0, &tc);
  const uint64_t kof = block_scan<(int)kNT>(live ? sd.klen : 0, &tk);
  const uint64_t r = r0 + ci;
  const bool out = live && r < count;
  // the decode's tile sums: ranks r0 .. r0 + tc lie in tile r0 / 256 and the next
  const uint64_t split = (r0 / kDecodeTile + 1) * kDecodeTile;
  uint64_t unused, va, vb;
  (void)block_scan_sum2<(int)kNT>(0, out && r < split ? sd.vdl : 0, out && r >= split ? sd.vdl : 0, &unused, &va,
                                  &vb);
  if (threadIdx.x == 0) {
    if (va) atomicAdd((unsigned long long*)(vsum + r0 / kDecodeTile), (unsigned long long)va);
    if (vb) atomicAdd((unsigned long long*)(vsum + r0 / kDecodeTile + 1), (unsigned long long)vb);
    if (blockIdx.x == 0 && count == totals[0]) key_off[count] = totals[2];  // no limit cut: the end of all keys
  }
  if (live) {
    s_off[ci] = kof;
    s_src[ci] = sd.src;
    // (rank == count: the first survivor past the limit, whose key offset is the end of the kept keys)
    if (r <= count) key_off[r] = tkeys[blockIdx.x] + kof;
  }
  if (out) {
    const uint32_t si = src_of(src, nsrc, g);
    which[r] = (int32_t)src_tab[si];
    if (rid) rid[r] = src_rng[si];  // (uniform: a scan of many ranges)
    vsrc[r] = (uint64_t)(uintptr_t)(sd.src + sd.klen + 1);
    dlen[r] = sd.vdl;
  }
  if (threadIdx.x == 0) s_off[tc] = tk;
  __syncthreads();
  const uint32_t nsv = r0 >= count ? 0u : (uint32_t)(count - r0 < tc ? count - r0 : tc);  // survivors under the limit
  if (!nsv) return;  // (uniform)
  // the tile's keys back to back (an empty key owns no byte)
  const uint64_t tl = s_off[nsv];
  copy_tile_bytes(keys + tkeys[blockIdx.x], tl, nsv, s_off,
                  [&](uint32_t i, uint64_t j) -> uint32_t { return s_src[i][j - s_off[i]]; });
}

// One lane per r in [0, nr]: the first entry of the non-decreasing rid[0..count)
// that is >= r.
__global__ __launch_bounds__(kNT) void k_scan_range_off(const uint32_t* __restrict__ rid, uint64_t count, uint32_t nr,
                                                        uint64_t* __restrict__ range_off) {
  const uint64_t r = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (r > nr) return;
  uint64_t lo = 0, hi = count;  // rid[i] < r for i < lo, rid[i] >= r for i >= hi
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (rid[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  range_off[r] = lo;
}

constexpr uint32_t kPast = 0xFFFFFFFFu;  // the range of a lane past the last record (nr - 1 is below it)

// The tail of both counting kernels, called by every lane of the block with
// its record's range (kPast: no record) and its flags, Fields of them packed
// Field bits apart (none passes 256). One block scan of the packed word, then
// each lane that ends a run of equal ranges adds the run's sums to its
// range's counters cnt[Fields rid ..]: as many atomics as the tile holds
// ranges with an entry, times the fields that are not zero.
template <uint32_t Field, uint32_t Fields>
__device__ __forceinline__ void count_runs(uint64_t p, uint64_t n, uint32_t rid, uint64_t v, uint32_t nr,
                                           uint64_t* __restrict__ cnt) {
  static_assert(Field >= 9 && Field * Fields <= 64, "a tile's sums fit their fields");
  __shared__ uint32_t s_rid[kNT + 1];
  __shared__ uint64_t s_inc[kNT];  // the inclusive scan of the packed flags
  const uint32_t t = threadIdx.x;
  uint64_t total;
  const uint64_t inc = block_scan<(int)kNT>(v, &total) + v;
  s_rid[t] = rid;
  s_inc[t] = inc;
  if (t == 0) s_rid[kNT] = kPast;
  __syncthreads();
  if (p >= n || s_rid[t + 1] == rid || rid >= nr) return;  // not the end of a run
  // the run's first lane: the first of the tile with this range
  uint32_t lo = 0, hi = t;  // s_rid[i] < rid for i < lo, s_rid[hi] == rid
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_rid[mid] < rid) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t sum = inc - (lo ? s_inc[lo - 1] : 0);
#pragma unroll
  for (uint32_t k = 0; k < Fields; ++k) {
    uint64_t f = sum >> k * Field;
    if (k + 1 < Fields) f &= (1ull << Field) - 1;
    if (f) atomicAdd((unsigned long long*)(cnt + (uint64_t)Fields * rid + k), (unsigned long long)f);
  }
}

// One block per tile of sorted records, after the plain select. Every record,
// survivor or not, has its source's range, and the ranges do not decrease
// along the sorted order, so a tile is a few runs of equal ranges. Two flags
// per lane (survivor in the low word, survivor and not dead in the high one)
// summed per run by count_runs.
__global__ __launch_bounds__(kNT) void k_scan_count(const SortKey* __restrict__ order,
                                                    const CompactSide* __restrict__ side,
                                                    const uint64_t* __restrict__ slen,
                                                    const CompactSrc* __restrict__ src,
                                                    const uint32_t* __restrict__ src_rng, uint32_t nsrc, uint64_t n,
                                                    uint32_t nr, uint64_t* __restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  uint32_t rid = kPast;
  uint64_t v = 0;
  if (p < n) {
    const uint32_t g = order[p].idx;
    rid = nr > 1 ? src_rng[src_of(src, nsrc, g)] : 0;  // (uniform)
    if (slen[p]) v = value_dead(side[g].vdl) ? 1ull : 1ull | 1ull << 32;
  }
  count_runs<32, 2>(p, n, rid, v, nr, cnt);
}

__global__ __launch_bounds__(kNT) void k_scan_ts(const uint64_t* __restrict__ val_off,
                                                 const uint8_t* __restrict__ vals, uint64_t count,
                                                 uint64_t* __restrict__ ts) {
  const uint64_t i = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (i >= count) return;
  const uint64_t o = val_off[i];
  ts[i] = decoded_ts(vals + o, val_off[i + 1] - o);
}

// Four characters of a value's text in a table's file by aligned dword
// loads (rowjson.hpp's Text policy): the text starts anywhere, so a quantum
// straddles two dwords, and the second is kept for the next quantum. The
// dword after the last character lies in the file's 16 bytes of slack at the
// latest, the one before the first in the line itself.
struct TextByDwords {
  const uint32_t* wp;
  uint32_t sh, cw;
  uint64_t cq;
  __device__ explicit TextByDwords(const uint8_t* t)
      : wp(reinterpret_cast<const uint32_t*>(t - ((uintptr_t)t & 3))), sh(8 * (uint32_t)((uintptr_t)t & 3)), cw(0), cq(~0ull) {}
  __device__ uint32_t quad(uint64_t q) {
    const uint32_t lo = q == cq ? cw : wp[q];
    if (!sh) return lo;
    const uint32_t hi = wp[q + 1];
    cq = q + 1;
    cw = hi;
    return lo >> sh | hi << (32 - sh);
  }
};

// k_scan_count with the matched rows beside the entries and the live ones:
// three flags packed 21 bits apart (none passes 256), cnt[3 r ..] = {entries,
// live, matched} of range r. Every lane reaches the block scan; only the
// lanes of live survivors read their lines.
__global__ __launch_bounds__(kNT) void k_scan_count_where(const SortKey* __restrict__ order,
                                                          const CompactSide* __restrict__ side,
                                                          const uint64_t* __restrict__ slen,
                                                          const CompactSrc* __restrict__ src,
                                                          const uint32_t* __restrict__ src_rng, uint32_t nsrc,
                                                          uint64_t n, uint32_t nr, const WherePred* __restrict__ w,
                                                          const uint32_t* __restrict__ skip,
                                                          uint64_t* __restrict__ cnt) {
  constexpr uint32_t kField = 21;
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  uint32_t rid = kPast;
  uint64_t v = 0;
  if (p < n) {
    const uint32_t g = order[p].idx;
    rid = nr > 1 ? src_rng[src_of(src, nsrc, g)] : 0;  // (uniform)
    if (slen[p]) {
      const CompactSide sd = side[g];
      v = 1;
      if (!value_dead(sd.vdl)) {
        v |= 1ull << kField;
        B64Bytes<TextByDwords> value(TextByDwords(sd.src + sd.klen + 1), sd.vdl);
        if (row_matches(*w, sd.src, sd.klen, skip && rid < nr ? skip[rid] : 0u, value)) v |= 1ull << 2 * kField;
      }
    }
  }
  count_runs<kField, 3>(p, n, rid, v, nr, cnt);
}

__global__ __launch_bounds__(kNT) void k_scan_match(const uint64_t* __restrict__ key_off,
                                                    const uint8_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ val_off,
                                                    const uint8_t* __restrict__ vals, uint64_t count,
                                                    const uint64_t* __restrict__ range_off,
                                                    const uint32_t* __restrict__ skip, uint32_t nr,
                                                    const WherePred* __restrict__ w, uint8_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (i >= count) return;
  uint32_t sk = 0;
  if (skip) sk = skip[last_le(nr, i, [&](uint32_t r) { return range_off[r]; })];  // the entry's range (range_off[0] = 0)
  const uint64_t ko = key_off[i], vo = val_off[i];
  DecodedBytes value(vals + vo, val_off[i + 1] - vo);
  flags[i] = row_matches(*w, keys + ko, key_off[i + 1] - ko, sk, value) ? 1 : 0;
}

}  // namespace

hipError_t launch_scan_bounds(const ScanTable* tab, uint32_t nt, const ScanRange* rng, uint32_t nr,
                              const uint8_t* bytes, ScanCut* cut, hipStream_t s) {
  if (!nt || !nr) return hipSuccess;
  ProfScope ps("k_scan_bounds", s);
  hipLaunchKernelGGL(k_scan_bounds, dim3(blocks_for(2ull * nt * nr * kGroup, kNT)), dim3(kNT), 0, s, tab, nt, rng, nr,
                     bytes, cut);
  return hipGetLastError();
}

hipError_t launch_scan_sources(const ScanTable* tab, const ScanCut* cut, uint32_t nt, uint32_t nr, CompactSrc* src,
                               uint32_t* src_tab, uint32_t* src_rng, uint64_t* totals, hipStream_t s) {
  ProfScope ps("k_scan_sources", s);
  hipLaunchKernelGGL(k_scan_sources, dim3(1), dim3(kNT), 0, s, tab, cut, nt, nr, src, src_tab, src_rng, totals);
  return hipGetLastError();
}

hipError_t launch_scan_emit(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                            const uint64_t* tcnt, const uint64_t* tkeys, const uint64_t* totals,
                            const CompactSrc* src, const uint32_t* src_tab, const uint32_t* src_rng, uint32_t nsrc,
                            uint64_t n, uint64_t count, uint8_t* keys, uint64_t* key_off, int32_t* which,
                            uint32_t* rid, uint64_t* vsrc, uint64_t* dlen, uint64_t* vsum, hipStream_t s) {
  if (!n || !count) return hipSuccess;
  ProfScope ps("k_scan_emit", s);
  hipLaunchKernelGGL(k_scan_emit, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, tcnt, tkeys, totals,
                     src, src_tab, src_rng, nsrc, n, count, keys, key_off, which, rid, vsrc, dlen, vsum);
  return hipGetLastError();
}

hipError_t launch_scan_count(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                             const CompactSrc* src, const uint32_t* src_rng, uint32_t nsrc, uint64_t n, uint32_t nr,
                             uint64_t* cnt, hipStream_t s) {
  if (!n || !nr) return hipSuccess;
  ProfScope ps("k_scan_count", s);
  hipLaunchKernelGGL(k_scan_count, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, src, src_rng, nsrc,
                     n, nr, cnt);
  return hipGetLastError();
}

hipError_t launch_scan_ts(const uint64_t* val_off, const uint8_t* vals, uint64_t count, uint64_t* ts, hipStream_t s) {
  if (!count) return hipSuccess;
  ProfScope ps("k_scan_ts", s);
  hipLaunchKernelGGL(k_scan_ts, dim3(blocks_for(count, kNT)), dim3(kNT), 0, s, val_off, vals, count, ts);
  return hipGetLastError();
}

hipError_t launch_scan_count_where(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                                   const CompactSrc* src, const uint32_t* src_rng, uint32_t nsrc, uint64_t n,
                                   uint32_t nr, const WherePred* w, const uint32_t* skip, uint64_t* cnt,
                                   hipStream_t s) {
  if (!n || !nr) return hipSuccess;
  ProfScope ps("k_scan_count_where", s);
  hipLaunchKernelGGL(k_scan_count_where, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, src, src_rng,
                     nsrc, n, nr, w, skip, cnt);
  return hipGetLastError();
}

hipError_t launch_scan_match(const uint64_t* key_off, const uint8_t* keys, const uint64_t* val_off,
                             const uint8_t* vals, uint64_t count, const uint64_t* range_off, const uint32_t* skip,
                             uint32_t nr, const WherePred* w, uint8_t* flags, hipStream_t s) {
  if (!count) return hipSuccess;
  ProfScope ps("k_scan_match", s);
  hipLaunchKernelGGL(k_scan_match, dim3(blocks_for(count, kNT)), dim3(kNT), 0, s, key_off, keys, val_off, vals, count,
                     range_off, skip, nr, w, flags);
  return hipGetLastError();
}

hipError_t launch_scan_range_off(const uint32_t* rid, uint64_t count, uint32_t nr, uint64_t* range_off, hipStream_t s) {
  ProfScope ps("k_scan_range_off", s);
  hipLaunchKernelGGL(k_scan_range_off, dim3(blocks_for((uint64_t)nr + 1, kNT)), dim3(kNT), 0, s, rid, count, nr,
                     range_off);
  return hipGetLastError();
}

}  // namespace cb
