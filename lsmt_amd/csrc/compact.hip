// compact.hip — the kernels of cb_tables_compact (compact.hpp): gather the
// input tables' keys into one batch, (the existing stable sort orders it),
// select each key's newest decodable line, and write the merged file.
//
//   k_compact_klen / k_compact_gather — one lane per input line, all tables
//       in one launch: the line's table is found by a binary search of the
//       sources' line bases (a few hundred entries, L2-resident), its key
//       copied to its scanned slot of the batch and its side record written.
//   k_compact_select — one lane per sorted record. The sort's order is strict
//       with the input index last, so the lines of one key are adjacent,
//       newest first. A record survives when its value decodes and no earlier
//       record of its run does: one compare with the predecessor in the
//       common case; only a run with spoiled values walks further back. The
//       walk reads global memory only, so a run may cross wave, block and
//       tile edges freely. Each block leaves three tile sums. Its DropDead
//       variant (the live-row entries) also drops a survivor whose own value
//       is a tombstone (liverow.hpp); the walk is the same, so a tombstone
//       still defeats the older lines of its key before it is dropped.
//   k_compact_ts, k_compact_lww_runs, k_compact_lww_tiles — the select of the
//       LWW entries in k_compact_select's place (rowts.hpp): every line's
//       timestamp from its value's text, then per run of equal keys the
//       decodable line with the greatest timestamp (the run's head lane walks
//       it once), then the tile sums. Launched for LWW merges only.
//   k_compact_format — one block per tile: the survivors' offsets from the
//       scanned tile sums and a block scan, then the block copies the tile's
//       bytes together (copy_tile_bytes, compact.hpp: the scan's emit copies
//       its keys the same way), aligned dwords of the output assembled from
//       the source lines (a line is `key \t text` in its input file already, so
//       only the '\n' is new). Each survivor also writes its entry of the
//       line index (LineRec with vdl carried over, pfx, the fence levels,
//       llen: the file is never re-read) and packs its key for the Bloom
//       build and the zone bounds. The directory follows from pfx
//       (k_pfx_masks, k_table_dir), as for a file indexed by cb_table_create.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "compact.hpp"
#include "launch.hpp"
#include "liverow.hpp"
#include "profile.hpp"
#include "rowts.hpp"
#include "zone.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = kCompactTile;

__global__ __launch_bounds__(kNT) void k_compact_klen(const CompactSrc* __restrict__ src, uint32_t nsrc, uint64_t n,
                                                      uint64_t* __restrict__ klen) {
  const uint64_t g = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (g >= n) return;
  const CompactSrc t = src[src_of(src, nsrc, g)];
  klen[g] = t.rec[g - t.base].klen;
}

__global__ __launch_bounds__(kNT) void k_compact_gather(const CompactSrc* __restrict__ src, uint32_t nsrc, uint64_t n,
                                                        const uint64_t* __restrict__ ko, uint8_t* __restrict__ kb,
                                                        CompactSide* __restrict__ side,
                                                        uint64_t* __restrict__ dmask) {
  // (whole blocks: the first kSampleBlocks of them)
  sample_pfx_masks(n, [&](uint64_t q) {
    const CompactSrc t = src[src_of(src, nsrc, q)];
    return t.rec[q - t.base].pfx0;
  }, dmask);
  const uint64_t g = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (g >= n) return;
  const CompactSrc t = src[src_of(src, nsrc, g)];
  const uint64_t l = g - t.base;
  const LineRec r = t.rec[l];
  CompactSide sd;
  sd.src = t.data + r.start;
  sd.llen = t.llen[l];
  sd.klen = r.klen;
  sd.vdl = r.vdl;
  sd.pad = 0;
  side[g] = sd;
  uint8_t* dst = kb + ko[g];
  for (uint32_t j = 0; j < r.klen; ++j) dst[j] = sd.src[j];
}

// Whether two sort records name the same key (their first 16 bytes and
// lengths from the records, the rest from the batch).
__device__ __forceinline__ bool same_key(const SortKey& a, const SortKey& b, const uint8_t* kb, const uint64_t* ko) {
  if (a.w0 != b.w0 || a.w1 != b.w1 || a.len != b.len) return false;
  if (a.len <= 16) return true;
  return bytes_cmp(kb + ko[a.idx] + 16, a.len - 16, kb + ko[b.idx] + 16, b.len - 16) == 0;
}

// A tile's three sums from its lanes' line lengths (0: not a survivor) and key
// lengths: the survivors, their line bytes and their key bytes. Contains
// barriers: every lane of the block calls it.
__device__ __forceinline__ void put_tile_sums(uint64_t len, uint64_t kl, uint64_t* __restrict__ tcnt,
                                              uint64_t* __restrict__ tbytes, uint64_t* __restrict__ tkeys) {
  uint64_t tc, tl, tk;
  (void)block_scan_sum2<(int)kNT>(len ? 1 : 0, len, kl, &tc, &tl, &tk);
  if (threadIdx.x == 0) {
    tcnt[blockIdx.x] = tc;
    tbytes[blockIdx.x] = tl;
    tkeys[blockIdx.x] = tk;
  }
}

template <bool DropDead>
__global__ __launch_bounds__(kNT) void k_compact_select(const SortKey* __restrict__ order,
                                                        const CompactSide* __restrict__ side,
                                                        const uint8_t* __restrict__ kb,
                                                        const uint64_t* __restrict__ ko, uint64_t n,
                                                        uint64_t* __restrict__ slen, uint64_t* __restrict__ tcnt,
                                                        uint64_t* __restrict__ tbytes,
                                                        uint64_t* __restrict__ tkeys) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  uint64_t len = 0, kl = 0;
  if (p < n) {
    const SortKey a = order[p];
    const CompactSide sa = side[a.idx];
    // (DropDead is a compile-time constant: the plain kernel has no such test)
    if (sa.vdl != kBadValue && !(DropDead && value_dead(sa.vdl))) {
      bool keep = true;
      for (uint64_t q = p; q-- > 0;) {  // the newer lines of the same key, dead or not
        const SortKey b = order[q];
        if (!same_key(a, b, kb, ko)) break;
        if (side[b.idx].vdl != kBadValue) {
          keep = false;
          break;
        }
      }
      if (keep) {
        len = (uint64_t)sa.llen + 1;
        kl = sa.klen;
      }
    }
    slen[p] = len;
  }
  put_tile_sums(len, kl, tcnt, tbytes, tkeys);
}

__global__ __launch_bounds__(kNT) void k_compact_ts(const CompactSide* __restrict__ side, uint64_t n,
                                                    uint64_t* __restrict__ ts) {
  const uint64_t g = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (g >= n) return;
  const CompactSide sd = side[g];
  ts[g] = sd.vdl != kBadValue ? value_ts(sd.src + sd.klen + 1, sd.vdl) : 0;
}

// The LWW select's first half: one lane per sorted record, and only a lane
// whose record heads a run (its predecessor names another key: one same_key
// compare) does anything. It walks forward through its run once, keeps the
// best decodable record so far (lww_beats; records ascend by input index,
// which ascends with the table index, so the index breaks ties), writes 0 to
// slen for every record it passes and, at the run's end, the winner's length
// over its 0. One writer per run and one visit per record: the work of a run
// is linear in its length whatever the order of its timestamps, and summed
// over the runs it is one pass over n records. Only global memory is read, so
// a run may cross wave, block and tile edges. The other lanes of a head's
// wave idle while it walks: with a key in t tables one lane in t works, each
// step two dependent loads (order[q], then side and ts at its index, 8-byte
// gathers that the sort scattered). Keys in few tables, the common case, walk
// a step or two.
template <bool DropDead>
__global__ __launch_bounds__(kNT) void k_compact_lww_runs(const SortKey* __restrict__ order,
                                                          const CompactSide* __restrict__ side,
                                                          const uint64_t* __restrict__ ts,
                                                          const uint8_t* __restrict__ kb,
                                                          const uint64_t* __restrict__ ko, uint64_t n,
                                                          uint64_t* __restrict__ slen) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (p >= n) return;
  const SortKey a = order[p];
  if (p && same_key(a, order[p - 1], kb, ko)) return;  // not a run's head
  bool any = false;
  uint64_t best = 0, best_ts = 0, best_idx = 0;
  SortKey b = a;
  for (uint64_t q = p;;) {
    const uint32_t vdl = side[b.idx].vdl;
    if (vdl != kBadValue) {
      const uint64_t t = ts[b.idx];
      if (!any || lww_beats(t, b.idx, best_ts, best_idx)) {
        any = true;
        best = q;
        best_ts = t;
        best_idx = b.idx;
      }
    }
    slen[q] = 0;
    if (++q >= n) break;
    b = order[q];
    if (!same_key(a, b, kb, ko)) break;
  }
  if (!any) return;
  const CompactSide sw = side[best_idx];
  // (DropDead is a compile-time constant: the plain kernel has no such test)
  if (!(DropDead && value_dead(sw.vdl))) slen[best] = (uint64_t)sw.llen + 1;
}

// Its second half: k_compact_select's three tile sums from slen.
__global__ __launch_bounds__(kNT) void k_compact_lww_tiles(const SortKey* __restrict__ order,
                                                           const CompactSide* __restrict__ side,
                                                           const uint64_t* __restrict__ slen, uint64_t n,
                                                           uint64_t* __restrict__ tcnt, uint64_t* __restrict__ tbytes,
                                                           uint64_t* __restrict__ tkeys) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const uint64_t len = p < n ? slen[p] : 0;
  const uint64_t kl = len ? side[order[p].idx].klen : 0;
  put_tile_sums(len, kl, tcnt, tbytes, tkeys);
}

__global__ __launch_bounds__(kNT) void k_compact_format(const SortKey* __restrict__ order,
                                                        const CompactSide* __restrict__ side,
                                                        const uint64_t* __restrict__ slen,
                                                        const uint64_t* __restrict__ tcnt,
                                                        const uint64_t* __restrict__ tbytes,
                                                        const uint64_t* __restrict__ tkeys,
                                                        const uint64_t* __restrict__ totals, uint64_t n,
                                                        uint64_t nl, uint8_t* __restrict__ out,
                                                        LineRec* __restrict__ rec, uint64_t* __restrict__ pfx,
                                                        uint64_t* __restrict__ fence, uint32_t* __restrict__ llen,
                                                        uint8_t* __restrict__ kb2, uint64_t* __restrict__ ko2) {
  __shared__ uint64_t s_off[kNT + 1];     // survivor i's first byte in the tile
  __shared__ const uint8_t* s_src[kNT];   // its `key \t text`
  __shared__ uint32_t s_ll[kNT];          // that many bytes, then '\n'
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const uint64_t len = p < n ? slen[p] : 0;
  CompactSide sd{};
  if (len) sd = side[order[p].idx];
  uint64_t tl, tc, tk;
  const uint64_t off = block_scan<(int)kNT>(len, &tl);
  const uint64_t ci = block_scan<(int)kNT>(len ? 1 : 0, &tc);
  const uint64_t kof = block_scan<(int)kNT>(len ? sd.klen : 0, &tk);
  if (blockIdx.x == 0 && threadIdx.x == 0) ko2[totals[0]] = totals[2];
  if (!tc) return;  // (uniform)
  if (len) {
    s_off[ci] = off;
    s_src[ci] = sd.src;
    s_ll[ci] = sd.llen;
    // the survivor's key into the packed batch
    const uint64_t k0 = tkeys[blockIdx.x] + kof;
    ko2[tcnt[blockIdx.x] + ci] = k0;
    for (uint32_t j = 0; j < sd.klen; ++j) kb2[k0 + j] = sd.src[j];
    // its index entry (line tcnt + ci of the new file), by k_format's writer
    uint64_t w0, w1;
    load16(sd.src, sd.klen, w0, w1);
    put_index_entry(rec, pfx, llen, fence, nl, tcnt[blockIdx.x] + ci, tbytes[blockIdx.x] + off, w0, w1, sd.klen,
                    sd.vdl, sd.llen);
  }
  if (threadIdx.x == 0) s_off[tc] = tl;
  __syncthreads();
  // the tile's lines: a survivor's `key \t text` from its file, then the '\n'
  copy_tile_bytes(out + tbytes[blockIdx.x], tl, (uint32_t)tc, s_off, [&](uint32_t i, uint64_t j) -> uint32_t {
    const uint64_t b = j - s_off[i];
    return b < s_ll[i] ? s_src[i][b] : (uint32_t)'\n';
  });
}

}  // namespace

hipError_t launch_compact_klen(const CompactSrc* src, uint32_t nsrc, uint64_t n, uint64_t* klen, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_compact_klen", s);
  hipLaunchKernelGGL(k_compact_klen, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, src, nsrc, n, klen);
  return hipGetLastError();
}

hipError_t launch_compact_gather(const CompactSrc* src, uint32_t nsrc, uint64_t n, const uint64_t* ko, uint8_t* kb,
                                 CompactSide* side, uint64_t* dmask, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_compact_gather", s);
  hipLaunchKernelGGL(k_compact_gather, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, src, nsrc, n, ko, kb, side, dmask);
  return hipGetLastError();
}

hipError_t launch_compact_select(const SortKey* order, const CompactSide* side, const uint8_t* kb, const uint64_t* ko,
                                 uint64_t n, bool drop_dead, uint64_t* slen, uint64_t* tcnt, uint64_t* tbytes,
                                 uint64_t* tkeys, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps(drop_dead ? "k_compact_select_live" : "k_compact_select", s);
  const auto k = drop_dead ? k_compact_select<true> : k_compact_select<false>;
  hipLaunchKernelGGL(k, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, kb, ko, n, slen, tcnt, tbytes, tkeys);
  return hipGetLastError();
}

hipError_t launch_compact_ts(const CompactSide* side, uint64_t n, uint64_t* ts, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_compact_ts", s);
  hipLaunchKernelGGL(k_compact_ts, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, side, n, ts);
  return hipGetLastError();
}

hipError_t launch_compact_select_lww(const SortKey* order, const CompactSide* side, const uint64_t* ts,
                                     const uint8_t* kb, const uint64_t* ko, uint64_t n, bool drop_dead,
                                     uint64_t* slen, uint64_t* tcnt, uint64_t* tbytes, uint64_t* tkeys,
                                     hipStream_t s) {
  if (!n) return hipSuccess;
  {
    ProfScope ps(drop_dead ? "k_compact_lww_runs_live" : "k_compact_lww_runs", s);
    const auto k = drop_dead ? k_compact_lww_runs<true> : k_compact_lww_runs<false>;
    hipLaunchKernelGGL(k, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, ts, kb, ko, n, slen);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return launch_compact_tiles(order, side, slen, n, tcnt, tbytes, tkeys, s);
}

hipError_t launch_compact_tiles(const SortKey* order, const CompactSide* side, const uint64_t* slen, uint64_t n,
                                uint64_t* tcnt, uint64_t* tbytes, uint64_t* tkeys, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_compact_lww_tiles", s);
  hipLaunchKernelGGL(k_compact_lww_tiles, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, n, tcnt,
                     tbytes, tkeys);
  return hipGetLastError();
}

hipError_t launch_compact_format(const SortKey* order, const CompactSide* side, const uint64_t* slen,
                                 const uint64_t* tcnt, const uint64_t* tbytes, const uint64_t* tkeys,
                                 const uint64_t* totals, uint64_t n, uint64_t nl, uint8_t* out, LineRec* rec,
                                 uint64_t* pfx, uint64_t* fence, uint32_t* llen, uint8_t* kb2, uint64_t* ko2,
                                 hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_compact_format", s);
  hipLaunchKernelGGL(k_compact_format, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, tcnt, tbytes,
                     tkeys, totals, n, nl, out, rec, pfx, fence, llen, kb2, ko2);
  return hipGetLastError();
}

}  // namespace cb
