// sstable.hip — making and indexing SSTable data files in HBM: the line index,
// SsTable::load's rebuild, the directory and the key buckets, and one table's
// batched search (see sstable.hpp for the reference mapping; the search
// itself is tablesearch.hpp, Database::get's walk getmany.hip, the values'
// decode b64decode.hip).
//
// Index build is streaming byte work (HBM-bound): each block owns a 4 KiB
// chunk, each thread 16 contiguous bytes read as one dwordx4. A byte i starts
// a line iff data[i] != '\n' and (i == 0 or data[i-1] == '\n') — exactly the
// non-empty pieces of raw.split('\n') (src/sstable.rs:142-146). Per-line work
// (TAB position, key prefixes, base64 validity of the value) is done once
// here, so the read path only touches the index and, at the end, the value.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "launch.hpp"
#include "logline.hpp"
#include "profile.hpp"
#include "sstable.hpp"
#include "tablesearch.hpp"
#include "zone.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;

}  // namespace

// ---- line index ----

namespace {

// The 16 bytes of a thread's slice and the byte before it ('\n' before the
// file: the first byte can start a line).
__device__ __forceinline__ void load_slice(const uint8_t* data, uint64_t len, uint64_t base,
                                           uint8_t b[16], uint32_t& prev) {
  if (base + 16 <= len) {
    const uint4 v = *reinterpret_cast<const uint4*>(data + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = base + i < len ? data[base + i] : (uint8_t)'\n';
  }
  prev = base ? data[base - 1] : (uint32_t)'\n';
}

__global__ __launch_bounds__(kNT) void k_line_count(const uint8_t* __restrict__ data, uint64_t len,
                                                    uint64_t* __restrict__ cnt) {
  const uint64_t base = (uint64_t)blockIdx.x * kLineChunk + threadIdx.x * 16;
  uint32_t c = 0;
  if (base < len) {
    uint8_t b[16];
    uint32_t prev;
    load_slice(data, len, base, b, prev);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      c += (b[i] != '\n') & (prev == '\n');
      prev = b[i];
    }
  }
  uint64_t total;
  block_scan<kNT>(c, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

}  // namespace

hipError_t launch_line_count(const uint8_t* data, uint64_t len, uint64_t* cnt, hipStream_t s) {
  if (!len) return hipSuccess;
  ProfScope ps("k_line_count", s);
  hipLaunchKernelGGL(k_line_count, dim3((uint32_t)line_blocks(len)), dim3(kNT), 0, s, data, len,
                     cnt);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(kNT) void k_line_emit(const uint8_t* __restrict__ data, uint64_t len,
                                                   const uint64_t* __restrict__ bbase,
                                                   uint64_t* __restrict__ start,
                                                   uint64_t* __restrict__ end) {
  const uint64_t base = (uint64_t)blockIdx.x * kLineChunk + threadIdx.x * 16;
  uint8_t b[16];
  uint32_t prev = '\n', c = 0;
  if (base < len) {
    load_slice(data, len, base, b, prev);
    uint32_t p = prev;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      c += (b[i] != '\n') & (p == '\n');
      p = b[i];
    }
  }
  uint64_t total;
  uint64_t idx = bbase[blockIdx.x] + block_scan<kNT>(c, &total);
  if (base >= len) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint64_t pos = base + i;
    if (pos < len) {
      if (b[i] != '\n' && prev == '\n') start[idx++] = pos;
      else if (b[i] == '\n' && prev != '\n') end[idx - 1] = pos;  // idx >= 1 here
    }
    prev = b[i];
  }
}

}  // namespace

hipError_t launch_line_emit(const uint8_t* data, uint64_t len, const uint64_t* base,
                            uint64_t* start, uint64_t* end, hipStream_t s) {
  if (!len) return hipSuccess;
  ProfScope ps("k_line_emit", s);
  hipLaunchKernelGGL(k_line_emit, dim3((uint32_t)line_blocks(len)), dim3(kNT), 0, s, data, len,
                     base, start, end);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(kNT) void k_line_finish(const uint8_t* __restrict__ data, uint64_t len,
                                                     uint64_t nlines,
                                                     const uint64_t* __restrict__ start,
                                                     const uint64_t* __restrict__ end,
                                                     LineRec* __restrict__ rec, uint32_t* __restrict__ llen,
                                                     uint32_t* err) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nlines) return;
  const uint64_t s = start[l];
  const uint64_t e = end[l] == ~0ull ? len : end[l];
  const uint64_t n = e - s;
  if (n >= kNoSep) {
    atomicOr(err, 1u);
    return;
  }
  uint32_t k = kNoSep;
  for (uint32_t i = 0; i < (uint32_t)n; i += 8) {  // first TAB, 8 bytes per step
    const uint64_t w = ld8(data + s + i);
    uint32_t hit = 8;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
      if (hit == 8 && i + j < n && ((w >> (8 * j)) & 0xFF) == '\t') hit = j;
    if (hit < 8) {
      k = i + hit;
      break;
    }
  }
  LineRec r;
  r.start = s;
  r.pfx2 = 0;
  r.klen = k;
  r.vdl = kBadValue;
  r.pfx0 = 0;
  rec[l] = r;
  llen[l] = (uint32_t)n;
}

}  // namespace

hipError_t launch_line_finish(const uint8_t* data, uint64_t len, uint64_t nlines,
                              const uint64_t* start, const uint64_t* end, LineRec* rec,
                              uint32_t* llen, uint32_t* err, hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_line_finish", s);
  hipLaunchKernelGGL(k_line_finish, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, data, len,
                     nlines, start, end, rec, llen, err);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(kNT) void k_line_keys(const uint8_t* __restrict__ data, uint64_t nlines,
                                                   LineRec* __restrict__ rec, const uint32_t* __restrict__ llen,
                                                   uint64_t* __restrict__ pfx,
                                                   uint64_t* __restrict__ fence, uint32_t* ok) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const bool live = l < nlines;
  LineRec r = live ? rec[l] : LineRec{};
  bool good = !live || r.klen != kNoSep;
  const uint8_t* p = data + r.start;
  uint64_t v = 0;
  if (live && good) {
    v = ld8_be(p, r.klen < 8 ? r.klen : 8);
    r.pfx2 = r.klen > 8 ? ld8_be(p + 8, r.klen - 8 < 8 ? r.klen - 8 : 8) : 0;
    const int64_t d = b64_len(p + r.klen + 1, llen[l] - r.klen - 1);
    r.vdl = d < 0 ? kBadValue : (uint32_t)d;
  }
  if (live) {
    pfx[l] = v;
    fence_put(fence, nlines, l, v);
    if (good && l > 0) {
      const LineRec q = rec[l - 1];  // start/klen only: written by k_line_finish
      good = q.klen != kNoSep && bytes_cmp(data + q.start, q.klen, p, r.klen) < 0;
    }
    // pfx2, vdl and pfx0 go to their own words so the neighbour read above
    // (start / klen) stays race-free
    rec[l].pfx2 = r.pfx2;
    rec[l].vdl = r.vdl;
    rec[l].pfx0 = v;
  }
  // one atomic per block, none once the flag is down
  if (__syncthreads_or(!good) && threadIdx.x == 0 && *(volatile uint32_t*)ok) atomicAnd(ok, 0u);
}

}  // namespace

hipError_t launch_line_keys(const uint8_t* data, uint64_t nlines, LineRec* rec, const uint32_t* llen,
                            uint64_t* pfx, uint64_t* fence, uint32_t* ok, hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_line_keys", s);
  hipLaunchKernelGGL(k_line_keys, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, data, nlines,
                     rec, llen, pfx, fence, ok);
  return hipGetLastError();
}

// ---- SsTable::load's rebuild from the data file (src/sstable.rs:109-120) ----

namespace {

// Per line: has[l] = 1 when the line has a TAB (its key is inserted), klen[l]
// = the key's bytes (0 otherwise); *bad = the first line whose key is not
// UTF-8 (the reference's load returns Err there; utf8_valid is logline.hpp's).
__global__ __launch_bounds__(kNT) void k_rebuild_mark(const uint8_t* __restrict__ data,
                                                      const LineRec* __restrict__ rec, uint64_t nlines,
                                                      uint64_t* __restrict__ has, uint64_t* __restrict__ klen,
                                                      unsigned long long* __restrict__ bad) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nlines) return;
  const LineRec r = rec[l];
  const bool tab = r.klen != kNoSep;
  has[l] = tab ? 1 : 0;
  klen[l] = tab ? r.klen : 0;
  if (tab && !utf8_valid(data + r.start, r.klen)) atomicMin(bad, (unsigned long long)l);
}

}  // namespace

hipError_t launch_rebuild_mark(const uint8_t* data, const LineRec* rec, uint64_t nlines, uint64_t* has,
                               uint64_t* klen, uint64_t* bad, hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_rebuild_mark", s);
  hipLaunchKernelGGL(k_rebuild_mark, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, data, rec, nlines, has,
                     klen, reinterpret_cast<unsigned long long*>(bad));
  return hipGetLastError();
}

namespace {

// The TAB lines' keys packed into one ragged batch in file order: key i =
// out[off[i] .. off[i+1]) is the key of line lmap[i].
__global__ __launch_bounds__(kNT) void k_rebuild_gather(const uint8_t* __restrict__ data,
                                                        const LineRec* __restrict__ rec, uint64_t nlines,
                                                        const uint64_t* __restrict__ has_scan,
                                                        const uint64_t* __restrict__ len_scan,
                                                        uint8_t* __restrict__ out, uint64_t* __restrict__ off,
                                                        uint64_t* __restrict__ lmap) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nlines) return;
  if (l == nlines - 1) off[has_scan[nlines]] = len_scan[nlines];
  const LineRec r = rec[l];
  if (r.klen == kNoSep) return;
  const uint64_t i = has_scan[l], o = len_scan[l];
  off[i] = o;
  lmap[i] = l;
  const uint8_t* src = data + r.start;
  for (uint32_t j = 0; j < r.klen; ++j) out[o + j] = src[j];
}

}  // namespace

hipError_t launch_rebuild_gather(const uint8_t* data, const LineRec* rec, uint64_t nlines,
                                 const uint64_t* has_scan, const uint64_t* len_scan, uint8_t* out,
                                 uint64_t* off, uint64_t* lmap, hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_rebuild_gather", s);
  hipLaunchKernelGGL(k_rebuild_gather, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, data, rec, nlines,
                     has_scan, len_scan, out, off, lmap);
  return hipGetLastError();
}

// Exclusive scan of n uint64 (out[n] = total) in three launches: each block
// of 4096 values reduces to one partial, k_tile_scan scans the partials in
// place (and writes the total to out[n]), and each block rescans its values
// from its partial. 16 B of traffic per value; used by the line index
// (per-4-KiB-block line counts) and SsTable::load's rebuild (per-line flags
// and key lengths).
constexpr uint64_t kScanPer = 4, kScanChunk = 1024 * kScanPer;

__global__ __launch_bounds__(1024) void k_scan_reduce(const uint64_t* __restrict__ in, uint64_t n,
                                                      uint64_t* __restrict__ part) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
  uint64_t sum = 0;
#pragma unroll
  for (uint64_t j = 0; j < kScanPer; ++j) sum += i0 + j < n ? in[i0 + j] : 0;
  uint64_t total;
  (void)block_scan<1024>(sum, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_scan_apply(const uint64_t* __restrict__ in, uint64_t n,
                                                     const uint64_t* __restrict__ part,
                                                     uint64_t* __restrict__ out) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
  uint64_t v[kScanPer], sum = 0;
#pragma unroll
  for (uint64_t j = 0; j < kScanPer; ++j) {
    v[j] = i0 + j < n ? in[i0 + j] : 0;
    sum += v[j];
  }
  const uint64_t base = part[blockIdx.x];
  uint64_t total;
  uint64_t p = base + block_scan<1024>(sum, &total);
#pragma unroll
  for (uint64_t j = 0; j < kScanPer; ++j) {
    if (i0 + j < n) out[i0 + j] = p;
    p += v[j];
  }
}

uint64_t scan_tmp_words(uint64_t n) { return (n + kScanChunk - 1) / kScanChunk + 1; }

hipError_t launch_scan_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp,
                           hipStream_t s) {
  if (!n) return hipMemsetAsync(out, 0, 8, s);
  const uint64_t nb = (n + kScanChunk - 1) / kScanChunk;
  {
    ProfScope ps("k_scan_reduce", s);
    hipLaunchKernelGGL(k_scan_reduce, dim3((uint32_t)nb), dim3(1024), 0, s, in, n, tmp);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_tile_scan(tmp, nb, out + n, s);
  if (e != hipSuccess) return e;
  ProfScope ps("k_scan_apply", s);
  hipLaunchKernelGGL(k_scan_apply, dim3((uint32_t)nb), dim3(1024), 0, s, in, n, tmp, out);
  return hipGetLastError();
}

// ---- the directory and the key buckets ----

namespace {

// dir from the sorted prefixes, one lane per line (dir_fill). Block 0 also
// stores the map (the table's device copy).
__global__ __launch_bounds__(kNT) void k_table_dir(const uint64_t* __restrict__ pfx, uint64_t nl, DirMap dm,
                                                   uint32_t* __restrict__ dir, DirMap* dmap_out) {
  __shared__ DirMap sdm;
  if (threadIdx.x == 0) {
    sdm = dm;
    if (blockIdx.x == 0) *dmap_out = dm;
  }
  __syncthreads();
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const bool live = p < nl;
  const uint64_t w = live ? pfx[p] : 0;
  const uint64_t b = live ? dir_bucket(sdm, w) : 0;
  uint64_t bp = __shfl_up(b, 1, 64);
  if (live && (threadIdx.x & 63u) == 0 && p > 0) bp = dir_bucket(sdm, pfx[p - 1]);
  dir_fill(dir, sdm.nbuckets, nl, p, live, b, bp);
}

}  // namespace

hipError_t launch_table_dir(const uint64_t* pfx, uint64_t nlines, const DirMap& dm, uint32_t* dir,
                            DirMap* dmap_out, hipStream_t s) {
  if (!nlines || !dir || !dmap_out) return hipErrorInvalidValue;
  ProfScope ps("k_table_dir", s);
  hipLaunchKernelGGL(k_table_dir, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, pfx, nlines, dm, dir, dmap_out);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(kNT) void k_pfx_masks(const uint64_t* __restrict__ pfx, uint64_t nl,
                                                   uint64_t* __restrict__ mask) {
  sample_pfx_masks(nl, [&](uint64_t q) { return pfx[q]; }, mask);
}

}  // namespace

hipError_t launch_pfx_masks(const uint64_t* pfx, uint64_t nlines, uint64_t* mask, hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_pfx_masks", s);
  hipLaunchKernelGGL(k_pfx_masks, dim3(kSampleBlocks), dim3(kNT), 0, s, pfx, nlines, mask);
  return hipGetLastError();
}

namespace {

// The key buckets (sstable.hpp) of a fast table, one lane per line: the
// bucket's count word hands out slots (1 per stored line, 16 per line left
// out, so a bucket holding one is never taken as complete).
__global__ __launch_bounds__(kNT) void k_table_buckets(const LineRec* __restrict__ rec, uint64_t nl,
                                                       uint64_t* __restrict__ bkt, uint32_t bits) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nl) return;
  const LineRec r = grec(rec, l);
  const bool keep = r.klen < 4095u && r.vdl <= 4095u && r.start < (1ull << 40);  // klen 0xFFF: unwritten slot
  uint64_t* b = bkt + bkt_index(r.pfx0, bits) * kBktWords;
  const uint64_t s = atomicAdd(reinterpret_cast<unsigned long long*>(b), keep ? 1ull : 16ull) + 1;
  if (keep && s < kBktSlots) {
    b[1 + s] = r.pfx0;
    b[6 + 2 * s] = r.pfx2;
    b[7 + 2 * s] = r.start | ((uint64_t)r.klen << 40) | ((uint64_t)r.vdl << 52);
  }
}

// The buckets' summary words (sstable.hpp bkt_fp), one lane per bucket,
// after k_table_buckets.
__global__ __launch_bounds__(kNT) void k_table_bucket_fp(uint64_t* __restrict__ bkt, uint32_t bits) {
  const uint64_t nbk = 1ull << bits;
  const uint64_t i = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (i >= nbk) return;
  const uint64_t* b = bkt + i * kBktWords;
  const uint64_t cnt = b[0] + 1;  // all-ones: empty
  uint64_t f = cnt <= kBktSlots ? cnt : 15u;
  if (f != 15u)
    for (uint32_t s = 0; s < (uint32_t)cnt; ++s) f |= (uint64_t)bkt_fp(b[1 + s]) << (4 + 15 * s);
  bkt[nbk * kBktWords + i] = f;
}

}  // namespace

hipError_t launch_table_buckets(const LineRec* rec, uint64_t nlines, uint64_t* bkt, uint32_t bits,
                                hipStream_t s) {
  if (!nlines) return hipSuccess;
  ProfScope ps("k_table_buckets", s);
  hipLaunchKernelGGL(k_table_buckets, dim3(blocks_for(nlines, kNT)), dim3(kNT), 0, s, rec, nlines, bkt, bits);
  hipLaunchKernelGGL(k_table_bucket_fp, dim3(blocks_for(1ull << bits, kNT)), dim3(kNT), 0, s, bkt, bits);
  return hipGetLastError();
}

// ---- one table's search ----

namespace {

template <int KEYK>
__global__ __launch_bounds__(kNT) void k_table_search(TableView t, KeySrc ks, uint64_t n,
                                                      int64_t* __restrict__ line) {
  const uint64_t k = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (k >= n) return;
  const Query q = make_query<KEYK>(ks, k);
  LineRec r;
  line[k] = search(t, q, r, t.dmap);
}

}  // namespace

hipError_t launch_table_search(int keyk, const TableView& t, const KeySrc& ks, uint64_t n,
                               int64_t* line, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_table_search", s);
  const dim3 g(blocks_for(n, kNT));
  CB_KEY_DISPATCH(keyk, hipLaunchKernelGGL(k_table_search<KK>, g, dim3(kNT), 0, s, t, ks, n, line));
  return hipGetLastError();
}

}  // namespace cb
