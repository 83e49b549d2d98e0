// tablesearch.hpp — one key's search of one table (device only):
// SsTable::binary_search's exact trajectory, and for well-formed files the
// key buckets, the directory and the fence descent (sstable.hpp). Included by
// the files that hold k_table_search (sstable.hip) and the get kernels
// (getmany.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

#include "sstable.hpp"
#include "tablebytes.hpp"
#include "zone.hpp"

namespace cb {

// Rust str order of a line key (table data, side a) against a query key.
__device__ __forceinline__ int line_cmp(const uint8_t* a, uint64_t al, const uint8_t* b,
                                        uint64_t bl) {
  const uint64_t n = al < bl ? al : bl;
  for (uint64_t i = 0; i < n; i += 8) {
    const uint64_t m = n - i < 8 ? n - i : 8;
    const uint64_t x = ld8_be(a + i, m), y = be_chunk(b + i, m);
    if (x != y) return x < y ? -1 : 1;
  }
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

// A query key with its first 16 bytes as big-endian words.
struct Query {
  const uint8_t* p;
  uint64_t len, w0, w1;
};

template <int KEYK>
__device__ __forceinline__ Query make_query(const KeySrc& ks, uint64_t k) {
  Query q;
  key_span<KEYK>(ks, k, q.p, q.len);
  if constexpr (KEYK == KEY_FIXED16) {
    const uint4 v = reinterpret_cast<const uint4*>(ks.bytes)[k];
    q.w0 = (uint64_t)__builtin_bswap32(v.x) << 32 | __builtin_bswap32(v.y);
    q.w1 = (uint64_t)__builtin_bswap32(v.z) << 32 | __builtin_bswap32(v.w);
  } else {
    q.w0 = be_chunk(q.p, q.len < 8 ? q.len : 8);
    q.w1 = q.len > 8 ? be_chunk(q.p + 8, q.len - 8 < 8 ? q.len - 8 : 8) : 0;
  }
  return q;
}

// Line key (pfx already known equal to q.w0) against the query. Keys of at
// most 16 bytes compare from the index alone: zero-padded 16-byte forms
// first, then length — the same order as Rust's str order for such keys.
__device__ __forceinline__ int rec_cmp(const TableView& t, const LineRec& r, const Query& q) {
  if (r.klen <= 16 && q.len <= 16) {
    if (r.pfx2 != q.w1) return r.pfx2 < q.w1 ? -1 : 1;
    return r.klen < q.len ? -1 : (r.klen > q.len ? 1 : 0);
  }
  return line_cmp(t.data + r.start, r.klen, q.p, q.len);
}

// Index loads as global (not flat) loads: every index array is device memory,
// and a flat load also holds the LDS counter, so the LDS-resident views and
// the search's loads would wait on each other.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u64x2* g64x2;
static_assert(sizeof(LineRec) == 32 && offsetof(LineRec, pfx2) == 8 && offsetof(LineRec, klen) == 16 &&
                  offsetof(LineRec, vdl) == 20 && offsetof(LineRec, pfx0) == 24,
              "grec reads LineRec as two 16-byte words");
__device__ __forceinline__ LineRec grec(const LineRec* r, uint64_t i) {
  const g64x2 p = (g64x2)(r + i);
  const u64x2 lo = p[0], hi = p[1];
  LineRec o;
  o.start = lo.x;
  o.pfx2 = lo.y;
  o.klen = (uint32_t)hi.x;
  o.vdl = (uint32_t)(hi.x >> 32);
  o.pfx0 = hi.y;
  return o;
}
__device__ __forceinline__ uint64_t g64(const uint64_t* p, uint64_t i) {
  return ((const __attribute__((address_space(1))) uint64_t*)p)[i];
}

// SsTable::binary_search (src/sstable.rs:161-179), same mid sequence.
__device__ __forceinline__ int64_t search_exact(const TableView& t, const Query& q, LineRec& hit) {
  uint64_t lo = 0, hi = t.nlines();
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    const LineRec r = grec(t.rec, mid);
    if (r.klen == kNoSep) break;
    const int c = line_cmp(t.data + r.start, r.klen, q.p, q.len);
    if (c < 0)
      lo = mid + 1;
    else if (c > 0)
      hi = mid;
    else {
      hit = r;
      return (int64_t)mid;
    }
  }
  return -1;
}

// First index in [lo, hi) with a[i] >= x, or hi (a non-decreasing).
__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (g64(a, mid) < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Line l's key against the query, in a well-formed file: its record (which
// holds the prefix) in one load, r receives it.
__device__ __forceinline__ int line_vs_query(const TableView& t, uint64_t l, const Query& q, LineRec& r) {
  r = grec(t.rec, l);
  if (r.pfx0 != q.w0) return r.pfx0 < q.w0 ? -1 : 1;
  return rec_cmp(t, r, q);
}

// The lines from b on that share the query's prefix, by a galloping search
// with record compares (b: the prefix's lower bound, < nlines).
// Line b (the prefix's lower bound, its prefix equal to the query's) with
// its record r already loaded: the record compare, then the lines after b
// that share the prefix by a galloping search.
__device__ __forceinline__ int64_t resolve_rec(const TableView& t, const Query& q, uint64_t b, LineRec r,
                                               LineRec& hit) {
  int c = rec_cmp(t, r, q);
  if (c == 0) {
    hit = r;
    return (int64_t)b;
  }
  if (c > 0) return -1;
  // every line before lo is below the query; gallop to a line above it
  uint64_t lo = b + 1, hi = t.nlines(), step = 1;
  while (lo < t.nlines()) {
    const uint64_t p = lo + step - 1 < t.nlines() ? lo + step - 1 : t.nlines() - 1;
    c = line_vs_query(t, p, q, r);
    if (c == 0) {
      hit = r;
      return (int64_t)p;
    }
    if (c > 0) {
      hi = p;
      break;
    }
    lo = p + 1;
    step <<= 1;
  }
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    c = line_vs_query(t, mid, q, r);
    if (c == 0) {
      hit = r;
      return (int64_t)mid;
    }
    if (c < 0)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

__device__ __forceinline__ int64_t resolve_from(const TableView& t, const Query& q, uint64_t b, LineRec& hit) {
  // line b's record holds its prefix: one load (the record is needed
  // whenever the prefix matches, i.e. for every key that is present)
  const LineRec r = grec(t.rec, b);
  if (r.pfx0 != q.w0) return -1;  // pfx0 > q.w0: b is the prefix's lower bound
  return resolve_rec(t, q, b, r, hit);
}

// Level j's array (0: pfx).
__device__ __forceinline__ const uint64_t* level_array(const TableView& t, uint32_t j) {
  return j ? t.fence + level_offset(t.nlines(), j) : t.pfx;
}

// The range of level j-1 that holds the lower bound, from level j's answer i
// (E_j[i-1] < x <= E_j[i], E_j[i] = E_{j-1}[16 i]): at most 16 entries.
__device__ __forceinline__ void level_down(const TableView& t, uint32_t j, uint64_t i, uint64_t& lo, uint64_t& hi) {
  const uint64_t cnt = level_count(t.nlines(), j - 1);
  lo = i ? ((i - 1) << kFanBits) + 1 : 0;
  hi = (i << kFanBits) < cnt ? (i << kFanBits) : cnt;
}

constexpr uint32_t kWin = 8;     // buckets of up to this many lines: one round of prefix loads
constexpr uint32_t kRecWin = 2;  // ... of up to this many: the records alone (32 B each, prefix inside)

// The key buckets' answer (sstable.hpp, TableView::bkt): kBktFound (hit
// holds the line's record, the line index unknown), -1 (absent, proven by a
// complete bucket), or kBktGoOn (the directory search decides).
constexpr int64_t kBktFound = INT64_MAX;
constexpr int64_t kBktGoOn = -2;
// The bucket's first 16 bytes (its count and slot 0's prefix) for key word
// w0: what bucket_probe reads first.
__device__ __forceinline__ u64x2 bucket_head(const TableView& t, uint64_t w0) {
  return *(g64x2)(t.bkt + bkt_index(w0, t.bkbits()) * kBktWords);
}

// bucket_probe with its first load (bucket_head) already made.
__device__ __forceinline__ int64_t bucket_probe_from(const TableView& t, const Query& q, LineRec& hit, u64x2 a) {
  const uint64_t* b = t.bkt + bkt_index(q.w0, t.bkbits()) * kBktWords;
  // the count and slot 0 first (at one line per bucket on average, most keys
  // are in slot 0), the next pairs only when needed: fewer registers live
  const uint64_t cnt = a.x + 1;  // all-ones: empty
  uint32_t c = 0;
  if (cnt == 0 || a.y != q.w0) {
    if (cnt <= 1) return -1;
    const u64x2 c23 = *(g64x2)(b + 2);
    c = (c23.x == q.w0) ? 1u : (cnt > 2 && c23.y == q.w0) ? 2u : 4u;
    if (c == 4u) {
      if (cnt <= 3) return -1;
      if (g64(b, 4) != q.w0) return cnt == 4 ? -1 : kBktGoOn;
      c = 3u;
    }
  }
  const u64x2 tl = *(g64x2)(b + 6 + 2 * c);
  LineRec r;
  r.start = tl.y & ((1ull << 40) - 1);
  r.pfx2 = tl.x;
  r.klen = (uint32_t)(tl.y >> 40) & 0xFFFu;
  if (r.klen == 0xFFFu) return kBktGoOn;  // a slot left unwritten (its bucket also holds a line left out)
  r.vdl = (uint32_t)(tl.y >> 52);
  r.pfx0 = q.w0;
  const int cmp = rec_cmp(t, r, q);
  if (cmp == 0) {
    hit = r;
    return kBktFound;
  }
  return kBktGoOn;  // another line with this prefix may be the one
}

__device__ __forceinline__ int64_t bucket_probe(const TableView& t, const Query& q, LineRec& hit) {
  return bucket_probe_from(t, q, hit, bucket_head(t, q.w0));
}

// Where x's descent starts: level j and the run [lo, hi) of at most 16
// entries holding its lower bound (returns false), or true when x is absent
// outright: its bucket is empty. dm: the table's DirMap (LDS-staged by the read path).
// Lines before dir[B] have smaller buckets (so smaller prefixes) and lines
// from dir[B+1] on larger ones, so on every level the entries sampled from
// [dir[B], dir[B+1]] bracket x's lower bound.
__device__ __forceinline__ bool dir_start(const TableView& t, const DirMap* dm, uint64_t x, uint32_t& j,
                                          uint64_t& lo, uint64_t& hi) {
  j = t.nlev();
  lo = 0;
  hi = level_count(t.nlines(), j);
  if (!t.dir) return false;
  const uint64_t bk = dir_bucket(*dm, x);
  // dir[B] and dir[B + 1] as one 8-byte load (one L2 request, not two: the
  // search is bound by the requests a CU keeps in flight)
  const u32x2 ae = *(const __attribute__((address_space(1))) u32x2*)(t.dir + bk);
  const uint64_t a = ae.x, e = ae.y;
  if (a == e) return true;
  for (uint32_t l = 0; l < t.nlev(); ++l) {
    const uint64_t l0 = a >> (kFanBits * l);
    const uint64_t c = level_count(t.nlines(), l);
    uint64_t l1 = (e + (1ull << (kFanBits * l)) - 1) >> (kFanBits * l);
    l1 = l1 < c ? l1 : c;
    if (l1 - l0 <= kFanout) {
      j = l;
      lo = l0;
      hi = l1;
      return false;
    }
  }
  return false;  // the top level (at most 16 entries)
}

// Well-formed files (keys strictly increasing, so any correct search returns
// the reference's line): the lower bound of the key's 8-byte prefix down the
// fence levels (one run of at most 16 entries, one 128-B line, per level),
// then the lines sharing that prefix by a galloping search with record
// compares: O(log run) for keys that share long prefixes ('user0000...'), one
// record compare when the prefix is unique.
__device__ __forceinline__ int64_t search_fast(const TableView& t, const Query& q, LineRec& hit,
                                               const DirMap* dm) {
  if (t.bkt) {
    const int64_t b = bucket_probe(t, q, hit);
    if (b != kBktGoOn) return b;
  }
  uint32_t j;
  uint64_t lo, hi;
  // an empty bucket: absent
  if (dir_start(t, dm, q.w0, j, lo, hi)) return -1;
  if (j == 0 && hi - lo <= kRecWin) {
    // a bucket of at most kRecWin lines: its records hold the prefixes, so
    // the records are all that is read (one round of independent loads: one
    // or two 128-B lines where the prefixes and then the matching record
    // took two); the matching one is already in registers
    LineRec rr[kRecWin];
#pragma unroll
    for (uint32_t k = 0; k < kRecWin; ++k)
      if (lo + k < hi) rr[k] = grec(t.rec, lo + k);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRecWin; ++k) c += (lo + k < hi && rr[k].pfx0 < q.w0) ? 1u : 0u;
    if (lo + c == hi) return -1;  // every line below the key: the next one is in a larger bucket
    LineRec r = rr[0];
#pragma unroll
    for (uint32_t k = 1; k < kRecWin; ++k)
      if (k == c) r = rr[k];
    if (r.pfx0 != q.w0) return -1;
    return resolve_rec(t, q, lo + c, r, hit);
  }
  if (j == 0 && hi - lo <= kWin) {
    // a larger bucket (or the whole table): its prefixes from the dense
    // prefix array in one round of independent loads (64 B for 8 lines),
    // then the matching record
    uint64_t v[kWin];
    // in pairs: two neighbouring prefixes as one 16-byte load where both
    // are in the bucket (one L2 request per pair, not per prefix)

#pragma unroll
    for (uint32_t k = 0; k < kWin; k += 2) {
      if (lo + k + 1 < hi) {
        const u64x2 pr = *(g64x2)(t.pfx + lo + k);
        v[k] = pr.x;
        v[k + 1] = pr.y;
      } else {
        v[k] = lo + k < hi ? g64(t.pfx, lo + k) : ~0ull;
        v[k + 1] = ~0ull;
      }
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWin; ++k) c += (lo + k < hi && v[k] < q.w0) ? 1u : 0u;
    // every line below the key: the next one is in a larger bucket
    if (lo + c == hi) return -1;
    uint64_t p0 = v[0];
#pragma unroll
    for (uint32_t k = 1; k < kWin; ++k) p0 = k == c ? v[k] : p0;
    if (p0 != q.w0) return -1;
    return resolve_rec(t, q, lo + c, grec(t.rec, lo + c), hit);
  }
  for (;; --j) {
    const uint64_t i = lower_bound_u64(level_array(t, j), lo, hi, q.w0);
    if (!j) {
      if (i >= t.nlines()) return -1;
      return resolve_from(t, q, i, hit);
    }
    level_down(t, j, i, lo, hi);
  }
}

// dm: the table's DirMap (LDS or global); used only when t.dir is set.
__device__ __forceinline__ int64_t search(const TableView& t, const Query& q, LineRec& hit, const DirMap* dm) {
  return t.fast() ? search_fast(t, q, hit, dm) : search_exact(t, q, hit);
}

}  // namespace cb
