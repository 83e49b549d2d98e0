// capi_table.hpp — what the SSTable entries' five translation units share
// (capi_table.cpp: the handle, its index and a file that already exists;
// capi_flush.cpp: SsTable::create; capi_get.cpp: the read path;
// capi_merge.cpp: the merge and compaction; capi_scan.cpp: scans and counts;
// the last two share capi_merge.hpp besides). Included only by them.
#pragma once
#include "capi_internal.hpp"
#include "tablehost.hpp"

namespace cbx {

// ---- pool blocks (capi_table.cpp) ----

// pool_alloc of `bytes` or the refusal CB_ENOMEM with `what` as its text; a
// failure leaves *p null.
int pool_alloc_or(int dev, size_t bytes, void** p, size_t* cap, const char* what);

// A pool block that is scratch for one call: released stream-ordered when it
// leaves scope, on every return path.
struct TempBlock {
  int dev;
  void* p = nullptr;
  size_t cap = 0;
  ~TempBlock() { pool_release(dev, p, cap); }
  // what a carver measured
  int alloc(const cb::Carver& c, const char* what) { return pool_alloc_or(dev, c.total(), &p, &cap, what); }
  uint8_t* at(size_t off) const { return (uint8_t*)p + off; }
};

// ---- the steps every maker of a table shares (capi_table.cpp) ----

// cb_table_force_exact: index files for the exact-trajectory search only.
bool table_exact();
// The file's buffer (the file and its 16 bytes of slack, or a bound on them)
// and the index of nl lines, from the pool; a failure leaves the pointer null.
int alloc_file(cb_table* t, uint64_t bytes);
int alloc_index(cb_table* t, uint64_t nl);
void drop_index(cb_table* t);
// Where the directory's map lives in t's index (nullptr: no directory).
cb::DirMap* dmap_slot(const cb_table* t);
// The directory of a table whose prefixes are written, in two halves around
// the caller's one copy-back and wait: the byte values of every prefix
// position into dmask (device, kDirMaskBytes), then, from their host copy,
// the map and the directory itself. Nothing for a table too small for one.
constexpr size_t kDirMaskBytes = sizeof(cb::CreateResult::dmask);
int enqueue_pfx_masks(const cb_table* t, uint64_t* dmask, hipStream_t s);
int enqueue_directory(cb_table* t, const uint64_t (&masks)[cb::kDirPos][4], hipStream_t s);
// An empty table's file: 16 zero bytes (allocated here unless the caller
// has), complete on return.
int finish_empty_file(cb_table* t, hipStream_t s);
// Line index of t->data[0..t->len). Temporaries come from the stream's
// workspace (taken here: callers must not hold its lock).
int index_table(cb_table* t, hipStream_t s);

// ---- the stable key sort (capi_flush.cpp; the merge sorts as a flush does) ----

// The stable sort of n keys: the bin sort for batches past one merge-sort tile
// (its fallback, the merge sort, enqueued behind it), the merge sort alone
// for smaller ones and past 2^24.
struct SortPlan {
  bool binned;
  uint32_t T;          // the bin sort's group target
  uint64_t tmp_bytes;  // the scratch enqueue_key_sort needs
};
SortPlan plan_key_sort(uint64_t n);
// order = the records of (kb, ko) in stable key order, on s. Every launch
// returns at once unless dr->flags[0] says the batch is unsorted; the merge
// sort behind a bin sort runs only when that set dr->flags[3] (one bin, or a
// bin larger than an LDS tile: keys sharing a long prefix), and then rewrites
// the records, value spans and tile sums whole. vo == nullptr: no value tail
// (vsp and tsum are not written).
int enqueue_key_sort(const SortPlan& plan, const uint8_t* kb, const uint64_t* ko, uint64_t n, cb::SortKey* order,
                     void* tmp, cb::CreateResult* dr, hipStream_t s, const uint64_t* vo, ulonglong2* vsp,
                     uint64_t* tsum);

// ---- the value tail's device half (capi_get.cpp; a scan decodes as a get does) ----

// The found values of n answers: their sources, decoded lengths and the
// lengths' tile sums (get_tiles(n) of them), and the offsets they decode to.
struct ValueSpans {
  const uint64_t *vsrc, *dlen;
  uint64_t* tsum;
  uint64_t* voff;  // n + 1
};
// Offsets and (vals != nullptr) bytes of the values on s. Batches of up to
// decode_raw_max() answers: the decode scans the tile sums itself (one launch
// fewer); larger ones, a caller without raw_ok, and CB_DECODE_RAW=0: the
// one-block scan first, which leaves voff[n]. again: a second decode of spans
// this function has already scanned (nothing is scanned twice).
int enqueue_value_decode(const ValueSpans& v, uint64_t n, uint8_t* vals, uint64_t cap, bool raw_ok, bool again,
                         hipStream_t s);

}  // namespace cbx
