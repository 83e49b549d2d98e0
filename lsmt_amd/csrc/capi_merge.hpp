// capi_merge.hpp — what the two users of the device merge share
// (capi_merge.cpp: the merge itself, the table-list checks and compaction;
// capi_scan.cpp: scans, counts and the scan result), capi_select.cpp, which
// stages its selection the way they stage theirs, capi_replay.cpp, whose
// log replay is the merge over one unsorted input, and capi_ring.cpp, whose
// compaction is compaction with one step more. Included only by them.
#pragma once
#include <functional>

#include "capi_table.hpp"
#include "compact.hpp"

namespace cbx {

constexpr cb::MergeRule kNewest{cb::MergeOrder::newest, false};  // the plain entries' rule
constexpr cb::MergeRule kLive{cb::MergeOrder::newest, true};     // the live-row entries'

// ---- the table list every entry takes (capi_merge.cpp) ----

// A non-empty list without a null table, all on one device (*dev).
int check_table_list(const cb_table* const* tables, uint32_t nt, int* dev);

// each(table, its place in the list) for the non-empty tables, newest first:
// every table is finalised on the way, and one that is not well-formed refused.
template <class Each>
int for_live_tables(const cb_table* const* tables, uint32_t nt, Each each) {
  for (uint32_t i = 0; i < nt; ++i) {
    cb_table* ti = const_cast<cb_table*>(tables[i]);
    if (int rc = finalize_table(ti)) return rc;
    if (!ti->nlines) continue;
    if (!ti->fast) return fail(CB_EINVAL, "an input table is not well-formed");
    each(ti, i);
  }
  return CB_OK;
}

// ---- the merge (capi_merge.cpp) ----

// The newest-wins merge that cb_tables_compact and cb_tables_scan run over
// their sources (compact.hpp): the lines' keys gathered into one batch, the
// stable key sort, the select of each key's newest decodable line and the
// scanned tile sums of the survivors. Its scratch is one pool block.
struct Merge {
  uint64_t n = 0, kbound = 0, tiles = 0;  // lines, a bound on their keys' bytes, select tiles
  SortPlan plan{};
  cb::CompactSrc* dsrc = nullptr;  // room for the caller's sources (nsrc_cap of them)
  uint64_t *klen = nullptr, *ko = nullptr, *scan = nullptr;
  uint8_t* kb = nullptr;
  cb::CompactSide* side = nullptr;
  cb::SortKey* order = nullptr;
  uint8_t* sort = nullptr;
  uint64_t *slen = nullptr, *tcnt = nullptr, *tbytes = nullptr, *tkeys = nullptr, *tot = nullptr;
  uint64_t* ts = nullptr;  // the lines' timestamps: an LWW merge's only
  cb::CreateResult* dr = nullptr;
};
int merge_alloc(uint32_t nsrc_cap, uint64_t n, uint64_t kbound, cb::MergeOrder order, TempBlock& tmp, Merge* m);
// The merge of sources dsrc[0..nsrc) (device, m.n lines in all) on s, up to
// and including the select (nothing is waited for): the sorted order and, per
// sorted record, whether it survives (slen) with the tiles' sums. The rule
// (compact.hpp) picks the select: newest enqueues k_compact_select, lww the
// lines' timestamps and the two launches of the LWW select (m was allocated
// for the same order); drop_dead: either keeps no tombstone (liverow.hpp).
int enqueue_merge_select(const Merge& m, const cb::CompactSrc* dsrc, uint32_t nsrc, cb::MergeRule rule, hipStream_t s);
// enqueue_merge_select's two halves around its gather, for a caller that
// gathers its own records into m (cb_log_replay, capi_replay.cpp): the bin
// sort's inputs reset (an unsorted batch, its prefix byte masks zeroed) before
// the gather, and behind it the sort and the rule's select.
int enqueue_sort_begin(const Merge& m, hipStream_t s);
int enqueue_sort_select(const Merge& m, cb::MergeRule rule, hipStream_t s);
// enqueue_merge's tail: the scans of the tile sums, the totals read back,
// waited for and checked.
int merge_totals(const Merge& m, hipStream_t s, uint64_t (&h)[3]);
// The rest of the merge for a caller that writes the survivors out: the scans
// of the tile sums and the survivors' totals h = {lines, file bytes, key
// bytes}, read back (they size the caller's output), the stream waited for,
// and checked against the inputs' bounds before anything is sized from them.
// (A count stops at the select: it places no survivor.)
int enqueue_merge(const Merge& m, const cb::CompactSrc* dsrc, uint32_t nsrc, cb::MergeRule rule, hipStream_t s,
                  uint64_t (&h)[3]);

// ---- the merged table (capi_merge.cpp: cb_tables_compact's steps behind the merge, which
// cb_log_replay takes too) ----

// The kept keys as one batch (device, in a block of the call's).
struct KeptKeys {
  uint8_t* kb = nullptr;
  uint64_t* ko = nullptr;
};
// The survivors (h = {lines, file bytes, key bytes}) formatted into t: the
// file and its line index in one pass, and the kept keys beside them (in
// `keys`). No survivor: the file's buffer alone.
int format_survivors(cb_table* t, const Merge& mg, const uint64_t (&h)[3], TempBlock& keys, KeptKeys* k,
                     hipStream_t s);
// The directory and the zone map's bounds of a formatted table with at least
// one line (two waits); t is well-formed by construction.
int finish_compacted(cb_table* t, const Merge& mg, const KeptKeys& k, const uint64_t (&h)[3], hipStream_t s);
// A filter of no bits: BloomFilter::insert's `% 0` (src/bloom.rs:36).
int zero_m_error();
// That refusal made before the table list is looked at, the outputs cleared
// (the live-row, LWW and ring compactions); CB_OK otherwise.
int zero_m_before_tables(uint64_t m_bits, cb_table** table_out, cb_filter** bloom_out);
// A step of the caller's between a merge's select and its totals, enqueued on
// the merge's stream: it may only clear survivors (slen[p] = 0) and must leave
// the tile sums right (compact.hpp launch_compact_tiles).
using AfterSelect = std::function<int(const Merge&, hipStream_t)>;
// Compaction: the table list checked, the sources merged under `rule` (after,
// nullable, behind the select), the survivors formatted into a new table with
// its Bloom filter (bloom_out nullable), line index and zone bounds.
int compact_tables(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, cb::MergeRule rule,
                   const AfterSelect* after, void* stream, cb_table** table_out, cb_filter** bloom_out);

// ---- host values on their way into a call's scratch block ----

// The parts carved from c before seal() are staged: filled at their carved
// offsets in a zeroed host copy, they go up in one copy to the front of the
// block allocated from c. What is carved after seal() is the device's alone.
// The host copy is pageable: it must outlive the copy (a wait on the stream).
struct Staging {
  cb::Carver c;
  std::vector<uint8_t> host;
  void seal() { host.assign(c.total(), 0); }
  uint8_t* at(size_t off) { return &host[off]; }
  void put(size_t off, const void* p, size_t bytes) {
    if (bytes) std::memcpy(&host[off], p, bytes);
  }
  hipError_t upload(const TempBlock& b, hipStream_t s) const {
    return hipMemcpyAsync(b.p, host.data(), host.size(), hipMemcpyHostToDevice, s);
  }
};

}  // namespace cbx
