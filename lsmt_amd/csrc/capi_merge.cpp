// capi_merge.cpp — merging SSTables on the device: the newest-wins merge
// (compact.hpp) with the checks of the table list every user of it takes, and
// compaction into one new table (cb_tables_compact). cb_tables_compact_live
// runs the same steps with the select that drops tombstones (liverow.hpp),
// cb_tables_compact_lww with the select that keeps a key's line of the
// greatest timestamp (rowts.hpp) in place of its newest one. The merge's
// other user, the scans and counts, is capi_scan.cpp, and the log replay
// (capi_replay.cpp) runs it over its own gather and then takes compaction's
// steps behind it, and the ring's compaction (capi_ring.cpp) is compact_tables
// with a step of its own behind the select; capi_merge.hpp declares what they
// need.
//
// Reference: src/sstable.rs:51-98 (the file a compaction writes),
// src/lib.rs:125-146 (Database::get, whose answers it reproduces), src/cluster.rs:405-416,
// 454-459 (the read's fold by timestamp, which the LWW entries reproduce).
#include "capi_merge.hpp"

using namespace cbx;
using cb::MergeOrder;
using cb::MergeRule;

namespace cbx {

int check_table_list(const cb_table* const* tables, uint32_t nt, int* dev) {
  if (!nt || !tables) return fail(CB_EINVAL, "no tables");
  for (uint32_t i = 0; i < nt; ++i)
    if (!tables[i]) return fail(CB_EINVAL, "null table");
  *dev = tables[0]->device;
  for (uint32_t i = 0; i < nt; ++i)
    if (tables[i]->device != *dev) return fail(CB_EINVAL, "tables live on different devices");
  return CB_OK;
}

int merge_alloc(uint32_t nsrc_cap, uint64_t n, uint64_t kbound, MergeOrder order, TempBlock& tmp, Merge* m) {
  m->n = n;
  m->kbound = kbound;
  m->tiles = cb::compact_tiles(n);
  m->plan = plan_key_sort(n);  // the order: sorted as cb_sstable_create sorts a batch
  cb::Carver c;
  const size_t o_src = c.take(nsrc_cap * sizeof(cb::CompactSrc)), o_klen = c.take(n * 8), o_ko = c.take((n + 1) * 8),
               o_scan = c.take(cb::scan_tmp_words(n) * 8), o_kb = c.take(kbound + 16),
               o_side = c.take(n * sizeof(cb::CompactSide)), o_order = c.take(n * sizeof(cb::SortKey)),
               o_sort = c.take(m->plan.tmp_bytes), o_slen = c.take(n * 8), o_tcnt = c.take(m->tiles * 8),
               o_tbytes = c.take(m->tiles * 8), o_tkeys = c.take(m->tiles * 8), o_tot = c.take(3 * 8),
               o_res = c.take(sizeof(cb::CreateResult)), o_ts = c.take(order == MergeOrder::lww ? n * 8 : 0);
  if (int rc = tmp.alloc(c, "device allocation failed for a merge's scratch")) return rc;
  m->dsrc = (cb::CompactSrc*)tmp.at(o_src);
  m->klen = (uint64_t*)tmp.at(o_klen);
  m->ko = (uint64_t*)tmp.at(o_ko);
  m->scan = (uint64_t*)tmp.at(o_scan);
  m->kb = tmp.at(o_kb);
  m->side = (cb::CompactSide*)tmp.at(o_side);
  m->order = (cb::SortKey*)tmp.at(o_order);
  m->sort = tmp.at(o_sort);
  m->slen = (uint64_t*)tmp.at(o_slen);
  m->tcnt = (uint64_t*)tmp.at(o_tcnt);
  m->tbytes = (uint64_t*)tmp.at(o_tbytes);
  m->tkeys = (uint64_t*)tmp.at(o_tkeys);
  m->tot = (uint64_t*)tmp.at(o_tot);
  m->dr = (cb::CreateResult*)tmp.at(o_res);
  m->ts = order == MergeOrder::lww ? (uint64_t*)tmp.at(o_ts) : nullptr;
  return CB_OK;
}
int enqueue_sort_begin(const Merge& m, hipStream_t s) {
  // the bin sort's inputs: an unsorted batch (flags[0]) and its prefix byte masks
  HIP_TRY(hipMemsetAsync(m.dr, 0, cb::kCreateHead, s));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&m.dr->flags[0], 1, 1, s));
  return CB_OK;
}
int enqueue_sort_select(const Merge& m, MergeRule rule, hipStream_t s) {
  const uint64_t n = m.n;
  // the stable sort by key, input index last: a key's lines leave it
  // adjacent, newest first
  if (int rc = enqueue_key_sort(m.plan, m.kb, m.ko, n, m.order, m.sort, m.dr, s, nullptr, nullptr, nullptr)) return rc;
  if (rule.order == MergeOrder::newest) {
    HIP_TRY(cb::launch_compact_select(m.order, m.side, m.kb, m.ko, n, rule.drop_dead, m.slen, m.tcnt, m.tbytes,
                                      m.tkeys, s));
    return CB_OK;
  }
  // (the sort moves records, not lines: ts is indexed like side, by input line)
  HIP_TRY(cb::launch_compact_ts(m.side, n, m.ts, s));
  HIP_TRY(cb::launch_compact_select_lww(m.order, m.side, m.ts, m.kb, m.ko, n, rule.drop_dead, m.slen, m.tcnt,
                                        m.tbytes, m.tkeys, s));
  return CB_OK;
}
int enqueue_merge_select(const Merge& m, const cb::CompactSrc* dsrc, uint32_t nsrc, MergeRule rule, hipStream_t s) {
  const uint64_t n = m.n;
  HIP_TRY(cb::launch_compact_klen(dsrc, nsrc, n, m.klen, s));
  HIP_TRY(cb::launch_scan_u64(m.klen, m.ko, n, m.scan, s));
  if (int rc = enqueue_sort_begin(m, s)) return rc;
  HIP_TRY(cb::launch_compact_gather(dsrc, nsrc, n, m.ko, m.kb, m.side, &m.dr->dmask[0][0], s));
  return enqueue_sort_select(m, rule, s);
}
int merge_totals(const Merge& m, hipStream_t s, uint64_t (&h)[3]) {
  HIP_TRY(cb::launch_tile_scan(m.tcnt, m.tiles, m.tot + 0, s));
  HIP_TRY(cb::launch_tile_scan(m.tbytes, m.tiles, m.tot + 1, s));
  HIP_TRY(cb::launch_tile_scan(m.tkeys, m.tiles, m.tot + 2, s));
  h[0] = h[1] = h[2] = 0;
  HIP_TRY(hipMemcpyAsync(h, m.tot, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] > m.n || h[2] > m.kbound || h[1] > m.kbound + m.n) return fail(CB_EHIP, "merge: inconsistent totals");
  return CB_OK;
}
int enqueue_merge(const Merge& m, const cb::CompactSrc* dsrc, uint32_t nsrc, MergeRule rule, hipStream_t s,
                  uint64_t (&h)[3]) {
  if (int rc = enqueue_merge_select(m, dsrc, nsrc, rule, s)) return rc;
  return merge_totals(m, s, h);
}

// ---- what a maker of a merged table does after the merge (cb_tables_compact's steps 3 and 5;
// cb_log_replay takes the same) ----

// 3: the survivors (h = {lines, file bytes, key bytes}) formatted into t: the
// file and its line index in one pass (the file is not re-read), and the kept
// keys beside them. No survivor: the file's buffer alone.
int format_survivors(cb_table* t, const Merge& mg, const uint64_t (&h)[3], TempBlock& keys, KeptKeys* k,
                     hipStream_t s) {
  const uint64_t cnt = h[0], len = h[1], kbytes = h[2];
  t->len = len;
  if (int rc = alloc_file(t, len + 16)) return rc;
  HIP_TRY(hipMemsetAsync(t->data + len, 0, 16, s));
  if (!cnt) return CB_OK;
  if (int rc = alloc_index(t, cnt)) return rc;
  cb::Carver c;
  const size_t o_kb = c.take(kbytes + 16), o_ko = c.take((cnt + 1) * 8);
  if (int rc = keys.alloc(c, "device allocation failed for a compaction's keys")) return rc;
  k->kb = keys.at(o_kb);
  k->ko = (uint64_t*)keys.at(o_ko);
  HIP_TRY(cb::launch_compact_format(mg.order, mg.side, mg.slen, mg.tcnt, mg.tbytes, mg.tkeys, mg.tot, mg.n, cnt,
                                    t->data, t->rec, t->pfx, t->fence, t->llen, k->kb, k->ko, s));
  return CB_OK;
}

// 5: the directory's map from the new prefixes (the merge's masks are
// reused) and the zone map's bounds, the first and last kept key: their
// offsets come back with the masks (one wait), their bytes after the
// directory is enqueued (one more: the zone bounds are host results).
int finish_compacted(cb_table* t, const Merge& mg, const KeptKeys& k, const uint64_t (&h)[3], hipStream_t s) {
  const uint64_t cnt = h[0], kbytes = h[2];
  uint64_t* dmask = &mg.dr->dmask[0][0];
  if (int rc = enqueue_pfx_masks(t, dmask, s)) return rc;
  uint64_t e[2] = {0, 0}, m[cb::kDirPos][4] = {};
  HIP_TRY(hipMemcpyAsync(&e[0], k.ko + 1, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&e[1], k.ko + cnt - 1, 8, hipMemcpyDeviceToHost, s));
  if (t->dir) HIP_TRY(hipMemcpyAsync(m, dmask, sizeof m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (e[0] > kbytes || e[1] > kbytes) return fail(CB_EHIP, "compaction: inconsistent key offsets");
  if (int rc = enqueue_directory(t, m, s)) return rc;
  t->zmin.resize(e[0]);
  t->zmax.resize(kbytes - e[1]);
  if (e[0]) HIP_TRY(hipMemcpyAsync(&t->zmin[0], k.kb, e[0], hipMemcpyDeviceToHost, s));
  if (kbytes - e[1]) HIP_TRY(hipMemcpyAsync(&t->zmax[0], k.kb + e[1], kbytes - e[1], hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // strictly increasing keys, a TAB on every line: by construction
  t->fast = !table_exact();
  t->has_zone = true;
  return CB_OK;
}

// A filter of no bits: BloomFilter::insert's `% 0` (src/bloom.rs:36).
int zero_m_error() { return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero"); }

}  // namespace cbx

namespace {

// ---- cb_tables_compact's steps, in the order it takes them ----

// 1: the sources: the non-empty tables, newest first, with their line bases;
// n their lines, kbound a bound on their keys' bytes.
int compact_sources(const cb_table* const* tables, uint32_t nt, std::vector<cb::CompactSrc>& srcs, uint64_t* n,
                    uint64_t* kbound) {
  if (int rc = for_live_tables(tables, nt, [&](cb_table* ti, uint32_t) {
        srcs.push_back(cb::CompactSrc{ti->data, ti->rec, ti->llen, *n});
        *n += ti->nlines;
        *kbound += ti->len;  // the keys' bytes are among the file's
      }))
    return rc;
  if (*n > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many lines for one compaction");
  return CB_OK;
}

// 2: the merge over the sources, staged into its scratch (one wait: the
// source is pageable), up to the survivors' totals h (enqueue_merge's wait).
// after (nullable): a step of the caller's between the select and the totals.
int merge_sources(const std::vector<cb::CompactSrc>& srcs, uint64_t n, uint64_t kbound, MergeRule rule,
                  const AfterSelect* after, TempBlock& tmp, Merge* mg, hipStream_t s, uint64_t (&h)[3]) {
  const uint32_t nsrc = (uint32_t)srcs.size();
  if (int rc = merge_alloc(nsrc, n, kbound, rule.order, tmp, mg)) return rc;
  HIP_TRY(hipMemcpyAsync(mg->dsrc, srcs.data(), nsrc * sizeof(cb::CompactSrc), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // the source is pageable
  if (!after) return enqueue_merge(*mg, mg->dsrc, nsrc, rule, s, h);
  if (int rc = enqueue_merge_select(*mg, mg->dsrc, nsrc, rule, s)) return rc;
  if (int rc = (*after)(*mg, s)) return rc;
  return merge_totals(*mg, s, h);
}

}  // namespace

// The live-row, LWW and ring compactions check their own arguments before they
// look at the table list (compact_tables looks at the list first): a filter of
// no bits is refused here, the outputs cleared. Without both outputs the
// refusal is compact_tables' own.
int cbx::zero_m_before_tables(uint64_t m_bits, cb_table** table_out, cb_filter** bloom_out) {
  if (!table_out || !bloom_out || m_bits != 0) return CB_OK;
  *table_out = nullptr;
  *bloom_out = nullptr;
  return zero_m_error();
}

// cb_tables_compact and, by their rules, cb_tables_compact_live and
// cb_tables_compact_lww: the same steps over the same merge, whose select
// alone knows the difference. cb_tables_compact_ring (capi_ring.cpp) takes
// them too, with its ownership filter as the step after the select.
int cbx::compact_tables(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, MergeRule rule,
                        const AfterSelect* after, void* stream, cb_table** table_out, cb_filter** bloom_out) {
  if (!table_out) return fail(CB_EINVAL, "null argument");
  *table_out = nullptr;
  if (bloom_out) *bloom_out = nullptr;
  int dev = 0;
  if (int rc = check_table_list(tables, nt, &dev)) return rc;
  if (bloom_out && m_bits == 0) return zero_m_error();
  hipStream_t s = (hipStream_t)stream;
  std::vector<cb::CompactSrc> srcs;
  uint64_t n = 0, kbound = 0;
  if (int rc = compact_sources(tables, nt, srcs, &n, &kbound)) return rc;
  int rc = cb_init(dev);
  if (rc) return rc;
  DeviceGuard dg(dev);
  Workspace& ws = workspace(dev, s);  // (registers s: the pool retires blocks behind it)
  std::unique_ptr<cb_table, int (*)(cb_table*)> t(new cb_table(), cb_table_destroy);
  std::unique_ptr<cb_filter, int (*)(cb_filter*)> f(nullptr, cb_filter_destroy);
  t->device = dev;
  if (bloom_out) {
    cb_filter* fp = nullptr;
    if ((rc = cb_filter_create(m_bits, dev, &fp))) return rc;
    f.reset(fp);
  }
  TempBlock tmp{dev}, keys{dev};
  uint64_t h[3] = {0, 0, 0};  // the survivors' lines, file bytes and key bytes
  if (n) {
    Merge mg;
    KeptKeys k;
    if ((rc = merge_sources(srcs, n, kbound, rule, after, tmp, &mg, s, h))) return rc;
    if ((rc = format_survivors(t.get(), mg, h, keys, &k, s))) return rc;
    if (h[0] && f) {
      // 4: BloomFilter::new(m) + insert per kept key (src/sstable.rs:59-63)
      std::lock_guard<std::mutex> lk(ws.mu);
      if ((rc = insert_locked(ws, f.get(), k.kb, k.ko, 0, h[0], s))) return rc;
    }
    if (h[0] && (rc = finish_compacted(t.get(), mg, k, h, s))) return rc;
  }
  // 6: no line survives: the empty file, as cb_sstable_create's n == 0
  if (!h[0] && (rc = finish_empty_file(t.get(), s))) return rc;
  if (bloom_out) *bloom_out = f.release();
  *table_out = t.release();
  return CB_OK;
}

extern "C" {

// Newest-wins merge (compact.hpp). Every temporary is carved from pool blocks
// released stream-ordered on return (error returns included: nothing the
// enqueued work touches is freed under it). The call waits for its own stream
// after staging the sources (pageable memory), for the survivors' totals (the
// output is sized from them), for the directory's map and at the end (the
// zone bounds are host results).
int cb_tables_compact(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, void* stream,
                      cb_table** table_out, cb_filter** bloom_out) {
  return compact_tables(tables, nt, m_bits, kNewest, nullptr, stream, table_out, bloom_out);
}

// The same with the live-row select: tombstones shadow and are then dropped
// (liverow.hpp). With no tombstone in the inputs it enqueues exactly what
// cb_tables_compact does.
// Like the other live-row entries it checks its own arguments before it looks
// at the table list (cb_tables_compact looks at the list first).
int cb_tables_compact_live(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, void* stream,
                           cb_table** table_out, cb_filter** bloom_out) {
  if (int rc = zero_m_before_tables(m_bits, table_out, bloom_out)) return rc;
  return compact_tables(tables, nt, m_bits, kLive, nullptr, stream, table_out, bloom_out);
}

// The LWW entries: the live-row entries' argument order (their own arguments
// before the table list, outputs cleared on every refusal) and the same steps
// under the lww order; drop_dead drops the winners that are tombstones.
int cb_tables_compact_lww(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, int drop_dead, void* stream,
                          cb_table** table_out, cb_filter** bloom_out) {
  if (int rc = zero_m_before_tables(m_bits, table_out, bloom_out)) return rc;
  return compact_tables(tables, nt, m_bits, MergeRule{MergeOrder::lww, drop_dead != 0}, nullptr, stream, table_out,
                        bloom_out);
}

}  // extern "C"
