// capi_scan.cpp — reading SSTables through the device merge (capi_merge.hpp):
// range and prefix scans, of one range or of many disjoint ones in one merge,
// into a result (cb_tables_scan*, scan.hpp), with the result's accessors
// (cb_scan_*). The live-row entries run the same steps: cb_tables_scan_live
// with the select that drops tombstones (liverow.hpp), cb_tables_count with
// the plain select and a counting kernel in place of the scan's tail. The LWW
// entries (cb_tables_scan_lww, cb_tables_count_lww) run them with the select
// that keeps a key's line of the greatest timestamp (rowts.hpp) in place of
// its newest one; cb_scan_ts reads the timestamps of any result. The WHERE
// entries (cb_tables_count_where, cb_scan_match, cb_row_matches) apply the row
// rule (rowjson.hpp): the count with a tail kernel that reads every live
// survivor's payload in place.
//
// Reference: src/lib.rs:125-146 (Database::get, whose answers a scan
// reproduces), src/cluster.rs:405-416, 454-459 (the read's fold by timestamp,
// which the LWW entries reproduce).
#include "capi_merge.hpp"
#include "keyrange.hpp"
#include "scan.hpp"

using namespace cbx;
using cb::MergeOrder;
using cb::MergeRule;

namespace {

// ---- the scan result ----

int scan_alloc(cb_scan* r, uint64_t count, uint64_t kb, uint64_t vb) {
  size_t o[5];
  const size_t bytes = cb::scan_layout(count, kb, vb, o);
  if (int rc = pool_alloc_or(r->device, bytes, &r->block, &r->block_cap,
                             "device allocation failed for a scan's result"))
    return rc;
  uint8_t* b = (uint8_t*)r->block;
  r->key_off = (uint64_t*)(b + o[0]);
  r->val_off = (uint64_t*)(b + o[1]);
  r->which = (int32_t*)(b + o[2]);
  r->keys = b + o[3];
  r->vals = b + o[4];
  return CB_OK;
}

// ---- the scan's steps, in the order scan_ranges takes them ----

// The ranges of one call (host memory, keyrange.hpp's list, already checked
// against its ordering rule): range r = [lo(r), hi(r)), the last one without
// a hi when last_unbounded.
struct RangeList {
  const uint8_t* bounds;
  const uint64_t* off;  // 2 nr + 1
  uint32_t nr;
  bool last_unbounded;
  const uint8_t* lo(uint32_t r) const { return bounds + off[2 * r]; }
  uint64_t lo_len(uint32_t r) const { return off[2 * r + 1] - off[2 * r]; }
  bool has_hi(uint32_t r) const { return r + 1 < nr || !last_unbounded; }
  const uint8_t* hi(uint32_t r) const { return bounds + off[2 * r + 1]; }
  uint64_t hi_len(uint32_t r) const { return has_hi(r) ? off[2 * r + 2] - off[2 * r + 1] : 0; }
  bool empty(uint32_t r) const { return has_hi(r) && cb::key_cmp(lo(r), lo_len(r), hi(r), hi_len(r)) >= 0; }
};

// The most cuts (ranges x non-empty tables) of one batched call:
// k_scan_sources is one block that walks them 256 at a time. (cb_tables_scan
// has no cap: its cuts are its tables.)
constexpr uint64_t kScanMaxCuts = 65536;

// What step 2 leaves on the device for the merge and the emit (in the call's
// `cuts` block), and the cuts' totals.
struct ScanCuts {
  const cb::CompactSrc* dsrc = nullptr;  // the cuts as the merge's sources
  const uint32_t* dmap = nullptr;        // each source's place in the caller's list
  const uint32_t* drng = nullptr;        // each source's range
  uint64_t n = 0, kbound = 0;            // lines inside the ranges, a bound on their keys' bytes
  uint32_t nsrc = 0;
};

// 1: the arguments of a scan of one range: the list, then the bounds (without
// has_hi, hi is ignored).
int check_scan_args(const cb_table* const* tables, uint32_t nt, const uint8_t* lo, uint64_t lo_len, const uint8_t* hi,
                    uint64_t* hi_len, int has_hi, int* dev) {
  if (int rc = check_table_list(tables, nt, dev)) return rc;
  if (lo_len && !lo) return fail(CB_EINVAL, "null lower bound with a length");
  if (!has_hi) *hi_len = 0;
  if (*hi_len && !hi) return fail(CB_EINVAL, "null upper bound with a length");
  return CB_OK;
}

// The list of a batched call (cb_tables_scan_many's format and ordering rule,
// keyrange.hpp), shared by every entry that takes one.
int check_range_list(const uint8_t* bounds, const uint64_t* bound_off, uint32_t nr, int last_unbounded) {
  if (!nr) return fail(CB_EINVAL, "no ranges");
  if (!bound_off) return fail(CB_EINVAL, "null bound offsets");
  if (!bounds)  // no byte may be read: every offset is the first, or the list is refused
    for (uint64_t i = 1; i <= 2ull * nr; ++i)
      if (bound_off[i] != bound_off[0]) return fail(CB_EINVAL, "null bounds with a non-zero total");
  if (cb::range_list_first_bad(bounds, bound_off, nr, last_unbounded != 0) >= 0)
    return fail(CB_EINVAL, "the ranges are not ascending and disjoint (or their offsets decrease)");
  return CB_OK;
}

// The tables a scan or a count searches: the non-empty ones, newest first,
// with their lines' and bytes' totals. *nothing: no device work can find an
// entry (no lines at all, or lo >= hi in every range).
struct ScanInput {
  std::vector<cb::ScanTable> tabs;
  uint64_t all_lines = 0, all_bytes = 0;
};
int scan_input(const cb_table* const* tables, uint32_t nt, const RangeList& rl, uint64_t max_cuts, ScanInput* in,
               bool* nothing) {
  if (int rc = for_live_tables(tables, nt, [&](cb_table* ti, uint32_t i) {
        in->tabs.push_back(cb::ScanTable{ti->data, ti->rec, ti->pfx, ti->fence, ti->llen, ti->nlines, ti->len, i, 0});
        in->all_lines += ti->nlines;
        in->all_bytes += ti->len;
      }))
    return rc;
  if (max_cuts && (uint64_t)rl.nr * in->tabs.size() > max_cuts)
    return fail(CB_EINVAL, "too many cuts (ranges x non-empty tables) for one scan");
  bool all_empty = true;
  for (uint32_t i = 0; all_empty && i < rl.nr; ++i) all_empty = rl.empty(i);
  *nothing = in->tabs.empty() || all_empty;
  return CB_OK;
}

// 2: every table's cut to every range, and the cuts as the merge's sources.
// Two waits: after staging the tables, the ranges and their bounds (pageable
// memory), and for the cuts' totals, checked against the tables' (all_lines,
// all_bytes: the ranges are disjoint, so a table's cuts share no line) before
// anything is sized from them.
int cut_tables(const std::vector<cb::ScanTable>& tabs, uint64_t all_lines, uint64_t all_bytes, const RangeList& rl,
               TempBlock& cuts, hipStream_t s, ScanCuts* out) {
  const uint32_t ntab = (uint32_t)tabs.size(), nr = rl.nr;
  const uint64_t ncut = (uint64_t)ntab * nr, at0 = rl.off[0], nbytes = rl.off[2 * (uint64_t)nr] - at0;
  Staging up;  // (the tables, the ranges and their bounds)
  cb::Carver& c = up.c;
  const size_t o_tab = c.take(ntab * sizeof(cb::ScanTable)), o_rng = c.take(nr * sizeof(cb::ScanRange)),
               o_bnd = c.take(nbytes + 16);
  up.seal();
  const size_t o_cut = c.take(ncut * sizeof(cb::ScanCut)), o_src = c.take(ncut * sizeof(cb::CompactSrc)),
               o_map = c.take(ncut * 4), o_rmap = c.take(ncut * 4), o_ctot = c.take(3 * 8);
  if (int rc = cuts.alloc(c, "device allocation failed for a scan's cuts")) return rc;
  up.put(o_tab, tabs.data(), ntab * sizeof(cb::ScanTable));
  cb::ScanRange* hr = (cb::ScanRange*)up.at(o_rng);
  for (uint32_t r = 0; r < nr; ++r) {
    const uint64_t lo_at = rl.off[2 * r] - at0;
    hr[r] = cb::ScanRange{lo_at, rl.lo_len(r), lo_at + rl.lo_len(r), rl.hi_len(r), rl.has_hi(r) ? 1u : 0u, 0};
    up.put(o_bnd + lo_at, rl.lo(r), rl.lo_len(r));
    up.put(o_bnd + hr[r].hi_at, rl.hi(r), rl.hi_len(r));
  }
  HIP_TRY(up.upload(cuts, s));
  HIP_TRY(hipStreamSynchronize(s));  // the source is pageable
  const cb::ScanTable* dtab = (const cb::ScanTable*)cuts.at(o_tab);
  cb::ScanCut* dcut = (cb::ScanCut*)cuts.at(o_cut);
  cb::CompactSrc* dsrc = (cb::CompactSrc*)cuts.at(o_src);
  uint32_t *dmap = (uint32_t*)cuts.at(o_map), *drng = (uint32_t*)cuts.at(o_rmap);
  uint64_t* dctot = (uint64_t*)cuts.at(o_ctot);
  HIP_TRY(cb::launch_scan_bounds(dtab, ntab, (const cb::ScanRange*)cuts.at(o_rng), nr, cuts.at(o_bnd), dcut, s));
  HIP_TRY(cb::launch_scan_sources(dtab, dcut, ntab, nr, dsrc, dmap, drng, dctot, s));
  uint64_t t[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(t, dctot, sizeof t, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t n = t[0], kbound = t[1], nsrc = t[2];
  if (n > all_lines || kbound > all_bytes || nsrc > ncut || nsrc > n || (n && !nsrc))
    return fail(CB_EHIP, "scan: inconsistent cut totals");
  if (n > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many lines inside the range for one scan");
  *out = ScanCuts{dsrc, dmap, drng, n, kbound, (uint32_t)nsrc};
  return CB_OK;
}

// 4: the result's block for `count` entries (room for kbytes key bytes and
// vcap value bytes) and, in it, the kept keys, their offsets and sources;
// the kept values' spans go into v, scratch in vtmp, for the decode. A scan
// of many ranges (nr > 1; count is then every survivor) also gets the
// entries' ranges and, from them, where each range begins (*droff, nr + 1
// offsets in vtmp).
int emit_scan_result(cb_scan* r, const Merge& mg, const ScanCuts& c, uint32_t nr, uint64_t count, uint64_t kbytes,
                     uint64_t vcap, TempBlock& vtmp, hipStream_t s, ValueSpans* v, const uint64_t** droff) {
  if (int rc = scan_alloc(r, count, kbytes, vcap)) return rc;
  const uint64_t vtiles = cb::get_tiles(count);
  cb::Carver vc;
  const size_t o_vsrc = vc.take(count * 8), o_dlen = vc.take(count * 8), o_vsum = vc.take(vtiles * 8),
               o_rid = vc.take(nr > 1 ? count * 4 : 0), o_roff = vc.take(nr > 1 ? (nr + 1ull) * 8 : 0);
  if (int rc = vtmp.alloc(vc, "device allocation failed for a scan's value spans")) return rc;
  uint64_t *vsrc = (uint64_t*)vtmp.at(o_vsrc), *dlen = (uint64_t*)vtmp.at(o_dlen), *vsum = (uint64_t*)vtmp.at(o_vsum);
  uint32_t* rid = nr > 1 ? (uint32_t*)vtmp.at(o_rid) : nullptr;
  HIP_TRY(hipMemsetAsync(vsum, 0, vtiles * 8, s));
  HIP_TRY(cb::launch_scan_emit(mg.order, mg.side, mg.slen, mg.tcnt, mg.tkeys, mg.tot, c.dsrc, c.dmap, c.drng, c.nsrc,
                               mg.n, count, r->keys, r->key_off, r->which, rid, vsrc, dlen, vsum, s));
  *droff = nullptr;
  if (nr > 1) {
    uint64_t* roff = (uint64_t*)vtmp.at(o_roff);
    HIP_TRY(cb::launch_scan_range_off(rid, count, nr, roff, s));
    *droff = roff;
  }
  *v = ValueSpans{vsrc, dlen, vsum, r->val_off};
  return CB_OK;
}

// 6: the kept keys' and values' byte totals and, for a scan of many ranges,
// the ranges' offsets (droff) (one wait: the result is complete when the call
// returns), checked against what the block was sized for.
int take_scan_totals(cb_scan* r, uint64_t count, uint64_t cnt, uint64_t kbytes, uint64_t vcap, const uint64_t* droff,
                     hipStream_t s) {
  uint64_t e[2] = {0, 0};
  std::vector<uint64_t>& ro = r->range_off;
  HIP_TRY(hipMemcpyAsync(&e[0], r->key_off + count, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&e[1], r->val_off + count, 8, hipMemcpyDeviceToHost, s));
  if (droff) HIP_TRY(hipMemcpyAsync(ro.data(), droff, ro.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (e[0] > kbytes || e[1] > vcap) return fail(CB_EHIP, "scan: inconsistent result totals");
  if (!droff) ro.back() = count;
  bool ok = ro.front() == 0 && ro.back() == count;
  for (size_t i = 0; ok && i + 1 < ro.size(); ++i) ok = ro[i] <= ro[i + 1];
  if (!ok) return fail(CB_EHIP, "scan: inconsistent range offsets");
  r->count = count;
  r->key_bytes = e[0];
  r->val_bytes = e[1];
  r->truncated = count < cnt;
  return CB_OK;
}

// 7: a limit's result was sized for the whole range: copied (and waited for)
// into a block of its own size, so what a caller keeps is sized by what it
// asked for.
int shrink_truncated(cb_scan* r, hipStream_t s) {
  size_t o[5];
  const uint64_t count = r->count, kb = r->key_bytes, vb = r->val_bytes;
  if (!r->truncated || cb::scan_layout(count, kb, vb, o) * 2 >= r->block_cap) return CB_OK;
  const cb_scan big = *r;
  TempBlock old{r->device, big.block, big.block_cap};
  r->block = nullptr;
  if (int rc = scan_alloc(r, count, kb, vb)) return rc;
  HIP_TRY(hipMemcpyAsync(r->key_off, big.key_off, (count + 1) * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(r->val_off, big.val_off, (count + 1) * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(r->which, big.which, count * 4, hipMemcpyDeviceToDevice, s));
  if (kb) HIP_TRY(hipMemcpyAsync(r->keys, big.keys, kb, hipMemcpyDeviceToDevice, s));
  if (vb) HIP_TRY(hipMemcpyAsync(r->vals, big.vals, vb, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// Offsets and bytes of a result into host or device memory (either may be NULL).
int scan_copy(const cb_scan* r, uint64_t* off_out, const uint64_t* off, uint8_t* out, const uint8_t* bytes,
              uint64_t nbytes) {
  if (!r) return fail(CB_EINVAL, "null scan");
  if (!r->count) {  // an empty result holds no device memory
    const uint64_t zero = 0;
    return off_out ? put_bytes((uint8_t*)off_out, &zero, 8) : CB_OK;
  }
  DeviceGuard dg(r->device);
  if (off_out) HIP_TRY(hipMemcpy(off_out, off, (r->count + 1) * 8, hipMemcpyDefault));
  if (out && nbytes) HIP_TRY(hipMemcpy(out, bytes, nbytes, hipMemcpyDefault));
  return CB_OK;
}

// ---- the scan itself ----

// Range scans (scan.hpp): the tables cut to every range on the device, the
// cuts merged as compaction merges whole tables, the survivors' keys and
// decoded values written into the result. One implementation: a scan of one
// range (cb_tables_scan, with its limit) is its nr = 1 case and skips the
// entries' ranges and their offsets. Scratch as in cb_tables_compact: pool
// blocks released stream-ordered on every return path. The call waits for its
// own stream after staging the table list (pageable memory) and then three
// times for a few words, each bound-checked before anything is sized from it:
// the cuts' totals (the merge's scratch), the survivors' totals (the result),
// and the kept keys' and values' byte totals at the end, with the ranges'
// offsets (the result is complete when the call returns); a truncated
// result's copy is one more.
// rule: the merge's select (compact.hpp). With drop_dead (cb_tables_scan_live)
// it keeps no tombstone, so every count, rank and offset below is of live
// entries; with the lww order (cb_tables_scan_lww) an entry is its key's line
// of the greatest timestamp, and `which` that line's table.
int scan_ranges(const cb_table* const* tables, uint32_t nt, int dev, const RangeList& rl, uint64_t max_cuts,
                uint64_t limit, MergeRule rule, hipStream_t s, void** out) {
  ScanInput in;
  bool nothing = false;
  if (int rc = scan_input(tables, nt, rl, max_cuts, &in, &nothing)) return rc;
  std::unique_ptr<cb_scan, int (*)(void*)> r(new cb_scan(), cb_scan_destroy);
  r->device = dev;
  r->range_off.assign(rl.nr + 1ull, 0);
  // an empty result: nothing to search (no lines at all, or lo >= hi in every
  // range), no line inside any range, or none that survives the merge
  auto done = [&] {
    *out = r.release();
    return CB_OK;
  };
  if (nothing) return done();
  int rc = cb_init(dev);
  if (rc) return rc;
  DeviceGuard dg(dev);
  (void)workspace(dev, s);  // (registers s: the pool retires blocks behind it)
  TempBlock cuts{dev}, tmp{dev}, vtmp{dev};
  ScanCuts c;
  if ((rc = cut_tables(in.tabs, in.all_lines, in.all_bytes, rl, cuts, s, &c))) return rc;
  if (!c.n) return done();
  // 3: compaction's merge over the cuts
  Merge mg;
  uint64_t h[3];
  if ((rc = merge_alloc(0, c.n, c.kbound, rule.order, tmp, &mg))) return rc;
  if ((rc = enqueue_merge(mg, c.dsrc, c.nsrc, rule, s, h))) return rc;
  const uint64_t cnt = h[0], len = h[1], kbytes = h[2];
  if (len < kbytes + 2 * cnt) return fail(CB_EHIP, "scan: inconsistent totals");
  if (!cnt) return done();
  // A kept line is `key \t text \n` and its value decodes to at most 3 bytes
  // per 4 of text, which bounds the values before any is decoded.
  const uint64_t count = limit && limit < cnt ? limit : cnt;
  const uint64_t vcap = (len - kbytes - 2 * cnt) / 4 * 3;
  ValueSpans v;
  const uint64_t* droff = nullptr;
  if ((rc = emit_scan_result(r.get(), mg, c, rl.nr, count, kbytes, vcap, vtmp, s, &v, &droff))) return rc;
  // 5: the read path's value tail
  if ((rc = enqueue_value_decode(v, count, r->vals, vcap, true, false, s))) return rc;
  if ((rc = take_scan_totals(r.get(), count, cnt, kbytes, vcap, droff, s))) return rc;
  if ((rc = shrink_truncated(r.get(), s))) return rc;
  return done();
}

// Counts per range without a result (cb_tables_count): the scan's cuts and
// the merge up to its plain select, then k_scan_count over the sorted records
// in place of everything a scan does from there on: no tile scans, no result
// block, no emit, no decode. The counters (2 nr words, zeroed by one memset)
// come back in one copy, the call's only wait after the cuts' totals, and are
// checked against the lines inside the ranges before they are handed out.
// order: which line of a key is its entry (cb_tables_count_lww: the winner by
// timestamp); no order drops anything here, live is counted beside entries.
// where (nullable; cb_tables_count_where): the tail is k_scan_count_where in
// place of k_scan_count, with a third counter per range, matched. The
// predicate and the ranges' skips travel as one small block, staged
// (stage_where) before the cuts so that the cuts' first wait covers it (the
// source is pageable): the call waits no more often than a count.
struct WhereCall {
  cb::WherePred pred;
  const uint32_t* skip;  // nr, or nullptr
};
// Where a count's results go (host, nr words each, zeroed by the caller;
// entries and live nullable, matched the WHERE count's only).
struct CountOut {
  uint64_t *entries, *live, *matched;
};
// The predicate and the ranges' skips in their block, enqueued only: `up` is
// read until the caller's next wait on s.
struct StagedWhere {
  const cb::WherePred* pred = nullptr;
  const uint32_t* skip = nullptr;
};
int stage_where(const WhereCall& w, uint32_t nr, TempBlock& blk, Staging& up, hipStream_t s, StagedWhere* out) {
  const size_t o_pred = up.c.take(sizeof(cb::WherePred)), o_skip = up.c.take(w.skip ? nr * 4ull : 0);
  up.seal();
  if (int rc = blk.alloc(up.c, "device allocation failed for a count's predicate")) return rc;
  up.put(o_pred, &w.pred, sizeof(cb::WherePred));
  if (w.skip) up.put(o_skip, w.skip, nr * 4ull);
  HIP_TRY(up.upload(blk, s));
  out->pred = (const cb::WherePred*)blk.at(o_pred);
  if (w.skip) out->skip = (const uint32_t*)blk.at(o_skip);
  return CB_OK;
}
int count_ranges(const cb_table* const* tables, uint32_t nt, int dev, const RangeList& rl, MergeOrder order,
                 hipStream_t s, const WhereCall* where, const CountOut& out) {
  ScanInput in;
  bool nothing = false;
  if (int rc = scan_input(tables, nt, rl, kScanMaxCuts, &in, &nothing)) return rc;
  if (nothing) return CB_OK;
  int rc = cb_init(dev);
  if (rc) return rc;
  DeviceGuard dg(dev);
  (void)workspace(dev, s);  // (registers s: the pool retires blocks behind it)
  TempBlock cuts{dev}, tmp{dev}, cnt{dev}, pred{dev};
  Staging up;  // (lives until the call's last wait)
  StagedWhere dw;
  if (where && (rc = stage_where(*where, rl.nr, pred, up, s, &dw))) return rc;
  ScanCuts c;
  if ((rc = cut_tables(in.tabs, in.all_lines, in.all_bytes, rl, cuts, s, &c))) {
    if (where) (void)hipStreamSynchronize(s);  // (a refusal before the cuts' first wait: `up` is still being read)
    return rc;
  }
  if (!c.n) return CB_OK;
  Merge mg;
  if ((rc = merge_alloc(0, c.n, c.kbound, order, tmp, &mg))) return rc;
  cb::Carver cc;
  const size_t per = where ? 3 : 2, words = per * (size_t)rl.nr, o_cnt = cc.take(words * 8);
  if ((rc = cnt.alloc(cc, "device allocation failed for a count's counters"))) return rc;
  uint64_t* dcnt = (uint64_t*)cnt.at(o_cnt);
  if ((rc = enqueue_merge_select(mg, c.dsrc, c.nsrc, MergeRule{order, false}, s))) return rc;
  HIP_TRY(hipMemsetAsync(dcnt, 0, words * 8, s));
  if (where)
    HIP_TRY(cb::launch_scan_count_where(mg.order, mg.side, mg.slen, c.dsrc, c.drng, c.nsrc, mg.n, rl.nr, dw.pred,
                                        dw.skip, dcnt, s));
  else
    HIP_TRY(cb::launch_scan_count(mg.order, mg.side, mg.slen, c.dsrc, c.drng, c.nsrc, mg.n, rl.nr, dcnt, s));
  std::vector<uint64_t> h(words, 0);
  HIP_TRY(hipMemcpyAsync(h.data(), dcnt, words * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint64_t all = 0;
  bool ok = true;
  for (uint32_t r = 0; ok && r < rl.nr; ++r) {
    ok = h[per * r] <= c.n - all && h[per * r + 1] <= h[per * r] && (!where || h[per * r + 2] <= h[per * r + 1]);
    all += h[per * r];
  }
  if (!ok) return fail(CB_EHIP, "count: inconsistent counters");
  for (uint32_t r = 0; r < rl.nr; ++r) {
    if (out.entries) out.entries[r] = h[per * r];
    if (out.live) out.live[r] = h[per * r + 1];
    if (where) out.matched[r] = h[per * r + 2];
  }
  return CB_OK;
}

// A cb_where checked and packed (rowjson.hpp): the three WHERE entries' first step.
int take_where(const void* where, cb::WherePred* pred) {
  const cb_where* w = (const cb_where*)where;
  if (!w) return fail(CB_EINVAL, "null predicate");
  if (const char* why = cb::where_check(w->cols, w->col_off, w->vals, w->val_off, w->part, w->nc))
    return fail(CB_EINVAL, why);
  cb::where_pack(w->cols, w->col_off, w->vals, w->val_off, w->part, w->nc, pred);
  return CB_OK;
}

// The arguments of an entry that takes a range list, to the device and the
// list. The two orders of refusal the entries have: the older ones
// (cb_tables_scan_many) look at the table list first, the live-row, LWW and
// WHERE ones at their own arguments first. A list of no ranges is refused by
// a scan (its result has a range) and nothing to do for a count: the list is
// then not looked at, and rl->nr == 0 tells the caller. A limit ranks within
// one range, so it is legal with one range only.
enum class ArgOrder { tables_first, own_first };
enum class NoRanges { refused, nothing };
int take_range_call(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                    uint32_t nr, int last_unbounded, uint64_t limit, ArgOrder order, NoRanges none, int* dev,
                    RangeList* rl) {
  if (order == ArgOrder::tables_first)
    if (int rc = check_table_list(tables, nt, dev)) return rc;
  if (nr || none == NoRanges::refused)
    if (int rc = check_range_list(bounds, bound_off, nr, last_unbounded)) return rc;
  if (limit && nr != 1) return fail(CB_EINVAL, "a limit takes exactly one range");
  if (order == ArgOrder::own_first)
    if (int rc = check_table_list(tables, nt, dev)) return rc;
  *rl = RangeList{bounds, bound_off, nr, last_unbounded != 0};
  return CB_OK;
}

// The scans of a range list: the result cleared, the arguments, the scan.
int scan_list(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off, uint32_t nr,
              int last_unbounded, uint64_t limit, ArgOrder order, MergeRule rule, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  int dev = 0;
  RangeList rl{};
  if (int rc = take_range_call(tables, nt, bounds, bound_off, nr, last_unbounded, limit, order, NoRanges::refused, &dev,
                               &rl))
    return rc;
  return scan_ranges(tables, nt, dev, rl, kScanMaxCuts, limit, rule, (hipStream_t)stream, out);
}

// The counts of a range list, after the entry has checked and zeroed its
// outputs (where: checked and packed too): the live-row entries' order.
int count_list(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
               uint32_t nr, int last_unbounded, MergeOrder order, void* stream, const WhereCall* where,
               const CountOut& out) {
  int dev = 0;
  RangeList rl{};
  if (int rc = take_range_call(tables, nt, bounds, bound_off, nr, last_unbounded, 0, ArgOrder::own_first,
                               NoRanges::nothing, &dev, &rl))
    return rc;
  if (!rl.nr) return CB_OK;
  return count_ranges(tables, nt, dev, rl, order, (hipStream_t)stream, where, out);
}

// cb_tables_count and cb_tables_count_lww: entries and live, either nullable.
int count_entries(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                  uint32_t nr, int last_unbounded, MergeOrder order, void* stream, uint64_t* entries, uint64_t* live) {
  if (!entries && !live) return fail(CB_EINVAL, "null argument");
  if (entries) std::fill(entries, entries + nr, 0);
  if (live) std::fill(live, live + nr, 0);
  return count_list(tables, nt, bounds, bound_off, nr, last_unbounded, order, stream, nullptr,
                    CountOut{entries, live, nullptr});
}

}  // namespace

extern "C" {

int cb_tables_scan(const cb_table* const* tables, uint32_t nt, const uint8_t* lo, uint64_t lo_len, const uint8_t* hi,
                   uint64_t hi_len, int has_hi, uint64_t limit, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  int dev = 0;
  if (int rc = check_scan_args(tables, nt, lo, lo_len, hi, &hi_len, has_hi, &dev)) return rc;
  // the list of one range: lo's bytes, then hi's
  std::vector<uint8_t> bounds(lo_len + hi_len);
  if (lo_len) std::memcpy(bounds.data(), lo, lo_len);
  if (hi_len) std::memcpy(bounds.data() + lo_len, hi, hi_len);
  const uint64_t off[3] = {0, lo_len, lo_len + hi_len};
  return scan_ranges(tables, nt, dev, RangeList{bounds.data(), off, 1, !has_hi}, 0, limit, kNewest, (hipStream_t)stream,
                     out);
}

int cb_tables_scan_many(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                        uint32_t nr, int last_unbounded, void* stream, void** out) {
  return scan_list(tables, nt, bounds, bound_off, nr, last_unbounded, 0, ArgOrder::tables_first, kNewest, stream, out);
}

// cb_tables_scan_many with the live-row select, and the call's own arguments
// before the table list, as in every live-row entry.
int cb_tables_scan_live(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                        uint32_t nr, int last_unbounded, uint64_t limit, void* stream, void** out) {
  return scan_list(tables, nt, bounds, bound_off, nr, last_unbounded, limit, ArgOrder::own_first, kLive, stream, out);
}

int cb_tables_count(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                    uint32_t nr, int last_unbounded, void* stream, uint64_t* entries, uint64_t* live) {
  return count_entries(tables, nt, bounds, bound_off, nr, last_unbounded, MergeOrder::newest, stream, entries, live);
}

// The LWW entries: the live-row entries' argument order (their own arguments
// before the table list, outputs cleared on every refusal) and the same steps
// under the lww order; drop_dead drops the winners that are tombstones.
int cb_tables_scan_lww(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                       uint32_t nr, int last_unbounded, int drop_dead, uint64_t limit, void* stream, void** out) {
  return scan_list(tables, nt, bounds, bound_off, nr, last_unbounded, limit, ArgOrder::own_first,
                   MergeRule{MergeOrder::lww, drop_dead != 0}, stream, out);
}

int cb_tables_count_lww(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                        uint32_t nr, int last_unbounded, void* stream, uint64_t* entries, uint64_t* live) {
  return count_entries(tables, nt, bounds, bound_off, nr, last_unbounded, MergeOrder::lww, stream, entries, live);
}

// cb_tables_count with the predicate's tail kernel. The live-row entries'
// order: the call's own arguments first, outputs cleared on every refusal.
int cb_tables_count_where(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds, const uint64_t* bound_off,
                          uint32_t nr, int last_unbounded, const uint32_t* skip, const void* w, int lww, void* stream,
                          uint64_t* live, uint64_t* matched) {
  if (live) std::fill(live, live + nr, 0);
  if (!matched) return fail(CB_EINVAL, "null argument");
  std::fill(matched, matched + nr, 0);
  auto wc = std::make_unique<WhereCall>();
  wc->skip = skip;
  if (int rc = take_where(w, &wc->pred)) return rc;
  return count_list(tables, nt, bounds, bound_off, nr, last_unbounded, lww ? MergeOrder::lww : MergeOrder::newest,
                    stream, wc.get(), CountOut{nullptr, live, matched});
}

// The verdicts of a finished result's entries (k_scan_match) into a scratch
// block on the null stream, then copied as cb_scan_ts copies. The predicate,
// the ranges' offsets and skips travel in the same block.
int cb_scan_match(const void* scan, const uint32_t* skip, const void* w, uint8_t* flags) {
  const cb_scan* r = (const cb_scan*)scan;
  auto pred = std::make_unique<cb::WherePred>();
  if (!flags) return fail(CB_EINVAL, "null argument");
  if (int rc = take_where(w, pred.get())) return rc;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (!r->count) return CB_OK;
  DeviceGuard dg(r->device);
  note_stream(r->device, nullptr);  // (the pool retires the scratch behind the null stream too)
  TempBlock tmp{r->device};
  const size_t nro = r->range_off.size(), nr = nro - 1;
  Staging up;
  cb::Carver& c = up.c;
  const size_t o_pred = c.take(sizeof(cb::WherePred)), o_roff = c.take(skip ? nro * 8 : 0),
               o_skip = c.take(skip ? nr * 4 : 0);
  up.seal();
  const size_t o_flags = c.take(r->count);
  if (int rc = tmp.alloc(c, "device allocation failed for a scan's verdicts")) return rc;
  up.put(o_pred, pred.get(), sizeof(cb::WherePred));
  if (skip) {
    up.put(o_roff, r->range_off.data(), nro * 8);
    up.put(o_skip, skip, nr * 4);
  }
  HIP_TRY(up.upload(tmp, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));  // the source is pageable
  uint8_t* dflags = tmp.at(o_flags);
  HIP_TRY(cb::launch_scan_match(r->key_off, r->keys, r->val_off, r->vals, r->count,
                                skip ? (const uint64_t*)tmp.at(o_roff) : nullptr,
                                skip ? (const uint32_t*)tmp.at(o_skip) : nullptr, (uint32_t)nr,
                                (const cb::WherePred*)tmp.at(o_pred), dflags, nullptr));
  HIP_TRY(hipMemcpy(flags, dflags, r->count, hipMemcpyDefault));
  return CB_OK;
}

int cb_row_matches(const uint8_t* key, uint64_t key_len, uint32_t skip, const uint8_t* value, uint64_t value_len,
                   const void* w, int* out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = 0;
  auto pred = std::make_unique<cb::WherePred>();
  if (int rc = take_where(w, pred.get())) return rc;
  if ((key_len && !key) || (value_len && !value)) return fail(CB_EINVAL, "null key or value with a length");
  cb::DecodedBytes v(value, value_len);
  *out = cb::row_matches(*pred, key, key_len, skip, v) ? 1 : 0;
  return CB_OK;
}

int cb_tables_scan_prefixes(const cb_table* const* tables, uint32_t nt, const uint8_t* prefixes,
                            const uint64_t* prefix_off, uint32_t np, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  int dev = 0;
  if (int rc = check_table_list(tables, nt, &dev)) return rc;
  if (!np) return fail(CB_EINVAL, "no prefixes");
  if (!prefix_off) return fail(CB_EINVAL, "null prefix offsets");
  if (!prefixes)
    for (uint64_t i = 1; i <= np; ++i)
      if (prefix_off[i] != prefix_off[0]) return fail(CB_EINVAL, "null prefixes with a non-zero total");
  std::vector<uint8_t> bounds;
  std::vector<uint64_t> off;
  bool last_unbounded = false;
  if (cb::prefix_list_to_ranges(prefixes, prefix_off, np, bounds, off, &last_unbounded) >= 0)
    return fail(CB_EINVAL, "a prefix without an end before the last one (or prefix offsets that decrease)");
  if (cb::range_list_first_bad(bounds.data(), off.data(), np, last_unbounded) >= 0)
    return fail(CB_EINVAL, "the prefixes are not ascending and disjoint");
  return scan_ranges(tables, nt, dev, RangeList{bounds.data(), off.data(), np, last_unbounded}, kScanMaxCuts, 0, kNewest,
                     (hipStream_t)stream, out);
}

int cb_key_prefix_end(const uint8_t* prefix, uint64_t len, uint8_t* out, uint64_t* out_len, int* has_end) {
  if ((len && (!prefix || !out)) || !out_len || !has_end) return fail(CB_EINVAL, "null argument");
  *has_end = cb::key_prefix_end(prefix, len, out, out_len) ? 1 : 0;
  return CB_OK;
}

int cb_tables_scan_prefix(const cb_table* const* tables, uint32_t nt, const uint8_t* prefix, uint64_t prefix_len,
                          uint64_t limit, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  if (prefix_len && !prefix) return fail(CB_EINVAL, "null prefix with a length");
  std::vector<uint8_t> end(prefix_len ? prefix_len : 1);
  uint64_t end_len = 0;
  const bool has_end = cb::key_prefix_end(prefix, prefix_len, end.data(), &end_len);
  return cb_tables_scan(tables, nt, prefix, prefix_len, end.data(), end_len, has_end ? 1 : 0, limit, stream, out);
}

int cb_scan_ranges(const void* scan, uint64_t* nr, uint64_t* range_off) {
  const cb_scan* r = (const cb_scan*)scan;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (nr) *nr = r->range_off.size() - 1;
  if (range_off) std::memcpy(range_off, r->range_off.data(), r->range_off.size() * 8);
  return CB_OK;
}

int cb_scan_info(const void* scan, uint64_t* count, uint64_t* key_bytes, uint64_t* val_bytes, int* truncated) {
  const cb_scan* r = (const cb_scan*)scan;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (count) *count = r->count;
  if (key_bytes) *key_bytes = r->key_bytes;
  if (val_bytes) *val_bytes = r->val_bytes;
  if (truncated) *truncated = r->truncated ? 1 : 0;
  return CB_OK;
}

int cb_scan_keys(const void* scan, uint64_t* key_off, uint8_t* keys) {
  const cb_scan* r = (const cb_scan*)scan;
  return scan_copy(r, key_off, r ? r->key_off : nullptr, keys, r ? r->keys : nullptr, r ? r->key_bytes : 0);
}

int cb_scan_values(const void* scan, uint64_t* val_off, uint8_t* vals) {
  const cb_scan* r = (const cb_scan*)scan;
  return scan_copy(r, val_off, r ? r->val_off : nullptr, vals, r ? r->vals : nullptr, r ? r->val_bytes : 0);
}

int cb_scan_which(const void* scan, int32_t* which) {
  const cb_scan* r = (const cb_scan*)scan;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (!r->count || !which) return CB_OK;
  DeviceGuard dg(r->device);
  HIP_TRY(hipMemcpy(which, r->which, r->count * 4, hipMemcpyDefault));
  return CB_OK;
}

// The entries' timestamps from their decoded values (k_scan_ts) into a
// scratch block on the null stream, then copied as cb_scan_which copies (the
// result was complete when its call returned, so nothing is waited for first).
int cb_scan_ts(const void* scan, uint64_t* ts) {
  const cb_scan* r = (const cb_scan*)scan;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (!r->count || !ts) return CB_OK;
  DeviceGuard dg(r->device);
  note_stream(r->device, nullptr);  // (the pool retires the scratch behind the null stream too)
  TempBlock tmp{r->device};
  cb::Carver c;
  const size_t o_ts = c.take(r->count * 8);
  if (int rc = tmp.alloc(c, "device allocation failed for a scan's timestamps")) return rc;
  uint64_t* dts = (uint64_t*)tmp.at(o_ts);
  HIP_TRY(cb::launch_scan_ts(r->val_off, r->vals, r->count, dts, nullptr));
  HIP_TRY(hipMemcpy(ts, dts, r->count * 8, hipMemcpyDefault));
  return CB_OK;
}

int cb_scan_destroy(void* scan) {
  cb_scan* r = (cb_scan*)scan;
  if (!r) return CB_OK;
  pool_release(r->device, r->block, r->block_cap);
  delete r;
  return CB_OK;
}

}  // extern "C"
