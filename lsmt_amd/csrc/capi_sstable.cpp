// capi_sstable.cpp — the C ABI for SSTable data files in HBM (SURVEY.md §8f
// rows 3 and 4): indexing an existing file (cb_table_create), SsTable::create
// on the device (cb_sstable_create), the batched binary search and
// Database::get's newest-first walk (cb_get_many_*), compaction
// (cb_tables_compact) and range scans (cb_tables_scan).
//
// Reference: /root/reference/src/sstable.rs:51-179, src/lib.rs:125-136.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <cstring>

#include "capi_internal.hpp"
#include "compact.hpp"
#include "keyrange.hpp"
#include "scan.hpp"

using namespace cbx;

namespace {

bool g_table_exact = false;  // cb_table_force_exact: index files for the exact-trajectory search only
std::atomic<uint64_t> g_bucket_limit{1ull << 30};  // cb_table_bucket_limit

// The most bytes a table's key buckets may take on this device now: the
// process-wide limit, and a quarter of the free device memory (the buckets
// are kept for the table's lifetime and must not starve later flushes).
uint64_t bucket_budget(int device) {
  const uint64_t lim = g_bucket_limit.load(std::memory_order_relaxed);
  if (!lim) return 0;
  size_t free_b = 0, total_b = 0;
  DeviceGuard dg(device);
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return std::min<uint64_t>(lim, free_b / 4);
}

int table_search_impl(const cb_table* t, const uint8_t* keys, const uint64_t* offsets,
                      uint32_t key_len, uint64_t n, int64_t* line_out, hipStream_t s) {
  if (!t || !line_out) return fail(CB_EINVAL, "null argument");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (n == 0) return CB_OK;
  DeviceGuard dg(t->device);
  Workspace& ws = workspace(t->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk);
  if (rc) return rc;
  int64_t* dl;
  if ((rc = out_buf(ws.t_line, line_out, n, s, &dl))) return rc;
  HIP_TRY(cb::launch_table_search(sk.keyk, t->view(), sk.ks, n, dl, s));
  return finish_out(line_out, dl, n * 8, sk.staged, s);
}

bool buckets_enabled() {
  static const bool off = cb::knob_int("CB_NO_BUCKETS", 0) == 1;
  return !off;
}

// The key buckets (sstable.hpp) for a read on stream s: the first read of a
// well-formed table enqueues their build on s and records bkt_ev after it.
// Until that event is seen complete, every read (on any stream, the building
// one included) enqueues a wait on it before using the buckets: the host never
// blocks, and no reader relies on stream-handle identity (the same handle can
// name another stream: hipStreamPerThread from two threads, or a destroyed
// stream's handle reused). A table whose bucket memory cannot be had is simply
// read without them. v receives bkt / bkbits.
int table_buckets(cb_table* t, hipStream_t s, cb::TableView* v) {
  int st = t->bkt_state.load(std::memory_order_acquire);
  if (st < 0 || (st == 0 && (!t->fast || !t->nlines || !buckets_enabled()))) return CB_OK;
  if (st == 1 || st == 0) {
    std::lock_guard<std::mutex> lk(t->bkt_mu);
    st = t->bkt_state.load(std::memory_order_relaxed);
    if (st == 0) {
      const uint32_t bits = cb::bkt_bits(t->nlines);
      const size_t bytes = (size_t)cb::bkt_bytes(bits);  // the buckets and their summary words
      if (bytes > bucket_budget(t->device) ||
          pool_alloc(t->device, bytes, (void**)&t->bkt, &t->bkt_cap) != hipSuccess) {
        t->bkt = nullptr;
        (void)hipGetLastError();
        t->bkt_state.store(-1, std::memory_order_release);
        return CB_OK;
      }
      t->bkbits = bits;
      // a failure past the allocation leaves the table without buckets for good
      // (the block is freed with the table) and reports the error once
      t->bkt_state.store(-1, std::memory_order_relaxed);
      HIP_TRY(hipMemsetAsync(t->bkt, 0xFF, bytes, s));
      HIP_TRY(cb::launch_table_buckets(t->rec, t->nlines, t->bkt, bits, s));
      HIP_TRY(hipEventCreateWithFlags(&t->bkt_ev, hipEventDisableTiming | hipEventDisableSystemFence));
      HIP_TRY(hipEventRecord(t->bkt_ev, s));
      t->bkt_state.store(st = 1, std::memory_order_release);
      // (s itself is ordered after the build: no wait needed on this call)
    } else if (st == 1) {
      if (hipEventQuery(t->bkt_ev) == hipSuccess) {
        t->bkt_state.store(st = 2, std::memory_order_release);
      } else {
        HIP_TRY(hipStreamWaitEvent(s, t->bkt_ev, 0));
      }
    }
  }
  if (st >= 1) cb::view_set_buckets(*v, t->bkt, t->bkbits);
  return CB_OK;
}

// How a get chooses each key's candidate tables. Each C entry pair builds
// its own; a field that is not its kind's stays NULL.
struct Gate {
  enum Kind { ROWS, SET, TIERS } kind;
  // ROWS (cb_get_many_*): table t is asked where hits has bit k of row
  // rows[t] (hits NULL: every table; then rows is not read)
  const uint64_t* hits;
  // ROWS: the tables' hit rows; SET: their slots (NULL: table t is row / slot t)
  const uint32_t* rows;
  // SET (cb_set_get_many_*): the gate comes from the FilterSet inside the
  // search kernel; a wide set takes the wide walk
  const cb_filterset* set;
  // TIERS (cb_tiers_get_many_*): the same over tiered sets, table t's tier
  // and slot from the list
  const TierList* tiers;
  static Gate of_rows(const uint64_t* hits, const uint32_t* rows) { return {ROWS, hits, rows, nullptr, nullptr}; }
  static Gate of_set(const cb_filterset* set, const uint32_t* slots) { return {SET, nullptr, slots, set, nullptr}; }
  static Gate of_tiers(const TierList* tl) { return {TIERS, nullptr, nullptr, nullptr, tl}; }
};

// Where a get's answers go (cassbloom.h cb_get_many_*). total == NULL:
// enqueue only (every buffer on the device; val_off[n] = the total).
struct GetOut {
  int32_t* which;
  uint64_t* val_off;
  uint8_t* vals;
  uint64_t cap;
  uint64_t* total;
  bool async() const { return total == nullptr; }
};

// The device side of one get: the tables' views and rows / slots, the
// answers (in place or in the workspace) and the value tail's scratch.
struct GetBufs {
  const cb::TableView* views;
  const uint32_t* rows;  // NULL: identity
  int32_t* which;
  uint64_t* voff;
  uint64_t *vsrc, *dlen, *tsum;
};

// The read path's two cache checks. Both are stream-ordered: earlier launches
// on s have read the old contents before new ones land.

// buf holds the bytes at src; uploaded only when they differ from `shadow`,
// the host copy of what buf holds (a call with the same tables, rows or
// groups uploads nothing).
int upload_if_changed(DevBuf& buf, std::vector<uint8_t>& shadow, const void* src, size_t bytes, hipStream_t s) {
  const uint8_t* b = (const uint8_t*)src;
  if (shadow.size() == bytes && !memcmp(shadow.data(), b, bytes)) return CB_OK;
  HIP_TRY(buf.reserve(bytes, s));
  HIP_TRY(hipMemcpyAsync(buf.p, b, bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // the source is pageable
  shadow.assign(b, b + bytes);
  return CB_OK;
}

// Device data made from the tables (the wide walk's screen and its copy of
// the maps): rebuilt by `build` when `sig`, what it would be made from now,
// differs from `held`, what it was made from.
template <class Build>
int rebuild_if_changed(std::vector<uint64_t>& held, std::vector<uint64_t>& sig, Build build) {
  if (sig == held) return CB_OK;
  if (int rc = build()) return rc;
  held.swap(sig);
  return CB_OK;
}

// The wide walk's screen for these tables in these slots (sstable.hpp
// WideScreen): built on s after their buckets, and kept in the stream's
// workspace until the tables, their slots or their buckets change (compared
// by the tables' process-unique ids). Only when the tables share one bucket
// count and the screen stays small; otherwise the walk runs without it.
// The most fingerprint bins (up to 256) whose screen fits kScreenMaxBytes.
// 300 tables of 1024 lines: 64 bins (a 2.6 MB screen) 1.91-1.92 G gets/s
// against 1.84-1.87 for 32 and 1.76-1.77 for 16; then 256 bins (10.5 MB)
// 1.92-1.99 against 1.89-1.92 for 64 and 1.90-1.96 for 128
// (experiments r05_wide5 and r05_wide6, HISTORY.md; alternating on one box).
constexpr uint32_t kScreenHbits = 8;
constexpr uint64_t kScreenMaxBytes = 16ull << 20;
int wide_screen(Workspace& ws, const cb_table* const* tables, const std::vector<cb::TableView>& views,
                const std::vector<uint32_t>& rows, uint32_t R, const cb::TableView* dviews, const uint32_t* drows,
                hipStream_t s, cb::WideScreen* out) {
  const uint32_t nt = (uint32_t)views.size();
  uint32_t hbits = kScreenHbits;
  static const bool off = cb::knob_int("CB_NO_SCREEN", 0) == 1;  // the A/B
  if (off) return CB_OK;
  static const int knob_h = cb::knob_int("CB_SCREEN_HBITS", -1);
  if (knob_h >= 0 && knob_h <= 8) hbits = (uint32_t)knob_h;
  uint32_t bits = 0;
  for (const auto& v : views)
    if (v.bkt && v.fast()) {
      bits = v.bkbits();
      break;
    }
  while (hbits > 4 && bits && cb::wide_screen_bytes(R, bits, hbits) > kScreenMaxBytes) --hbits;
  if (!bits || cb::wide_screen_bytes(R, bits, hbits) > kScreenMaxBytes) return CB_OK;
  std::vector<uint64_t> sig;
  sig.reserve(4 + 4 * (size_t)nt);
  sig.push_back(nt);
  sig.push_back(R);
  sig.push_back(bits);
  sig.push_back(hbits);
  for (uint32_t i = 0; i < nt; ++i) {
    sig.push_back(tables[i]->uid);
    sig.push_back(rows.empty() ? i : rows[i]);
    sig.push_back((uint64_t)(uintptr_t)views[i].bkt);
    sig.push_back(views[i].meta);
  }
  if (int rc = rebuild_if_changed(ws.w_scr_sig, sig, [&]() -> int {
        HIP_TRY(ws.w_scr.reserve(cb::wide_screen_bytes(R, bits, hbits), s));
        HIP_TRY(cb::launch_wide_screen(dviews, rows.empty() ? nullptr : drows, nt, R, bits, hbits,
                                       (uint64_t*)ws.w_scr.p, s));
        return CB_OK;
      }))
    return rc;
  *out = cb::WideScreen{(const uint64_t*)ws.w_scr.p, bits, hbits, 0};
  return CB_OK;
}

// ---- get_many_impl's steps, in the order it takes them ----

// 1: the arguments and, for an enqueue-only call, where they live. ta /
// gate_dev: a tiered gate's kernel argument and its sets' device.
int check_get_args(const cb_table* const* tables, uint32_t nt, const Gate& g, const uint8_t* keys,
                   const uint64_t* offsets, uint64_t n, const GetOut& o, cb::TierArgs* ta, int* gate_dev) {
  if (!o.which || !o.val_off || (nt && !tables)) return fail(CB_EINVAL, "null argument");
  if (g.kind == Gate::TIERS)
    if (int rc = tier_args(*g.tiers, nt, true, ta, gate_dev)) return rc;
  if (g.kind == Gate::SET) {
    if (nt > g.set->width) return fail(CB_EINVAL, "more tables than the set's slots");
    if (g.rows)
      for (uint32_t i = 0; i < nt; ++i)
        if (g.rows[i] >= g.set->width) return fail(CB_EINVAL, "slot out of range");
  }
  if (o.async() && (!is_device_ptr(o.which) || !is_device_ptr(o.val_off) || (o.vals && !is_device_ptr(o.vals)) ||
                    (g.hits && !is_device_ptr(g.hits)) || (n && keys && !is_device_ptr(keys)) ||
                    (offsets && !is_device_ptr(offsets))))
    return fail(CB_EINVAL, "total may be NULL only when keys, hits and outputs are device memory");
  return CB_OK;
}

// 2: no keys: val_off[0] = 0 and nothing else.
int answer_no_keys(const GetOut& o, hipStream_t s) {
  const uint64_t z = 0;
  if (o.async()) {
    HIP_TRY(hipMemsetAsync(o.val_off, 0, 8, s));
    return CB_OK;
  }
  return put_bytes((uint8_t*)o.val_off, &z, 8);
}

// 3: the tables as views (all on device dev, the caller's current device),
// the gate's sets on the same device, then each table's key buckets.
int tables_to_views(const cb_table* const* tables, uint32_t nt, int dev, const Gate& g, int gate_dev, hipStream_t s,
                    std::vector<cb::TableView>& views) {
  for (uint32_t i = 0; i < nt; ++i) {
    if (!tables[i]) return fail(CB_EINVAL, "null table");
    if (tables[i]->device != dev) return fail(CB_EINVAL, "tables live on different devices");
    if (int rc = finalize_table(const_cast<cb_table*>(tables[i]))) return rc;
    views[i] = tables[i]->view();
  }
  if (g.kind == Gate::SET && g.set->device != dev) return fail(CB_EINVAL, "set and tables live on different devices");
  if (g.kind == Gate::TIERS && gate_dev != dev) return fail(CB_EINVAL, "sets and tables live on different devices");
  for (uint32_t i = 0; i < nt; ++i)
    if (int rc = table_buckets(const_cast<cb_table*>(tables[i]), s, &views[i])) return rc;
  return CB_OK;
}

// 4: the keys as the kernels see them, the tables' rows / slots (empty:
// identity) and, for the ROWS gate, the hit rows on the device.
int stage_keys_and_rows(Workspace& ws, const Gate& g, uint32_t nt, const uint8_t* keys, const uint64_t* offsets,
                        uint32_t key_len, uint64_t n, hipStream_t s, StagedKeys& sk, std::vector<uint32_t>& rows,
                        const uint64_t** dhits) {
  uint64_t nrows = nt;
  if ((g.hits || g.kind == Gate::SET) && g.rows) {
    rows.assign(g.rows, g.rows + nt);
    nrows = 0;
    for (uint32_t r : rows) nrows = std::max<uint64_t>(nrows, (uint64_t)r + 1);
  }
  if (int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk)) return rc;
  *dhits = g.hits;
  if (g.hits && !is_device_ptr(g.hits)) {
    const uint64_t hbytes = nrows * ((n + 63) / 64) * 8;
    HIP_TRY(ws.hits.reserve(hbytes, s));
    HIP_TRY(hipMemcpyAsync(ws.hits.p, g.hits, hbytes, hipMemcpyHostToDevice, s));
    *dhits = (const uint64_t*)ws.hits.p;
  }
  return CB_OK;
}

// 5: views and rows to the device (when they changed), the answers' buffers
// and the tail's scratch.
int upload_tables(Workspace& ws, const std::vector<cb::TableView>& views, const std::vector<uint32_t>& rows,
                  const GetOut& o, uint64_t n, hipStream_t s, GetBufs* b) {
  if (int rc = upload_if_changed(ws.t_views, ws.t_views_host, views.data(), views.size() * sizeof(cb::TableView), s))
    return rc;
  b->views = (const cb::TableView*)ws.t_views.p;
  b->rows = nullptr;
  if (!rows.empty()) {
    if (int rc = upload_if_changed(ws.t_rows, ws.t_rows_host, rows.data(), rows.size() * 4, s)) return rc;
    b->rows = (const uint32_t*)ws.t_rows.p;
  }
  if (int rc = out_buf(ws.t_which, o.which, n, s, &b->which)) return rc;
  if (int rc = out_buf(ws.t_voff, o.val_off, n + 1, s, &b->voff)) return rc;
  HIP_TRY(ws.t_line.reserve(n * 8, s));
  HIP_TRY(ws.t_dlen.reserve(n * 8, s));
  HIP_TRY(ws.t_scan.reserve(cb::get_tiles(n) * 8, s));
  b->vsrc = (uint64_t*)ws.t_line.p;
  b->dlen = (uint64_t*)ws.t_dlen.p;
  b->tsum = (uint64_t*)ws.t_scan.p;
  return CB_OK;
}

// 6: the gate's launch, one function per gate.

int launch_rows_gate(const uint64_t* dhits, uint32_t nt, const StagedKeys& sk, uint64_t n, const GetBufs& b,
                     hipStream_t s) {
  HIP_TRY(cb::launch_get_many(sk.keyk, b.views, nt, dhits, b.rows, (n + 63) / 64, sk.ks, n, b.which, b.vsrc, b.dlen,
                              b.tsum, s));
  return CB_OK;
}

int launch_set_gate(const cb_filterset* set, uint32_t nt, const StagedKeys& sk, uint64_t n, const GetBufs& b,
                    hipStream_t s) {
  const cb::ZoneView zv = set_zone_view(set);
  HIP_TRY(cb::launch_set_get_many(sk.keyk, set->mode, set->width, set->words, set->mp, set->zany ? &zv : nullptr,
                                  b.views, nt, b.rows, sk.ks, n, b.which, b.vsrc, b.dlen, b.tsum, s));
  return set->zany ? note_zone_read(set, s) : CB_OK;
}

int launch_tier_gate(const TierList& tl, const cb::TierArgs& ta, const StagedKeys& sk, uint64_t n, const GetBufs& b,
                     hipStream_t s) {
  HIP_TRY(cb::launch_tier_get_many(sk.keyk, ta, b.views, sk.ks, n, b.which, b.vsrc, b.dlen, b.tsum, s));
  return note_tier_reads(tl, ta, s);
}

// The wide gate takes its groups, its screen and its copy of the maps with it.
int launch_wide_gate(Workspace& ws, const cb_filterset* set, const cb_table* const* tables,
                     const std::vector<cb::TableView>& views, const std::vector<uint32_t>& rows,
                     const StagedKeys& sk, uint64_t n, const GetBufs& b, hipStream_t s) {
  const uint32_t nt = (uint32_t)views.size();
  // the groups of 64 tables (newest first) and how each maps to slots:
  // ascending or descending runs take their candidate bits from one window
  // of the rows (wideset.hpp WideGroup), anything else one bit per table
  const uint32_t ng = (nt + 63) / 64;
  std::vector<cb::WideGroup> groups(ng);
  bool need_slots = false;
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t t0 = 64 * g, gn = std::min<uint32_t>(64, nt - t0);
    auto slot = [&](uint32_t i) { return rows.empty() ? t0 + i : rows[t0 + i]; };
    bool asc = true, desc = true;
    for (uint32_t i = 1; i < gn; ++i) {
      asc = asc && slot(i) == slot(0) + i;
      desc = desc && slot(i) + i == slot(0);
    }
    cb::WideGroup& gd = groups[g];
    gd.gn = gn;
    if (asc) {
      gd.kind = 0;
      gd.lo = slot(0);
    } else if (desc) {
      gd.kind = 1;
      gd.lo = slot(gn - 1);
    } else {
      gd.kind = 2;
      gd.lo = 0;
      need_slots = true;
    }
  }
  if (int rc = upload_if_changed(ws.t_groups, ws.t_groups_host, groups.data(), ng * sizeof(cb::WideGroup), s))
    return rc;
  const cb::WideZone wz = wide_zone_view(set);
  cb::WideScreen scr{nullptr, 0, 0, 0};
  if (int rc = wide_screen(ws, tables, views, rows, set->R, b.views, b.rows, s, &scr)) return rc;
  // the tables' DirMaps in one contiguous array (gathered on the device
  // when the table list changes: the walk stages a group's maps in the same
  // pass as its views)
  std::vector<uint64_t> msig;
  msig.reserve(2 * (size_t)nt);
  for (uint32_t i = 0; i < nt; ++i) {
    msig.push_back(tables[i]->uid);
    msig.push_back((uint64_t)(uintptr_t)views[i].dmap);
  }
  if (int rc = rebuild_if_changed(ws.t_maps_sig, msig, [&]() -> int {
        HIP_TRY(ws.t_maps.reserve((size_t)nt * sizeof(cb::DirMap), s));
        HIP_TRY(cb::launch_gather_maps(b.views, nt, (cb::DirMap*)ws.t_maps.p, s));
        return CB_OK;
      }))
    return rc;
  const cb::DirMap* dmaps = (const cb::DirMap*)ws.t_maps.p;
  // the A/B: maps found through the views (the round-5 staging)
  static const bool no_maps = cb::knob_int("CB_WIDE_MAPS", 1) == 0;
  if (no_maps) dmaps = nullptr;
  HIP_TRY(cb::launch_wide_get_many(sk.keyk, set->mode, set->R, (const uint64_t*)set->words, set->mp,
                                   set->zany ? &wz : nullptr, b.views, nt, (const cb::WideGroup*)ws.t_groups.p,
                                   need_slots ? b.rows : nullptr, sk.ks, n, b.which, b.vsrc, b.dlen, b.tsum, s,
                                   scr.scr ? &scr : nullptr, dmaps));
  return set->zany ? note_zone_read(set, s) : CB_OK;
}

// 7: the value tail, the same after every gate: the found values' offsets
// (the tile sums' scan), their decode, and the answers back to the host.
int value_tail(Workspace& ws, const GetBufs& b, uint64_t n, const GetOut& o, hipStream_t s) {
  // batches of up to 256K keys: the decode scans the tile sums itself (one
  // launch fewer per batch); larger ones: the one-block scan between
  bool raw = n && n <= cb::decode_raw_max();  // (n = 0: the scan kernel writes voff[0] = 0)
  static const bool no_raw = cb::knob_int("CB_DECODE_RAW", 1) == 0;
  if (no_raw) raw = false;
  if (!raw) HIP_TRY(cb::launch_tile_scan(b.tsum, cb::get_tiles(n), b.voff + n, s));
  if (!ws.htot) HIP_TRY(hipHostMalloc((void**)&ws.htot, kHostScratch, hipHostMallocDefault));
  if (o.async()) {
    HIP_TRY(cb::launch_b64_decode(b.vsrc, b.dlen, b.tsum, n, b.voff, o.vals, o.vals ? o.cap : 0, s, raw));
    return CB_OK;
  }
  if (o.vals && is_device_ptr(o.vals)) {
    // device values: offsets and values in one pass (the kernel skips the
    // value writes when the total exceeds cap): one host round trip
    HIP_TRY(cb::launch_b64_decode(b.vsrc, b.dlen, b.tsum, n, b.voff, o.vals, o.cap, s, raw));
    HIP_TRY(hipMemcpyAsync(ws.htot, b.voff + n, 8, hipMemcpyDeviceToHost, s));
  } else {
    HIP_TRY(cb::launch_b64_decode(b.vsrc, b.dlen, b.tsum, n, b.voff, nullptr, 0, s, raw));  // offsets only
    HIP_TRY(hipMemcpyAsync(ws.htot, b.voff + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t tot = *ws.htot;
    if (o.vals && o.cap >= tot && tot) {
      uint8_t* dvals;
      if (int rc = out_buf(ws.t_vals, o.vals, tot, s, &dvals)) return rc;
      HIP_TRY(cb::launch_b64_decode(b.vsrc, b.dlen, b.tsum, n, b.voff, dvals, tot, s, raw));
      HIP_TRY(hipMemcpyAsync(o.vals, dvals, tot, hipMemcpyDeviceToHost, s));
    }
  }
  if (b.which != o.which) HIP_TRY(hipMemcpyAsync(o.which, b.which, n * 4, hipMemcpyDeviceToHost, s));
  if (b.voff != o.val_off) HIP_TRY(hipMemcpyAsync(o.val_off, b.voff, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *o.total = *ws.htot;
  return CB_OK;
}

// Database::get for a batch of keys over tables[0..nt) (tables[0] newest),
// the candidates chosen by gate g (cb_get_many_*, cb_set_get_many_*,
// cb_tiers_get_many_*).
int get_many_impl(const cb_table* const* tables, uint32_t nt, const Gate& g, const uint8_t* keys,
                  const uint64_t* offsets, uint32_t key_len, uint64_t n, const GetOut& o, hipStream_t s) {
  cb::TierArgs ta;
  int gate_dev = 0;
  if (int rc = check_get_args(tables, nt, g, keys, offsets, n, o, &ta, &gate_dev)) return rc;
  if (o.total) *o.total = 0;
  if (n == 0) return answer_no_keys(o, s);
  if (int rc = null_keys(keys, offsets, key_len)) return rc;  // (here: ahead of the table checks)
  if (nt == 0) return fail(CB_EINVAL, "no tables");
  const int dev = tables[0] ? tables[0]->device : 0;
  DeviceGuard dg(dev);
  std::vector<cb::TableView> views(nt);
  if (int rc = tables_to_views(tables, nt, dev, g, gate_dev, s, views)) return rc;
  Workspace& ws = workspace(dev, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  std::vector<uint32_t> rows;
  const uint64_t* dhits;
  if (int rc = stage_keys_and_rows(ws, g, nt, keys, offsets, key_len, n, s, sk, rows, &dhits)) return rc;
  GetBufs b;
  if (int rc = upload_tables(ws, views, rows, o, n, s, &b)) return rc;
  int rc = CB_OK;
  switch (g.kind) {
    case Gate::ROWS: rc = launch_rows_gate(dhits, nt, sk, n, b, s); break;
    case Gate::SET:
      rc = set_is_wide(g.set) ? launch_wide_gate(ws, g.set, tables, views, rows, sk, n, b, s)
                              : launch_set_gate(g.set, nt, sk, n, b, s);
      break;
    case Gate::TIERS: rc = launch_tier_gate(*g.tiers, ta, sk, n, b, s); break;
  }
  if (rc) return rc;
  return value_tail(ws, b, n, o, s);
}

// The index of nl lines is one allocation: rec | pfx | fence | dir | dmap | llen.
size_t dir_bytes(uint64_t nl) { return cb::dir_words(nl) ? ((cb::dir_words(nl) * 4 + 15) & ~15ull) : 0; }
size_t index_bytes(uint64_t nl) {
  return nl * sizeof(cb::LineRec) + nl * 8 + cb::fence_words(nl) * 8 + 8 + dir_bytes(nl) +
         (cb::dir_words(nl) ? sizeof(cb::DirMap) : 0) + nl * 4;
}
void carve_index(cb_table* t) {
  const uint64_t nl = t->nlines;
  t->pfx = (uint64_t*)(t->rec + nl);
  t->fence = t->pfx + nl;
  // 16-B aligned: the read path copies the map into LDS in 16-B words
  uint8_t* d = (uint8_t*)(((uintptr_t)(t->fence + cb::fence_words(nl)) + 15) & ~(uintptr_t)15);
  t->dir = cb::dir_words(nl) ? (uint32_t*)d : nullptr;
  t->dmap = nullptr;  // set once the directory is written (make_dirmap needs every prefix)
  t->llen = (uint32_t*)(d + (t->dir ? dir_bytes(nl) + sizeof(cb::DirMap) : 0));
}
cb::DirMap* dmap_slot(const cb_table* t) {
  return t->dir ? (cb::DirMap*)((uint8_t*)t->dir + dir_bytes(t->nlines)) : nullptr;
}

// ---- the steps every maker of a table shares (cb_table_create's index_table,
// cb_sstable_create's sstable_enqueue / finalize_locked, cb_tables_compact) ----

// The file's buffer (the file and its 16 bytes of slack, or a bound on them)
// and the index of nl lines, from the pool; a failure leaves the pointer null.
int alloc_file(cb_table* t, uint64_t bytes) {
  if (pool_alloc(t->device, bytes, (void**)&t->data, &t->data_cap) != hipSuccess) {
    t->data = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for an SSTable buffer");
  }
  return CB_OK;
}
int alloc_index(cb_table* t, uint64_t nl) {
  t->nlines = nl;
  if (pool_alloc(t->device, index_bytes(nl), (void**)&t->rec, &t->rec_cap) != hipSuccess) {
    t->rec = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for an SSTable index");
  }
  carve_index(t);
  return CB_OK;
}
void drop_index(cb_table* t) {
  pool_release(t->device, t->rec, t->rec_cap);
  t->rec = nullptr;
  t->pfx = t->fence = nullptr;
  t->dir = t->llen = nullptr;
  t->dmap = nullptr;
  t->nlines = 0;
}

// Bin-sort group target: ~n / 1536 records (six 1024-record group sorts per
// CU on 256 CUs, one wave), at least 640, at most 1536 (2048-record sorts).
uint32_t bin_group_target(uint64_t n) {
  static const int knob = cb::knob_int("CB_BIN_T", -1);  // group size target (tuning); 0 disables the bin sort
  if (knob >= 0) return (uint32_t)knob;
  return (uint32_t)std::min<uint64_t>(1536, std::max<uint64_t>(640, (n + 1535) / 1536));
}

// The stable sort of n keys: the bin sort for batches past one merge-sort tile
// (its fallback, the merge sort, enqueued behind it), the merge sort alone
// for smaller ones and past 2^24.
struct SortPlan {
  bool binned;
  uint32_t T;          // the bin sort's group target
  uint64_t tmp_bytes;  // the scratch enqueue_key_sort needs
};
SortPlan plan_key_sort(uint64_t n) {
  const uint32_t T = bin_group_target(n);
  const bool binned = T && T <= cb::bin_sort_max_group() && n > 4096 && n <= (1ull << 24);
  return SortPlan{binned, T, binned ? cb::bin_sort_tmp_bytes(n, T) : cb::entry_sort_tmp_bytes(n)};
}
// order = the records of (kb, ko) in stable key order, on s. Every launch
// returns at once unless dr->flags[0] says the batch is unsorted; the merge
// sort behind a bin sort runs only when that set dr->flags[3] (one bin, or a
// bin larger than an LDS tile: keys sharing a long prefix), and then rewrites
// the records, value spans and tile sums whole. vo == nullptr: no value tail
// (vsp and tsum are not written).
int enqueue_key_sort(const SortPlan& plan, const uint8_t* kb, const uint64_t* ko, uint64_t n, cb::SortKey* order,
                     void* tmp, cb::CreateResult* dr, hipStream_t s, const uint64_t* vo, ulonglong2* vsp,
                     uint64_t* tsum) {
  const auto& [binned, T, tmp_bytes] = plan;
  if (binned) HIP_TRY(cb::launch_bin_sort(kb, ko, n, T, order, tmp, s, vo, vsp, tsum, dr));
  HIP_TRY(cb::launch_entry_sort(order, (cb::SortKey*)tmp, n, kb, ko, s, vo, vsp, tsum, &dr->flags[binned ? 3 : 0]));
  return CB_OK;
}

// A pool block that is scratch for one call: released stream-ordered when it
// leaves scope, on every return path.
struct TempBlock {
  int dev;
  void* p = nullptr;
  size_t cap = 0;
  ~TempBlock() { pool_release(dev, p, cap); }
};

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
  cb::CreateResult* dr = nullptr;
};
int merge_alloc(int dev, uint32_t nsrc_cap, uint64_t n, uint64_t kbound, TempBlock& tmp, Merge* m) {
  m->n = n;
  m->kbound = kbound;
  m->tiles = cb::compact_tiles(n);
  m->plan = plan_key_sort(n);  // the order: sorted as cb_sstable_create sorts a batch
  size_t at = 0;
  auto take = [&](uint64_t bytes) {
    const size_t o = at;
    at += (size_t)((bytes + 15) & ~15ull);
    return o;
  };
  const size_t o_src = take(nsrc_cap * sizeof(cb::CompactSrc)), o_klen = take(n * 8), o_ko = take((n + 1) * 8),
               o_scan = take(cb::scan_tmp_words(n) * 8), o_kb = take(kbound + 16),
               o_side = take(n * sizeof(cb::CompactSide)), o_order = take(n * sizeof(cb::SortKey)),
               o_sort = take(m->plan.tmp_bytes), o_slen = take(n * 8), o_tcnt = take(m->tiles * 8),
               o_tbytes = take(m->tiles * 8), o_tkeys = take(m->tiles * 8), o_tot = take(3 * 8),
               o_res = take(sizeof(cb::CreateResult));
  if (pool_alloc(dev, at, &tmp.p, &tmp.cap) != hipSuccess) {
    tmp.p = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for a merge's scratch");
  }
  uint8_t* b = (uint8_t*)tmp.p;
  m->dsrc = (cb::CompactSrc*)(b + o_src);
  m->klen = (uint64_t*)(b + o_klen);
  m->ko = (uint64_t*)(b + o_ko);
  m->scan = (uint64_t*)(b + o_scan);
  m->kb = b + o_kb;
  m->side = (cb::CompactSide*)(b + o_side);
  m->order = (cb::SortKey*)(b + o_order);
  m->sort = b + o_sort;
  m->slen = (uint64_t*)(b + o_slen);
  m->tcnt = (uint64_t*)(b + o_tcnt);
  m->tbytes = (uint64_t*)(b + o_tbytes);
  m->tkeys = (uint64_t*)(b + o_tkeys);
  m->tot = (uint64_t*)(b + o_tot);
  m->dr = (cb::CreateResult*)(b + o_res);
  return CB_OK;
}
// The merge of sources dsrc[0..nsrc) (device, m.n lines in all) on s, up to
// the survivors' totals h = {lines, file bytes, key bytes}: read back (they
// size the caller's output), the stream waited for, and checked against the
// inputs' bounds before anything is sized from them.
int enqueue_merge(const Merge& m, const cb::CompactSrc* dsrc, uint32_t nsrc, hipStream_t s, uint64_t (&h)[3]) {
  const uint64_t n = m.n;
  HIP_TRY(cb::launch_compact_klen(dsrc, nsrc, n, m.klen, s));
  HIP_TRY(cb::launch_scan_u64(m.klen, m.ko, n, m.scan, s));
  // the bin sort's inputs: an unsorted batch (flags[0]) and its prefix byte masks
  HIP_TRY(hipMemsetAsync(m.dr, 0, cb::kCreateHead, s));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&m.dr->flags[0], 1, 1, s));
  HIP_TRY(cb::launch_compact_gather(dsrc, nsrc, n, m.ko, m.kb, m.side, &m.dr->dmask[0][0], s));
  // the stable sort by key, input index last: a key's lines leave it
  // adjacent, newest first
  if (int rc = enqueue_key_sort(m.plan, m.kb, m.ko, n, m.order, m.sort, m.dr, s, nullptr, nullptr, nullptr)) return rc;
  HIP_TRY(cb::launch_compact_select(m.order, m.side, m.kb, m.ko, n, m.slen, m.tcnt, m.tbytes, m.tkeys, s));
  HIP_TRY(cb::launch_tile_scan(m.tcnt, m.tiles, m.tot + 0, s));
  HIP_TRY(cb::launch_tile_scan(m.tbytes, m.tiles, m.tot + 1, s));
  HIP_TRY(cb::launch_tile_scan(m.tkeys, m.tiles, m.tot + 2, s));
  h[0] = h[1] = h[2] = 0;
  HIP_TRY(hipMemcpyAsync(h, m.tot, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] > n || h[2] > m.kbound || h[1] > m.kbound + n) return fail(CB_EHIP, "merge: inconsistent totals");
  return CB_OK;
}

// The directory of a table whose prefixes are written, in two halves around
// the caller's one copy-back and wait: the byte values of every prefix
// position into dmask (device, kDirMaskBytes), then, from their host copy,
// the map and the directory itself. Nothing for a table too small for one.
constexpr size_t kDirMaskBytes = sizeof(cb::CreateResult::dmask);
int enqueue_pfx_masks(const cb_table* t, uint64_t* dmask, hipStream_t s) {
  if (!t->dir) return CB_OK;
  HIP_TRY(hipMemsetAsync(dmask, 0, kDirMaskBytes, s));
  HIP_TRY(cb::launch_pfx_masks(t->pfx, t->nlines, dmask, s));
  return CB_OK;
}
int enqueue_directory(cb_table* t, const uint64_t (&masks)[cb::kDirPos][4], hipStream_t s) {
  if (!t->dir) return CB_OK;
  t->dmap = dmap_slot(t);
  HIP_TRY(cb::launch_table_dir(t->pfx, t->nlines, cb::make_dirmap(masks, t->nlines), t->dir, t->dmap, s));
  return CB_OK;
}

// An empty table's file: 16 zero bytes (allocated here unless the caller
// has), complete on return.
int finish_empty_file(cb_table* t, hipStream_t s) {
  if (!t->data)
    if (int rc = alloc_file(t, 16)) return rc;
  HIP_TRY(hipMemsetAsync(t->data, 0, 16, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// Line index of t->data[0..t->len) (count -> scan -> emit -> finish -> keys).
// Temporaries come from the stream's workspace (taken here: callers must not
// hold its lock); the index itself is one allocation: rec | pfx | fence.
int index_table(cb_table* t, hipStream_t s) {
  const uint64_t len = t->len;
  if (!len) return CB_OK;
  Workspace& ws = workspace(t->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  const uint64_t nb = cb::line_blocks(len);
  HIP_TRY(ws.i_cnt.reserve(nb * 8, s));
  HIP_TRY(ws.i_base.reserve((nb + 1) * 8, s));
  HIP_TRY(ws.i_tmp.reserve(cb::scan_tmp_words(nb) * 8, s));
  HIP_TRY(ws.i_err.reserve(16 + kDirMaskBytes, s));  // error words, then the prefix byte masks
  uint64_t* cnt = (uint64_t*)ws.i_cnt.p;
  uint64_t* base = (uint64_t*)ws.i_base.p;
  uint32_t* err = (uint32_t*)ws.i_err.p;
  HIP_TRY(cb::launch_line_count(t->data, len, cnt, s));
  HIP_TRY(cb::launch_scan_u64(cnt, base, nb, (uint64_t*)ws.i_tmp.p, s));
  HIP_TRY(hipMemcpyAsync(&t->nlines, base + nb, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!t->nlines) return CB_OK;
  const uint64_t nl = t->nlines;
  if (int rc = alloc_index(t, nl)) return rc;
  HIP_TRY(ws.i_start.reserve(nl * 8, s));
  HIP_TRY(ws.i_end.reserve(nl * 8, s));
  uint64_t* start = (uint64_t*)ws.i_start.p;
  uint64_t* end = (uint64_t*)ws.i_end.p;
  HIP_TRY(hipMemsetAsync(end, 0xFF, nl * 8, s));
  HIP_TRY(hipMemsetAsync(err, 0, 4, s));
  const uint32_t one = 1;
  HIP_TRY(hipMemcpyAsync(err + 1, &one, 4, hipMemcpyHostToDevice, s));
  HIP_TRY(cb::launch_line_emit(t->data, len, base, start, end, s));
  HIP_TRY(cb::launch_line_finish(t->data, len, nl, start, end, t->rec, t->llen, err, s));
  // prefix + fence index, value validity and the well-formed check (sstable.hpp)
  HIP_TRY(cb::launch_line_keys(t->data, nl, t->rec, t->llen, t->pfx, t->fence, err + 1, s));
  // the byte values of every prefix position (the directory's map)
  if (int rc = enqueue_pfx_masks(t, (uint64_t*)(err + 4), s)) return rc;
  // the error words and the masks in one pinned copy, one wait
  if (!ws.htot) HIP_TRY(hipHostMalloc((void**)&ws.htot, kHostScratch, hipHostMallocDefault));
  HIP_TRY(hipMemcpyAsync(ws.htot, err, 16 + (t->dir ? kDirMaskBytes : 0), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint32_t e[2];
  memcpy(e, ws.htot, 8);
  if (e[0]) return fail(CB_EINVAL, "an SSTable line is 4 GiB or longer");
  t->fast = e[1] != 0 && !g_table_exact;
  if (!e[1]) return CB_OK;  // not well-formed: no directory (it needs sorted prefixes)
  uint64_t m[cb::kDirPos][4];
  memcpy(m, ws.htot + 2, sizeof m);
  return enqueue_directory(t, m, s);
}

// ---- SsTable::create: enqueue now, finalise on first use ----
//
// cb_sstable_create only enqueues its kernels (sortedness check, Bloom
// build, the sort the device picks, tile scan, format) and one copy of the
// CreateResult into a pinned block, followed by an event; nothing waits. The
// host-side results (file length, zone bounds, the well-formed flag) are read
// when the table is first used (finalize_table). One case needs the host
// there: a key holding '\n' or '\t' (the file is re-indexed the way
// SsTable::get splits it). A batch the bin sort cannot place (one bin, or a
// bin larger than an LDS tile) is sorted again on the device, by the merge
// sort enqueued after it that runs only then. Until a table is finalised its inputs must stay valid (host
// inputs are staged into a block the table owns).

// Pinned result blocks and their events, reused across tables.
struct ResultSlot {
  cb::CreateResult* h = nullptr;
  hipEvent_t ev = nullptr;
};
std::mutex g_res_mu;
std::vector<ResultSlot> g_res_free;

int result_slot(ResultSlot* out) {
  {
    std::lock_guard<std::mutex> lk(g_res_mu);
    if (!g_res_free.empty()) {
      *out = g_res_free.back();
      g_res_free.pop_back();
      return CB_OK;
    }
  }
  ResultSlot r;
  HIP_TRY(hipHostMalloc((void**)&r.h, sizeof(cb::CreateResult), hipHostMallocDefault));
  // host-waited after a copy into pinned memory: the default (system-scope) release
  HIP_TRY(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
  *out = r;
  return CB_OK;
}

void result_release(cb::CreateResult* h, hipEvent_t ev) {
  if (!h) return;
  std::lock_guard<std::mutex> lk(g_res_mu);
  g_res_free.push_back(ResultSlot{h, ev});
}

}  // namespace

TablePending::~TablePending() {
  if (staged) pool_release(device, staged, staged_cap);
  result_release(hres, ev);
}

namespace {

// The format pass and everything after the sort, on s (ws.mu held).
int enqueue_format(cb_table* t, Workspace& ws, const TablePending& p, cb::CreateResult* dr, hipStream_t s) {
  const uint64_t n = p.n;
  uint64_t* tsum = (uint64_t*)ws.f_tsum.p;
  const bool inline_scan = cb::format_tiles(n) <= cb::kFormatInlineTiles;  // small flushes: no scan launch
  if (!inline_scan) HIP_TRY(cb::launch_tile_scan(tsum, cb::format_tiles(n), &dr->len, s));
  HIP_TRY(cb::launch_format((const cb::SortKey*)ws.f_sk2.p, p.dk, p.dko, p.dv, p.dvo, tsum, n, t->data, t->rec,
                            t->pfx, t->fence, t->llen, dr, p.cap_bytes, s, (const ulonglong2*)ws.f_vsp.p, t->dir,
                            t->dir ? dmap_slot(t) : nullptr, inline_scan));
  return CB_OK;
}

int sstable_enqueue(const uint8_t* keys, const uint64_t* key_off, uint64_t kbytes, const uint8_t* vals,
                    const uint64_t* val_off, uint64_t vbytes, uint64_t n, uint64_t m_bits, int device, hipStream_t s,
                    cb_table** table_out, cb_filter** bloom_out) {
  *table_out = nullptr;
  if (bloom_out) *bloom_out = nullptr;
  if (n >= 0xFFFFFFFFull) return fail(CB_EINVAL, "too many entries for one table");
  int rc = cb_init(device);
  if (rc) return rc;
  if (bloom_out && n && m_bits == 0)  // BloomFilter::insert's `% 0` (src/bloom.rs:36)
    return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  if ((kbytes && !keys) || (vbytes && !vals)) return fail(CB_EINVAL, "null bytes");
  DeviceGuard dg(device);
  std::unique_ptr<cb_table, int (*)(cb_table*)> t(new cb_table(), cb_table_destroy);
  std::unique_ptr<cb_filter, int (*)(cb_filter*)> f(nullptr, cb_filter_destroy);
  t->device = device;
  std::unique_ptr<TablePending> pend(new TablePending());
  TablePending& p = *pend;
  p.device = device;
  p.n = n;
  // an error return past this point may leave work enqueued that reads the
  // staged block or writes the result slot: finish the stream before `pend`
  // hands them back (declared after pend, so it runs first)
  // (armed only at the first enqueue: a refusal before it — bad offsets,
  // bounds, a failed allocation — returns without blocking on the caller's
  // stream)
  struct SyncOnError {
    hipStream_t s;
    bool ok = true;
    ~SyncOnError() {
      if (!ok) (void)hipStreamSynchronize(s);
    }
  } on_error{s};
  // Host inputs go into one block the table owns (the work reads them after
  // this call returns, and a fallback sort at finalisation reads them again);
  // device inputs are used in place.
  const bool ko_h = !is_device_ptr(key_off), vo_h = !is_device_ptr(val_off);
  const bool kb_h = kbytes && !is_device_ptr(keys), vb_h = vbytes && !is_device_ptr(vals);
  if (ko_h)
    for (uint64_t i = 0; i < n; ++i)
      if (key_off[i + 1] < key_off[i]) return fail(CB_EINVAL, "offsets must be non-decreasing");
  if (vo_h)
    for (uint64_t i = 0; i < n; ++i)
      if (val_off[i + 1] < val_off[i]) return fail(CB_EINVAL, "offsets must be non-decreasing");
  if ((kb_h && !ko_h) || (vb_h && !vo_h)) {
    // host bytes with device offsets: they are staged into exactly kbytes /
    // vbytes, so offsets past those would send every kernel past the staged
    // block. Check the totals before anything is enqueued (one read-back).
    uint64_t tot[2] = {0, 0};
    if (kb_h && !ko_h) HIP_TRY(hipMemcpyAsync(&tot[0], key_off + n, 8, hipMemcpyDeviceToHost, s));
    if (vb_h && !vo_h) HIP_TRY(hipMemcpyAsync(&tot[1], val_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] > kbytes) return fail(CB_EINVAL, "key bytes exceed key_bytes");
    if (tot[1] > vbytes) return fail(CB_EINVAL, "value bytes exceed val_bytes");
  }
  auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
  const uint64_t offb = up16((n + 1) * 8);
  const uint64_t stage = (ko_h ? offb : 0) + (vo_h ? offb : 0) + (kb_h ? up16(kbytes) : 0) + (vb_h ? up16(vbytes) : 0);
  if (stage) {
    if (pool_alloc(device, stage, &p.staged, &p.staged_cap) != hipSuccess) {
      p.staged = nullptr;
      return fail(CB_ENOMEM, "device allocation failed for a staged flush batch");
    }
    on_error.ok = false;  // the staging copies are the first enqueued work
    uint8_t* at = (uint8_t*)p.staged;
    auto put = [&](const void* src, uint64_t bytes) -> uint8_t* {
      uint8_t* d = at;
      at += up16(bytes);
      return d;
    };
    if (ko_h) {
      uint8_t* d = put(key_off, (n + 1) * 8);
      HIP_TRY(hipMemcpyAsync(d, key_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
      key_off = (const uint64_t*)d;
    }
    if (vo_h) {
      uint8_t* d = put(val_off, (n + 1) * 8);
      HIP_TRY(hipMemcpyAsync(d, val_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
      val_off = (const uint64_t*)d;
    }
    if (kb_h) {
      uint8_t* d = put(keys, kbytes);
      HIP_TRY(hipMemcpyAsync(d, keys, kbytes, hipMemcpyHostToDevice, s));
      keys = d;
    }
    if (vb_h) {
      uint8_t* d = put(vals, vbytes);
      HIP_TRY(hipMemcpyAsync(d, vals, vbytes, hipMemcpyHostToDevice, s));
      vals = d;
    }
  }
  p.dk = keys;
  p.dko = key_off;
  p.dv = vals;
  p.dvo = val_off;
  // the file's buffer: sum(k + 2 + 4 ceil(v / 3)) <= K + 2n + (4V + 8n) / 3,
  // plus slack; its length comes back with the results
  p.cap_bytes = kbytes + 2 * n + (4 * vbytes + 8 * n) / 3 + 1 + 16;
  if ((rc = alloc_file(t.get(), p.cap_bytes))) return rc;
  if (!n) {  // an empty file: nothing to sort, index or bound
    on_error.ok = false;
    if (bloom_out) {
      cb_filter* fp = nullptr;
      if ((rc = cb_filter_create(m_bits, device, &fp))) return rc;
      *bloom_out = fp;
    }
    t->pend = std::move(pend);  // (no result block: the staged block is released with the table)
    if ((rc = finish_empty_file(t.get(), s))) return rc;
    on_error.ok = true;
    *table_out = t.release();
    return CB_OK;
  }
  if ((rc = alloc_index(t.get(), n))) return rc;
  ResultSlot slot;
  if ((rc = result_slot(&slot))) return rc;
  p.hres = slot.h;
  p.ev = slot.ev;
  on_error.ok = false;  // from here on every step enqueues
  Workspace& ws = workspace(device, s);
  std::unique_lock<std::mutex> lk(ws.mu);
  HIP_TRY(ws.f_flag.reserve(sizeof(cb::CreateResult), s));
  HIP_TRY(ws.f_tsum.reserve(cb::format_tiles(n) * 8, s));
  HIP_TRY(ws.f_sk2.reserve(n * sizeof(cb::SortKey), s));
  HIP_TRY(ws.f_vsp.reserve(n * sizeof(ulonglong2), s));
  cb::CreateResult* dr = (cb::CreateResult*)ws.f_flag.p;
  uint64_t* tsum = (uint64_t*)ws.f_tsum.p;
  HIP_TRY(hipMemsetAsync(dr, 0, cb::kCreateHead, s));
  HIP_TRY(cb::launch_sorted_check(p.dk, p.dko, p.dvo, n, dr, tsum, kbytes, vbytes, s));
  // the Bloom build needs neither the order nor the totals (OR is order-free)
  if (bloom_out) {
    cb_filter* fp = nullptr;
    if ((rc = cb_filter_create(m_bits, device, &fp))) return rc;
    f.reset(fp);
    if ((rc = insert_locked(ws, fp, p.dk, p.dko, 0, n, s))) return rc;
  }
  // the stable sort by key, enqueued before anyone knows whether the batch
  // needs one: every sort launch returns at once for a sorted batch (memtable
  // flushes arrive sorted)
  const SortPlan plan = plan_key_sort(n);
  HIP_TRY(ws.f_sort.reserve(plan.tmp_bytes, s));
  if ((rc = enqueue_key_sort(plan, p.dk, p.dko, n, (cb::SortKey*)ws.f_sk2.p, ws.f_sort.p, dr, s, p.dvo,
                             (ulonglong2*)ws.f_vsp.p, tsum)))
    return rc;
  if ((rc = enqueue_format(t.get(), ws, p, dr, s))) return rc;
  HIP_TRY(hipMemcpyAsync(p.hres, dr, sizeof(cb::CreateResult), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(p.ev, s));
  lk.unlock();
  t->dmap = t->dir ? dmap_slot(t.get()) : nullptr;
  t->pend = std::move(pend);
  t->ready.store(false, std::memory_order_release);
  on_error.ok = true;
  if (bloom_out) *bloom_out = f.release();
  *table_out = t.release();
  return CB_OK;
}

// Release what a finalised (or destroyed) table no longer needs.
void drop_pending(cb_table* t) {
  t->pend.reset();  // (~TablePending returns the staged block and the result slot)
}

int finalize_locked(cb_table* t) {
  TablePending& p = *t->pend;
  DeviceGuard dg(t->device);
  if (p.ev) HIP_TRY(hipEventSynchronize(p.ev));
  if (!p.n) return CB_OK;
  cb::CreateResult* hr = p.hres;
  if (hr->flags[4]) {
    t->ferr = CB_EINVAL;
    t->ferr_msg = "SsTable::create: the batch's key or value bytes exceed the bounds the table was sized from";
    return CB_OK;
  }
  // (hr->flags[3]: the bin sort could not place the batch and the merge sort
  // ran after it on the create's stream; the file is already written)
  t->len = hr->len;
  // zone map: ZoneMap::update over the sorted keys = first / last line
  t->zidx[0] = hr->idx_min;
  t->zidx[1] = hr->idx_max;
  for (int w = 0; w < 2; ++w) {
    const uint64_t kl = hr->zlen[w];
    std::string& z = w ? t->zmax : t->zmin;
    z.assign((const char*)hr->zkey[w], (size_t)std::min<uint64_t>(kl, cb::kZoneInline));
    if (kl > cb::kZoneInline) {  // a long key: the rest in one more copy
      const uint64_t i = w ? hr->idx_max : hr->idx_min;
      uint64_t o = 0;
      HIP_TRY(hipMemcpy(&o, p.dko + i, 8, hipMemcpyDeviceToHost));
      z.resize(kl);
      HIP_TRY(hipMemcpy(&z[cb::kZoneInline], p.dk + o + cb::kZoneInline, kl - cb::kZoneInline,
                        hipMemcpyDeviceToHost));
    }
  }
  t->has_zone = true;
  if (hr->flags[1]) {
    // a key holds '\n' or '\t': the file's lines are not the entries, so
    // index it the way SsTable::get splits it (src/sstable.rs:142-146)
    drop_index(t);
    int rc = index_table(t, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
  } else {
    t->fast = !hr->flags[2] && !g_table_exact;
  }
  return CB_OK;
}

}  // namespace

namespace cbx {

int finalize_table(cb_table* t) {
  if (!t->ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(t->fin_mu);
    if (!t->ready.load(std::memory_order_acquire)) {
      const int rc = finalize_locked(t);
      drop_pending(t);
      if (rc && !t->ferr) {
        t->ferr = rc;
        t->ferr_msg = cbx::g_err;
      }
      t->ready.store(true, std::memory_order_release);
    }
  }
  return t->ferr ? fail(t->ferr, t->ferr_msg.c_str()) : CB_OK;
}

}  // namespace cbx

extern "C" {

// ---- SSTable data files and the batched read path ----

int cb_table_destroy(cb_table* t) {
  if (!t) return CB_OK;
  {
    DeviceGuard dg(t->device);
    if (t->pend) {  // enqueued work may still be running: let it finish first
      std::lock_guard<std::mutex> lk(t->fin_mu);
      if (t->pend->ev && !t->ready.load()) (void)hipEventSynchronize(t->pend->ev);
      drop_pending(t);
    }
    pool_release(t->device, t->data, t->data_cap);
    pool_release(t->device, t->rec, t->rec_cap);  // rec heads the one index allocation
    if (t->bkt) pool_release(t->device, t->bkt, t->bkt_cap);
    if (t->bkt_ev) (void)hipEventDestroy(t->bkt_ev);
  }
  delete t;
  return CB_OK;
}

int cb_table_create(const uint8_t* data, uint64_t len, int device, void* stream, cb_table** out) {
  if (!out || (!data && len)) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  int rc = cb_init(device);
  if (rc) return rc;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  note_stream(device, s);
  std::unique_ptr<cb_table, int (*)(cb_table*)> t(new cb_table(), cb_table_destroy);
  t->device = device;
  t->len = len;
  if ((rc = alloc_file(t.get(), len + 16))) return rc;
  HIP_TRY(hipMemsetAsync(t->data + len, 0, 16, s));
  if (len) HIP_TRY(hipMemcpyAsync(t->data, data, len, hipMemcpyDefault, s));
  if ((rc = index_table(t.get(), s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  *out = t.release();
  return CB_OK;
}

int cb_table_data(const cb_table* t, const uint8_t** data, uint64_t* len) {
  if (!t) return fail(CB_EINVAL, "null table");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (data) *data = t->data;
  if (len) *len = t->len;
  return CB_OK;
}

int cb_table_copy(const cb_table* t, uint64_t offset, uint64_t len, uint8_t* out) {
  if (!t || (!out && len)) return fail(CB_EINVAL, "null argument");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (offset > t->len || len > t->len - offset) return fail(CB_EINVAL, "range outside the file");
  if (!len) return CB_OK;
  DeviceGuard dg(t->device);
  HIP_TRY(hipMemcpy(out, t->data + offset, len, hipMemcpyDefault));
  return CB_OK;
}

int cb_sstable_create(const uint8_t* keys, const uint64_t* key_off, const uint8_t* vals,
                      const uint64_t* val_off, uint64_t n, uint64_t m_bits, int device, void* stream,
                      cb_table** table_out, cb_filter** bloom_out, uint64_t* zone_min_idx,
                      uint64_t* zone_max_idx) {
  if (!table_out || !key_off || !val_off) return fail(CB_EINVAL, "null argument");
  if (zone_min_idx) *zone_min_idx = ~0ull;
  if (zone_max_idx) *zone_max_idx = ~0ull;
  // byte totals: host offsets carry them; device offsets are read back (one
  // round trip: cb_sstable_create_bounded takes the bounds instead)
  uint64_t kt = 0, vt = 0;
  const bool kdev = is_device_ptr(key_off), vdev = is_device_ptr(val_off);
  if (kdev || vdev) {
    int rc = cb_init(device);
    if (rc) return rc;
    DeviceGuard dg(device);
    hipStream_t s = (hipStream_t)stream;
    uint64_t tot[2] = {0, 0};
    if (kdev) HIP_TRY(hipMemcpyAsync(&tot[0], key_off + n, 8, hipMemcpyDeviceToHost, s));
    if (vdev) HIP_TRY(hipMemcpyAsync(&tot[1], val_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    kt = tot[0];
    vt = tot[1];
  }
  if (!kdev) kt = key_off[n];
  if (!vdev) vt = val_off[n];
  int rc = sstable_enqueue(keys, key_off, kt, vals, val_off, vt, n, m_bits, device, (hipStream_t)stream, table_out,
                           bloom_out);
  if (rc || !(zone_min_idx || zone_max_idx) || !n) return rc;
  // the zone map's input indices are host values: wait for them
  cb_table* t = *table_out;
  if ((rc = finalize_table(t))) {
    cb_table_destroy(t);
    *table_out = nullptr;
    if (bloom_out && *bloom_out) {
      cb_filter_destroy(*bloom_out);
      *bloom_out = nullptr;
    }
    return rc;
  }
  if (zone_min_idx) *zone_min_idx = t->zidx[0];
  if (zone_max_idx) *zone_max_idx = t->zidx[1];
  return CB_OK;
}

int cb_sstable_create_bounded(const uint8_t* keys, const uint64_t* key_off, uint64_t key_bytes, const uint8_t* vals,
                              const uint64_t* val_off, uint64_t val_bytes, uint64_t n, uint64_t m_bits, int device,
                              void* stream, cb_table** table_out, cb_filter** bloom_out) {
  if (!table_out || !key_off || !val_off) return fail(CB_EINVAL, "null argument");
  if (!is_device_ptr(key_off) && key_off[n] > key_bytes) return fail(CB_EINVAL, "key bytes exceed key_bytes");
  if (!is_device_ptr(val_off) && val_off[n] > val_bytes) return fail(CB_EINVAL, "value bytes exceed val_bytes");
  return sstable_enqueue(keys, key_off, key_bytes, vals, val_off, val_bytes, n, m_bits, device, (hipStream_t)stream,
                         table_out, bloom_out);
}

int cb_table_wait(const cb_table* t) {
  if (!t) return fail(CB_EINVAL, "null table");
  return finalize_table(const_cast<cb_table*>(t));
}

int cb_table_rebuild(const cb_table* t, uint64_t m_bits, void* stream, cb_filter** bloom_out,
                     uint64_t* zone_min_line, uint64_t* zone_max_line) {
  if (!t || !bloom_out) return fail(CB_EINVAL, "null argument");
  *bloom_out = nullptr;
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (zone_min_line) *zone_min_line = ~0ull;
  if (zone_max_line) *zone_max_line = ~0ull;
  hipStream_t s = (hipStream_t)stream;
  cb_filter* fp = nullptr;
  int rc = cb_filter_create(m_bits, t->device, &fp);  // BloomFilter::new(1024) (src/sstable.rs:111)
  if (rc) return rc;
  std::unique_ptr<cb_filter, int (*)(cb_filter*)> f(fp, cb_filter_destroy);
  const uint64_t nl = t->nlines;
  if (nl) {
    DeviceGuard dg(t->device);
    Workspace& ws = workspace(t->device, s);
    std::lock_guard<std::mutex> lk(ws.mu);
    HIP_TRY(ws.i_cnt.reserve((nl + 1) * 8, s));
    HIP_TRY(ws.i_base.reserve((nl + 1) * 8, s));
    HIP_TRY(ws.i_start.reserve((nl + 1) * 8, s));
    HIP_TRY(ws.i_end.reserve((nl + 1) * 8, s));
    HIP_TRY(ws.i_tmp.reserve(cb::scan_tmp_words(nl) * 8, s));
    HIP_TRY(ws.i_err.reserve(8, s));
    uint64_t* has = (uint64_t*)ws.i_cnt.p;
    uint64_t* has_scan = (uint64_t*)ws.i_base.p;
    uint64_t* klen = (uint64_t*)ws.i_start.p;
    uint64_t* len_scan = (uint64_t*)ws.i_end.p;
    uint64_t* bad = (uint64_t*)ws.i_err.p;
    HIP_TRY(hipMemsetAsync(bad, 0xFF, 8, s));
    HIP_TRY(cb::launch_rebuild_mark(t->data, t->rec, nl, has, klen, bad, s));
    HIP_TRY(cb::launch_scan_u64(has, has_scan, nl, (uint64_t*)ws.i_tmp.p, s));
    HIP_TRY(cb::launch_scan_u64(klen, len_scan, nl, (uint64_t*)ws.i_tmp.p, s));
    uint64_t h[3];
    HIP_TRY(hipMemcpyAsync(&h[0], bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h[1], has_scan + nl, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h[2], len_scan + nl, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[0] != ~0ull) {  // std::str::from_utf8(..).map_err(..)? (src/sstable.rs:115-116)
      char msg[96];
      std::snprintf(msg, sizeof msg, "SsTable::load: the key on line %llu is not UTF-8",
                    (unsigned long long)h[0]);
      return fail(CB_EUTF8, msg);
    }
    const uint64_t nk = h[1], kbytes = h[2];
    if (nk) {
      HIP_TRY(ws.lkey.reserve(kbytes + 16, s));
      HIP_TRY(ws.t_line.reserve((nk + 1) * 8, s));
      HIP_TRY(ws.t_which.reserve(nk * 8, s));
      uint8_t* kb = (uint8_t*)ws.lkey.p;
      uint64_t* ko = (uint64_t*)ws.t_line.p;
      uint64_t* lmap = (uint64_t*)ws.t_which.p;
      HIP_TRY(cb::launch_rebuild_gather(t->data, t->rec, nl, has_scan, len_scan, kb, ko, lmap, s));
      // bloom.insert(key) for every TAB line (src/sstable.rs:117)
      if ((rc = insert_locked(ws, f.get(), kb, ko, 0, nk, s))) return rc;
      // zone_map.update(key) for every TAB line (src/sstable.rs:118)
      HIP_TRY(ws.zone.reserve((2 * 1024 + 2) * 8, s));
      uint64_t* dtmp = (uint64_t*)ws.zone.p;
      uint64_t* didx = dtmp + 2 * 1024;
      HIP_TRY(cb::launch_zone_bounds(cb::KEY_VAR, cb::KeySrc{kb, ko, 0}, nk, dtmp, didx, s));
      uint64_t idx[2], line[2];
      HIP_TRY(hipMemcpyAsync(idx, didx, 16, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      HIP_TRY(hipMemcpyAsync(&line[0], lmap + idx[0], 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&line[1], lmap + idx[1], 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (zone_min_line) *zone_min_line = line[0];
      if (zone_max_line) *zone_max_line = line[1];
    }
  }
  *bloom_out = f.release();
  return CB_OK;
}

// Newest-wins merge (compact.hpp). Every temporary is carved from pool blocks
// released stream-ordered on return (error returns included: nothing the
// enqueued work touches is freed under it). The call waits for its own stream
// for the survivors' totals (the output is sized from them), for the
// directory's map and at the end (the zone bounds are host results).
int cb_tables_compact(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, void* stream,
                      cb_table** table_out, cb_filter** bloom_out) {
  if (!table_out) return fail(CB_EINVAL, "null argument");
  *table_out = nullptr;
  if (bloom_out) *bloom_out = nullptr;
  if (!nt || !tables) return fail(CB_EINVAL, "no tables");
  for (uint32_t i = 0; i < nt; ++i)
    if (!tables[i]) return fail(CB_EINVAL, "null table");
  const int dev = tables[0]->device;
  for (uint32_t i = 0; i < nt; ++i)
    if (tables[i]->device != dev) return fail(CB_EINVAL, "tables live on different devices");
  if (bloom_out && m_bits == 0)  // BloomFilter::insert's `% 0` (src/bloom.rs:36)
    return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  hipStream_t s = (hipStream_t)stream;
  // the sources: the non-empty tables, newest first, with their line bases
  std::vector<cb::CompactSrc> srcs;
  uint64_t n = 0, kbound = 0;
  for (uint32_t i = 0; i < nt; ++i) {
    cb_table* ti = const_cast<cb_table*>(tables[i]);
    if (int rc = finalize_table(ti)) return rc;
    if (!ti->nlines) continue;
    if (!ti->fast) return fail(CB_EINVAL, "an input table is not well-formed");
    srcs.push_back(cb::CompactSrc{ti->data, ti->rec, ti->llen, n});
    n += ti->nlines;
    kbound += ti->len;  // the keys' bytes are among the file's
  }
  if (n > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many lines for one compaction");
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
  uint64_t cnt = 0, len = 0, kbytes = 0;
  if (n) {
    Merge mg;
    if ((rc = merge_alloc(dev, (uint32_t)srcs.size(), n, kbound, tmp, &mg))) return rc;
    const uint32_t nsrc = (uint32_t)srcs.size();
    HIP_TRY(hipMemcpyAsync(mg.dsrc, srcs.data(), nsrc * sizeof(cb::CompactSrc), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the source is pageable
    uint64_t h[3];
    if ((rc = enqueue_merge(mg, mg.dsrc, nsrc, s, h))) return rc;
    cnt = h[0];
    len = h[1];
    kbytes = h[2];
    cb::SortKey* order = mg.order;
    cb::CompactSide* side = mg.side;
    uint64_t *slen = mg.slen, *tcnt = mg.tcnt, *tbytes = mg.tbytes, *tkeys = mg.tkeys, *tot = mg.tot;
    cb::CreateResult* dr = mg.dr;
    t->len = len;
    if ((rc = alloc_file(t.get(), len + 16))) return rc;
    HIP_TRY(hipMemsetAsync(t->data + len, 0, 16, s));
    if (cnt) {
      if ((rc = alloc_index(t.get(), cnt))) return rc;
      const size_t kb2_bytes = (size_t)((kbytes + 16 + 15) & ~15ull);
      if (pool_alloc(dev, kb2_bytes + (cnt + 1) * 8, &keys.p, &keys.cap) != hipSuccess) {
        keys.p = nullptr;
        return fail(CB_ENOMEM, "device allocation failed for a compaction's keys");
      }
      uint8_t* kb2 = (uint8_t*)keys.p;
      uint64_t* ko2 = (uint64_t*)(kb2 + kb2_bytes);
      // the file and its line index in one pass (the file is not re-read)
      HIP_TRY(cb::launch_compact_format(order, side, slen, tcnt, tbytes, tkeys, tot, n, cnt, t->data, t->rec, t->pfx,
                                        t->fence, t->llen, kb2, ko2, s));
      // BloomFilter::new(m) + insert per kept key (src/sstable.rs:59-63)
      if (f) {
        std::lock_guard<std::mutex> lk(ws.mu);
        if ((rc = insert_locked(ws, f.get(), kb2, ko2, 0, cnt, s))) return rc;
      }
      // the directory's map from the new prefixes (dr's masks are reused), and
      // the zone map's key offsets: the first and last kept key
      uint64_t* dmask = &dr->dmask[0][0];
      if ((rc = enqueue_pfx_masks(t.get(), dmask, s))) return rc;
      uint64_t e[2] = {0, 0}, m[cb::kDirPos][4] = {};
      HIP_TRY(hipMemcpyAsync(&e[0], ko2 + 1, 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&e[1], ko2 + cnt - 1, 8, hipMemcpyDeviceToHost, s));
      if (t->dir) HIP_TRY(hipMemcpyAsync(m, dmask, sizeof m, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (e[0] > kbytes || e[1] > kbytes) return fail(CB_EHIP, "compaction: inconsistent key offsets");
      if ((rc = enqueue_directory(t.get(), m, s))) return rc;
      t->zmin.resize(e[0]);
      t->zmax.resize(kbytes - e[1]);
      if (e[0]) HIP_TRY(hipMemcpyAsync(&t->zmin[0], kb2, e[0], hipMemcpyDeviceToHost, s));
      if (kbytes - e[1]) HIP_TRY(hipMemcpyAsync(&t->zmax[0], kb2 + e[1], kbytes - e[1], hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      // strictly increasing keys, a TAB on every line: by construction
      t->fast = !g_table_exact;
      t->has_zone = true;
    }
  }
  // no line survives: the empty file, as cb_sstable_create's n == 0
  if (!cnt && (rc = finish_empty_file(t.get(), s))) return rc;
  if (bloom_out) *bloom_out = f.release();
  *table_out = t.release();
  return CB_OK;
}

namespace {
// A result's block: key_off | val_off | which | keys | vals, for count entries
// and room for kb key bytes and vb value bytes.
size_t scan_layout(uint64_t count, uint64_t kb, uint64_t vb, size_t (&o)[5]) {
  size_t at = 0;
  const uint64_t part[5] = {(count + 1) * 8, (count + 1) * 8, count * 4, kb + 16, vb + 16};
  for (int i = 0; i < 5; ++i) {
    o[i] = at;
    at += (size_t)((part[i] + 15) & ~15ull);
  }
  return at;
}
size_t scan_bytes(uint64_t count, uint64_t kb, uint64_t vb) {
  size_t o[5];
  return scan_layout(count, kb, vb, o);
}
int scan_alloc(cb_scan* r, uint64_t count, uint64_t kb, uint64_t vb) {
  size_t o[5];
  const size_t bytes = scan_layout(count, kb, vb, o);
  if (pool_alloc(r->device, bytes, &r->block, &r->block_cap) != hipSuccess) {
    r->block = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for a scan's result");
  }
  uint8_t* b = (uint8_t*)r->block;
  r->key_off = (uint64_t*)(b + o[0]);
  r->val_off = (uint64_t*)(b + o[1]);
  r->which = (int32_t*)(b + o[2]);
  r->keys = b + o[3];
  r->vals = b + o[4];
  return CB_OK;
}
}  // namespace

// Range scan (scan.hpp): the tables cut to [lo, hi) on the device, the cuts
// merged as compaction merges whole tables, the survivors' keys and decoded
// values written into the result. Scratch as in cb_tables_compact: pool blocks
// released stream-ordered on every return path. The call waits for its own
// stream after staging the table list (pageable memory) and then three times
// for a few words, each bound-checked before anything is sized from it: the
// cuts' totals (the merge's scratch), the survivors' totals (the result), and
// the kept keys' and values' byte totals at the end (the result is complete
// when the call returns). A limit's result is then copied into a block of its
// own size, so what a caller keeps is sized by what it asked for.
int cb_tables_scan(const cb_table* const* tables, uint32_t nt, const uint8_t* lo, uint64_t lo_len, const uint8_t* hi,
                   uint64_t hi_len, int has_hi, uint64_t limit, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  if (!nt || !tables) return fail(CB_EINVAL, "no tables");
  for (uint32_t i = 0; i < nt; ++i)
    if (!tables[i]) return fail(CB_EINVAL, "null table");
  const int dev = tables[0]->device;
  for (uint32_t i = 0; i < nt; ++i)
    if (tables[i]->device != dev) return fail(CB_EINVAL, "tables live on different devices");
  if (lo_len && !lo) return fail(CB_EINVAL, "null lower bound with a length");
  if (!has_hi) hi_len = 0;
  if (hi_len && !hi) return fail(CB_EINVAL, "null upper bound with a length");
  hipStream_t s = (hipStream_t)stream;
  // the non-empty tables, newest first
  std::vector<cb::ScanTable> tabs;
  uint64_t all_lines = 0, all_bytes = 0;
  for (uint32_t i = 0; i < nt; ++i) {
    cb_table* ti = const_cast<cb_table*>(tables[i]);
    if (int rc = finalize_table(ti)) return rc;
    if (!ti->nlines) continue;
    if (!ti->fast) return fail(CB_EINVAL, "an input table is not well-formed");
    tabs.push_back(cb::ScanTable{ti->data, ti->rec, ti->pfx, ti->fence, ti->llen, ti->nlines, ti->len, i, 0});
    all_lines += ti->nlines;
    all_bytes += ti->len;
  }
  std::unique_ptr<cb_scan, int (*)(void*)> r(new cb_scan(), cb_scan_destroy);
  r->device = dev;
  // nothing to search: no lines at all, or lo >= hi
  if (tabs.empty() || (has_hi && cb::key_cmp(lo, lo_len, hi, hi_len) >= 0)) {
    *out = r.release();
    return CB_OK;
  }
  int rc = cb_init(dev);
  if (rc) return rc;
  DeviceGuard dg(dev);
  (void)workspace(dev, s);  // (registers s: the pool retires blocks behind it)
  TempBlock cuts{dev}, tmp{dev}, vtmp{dev};
  size_t at = 0;
  auto take = [&](uint64_t bytes) {
    const size_t o = at;
    at += (size_t)((bytes + 15) & ~15ull);
    return o;
  };
  // 1: every table's cut, and the cuts as the merge's sources
  const uint32_t ntab = (uint32_t)tabs.size();
  const size_t o_tab = take(ntab * sizeof(cb::ScanTable)), o_bnd = take(lo_len + hi_len + 16), up_bytes = at,
               o_cut = take(ntab * sizeof(cb::ScanCut)), o_src = take(ntab * sizeof(cb::CompactSrc)),
               o_map = take(ntab * 4), o_ctot = take(3 * 8);
  if (pool_alloc(dev, at, &cuts.p, &cuts.cap) != hipSuccess) {
    cuts.p = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for a scan's cuts");
  }
  uint8_t* cbase = (uint8_t*)cuts.p;
  std::vector<uint8_t> up(up_bytes, 0);
  std::memcpy(&up[o_tab], tabs.data(), ntab * sizeof(cb::ScanTable));
  if (lo_len) std::memcpy(&up[o_bnd], lo, lo_len);
  if (hi_len) std::memcpy(&up[o_bnd + lo_len], hi, hi_len);
  HIP_TRY(hipMemcpyAsync(cbase, up.data(), up_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // the source is pageable
  const cb::ScanTable* dtab = (const cb::ScanTable*)(cbase + o_tab);
  cb::ScanCut* dcut = (cb::ScanCut*)(cbase + o_cut);
  cb::CompactSrc* dsrc = (cb::CompactSrc*)(cbase + o_src);
  uint32_t* dmap = (uint32_t*)(cbase + o_map);
  uint64_t* dctot = (uint64_t*)(cbase + o_ctot);
  const cb::ScanRange range{cbase + o_bnd, lo_len, lo_len, hi_len, has_hi ? 1u : 0u, 0};
  HIP_TRY(cb::launch_scan_bounds(dtab, ntab, range, dcut, s));
  HIP_TRY(cb::launch_scan_sources(dtab, dcut, ntab, dsrc, dmap, dctot, s));
  uint64_t c[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(c, dctot, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t n = c[0], kbound = c[1], nsrc = c[2];
  if (n > all_lines || kbound > all_bytes || nsrc > ntab || nsrc > n || (n && !nsrc))
    return fail(CB_EHIP, "scan: inconsistent cut totals");
  if (n > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many lines inside the range for one scan");
  if (!n) {
    *out = r.release();
    return CB_OK;
  }
  // 2: compaction's merge over the cuts
  Merge mg;
  if ((rc = merge_alloc(dev, 0, n, kbound, tmp, &mg))) return rc;
  uint64_t h[3];
  if ((rc = enqueue_merge(mg, dsrc, (uint32_t)nsrc, s, h))) return rc;
  const uint64_t cnt = h[0], len = h[1], kbytes = h[2];
  if (len < kbytes + 2 * cnt) return fail(CB_EHIP, "scan: inconsistent totals");
  if (!cnt) {
    *out = r.release();
    return CB_OK;
  }
  // 3: the result. A kept line is `key \t text \n` and its value decodes to at
  // most 3 bytes per 4 of text, which bounds the values before any is decoded.
  const uint64_t count = limit && limit < cnt ? limit : cnt;
  const uint64_t vcap = (len - kbytes - 2 * cnt) / 4 * 3;
  if ((rc = scan_alloc(r.get(), count, kbytes, vcap))) return rc;
  const uint64_t vtiles = cb::get_tiles(count);
  at = 0;
  const size_t o_vsrc = take(count * 8), o_dlen = take(count * 8), o_vsum = take(vtiles * 8);
  if (pool_alloc(dev, at, &vtmp.p, &vtmp.cap) != hipSuccess) {
    vtmp.p = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for a scan's value spans");
  }
  uint8_t* vb = (uint8_t*)vtmp.p;
  uint64_t *vsrc = (uint64_t*)(vb + o_vsrc), *dlen = (uint64_t*)(vb + o_dlen), *vsum = (uint64_t*)(vb + o_vsum);
  HIP_TRY(hipMemsetAsync(vsum, 0, vtiles * 8, s));
  HIP_TRY(cb::launch_scan_emit(mg.order, mg.side, mg.slen, mg.tcnt, mg.tkeys, mg.tot, dsrc, dmap, (uint32_t)nsrc, n,
                               count, r->keys, r->key_off, r->which, vsrc, dlen, vsum, s));
  // the read path's value tail: small results scan the tile sums in the decode itself
  const bool raw = count <= cb::decode_raw_max();
  if (!raw) HIP_TRY(cb::launch_tile_scan(vsum, vtiles, r->val_off + count, s));
  HIP_TRY(cb::launch_b64_decode(vsrc, dlen, vsum, count, r->val_off, r->vals, vcap, s, raw));
  uint64_t e[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&e[0], r->key_off + count, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&e[1], r->val_off + count, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (e[0] > kbytes || e[1] > vcap) return fail(CB_EHIP, "scan: inconsistent result totals");
  r->count = count;
  r->key_bytes = e[0];
  r->val_bytes = e[1];
  r->truncated = count < cnt;
  // a limit's result was sized for the whole range: keep a block of its own size
  if (r->truncated && scan_bytes(count, e[0], e[1]) * 2 < r->block_cap) {
    cb_scan big = *r;
    TempBlock old{dev, big.block, big.block_cap};
    r->block = nullptr;
    if ((rc = scan_alloc(r.get(), count, e[0], e[1]))) return rc;
    HIP_TRY(hipMemcpyAsync(r->key_off, big.key_off, (count + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(r->val_off, big.val_off, (count + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(r->which, big.which, count * 4, hipMemcpyDeviceToDevice, s));
    if (e[0]) HIP_TRY(hipMemcpyAsync(r->keys, big.keys, e[0], hipMemcpyDeviceToDevice, s));
    if (e[1]) HIP_TRY(hipMemcpyAsync(r->vals, big.vals, e[1], hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  *out = r.release();
  return CB_OK;
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

int cb_scan_info(const void* scan, uint64_t* count, uint64_t* key_bytes, uint64_t* val_bytes, int* truncated) {
  const cb_scan* r = (const cb_scan*)scan;
  if (!r) return fail(CB_EINVAL, "null scan");
  if (count) *count = r->count;
  if (key_bytes) *key_bytes = r->key_bytes;
  if (val_bytes) *val_bytes = r->val_bytes;
  if (truncated) *truncated = r->truncated ? 1 : 0;
  return CB_OK;
}

namespace {
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
}  // namespace

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

int cb_scan_destroy(void* scan) {
  cb_scan* r = (cb_scan*)scan;
  if (!r) return CB_OK;
  pool_release(r->device, r->block, r->block_cap);
  delete r;
  return CB_OK;
}

int cb_table_zone(const cb_table* t, int which, uint8_t* out, uint64_t cap, uint64_t* len) {
  if (!t || !len || (which != 0 && which != 1)) return fail(CB_EINVAL, "bad argument");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (!t->has_zone) return fail(CB_EINVAL, "table has no zone bounds (not made by cb_sstable_create, or empty)");
  const std::string& z = which ? t->zmax : t->zmin;
  *len = z.size();
  if (out && cap) std::memcpy(out, z.data(), (size_t)std::min<uint64_t>(cap, z.size()));
  return CB_OK;
}

int cb_table_info(const cb_table* t, uint64_t* nlines, uint64_t* bytes) {
  if (!t) return fail(CB_EINVAL, "null table");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  if (nlines) *nlines = t->nlines;
  if (bytes) *bytes = t->len;
  return CB_OK;
}

int cb_table_well_formed(const cb_table* t, int* out) {
  if (!t || !out) return fail(CB_EINVAL, "null argument");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  *out = t->fast ? 1 : 0;
  return CB_OK;
}

int cb_table_force_exact(int on) {
  g_table_exact = on != 0;
  return CB_OK;
}

int cb_table_bucket_limit(uint64_t max_bytes) {
  g_bucket_limit.store(max_bytes, std::memory_order_relaxed);
  return CB_OK;
}

int cb_table_lines(const cb_table* t, uint64_t* start, uint32_t* key_len, uint32_t* line_len) {
  if (!t) return fail(CB_EINVAL, "null table");
  if (int rc = finalize_table(const_cast<cb_table*>(t))) return rc;
  DeviceGuard dg(t->device);
  if (!t->nlines) return CB_OK;
  // strided copies out of the 32-byte records
  const size_t pitch = sizeof(cb::LineRec);
  const uint8_t* r = (const uint8_t*)t->rec;
  if (start)
    HIP_TRY(hipMemcpy2D(start, 8, r + offsetof(cb::LineRec, start), pitch, 8, t->nlines, hipMemcpyDefault));
  if (key_len)
    HIP_TRY(hipMemcpy2D(key_len, 4, r + offsetof(cb::LineRec, klen), pitch, 4, t->nlines, hipMemcpyDefault));
  if (line_len) HIP_TRY(hipMemcpy(line_len, t->llen, t->nlines * 4, hipMemcpyDefault));
  return CB_OK;
}

int cb_table_search_fixed(const cb_table* t, const uint8_t* keys, uint32_t key_len, uint64_t n,
                          int64_t* line_out, void* stream) {
  return table_search_impl(t, keys, nullptr, key_len, n, line_out, (hipStream_t)stream);
}

int cb_table_search_var(const cb_table* t, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                        int64_t* line_out, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return table_search_impl(t, bytes, offsets, 0, n, line_out, (hipStream_t)stream);
}

int cb_get_many_fixed(const cb_table* const* tables, uint32_t nt, const uint64_t* hits,
                      const uint32_t* hit_rows, const uint8_t* keys, uint32_t key_len, uint64_t n,
                      int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap,
                      uint64_t* total, void* stream) {
  return get_many_impl(tables, nt, Gate::of_rows(hits, hit_rows), keys, nullptr, key_len, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

int cb_get_many_var(const cb_table* const* tables, uint32_t nt, const uint64_t* hits,
                    const uint32_t* hit_rows, const uint8_t* bytes, const uint64_t* offsets,
                    uint64_t n, int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap,
                    uint64_t* total, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return get_many_impl(tables, nt, Gate::of_rows(hits, hit_rows), bytes, offsets, 0, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

int cb_set_get_many_fixed(const cb_filterset* set, const cb_table* const* tables, uint32_t nt,
                          const uint32_t* slots, const uint8_t* keys, uint32_t key_len, uint64_t n,
                          int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap, uint64_t* total,
                          void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  return get_many_impl(tables, nt, Gate::of_set(set, slots), keys, nullptr, key_len, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

int cb_set_get_many_var(const cb_filterset* set, const cb_table* const* tables, uint32_t nt,
                        const uint32_t* slots, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                        int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap, uint64_t* total,
                        void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return get_many_impl(tables, nt, Gate::of_set(set, slots), bytes, offsets, 0, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

int cb_tiers_get_many_fixed(const cb_filterset* const* sets, uint32_t ns, const cb_table* const* tables,
                            uint32_t nt, const uint32_t* tiers, const uint32_t* slots, const uint8_t* keys,
                            uint32_t key_len, uint64_t n, int32_t* which, uint64_t* val_off, uint8_t* vals,
                            uint64_t cap, uint64_t* total, void* stream) {
  const TierList tl{sets, ns, tiers, slots};
  return get_many_impl(tables, nt, Gate::of_tiers(&tl), keys, nullptr, key_len, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

int cb_tiers_get_many_var(const cb_filterset* const* sets, uint32_t ns, const cb_table* const* tables, uint32_t nt,
                          const uint32_t* tiers, const uint32_t* slots, const uint8_t* bytes,
                          const uint64_t* offsets, uint64_t n, int32_t* which, uint64_t* val_off, uint8_t* vals,
                          uint64_t cap, uint64_t* total, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  const TierList tl{sets, ns, tiers, slots};
  return get_many_impl(tables, nt, Gate::of_tiers(&tl), bytes, offsets, 0, n,
                       GetOut{which, val_off, vals, cap, total}, (hipStream_t)stream);
}

}  // extern "C"
