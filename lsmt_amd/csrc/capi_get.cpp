// capi_get.cpp — the batched read path over SSTables in HBM (SURVEY.md §8f
// row 3): the tables' key buckets, the gates that choose each key's candidate
// tables, Database::get's newest-first walk (cb_get_many_*, cb_set_get_many_*,
// cb_tiers_get_many_*) and the value tail that decodes what it found.
//
// Reference: src/sstable.rs:136-179, src/lib.rs:125-136.
#include "capi_table.hpp"

using namespace cbx;

namespace {

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
  // of the rows (tablehost.hpp WideGroup), anything else one bit per table
  std::vector<cb::WideGroup> groups(cb::wide_group_count(nt));
  const bool need_slots = cb::wide_groups(rows.empty() ? nullptr : rows.data(), nt, groups.data());
  if (int rc = upload_if_changed(ws.t_groups, ws.t_groups_host, groups.data(),
                                 groups.size() * sizeof(cb::WideGroup), s))
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
// and their decode (enqueue_value_decode), and the answers back to the host.
int value_tail(Workspace& ws, const GetBufs& b, uint64_t n, const GetOut& o, hipStream_t s) {
  const ValueSpans v{b.vsrc, b.dlen, b.tsum, b.voff};
  const bool raw_ok = n != 0;  // (n = 0: the scan kernel writes voff[0] = 0)
  if (!ws.htot) HIP_TRY(hipHostMalloc((void**)&ws.htot, kHostScratch, hipHostMallocDefault));
  if (o.async()) return enqueue_value_decode(v, n, o.vals, o.vals ? o.cap : 0, raw_ok, false, s);
  if (o.vals && is_device_ptr(o.vals)) {
    // device values: offsets and values in one pass (the kernel skips the
    // value writes when the total exceeds cap): one host round trip
    if (int rc = enqueue_value_decode(v, n, o.vals, o.cap, raw_ok, false, s)) return rc;
    HIP_TRY(hipMemcpyAsync(ws.htot, b.voff + n, 8, hipMemcpyDeviceToHost, s));
  } else {
    if (int rc = enqueue_value_decode(v, n, nullptr, 0, raw_ok, false, s)) return rc;  // offsets only
    HIP_TRY(hipMemcpyAsync(ws.htot, b.voff + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t tot = *ws.htot;
    if (o.vals && o.cap >= tot && tot) {
      uint8_t* dvals;
      if (int rc = out_buf(ws.t_vals, o.vals, tot, s, &dvals)) return rc;
      if (int rc = enqueue_value_decode(v, n, dvals, tot, raw_ok, true, s)) return rc;
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

}  // namespace

namespace cbx {

int enqueue_value_decode(const ValueSpans& v, uint64_t n, uint8_t* vals, uint64_t cap, bool raw_ok, bool again,
                         hipStream_t s) {
  bool raw = raw_ok && n <= cb::decode_raw_max();
  static const bool no_raw = cb::knob_int("CB_DECODE_RAW", 1) == 0;
  if (no_raw) raw = false;
  if (!raw && !again) HIP_TRY(cb::launch_tile_scan(v.tsum, cb::get_tiles(n), v.voff + n, s));
  HIP_TRY(cb::launch_b64_decode(v.vsrc, v.dlen, v.tsum, n, v.voff, vals, cap, s, raw));
  return CB_OK;
}

}  // namespace cbx

extern "C" {

int cb_table_bucket_limit(uint64_t max_bytes) {
  g_bucket_limit.store(max_bytes, std::memory_order_relaxed);
  return CB_OK;
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
