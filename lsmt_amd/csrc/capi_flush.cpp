// capi_flush.cpp — SsTable::create on the device:
// cb_sstable_create enqueues now, the table is finalised on first use.
//
// cb_sstable_create only enqueues its kernels (sortedness check, Bloom
// build, the sort the device picks, tile scan, format) and one copy of the
// CreateResult into a pinned block, followed by an event; nothing waits. The
// host-side results (file length, zone bounds, the well-formed flag) are read
// when the table is first used (finalize_table). One case needs the host
// there: a key holding '\n' or '\t' (the file is re-indexed the way
// SsTable::get splits it). A batch the bin sort cannot place (one bin, or a
// bin larger than an LDS tile) is sorted again on the device, by the merge
// sort enqueued after it that runs only then. Until a table is finalised its
// inputs must stay valid (host inputs are staged into a block the table owns).
//
// Reference: src/sstable.rs:51-98.
#include "capi_table.hpp"

using namespace cbx;

namespace {

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

// Bin-sort group target: ~n / 1536 records (six 1024-record group sorts per
// CU on 256 CUs, one wave), at least 640, at most 1536 (2048-record sorts).
uint32_t bin_group_target(uint64_t n) {
  static const int knob = cb::knob_int("CB_BIN_T", -1);  // group size target (tuning); 0 disables the bin sort
  if (knob >= 0) return (uint32_t)knob;
  return (uint32_t)std::min<uint64_t>(1536, std::max<uint64_t>(640, (n + 1535) / 1536));
}

}  // namespace

TablePending::~TablePending() {
  if (staged) pool_release(device, staged, staged_cap);
  result_release(hres, ev);
}

namespace cbx {

SortPlan plan_key_sort(uint64_t n) {
  const uint32_t T = bin_group_target(n);
  const bool binned = T && T <= cb::bin_sort_max_group() && n > 4096 && n <= (1ull << 24);
  return SortPlan{binned, T, binned ? cb::bin_sort_tmp_bytes(n, T) : cb::entry_sort_tmp_bytes(n)};
}

int enqueue_key_sort(const SortPlan& plan, const uint8_t* kb, const uint64_t* ko, uint64_t n, cb::SortKey* order,
                     void* tmp, cb::CreateResult* dr, hipStream_t s, const uint64_t* vo, ulonglong2* vsp,
                     uint64_t* tsum) {
  const auto& [binned, T, tmp_bytes] = plan;
  if (binned) HIP_TRY(cb::launch_bin_sort(kb, ko, n, T, order, tmp, s, vo, vsp, tsum, dr));
  HIP_TRY(cb::launch_entry_sort(order, (cb::SortKey*)tmp, n, kb, ko, s, vo, vsp, tsum, &dr->flags[binned ? 3 : 0]));
  return CB_OK;
}

}  // namespace cbx

namespace {

// An error return past the first enqueue may leave work enqueued that reads
// the staged block or writes the result slot: finish the stream before the
// table's TablePending hands them back (declared after it, so it runs first).
// Armed only at the first enqueue: a refusal before it — bad offsets, bounds,
// a failed allocation — returns without blocking on the caller's stream
// (ADVICE r5).
struct SyncOnError {
  hipStream_t s;
  bool ok = true;
  ~SyncOnError() {
    if (!ok) (void)hipStreamSynchronize(s);
  }
};

// A flush's four inputs: key offsets, value offsets, key bytes, value bytes.
// Host inputs go into one block the table owns (the work reads them after the
// call returns, and a fallback sort at finalisation reads them again); device
// inputs are used in place.
enum { IN_KO, IN_VO, IN_KB, IN_VB };
struct FlushInputs {
  const void* src[4];
  uint64_t bytes[4];
  bool host[4];
};

// The totals key_off[n] / val_off[n] of device-resident offsets (which[i]:
// read that one; the other stays 0), read back on s and waited for.
int read_offset_totals(const uint64_t* key_off, const uint64_t* val_off, uint64_t n, const bool (&which)[2],
                       hipStream_t s, uint64_t (&tot)[2]) {
  tot[0] = tot[1] = 0;
  if (which[0]) HIP_TRY(hipMemcpyAsync(&tot[0], key_off + n, 8, hipMemcpyDeviceToHost, s));
  if (which[1]) HIP_TRY(hipMemcpyAsync(&tot[1], val_off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// ---- sstable_enqueue's steps, in the order it takes them ----

// 1: the offsets, before anything is enqueued: host ones must not decrease;
// device ones beside host bytes must stay inside them (the bytes are staged
// into exactly kbytes / vbytes, so offsets past those would send every kernel
// past the staged block: one read-back).
int check_flush_offsets(const FlushInputs& in, uint64_t n, hipStream_t s) {
  for (int w : {IN_KO, IN_VO}) {
    const uint64_t* off = (const uint64_t*)in.src[w];
    if (in.host[w])
      for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(CB_EINVAL, "offsets must be non-decreasing");
  }
  const bool dev_off[2] = {in.host[IN_KB] && !in.host[IN_KO], in.host[IN_VB] && !in.host[IN_VO]};
  if (dev_off[0] || dev_off[1]) {
    uint64_t tot[2];
    if (int rc = read_offset_totals((const uint64_t*)in.src[IN_KO], (const uint64_t*)in.src[IN_VO], n, dev_off, s, tot))
      return rc;
    if (tot[0] > in.bytes[IN_KB]) return fail(CB_EINVAL, "key bytes exceed key_bytes");
    if (tot[1] > in.bytes[IN_VB]) return fail(CB_EINVAL, "value bytes exceed val_bytes");
  }
  return CB_OK;
}

// 2: the host inputs into the table's staged block; in.src then names device
// memory throughout. The copies are the first enqueued work.
int stage_host_inputs(FlushInputs& in, TablePending& p, SyncOnError& on_error, hipStream_t s) {
  const cb::FlushStage st = cb::flush_stage_layout(in.host, in.bytes);
  if (!st.total) return CB_OK;
  if (int rc = pool_alloc_or(p.device, st.total, &p.staged, &p.staged_cap,
                             "device allocation failed for a staged flush batch"))
    return rc;
  on_error.ok = false;
  for (int i = 0; i < 4; ++i) {
    if (!in.host[i]) continue;
    uint8_t* d = (uint8_t*)p.staged + st.off[i];
    HIP_TRY(hipMemcpyAsync(d, in.src[i], in.bytes[i], hipMemcpyHostToDevice, s));
    in.src[i] = d;
  }
  return CB_OK;
}

// 3 (n == 0): an empty file: nothing to sort, index or bound.
int empty_flush(cb_table* t, std::unique_ptr<TablePending>& pend, uint64_t m_bits, SyncOnError& on_error,
                hipStream_t s, cb_filter** bloom_out) {
  on_error.ok = false;
  if (bloom_out) {
    cb_filter* fp = nullptr;
    if (int rc = cb_filter_create(m_bits, t->device, &fp)) return rc;
    *bloom_out = fp;
  }
  t->pend = std::move(pend);  // (no result block: the staged block is released with the table)
  if (int rc = finish_empty_file(t, s)) return rc;
  on_error.ok = true;
  return CB_OK;
}

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

// 4: the create's work on s (ws.mu held): sortedness check, the Bloom build
// (f != nullptr: a new filter of m_bits into *f), the sort, the format, the
// results' copy into p.hres and the event behind it.
int enqueue_create(Workspace& ws, cb_table* t, const TablePending& p, uint64_t kbytes, uint64_t vbytes,
                   std::unique_ptr<cb_filter, int (*)(cb_filter*)>* f, uint64_t m_bits, hipStream_t s) {
  const uint64_t n = p.n;
  HIP_TRY(ws.f_flag.reserve(sizeof(cb::CreateResult), s));
  HIP_TRY(ws.f_tsum.reserve(cb::format_tiles(n) * 8, s));
  HIP_TRY(ws.f_sk2.reserve(n * sizeof(cb::SortKey), s));
  HIP_TRY(ws.f_vsp.reserve(n * sizeof(ulonglong2), s));
  cb::CreateResult* dr = (cb::CreateResult*)ws.f_flag.p;
  uint64_t* tsum = (uint64_t*)ws.f_tsum.p;
  HIP_TRY(hipMemsetAsync(dr, 0, cb::kCreateHead, s));
  HIP_TRY(cb::launch_sorted_check(p.dk, p.dko, p.dvo, n, dr, tsum, kbytes, vbytes, s));
  // the Bloom build needs neither the order nor the totals (OR is order-free)
  if (f) {
    cb_filter* fp = nullptr;
    if (int rc = cb_filter_create(m_bits, t->device, &fp)) return rc;
    f->reset(fp);
    if (int rc = insert_locked(ws, fp, p.dk, p.dko, 0, n, s)) return rc;
  }
  // the stable sort by key, enqueued before anyone knows whether the batch
  // needs one: every sort launch returns at once for a sorted batch (memtable
  // flushes arrive sorted)
  const SortPlan plan = plan_key_sort(n);
  HIP_TRY(ws.f_sort.reserve(plan.tmp_bytes, s));
  if (int rc = enqueue_key_sort(plan, p.dk, p.dko, n, (cb::SortKey*)ws.f_sk2.p, ws.f_sort.p, dr, s, p.dvo,
                                (ulonglong2*)ws.f_vsp.p, tsum))
    return rc;
  if (int rc = enqueue_format(t, ws, p, dr, s)) return rc;
  HIP_TRY(hipMemcpyAsync(p.hres, dr, sizeof(cb::CreateResult), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(p.ev, s));
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
  SyncOnError on_error{s};
  FlushInputs in{{key_off, val_off, keys, vals},
                 {(n + 1) * 8, (n + 1) * 8, kbytes, vbytes},
                 {!is_device_ptr(key_off), !is_device_ptr(val_off), kbytes && !is_device_ptr(keys),
                  vbytes && !is_device_ptr(vals)}};
  if ((rc = check_flush_offsets(in, n, s))) return rc;
  if ((rc = stage_host_inputs(in, p, on_error, s))) return rc;
  p.dko = (const uint64_t*)in.src[IN_KO];
  p.dvo = (const uint64_t*)in.src[IN_VO];
  p.dk = (const uint8_t*)in.src[IN_KB];
  p.dv = (const uint8_t*)in.src[IN_VB];
  // the file's buffer, by its bound; its length comes back with the results
  p.cap_bytes = cb::flush_file_bound(n, kbytes, vbytes);
  if ((rc = alloc_file(t.get(), p.cap_bytes))) return rc;
  if (!n) {
    if ((rc = empty_flush(t.get(), pend, m_bits, on_error, s, bloom_out))) return rc;
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
  {
    std::lock_guard<std::mutex> lk(ws.mu);
    if ((rc = enqueue_create(ws, t.get(), p, kbytes, vbytes, bloom_out ? &f : nullptr, m_bits, s))) return rc;
  }
  t->dmap = t->dir ? dmap_slot(t.get()) : nullptr;
  t->pend = std::move(pend);
  t->ready.store(false, std::memory_order_release);
  on_error.ok = true;
  if (bloom_out) *bloom_out = f.release();
  *table_out = t.release();
  return CB_OK;
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
    t->fast = !hr->flags[2] && !table_exact();
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
      t->pend.reset();  // (~TablePending returns the staged block and the result slot)
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

int cb_sstable_create(const uint8_t* keys, const uint64_t* key_off, const uint8_t* vals,
                      const uint64_t* val_off, uint64_t n, uint64_t m_bits, int device, void* stream,
                      cb_table** table_out, cb_filter** bloom_out, uint64_t* zone_min_idx,
                      uint64_t* zone_max_idx) {
  if (!table_out || !key_off || !val_off) return fail(CB_EINVAL, "null argument");
  if (zone_min_idx) *zone_min_idx = ~0ull;
  if (zone_max_idx) *zone_max_idx = ~0ull;
  // byte totals: host offsets carry them; device offsets are read back (one
  // round trip: cb_sstable_create_bounded takes the bounds instead)
  uint64_t tot[2] = {0, 0};
  const bool dev_off[2] = {is_device_ptr(key_off), is_device_ptr(val_off)};
  if (dev_off[0] || dev_off[1]) {
    int rc = cb_init(device);
    if (rc) return rc;
    DeviceGuard dg(device);
    if ((rc = read_offset_totals(key_off, val_off, n, dev_off, (hipStream_t)stream, tot))) return rc;
  }
  if (!dev_off[0]) tot[0] = key_off[n];
  if (!dev_off[1]) tot[1] = val_off[n];
  int rc = sstable_enqueue(keys, key_off, tot[0], vals, val_off, tot[1], n, m_bits, device, (hipStream_t)stream,
                           table_out, bloom_out);
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

}  // extern "C"
