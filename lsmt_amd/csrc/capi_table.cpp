// capi_table.cpp — the cb_table handle: the index of a
// file's lines and its layout, the steps every maker of a table shares,
// indexing a file that already exists (cb_table_create), the handle's
// accessors, the batched binary search and SsTable::load's filter and zone
// bounds (cb_table_rebuild).
//
// Reference: src/sstable.rs:100-179.
#include "capi_table.hpp"

using namespace cbx;

namespace {

bool g_table_exact = false;  // cb_table_force_exact: index files for the exact-trajectory search only

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

}  // namespace

namespace cbx {

bool table_exact() { return g_table_exact; }

int pool_alloc_or(int dev, size_t bytes, void** p, size_t* cap, const char* what) {
  if (pool_alloc(dev, bytes, p, cap) != hipSuccess) {
    *p = nullptr;
    return fail(CB_ENOMEM, what);
  }
  return CB_OK;
}

cb::DirMap* dmap_slot(const cb_table* t) {
  return t->dir ? (cb::DirMap*)((uint8_t*)t->dir + dir_bytes(t->nlines)) : nullptr;
}

int alloc_file(cb_table* t, uint64_t bytes) {
  return pool_alloc_or(t->device, bytes, (void**)&t->data, &t->data_cap,
                       "device allocation failed for an SSTable buffer");
}
int alloc_index(cb_table* t, uint64_t nl) {
  t->nlines = nl;
  if (int rc = pool_alloc_or(t->device, index_bytes(nl), (void**)&t->rec, &t->rec_cap,
                             "device allocation failed for an SSTable index"))
    return rc;
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

int finish_empty_file(cb_table* t, hipStream_t s) {
  if (!t->data)
    if (int rc = alloc_file(t, 16)) return rc;
  HIP_TRY(hipMemsetAsync(t->data, 0, 16, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// count -> scan -> emit -> finish -> keys; the index itself is one
// allocation: rec | pfx | fence.
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

}  // namespace cbx

namespace {

int table_search_impl(const cb_table* t, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                      int64_t* line_out, hipStream_t s) {
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

// ---- cb_table_rebuild's steps, in the order it takes them (ws.mu held) ----

// The keys of a table's TAB lines as one batch (device, in the workspace),
// and each key's line.
struct TabKeys {
  uint64_t nk = 0, kbytes = 0;
  uint64_t *has_scan = nullptr, *len_scan = nullptr;  // the scans the gather places the keys by
  uint8_t* kb = nullptr;
  uint64_t *ko = nullptr, *lmap = nullptr;
};

// 1: which lines hold a TAB and how long their keys are, scanned; the counts
// come back to the host (one wait) with the first line whose key is not UTF-8.
int mark_tab_lines(Workspace& ws, const cb_table* t, hipStream_t s, TabKeys* k) {
  const uint64_t nl = t->nlines;
  HIP_TRY(ws.i_cnt.reserve((nl + 1) * 8, s));
  HIP_TRY(ws.i_base.reserve((nl + 1) * 8, s));
  HIP_TRY(ws.i_start.reserve((nl + 1) * 8, s));
  HIP_TRY(ws.i_end.reserve((nl + 1) * 8, s));
  HIP_TRY(ws.i_tmp.reserve(cb::scan_tmp_words(nl) * 8, s));
  HIP_TRY(ws.i_err.reserve(8, s));
  uint64_t* has = (uint64_t*)ws.i_cnt.p;
  uint64_t* klen = (uint64_t*)ws.i_start.p;
  uint64_t* bad = (uint64_t*)ws.i_err.p;
  k->has_scan = (uint64_t*)ws.i_base.p;
  k->len_scan = (uint64_t*)ws.i_end.p;
  HIP_TRY(hipMemsetAsync(bad, 0xFF, 8, s));
  HIP_TRY(cb::launch_rebuild_mark(t->data, t->rec, nl, has, klen, bad, s));
  HIP_TRY(cb::launch_scan_u64(has, k->has_scan, nl, (uint64_t*)ws.i_tmp.p, s));
  HIP_TRY(cb::launch_scan_u64(klen, k->len_scan, nl, (uint64_t*)ws.i_tmp.p, s));
  uint64_t h[3];
  HIP_TRY(hipMemcpyAsync(&h[0], bad, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h[1], k->has_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h[2], k->len_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] != ~0ull) {  // std::str::from_utf8(..).map_err(..)? (src/sstable.rs:115-116)
    char msg[96];
    std::snprintf(msg, sizeof msg, "SsTable::load: the key on line %llu is not UTF-8", (unsigned long long)h[0]);
    return fail(CB_EUTF8, msg);
  }
  k->nk = h[1];
  k->kbytes = h[2];
  return CB_OK;
}

// 2: the keys gathered into one batch.
int gather_tab_keys(Workspace& ws, const cb_table* t, hipStream_t s, TabKeys* k) {
  HIP_TRY(ws.lkey.reserve(k->kbytes + 16, s));
  HIP_TRY(ws.t_line.reserve((k->nk + 1) * 8, s));
  HIP_TRY(ws.t_which.reserve(k->nk * 8, s));
  k->kb = (uint8_t*)ws.lkey.p;
  k->ko = (uint64_t*)ws.t_line.p;
  k->lmap = (uint64_t*)ws.t_which.p;
  HIP_TRY(cb::launch_rebuild_gather(t->data, t->rec, t->nlines, k->has_scan, k->len_scan, k->kb, k->ko, k->lmap, s));
  return CB_OK;
}

// 4: zone_map.update(key) for every TAB line (src/sstable.rs:118): the lines
// of the least and the greatest key (two waits: their indices, then their lines).
int zone_lines(Workspace& ws, const TabKeys& k, hipStream_t s, uint64_t (&line)[2]) {
  HIP_TRY(ws.zone.reserve((2 * 1024 + 2) * 8, s));
  uint64_t* dtmp = (uint64_t*)ws.zone.p;
  uint64_t* didx = dtmp + 2 * 1024;
  HIP_TRY(cb::launch_zone_bounds(cb::KEY_VAR, cb::KeySrc{k.kb, k.ko, 0}, k.nk, dtmp, didx, s));
  uint64_t idx[2];
  HIP_TRY(hipMemcpyAsync(idx, didx, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpyAsync(&line[0], k.lmap + idx[0], 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&line[1], k.lmap + idx[1], 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

}  // namespace

extern "C" {

int cb_table_destroy(cb_table* t) {
  if (!t) return CB_OK;
  {
    DeviceGuard dg(t->device);
    if (t->pend) {  // enqueued work may still be running: let it finish first
      std::lock_guard<std::mutex> lk(t->fin_mu);
      if (t->pend->ev && !t->ready.load()) (void)hipEventSynchronize(t->pend->ev);
      t->pend.reset();  // (~TablePending returns the staged block and the result slot)
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

// SsTable::load's filter and zone bounds for a file that is already indexed
// (src/sstable.rs:111-118). The call waits for its stream three times: for
// the TAB lines' counts, and twice for the zone's lines.
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
  if (t->nlines) {
    DeviceGuard dg(t->device);
    Workspace& ws = workspace(t->device, s);
    std::lock_guard<std::mutex> lk(ws.mu);
    TabKeys k;
    if ((rc = mark_tab_lines(ws, t, s, &k))) return rc;
    if (k.nk) {
      if ((rc = gather_tab_keys(ws, t, s, &k))) return rc;
      // 3: bloom.insert(key) for every TAB line (src/sstable.rs:117)
      if ((rc = insert_locked(ws, f.get(), k.kb, k.ko, 0, k.nk, s))) return rc;
      uint64_t line[2];
      if ((rc = zone_lines(ws, k, s, line))) return rc;
      if (zone_min_line) *zone_min_line = line[0];
      if (zone_max_line) *zone_max_line = line[1];
    }
  }
  *bloom_out = f.release();
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

}  // extern "C"
