// capi_write.cpp — a batch of SQL writes turned into keys, values and log
// records on the device (cb_rows_write; write.hpp) and, for one row on the
// host, cb_row_write, with the result's accessors (cb_written_*). The rule is
// rowwrite.hpp's; the old rows of an UPDATE are the buffers an enqueue-only
// cb_*get_many fills.
//
// Reference: src/query.rs:162-261 (exec_insert, exec_update, exec_delete),
// 716-731 (build_row), src/schema.rs:37-39 (encode_row), src/lib.rs:96-116,
// 154-157 (insert_internal's log record, insert_ns_ts's key and timestamp).
#include "capi_merge.hpp"
#include "write.hpp"

using namespace cbx;

// A written batch: flags | key_off | val_off | log_off in one pool block, keys
// | vals | log in another (sized only once the rows' lengths are known),
// complete when the call returns. A batch of no rows holds no device memory.
struct cb_written {
  int device = 0;
  uint64_t count = 0, key_bytes = 0, val_bytes = 0, log_bytes = 0, flagged = 0;
  void *block = nullptr, *data_block = nullptr;
  size_t block_cap = 0, data_cap = 0;
  uint8_t *flags = nullptr, *keys = nullptr, *vals = nullptr, *log = nullptr;
  uint64_t *key_off = nullptr, *val_off = nullptr, *log_off = nullptr;
};

namespace {

// A cb_write checked and packed (rowwrite.hpp): every writing entry's first
// step, before any device is touched.
int take_write(const void* stmt, cb::WriteCols* cols, const cb_write** q_out) {
  const cb_write* q = (const cb_write*)stmt;
  if (!q) return fail(CB_EINVAL, "null statement");
  if (const char* why = cb::write_check(q->ns, q->ns_len, q->nk, q->cols, q->col_off, q->set, q->nc, q->op))
    return fail(CB_EINVAL, why);
  cb::write_pack(q->nk, q->cols, q->col_off, q->set, q->nc, q->op, cols);
  *q_out = q;
  return CB_OK;
}

// The batch on s: the staged inputs, the sizes, their three scans, one wait
// for the totals and the two counts, the outputs' block, the emit, and the
// wait that makes the result complete.
int write_rows(int dev, const cb_write* q, const cb::WriteCols& cols, const uint8_t* cells, const uint64_t* cell_off,
               const uint64_t* ts, uint64_t ts_all, const int32_t* old_which, const uint8_t* old_vals,
               const uint64_t* old_val_off, uint64_t n, hipStream_t s, void** out) {
  std::unique_ptr<cb_written, int (*)(void*)> r(new cb_written(), cb_written_destroy);
  r->device = dev;
  const uint64_t ncell = n * cols.width, nc = cols.sel.nc;
  const bool off_host = ncell && !is_device_ptr(cell_off), ts_host = ts && !is_device_ptr(ts);
  uint64_t cell_bytes = 0;  // what a host `cells` holds: up to the last offset
  const bool cells_host = ncell && !is_device_ptr(cells);
  if (cells_host) {
    if (off_host) cell_bytes = cell_off[ncell];
    else HIP_TRY(hipMemcpy(&cell_bytes, cell_off + ncell, 8, hipMemcpyDeviceToHost));
  }
  TempBlock tmp{dev};
  Staging up;  // (the statement and the namespace; lives until the first wait)
  cb::Carver& c = up.c;
  const size_t o_cols = c.take(sizeof(cb::WriteCols)), o_ns = c.take(q->ns_len);
  up.seal();
  const size_t o_coff = c.take(off_host ? (ncell + 1) * 8 : 0), o_cells = c.take(cell_bytes),
               o_ts = c.take(ts_host ? n * 8 : 0), o_klen = c.take(n * 8), o_vlen = c.take(n * 8),
               o_rlen = c.take(n * 8), o_sat = c.take(nc * n * 8), o_slen = c.take(nc * n * 8),
               o_scan = c.take(cb::scan_tmp_words(n) * 8), o_cnt = c.take(16);
  if (int rc = tmp.alloc(c, "device allocation failed for a write batch's scratch")) return rc;
  cb::Carver rc_;
  const size_t o_flags = rc_.take(n), o_ko = rc_.take((n + 1) * 8), o_vo = rc_.take((n + 1) * 8),
               o_lo = rc_.take((n + 1) * 8);
  if (int rc = pool_alloc_or(dev, rc_.total(), &r->block, &r->block_cap,
                             "device allocation failed for a write batch's offsets"))
    return rc;
  r->flags = (uint8_t*)r->block + o_flags;
  r->key_off = (uint64_t*)((uint8_t*)r->block + o_ko);
  r->val_off = (uint64_t*)((uint8_t*)r->block + o_vo);
  r->log_off = (uint64_t*)((uint8_t*)r->block + o_lo);
  up.put(o_cols, &cols, sizeof(cb::WriteCols));
  up.put(o_ns, q->ns, q->ns_len);
  cb::WriteBatch b{cells,    cell_off,    ts,
                   ts_all,   old_which,   old_vals,
                   old_val_off, n,        tmp.at(o_ns),
                   q->ns_len, cb::key_ctl(q->ns, q->ns_len) ? 1u : 0u};
  auto wait = [&](hipError_t e) {  // (host inputs are pageable: no return before the stream has read them)
    (void)hipStreamSynchronize(s);
    return hip_fail(e, "write: enqueue");
  };
  hipError_t e = up.upload(tmp, s);
  if (e == hipSuccess && off_host) {
    e = hipMemcpyAsync(tmp.at(o_coff), cell_off, (ncell + 1) * 8, hipMemcpyHostToDevice, s);
    b.cell_off = (const uint64_t*)tmp.at(o_coff);
  }
  if (e == hipSuccess && cells_host) {
    if (cell_bytes) e = hipMemcpyAsync(tmp.at(o_cells), cells, cell_bytes, hipMemcpyHostToDevice, s);
    b.cells = tmp.at(o_cells);
  }
  if (e == hipSuccess && ts_host) {
    e = hipMemcpyAsync(tmp.at(o_ts), ts, n * 8, hipMemcpyHostToDevice, s);
    b.ts = (const uint64_t*)tmp.at(o_ts);
  }
  const cb::WriteCols* dcols = (const cb::WriteCols*)tmp.at(o_cols);
  uint64_t *klen = (uint64_t*)tmp.at(o_klen), *vlen = (uint64_t*)tmp.at(o_vlen), *rlen = (uint64_t*)tmp.at(o_rlen);
  uint64_t *sat = (uint64_t*)tmp.at(o_sat), *slen = (uint64_t*)tmp.at(o_slen), *scan = (uint64_t*)tmp.at(o_scan);
  uint64_t* cnt = (uint64_t*)tmp.at(o_cnt);
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, 16, s);
  if (e == hipSuccess) e = cb::launch_write_size(b, dcols, r->flags, klen, vlen, rlen, sat, slen, cnt, s);
  if (e == hipSuccess) e = cb::launch_scan_u64(klen, r->key_off, n, scan, s);
  if (e == hipSuccess) e = cb::launch_scan_u64(vlen, r->val_off, n, scan, s);
  if (e == hipSuccess) e = cb::launch_scan_u64(rlen, r->log_off, n, scan, s);
  uint64_t t[3] = {0, 0, 0}, counts[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(&t[0], r->key_off + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&t[1], r->val_off + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&t[2], r->log_off + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(counts, cnt, 16, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return wait(e);
  HIP_TRY(hipStreamSynchronize(s));
  if (counts[1]) return fail(CB_EINVAL, "a row's log record of 4 GiB or more");
  if (counts[0] > n || t[0] < n || t[2] < t[1])  // (a key holds its ':'; a record is longer than its value)
    return fail(CB_EHIP, "write: inconsistent totals");
  r->count = n;
  r->key_bytes = t[0];
  r->val_bytes = t[1];
  r->log_bytes = t[2];
  r->flagged = counts[0];
  cb::Carver dc;  // (16 bytes behind each array: a reader may load past its end)
  const size_t o_keys = dc.take(t[0] + 16), o_vals = dc.take(t[1] + 16), o_log = dc.take(t[2] + 16);
  if (int rc = pool_alloc_or(dev, dc.total(), &r->data_block, &r->data_cap,
                             "device allocation failed for a write batch's bytes"))
    return rc;
  r->keys = (uint8_t*)r->data_block + o_keys;
  r->vals = (uint8_t*)r->data_block + o_vals;
  r->log = (uint8_t*)r->data_block + o_log;
  HIP_TRY(cb::launch_write_emit(b, dcols, r->flags, r->key_off, r->val_off, r->log_off, sat, slen, r->keys, r->vals,
                                r->log, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out = r.release();
  return CB_OK;
}

}  // namespace

extern "C" {

int cb_rows_write(const void* w, const uint8_t* cells, const uint64_t* cell_off, const uint64_t* ts, uint64_t ts_all,
                  const int32_t* old_which, const uint8_t* old_vals, const uint64_t* old_val_off, uint64_t n,
                  int device, void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  auto cols = std::make_unique<cb::WriteCols>();
  const cb_write* q = nullptr;
  if (int rc = take_write(w, cols.get(), &q)) return rc;
  const bool any_old = old_which || old_vals || old_val_off;
  if (any_old && q->op != CB_WRITE_UPDATE) return fail(CB_EINVAL, "old rows with an insert or a delete");
  if (any_old && (!old_which || !old_vals || !old_val_off)) return fail(CB_EINVAL, "old rows without all three arrays");
  if (n && cols->width && (!cells || !cell_off)) return fail(CB_EINVAL, "null cells with a non-zero count");
  if (n > (1ull << 56)) return fail(CB_EINVAL, "too many rows");
  hipStream_t s = (hipStream_t)stream;
  if (!n) {  // no row: a valid result and no device
    cb_written* r = new cb_written();
    r->device = device;
    *out = r;
    return CB_OK;
  }
  const uint64_t ncell = n * cols->width;
  if (ncell && !is_device_ptr(cell_off))  // (without a device every pointer counts as the host's)
    for (uint64_t j = 0; j < ncell; ++j)
      if (cell_off[j + 1] < cell_off[j]) return fail(CB_EINVAL, "cell offsets decrease");
  if (int rc = cb_init(device)) return rc;
  DeviceGuard dg(device);
  if (any_old && (!is_device_ptr(old_which) || !is_device_ptr(old_vals) || !is_device_ptr(old_val_off)))
    return fail(CB_EINVAL, "the old rows are not in device memory");
  (void)workspace(device, s);  // (registers s: the pool retires blocks behind it)
  return write_rows(device, q, *cols, cells, cell_off, ts, ts_all, old_which, old_vals, old_val_off, n, s, out);
}

int cb_row_write(const void* w, const uint8_t* cells, const uint64_t* cell_off, uint64_t ts, const uint8_t* old_value,
                 uint64_t old_len, int has_old, uint8_t* out, uint64_t cap, uint64_t* key_len, uint64_t* val_len,
                 uint64_t* log_len, uint8_t* flags) {
  if (key_len) *key_len = 0;
  if (val_len) *val_len = 0;
  if (log_len) *log_len = 0;
  if (flags) *flags = 0;
  if (!key_len || !val_len || !log_len) return fail(CB_EINVAL, "null argument");
  auto cols = std::make_unique<cb::WriteCols>();
  const cb_write* q = nullptr;
  if (int rc = take_write(w, cols.get(), &q)) return rc;
  if (has_old && q->op != CB_WRITE_UPDATE) return fail(CB_EINVAL, "old rows with an insert or a delete");
  if (has_old && old_len && !old_value) return fail(CB_EINVAL, "null old value with a length");
  if (cols->width && (!cells || !cell_off)) return fail(CB_EINVAL, "null cells with a non-zero count");
  for (uint32_t j = 0; j < cols->width; ++j)
    if (cell_off[j + 1] < cell_off[j]) return fail(CB_EINVAL, "cell offsets decrease");
  if (cap && !out) return fail(CB_EINVAL, "null output with a capacity");
  cb::ArraySlots slots;
  uint8_t f = 0;
  uint64_t kl = 0, vl = 0, rl = 0;
  cb::DecodedBytes old(has_old ? old_value : nullptr, has_old ? old_len : 0);
  cb::write_size(*cols, q->ns_len, cb::key_ctl(q->ns, q->ns_len), cells, cell_off, has_old != 0, old, slots, &f, &kl,
                 &vl, &rl);
  if (rl >= cb::kWriteMaxRecord) return fail(CB_EINVAL, "a row's log record of 4 GiB or more");
  *key_len = kl;
  *val_len = vl;
  *log_len = rl;
  if (flags) *flags = f;
  if (out && kl + vl + rl <= cap)
    cb::write_emit(*cols, q->ns, q->ns_len, cells, cell_off, ts, old, f, slots, out, out + kl, out + kl + vl);
  return CB_OK;
}

int cb_written_info(const void* written, uint64_t* count, uint64_t* key_bytes, uint64_t* val_bytes,
                    uint64_t* log_bytes, uint64_t* flagged) {
  const cb_written* r = (const cb_written*)written;
  if (!r) return fail(CB_EINVAL, "null written batch");
  if (count) *count = r->count;
  if (key_bytes) *key_bytes = r->key_bytes;
  if (val_bytes) *val_bytes = r->val_bytes;
  if (log_bytes) *log_bytes = r->log_bytes;
  if (flagged) *flagged = r->flagged;
  return CB_OK;
}

int cb_written_arrays(const void* written, const uint8_t** keys, const uint64_t** key_off, const uint8_t** vals,
                      const uint64_t** val_off, const uint8_t** log, const uint64_t** log_off,
                      const uint8_t** flags) {
  const cb_written* r = (const cb_written*)written;
  if (!r) return fail(CB_EINVAL, "null written batch");
  if (keys) *keys = r->keys;
  if (key_off) *key_off = r->key_off;
  if (vals) *vals = r->vals;
  if (val_off) *val_off = r->val_off;
  if (log) *log = r->log;
  if (log_off) *log_off = r->log_off;
  if (flags) *flags = r->flags;
  return CB_OK;
}

int cb_written_copy(const void* written, uint8_t* keys, uint64_t* key_off, uint8_t* vals, uint64_t* val_off,
                    uint8_t* log, uint64_t* log_off, uint8_t* flags) {
  const cb_written* r = (const cb_written*)written;
  if (!r) return fail(CB_EINVAL, "null written batch");
  if (!r->count) {  // no device memory is held: the offsets of no row are one 0
    const uint64_t zero = 0;
    for (uint64_t* o : {key_off, val_off, log_off})
      if (o)
        if (int rc = put_bytes((uint8_t*)o, &zero, 8)) return rc;
    return CB_OK;
  }
  DeviceGuard dg(r->device);
  const uint64_t n = r->count;
  if (keys && r->key_bytes) HIP_TRY(hipMemcpy(keys, r->keys, r->key_bytes, hipMemcpyDefault));
  if (key_off) HIP_TRY(hipMemcpy(key_off, r->key_off, (n + 1) * 8, hipMemcpyDefault));
  if (vals && r->val_bytes) HIP_TRY(hipMemcpy(vals, r->vals, r->val_bytes, hipMemcpyDefault));
  if (val_off) HIP_TRY(hipMemcpy(val_off, r->val_off, (n + 1) * 8, hipMemcpyDefault));
  if (log && r->log_bytes) HIP_TRY(hipMemcpy(log, r->log, r->log_bytes, hipMemcpyDefault));
  if (log_off) HIP_TRY(hipMemcpy(log_off, r->log_off, (n + 1) * 8, hipMemcpyDefault));
  if (flags) HIP_TRY(hipMemcpy(flags, r->flags, n, hipMemcpyDefault));
  return CB_OK;
}

int cb_written_destroy(void* written) {
  cb_written* r = (cb_written*)written;
  if (!r) return CB_OK;
  pool_release(r->device, r->block, r->block_cap);
  pool_release(r->device, r->data_block, r->data_cap);
  delete r;
  return CB_OK;
}

}  // extern "C"
