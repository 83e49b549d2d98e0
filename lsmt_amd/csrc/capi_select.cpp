// capi_select.cpp — rows projected and re-encoded on the device
// (cb_scan_select, cb_rows_select; select.hpp) and, for one row on the host,
// cb_row_select, with the result's accessors (cb_rows_*). The rule is
// rowselect.hpp's; the rows are a finished scan result's, or the buffers an
// enqueue-only cb_*get_many fills.
//
// Reference: src/query.rs:365-432 (exec_select_schema, whose response bytes
// the result's text is), src/cluster.rs:404-421 (the coordinator's parse of
// the `key \t ts \t val` form).
#include "capi_merge.hpp"
#include "select.hpp"

using namespace cbx;

// A selection's result: flags | row_at | row_len in one pool block, the text
// in another (sized only once the rows' lengths are known), complete when the
// call returns. A result of no rows holds no device memory.
struct cb_rows {
  int device = 0, mode = 0;
  uint64_t count = 0, with_text = 0, bytes = 0;
  void *block = nullptr, *text_block = nullptr;
  size_t block_cap = 0, text_cap = 0;
  uint8_t *flags = nullptr, *text = nullptr;
  uint64_t *row_at = nullptr, *row_len = nullptr;
};

namespace {

// A cb_select checked and packed (rowselect.hpp), the mode and the result's
// place: every selecting entry's first step, before any device is touched.
int take_select(const void* sel, int mode, cb::SelectCols* cols) {
  const cb_select* q = (const cb_select*)sel;
  if (!q) return fail(CB_EINVAL, "null selection");
  if (const char* why = cb::select_check(q->cols, q->col_off, q->part, q->cast, q->nc)) return fail(CB_EINVAL, why);
  if (mode != CB_SELECT_JSON && mode != CB_SELECT_META) return fail(CB_EINVAL, "a mode that is neither 0 nor 1");
  cb::select_pack(q->cols, q->col_off, q->part, q->cast, q->nc, cols);
  return CB_OK;
}

// The response's length from the scanned total (select.hpp).
uint64_t response_bytes(int mode, uint64_t total) {
  if (mode == CB_SELECT_JSON) return total ? total + 1 : 2;
  return total ? total - 1 : 0;
}

// The selection over rows in device memory (rows.range_off and rows.skip:
// host memory, staged here), on s: the sizes, their scan, one wait for the
// total and the rows with text, the text's block, the write, and the wait
// that makes the result complete.
int select_rows(int dev, cb::SelectRows rows, const cb::SelectCols& cols, int mode, hipStream_t s, void** out) {
  std::unique_ptr<cb_rows, int (*)(void*)> r(new cb_rows(), cb_rows_destroy);
  r->device = dev;
  r->mode = mode;
  r->bytes = response_bytes(mode, 0);
  const uint64_t n = rows.n;
  if (!n) {
    *out = r.release();
    return CB_OK;
  }
  TempBlock tmp{dev};
  Staging up;  // (lives until the first wait)
  cb::Carver& c = up.c;
  const size_t o_sel = c.take(sizeof(cb::SelectCols)), o_roff = c.take(rows.skip ? (rows.nr + 1ull) * 8 : 0),
               o_skip = c.take(rows.skip ? rows.nr * 4ull : 0);
  up.seal();
  const uint64_t slots = (uint64_t)cols.nc * n;
  const size_t o_inc = c.take(n * 8), o_off = c.take((n + 2) * 8), o_sat = c.take(slots * 8),
               o_slen = c.take(slots * 8), o_scan = c.take(cb::scan_tmp_words(n) * 8);
  if (int rc = tmp.alloc(c, "device allocation failed for a selection's scratch")) return rc;
  cb::Carver rc_;
  const size_t o_flags = rc_.take(n), o_at = rc_.take(n * 8), o_len = rc_.take(n * 8);
  if (int rc = pool_alloc_or(dev, rc_.total(), &r->block, &r->block_cap,
                             "device allocation failed for a selection's result"))
    return rc;
  r->flags = (uint8_t*)r->block + o_flags;
  r->row_at = (uint64_t*)((uint8_t*)r->block + o_at);
  r->row_len = (uint64_t*)((uint8_t*)r->block + o_len);
  up.put(o_sel, &cols, sizeof(cb::SelectCols));
  if (rows.skip) {
    up.put(o_roff, rows.range_off, (rows.nr + 1ull) * 8);
    up.put(o_skip, rows.skip, rows.nr * 4ull);
    rows.range_off = (const uint64_t*)tmp.at(o_roff);
    rows.skip = (const uint32_t*)tmp.at(o_skip);
  }
  const cb::SelectCols* dsel = (const cb::SelectCols*)tmp.at(o_sel);
  uint64_t *inc = (uint64_t*)tmp.at(o_inc), *off = (uint64_t*)tmp.at(o_off);
  uint64_t *sat = (uint64_t*)tmp.at(o_sat), *slen = (uint64_t*)tmp.at(o_slen);
  auto wait = [&](hipError_t e) {  // (`up` is pageable: no return before the stream has read it)
    (void)hipStreamSynchronize(s);
    return hip_fail(e, "select: enqueue");
  };
  HIP_TRY(up.upload(tmp, s));
  hipError_t e = hipMemsetAsync(off + n + 1, 0, 8, s);  // the rows with text, behind the scan's total
  if (e == hipSuccess) e = cb::launch_select_size(rows, dsel, mode, r->flags, inc, sat, slen, off + n + 1, s);
  if (e == hipSuccess) e = cb::launch_scan_u64(inc, off, n, (uint64_t*)tmp.at(o_scan), s);
  uint64_t t[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(t, off + n, sizeof t, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return wait(e);
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t total = t[0], with_text = t[1];
  if (with_text > n || total < 3 * with_text || (total != 0) != (with_text != 0))  // (a text and its separator: 3 bytes at least)
    return fail(CB_EHIP, "select: inconsistent totals");
  r->count = n;
  r->with_text = with_text;
  r->bytes = response_bytes(mode, total);
  if (int rc = pool_alloc_or(dev, total + 2, &r->text_block, &r->text_cap,
                             "device allocation failed for a selection's text"))
    return rc;
  r->text = (uint8_t*)r->text_block;
  HIP_TRY(cb::launch_select_write(rows, dsel, mode, r->flags, inc, off, sat, slen, r->row_at, r->row_len, r->text, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out = r.release();
  return CB_OK;
}

}  // namespace

extern "C" {

// The entries of a finished result on the null stream, as cb_scan_match runs.
int cb_scan_select(const void* scan, const uint32_t* skip, const void* sel, int mode, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  const cb_scan* r = (const cb_scan*)scan;
  auto cols = std::make_unique<cb::SelectCols>();
  if (int rc = take_select(sel, mode, cols.get())) return rc;
  if (!r) return fail(CB_EINVAL, "null scan");
  cb::SelectRows rows{r->key_off, r->keys, nullptr, r->val_off, r->vals, r->count, nullptr, nullptr, 0, 0};
  if (skip && r->count) {
    rows.range_off = r->range_off.data();
    rows.skip = skip;
    rows.nr = (uint32_t)(r->range_off.size() - 1);
  }
  if (!r->count) return select_rows(r->device, rows, *cols, mode, nullptr, out);
  DeviceGuard dg(r->device);
  note_stream(r->device, nullptr);  // (the pool retires the scratch behind the null stream too)
  return select_rows(r->device, rows, *cols, mode, nullptr, out);
}

int cb_rows_select(const uint8_t* keys, const uint64_t* key_off, const int32_t* which, const uint8_t* vals,
                   const uint64_t* val_off, uint64_t n, uint32_t skip, const void* sel, int mode, int device,
                   void* stream, void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  auto cols = std::make_unique<cb::SelectCols>();
  if (int rc = take_select(sel, mode, cols.get())) return rc;
  if (n && (!keys || !key_off || !vals || !val_off)) return fail(CB_EINVAL, "null rows with a non-zero count");
  cb::SelectRows rows{key_off, keys, which, val_off, vals, n, nullptr, nullptr, 0, skip};
  hipStream_t s = (hipStream_t)stream;
  if (!n) return select_rows(device, rows, *cols, mode, s, out);
  if (int rc = cb_init(device)) return rc;
  DeviceGuard dg(device);
  if (!is_device_ptr(keys) || !is_device_ptr(key_off) || !is_device_ptr(vals) || !is_device_ptr(val_off) ||
      (which && !is_device_ptr(which)))
    return fail(CB_EINVAL, "the rows are not in device memory");
  (void)workspace(device, s);  // (registers s: the pool retires blocks behind it)
  return select_rows(device, rows, *cols, mode, s, out);
}

int cb_row_select(const uint8_t* key, uint64_t key_len, uint32_t skip, const uint8_t* value, uint64_t value_len,
                  const void* sel, int mode, uint8_t* out, uint64_t cap, uint64_t* len, uint8_t* flags) {
  if (len) *len = 0;
  if (flags) *flags = 0;
  if (!len) return fail(CB_EINVAL, "null argument");
  auto cols = std::make_unique<cb::SelectCols>();
  if (int rc = take_select(sel, mode, cols.get())) return rc;
  if ((key_len && !key) || (value_len && !value)) return fail(CB_EINVAL, "null key or value with a length");
  if (cap && !out) return fail(CB_EINVAL, "null text with a capacity");
  cb::ArraySlots slots;
  uint8_t f = 0;
  cb::DecodedBytes v(value, value_len);
  *len = cb::select_size(*cols, key, key_len, skip, false, v, mode, slots, &f);
  if (flags) *flags = f;
  if ((f & cb::kRowText) && *len <= cap) cb::select_write(*cols, key, key_len, skip, v, mode, f, slots, out);
  return CB_OK;
}

int cb_rows_info(const void* rows, uint64_t* count, uint64_t* with_text, uint64_t* bytes) {
  const cb_rows* r = (const cb_rows*)rows;
  if (!r) return fail(CB_EINVAL, "null rows");
  if (count) *count = r->count;
  if (with_text) *with_text = r->with_text;
  if (bytes) *bytes = r->bytes;
  return CB_OK;
}

int cb_rows_text(const void* rows, uint8_t* text, uint64_t* row_at, uint64_t* row_len, uint8_t* flags) {
  const cb_rows* r = (const cb_rows*)rows;
  if (!r) return fail(CB_EINVAL, "null rows");
  if (!r->count) return text && r->bytes ? put_bytes(text, "[]", r->bytes) : CB_OK;  // no device memory is held
  DeviceGuard dg(r->device);
  if (text && r->bytes) HIP_TRY(hipMemcpy(text, r->text, r->bytes, hipMemcpyDefault));
  if (row_at) HIP_TRY(hipMemcpy(row_at, r->row_at, r->count * 8, hipMemcpyDefault));
  if (row_len) HIP_TRY(hipMemcpy(row_len, r->row_len, r->count * 8, hipMemcpyDefault));
  if (flags) HIP_TRY(hipMemcpy(flags, r->flags, r->count, hipMemcpyDefault));
  return CB_OK;
}

int cb_rows_destroy(void* rows) {
  cb_rows* r = (cb_rows*)rows;
  if (!r) return CB_OK;
  pool_release(r->device, r->block, r->block_cap);
  pool_release(r->device, r->text_block, r->text_cap);
  delete r;
  return CB_OK;
}

}  // extern "C"
