// capi_replay.cpp — the write-ahead log replayed on the device into the table
// a flush of the replayed memtable would write (cb_log_replay), and the
// verdict of one piece of a log on the host (cb_log_line). The rule is
// logline.hpp's, the kernels replay.hip's; from the sort on the steps are the
// merge's and compaction's own (capi_merge.hpp).
//
// Reference: src/wal.rs:14-31 (parse_entries), src/lib.rs:30-39 (Database::new
// inserts the records in log order), src/lib.rs:96-102 (the record's writer),
// src/sstable.rs:51-87 (the file the flush writes).
#include "capi_merge.hpp"
#include "logline.hpp"
#include "replay.hpp"

using namespace cbx;

static_assert(cb::kLogBadKey == CB_EUTF8 && cb::kLogBadValue == CB_EBASE64, "logline.hpp's kinds are the ABI's codes");

namespace {

// ---- cb_log_replay's steps, in the order it takes them ----

// The log's pieces on the device: the log itself with a table file's 16 bytes
// of slack, and per non-empty piece its record (start, TAB) and length.
struct LogPieces {
  uint8_t* data = nullptr;
  uint64_t len = 0, nl = 0;
  cb::LineRec* rec = nullptr;
  uint32_t *llen = nullptr, *vdl = nullptr, *err = nullptr;
  uint64_t *has = nullptr, *klen = nullptr, *has_scan = nullptr, *len_scan = nullptr, *scan = nullptr, *bad = nullptr;
};

// 1: the log staged (host or device memory alike) and its non-empty pieces
// counted: the line index's count and scan, one wait for the count.
int stage_log(const uint8_t* log, uint64_t len, TempBlock& blk, LogPieces* p, uint64_t** base_out, hipStream_t s) {
  const uint64_t nb = cb::line_blocks(len);
  cb::Carver c;
  const size_t o_data = c.take(len + 16), o_cnt = c.take(nb * 8), o_base = c.take((nb + 1) * 8),
               o_tmp = c.take(cb::scan_tmp_words(nb) * 8);
  if (int rc = blk.alloc(c, "device allocation failed for a log")) return rc;
  p->data = blk.at(o_data);
  p->len = len;
  uint64_t *cnt = (uint64_t*)blk.at(o_cnt), *base = (uint64_t*)blk.at(o_base);
  HIP_TRY(hipMemsetAsync(p->data + len, 0, 16, s));
  HIP_TRY(hipMemcpyAsync(p->data, log, len, hipMemcpyDefault, s));
  HIP_TRY(cb::launch_line_count(p->data, len, cnt, s));
  HIP_TRY(cb::launch_scan_u64(cnt, base, nb, (uint64_t*)blk.at(o_tmp), s));
  HIP_TRY(hipMemcpyAsync(&p->nl, base + nb, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (p->nl > len) return fail(CB_EHIP, "log replay: inconsistent piece count");
  *base_out = base;
  return CB_OK;
}

// 2: the pieces' starts, ends and TABs (the line index's emit and finish),
// logline.hpp's verdict of each (k_log_mark) and the scans that place the
// entries' keys; the counts come back with the first bad piece (one wait).
// h = {the first bad piece packed, entries, their keys' bytes}.
int mark_pieces(LogPieces* p, const uint64_t* base, TempBlock& blk, hipStream_t s, uint64_t (&h)[3]) {
  const uint64_t nl = p->nl;
  cb::Carver c;
  const size_t o_start = c.take(nl * 8), o_end = c.take(nl * 8), o_rec = c.take(nl * sizeof(cb::LineRec)),
               o_llen = c.take(nl * 4), o_vdl = c.take(nl * 4), o_has = c.take(nl * 8), o_klen = c.take(nl * 8),
               o_hs = c.take((nl + 1) * 8), o_ls = c.take((nl + 1) * 8), o_scan = c.take(cb::scan_tmp_words(nl) * 8),
               o_bad = c.take(8), o_err = c.take(4);
  if (int rc = blk.alloc(c, "device allocation failed for a log's pieces")) return rc;
  uint64_t *start = (uint64_t*)blk.at(o_start), *end = (uint64_t*)blk.at(o_end);
  p->rec = (cb::LineRec*)blk.at(o_rec);
  p->llen = (uint32_t*)blk.at(o_llen);
  p->vdl = (uint32_t*)blk.at(o_vdl);
  p->has = (uint64_t*)blk.at(o_has);
  p->klen = (uint64_t*)blk.at(o_klen);
  p->has_scan = (uint64_t*)blk.at(o_hs);
  p->len_scan = (uint64_t*)blk.at(o_ls);
  p->scan = (uint64_t*)blk.at(o_scan);
  p->bad = (uint64_t*)blk.at(o_bad);
  p->err = (uint32_t*)blk.at(o_err);
  HIP_TRY(hipMemsetAsync(end, 0xFF, nl * 8, s));
  HIP_TRY(hipMemsetAsync(p->err, 0, 4, s));
  HIP_TRY(hipMemsetAsync(p->bad, 0xFF, 8, s));
  // (has / klen of a log with an oversized piece are never written: the scans then run over zeros)
  HIP_TRY(hipMemsetAsync(p->has, 0, (size_t)((uint8_t*)p->has_scan - (uint8_t*)p->has), s));
  HIP_TRY(cb::launch_line_emit(p->data, p->len, base, start, end, s));
  HIP_TRY(cb::launch_line_finish(p->data, p->len, nl, start, end, p->rec, p->llen, p->err, s));
  HIP_TRY(cb::launch_log_mark(p->data, p->rec, p->llen, nl, p->err, p->has, p->klen, p->vdl, p->bad, s));
  HIP_TRY(cb::launch_scan_u64(p->has, p->has_scan, nl, p->scan, s));
  HIP_TRY(cb::launch_scan_u64(p->klen, p->len_scan, nl, p->scan, s));
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&err, p->err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h[0], p->bad, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h[1], p->has_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h[2], p->len_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (err) return fail(CB_EINVAL, "a piece of the log is 4 GiB or longer");
  if (h[1] > nl || h[2] > p->len) return fail(CB_EHIP, "log replay: inconsistent entry counts");
  if (h[1] > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many entries for one replay");
  return CB_OK;
}

// Wal::new's Err (src/wal.rs:21-26): the first failing piece, its kind from
// the packed word, its offset read back (one wait).
int bad_piece(const LogPieces& p, uint64_t packed, hipStream_t s, cb_log_stats* st) {
  const uint64_t l = cb::log_bad_piece(packed);
  if (l >= p.nl) return fail(CB_EHIP, "log replay: inconsistent bad piece");
  uint64_t off = 0;
  HIP_TRY(hipMemcpyAsync(&off, &p.rec[l].start, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  st->bad_line = l;
  st->bad_offset = off;
  char msg[160];
  if (cb::log_bad_is_value(packed)) {
    std::snprintf(msg, sizeof msg, "Wal::new: the value on line %llu (byte %llu) of the log is not STANDARD base64",
                  (unsigned long long)l, (unsigned long long)off);
    return fail(CB_EBASE64, msg);
  }
  std::snprintf(msg, sizeof msg, "Wal::new: the key on line %llu (byte %llu) of the log is not UTF-8",
                (unsigned long long)l, (unsigned long long)off);
  return fail(CB_EUTF8, msg);
}

// 3: the entries as the merge's records, newest first (k_log_gather in the
// place of compaction's gather), then the merge as it stands: the stable sort,
// the plain select (every value decodes here, so a record looks at one
// neighbour) and the survivors' totals (one wait).
int merge_entries(const LogPieces& p, uint64_t entries, TempBlock& tmp, Merge* mg, hipStream_t s, uint64_t (&h)[3]) {
  // (the keys' bytes are among the log's: the bound compaction takes of its files)
  if (int rc = merge_alloc(0, entries, p.len, cb::MergeOrder::newest, tmp, mg)) return rc;
  if (int rc = enqueue_sort_begin(*mg, s)) return rc;
  HIP_TRY(cb::launch_log_gather(p.data, p.rec, p.llen, p.vdl, p.nl, p.has_scan, p.len_scan, mg->kb, mg->ko, mg->side,
                                &mg->dr->dmask[0][0], s));
  if (int rc = enqueue_sort_select(*mg, kNewest, s)) return rc;
  return merge_totals(*mg, s, h);
}

}  // namespace

extern "C" {

// Every temporary is carved from pool blocks released stream-ordered on return
// (error returns included). The call waits for its own stream for the pieces'
// count, for the entries' counts and the first bad piece, for the survivors'
// totals, for the directory's map and at the end (the zone bounds), as
// cb_tables_compact does from its totals on.
int cb_log_replay(const uint8_t* log, uint64_t len, uint64_t m_bits, int device, void* stream, cb_table** table_out,
                  cb_filter** bloom_out, void* stats_out) {
  cb_log_stats* stats = static_cast<cb_log_stats*>(stats_out);
  cb_log_stats st{0, 0, 0, ~0ull, ~0ull};
  if (stats) *stats = st;
  if (bloom_out) *bloom_out = nullptr;
  if (!table_out) return fail(CB_EINVAL, "null argument");
  *table_out = nullptr;
  if (bloom_out && m_bits == 0) return zero_m_error();
  if (!log && len) return fail(CB_EINVAL, "null log with a non-zero length");
  int rc = cb_init(device);
  if (rc) return rc;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  Workspace& ws = workspace(device, s);  // (registers s: the pool retires blocks behind it)
  std::unique_ptr<cb_table, int (*)(cb_table*)> t(new cb_table(), cb_table_destroy);
  std::unique_ptr<cb_filter, int (*)(cb_filter*)> f(nullptr, cb_filter_destroy);
  t->device = device;
  if (bloom_out) {
    cb_filter* fp = nullptr;
    if ((rc = cb_filter_create(m_bits, device, &fp))) return rc;
    f.reset(fp);
  }
  TempBlock staged{device}, pieces{device}, tmp{device}, keys{device};
  uint64_t h[3] = {0, 0, 0};  // the survivors' lines, file bytes and key bytes
  LogPieces p;
  uint64_t* base = nullptr;
  if (len && (rc = stage_log(log, len, staged, &p, &base, s))) return rc;
  st.lines = p.nl;
  if (p.nl) {
    uint64_t e[3] = {cb::kLogNoBad, 0, 0};
    rc = mark_pieces(&p, base, pieces, s, e);
    if (!rc) st.entries = e[1];
    if (!rc && e[0] != cb::kLogNoBad) rc = bad_piece(p, e[0], s, &st);
    if (rc) {
      if (stats) *stats = st;
      return rc;
    }
    if (st.entries) {
      Merge mg;
      KeptKeys k;
      if ((rc = merge_entries(p, st.entries, tmp, &mg, s, h))) return rc;
      if (!h[0]) return fail(CB_EHIP, "log replay: entries without a key");
      if ((rc = format_survivors(t.get(), mg, h, keys, &k, s))) return rc;
      if (f) {
        // BloomFilter::new(m) + insert per kept key (src/sstable.rs:59-63)
        std::lock_guard<std::mutex> lk(ws.mu);
        if ((rc = insert_locked(ws, f.get(), k.kb, k.ko, 0, h[0], s))) return rc;
      }
      if ((rc = finish_compacted(t.get(), mg, k, h, s))) return rc;
    }
  }
  // no entry: the empty file, as cb_tables_compact's empty result
  if (!h[0] && (rc = finish_empty_file(t.get(), s))) return rc;
  st.keys = h[0];
  if (stats) *stats = st;
  if (bloom_out) *bloom_out = f.release();
  *table_out = t.release();
  return CB_OK;
}

int cb_log_line(const uint8_t* piece, uint64_t len, int* kind, uint64_t* key_len, uint64_t* value_len) {
  if (!kind || (!piece && len)) return fail(CB_EINVAL, "null argument");
  for (uint64_t i = 0; i < len; ++i)
    if (piece[i] == '\n') return fail(CB_EINVAL, "a piece holds no newline: the log is split on them");
  const cb::LogLine v = cb::log_line(piece, len);
  *kind = v.kind;
  if (key_len) *key_len = v.klen;
  if (value_len) *value_len = v.vdl;
  return CB_OK;
}

}  // extern "C"
