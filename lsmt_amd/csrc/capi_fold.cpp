// capi_fold.cpp — the coordinator's read merge: the replicas' replies folded
// by timestamp into the response (cb_replies_fold) on the device or, for
// device == -1, on the host, the result's accessors (cb_fold_*) and the verdict
// of one piece on the host (cb_reply_line). The rule is replyline.hpp's, the
// kernels fold.hip's, the host fold replyfold.hpp's; between the gather and
// the winners the steps are the merge's own (capi_merge.hpp).
//
// Reference: src/cluster.rs:394-473 (Cluster::execute's tail for a read).
#include "capi_merge.hpp"
#include "fold.hpp"
#include "replyfold.hpp"
#include "replyline.hpp"

using namespace cbx;

static_assert(cb::kReplyBadUtf8 == CB_EUTF8, "replyline.hpp's kinds are the ABI's codes");
static_assert(cb::kFoldText == CB_FOLD_TEXT && cb::kFoldDead == CB_FOLD_DEAD && cb::kFoldHost == CB_FOLD_HOST,
              "replyline.hpp's flags are the ABI's");
static_assert(sizeof(cb_fold_stats) == 11 * 8 && sizeof(cb::FoldCounts) == 6 * 8, "packed words");

// A fold's result. A host fold (device -1) keeps everything in `h`; a device
// fold keeps the winners' rows in one pool block and the text in another
// (sized only once the winners' lengths are known), or, where no entry exists,
// the short text in h.text and no device memory at all.
struct cb_fold {
  int device = -1;
  cb_fold_stats st{};
  cb::HostFold h;
  void *block = nullptr, *text_block = nullptr;
  size_t block_cap = 0, text_cap = 0;
  cb::FoldRows rows{};
  uint8_t* text = nullptr;
};

namespace {

void stats_of(const cb::HostFold& h, cb_fold_stats* st) {
  *st = cb_fold_stats{h.replies, h.lines,     h.entries, h.others,    h.keys,      h.with_text,
                      h.dead,    h.host_rows, h.bytes,   h.bad_reply, h.bad_offset};
}

// ---- cb_replies_fold's steps on the device, in the order it takes them ----

// The staged replies (fold.hpp) and what the marks leave per piece.
struct ReplyPieces {
  uint8_t* data = nullptr;
  uint64_t len = 0, nl = 0;
  uint32_t nr = 0;
  uint64_t *soff = nullptr, *coff = nullptr;  // device: staged / caller's offsets of the replies
  cb::LineRec* rec = nullptr;
  uint32_t *llen = nullptr, *err = nullptr;
  cb::ReplyPiece* pc = nullptr;
  uint64_t *has = nullptr, *klen = nullptr, *has_scan = nullptr, *len_scan = nullptr, *scan = nullptr;
  cb::FoldCounts* cnt = nullptr;
};

// 1: the replies staged, each with its separator behind it, and the non-empty
// pieces counted: the line index's count and scan, one wait for the count
// (which also covers the pageable offsets in hoff).
int stage_replies(const uint8_t* bytes, const uint64_t* off, uint32_t nr, const std::vector<uint64_t>& hoff,
                  TempBlock& blk, ReplyPieces* p, uint64_t** base_out, hipStream_t s) {
  const uint64_t len = hoff[nr];  // the replies' bytes and nr separators
  const uint64_t nb = cb::line_blocks(len);
  cb::Carver c;
  const size_t o_off = c.take(2 * (nr + 1ull) * 8), o_data = c.take(len + 16), o_cnt = c.take(nb * 8),
               o_base = c.take((nb + 1) * 8), o_tmp = c.take(cb::scan_tmp_words(nb) * 8);
  if (int rc = blk.alloc(c, "device allocation failed for the replies")) return rc;
  p->data = blk.at(o_data);
  p->len = len;
  p->nr = nr;
  p->soff = (uint64_t*)blk.at(o_off);
  p->coff = p->soff + nr + 1;
  uint64_t *cnt = (uint64_t*)blk.at(o_cnt), *base = (uint64_t*)blk.at(o_base);
  HIP_TRY(hipMemcpyAsync(p->soff, hoff.data(), 2 * (nr + 1ull) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(p->data + len, 0, 16, s));
  for (uint32_t r = 0; r < nr; ++r) {
    const uint64_t n = off[r + 1] - off[r];
    if (n) HIP_TRY(hipMemcpyAsync(p->data + hoff[r], bytes + off[r], n, hipMemcpyDefault, s));
    HIP_TRY(hipMemsetAsync(p->data + hoff[r] + n, '\n', 1, s));
  }
  HIP_TRY(cb::launch_line_count(p->data, len, cnt, s));
  HIP_TRY(cb::launch_scan_u64(cnt, base, nb, (uint64_t*)blk.at(o_tmp), s));
  HIP_TRY(hipMemcpyAsync(&p->nl, base + nb, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (p->nl > len) return fail(CB_EHIP, "replies fold: inconsistent piece count");
  *base_out = base;
  return CB_OK;
}

// 2: the pieces' starts, ends and first TABs (the line index's emit and
// finish), replyline.hpp's verdict of each (k_reply_mark) and the scans that
// place the entries' keys; the counts come back (one wait). e = {entries,
// their keys' bytes}.
int mark_replies(ReplyPieces* p, const uint64_t* base, TempBlock& blk, hipStream_t s, cb::FoldCounts* hc,
                 uint64_t (&e)[2]) {
  const uint64_t nl = p->nl;
  cb::Carver c;
  const size_t o_start = c.take(nl * 8), o_end = c.take(nl * 8), o_rec = c.take(nl * sizeof(cb::LineRec)),
               o_llen = c.take(nl * 4), o_pc = c.take(nl * sizeof(cb::ReplyPiece)), o_has = c.take(nl * 8),
               o_klen = c.take(nl * 8), o_hs = c.take((nl + 1) * 8), o_ls = c.take((nl + 1) * 8),
               o_scan = c.take(cb::scan_tmp_words(nl) * 8), o_cnt = c.take(sizeof(cb::FoldCounts)), o_err = c.take(4);
  if (int rc = blk.alloc(c, "device allocation failed for the replies' pieces")) return rc;
  uint64_t *start = (uint64_t*)blk.at(o_start), *end = (uint64_t*)blk.at(o_end);
  p->rec = (cb::LineRec*)blk.at(o_rec);
  p->llen = (uint32_t*)blk.at(o_llen);
  p->pc = (cb::ReplyPiece*)blk.at(o_pc);
  p->has = (uint64_t*)blk.at(o_has);
  p->klen = (uint64_t*)blk.at(o_klen);
  p->has_scan = (uint64_t*)blk.at(o_hs);
  p->len_scan = (uint64_t*)blk.at(o_ls);
  p->scan = (uint64_t*)blk.at(o_scan);
  p->cnt = (cb::FoldCounts*)blk.at(o_cnt);
  p->err = (uint32_t*)blk.at(o_err);
  HIP_TRY(hipMemsetAsync(end, 0xFF, nl * 8, s));
  HIP_TRY(hipMemsetAsync(p->err, 0, 4, s));
  HIP_TRY(hipMemsetAsync(p->cnt, 0, sizeof(cb::FoldCounts), s));
  HIP_TRY(hipMemsetAsync(&p->cnt->bad, 0xFF, 8, s));
  // (has / klen of replies with an oversized piece are never written: the scans then run over zeros)
  HIP_TRY(hipMemsetAsync(p->has, 0, (size_t)((uint8_t*)p->has_scan - (uint8_t*)p->has), s));
  HIP_TRY(cb::launch_line_emit(p->data, p->len, base, start, end, s));
  HIP_TRY(cb::launch_line_finish(p->data, p->len, nl, start, end, p->rec, p->llen, p->err, s));
  HIP_TRY(cb::launch_reply_mark(p->data, p->rec, p->llen, nl, p->err, p->soff, p->nr, p->pc, p->has, p->klen, p->cnt,
                                s));
  HIP_TRY(cb::launch_scan_u64(p->has, p->has_scan, nl, p->scan, s));
  HIP_TRY(cb::launch_scan_u64(p->klen, p->len_scan, nl, p->scan, s));
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&err, p->err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hc, p->cnt, sizeof *hc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&e[0], p->has_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&e[1], p->len_scan + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (err) return fail(CB_EINVAL, "a piece of a reply is 4 GiB or longer");
  if (e[0] > nl || e[1] > p->len || hc->lines > nl || e[0] + hc->others != hc->lines)
    return fail(CB_EHIP, "replies fold: inconsistent entry counts");
  if (e[0] > 0xFFFFFFFFull) return fail(CB_EINVAL, "too many entries for one fold");
  return CB_OK;
}

// The first failing piece: its reply and its place in the caller's bytes, read
// back (one wait).
int bad_reply(const ReplyPieces& p, uint64_t l, const uint64_t* off, hipStream_t s, cb_fold_stats* st) {
  if (l >= p.nl) return fail(CB_EHIP, "replies fold: inconsistent bad piece");
  uint64_t at = 0;
  cb::ReplyPiece v{};
  HIP_TRY(hipMemcpyAsync(&at, &p.rec[l].start, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&v, &p.pc[l], sizeof v, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (v.reply >= p.nr) return fail(CB_EHIP, "replies fold: inconsistent bad reply");
  *st = cb_fold_stats{p.nr, 0, 0, 0, 0, 0, 0, 0, 0, v.reply, at - (off[v.reply] - off[0] + v.reply) + off[v.reply]};
  char msg[160];
  std::snprintf(msg, sizeof msg, "reply %u is not UTF-8 (the piece at byte %llu)", v.reply,
                (unsigned long long)st->bad_offset);
  return fail(CB_EUTF8, msg);
}

// No entry but others: the pieces' verdicts read back (and, for replies in
// device memory, the staged bytes), the least other line taken on the host
// (one wait; in everything the reference sends here the others are one short
// line per reply).
int least_other(const ReplyPieces& p, const uint8_t* bytes, const uint64_t* off, const std::vector<uint64_t>& hoff,
                hipStream_t s, cb_fold* f) {
  std::vector<cb::ReplyPiece> pc(p.nl);
  std::vector<cb::LineRec> rec(p.nl);
  std::vector<uint8_t> staged;
  const bool dev_bytes = is_device_ptr(bytes);
  HIP_TRY(hipMemcpyAsync(pc.data(), p.pc, p.nl * sizeof(cb::ReplyPiece), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(rec.data(), p.rec, p.nl * sizeof(cb::LineRec), hipMemcpyDeviceToHost, s));
  if (dev_bytes) {
    staged.resize(p.len);
    HIP_TRY(hipMemcpyAsync(staged.data(), p.data, p.len, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  const uint8_t* best = nullptr;
  for (uint64_t l = 0; l < p.nl; ++l) {
    if (pc[l].kind != cb::kReplyOther) continue;
    const uint32_t r = pc[l].reply;
    if (r >= p.nr || rec[l].start < hoff[r] || rec[l].start + pc[l].len >= hoff[r + 1])
      return fail(CB_EHIP, "replies fold: inconsistent other line");
    const uint64_t at = rec[l].start - hoff[r] + off[r];  // in the caller's bytes
    const uint8_t* q = dev_bytes ? staged.data() + rec[l].start : bytes + at;
    if (!best || cb::bytes_order(q, pc[l].len, best, f->h.other_len) < 0) {
      best = q;
      f->h.other_at = at;
      f->h.other_len = pc[l].len;
    }
  }
  if (!best) return fail(CB_EHIP, "replies fold: others without a line");
  f->h.text.assign(best, best + f->h.other_len);
  return CB_OK;
}

// 3: the entries as the merge's records in (reply, line) order (k_reply_gather
// in the place of compaction's gather, the parsed timestamps in Merge::ts in
// the place of launch_compact_ts), then the merge as it stands: the stable key
// sort and the LWW select, which keeps every winner (nothing is waited for).
int merge_entries(const ReplyPieces& p, uint64_t entries, uint64_t kbytes, TempBlock& tmp, Merge* mg, hipStream_t s) {
  if (int rc = merge_alloc(0, entries, kbytes, cb::MergeOrder::lww, tmp, mg)) return rc;
  if (int rc = enqueue_sort_begin(*mg, s)) return rc;
  HIP_TRY(cb::launch_reply_gather(p.data, p.rec, p.pc, p.nl, p.has_scan, p.len_scan, mg->kb, mg->ko, mg->side, mg->ts,
                                  &mg->dr->dmask[0][0], s));
  if (int rc = enqueue_key_sort(mg->plan, mg->kb, mg->ko, entries, mg->order, mg->sort, mg->dr, s, nullptr, nullptr,
                                nullptr))
    return rc;
  HIP_TRY(cb::launch_compact_select_lww(mg->order, mg->side, mg->ts, mg->kb, mg->ko, entries, false, mg->slen,
                                        mg->tcnt, mg->tbytes, mg->tkeys, s));
  return CB_OK;
}

// 4: the winners' verdicts and lengths (k_fold_size), the two scans that place
// the texts and the rows, their totals read back (one wait), the result's
// blocks sized from them, the response and the rows written (k_fold_write) and
// the wait that makes the result complete.
int write_response(const ReplyPieces& p, const Merge& mg, TempBlock& blk, hipStream_t s, cb_fold* f) {
  const uint64_t n = mg.n;
  cb::Carver c;
  const size_t o_flags = c.take(n), o_inc = c.take(n * 8), o_off = c.take((n + 1) * 8), o_win = c.take(n * 8),
               o_wrow = c.take((n + 1) * 8), o_scan = c.take(cb::scan_tmp_words(n) * 8);
  if (int rc = blk.alloc(c, "device allocation failed for a fold's scratch")) return rc;
  uint8_t* flags = blk.at(o_flags);
  uint64_t *inc = (uint64_t*)blk.at(o_inc), *off = (uint64_t*)blk.at(o_off), *win = (uint64_t*)blk.at(o_win),
           *wrow = (uint64_t*)blk.at(o_wrow), *scan = (uint64_t*)blk.at(o_scan);
  HIP_TRY(cb::launch_fold_size(mg.order, mg.side, mg.slen, n, flags, inc, win, p.cnt, s));
  HIP_TRY(cb::launch_scan_u64(inc, off, n, scan, s));
  HIP_TRY(cb::launch_scan_u64(win, wrow, n, scan, s));
  uint64_t total = 0, keys = 0;
  cb::FoldCounts hc{};
  HIP_TRY(hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&keys, wrow + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&hc, p.cnt, sizeof hc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // (a text and its separator: 3 bytes at least; the vals lie in the replies)
  if (!keys || keys > n || hc.with_text + hc.dead + hc.host != keys || total < 3 * hc.with_text || total > p.len + n ||
      (total != 0) != (hc.with_text != 0))
    return fail(CB_EHIP, "replies fold: inconsistent totals");
  f->st.keys = keys;
  f->st.with_text = hc.with_text;
  f->st.dead = hc.dead;
  f->st.host_rows = hc.host;
  f->st.bytes = total ? total + 1 : 2;
  cb::Carver rc_;
  const size_t o_ka = rc_.take(keys * 8), o_kl = rc_.take(keys * 8), o_ts = rc_.take(keys * 8),
               o_va = rc_.take(keys * 8), o_vl = rc_.take(keys * 8), o_rp = rc_.take(keys * 4), o_fl = rc_.take(keys);
  if (int rc = pool_alloc_or(f->device, rc_.total(), &f->block, &f->block_cap,
                             "device allocation failed for a fold's rows"))
    return rc;
  uint8_t* b = (uint8_t*)f->block;
  f->rows = cb::FoldRows{(uint64_t*)(b + o_ka), (uint64_t*)(b + o_kl), (uint64_t*)(b + o_ts), (uint64_t*)(b + o_va),
                         (uint64_t*)(b + o_vl), (uint32_t*)(b + o_rp), b + o_fl};
  if (int rc = pool_alloc_or(f->device, total + 2, &f->text_block, &f->text_cap,
                             "device allocation failed for a fold's text"))
    return rc;
  f->text = (uint8_t*)f->text_block;
  HIP_TRY(cb::launch_fold_write(mg.order, mg.side, mg.ts, flags, inc, off, win, wrow, n, p.data, p.soff, p.coff, p.nr,
                                f->rows, f->text, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

int fold_on_device(const uint8_t* bytes, const uint64_t* off, uint32_t nr, int device, hipStream_t s, cb_fold* f,
                   cb_fold_stats* st) {
  if (int rc = cb_init(device)) return rc;
  DeviceGuard dg(device);
  (void)workspace(device, s);  // (registers s: the pool retires blocks behind it)
  f->device = device;
  // the replies' offsets in the staged buffer, then in the caller's bytes
  std::vector<uint64_t> hoff(2 * (nr + 1ull));
  for (uint32_t r = 0; r <= nr; ++r) {
    hoff[r] = off[r] - off[0] + r;
    hoff[nr + 1 + r] = off[r];
  }
  TempBlock staged{device}, pieces{device}, tmp{device}, sizes{device};
  ReplyPieces p;
  uint64_t* base = nullptr;
  if (int rc = stage_replies(bytes, off, nr, hoff, staged, &p, &base, s)) {
    (void)hipStreamSynchronize(s);  // (hoff is pageable: no return before the stream has read it)
    return rc;
  }
  if (!p.nl) return CB_OK;
  cb::FoldCounts hc{};
  uint64_t e[2] = {0, 0};
  if (int rc = mark_replies(&p, base, pieces, s, &hc, e)) return rc;
  if (hc.bad != ~0ull) return bad_reply(p, hc.bad, off, s, st);
  f->st.lines = hc.lines;
  f->st.entries = e[0];
  f->st.others = hc.others;
  if (!e[0]) {
    if (!hc.others) return CB_OK;
    if (int rc = least_other(p, bytes, off, hoff, s, f)) return rc;
    f->st.bytes = f->h.text.size();
    return CB_OK;
  }
  Merge mg;
  if (int rc = merge_entries(p, e[0], e[1], tmp, &mg, s)) return rc;
  return write_response(p, mg, sizes, s, f);
}

// Bytes of a result into an output that may be host or device memory.
int copy_out(const cb_fold* f, void* dst, const void* host_src, const void* dev_src, size_t n) {
  if (!dst || !n) return CB_OK;
  if (f->device < 0 || !dev_src) return put_bytes((uint8_t*)dst, host_src, n);
  HIP_TRY(hipMemcpy(dst, dev_src, n, hipMemcpyDefault));
  return CB_OK;
}

}  // namespace

extern "C" {

// Every temporary is carved from pool blocks released stream-ordered on return
// (error returns included). The call waits for its own stream for the pieces'
// count, for the entries' counts and the first bad piece, for the winners'
// totals and at the end (the result is complete when the call returns).
int cb_replies_fold(const uint8_t* bytes, const uint64_t* off, uint32_t nr, int device, void* stream, void** out,
                    void* stats_out) {
  cb_fold_stats* stats = static_cast<cb_fold_stats*>(stats_out);
  cb_fold_stats st{nr, 0, 0, 0, 0, 0, 0, 0, 0, ~0ull, ~0ull};
  if (stats) *stats = st;
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  if (nr > cb::kFoldMaxReplies) return fail(CB_EINVAL, "too many replies (at most 4096)");
  if (nr && !off) return fail(CB_EINVAL, "null offsets with a non-zero count");
  for (uint32_t r = 0; r < nr; ++r)
    if (off[r + 1] < off[r]) return fail(CB_EINVAL, "reply offsets decrease");
  const uint64_t total = nr ? off[nr] - off[0] : 0;
  if (total && !bytes) return fail(CB_EINVAL, "null replies with a non-zero total");
  if (device < -1) return fail(CB_EINVAL, "a device below -1");
  std::unique_ptr<cb_fold, int (*)(void*)> f(new cb_fold(), cb_fold_destroy);
  f->st = st;
  f->st.bytes = 2;
  f->h.text = {'[', ']'};
  if (total && device == -1) {
    const char* why = "";
    const int rc = cb::fold_host(bytes, off, nr, &f->h, &why);
    stats_of(f->h, &st);
    if (rc == cb::kReplyBadUtf8) {
      if (stats) *stats = st;
      char msg[160];
      std::snprintf(msg, sizeof msg, "reply %llu is not UTF-8 (the piece at byte %llu)",
                    (unsigned long long)st.bad_reply, (unsigned long long)st.bad_offset);
      return fail(CB_EUTF8, msg);
    }
    if (rc) return fail(CB_EINVAL, why);
    f->st = st;
  } else if (total) {
    const int rc = fold_on_device(bytes, off, nr, device, (hipStream_t)stream, f.get(), &st);
    if (rc) {
      if (rc == CB_EUTF8 && stats) *stats = st;
      return rc;
    }
  }
  if (stats) *stats = f->st;
  *out = f.release();
  return CB_OK;
}

int cb_fold_info(const void* fold, void* stats) {
  const cb_fold* f = (const cb_fold*)fold;
  if (!f || !stats) return fail(CB_EINVAL, "null argument");
  *static_cast<cb_fold_stats*>(stats) = f->st;
  return CB_OK;
}

int cb_fold_text(const void* fold, uint8_t* text) {
  const cb_fold* f = (const cb_fold*)fold;
  if (!f) return fail(CB_EINVAL, "null fold");
  if (f->device >= 0) {
    DeviceGuard dg(f->device);
    return copy_out(f, text, f->h.text.data(), f->text, f->st.bytes);
  }
  return copy_out(f, text, f->h.text.data(), nullptr, f->st.bytes);
}

int cb_fold_rows(const void* fold, uint64_t* key_at, uint64_t* key_len, uint64_t* ts, uint64_t* val_at,
                 uint64_t* val_len, uint32_t* reply, uint8_t* flags) {
  const cb_fold* f = (const cb_fold*)fold;
  if (!f) return fail(CB_EINVAL, "null fold");
  const uint64_t n = f->st.keys;
  if (!n) return CB_OK;
  const cb::HostFold& h = f->h;
  const cb::FoldRows& d = f->rows;
  std::unique_ptr<DeviceGuard> dg(f->device >= 0 ? new DeviceGuard(f->device) : nullptr);
  if (int rc = copy_out(f, key_at, h.key_at.data(), d.key_at, n * 8)) return rc;
  if (int rc = copy_out(f, key_len, h.key_len.data(), d.key_len, n * 8)) return rc;
  if (int rc = copy_out(f, ts, h.ts.data(), d.ts, n * 8)) return rc;
  if (int rc = copy_out(f, val_at, h.val_at.data(), d.val_at, n * 8)) return rc;
  if (int rc = copy_out(f, val_len, h.val_len.data(), d.val_len, n * 8)) return rc;
  if (int rc = copy_out(f, reply, h.reply.data(), d.reply, n * 4)) return rc;
  return copy_out(f, flags, h.flags.data(), d.flags, n);
}

int cb_fold_other(const void* fold, uint64_t* at, uint64_t* len) {
  const cb_fold* f = (const cb_fold*)fold;
  if (!f) return fail(CB_EINVAL, "null fold");
  if (at) *at = f->h.other_at;
  if (len) *len = f->h.other_len;
  return CB_OK;
}

int cb_fold_destroy(void* fold) {
  cb_fold* f = (cb_fold*)fold;
  if (!f) return CB_OK;
  if (f->device >= 0) {
    pool_release(f->device, f->block, f->block_cap);
    pool_release(f->device, f->text_block, f->text_cap);
  }
  delete f;
  return CB_OK;
}

int cb_reply_line(const uint8_t* piece, uint64_t len, int terminated, int* kind, uint64_t* key_len, uint64_t* ts,
                  uint64_t* val_at, uint64_t* val_len, uint8_t* val_flags) {
  if (!kind || (!piece && len)) return fail(CB_EINVAL, "null argument");
  for (uint64_t i = 0; i < len; ++i)
    if (piece[i] == '\n') return fail(CB_EINVAL, "a piece holds no newline: a reply is split on them");
  const cb::ReplyLine v = cb::reply_line(piece, len, terminated != 0);
  const bool entry = v.kind == cb::kReplyEntry;
  const uint64_t va = entry ? v.tab2 + 1 : 0, vl = entry ? v.len - va : 0;
  *kind = v.kind;
  if (key_len) *key_len = entry ? v.tab1 : 0;
  if (ts) *ts = entry ? v.ts : 0;
  if (val_at) *val_at = va;
  if (val_len) *val_len = vl;
  if (val_flags) *val_flags = entry ? cb::reply_val_flags(piece + va, vl) : 0;
  return CB_OK;
}

}  // extern "C"
