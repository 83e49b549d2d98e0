// capi_filter.cpp — the filter half of the extern "C" boundary
// (include/cassbloom.h) over the gfx950 kernels: filter handles in HBM with
// their lazy clear, write marks and host mirror, path selection, the batched
// insert and probe, import / export, and the device halves of the BloomProto /
// TableMeta (prost) codec, whose host half is codec.cpp.
//
// Reference: src/bloom.rs (BloomFilter / BloomProto) and its
// callers src/sstable.rs:59-65,96-119,138 and src/lib.rs:129-134.
#include "capi_internal.hpp"
#include "codec.hpp"

using namespace cbx;

namespace {

int g_path_override = 0;  // 0 auto, 1 direct, 2 tiled

constexpr int PATH_DIRECT = 1, PATH_TILED = 2;

uint64_t alloc_words_for(uint64_t m) {
  // Pad to whole tiles of kTileAlignBits (the largest LDS tile, the build's)
  // so tiled passes never read or write past the allocation; small filters
  // pad to one tile of kSmallAlignBits (the smallest probe tile).
  const uint64_t align = m >= cb::kSmallAlignBits ? cb::kTileAlignBits : cb::kSmallAlignBits;
  const uint64_t bits = std::max<uint64_t>((m + align - 1) / align * align, align);
  return bits / 32;
}

hipError_t ensure_pad_zeroed(const cb_filter* cf, hipStream_t s) {
  cb_filter* f = const_cast<cb_filter*>(cf);
  const uint64_t nw = (f->m + 31) / 32;
  if (f->needs_pad_zero.exchange(false) && f->nwords_alloc > nw)
    return hipMemsetAsync(f->words + nw, 0, (f->nwords_alloc - nw) * 4, s);
  return hipSuccess;
}

// Readies f's words for a tiled build on s. A fresh filter's build writes
// every tile of [0, T * 2^tb): a pending clear is moot there, and only the
// padding past them (tiles past ceil(m/32) may not all be rewritten) is
// zeroed; any other filter gets its pending clear.
hipError_t ready_for_tiled_build(cb_filter* f, hipStream_t s) {
  if (!f->known_zero) return cbx::ensure_zeroed(f, s);
  if (f->needs_zero.exchange(false)) f->needs_pad_zero.store(true);
  return ensure_pad_zeroed(f, s);
}

// A new write mark (recorded with the system-scope release: the mirror's
// refresh copies right after waiting on it).
hipError_t make_mark(std::shared_ptr<WriteMark>* out) {
  auto m = std::make_shared<WriteMark>();
  const hipError_t e = hipEventCreateWithFlags(&m->ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  *out = std::move(m);
  return hipSuccess;
}

// Record f's write mark on s: its own mark again when no one else holds it
// (no batch shares it, no mirror refresh is waiting on it), else a new one.
// With the mirror off nothing is recorded (an event per write cost the C2
// one-lane build 1 us of device time, round 6): the write is only flagged,
// and the refresh that meets the flag waits for every stream the library
// knows (wait_known_streams), never for a stored stream handle.
hipError_t record_own_mark(cb_filter* f, hipStream_t s) {
  if (!mirror_on(f)) {
    f->unmarked.store(true, std::memory_order_release);
    return hipSuccess;
  }
  std::shared_ptr<WriteMark> m = std::atomic_load(&f->wmark);
  if (!m || m.use_count() > 2) {  // (2: f's reference and this copy)
    const hipError_t e = make_mark(&m);
    if (e != hipSuccess) return e;
  }
  const hipError_t e = hipEventRecord(m->ev, s);
  if (e == hipSuccess) std::atomic_store(&f->wmark, m);
  return e;
}

// Every tiled pass reads/writes whole tiles [0, T * 2^tb): refuse to launch
// one the allocation does not cover (a safety net over alloc_words_for).
bool covers(const cb_filter* f, const TilePlan& p) {
  return cb::plan_ok(p) && ((uint64_t)p.T << p.tb) <= f->nwords_alloc * 32;
}

// Largest m a tiled pass covers: kMaxTiles tiles of the largest tile size.
bool build_tiled_ok(uint64_t m) { return m >= 1 && m <= (uint64_t)cb::kMaxTiles << cb::kMaxTileBits; }
bool probe_tiled_ok(uint64_t m) {
  return m >= 1 && m <= (uint64_t)cb::kMaxTiles << cb::kMaxProbeTileBits;
}

int choose_build_path(uint64_t m, uint64_t n) {
  if (g_path_override == PATH_DIRECT || !build_tiled_ok(m)) return PATH_DIRECT;
  if (g_path_override == PATH_TILED) return PATH_TILED;
  return (m >= (1ull << 20) && n >= (1ull << 15)) ? PATH_TILED : PATH_DIRECT;
}

int choose_probe_path(uint64_t m, uint64_t n, uint32_t nf) {
  if (g_path_override == PATH_DIRECT || !probe_tiled_ok(m)) return PATH_DIRECT;
  if (g_path_override == PATH_TILED) return PATH_TILED;
  (void)nf;
  return (m >= (1ull << 20) && n >= (1ull << 16)) ? PATH_TILED : PATH_DIRECT;
}

}  // namespace

namespace cbx {

// The pending lazy clear, issued on s by whichever operation needs the words
// first (readers may race: zero_mu makes the exchange, the memset and the
// event that orders the host mirror's refresh after it one step).
hipError_t ensure_zeroed(const cb_filter* cf, hipStream_t s) {
  cb_filter* f = const_cast<cb_filter*>(cf);
  note_stream(f->device, s);  // (pool_release retires the words behind every stream that touched them)
  if (!f->needs_zero.load()) return hipSuccess;
  std::lock_guard<std::mutex> lk(f->zero_mu);
  if (f->needs_zero.exchange(false)) {
    f->needs_pad_zero.store(false);
    hipError_t e = hipMemsetAsync(f->words, 0, f->nwords_alloc * 4, s);
    if (e == hipSuccess) e = record_own_mark(f, s);
    return e;
  }
  return hipSuccess;
}

// insert_impl with the stream's workspace already locked by the caller.
int insert_locked(Workspace& ws, cb_filter* f, const uint8_t* keys, const uint64_t* offsets,
                  uint32_t key_len, uint64_t n, hipStream_t s) {
  StagedKeys sk;
  if (int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk)) return rc;

  const int path = choose_build_path(f->m, n);
  g_last_path = path;
  if (path == PATH_DIRECT && f->m <= cb::kInsertLdsMaxBits) {
    // small filters (the product's m = 1024): the batch ORed in LDS; a fresh
    // filter built by one block is written whole, without a fill first
    const bool store_all = f->known_zero && n <= cb::kInsertLdsOneBlock;
    if (store_all) {
      std::lock_guard<std::mutex> lk(f->zero_mu);
      f->needs_zero.store(false);
      f->needs_pad_zero.store(false);
    } else {
      HIP_TRY(ensure_zeroed(f, s));
    }
    HIP_TRY(cb::launch_insert_lds(sk.keyk, f->mode, f->words, f->m, f->nwords_alloc, sk.ks, n, f->mp, store_all, s));
  } else if (path == PATH_DIRECT) {
    HIP_TRY(ensure_zeroed(f, s));
    HIP_TRY(cb::launch_insert_direct(sk.keyk, f->mode, f->words, sk.ks, n, f->mp, s));
  } else {
    HIP_TRY(ready_for_tiled_build(f, s));
    const uint64_t chunk = cb::build_chunk_keys();
    for (uint64_t k0 = 0; k0 < n; k0 += chunk) {
      const uint64_t nk = std::min(chunk, n - k0);
      const TilePlan p = cb::plan_build(f->m, nk);
      if (!covers(f, p)) return fail(CB_EINVAL, "internal: build tile plan exceeds the filter allocation");
      HIP_TRY(ws.seg.reserve(cb::build_seg_bytes(p), s));
      HIP_TRY(ws.ent.reserve(cb::build_ent_bytes(p), s));
      HIP_TRY(cb::launch_build_tiled(sk.keyk, f->mode, f->words, f->known_zero, slice_keys(sk, k0), nk, f->mp, p,
                                     (uint32_t*)ws.seg.p, (uint32_t*)ws.ent.p, s));
      f->known_zero = false;
    }
  }
  f->known_zero = false;
  int mrc = mark_written(f, s);
  if (mrc) return mrc;
  if (sk.staged) HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

int mark_written(cb_filter* f, hipStream_t s) {
  HIP_TRY(record_own_mark(f, s));
  f->gen.fetch_add(1, std::memory_order_acq_rel);
  return CB_OK;
}

int mark_written_many(Workspace& ws, cb_filter* const* fs, uint32_t nf, hipStream_t s) {
  if (!nf) return CB_OK;
  bool any_on = false;
  for (uint32_t i = 0; i < nf; ++i) any_on |= mirror_on(fs[i]);
  if (!any_on) {  // no mirror to order: flagged only (see record_own_mark)
    for (uint32_t i = 0; i < nf; ++i) {
      fs[i]->unmarked.store(true, std::memory_order_release);
      fs[i]->gen.fetch_add(1, std::memory_order_acq_rel);
    }
    return CB_OK;
  }
  std::shared_ptr<WriteMark> m;
  for (auto& c : ws.marks)
    if (c.use_count() == 1) {  // only the pool holds it: no filter, no waiting refresh
      m = c;
      break;
    }
  if (!m) {
    HIP_TRY(make_mark(&m));
    ws.marks.push_back(m);
  }
  HIP_TRY(hipEventRecord(m->ev, s));
  for (uint32_t i = 0; i < nf; ++i) {
    std::atomic_store(&fs[i]->wmark, m);
    fs[i]->gen.fetch_add(1, std::memory_order_acq_rel);
  }
  return CB_OK;
}

}  // namespace cbx

namespace {

int insert_impl(cb_filter* f, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len,
                uint64_t n, hipStream_t s) {
  if (!f) return fail(CB_EINVAL, "null filter");
  if (n == 0) return CB_OK;  // no hashes() call in the reference: no panic
  if (f->m == 0) return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  DeviceGuard dg(f->device);
  Workspace& ws = workspace(f->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  return insert_locked(ws, f, keys, offsets, key_len, n, s);  // (its staging refuses null keys)
}

int probe_impl(const cb_filter* const* filters, uint32_t nf, const uint8_t* keys,
               const uint64_t* offsets, uint32_t key_len, uint64_t n, uint64_t* hits,
               hipStream_t s) {
  if (nf == 0 || n == 0) return CB_OK;
  if (!filters || !hits) return fail(CB_EINVAL, "null filters or hits");
  for (uint32_t i = 0; i < nf; ++i) {
    if (!filters[i]) return fail(CB_EINVAL, "null filter");
    if (filters[i]->device != filters[0]->device)
      return fail(CB_EINVAL, "all filters of one probe must live on one device");
    if (filters[i]->m == 0)
      return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  }
  for (uint32_t i = 0; i < nf; ++i) HIP_TRY(ensure_zeroed(filters[i], s));
  const int dev = filters[0]->device;
  DeviceGuard dg(dev);
  Workspace& ws = workspace(dev, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk);
  if (rc) return rc;

  const uint64_t hwords = (n + 63) / 64;
  uint64_t* dhits;
  if ((rc = out_buf(ws.hits, hits, (size_t)nf * hwords, s, &dhits))) return rc;

  // Group filters by m (positions depend only on m), preserving hit rows.
  std::map<uint64_t, std::vector<uint32_t>> groups;
  for (uint32_t i = 0; i < nf; ++i) groups[filters[i]->m].push_back(i);

  int last_path = PATH_DIRECT;
  for (auto& kv : groups) {
    const uint64_t m = kv.first;
    const std::vector<uint32_t>& idx = kv.second;
    const cb_filter* f0 = filters[idx[0]];
    const int path = choose_probe_path(m, n, (uint32_t)idx.size());
    last_path = path;
    // the filters and hit rows of the launch that starts at idx[g0] (kMaxFiltersPerLaunch to a launch)
    auto launch_filters = [&](size_t g0, FilterPtrs& fp) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(cb::kMaxFiltersPerLaunch, idx.size() - g0);
      for (uint32_t j = 0; j < cnt; ++j) {
        fp.w[j] = filters[idx[g0 + j]]->words;
        fp.row[j] = idx[g0 + j];
      }
      return cnt;
    };
    if (path == PATH_DIRECT) {
      for (size_t g0 = 0; g0 < idx.size(); g0 += cb::kMaxFiltersPerLaunch) {
        FilterPtrs fp{};
        const uint32_t cnt = launch_filters(g0, fp);
        HIP_TRY(cb::launch_probe_direct(sk.keyk, f0->mode, fp, cnt, sk.ks, n, f0->mp, dhits, hwords, s));
      }
    } else {
      const uint64_t chunk = cb::probe_chunk_keys();  // keys per partition pass (multiple of 64)
      for (uint64_t k0 = 0; k0 < n; k0 += chunk) {
        const uint64_t nk = std::min(chunk, n - k0);
        const TilePlan p = cb::plan_probe(m, nk);
        for (uint32_t i : idx)
          if (!covers(filters[i], p))
            return fail(CB_EINVAL, "internal: probe tile plan exceeds the filter allocation");
        HIP_TRY(ws.seg.reserve(cb::probe_seg_bytes(p), s));
        HIP_TRY(ws.ent.reserve(cb::probe_ent_bytes(p), s));
        HIP_TRY(ws.masks.reserve((size_t)2 * nk * 4, s));
        HIP_TRY(ws.lkey.reserve(cb::probe_lkey_bytes(p), s));
        HIP_TRY(cb::launch_probe_partition(sk.keyk, f0->mode, slice_keys(sk, k0), nk, f0->mp, p,
                                           (uint32_t*)ws.seg.p, (uint2*)ws.ent.p, (uint16_t*)ws.lkey.p, s));
        for (size_t g0 = 0; g0 < idx.size(); g0 += cb::kMaxFiltersPerLaunch) {
          FilterPtrs fp{};
          const uint32_t cnt = launch_filters(g0, fp);
          HIP_TRY(cb::launch_probe_tiles(fp, cnt, nk, p, (const uint32_t*)ws.seg.p,
                                         (const uint2*)ws.ent.p, (const uint16_t*)ws.lkey.p,
                                         (uint32_t*)ws.masks.p, dhits + k0 / 64, hwords, s));
        }
      }
    }
  }
  g_last_path = last_path;
  return finish_out(hits, dhits, (size_t)nf * hwords * 8, sk.staged, s);
}

// Refresh the host mirror if a write happened since it was taken: wait for
// the last write's event (on its own stream: no device-wide sync), then copy
// the words back once. Readers race only on the flag (acquire/release).
//
// A write made while the mirror was off recorded nothing (record_own_mark):
// the refresh that meets it waits for every stream the library has enqueued
// on for the device (wait_known_streams), by events, so a destroyed stream's
// handle never matters and streams the library never saw (the
// caller's other work) are not waited for.
int refresh_mirror(const cb_filter* cf) {
  cb_filter* f = const_cast<cb_filter*>(cf);
  const uint64_t g = f->gen.load(std::memory_order_acquire);
  if (f->host_gen.load(std::memory_order_acquire) == g) return CB_OK;
  std::lock_guard<std::mutex> lk(f->host_mu);
  const uint64_t g2 = f->gen.load(std::memory_order_acquire);
  if (f->host_gen.load(std::memory_order_acquire) == g2) return CB_OK;
  const uint64_t nw = (f->m + 31) / 32;
  f->host.resize(nw);
  {
    std::lock_guard<std::mutex> zl(f->zero_mu);  // a racing reader's lazy clear is issued and recorded, or not yet
    if (f->needs_zero.load()) {  // cleared, nothing on the device yet: all zero
      std::fill(f->host.begin(), f->host.end(), 0u);
    } else {
      DeviceGuard dg(f->device);
      // the last write's mark (every write to one filter is ordered by its
      // exclusive writer, so it covers them all): an event, not a stream, so
      // a stream destroyed since, or its handle reused, changes nothing
      if (f->unmarked.exchange(false, std::memory_order_acq_rel)) {
        int rc = wait_known_streams(f->device);
        if (rc) return rc;
      }
      const std::shared_ptr<WriteMark> m = std::atomic_load(&f->wmark);
      if (m) HIP_TRY(hipEventSynchronize(m->ev));
      HIP_TRY(hipMemcpy(f->host.data(), f->words, nw * 4, hipMemcpyDeviceToHost));
    }
  }
  f->host_gen.store(g2, std::memory_order_release);
  return CB_OK;
}

// BloomFilter::hashes + may_contain (src/bloom.rs:26-37,48-51) on the mirror:
// u64 wrapping x33 / x31 folds, h % m, and bit b read only when bit a is set.
int mirror_contains(const cb_filter* f, const uint8_t* key, uint64_t len) {
  uint64_t h1 = 5381, h2 = 0;
  for (uint64_t i = 0; i < len; ++i) {
    h1 = (h1 << 5) + h1 + key[i];
    h2 = h2 * 31 + key[i];
  }
  const uint64_t a = h1 % f->m, b = h2 % f->m;
  const uint32_t* w = f->host.data();
  return ((w[a >> 5] >> (a & 31)) & 1u) && ((w[b >> 5] >> (b & 31)) & 1u);
}

// The device half of a decode: a new filter holding the m 0/1 bytes at bits.
int filter_from_bits(const uint8_t* bits, uint64_t m, int device, cb_filter** out) {
  cb_filter* f = nullptr;
  int rc = cb_filter_create(m, device, &f);
  if (rc) return rc;
  if (m) {
    rc = cb_filter_import_bools(f, bits, m, nullptr);
    if (rc) {
      cb_filter_destroy(f);
      return rc;
    }
  }
  *out = f;
  return CB_OK;
}

}  // namespace

extern "C" {

int cb_set_path(int path) {
  if (path < 0 || path > 2) return fail(CB_EINVAL, "path must be 0, 1 or 2");
  g_path_override = path;
  return CB_OK;
}
int cb_last_path(void) { return g_last_path; }

int cb_filter_create(uint64_t m_bits, int device, cb_filter** out) {
  if (!out) return fail(CB_EINVAL, "null out");
  *out = nullptr;
  int rc = cb_init(device);
  if (rc) return rc;
  DeviceGuard dg(device);
  std::unique_ptr<cb_filter> f(new cb_filter());
  f->m = m_bits;
  f->device = device;
  f->nwords_alloc = alloc_words_for(m_bits);
  if (m_bits) f->mp = cb::make_modp(m_bits, &f->mode);
  if (pool_alloc(device, f->nwords_alloc * 4, (void**)&f->words, &f->words_cap) != hipSuccess)
    return fail(CB_ENOMEM, "device allocation failed for filter words");
  // zero-filled lazily by the first operation that reads the words; a fresh
  // tiled build writes every tile and skips the fill (see ensure_zeroed)
  f->needs_zero.store(true);
  f->known_zero = true;
  *out = f.release();
  return CB_OK;
}

int cb_filter_destroy(cb_filter* f) {
  if (!f) return CB_OK;
  {
    DeviceGuard dg(f->device);
    pool_release(f->device, f->words, f->words_cap);
    std::atomic_store(&f->wmark, std::shared_ptr<WriteMark>());
  }
  delete f;
  return CB_OK;
}

int cb_filter_bits(const cb_filter* f, uint64_t* m_out) {
  if (!f || !m_out) return fail(CB_EINVAL, "null argument");
  *m_out = f->m;
  return CB_OK;
}

int cb_filter_device(const cb_filter* f, int* device_out) {
  if (!f || !device_out) return fail(CB_EINVAL, "null argument");
  *device_out = f->device;
  return CB_OK;
}

int cb_filter_words(const cb_filter* f, const uint32_t** words_out, uint64_t* nwords_out) {
  if (!f || !words_out || !nwords_out) return fail(CB_EINVAL, "null argument");
  if (f->needs_zero.load()) {
    DeviceGuard dg(f->device);
    HIP_TRY(ensure_zeroed(f, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  *words_out = f->words;
  *nwords_out = f->nwords_alloc;
  return CB_OK;
}

int cb_filter_clear(cb_filter* f, void* stream) {
  if (!f) return fail(CB_EINVAL, "null filter");
  (void)stream;
  f->known_zero = true;
  f->needs_zero.store(true);
  f->gen.fetch_add(1, std::memory_order_acq_rel);  // the mirror refresh sees needs_zero: all-zero words
  return CB_OK;
}

int cb_filter_host_mirror(cb_filter* f, int mode) {
  if (!f) return fail(CB_EINVAL, "null filter");
  if (mode < -1 || mode > 1) return fail(CB_EINVAL, "mode must be -1 (auto), 0 (off) or 1 (on)");
  f->mirror.store(mode, std::memory_order_relaxed);
  return CB_OK;
}

int cb_filter_host_mirror_info(const cb_filter* f, int* on, int* current) {
  if (!f) return fail(CB_EINVAL, "null filter");
  if (on) *on = mirror_on(f);
  if (current)
    *current = f->host_gen.load(std::memory_order_acquire) == f->gen.load(std::memory_order_acquire);
  return CB_OK;
}

int cb_filter_insert_fixed(cb_filter* f, const uint8_t* keys, uint32_t key_len, uint64_t n,
                           void* stream) {
  return insert_impl(f, keys, nullptr, key_len, n, (hipStream_t)stream);
}

int cb_filter_insert_var(cb_filter* f, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                         void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return insert_impl(f, bytes, offsets, 0, n, (hipStream_t)stream);
}

int cb_probe_fixed(const cb_filter* const* filters, uint32_t nf, const uint8_t* keys,
                   uint32_t key_len, uint64_t n, uint64_t* hits, void* stream) {
  return probe_impl(filters, nf, keys, nullptr, key_len, n, hits, (hipStream_t)stream);
}

int cb_probe_var(const cb_filter* const* filters, uint32_t nf, const uint8_t* bytes,
                 const uint64_t* offsets, uint64_t n, uint64_t* hits, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return probe_impl(filters, nf, bytes, offsets, 0, n, hits, (hipStream_t)stream);
}

int cb_may_contain(const cb_filter* f, const uint8_t* key, uint64_t len, int* out) {
  if (!f || !out || (!key && len)) return fail(CB_EINVAL, "null argument");
  if (f->m == 0) return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  if (mirror_on(f)) {
    int rc = refresh_mirror(f);
    if (rc) return rc;
    *out = mirror_contains(f, key, len);
    g_last_path = 5;
    return CB_OK;
  }
  uint64_t offs[2] = {0, len};
  uint64_t hit = 0;
  const cb_filter* fs[1] = {f};
  int rc = probe_impl(fs, 1, key ? key : (const uint8_t*)"", offs, 0, 1, &hit, nullptr);
  if (rc) return rc;
  *out = (int)(hit & 1);
  return CB_OK;
}

int cb_filter_export_bools(const cb_filter* f, uint8_t* out, void* stream) {
  if (!f) return fail(CB_EINVAL, "null filter");
  if (f->m == 0) return CB_OK;
  if (!out) return fail(CB_EINVAL, "null out");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(f->device);
  note_stream(f->device, s);
  HIP_TRY(ensure_zeroed(f, s));
  if (is_device_ptr(out)) {
    HIP_TRY(cb::launch_export_bools(f->words, f->m, out, s));
    return CB_OK;
  }
  Workspace& ws = workspace(f->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  HIP_TRY(ws.bools.reserve(f->m, s));
  HIP_TRY(cb::launch_export_bools(f->words, f->m, (uint8_t*)ws.bools.p, s));
  HIP_TRY(hipMemcpyAsync(out, ws.bools.p, f->m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

int cb_filter_import_bools(cb_filter* f, const uint8_t* in, uint64_t m, void* stream) {
  if (!f) return fail(CB_EINVAL, "null filter");
  if (m != f->m) return fail(CB_EINVAL, "bool array length differs from the filter's m");
  if (m == 0) return CB_OK;
  if (!in) return fail(CB_EINVAL, "null input");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(f->device);
  note_stream(f->device, s);
  if (is_device_ptr(in)) {
    HIP_TRY(cb::launch_import_bools(f->words, m, in, s));
  } else {
    Workspace& ws = workspace(f->device, s);
    std::lock_guard<std::mutex> lk(ws.mu);
    HIP_TRY(ws.bools.reserve(m, s));
    HIP_TRY(hipMemcpyAsync(ws.bools.p, in, m, hipMemcpyHostToDevice, s));
    HIP_TRY(cb::launch_import_bools(f->words, m, (const uint8_t*)ws.bools.p, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (f->needs_zero.exchange(false)) f->needs_pad_zero.store(true);
  HIP_TRY(ensure_pad_zeroed(f, s));  // every word < ceil(m/32) was rewritten
  f->known_zero = false;
  return mark_written(f, s);
}

int cb_filter_export_packed(const cb_filter* f, uint32_t* out, void* stream) {
  if (!f) return fail(CB_EINVAL, "null filter");
  const uint64_t nw = (f->m + 31) / 32;
  if (!nw) return CB_OK;
  if (!out) return fail(CB_EINVAL, "null out");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(f->device);
  note_stream(f->device, s);
  HIP_TRY(ensure_zeroed(f, s));
  const bool dev = is_device_ptr(out);
  HIP_TRY(hipMemcpyAsync(out, f->words, nw * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                         s));
  if (!dev) HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

int cb_filter_import_packed(cb_filter* f, const uint32_t* in, uint64_t nwords, void* stream) {
  if (!f) return fail(CB_EINVAL, "null filter");
  const uint64_t nw = (f->m + 31) / 32;
  if (nwords != nw) return fail(CB_EINVAL, "word count differs from ceil(m/32)");
  if (!nw) return CB_OK;
  if (!in) return fail(CB_EINVAL, "null input");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(f->device);
  note_stream(f->device, s);
  const bool dev = is_device_ptr(in);
  HIP_TRY(hipMemcpyAsync(f->words, in, nw * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         s));
  HIP_TRY(cb::launch_mask_tail(f->words, f->m, s));
  if (f->needs_zero.exchange(false)) f->needs_pad_zero.store(true);
  HIP_TRY(ensure_pad_zeroed(f, s));
  if (!dev) HIP_TRY(hipStreamSynchronize(s));
  f->known_zero = false;
  return mark_written(f, s);
}

// ---- the prost codec's device halves (host side: codec.cpp) ----

int cb_filter_to_bytes(const cb_filter* f, uint8_t* out, uint64_t cap, uint64_t* len_out) {
  if (!f || !len_out) return fail(CB_EINVAL, "null argument");
  // prost: proto3 repeated scalars are packed; an empty field is omitted.
  const uint64_t total = codec::bloom_len(f->m);
  *len_out = total;
  if (!out || cap < total || !total) return CB_OK;
  uint8_t hdr[11];
  const size_t hl = codec::put_bloom_header(hdr, f->m);
  int rc = put_bytes(out, hdr, hl);
  if (rc) return rc;
  return cb_filter_export_bools(f, out + hl, nullptr);
}

int cb_filter_from_bytes(const uint8_t* in, uint64_t len, int device, cb_filter** out) {
  if (!out || (!in && len)) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  codec::BloomBits b;
  std::string err;
  if (int rc = codec::parse_bloom(in, len, b, err)) return fail(rc, err.c_str());
  return filter_from_bits(b.src, b.m, device, out);
}

// ---- TableMeta, the SSTable `.meta` file (src/sstable.rs:31-37) ----

int cb_meta_encode(const cb_filter* bloom, const cb_zone_bounds* zone, uint8_t* out, uint64_t cap,
                   uint64_t* len_out) {
  if (!len_out) return fail(CB_EINVAL, "null len_out");
  if (zone && ((zone->has_min && zone->min_len && !zone->min) ||
               (zone->has_max && zone->max_len && !zone->max)))
    return fail(CB_EINVAL, "null zone bound");
  if (zone && ((zone->has_min && !codec::utf8_ok(zone->min, zone->min_len)) ||
               (zone->has_max && !codec::utf8_ok(zone->max, zone->max_len))))
    return fail(CB_EINVAL, "zone bound is not UTF-8 (ZoneMapProto strings are Rust Strings)");
  codec::MetaFrame fr;
  codec::meta_frame(bloom != nullptr, bloom ? bloom->m : 0, zone, fr);
  *len_out = fr.total;
  if (!out || cap < fr.total) return CB_OK;
  int rc;
  if ((rc = put_bytes(out, fr.head, fr.head_len))) return rc;
  uint64_t pos = fr.head_len;
  if (bloom && bloom->m) {
    if ((rc = cb_filter_export_bools(bloom, out + pos, nullptr))) return rc;
    pos += bloom->m;
  }
  return put_bytes(out + pos, fr.zone.data(), fr.zone.size());
}

int cb_meta_decode(const uint8_t* in, uint64_t len, int device, cb_filter** bloom_out,
                   cb_meta_info* info) {
  if (!bloom_out || !info || (!in && len)) return fail(CB_EINVAL, "null argument");
  *bloom_out = nullptr;
  memset(info, 0, sizeof(*info));
  codec::MetaParse mp;
  std::string err;
  int rc = codec::parse_meta(in, len, mp, err);
  if (rc) return fail(rc, err.c_str());
  const codec::MetaScan& ms = mp.scan;
  cb_filter* f = nullptr;
  // SsTable::load: meta.bloom.map(from_proto).unwrap_or_else(|| BloomFilter::new(1024))
  rc = mp.has_bloom() ? filter_from_bits(mp.bloom.src, mp.bloom.m, device, &f) : cb_filter_create(1024, device, &f);
  if (rc) return rc;
  *bloom_out = f;
  info->has_bloom = mp.has_bloom();
  info->has_zone = ms.has_zone;
  info->zone = cb_zone_bounds{ms.min, ms.min_len, ms.has_min, ms.max, ms.max_len, ms.has_max};
  return CB_OK;
}

int cb_filter_insert_fixed_many(cb_filter* const* filters, uint32_t nf, const uint8_t* const* keys,
                                uint32_t key_len, const uint64_t* n, void* stream) {
  if (nf == 0) return CB_OK;
  if (!filters || !keys || !n) return fail(CB_EINVAL, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const cb_filter* f0 = filters[0];
  if (!f0) return fail(CB_EINVAL, "null filter");
  uint64_t nmax = 0;
  for (uint32_t i = 0; i < nf; ++i) {
    const cb_filter* f = filters[i];
    if (!f) return fail(CB_EINVAL, "null filter");
    if (f->m != f0->m || f->device != f0->device)
      return fail(CB_EINVAL, "batched builds need filters of one size on one device");
    if (n[i] && f->m == 0) return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
    if (n[i])
      if (int rc = null_keys(keys[i], nullptr, key_len)) return rc;
    nmax = std::max(nmax, n[i]);
  }
  if (nmax == 0) return CB_OK;
  if (choose_build_path(f0->m, nmax) != PATH_TILED || nmax > cb::build_chunk_keys()) {
    for (uint32_t i = 0; i < nf; ++i) {  // per-filter builds (direct path or huge batches)
      int rc = insert_impl(filters[i], keys[i], nullptr, key_len, n[i], s);
      if (rc) return rc;
    }
    return CB_OK;
  }
  DeviceGuard dg(f0->device);
  Workspace& ws = workspace(f0->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  // Stage host key arrays into one workspace buffer (16-byte aligned slices).
  std::vector<const uint8_t*> dkeys(nf);
  std::vector<uint64_t> stage_off(nf, 0);
  uint64_t stage_bytes = 0;
  for (uint32_t i = 0; i < nf; ++i) {
    dkeys[i] = keys[i];
    if (n[i] && key_len && !is_device_ptr(keys[i])) {
      stage_off[i] = stage_bytes;
      stage_bytes += ((uint64_t)key_len * n[i] + 15) & ~15ull;
      dkeys[i] = nullptr;
    }
  }
  bool staged = false;
  if (stage_bytes) {
    HIP_TRY(ws.keys.reserve(stage_bytes, s));
    for (uint32_t i = 0; i < nf; ++i)
      if (!dkeys[i]) {
        HIP_TRY(hipMemcpyAsync((uint8_t*)ws.keys.p + stage_off[i], keys[i], (uint64_t)key_len * n[i],
                               hipMemcpyHostToDevice, s));
        dkeys[i] = (const uint8_t*)ws.keys.p + stage_off[i];
      }
    staged = true;
  }
  static const int batch_knob = cb::knob_int("CB_BUILD_BATCH", 0);  // filters per launch pair (tuning)
  const uint32_t kBatch =
      batch_knob >= 1 && batch_knob <= (int)cb::kMaxBuildBatch ? (uint32_t)batch_knob : cb::kMaxBuildBatch;
  const TilePlan p = cb::plan_build(f0->m, nmax, std::min<uint32_t>(nf, kBatch));
  for (uint32_t i = 0; i < nf; ++i)
    if (!covers(filters[i], p)) return fail(CB_EINVAL, "internal: build tile plan exceeds the filter allocation");
  int keyk = cb::KEY_FIXED16;  // only when every filter's keys qualify
  for (uint32_t i = 0; i < nf; ++i)
    if (fixed_keyk(dkeys[i], key_len) != cb::KEY_FIXED16) keyk = cb::KEY_FIXED;
  for (uint32_t b0 = 0; b0 < nf; b0 += kBatch) {
    const uint32_t nb = std::min<uint32_t>(kBatch, nf - b0);
    cb::BuildBatch bb{};
    for (uint32_t j = 0; j < nb; ++j) {
      cb_filter* f = filters[b0 + j];
      HIP_TRY(ready_for_tiled_build(f, s));
      bb.ks[j].bytes = dkeys[b0 + j];
      bb.ks[j].offsets = nullptr;
      bb.ks[j].key_len = key_len;
      bb.n[j] = n[b0 + j];
      bb.words[j] = f->words;
      bb.fresh |= (f->known_zero ? 1ull : 0ull) << j;
    }
    HIP_TRY(ws.seg.reserve(cb::build_seg_bytes(p) * nb, s));
    HIP_TRY(ws.ent.reserve(cb::build_ent_bytes(p) * nb, s));
    HIP_TRY(cb::launch_build_batch(keyk, f0->mode, bb, nb, f0->mp, p, (uint32_t*)ws.seg.p,
                                   (uint32_t*)ws.ent.p, s));
    for (uint32_t j = 0; j < nb; ++j)
      if (n[b0 + j]) filters[b0 + j]->known_zero = false;
    if (int rc = mark_written_many(ws, filters + b0, nb, s)) return rc;  // one event for the batch
  }
  g_last_path = PATH_TILED;
  if (staged) HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

}  // extern "C"
