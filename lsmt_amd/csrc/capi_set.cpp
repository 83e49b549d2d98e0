// capi_set.cpp — the filter-set half of the extern "C" boundary
// (include/cassbloom.h): bit-sliced filter sets and their slots, zone maps
// and the gate, tiered sets, the set probes (zero-copy, dense, wide, fused
// with the exchange pack) and the multi-GPU hit exchange's entry points.
//
// Reference: src/zonemap.rs, src/sstable.rs:138 and src/lib.rs:129-134.
#include "capi_internal.hpp"

using namespace cbx;

namespace {

// The dense set probe (densefs.hip) for this batch? cb_set_dense: 0 auto (by
// density), 1 whenever the shape allows it, -1 never. Never with the zone gate
// or a fused exchange pack.
std::atomic<int> g_set_dense{0};

bool use_dense(const cb_filterset* set, uint64_t n, bool gated, bool pack) {
  const int mode = g_set_dense.load(std::memory_order_relaxed);
  if (mode < 0 || gated || pack || set_is_wide(set)) return false;
  if (mode > 0) return cb::set_dense_shape_ok(set->width, set->m);
  return cb::set_probe_dense_ok(set->width, set->m, n);
}

// The one launch of a set probe: this set, these device keys, this gate
// (gate_on), these device rows, an optional exchange pack sink. Picks the
// wide, dense or plain kernel and builds the zone view the gate needs.
// dense: receives whether the dense probe ran (it sets cb_last_path 6, the
// caller sets every other path); NULL: the dense probe is not an option.
int launch_set(Workspace& ws, const cb_filterset* set, int keyk, const KeySrc& ks, uint64_t n, bool gate,
               uint64_t* hits, const cb::PackSink* sink, bool* dense, hipStream_t s) {
  const uint64_t hwords = (n + 63) / 64;
  hipError_t e;
  if (dense && (*dense = use_dense(set, n, gate, sink != nullptr))) {
    e = ws.dense.reserve(cb::dense_scratch_bytes(set->width, set->m, n), s);
    if (e == hipSuccess)
      e = cb::launch_set_probe_dense(keyk, set->mode, set->width, set->words, set->used, ks, n, set->mp, hits, hwords,
                                     ws.dense.p, s);
    if (e == hipSuccess) g_last_path = 6;
  } else if (set_is_wide(set)) {
    const cb::WideZone wz = wide_zone_view(set);
    e = cb::launch_wide_probe(keyk, set->mode, set->R, (const uint64_t*)set->words, set->used, ks, n, set->mp,
                              gate ? &wz : nullptr, hits, hwords, s);
  } else {
    const cb::ZoneView zv = set_zone_view(set);
    e = cb::launch_set_probe(keyk, set->mode, set->width, set->words, set->used, ks, n, set->mp,
                             gate ? &zv : nullptr, hits, hwords, s, sink);
  }
  if (e != hipSuccess) return hip_fail(e, "launch_set_probe");
  return CB_OK;
}

// Pinned host keys in, pinned host hits out (the query layer's buffers,
// SURVEY.md §8d end-to-end leg): the probe kernel itself loads the keys over
// PCIe and stores the hit rows over PCIe (zero-copy; pinned memory is mapped
// into the device's address space), so the two PCIe directions overlap each
// other and the HBM gathers inside ONE launch. Measured on this stack
// (tools/ubench_pcie.hip): chunked pipelines across copy streams cost more
// per cross-stream event than they overlap (4 chunks, 3 streams: 0.87 ms vs
// 0.50 ms on one stream), while kernel loads from pinned memory run at
// 43-46 GB/s and kernel stores to it at 53 GB/s, the copy engines' rates.
int set_probe_zero_copy(Workspace& ws, const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n,
                        uint64_t* hits, bool gate, hipStream_t s) {
  void *dk = nullptr, *dh = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&dk, const_cast<uint8_t*>(keys), 0));
  HIP_TRY(hipHostGetDevicePointer(&dh, hits, 0));
  const cb::KeySrc ks{(const uint8_t*)dk, nullptr, key_len};
  if (int rc = launch_set(ws, set, fixed_keyk(dk, key_len), ks, n, gate, (uint64_t*)dh, nullptr, nullptr, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));  // the table is no longer read: no reader event needed
  return CB_OK;
}

int set_probe_impl(const cb_filterset* set, const uint8_t* keys, const uint64_t* offsets,
                   uint32_t key_len, uint64_t n, uint64_t* hits, hipStream_t s, bool gated) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (n == 0 || set->used == 0) return CB_OK;
  if (!hits) return fail(CB_EINVAL, "null hits");
  DeviceGuard dg(set->device);
  Workspace& ws = workspace(set->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  const bool gate = gate_on(set, gated);
  if (!offsets && key_len && is_pinned_host(keys) && is_pinned_host(hits)) {
    g_last_path = 4;
    return set_probe_zero_copy(ws, set, keys, key_len, n, hits, gate, s);
  }
  StagedKeys sk;
  int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk);  // (null keys are no pinned keys: refused here)
  if (rc) return rc;
  const size_t rows = (size_t)set->used * ((n + 63) / 64);
  uint64_t* dhits;
  if ((rc = out_buf(ws.hits, hits, rows, s, &dhits))) return rc;
  bool dense = false;
  if ((rc = launch_set(ws, set, sk.keyk, sk.ks, n, gate, dhits, nullptr, &dense, s))) return rc;
  if (gate && (rc = note_zone_read(set, s))) return rc;
  if (!dense) g_last_path = 3;
  return finish_out(hits, dhits, rows * 8, sk.staged, s);
}

}  // namespace

namespace cbx {

int set_probe_device(const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n, bool gated,
                     uint64_t* hits, uint32_t* sink_pack, uint64_t cap, hipStream_t s) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (!n || !set->used) {
    if (sink_pack) {  // no rows or no keys: an empty pack (count 0, every directory entry empty)
      DeviceGuard dg(set->device);
      HIP_TRY(hipMemsetAsync(sink_pack, 0, 8, s));
      if (n) HIP_TRY(hipMemsetAsync(sink_pack + 2 + cap, 0, 8 * cb::set_probe_blocks(n), s));
    }
    return CB_OK;
  }
  if (!hits || (!keys && key_len)) return fail(CB_EINVAL, "null argument");
  if (!is_device_ptr(hits) || (key_len && !is_device_ptr(keys)) || (sink_pack && !is_device_ptr(sink_pack)))
    return fail(CB_EINVAL, "keys, hits and pack must be device memory");
  const uint64_t hwords = (n + 63) / 64;
  if (sink_pack && set_is_wide(set))
    return fail(CB_EINVAL, "the fused probe + pack takes sets of at most 64 slots");
  if (sink_pack && (uint64_t)set->used * hwords * 64 >= (1ull << 32))
    return fail(CB_EINVAL, "used * ceil(n/64) * 64 must be below 2^32 (u32 positions and counts)");
  DeviceGuard dg(set->device);
  Workspace& ws = workspace(set->device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  const bool gate = gate_on(set, gated);
  const cb::KeySrc ks{keys, nullptr, key_len};
  cb::PackSink sink{};
  cb::CompressState* st = nullptr;
  if (sink_pack) {
    int rc = compress_state(ws, s, &st);
    if (rc) return rc;
    sink = cb::PackSink{sink_pack, cap, reinterpret_cast<unsigned long long*>(st->ctl), st->parity};
  }
  bool dense = false;
  if (int rc = launch_set(ws, set, fixed_keyk(keys, key_len), ks, n, gate, hits, sink_pack ? &sink : nullptr, &dense,
                          s)) {
    // the kernel may still have been queued (an earlier sticky error): clear
    // both claim words behind it, so the next launch never reuses a dirty one
    if (st) (void)hipMemsetAsync(st->ctl, 0, 16, s);
    return rc;
  }
  if (dense) return CB_OK;  // (never gated, never with a pack: no reader to note, no claim word used)
  if (st) st->parity ^= 1u;  // the launch cleared the other claim word for the next one
  g_last_path = 3;
  if (gate) return note_zone_read(set, s);
  return CB_OK;
}

int note_zone_read(const cb_filterset* set, hipStream_t s) {
  std::lock_guard<std::mutex> lk(set->zmu);
  hipEvent_t& ev = set->zread[s];
  // The event only tells the host that the readers of the zone table are done
  // (they never write it), so it needs no system-scope release: without the
  // cache write-back an event costs the stream little GPU time.
  if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence));
  HIP_TRY(hipEventRecord(ev, s));
  return CB_OK;
}

int tier_args(const TierList& tl, uint32_t nt, bool gated, cb::TierArgs* out, int* device) {
  if (!tl.sets || !tl.tiers || !tl.slots) return fail(CB_EINVAL, "null argument");
  if (tl.ns < 1 || tl.ns > cb::kMaxTiers) return fail(CB_EINVAL, "a tiered call takes 1 to 8 sets");
  if (nt < 1 || nt > cb::kTierTables) return fail(CB_EINVAL, "a tiered call takes 1 to 64 tables");
  for (uint32_t i = 0; i < tl.ns; ++i) {
    const cb_filterset* set = tl.sets[i];
    if (!set) return fail(CB_EINVAL, "null set");
    if (set->width != 32 && set->width != 64) return fail(CB_EINVAL, "a tier is a set of 32 or 64 slots");
    if (set->device != tl.sets[0]->device) return fail(CB_EINVAL, "tiers live on different devices");
  }
  cb::TierArgs ta;
  std::memset(&ta, 0, sizeof ta);
  ta.ns = tl.ns;
  ta.nt = nt;
  uint32_t count[cb::kMaxTiers] = {};
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t i = tl.tiers[t], sl = tl.slots[t];
    if (i >= tl.ns) return fail(CB_EINVAL, "tier out of range");
    if (sl >= tl.sets[i]->width) return fail(CB_EINVAL, "slot out of range");
    ta.tbl[t] = (uint16_t)(i << 8 | sl);
    ta.tier[i].live |= 1ull << sl;
    ++count[i];
  }
  // the tables grouped by tier (a counting sort: table order kept inside a tier)
  uint32_t at[cb::kMaxTiers];
  for (uint32_t i = 0, o = 0; i < cb::kMaxTiers; ++i) {
    ta.start[i] = (uint8_t)o;
    at[i] = o;
    o += count[i];
    ta.start[i + 1] = (uint8_t)o;
  }
  for (uint32_t t = 0; t < nt; ++t) ta.srt[at[tl.tiers[t]]++] = (uint16_t)(t << 8 | tl.slots[t]);
  ta.all32 = 1;
  int named = -1;
  for (uint32_t i = 0; i < tl.ns; ++i) {
    const cb_filterset* set = tl.sets[i];
    cb::TierDesc& d = ta.tier[i];
    if (!d.live) continue;
    if (named < 0) named = (int)i;
    d.words = set->words;
    d.mp = set->mp;
    d.generic = set->mode == cb::MOD_GENERIC ? ~0ull : 0ull;
    d.half = set->width == 32 ? 1u : 0u;
    if (set->mode != cb::MOD_POW2_32) ta.all32 = 0;
    if (gate_on(set, gated)) {
      d.zv = set_zone_view(set);
      d.zv.gated &= d.live;
    }
  }
  for (uint32_t t = 0; t < nt; ++t)
    if ((ta.tier[tl.tiers[t]].zv.gated >> tl.slots[t]) & 1ull) {
      ta.tgated |= 1ull << t;
      ta.zpre[t] = ta.tier[tl.tiers[t]].zv.pre + 2 * tl.slots[t];
    }
  // tiers no table names, and the entries past ns: a named tier's words with
  // no live slot (in-bounds loads, and the unnamed set is never read)
  for (uint32_t i = 0; i < cb::kMaxTiers; ++i) {
    if (ta.tier[i].live) continue;
    ta.tier[i] = ta.tier[named];
    ta.tier[i].live = 0;
    ta.tier[i].zv.gated = 0;
  }
  *out = ta;
  *device = tl.sets[0]->device;
  return CB_OK;
}

int note_tier_reads(const TierList& tl, const cb::TierArgs& ta, hipStream_t s) {
  for (uint32_t i = 0; i < tl.ns; ++i)
    if (ta.tier[i].zv.gated)
      if (int rc = note_zone_read(tl.sets[i], s)) return rc;
  return CB_OK;
}

}  // namespace cbx

namespace {

// cb_tiers_probe_*: the gate rows of a table list over tiered sets.
int tiers_probe_impl(const TierList& tl, uint32_t nt, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len,
                     uint64_t n, bool gated, uint64_t* hits, hipStream_t s) {
  cb::TierArgs ta;
  int dev = 0;
  if (int rc = tier_args(tl, nt, gated, &ta, &dev)) return rc;
  if (n == 0) return CB_OK;
  if (!hits) return fail(CB_EINVAL, "null hits");
  DeviceGuard dg(dev);
  Workspace& ws = workspace(dev, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  int rc = stage_keys(ws, keys, offsets, key_len, n, s, sk);
  if (rc) return rc;
  const uint64_t hwords = (n + 63) / 64;
  uint64_t* dhits;
  if ((rc = out_buf(ws.hits, hits, (size_t)nt * hwords, s, &dhits))) return rc;
  HIP_TRY(cb::launch_tier_probe(sk.keyk, ta, sk.ks, n, dhits, hwords, s));
  if ((rc = note_tier_reads(tl, ta, s))) return rc;
  return finish_out(hits, dhits, (size_t)nt * hwords * 8, sk.staged, s);
}

// Rebuild and upload the set's zone table (cb::ZoneView layout). Called on
// zone updates, which happen once per table flush: the upload is ordered on
// stream s and waited for, so the host staging vector can be reused.
int upload_zones(cb_filterset* set, hipStream_t s) {
  // layout: 32/64-slot sets cb::ZoneView (64 headers, 128 prefixes, blob);
  // wide sets cb::WideZone (W headers, 2 W prefixes, the gated bits, blob)
  const bool wide = set_is_wide(set);
  const uint32_t nslot = wide ? set->width : 64;
  const size_t hdr_bytes = wide ? wide_zone_hdr_bytes(nslot) : cb_zone_hdr_bytes;
  const size_t pre_bytes = wide ? wide_zone_pre_bytes(nslot) : cb_zone_pre_bytes;
  const size_t blob_off = wide ? wide_zone_blob_off(nslot) : cb_zone_blob_off;
  std::vector<uint32_t> hdr((size_t)nslot * 4, 0u);
  std::vector<cb::BoundPrefix> pre((size_t)nslot * 2);
  std::memset(pre.data(), 0, pre.size() * sizeof(cb::BoundPrefix));
  std::vector<uint8_t> blob;
  set->zg.assign(std::max<uint32_t>(1, set->width / 64), 0ull);
  set->zany = false;
  for (uint32_t i = 0; i < set->width; ++i) {
    if (!(set->zhas_lo[i] && set->zhas_hi[i])) continue;
    set->zg[i >> 6] |= 1ull << (i & 63);
    set->zany = true;
    hdr[4 * i + 0] = (uint32_t)blob.size();
    hdr[4 * i + 1] = (uint32_t)set->zlo[i].size();
    blob.insert(blob.end(), set->zlo[i].begin(), set->zlo[i].end());
    hdr[4 * i + 2] = (uint32_t)blob.size();
    hdr[4 * i + 3] = (uint32_t)set->zhi[i].size();
    blob.insert(blob.end(), set->zhi[i].begin(), set->zhi[i].end());
    // big-endian 16-byte prefixes of both bounds (cb::cmp16's operands)
    for (int j = 0; j < 2; ++j) {
      const std::string& bnd = j ? set->zhi[i] : set->zlo[i];
      cb::BoundPrefix& p = pre[2 * i + j];
      for (size_t k = 0; k < bnd.size() && k < 16; ++k)
        p.w[k >> 2] |= (uint32_t)(uint8_t)bnd[k] << (24 - 8 * (k & 3));
      p.len = (uint32_t)bnd.size();
    }
  }
  set->zgated = wide ? 0 : set->zg[0];
  std::vector<uint8_t> tab(blob_off + blob.size());
  memcpy(tab.data(), hdr.data(), hdr_bytes);
  memcpy(tab.data() + hdr_bytes, pre.data(), pre_bytes);
  if (wide) memcpy(tab.data() + hdr_bytes + pre_bytes, set->zg.data(), set->zg.size() * 8);
  if (!blob.empty()) memcpy(tab.data() + blob_off, blob.data(), blob.size());
  if (!set->zany) return CB_OK;
  // A gated probe or fused read queued on another stream may still read the
  // old table: wait for every stream's last reader (their events), not the
  // whole device, before overwriting it. An outgrown table is retired, not
  // freed (hipFree would synchronise the device), until cb_set_destroy.
  {
    std::lock_guard<std::mutex> lk(set->zmu);
    for (auto& kv : set->zread) HIP_TRY(hipEventSynchronize(kv.second));
  }
  if (tab.size() > set->zcap) {
    if (set->zdev) set->zretired.push_back(set->zdev);
    set->zdev = nullptr;
    set->zcap = 0;
    const size_t want = (tab.size() * 2 + 4095) & ~size_t(4095);
    if (hipMalloc(&set->zdev, want) != hipSuccess) {
      (void)hipGetLastError();
      set->zgated = 0;
      set->zany = false;
      return fail(CB_ENOMEM, "hipMalloc failed for zone table");
    }
    set->zcap = want;
  }
  HIP_TRY(hipMemcpyAsync(set->zdev, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// A slot that receives another table's filter starts with no zone map
// (accept-all), so a stale zone can never hide a key. Headers of ungated
// slots are never read, so no upload is needed.
bool reset_zone(cb_filterset* set, uint32_t slot) {
  const bool was = (slot >> 6) < set->zg.size() && ((set->zg[slot >> 6] >> (slot & 63)) & 1ull);
  set->zlo[slot].clear();
  set->zhi[slot].clear();
  set->zhas_lo[slot] = set->zhas_hi[slot] = 0;
  if (slot < 64) set->zgated &= ~(1ull << slot);
  if ((slot >> 6) < set->zg.size()) set->zg[slot >> 6] &= ~(1ull << (slot & 63));
  bool any = false;
  for (uint64_t w : set->zg) any |= w != 0;
  set->zany = any;
  return was;
}

// After zone resets: a wide set's kernels read the gated bits from its device
// table (a 32/64-slot set passes them by value), so a reset slot that was
// gated needs a new table before the next gated launch.
int zones_after_reset(cb_filterset* set, bool changed, hipStream_t s) {
  if (!changed || !set_is_wide(set)) return CB_OK;
  return upload_zones(set, s);
}

bool slot_dirty(const cb_filterset* set, uint32_t slot) { return (set->dirty[slot >> 6] >> (slot & 63)) & 1ull; }

// Bytes of key i of a staged batch (device-resident) into out.
int fetch_key(const StagedKeys& sk, uint64_t i, std::string& out, hipStream_t s) {
  uint64_t o[2];
  if (sk.keyk == cb::KEY_VAR) {
    HIP_TRY(hipMemcpyAsync(o, sk.ks.offsets + i, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else {
    o[0] = i * sk.ks.key_len;
    o[1] = o[0] + sk.ks.key_len;
  }
  out.assign((size_t)(o[1] - o[0]), '\0');
  if (o[1] > o[0]) {
    HIP_TRY(hipMemcpyAsync(&out[0], sk.ks.bytes + o[0], (size_t)(o[1] - o[0]),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return CB_OK;
}

int zone_bounds_impl(int device, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len,
                     uint64_t n, hipStream_t s, uint64_t* min_idx, uint64_t* max_idx,
                     std::string* lo, std::string* hi) {
  if (min_idx) *min_idx = ~0ull;
  if (max_idx) *max_idx = ~0ull;
  if (n == 0) return CB_OK;
  int rc = null_keys(keys, offsets, key_len);  // (before the device is looked at, as ever)
  if (rc) return rc;
  if ((rc = cb_init(device))) return rc;
  DeviceGuard dg(device);
  Workspace& ws = workspace(device, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  if ((rc = stage_keys(ws, keys, offsets, key_len, n, s, sk))) return rc;
  HIP_TRY(ws.zone.reserve((2 * 1024 + 2) * 8, s));
  uint64_t* dtmp = (uint64_t*)ws.zone.p;
  uint64_t* didx = dtmp + 2 * 1024;
  HIP_TRY(cb::launch_zone_bounds(sk.keyk, sk.ks, n, dtmp, didx, s));
  uint64_t idx[2];
  HIP_TRY(hipMemcpyAsync(idx, didx, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (min_idx) *min_idx = idx[0];
  if (max_idx) *max_idx = idx[1];
  if (lo && (rc = fetch_key(sk, idx[0], *lo, s))) return rc;
  if (hi && (rc = fetch_key(sk, idx[1], *hi, s))) return rc;
  return CB_OK;
}

// cb_set_zone_from_keys_*: ZoneMap::update over the batch, merged with the
// slot's current bounds.
int set_zone_from_keys(cb_filterset* set, uint32_t slot, const uint8_t* keys, const uint64_t* offsets,
                       uint32_t key_len, uint64_t n, hipStream_t s) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  std::string lo, hi;
  int rc = zone_bounds_impl(set->device, keys, offsets, key_len, n, s, nullptr, nullptr, &lo, &hi);
  if (rc || n == 0) return rc;  // no keys: ZoneMap::update never ran, zone unchanged
  DeviceGuard dg(set->device);
  auto less = [](const std::string& a, const std::string& b) {
    return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end(),
                                        [](char x, char y) { return (uint8_t)x < (uint8_t)y; });
  };
  if (!set->zhas_lo[slot] || less(lo, set->zlo[slot])) set->zlo[slot] = lo;
  if (!set->zhas_hi[slot] || less(set->zhi[slot], hi)) set->zhi[slot] = hi;
  set->zhas_lo[slot] = set->zhas_hi[slot] = 1;
  return upload_zones(set, s);
}

}  // namespace

extern "C" {

int cb_set_dense(int mode) {
  if (mode < -1 || mode > 1) return fail(CB_EINVAL, "mode must be -1, 0 or 1");
  g_set_dense.store(mode, std::memory_order_relaxed);
  return CB_OK;
}

// ---- the multi-GPU hit exchange ----

int cb_hits_compress(const uint64_t* hits, uint64_t rows, uint64_t words, uint32_t* pack,
                     uint64_t cap, void* stream) {
  if (!pack || (rows * words && !hits)) return fail(CB_EINVAL, "null argument");
  if (rows && words && (words > cb::kMaxCompressWords || rows * words > cb::kMaxCompressWords))
    return fail(CB_EINVAL, "rows * words * 64 must be below 2^32");
  hipStream_t s = (hipStream_t)stream;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  Workspace& ws = workspace(dev, s);
  std::lock_guard<std::mutex> lk(ws.mu);
  cb::CompressState* st = nullptr;
  int rc = compress_state(ws, s, &st);
  if (rc) return rc;
  HIP_TRY(cb::launch_hits_compress(hits, rows, words, pack, cap, *st, s));
  return CB_OK;
}

int cb_hits_expand(const uint32_t* packs, uint32_t nranks, uint64_t cap, const uint64_t* row_off,
                   uint64_t words, uint64_t total_rows, uint64_t* full, uint32_t* ok, void* stream) {
  if (!full || (nranks && (!packs || !row_off))) return fail(CB_EINVAL, "null argument");
  if (nranks > cb::kMaxRanks) return fail(CB_EINVAL, "more than 64 ranks");
  cb::RankRows rr{};
  for (uint32_t r = 0; r < nranks; ++r) {
    rr.row_off[r] = row_off[r];
    const uint64_t end = r + 1 < nranks ? row_off[r + 1] : total_rows;
    if ((r == 0 && row_off[0] != 0) || end < row_off[r] || end > total_rows)
      return fail(CB_EINVAL, "row_off must start at 0 and be non-decreasing up to total_rows");
    if ((end - row_off[r]) * words > cb::kMaxCompressWords)
      return fail(CB_EINVAL, "a rank's rows * words * 64 must be below 2^32");
  }
  HIP_TRY(cb::launch_hits_expand(packs, nranks, cap, rr, words, total_rows, full, ok, (hipStream_t)stream));
  return CB_OK;
}

int cb_hits_pack_words(uint64_t rows, uint64_t words, uint64_t cap, uint64_t* out) {
  if (!out) return fail(CB_EINVAL, "null out");
  *out = cb::pack_words(rows * words, cap);
  return CB_OK;
}

int cb_set_pack_words(uint64_t n, uint64_t cap, uint64_t* out) {
  if (!out) return fail(CB_EINVAL, "null out");
  *out = 2 + cap + 2 * cb::set_probe_blocks(n);
  return CB_OK;
}

int cb_set_probe_pack_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n, int gated,
                            uint64_t* hits, uint32_t* pack, uint64_t cap, void* stream) {
  if (!pack) return fail(CB_EINVAL, "null pack");
  return set_probe_device(set, keys, key_len, n, gated != 0, hits, pack, cap, (hipStream_t)stream);
}

int cb_hits_expand_set(const uint32_t* packs, uint32_t nranks, uint64_t cap, const uint64_t* row_off, uint64_t n,
                       uint64_t total_rows, uint64_t* full, uint32_t* ok, void* stream) {
  if (!full || (nranks && (!packs || !row_off))) return fail(CB_EINVAL, "null argument");
  if (!nranks || nranks > cb::kMaxRanks) return fail(CB_EINVAL, "need 1..64 ranks");
  cb::RankRows rr{};
  for (uint32_t r = 0; r < nranks; ++r) rr.row_off[r] = row_off[r];
  const uint64_t nblk = cb::set_probe_blocks(n);
  const uint64_t stride = 2 + cap + 2 * nblk;
  hipError_t e = cb::launch_hits_expand_blocks(packs, nranks, cap, stride, rr, (n + 63) / 64, total_rows,
                                               (uint32_t)nblk, cb::kSetWords, full, ok, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(CB_EINVAL, "row_off must start at 0 and grow to total_rows with at most 64 rows per rank");
  HIP_TRY(e);
  return CB_OK;
}

int cb_set_load_meta(cb_filterset* set, uint32_t slot, const uint8_t* in, uint64_t len, void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  cb_filter* f = nullptr;
  cb_meta_info info;
  int rc = cb_meta_decode(in, len, set->device, &f, &info);
  if (rc) return rc;
  if (f->m != set->m) {
    cb_filter_destroy(f);
    return fail(CB_EINVAL, "the table's filter size differs from the set's m");
  }
  rc = cb_set_assign(set, slot, f, stream);
  if (!rc) {
    const cb_zone_bounds& z = info.zone;
    rc = cb_set_zone(set, slot, z.min, z.min_len, z.has_min, z.max, z.max_len, z.has_max, stream);
  }
  // the assign is stream-ordered: wait before the temporary filter goes away
  if (!rc) rc = cb_stream_synchronize(stream);
  cb_filter_destroy(f);
  return rc;
}

// ---- bit-sliced filter sets ----

int cb_set_create(uint64_t m_bits, uint32_t width, int device, cb_filterset** out) {
  if (!out) return fail(CB_EINVAL, "null out");
  *out = nullptr;
  if (!(width == 32 || width == 64 || (width % 64 == 0 && width <= cb::kWideMax)))
    return fail(CB_EINVAL, "set width must be 32, 64 or a multiple of 64 up to 4096");
  if (m_bits == 0) return fail(CB_EZEROM, "attempt to calculate the remainder with a divisor of zero");
  int rc = cb_init(device);
  if (rc) return rc;
  DeviceGuard dg(device);
  std::unique_ptr<cb_filterset> set(new cb_filterset());
  set->m = m_bits;
  set->device = device;
  set->width = width;
  set->mp = cb::make_modp(m_bits, &set->mode);
  set->zlo.assign(width, std::string());
  set->zhi.assign(width, std::string());
  set->zhas_lo.assign(width, 0);
  set->zhas_hi.assign(width, 0);
  set->dirty.assign(std::max<uint32_t>(1, width / 64), 0ull);
  set->zg.assign(std::max<uint32_t>(1, width / 64), 0ull);
  set->R = width > 64 ? width / 64 : 0;
  const size_t bytes = width > 64 ? (size_t)m_bits * (width / 8) : (size_t)((m_bits + 31) / 32 * 32) * (width / 8);
  if (pool_alloc(device, bytes, &set->words, &set->words_cap) != hipSuccess) {
    set->words = nullptr;
    return fail(CB_ENOMEM, "device allocation failed for filter set words");
  }
  HIP_TRY(hipMemsetAsync(set->words, 0, bytes, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = set.release();
  return CB_OK;
}

int cb_set_destroy(cb_filterset* set) {
  if (!set) return CB_OK;
  {
    DeviceGuard dg(set->device);
    pool_release(set->device, set->words, set->words_cap);  // (stream-ordered: no device sync)
    if (set->zdev) (void)hipFree(set->zdev);
    if (set->wfw) (void)hipFree(set->wfw);
    for (void* z : set->zretired) (void)hipFree(z);
    for (auto& kv : set->zread) (void)hipEventDestroy(kv.second);
  }
  delete set;
  return CB_OK;
}

int cb_set_info(const cb_filterset* set, uint64_t* m_out, uint32_t* width_out, uint32_t* used_out) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (m_out) *m_out = set->m;
  if (width_out) *width_out = set->width;
  if (used_out) *used_out = set->used;
  return CB_OK;
}

int cb_set_assign(cb_filterset* set, uint32_t slot, const cb_filter* f, void* stream) {
  if (!set || !f) return fail(CB_EINVAL, "null argument");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  if (f->m != set->m) return fail(CB_EINVAL, "filter size differs from the set's m");
  if (f->device != set->device) return fail(CB_EINVAL, "filter and set live on different devices");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(set->device);
  HIP_TRY(ensure_zeroed(f, s));
  if (set_is_wide(set)) {
    uint64_t* w = (uint64_t*)set->words;
    if (slot_dirty(set, slot))
      HIP_TRY(cb::launch_wide_put_slot(f->words, set->m, slot, set->R, w, s));
    else
      HIP_TRY(cb::launch_wide_or_slot(f->words, set->m, slot, set->R, w, s));
  } else if (slot_dirty(set, slot)) {
    HIP_TRY(cb::launch_set_put_slot(f->words, set->m, slot, set->width, set->words, s));
  } else {
    HIP_TRY(cb::launch_set_or_slot(f->words, set->m, slot, set->width, set->words, s));
  }
  set->dirty[slot >> 6] |= 1ull << (slot & 63);
  set->used = std::max(set->used, slot + 1);
  return zones_after_reset(set, reset_zone(set, slot), s);
}

int cb_set_assign_all(cb_filterset* set, const cb_filter* const* filters, uint32_t nf, void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (nf > set->width) return fail(CB_EINVAL, "more filters than set slots");
  if (nf && !filters) return fail(CB_EINVAL, "null filters");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard dg(set->device);
  FilterPtrs fp{};
  std::vector<const uint32_t*> ptrs(nf);
  for (uint32_t i = 0; i < nf; ++i) {
    const cb_filter* f = filters[i];
    if (!f) return fail(CB_EINVAL, "null filter");
    if (f->m != set->m) return fail(CB_EINVAL, "filter size differs from the set's m");
    if (f->device != set->device) return fail(CB_EINVAL, "filter and set live on different devices");
    HIP_TRY(ensure_zeroed(f, s));
    ptrs[i] = f->words;
    if (i < 64) {
      fp.w[i] = f->words;
      fp.row[i] = i;
    }
  }
  if (set_is_wide(set)) {
    // the filters' word pointers in device memory for the one-launch build
    const size_t pb = std::max<size_t>(8, (size_t)nf * sizeof(void*));
    if (pb > set->wfw_cap) {
      HIP_TRY(hipStreamSynchronize(s));  // an earlier build may still read the old array
      if (set->wfw) HIP_TRY(hipFree(set->wfw));
      set->wfw = nullptr;
      set->wfw_cap = 0;
      HIP_TRY(hipMalloc(&set->wfw, pb));
      set->wfw_cap = pb;
    }
    if (nf) HIP_TRY(hipMemcpyAsync(set->wfw, ptrs.data(), (size_t)nf * sizeof(void*), hipMemcpyHostToDevice, s));
    HIP_TRY(cb::launch_wide_build((const uint32_t* const*)set->wfw, nf, set->m, set->R, (uint64_t*)set->words, s));
    HIP_TRY(hipStreamSynchronize(s));  // the pageable pointer array is copied, and wfw is reused
  } else {
    HIP_TRY(cb::launch_set_build(fp, nf, set->m, set->width, set->words, s));
  }
  set->used = nf;
  for (size_t j = 0; j < set->dirty.size(); ++j) {
    const uint32_t lo = (uint32_t)j * 64;
    set->dirty[j] = nf >= lo + 64 ? ~0ull : (nf > lo ? ((1ull << (nf - lo)) - 1) : 0ull);
  }
  bool changed = false;
  for (uint32_t i = 0; i < set->width; ++i) changed |= reset_zone(set, i);
  return zones_after_reset(set, changed, s);
}

int cb_set_clear_slot(cb_filterset* set, uint32_t slot, void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  DeviceGuard dg(set->device);
  note_stream(set->device, (hipStream_t)stream);
  int rc = zones_after_reset(set, reset_zone(set, slot), (hipStream_t)stream);
  if (rc || !slot_dirty(set, slot)) return rc;
  if (set_is_wide(set))
    HIP_TRY(cb::launch_wide_put_slot(nullptr, set->m, slot, set->R, (uint64_t*)set->words, (hipStream_t)stream));
  else
    HIP_TRY(cb::launch_set_put_slot(nullptr, set->m, slot, set->width, set->words,
                                    (hipStream_t)stream));
  set->dirty[slot >> 6] &= ~(1ull << (slot & 63));
  return CB_OK;
}

int cb_set_probe_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n,
                       uint64_t* hits, void* stream) {
  return set_probe_impl(set, keys, nullptr, key_len, n, hits, (hipStream_t)stream, false);
}

int cb_set_probe_var(const cb_filterset* set, const uint8_t* bytes, const uint64_t* offsets,
                     uint64_t n, uint64_t* hits, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return set_probe_impl(set, bytes, offsets, 0, n, hits, (hipStream_t)stream, false);
}

// ---- zone maps (src/zonemap.rs) and the SsTable::get gate ----

int cb_set_zone(cb_filterset* set, uint32_t slot, const uint8_t* min, uint64_t min_len,
                int has_min, const uint8_t* max, uint64_t max_len, int has_max, void* stream) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  if ((has_min && min_len && !min) || (has_max && max_len && !max))
    return fail(CB_EINVAL, "null zone bound");
  if ((has_min && min_len > 0xFFFFFFFFull) || (has_max && max_len > 0xFFFFFFFFull))
    return fail(CB_EINVAL, "zone bound longer than 4 GiB");
  DeviceGuard dg(set->device);
  set->zlo[slot].assign(has_min ? (const char*)min : "", has_min ? (size_t)min_len : 0);
  set->zhi[slot].assign(has_max ? (const char*)max : "", has_max ? (size_t)max_len : 0);
  set->zhas_lo[slot] = has_min ? 1 : 0;
  set->zhas_hi[slot] = has_max ? 1 : 0;
  return upload_zones(set, (hipStream_t)stream);
}

int cb_set_zone_get(const cb_filterset* set, uint32_t slot, uint8_t* min, uint64_t min_cap,
                    uint64_t* min_len, int* has_min, uint8_t* max, uint64_t max_cap,
                    uint64_t* max_len, int* has_max) {
  if (!set) return fail(CB_EINVAL, "null set");
  if (slot >= set->width) return fail(CB_EINVAL, "slot out of range");
  const std::string &lo = set->zlo[slot], &hi = set->zhi[slot];
  if (has_min) *has_min = set->zhas_lo[slot];
  if (has_max) *has_max = set->zhas_hi[slot];
  if (min_len) *min_len = lo.size();
  if (max_len) *max_len = hi.size();
  if (min && min_cap >= lo.size() && !lo.empty()) memcpy(min, lo.data(), lo.size());
  if (max && max_cap >= hi.size() && !hi.empty()) memcpy(max, hi.data(), hi.size());
  return CB_OK;
}

int cb_set_zone_from_keys_fixed(cb_filterset* set, uint32_t slot, const uint8_t* keys,
                                uint32_t key_len, uint64_t n, void* stream) {
  return set_zone_from_keys(set, slot, keys, nullptr, key_len, n, (hipStream_t)stream);
}

int cb_set_zone_from_keys_var(cb_filterset* set, uint32_t slot, const uint8_t* bytes,
                              const uint64_t* offsets, uint64_t n, void* stream) {
  // (a null set and a slot out of range are refused first, by set_zone_from_keys)
  if (set && slot < set->width && !offsets) return fail(CB_EINVAL, "null offsets");
  return set_zone_from_keys(set, slot, bytes, offsets, 0, n, (hipStream_t)stream);
}

int cb_zone_bounds_fixed(const uint8_t* keys, uint32_t key_len, uint64_t n, int device,
                         uint64_t* min_idx, uint64_t* max_idx, void* stream) {
  return zone_bounds_impl(device, keys, nullptr, key_len, n, (hipStream_t)stream, min_idx,
                          max_idx, nullptr, nullptr);
}

int cb_zone_bounds_var(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, int device,
                       uint64_t* min_idx, uint64_t* max_idx, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return zone_bounds_impl(device, bytes, offsets, 0, n, (hipStream_t)stream, min_idx, max_idx,
                          nullptr, nullptr);
}

int cb_set_probe_gated_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len,
                             uint64_t n, uint64_t* hits, void* stream) {
  return set_probe_impl(set, keys, nullptr, key_len, n, hits, (hipStream_t)stream, true);
}

int cb_set_probe_gated_var(const cb_filterset* set, const uint8_t* bytes, const uint64_t* offsets,
                           uint64_t n, uint64_t* hits, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return set_probe_impl(set, bytes, offsets, 0, n, hits, (hipStream_t)stream, true);
}

int cb_tiers_probe_fixed(const cb_filterset* const* sets, uint32_t ns, const uint32_t* tiers,
                         const uint32_t* slots, uint32_t nt, const uint8_t* keys, uint32_t key_len, uint64_t n,
                         int gated, uint64_t* hits, void* stream) {
  return tiers_probe_impl(TierList{sets, ns, tiers, slots}, nt, keys, nullptr, key_len, n, gated != 0, hits,
                          (hipStream_t)stream);
}

int cb_tiers_probe_var(const cb_filterset* const* sets, uint32_t ns, const uint32_t* tiers, const uint32_t* slots,
                       uint32_t nt, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, int gated,
                       uint64_t* hits, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return tiers_probe_impl(TierList{sets, ns, tiers, slots}, nt, bytes, offsets, 0, n, gated != 0, hits,
                          (hipStream_t)stream);
}

}  // extern "C"
