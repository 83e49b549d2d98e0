// capi_ring.cpp — the token ring's entries (ring.hpp): the ring handle and its
// host answers (cb_ring_create*, cb_ring_info, cb_ring_tokens,
// cb_ring_replicas), the batched route (cb_ring_route_*, cb_scan_route) and
// the compaction that keeps what a node owns (cb_tables_compact_ring), which
// is compaction's steps (capi_merge.hpp) with k_ring_keep behind the select.
//
// Reference: src/cluster.rs:46-54 (Cluster::new's ring), src/cluster.rs:102-123
// (replicas_for), src/query.rs:448-528, 697-713, 734-760 (the partition keys
// it is asked about), src/cluster.rs:277-286, 313-314 (catalog writes go to
// the whole ring).
#include "capi_merge.hpp"
#include "keyrange.hpp"
#include "ring.hpp"

using namespace cbx;
using cb::MergeOrder;
using cb::MergeRule;

namespace {

// A ring: its host form (immutable once built) and, per device, a copy made
// on that device's first route or compaction.
struct RingDevice {
  void* block = nullptr;
  size_t cap = 0;
  cb::RingView view{};
};
struct Ring {
  cb::RingHost host;
  std::mutex mu;
  std::map<int, RingDevice> dev;
};

int adopt_ring(const char* why, cb::RingHost& built, void** out) {
  if (why) return fail(CB_EINVAL, why);
  Ring* r = new Ring();
  r->host = std::move(built);
  *out = r;
  return CB_OK;
}

// The ring on `dev` (the current device): made on first use, under the
// ring's lock, on s, and waited for there (the source is pageable, and later
// calls on other streams find it complete).
int ring_on_device(const Ring* ring, int dev, hipStream_t s, cb::RingView* out) {
  Ring* r = const_cast<Ring*>(ring);
  std::lock_guard<std::mutex> lk(r->mu);
  auto it = r->dev.find(dev);
  if (it != r->dev.end()) {
    *out = it->second.view;
    return CB_OK;
  }
  const cb::RingHost& h = r->host;
  const uint64_t npos = h.tokens.size();
  const bool big = npos > cb::kRingLdsPositions;
  const uint32_t bits = big ? cb::ring_bucket_bits(npos) : 0;
  std::vector<uint32_t> first;
  if (big) {
    first.assign((1ull << bits) + 1, (uint32_t)npos);
    uint64_t p = 0;
    for (uint64_t b = 0; b < (1ull << bits); ++b) {  // the first position whose top bits are >= b
      while (p < npos && (h.tokens[p] >> (32 - bits)) < b) ++p;
      first[b] = (uint32_t)p;
    }
  }
  cb::Carver c;
  const size_t o_tok = c.take(npos * 4), o_rows = c.take(h.rows.size() * 4), o_first = c.take(first.size() * 4);
  RingDevice d;
  if (int rc = pool_alloc_or(dev, c.total(), &d.block, &d.cap, "device allocation failed for a ring")) return rc;
  uint8_t* b = (uint8_t*)d.block;
  hipError_t e = hipMemcpyAsync(b + o_tok, h.tokens.data(), npos * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_rows, h.rows.data(), h.rows.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && big)
    e = hipMemcpyAsync(b + o_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    pool_release(dev, d.block, d.cap);
    return hip_fail(e, "ring upload");
  }
  d.view = cb::RingView{(const uint32_t*)(b + o_tok), (const int32_t*)(b + o_rows),
                        big ? (const uint32_t*)(b + o_first) : nullptr, (uint32_t)npos, h.rf, bits};
  r->dev[dev] = d;
  *out = d.view;
  return CB_OK;
}

int launch_try(int e, const char* where) { return e ? hip_fail((hipError_t)e, where) : CB_OK; }

// cb_ring_route_fixed / _var: cb_probe_*'s frame (device buffers in place and
// asynchronous, host buffers staged and waited for) around k_ring_route.
int route_impl(const void* ring, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len, uint64_t n,
               uint32_t skip, uint32_t npk, int device, uint32_t* tokens, int32_t* replicas, hipStream_t s) {
  const Ring* r = (const Ring*)ring;
  if (!tokens && !replicas) return fail(CB_EINVAL, "null argument");
  if (!r) return fail(CB_EINVAL, "null ring");
  if (!n) return CB_OK;
  int rc = cb_init(device);
  if (rc) return rc;
  DeviceGuard dg(device);
  Workspace& ws = workspace(device, s);
  cb::RingView rv;
  if ((rc = ring_on_device(r, device, s, &rv))) return rc;
  std::lock_guard<std::mutex> lk(ws.mu);
  StagedKeys sk;
  if ((rc = stage_keys(ws, keys, offsets, key_len, n, s, sk))) return rc;
  // host outputs are produced in a scratch block and copied back
  const bool tok_here = tokens && !is_device_ptr(tokens), rep_here = replicas && !is_device_ptr(replicas);
  TempBlock tmp{device};
  cb::Carver c;
  const size_t o_tok = c.take(tok_here ? n * 4 : 0), o_rep = c.take(rep_here ? n * rv.rf * 4 : 0);
  if (c.total() && (rc = tmp.alloc(c, "device allocation failed for a route's answers"))) return rc;
  uint32_t* dtok = tok_here ? (uint32_t*)tmp.at(o_tok) : tokens;
  int32_t* drep = rep_here ? (int32_t*)tmp.at(o_rep) : replicas;
  const cb::RouteKeys ks{sk.ks.bytes, sk.keyk == cb::KEY_VAR ? sk.ks.offsets : nullptr, sk.ks.key_len};
  const cb::RouteRule rule{skip, npk, nullptr, nullptr, nullptr, 0};
  if ((rc = launch_try(cb::launch_ring_route(rv, ks, rule, n, dtok, drep, s), "k_ring_route"))) return rc;
  if (tok_here) HIP_TRY(hipMemcpyAsync(tokens, dtok, n * 4, hipMemcpyDeviceToHost, s));
  if (rep_here) HIP_TRY(hipMemcpyAsync(replicas, drep, n * rv.rf * 4, hipMemcpyDeviceToHost, s));
  if (tok_here || rep_here || sk.staged) HIP_TRY(hipStreamSynchronize(s));
  return CB_OK;
}

// A cb_key_rules checked (cb_tables_scan_prefixes' ordering rule through the
// same check) and packed.
int take_rules(const void* rules, cb::KeyRules* out) {
  const cb_key_rules* k = (const cb_key_rules*)rules;
  if (!k) return fail(CB_EINVAL, "null rules");
  *out = cb::KeyRules{};
  const uint32_t np = k->np;
  if (!np) return CB_OK;
  if (np > cb::kRingMaxPrefixes) return fail(CB_EINVAL, "too many prefixes (at most 256)");
  if (!k->prefix_off || !k->npk) return fail(CB_EINVAL, "null prefix offsets or npk with a non-zero count");
  for (uint32_t i = 0; i < np; ++i)
    if (k->prefix_off[i + 1] < k->prefix_off[i]) return fail(CB_EINVAL, "prefix offsets decrease");
  const uint64_t bytes = k->prefix_off[np] - k->prefix_off[0];
  if (bytes > cb::kRingMaxPrefixBytes) return fail(CB_EINVAL, "too many prefix bytes (at most 4096)");
  if (bytes && !k->prefixes) return fail(CB_EINVAL, "null prefixes with a non-zero total");
  std::vector<uint8_t> bounds;
  std::vector<uint64_t> off;
  bool last_unbounded = false;
  if (cb::prefix_list_to_ranges(k->prefixes, k->prefix_off, np, bounds, off, &last_unbounded) >= 0)
    return fail(CB_EINVAL, "a prefix without an end before the last one (or prefix offsets that decrease)");
  if (cb::range_list_first_bad(bounds.data(), off.data(), np, last_unbounded) >= 0)
    return fail(CB_EINVAL, "the prefixes are not ascending and disjoint");
  out->np = np;
  for (uint32_t i = 0; i < np; ++i) {
    out->npk[i] = k->npk[i];
    out->at[i] = (uint16_t)(k->prefix_off[i] - k->prefix_off[0]);
  }
  for (uint32_t i = np; i <= cb::kRingMaxPrefixes; ++i) out->at[i] = (uint16_t)bytes;
  if (bytes) std::memcpy(out->bytes, k->prefixes + k->prefix_off[0], bytes);
  return CB_OK;
}

}  // namespace

extern "C" {

int cb_ring_create_tokens(const uint32_t* tokens, const uint32_t* owners, uint64_t npos, uint32_t nnodes, uint32_t rf,
                          void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  if (!tokens || !owners) return fail(CB_EINVAL, "null argument");
  cb::RingHost h;
  return adopt_ring(cb::ring_build_tokens(tokens, owners, npos, nnodes, rf, &h), h, out);
}

int cb_ring_create(const uint8_t* names, const uint64_t* name_off, uint32_t nnodes, uint32_t vnodes, uint32_t rf,
                   void** out) {
  if (!out) return fail(CB_EINVAL, "null argument");
  *out = nullptr;
  if (!names || !name_off) return fail(CB_EINVAL, "null argument");
  cb::RingHost h;
  return adopt_ring(cb::ring_build_names(names, name_off, nnodes, vnodes, rf, &h), h, out);
}

int cb_ring_info(const void* ring, uint32_t* nnodes, uint32_t* rf, uint64_t* positions, uint32_t* width) {
  const Ring* r = (const Ring*)ring;
  if (!r) return fail(CB_EINVAL, "null ring");
  if (nnodes) *nnodes = r->host.nnodes;
  if (rf) *rf = r->host.rf;
  if (positions) *positions = r->host.tokens.size();
  if (width) *width = r->host.width;
  return CB_OK;
}

int cb_ring_tokens(const void* ring, uint32_t* tokens, uint32_t* owners) {
  const Ring* r = (const Ring*)ring;
  if (!r) return fail(CB_EINVAL, "null ring");
  const size_t bytes = r->host.tokens.size() * 4;
  if (tokens) std::memcpy(tokens, r->host.tokens.data(), bytes);
  if (owners) std::memcpy(owners, r->host.owners.data(), bytes);
  return CB_OK;
}

int cb_ring_replicas(const void* ring, const uint8_t* key, uint64_t len, uint32_t skip, uint32_t npk, uint32_t* token,
                     int32_t* replicas) {
  const Ring* r = (const Ring*)ring;
  if (!r) return fail(CB_EINVAL, "null ring");
  if (len && !key) return fail(CB_EINVAL, "null key with a length");
  const uint64_t s = skip < len ? skip : len;
  const uint8_t* rest = key + s;
  const uint32_t t = cb::murmur3_32(rest, cb::partition_key_len(rest, len - s, npk));
  if (token) *token = t;
  if (replicas) {
    const int32_t* row = &r->host.rows[cb::ring_position(r->host, t) * r->host.rf];
    std::copy(row, row + r->host.rf, replicas);
  }
  return CB_OK;
}

// The device copies are retired through the block pool: nothing is waited for.
int cb_ring_destroy(void* ring) {
  Ring* r = (Ring*)ring;
  if (!r) return CB_OK;
  for (auto& kv : r->dev) {
    DeviceGuard dg(kv.first);
    pool_release(kv.first, kv.second.block, kv.second.cap);
  }
  delete r;
  return CB_OK;
}

int cb_ring_route_fixed(const void* ring, const uint8_t* keys, uint32_t key_len, uint64_t n, uint32_t skip,
                        uint32_t npk, int device, uint32_t* tokens, int32_t* replicas, void* stream) {
  return route_impl(ring, keys, nullptr, key_len, n, skip, npk, device, tokens, replicas, (hipStream_t)stream);
}

int cb_ring_route_var(const void* ring, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t skip,
                      uint32_t npk, int device, uint32_t* tokens, int32_t* replicas, void* stream) {
  if (!offsets) return fail(CB_EINVAL, "null offsets");
  return route_impl(ring, bytes, offsets, 0, n, skip, npk, device, tokens, replicas, (hipStream_t)stream);
}

// The route over a finished result's keys, into a scratch block on the null
// stream, then copied as cb_scan_which copies. The ranges' offsets, skips and
// npks travel in the same block.
int cb_scan_route(const void* scan, const void* ring, const uint32_t* skip, const uint32_t* npk, uint32_t* tokens,
                  int32_t* replicas) {
  const cb_scan* r = (const cb_scan*)scan;
  const Ring* rg = (const Ring*)ring;
  if (!tokens && !replicas) return fail(CB_EINVAL, "null argument");
  if (!rg) return fail(CB_EINVAL, "null ring");
  if (!r) return fail(CB_EINVAL, "null scan");
  if (!r->count) return CB_OK;
  DeviceGuard dg(r->device);
  note_stream(r->device, nullptr);  // (the pool retires the scratch behind the null stream too)
  cb::RingView rv;
  if (int rc = ring_on_device(rg, r->device, nullptr, &rv)) return rc;
  TempBlock tmp{r->device};
  const size_t nro = r->range_off.size(), nr = nro - 1;
  const bool ranged = skip || npk;
  Staging up;
  cb::Carver& c = up.c;
  const size_t o_roff = c.take(ranged ? nro * 8 : 0), o_skip = c.take(skip ? nr * 4 : 0),
               o_npk = c.take(npk ? nr * 4 : 0);
  up.seal();
  const size_t o_tok = c.take(tokens ? r->count * 4 : 0), o_rep = c.take(replicas ? r->count * rv.rf * 4 : 0);
  if (int rc = tmp.alloc(c, "device allocation failed for a scan's route")) return rc;
  if (ranged) {
    up.put(o_roff, r->range_off.data(), nro * 8);
    if (skip) up.put(o_skip, skip, nr * 4);
    if (npk) up.put(o_npk, npk, nr * 4);
    HIP_TRY(up.upload(tmp, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));  // the source is pageable
  }
  uint32_t* dtok = tokens ? (uint32_t*)tmp.at(o_tok) : nullptr;
  int32_t* drep = replicas ? (int32_t*)tmp.at(o_rep) : nullptr;
  const cb::RouteKeys ks{r->keys, r->key_off, 0};
  const cb::RouteRule rule{0,
                           0,
                           ranged ? (const uint64_t*)tmp.at(o_roff) : nullptr,
                           skip ? (const uint32_t*)tmp.at(o_skip) : nullptr,
                           npk ? (const uint32_t*)tmp.at(o_npk) : nullptr,
                           (uint32_t)nr};
  if (int rc = launch_try(cb::launch_ring_route(rv, ks, rule, r->count, dtok, drep, nullptr), "k_ring_route"))
    return rc;
  if (tokens) HIP_TRY(hipMemcpy(tokens, dtok, r->count * 4, hipMemcpyDefault));
  if (replicas) HIP_TRY(hipMemcpy(replicas, drep, r->count * rv.rf * 4, hipMemcpyDefault));
  return CB_OK;
}

// Compaction's steps with the ownership filter behind the select: k_ring_keep
// clears the survivors the node does not own, k_compact_lww_tiles takes the
// tile sums again, and the totals, the format and the finish are compaction's.
// The rules travel in a block of the call's, uploaded in front of the filter:
// the wait for the totals covers the copy (the source is pageable).
int cb_tables_compact_ring(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, const void* ring, uint32_t node,
                           uint32_t ranks, const void* rules, int lww, int drop_dead, void* stream,
                           cb_table** table_out, cb_filter** bloom_out) {
  if (!table_out) return fail(CB_EINVAL, "null argument");
  *table_out = nullptr;
  if (bloom_out) *bloom_out = nullptr;
  const Ring* rg = (const Ring*)ring;
  if (!rg) return fail(CB_EINVAL, "null ring");
  if (node >= rg->host.nnodes) return fail(CB_EINVAL, "the node is not a node of the ring");
  if (ranks > cb::kRingMaxRf) return fail(CB_EINVAL, "ranks is at most 16");
  auto kr = std::make_unique<cb::KeyRules>();
  if (int rc = take_rules(rules, kr.get())) return rc;
  if (int rc = zero_m_before_tables(m_bits, table_out, bloom_out)) return rc;
  const uint32_t rf = rg->host.rf, first_ranks = ranks && ranks < rf ? ranks : rf;
  int dev = 0;
  if (int rc = check_table_list(tables, nt, &dev)) return rc;
  DeviceGuard dg(dev);  // (blk is released on the tables' device)
  TempBlock blk{dev};
  bool uploading = false;  // the rules' copy was enqueued: `kr` is read until the next wait
  const AfterSelect keep = [&](const Merge& mg, hipStream_t s) -> int {
    if (!kr->np) return CB_OK;  // no prefix: every entry is every node's, and compaction's launches are the call's
    cb::RingView rv;
    if (int rc = ring_on_device(rg, dev, s, &rv)) return rc;
    cb::Carver c;
    const size_t o_kr = c.take(sizeof(cb::KeyRules));
    if (int rc = blk.alloc(c, "device allocation failed for a compaction's key rules")) return rc;
    uploading = true;
    HIP_TRY(hipMemcpyAsync(blk.at(o_kr), kr.get(), sizeof(cb::KeyRules), hipMemcpyHostToDevice, s));
    if (int rc = launch_try(cb::launch_ring_keep(rv, (const cb::KeyRules*)blk.at(o_kr), node, first_ranks, mg.order,
                                                 mg.side, mg.n, mg.slen, s),
                            "k_ring_keep"))
      return rc;
    HIP_TRY(cb::launch_compact_tiles(mg.order, mg.side, mg.slen, mg.n, mg.tcnt, mg.tbytes, mg.tkeys, s));
    return CB_OK;
  };
  const MergeRule rule{lww ? MergeOrder::lww : MergeOrder::newest, drop_dead != 0};
  const int rc = compact_tables(tables, nt, m_bits, rule, &keep, stream, table_out, bloom_out);
  if (rc && uploading) (void)hipStreamSynchronize((hipStream_t)stream);  // (a refusal before the totals' wait)
  return rc;
}

}  // extern "C"
