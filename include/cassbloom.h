/*
 * cassbloom.h — C ABI of the MI355X-native Bloom-filter path for the `cass`
 * LSM store (mweiden/lsmt). Drop-in for /root/reference/src/bloom.rs.
 *
 * Every entry point is plain C: opaque handles, pointers and sizes; no HIP,
 * torch or C++ types. Streams are passed as `void*` (a hipStream_t; NULL = the
 * device's null stream). Return value: CB_OK (0) or a negative CB_E* code;
 * cb_last_error() gives a thread-local message for the last failure.
 *
 * Bit layout of a device filter (the "packed" form): bit p of the reference's
 * Vec<bool> lives in 32-bit word p>>5 at bit p&31 (LSB-first), i.e. byte p>>3
 * bit p&7 — little-endian packbits(bitorder="little") of the bool array.
 *
 * Pointer residency: key, offset and hit buffers may be device memory
 * (hipMalloc / torch) or host memory (pageable or pinned). Device buffers are
 * used in place and the call is asynchronous on `stream`. Host buffers are
 * staged through library-owned device buffers and the call synchronises the
 * stream before returning, so host outputs are valid on return.
 *
 * Reference interface replaced by each entry point (file:line in
 * /root/reference):
 *   cb_filter_create        BloomFilter::new(size)               src/bloom.rs:17-21
 *   cb_filter_insert_*      BloomFilter::insert(&mut, &str)      src/bloom.rs:40-44
 *                           batched over SsTable::create's loop  src/sstable.rs:62-65
 *                           and SsTable::load's rebuild loop     src/sstable.rs:113-119
 *   cb_probe_*              BloomFilter::may_contain(&, &str)    src/bloom.rs:48-51
 *                           batched over Database::get's fan-out src/lib.rs:129-134
 *   cb_may_contain          BloomFilter::may_contain (one key)   src/bloom.rs:48-51
 *   cb_filter_export_bools  BloomFilter::to_proto (bits clone)   src/bloom.rs:54-58
 *   cb_filter_import_bools  BloomFilter::from_proto              src/bloom.rs:61-63
 *   cb_filter_to_bytes      BloomFilter::to_bytes (prost)        src/bloom.rs:66-70
 *   cb_filter_from_bytes    BloomFilter::from_bytes (prost)      src/bloom.rs:74-77
 *   cb_filter_destroy       Drop for BloomFilter (Vec<bool> free)
 *
 * Error behaviour mirrors the reference's panics as codes: inserting into or
 * probing an m == 0 filter returns CB_EZEROM (`h % 0` panics at
 * src/bloom.rs:36); malformed proto bytes return CB_EDECODE (`unwrap()` panics
 * at src/bloom.rs:75). A Rust shim turns both back into panics.
 *
 * Threading: probes are reentrant and read-only on filters (the reference's
 * concurrent `&self` readers under sstables.read(), src/lib.rs:129). Inserts
 * need exclusive access to the target filter (the reference's `&mut self`).
 */
#ifndef CASSBLOOM_H
#define CASSBLOOM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CB_OK 0
#define CB_EINVAL (-1)  /* bad argument (null pointer, bad offsets, ...) */
#define CB_EZEROM (-2)  /* m == 0: the reference panics with `% 0` */
#define CB_ENOMEM (-3)  /* device or host allocation failed */
#define CB_EHIP (-4)    /* HIP runtime error */
#define CB_EDECODE (-5) /* malformed BloomProto bytes */
#define CB_ENODEV (-6)  /* no usable gfx950 device */
#define CB_EUTF8 (-7)   /* a data-file key is not UTF-8: SsTable::load returns Err */
#define CB_EBASE64 (-8) /* a log record's value is not STANDARD base64: Wal::new returns Err */

typedef struct cb_filter cb_filter;
typedef struct cb_filterset cb_filterset; /* bit-sliced filter sets, see below */
typedef struct cb_table cb_table;         /* an SSTable data file in HBM, see below */

/* ---- device / library ---- */
int cb_init(int device);
int cb_device_count(int* out);
const char* cb_last_error(void);
const char* cb_version(void);
int cb_stream_synchronize(void* stream);
/* The caller is done with `stream` (call before hipStreamDestroy, with no
 * library call on it in flight): waits for the stream's queued work, frees
 * the per-stream buffers the library keeps for it (keys staging, partition
 * scratch, search outputs) and forgets it. Destroying handles never waits for
 * the device: a filter, table or set's memory is retired behind an event on
 * every stream the library has seen and reused once they have all passed
 * them, so a stream destroyed without this call makes the next destroy fall
 * back to a device-wide synchronise. Ends no work of the caller's. */
int cb_stream_release(void* stream);
/* Pinned (page-locked, device-mapped) host memory for key and hit buffers:
 * FilterSet probes whose keys AND hits live in it run zero-copy (see
 * cb_set_probe_fixed). For callers without the HIP runtime (the Rust shim,
 * INTEGRATION.md §4). */
int cb_host_alloc(uint64_t bytes, void** out);
int cb_host_free(void* p);

/* ---- filter lifetime (BloomFilter::new / Drop) ---- */
/* m_bits may be 0 (legal in the reference; inserts/probes then fail with
 * CB_EZEROM). The filter starts all-zero. */
int cb_filter_create(uint64_t m_bits, int device, cb_filter** out);
int cb_filter_destroy(cb_filter* f);
int cb_filter_bits(const cb_filter* f, uint64_t* m_out);
int cb_filter_device(const cb_filter* f, int* device_out);
/* Device pointer to the packed words (ceil(m/32) uint32 LSB-first, padded
 * with zero words to the allocation). Read-only use by callers. */
int cb_filter_words(const cb_filter* f, const uint32_t** words_out, uint64_t* nwords_out);
int cb_filter_clear(cb_filter* f, void* stream);

/* ---- build (BloomFilter::insert, batched) ---- */
/* n keys of key_len bytes each, contiguous. key_len may be 0. */
int cb_filter_insert_fixed(cb_filter* f, const uint8_t* keys, uint32_t key_len, uint64_t n,
                           void* stream);
/* n ragged keys: key i is bytes[offsets[i] .. offsets[i+1]) (offsets: n+1
 * non-decreasing uint64). */
int cb_filter_insert_var(cb_filter* f, const uint8_t* bytes, const uint64_t* offsets,
                         uint64_t n, void* stream);

/* Concurrent flush builds: filters[i] += keys[i][0 .. n[i]) (key_len bytes
 * each), all filters of one m on one device, built together (one partition
 * and one tile launch per 64 filters). Each keys[i] may be host or device. */
int cb_filter_insert_fixed_many(cb_filter* const* filters, uint32_t nf, const uint8_t* const* keys,
                                uint32_t key_len, const uint64_t* n, void* stream);

/* ---- probe (BloomFilter::may_contain over many filters, batched) ---- */
/* hits: [nf][ceil(n/64)] uint64; bit k%64 of word [f][k/64] is
 * filters[f].may_contain(key k). Tail bits of the last word are zero. Filters
 * may have different m; all must live on the same device. */
int cb_probe_fixed(const cb_filter* const* filters, uint32_t nf, const uint8_t* keys,
                   uint32_t key_len, uint64_t n, uint64_t* hits, void* stream);
int cb_probe_var(const cb_filter* const* filters, uint32_t nf, const uint8_t* bytes,
                 const uint64_t* offsets, uint64_t n, uint64_t* hits, void* stream);
/* Single-key may_contain (host key, synchronous). *out = 0/1. The per-key
 * call of SsTable::get (src/sstable.rs:138) answers from a host mirror of the
 * filter's packed words when the mirror is on: the first call after a write
 * (build, import, clear) waits for that write's stream position and copies
 * ceil(m/32) words back once; later calls are two host word loads, no GPU
 * round trip. With the mirror off every call is a one-key GPU probe.
 * Reentrant: concurrent callers may share a filter (`&self`). */
int cb_may_contain(const cb_filter* f, const uint8_t* key, uint64_t len, int* out);
/* Host mirror policy: 1 on, 0 off, -1 auto (the default: on when m <= 2^24,
 * i.e. up to 2 MiB of host words). With the mirror on every write records an
 * event and the first refresh waits for it. A write made with the mirror off
 * records nothing (it costs the write's stream no event); the first refresh
 * after the mirror is turned on then waits, by events, for the work queued
 * on every stream the library has seen on the device: never for a stored
 * stream handle and never for the whole device, unless such a stream was
 * destroyed without cb_stream_release (then its handle is invalid and the
 * refresh synchronises the device). */
int cb_filter_host_mirror(cb_filter* f, int mode);
/* *on = whether cb_may_contain uses the mirror; *current = whether the mirror
 * already holds the latest write (either may be NULL). Host only. */
int cb_filter_host_mirror_info(const cb_filter* f, int* on, int* current);

/* ---- persistence (to_proto / from_proto / to_bytes / from_bytes) ---- */
/* Vec<bool> layout: m bytes of 0/1. */
int cb_filter_export_bools(const cb_filter* f, uint8_t* out, void* stream);
/* Replaces the filter's contents; m must equal the filter's m. */
int cb_filter_import_bools(cb_filter* f, const uint8_t* in, uint64_t m, void* stream);
/* Packed layout: ceil(m/32) uint32 words (bits >= m in the last word are 0). */
int cb_filter_export_packed(const cb_filter* f, uint32_t* out, void* stream);
int cb_filter_import_packed(cb_filter* f, const uint32_t* in, uint64_t nwords, void* stream);
/* prost encoding of `BloomProto { repeated bool bits = 1; }` (packed): the
 * exact bytes of BloomFilter::to_bytes. Writes at most `cap` bytes; *len_out
 * always receives the full length (call with out=NULL, cap=0 to size). */
int cb_filter_to_bytes(const cb_filter* f, uint8_t* out, uint64_t cap, uint64_t* len_out);
/* BloomFilter::from_bytes: decodes (packed or unpacked elements, unknown
 * fields skipped) into a new filter on `device`. */
int cb_filter_from_bytes(const uint8_t* in, uint64_t len, int device, cb_filter** out);

/* ---- TableMeta: the SSTable `.meta` file ----
 *   message TableMeta { optional BloomProto bloom = 1;          src/sstable.rs:31-37
 *                       optional ZoneMapProto zone_map = 2; }
 *   message ZoneMapProto { optional string min = 1; optional string max = 2; }
 *                                                               src/zonemap.rs:11-17 */
typedef struct cb_zone_bounds {
  const uint8_t* min;
  uint64_t min_len;
  int has_min; /* 0: None */
  const uint8_t* max;
  uint64_t max_len;
  int has_max;
} cb_zone_bounds;
typedef struct cb_meta_info {
  int has_bloom; /* 0: no bloom field; the returned filter is BloomFilter::new(1024) */
  int has_zone;  /* 0: no zone_map field (ZoneMap::default()) */
  cb_zone_bounds zone; /* min/max point INTO the decoded input buffer */
} cb_meta_info;
/* TableMeta{bloom, zone_map}.encode (SsTable::create, src/sstable.rs:74-81).
 * bloom NULL / zone NULL omit that field. The filter's bits are expanded to
 * the prost 0/1 bytes on the device. out may be host or device memory;
 * *len_out is always the encoded length, bytes are written only if cap
 * suffices. CB_EINVAL if a zone bound is not UTF-8. */
int cb_meta_encode(const cb_filter* bloom, const cb_zone_bounds* zone, uint8_t* out, uint64_t cap,
                   uint64_t* len_out);
/* TableMeta::decode + the map()s of SsTable::load (src/sstable.rs:96-108):
 * prost merge semantics (repeated bloom fields append bits, zone strings are
 * last-wins, unknown fields skipped, strings must be UTF-8). CB_EDECODE on a
 * malformed message — the reference then rebuilds from the data file
 * (src/sstable.rs:109-120). The new filter lives on `device`. */
int cb_meta_decode(const uint8_t* in, uint64_t len, int device, cb_filter** bloom_out,
                   cb_meta_info* info);
/* Restart path for a set: decode one table's `.meta` straight into `slot`
 * (filter bits and zone map). The table's m must equal the set's m. */
int cb_set_load_meta(cb_filterset* set, uint32_t slot, const uint8_t* in, uint64_t len,
                     void* stream);

/* ---- bit-sliced filter sets (the read-path fan-out) ---- */
/* A FilterSet holds up to `width` filters of one size m in a position-major
 * layout: word p (uint32 / uint64) has bit s = bit p of the filter in slot s.
 * Probing it answers may_contain for every slot with two word reads per key
 * (Database::get's per-table loop, src/lib.rs:129-134, collapsed; m is
 * uniform across SSTables, src/sstable.rs:44,59). The set is a derived copy:
 * the cb_filter handles stay the source of truth.
 * width is 32, 64, or a multiple of 64 up to 4096 (a "wide" set: row p is
 * width/64 uint64 words, 128 B per row at 1024 slots; at the product's
 * m = 1024 the whole set is 128 KiB). A wide set serves the reference's
 * real shape — a table per 1024 inserts (src/lib.rs:72,105), hundreds of
 * m = 1024 filters — in one launch: cb_set_get_many_* take up to `width`
 * tables. Its probe reads row b's word only where row a's is non-zero (the
 * reference's `&&`, src/bloom.rs:50). cb_set_probe_pack_fixed takes sets of
 * at most 64 slots; cb_set_probe_allgather_fixed takes wide sets when every
 * rank's shard is past 64 rows (below). */
int cb_set_create(uint64_t m_bits, uint32_t width, int device, cb_filterset** out);
int cb_set_destroy(cb_filterset* set);
/* used = 1 + the highest slot assigned so far (the number of hit rows). */
int cb_set_info(const cb_filterset* set, uint64_t* m_out, uint32_t* width_out, uint32_t* used_out);
/* slot := f's bits (f->m must equal the set's m). O(set bits) when the slot is
 * empty (the LSM case: a new SSTable takes a free slot), a full pass otherwise. */
int cb_set_assign(cb_filterset* set, uint32_t slot, const cb_filter* f, void* stream);
/* slots 0..nf-1 := filters[0..nf-1], other slots cleared; used = nf. */
int cb_set_assign_all(cb_filterset* set, const cb_filter* const* filters, uint32_t nf, void* stream);
int cb_set_clear_slot(cb_filterset* set, uint32_t slot, void* stream);
/* hits: [used][ceil(n/64)] uint64, row s = slot s's may_contain bits.
 * Pinned host keys AND hits (hipHostMalloc / torch pin_memory) of fixed-length
 * keys take the zero-copy path: the probe kernel loads the keys and stores the
 * hit rows over PCIe itself (both directions and the HBM gathers overlap in one
 * launch); the call returns when the hits are in host memory. */
int cb_set_probe_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n,
                       uint64_t* hits, void* stream);
int cb_set_probe_var(const cb_filterset* set, const uint8_t* bytes, const uint64_t* offsets,
                     uint64_t n, uint64_t* hits, void* stream);

/* ---- zone maps and the SsTable::get gate ----
 * Each slot may carry its table's ZoneMap (src/zonemap.rs:3-8: optional
 * min/max key, compared byte-wise like Rust's str Ord). A slot whose zone
 * lacks either bound accepts every key (zonemap.rs:37-42). cb_set_assign,
 * cb_set_assign_all and cb_set_clear_slot reset the slot's zone to "none";
 * set the zone after assigning the table's filter. Zone updates wait for
 * `stream` (they happen once per flush). */
/* The slot's zone := {min, max} — ZoneMap::from_proto (zonemap.rs:55-61). */
int cb_set_zone(cb_filterset* set, uint32_t slot, const uint8_t* min, uint64_t min_len,
                int has_min, const uint8_t* max, uint64_t max_len, int has_max, void* stream);
/* Reads the slot's zone back (to_proto, zonemap.rs:46-52). Bytes are copied
 * only when the buffer is large enough; lengths are always written. */
int cb_set_zone_get(const cb_filterset* set, uint32_t slot, uint8_t* min, uint64_t min_cap,
                    uint64_t* min_len, int* has_min, uint8_t* max, uint64_t max_cap,
                    uint64_t* max_len, int* has_max);
/* ZoneMap::update for every key of a batch, on the device (the zone half of
 * SsTable::create's loop, src/sstable.rs:62-65). n == 0 leaves it as is. */
int cb_set_zone_from_keys_fixed(cb_filterset* set, uint32_t slot, const uint8_t* keys,
                                uint32_t key_len, uint64_t n, void* stream);
int cb_set_zone_from_keys_var(cb_filterset* set, uint32_t slot, const uint8_t* bytes,
                              const uint64_t* offsets, uint64_t n, void* stream);
/* Index of the first lexicographically smallest / largest key of a batch
 * (UINT64_MAX when n == 0). */
int cb_zone_bounds_fixed(const uint8_t* keys, uint32_t key_len, uint64_t n, int device,
                         uint64_t* min_idx, uint64_t* max_idx, void* stream);
int cb_zone_bounds_var(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, int device,
                       uint64_t* min_idx, uint64_t* max_idx, void* stream);
/* SsTable::get's gate for every (key, slot): bit set iff
 * zone_map.contains(key) && bloom.may_contain(key) (src/sstable.rs:138).
 * Same hits layout as cb_set_probe_*. */
int cb_set_probe_gated_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len,
                             uint64_t n, uint64_t* hits, void* stream);
int cb_set_probe_gated_var(const cb_filterset* set, const uint8_t* bytes, const uint64_t* offsets,
                           uint64_t n, uint64_t* hits, void* stream);

/* ---- SSTable data files and the batched read path ----
 * A data file is SsTable::create's output (src/sstable.rs:57-72): lines
 * `key \t base64(value) \n` sorted by key. cb_table_create uploads one (host
 * or device bytes) and indexes its lines on the device exactly as SsTable::get
 * splits them (raw.split('\n') minus empty lines, src/sstable.rs:142-146). */
int cb_table_create(const uint8_t* data, uint64_t len, int device, void* stream, cb_table** out);
int cb_table_destroy(cb_table* t);
/* Device pointer to the file bytes (valid until cb_table_destroy) and length. */
int cb_table_data(const cb_table* t, const uint8_t** data, uint64_t* len);
/* Copies file bytes [offset, offset+len) to out (host or device), synchronous:
 * what storage.put(&path, data) writes (src/sstable.rs:73). */
int cb_table_copy(const cb_table* t, uint64_t offset, uint64_t len, uint8_t* out);
/* SsTable::create (src/sstable.rs:51-87) on the device, for n entries given as
 * ragged key and value arrays (host or device): stable sort by key (skipped
 * when already sorted, as memtable flushes are), the data file `key \t
 * STANDARD.encode(value) \n` (*table_out, indexed and searchable), the
 * table's Bloom filter of m_bits (*bloom_out, nullable: BloomFilter::new(1024)
 * + insert per key in the reference) and its zone map as the input indices of
 * a smallest and a largest key (UINT64_MAX when n == 0).
 * The call only ENQUEUES its work on `stream` (the device decides whether the
 * batch needs a sort) and returns; the table finalises on first use — every
 * call that reads it (cb_table_*, searches, get_many, cb_table_wait) first
 * waits for the work and takes its results once. zone_min_idx / zone_max_idx
 * non-NULL are host results: the call then waits itself. Device offsets cost
 * one read-back of their totals (cb_sstable_create_bounded takes bounds
 * instead). Host inputs are staged into memory the table owns; device inputs
 * must stay valid until the table is finalised (a batch the bin sort cannot
 * place — keys sharing long prefixes — is sorted again from them then). */
int cb_sstable_create(const uint8_t* keys, const uint64_t* key_off, const uint8_t* vals,
                      const uint64_t* val_off, uint64_t n, uint64_t m_bits, int device, void* stream,
                      cb_table** table_out, cb_filter** bloom_out, uint64_t* zone_min_idx,
                      uint64_t* zone_max_idx);
/* The same, enqueue-only for device offsets too: key_bytes / val_bytes bound
 * key_off[n] / val_off[n] (the file buffer is sized from them). A batch past
 * its bounds writes no file; its table reports CB_EINVAL when finalised, and
 * the Bloom filter returned with it must be discarded (device offsets past a
 * device buffer's end are the caller's error, as for any device pointer).
 * Host key or value bytes with device offsets are checked before the call
 * returns (one read-back of the offsets' totals): the bytes are staged into a
 * block of exactly key_bytes / val_bytes, so a batch past them is refused
 * with CB_EINVAL and nothing is enqueued. */
int cb_sstable_create_bounded(const uint8_t* keys, const uint64_t* key_off, uint64_t key_bytes, const uint8_t* vals,
                              const uint64_t* val_off, uint64_t val_bytes, uint64_t n, uint64_t m_bits, int device,
                              void* stream, cb_table** table_out, cb_filter** bloom_out);
/* Compaction: the newest-wins merge of nt tables into one, on the device.
 * The reference never merges its tables (every flush pushes one more onto
 * Database::sstables and get walks them all, src/lib.rs:128-134), so the
 * result is defined through the two reference functions it must be
 * indistinguishable from. With tables[0] the NEWEST (cb_get_many_*'s order)
 * and K the keys of all their lines, the new data file is, byte for byte,
 *   SsTable::create(entries)   (src/sstable.rs:51-87)
 *   entries = { (k, Database::get(k)) : k in K, Database::get(k) is Some }
 * with Database::get taken over these tables alone. So: a key present in
 * several tables keeps the line of the newest one; a line whose value
 * STANDARD.decode rejects is an Err the walk falls through (src/lib.rs:131,
 * src/sstable.rs:147-149), so the kept line is the newest whose value decodes
 * and a key whose value decodes nowhere is dropped (get returns None for it
 * before and after); lines are `key \t text \n` sorted by key bytes, every
 * one ending in '\n', the value text copied (for a decodable text
 * STANDARD.encode(decode(text)) == text). *bloom_out (nullable) is
 * BloomFilter::new(m_bits) plus an insert per kept key; the zone map is the
 * first and last kept key (cb_table_zone); cb_meta_encode gives the `.meta`.
 * All tables on one device; inputs still pending from cb_sstable_create are
 * finalised first; inputs are not modified, stay valid and are the caller's to
 * destroy — the output owns all its memory, so they may be destroyed as soon
 * as the call returns. CB_EINVAL (nothing returned): nt == 0, a null entry,
 * tables on different devices, an input with lines that is not well-formed
 * (cb_table_well_formed), 2^32 or more lines in all. CB_EZEROM: m_bits == 0
 * with bloom_out non-NULL. The returned table behaves as one made by
 * cb_sstable_create (already finalised); a result without lines is a table of
 * length 0 (cb_table_zone: CB_EINVAL, as for n == 0). The call waits for its
 * own stream (the output's size depends on the data), never for the device. */
int cb_tables_compact(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, void* stream,
                      cb_table** table_out, cb_filter** bloom_out /* nullable */);

/* ---- range and prefix scans over tables ------------------------------------
 * The reference scans its memtable alone (Database::scan / scan_ns,
 * src/lib.rs:144-146, 178-186): rows drop out of every scan and count once
 * their memtable is flushed, while get still finds them. The scan of the
 * tables is therefore defined as compaction is, through the reference
 * functions it must be indistinguishable from. With tables[0] the NEWEST
 * (cb_get_many_*'s order), K the keys of all their lines and a byte range
 * [lo, hi), the result is, sorted ascending by key bytes (Rust's str Ord),
 *   { (k, Database::get(k)) : k in K, lo <= k, (no hi or k < hi),
 *                             Database::get(k) is Some }
 * with Database::get (src/lib.rs:128-134) taken over these tables alone: a
 * key keeps the value of the newest table whose line for it decodes, a key
 * whose value decodes nowhere is absent, and values are the decoded bytes.
 * With limit > 0 only the first `limit` entries are returned, and `truncated`
 * says whether more qualified (the whole range is still merged: the limit
 * bounds the result, not the work). The full range (lo_len == 0, has_hi == 0,
 * limit == 0) is entry for entry the lines of cb_tables_compact's file, with
 * the values decoded.
 * The scan covers the tables only: a store merges its memtable's own scan
 * over the result, memtable entries overriding, as it does for get.
 *
 * lo / hi: host bytes of any content (a prefix's end need not be UTF-8).
 * lo_len == 0: from the first key. has_hi == 0: unbounded above (hi is
 * ignored and may be NULL). lo >= hi: an empty result, not an error.
 * which[i] = the index into tables[] of the table that supplied entry i
 * (cb_get_many_*'s meaning). The inputs are not modified, inputs still
 * pending from cb_sstable_create are finalised first, and the result owns all
 * its memory, so the inputs may be destroyed as soon as the call returns.
 * The call waits for its own stream (the result's size depends on the data),
 * never for the device. CB_EINVAL (nothing returned, *out = NULL): out NULL,
 * nt == 0, a null entry, tables on different devices, an input with lines
 * that is not well-formed (cb_table_well_formed), lo or hi NULL with a
 * non-zero length, 2^32 or more lines inside the range in all. Tables
 * without lines are legal anywhere in the list. */
/* A scan's result lives in device memory behind an opaque handle. The handle
 * is spelled `void*` in these prototypes (cb_scan below is a name for it in
 * prose only): it is made by cb_tables_scan*, read by cb_scan_*, and freed by
 * cb_scan_destroy, and nothing else may be passed where one is expected. */
int cb_tables_scan(const cb_table* const* tables, uint32_t nt, const uint8_t* lo, uint64_t lo_len,
                   const uint8_t* hi, uint64_t hi_len, int has_hi, uint64_t limit, void* stream, void** out /* cb_scan */);
/* cb_tables_scan over [prefix, cb_key_prefix_end(prefix)): every key that
 * starts with prefix. Database::scan_ns(ns) is the prefix ns + ":"; stripping
 * it from the returned keys is the caller's (src/lib.rs:184). */
int cb_tables_scan_prefix(const cb_table* const* tables, uint32_t nt, const uint8_t* prefix, uint64_t prefix_len,
                          uint64_t limit, void* stream, void** out /* cb_scan */);
/* Many ranges in one call: the result holds the entries of
 * cb_tables_scan(tables, lo_r, hi_r, limit = 0) for r = 0, 1, ... one after the
 * other (keys, values and which exactly as those nr calls return them), from
 * one merge instead of nr, and cb_scan_ranges says where each range's entries
 * begin. The ranges must ascend and be pairwise disjoint, in Rust's `Ord for
 * [u8]` (bytes, then length): for every r < nr - 1, lo_r <= lo_{r+1} and
 * hi_r <= lo_{r+1}, and only the last range may be unbounded above. A range
 * with lo_r >= hi_r is legal and empty; touching ranges (hi_r == lo_{r+1}) are
 * legal, a key equal to that bound belonging to the later one. The whole
 * result is therefore sorted by key bytes too. Overlapping ranges, ranges in
 * descending order and nested prefixes ("a:" with "a:b:") are refused: every
 * range's cut of a table is one source of the one sort, a line inside two
 * ranges would stand in two sources, and the merge's select, which keeps one
 * line per run of equal keys, would fold the copies into one entry. Sorting
 * the ranges and splitting them at overlaps is the caller's.
 * There is no limit in this form (a per-range limit needs ranks within a
 * range, which the merge does not compute); cb_tables_scan keeps its limit.
 * ranges: range r = [ bounds[bound_off[2r] .. bound_off[2r+1]),
 *                     bounds[bound_off[2r+1] .. bound_off[2r+2]) );
 * bound_off: 2*nr+1 non-decreasing host uint64. last_unbounded != 0: the last
 * range has no upper bound (its hi bytes are ignored).
 * Everything else is as for cb_tables_scan. CB_EINVAL (nothing returned,
 * *out = NULL, nothing enqueued): out NULL, cb_tables_scan's table-list
 * errors, nr == 0, bound_off NULL, bounds NULL with a non-zero total,
 * bound_off that decreases, ranges that break the ordering rule, and more
 * than 65536 cuts (nr * the number of tables with lines: one block of the
 * device walks the cuts). */
int cb_tables_scan_many(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                        const uint64_t* bound_off, uint32_t nr, int last_unbounded,
                        void* stream, void** out /* cb_scan */);
/* cb_tables_scan_many over prefixes: prefix r = prefixes[prefix_off[r] ..
 * prefix_off[r+1]) (prefix_off: np+1 non-decreasing host uint64); range r =
 * [p_r, cb_key_prefix_end(p_r)). A prefix without an end (empty, all 0xFF) is
 * legal only as the last one. Database::scan_ns over many namespaces is the
 * prefixes ns_r + ":" in ascending order; a namespace that starts with
 * another's prefix ("a" and "a:b") nests and takes a call of its own. */
int cb_tables_scan_prefixes(const cb_table* const* tables, uint32_t nt, const uint8_t* prefixes,
                            const uint64_t* prefix_off, uint32_t np, void* stream, void** out /* cb_scan */);
/* ---- live rows: tombstones in the tables -----------------------------------
 * The reference deletes a row by writing a tombstone: exec_delete inserts the
 * 8-byte timestamp with an empty payload (src/query.rs:240-261), and every
 * reader of a scan (SELECT COUNT(*), the schema-less select, SHOW TABLES)
 * does `let (_, data) = split_ts(&bytes); if data.is_empty() { continue; }`
 * (src/query.rs:21-27, 343-346, 395-398). split_ts returns the bytes
 * themselves below 8 and strips 8 from there on, so a decoded value of length
 * L is DEAD exactly when L == 0 or L == 8. A value that does not decode is
 * neither live nor dead: such a line is no entry at all, as everywhere above.
 * A tombstone SHADOWS AND IS THEN DROPPED: Database::get stops at the newest
 * line that decodes, tombstone or not, so a key's fate is decided by that
 * line alone. If it is dead the key is absent from live results, even when
 * an older table holds a live value for it; no older value ever comes back.
 * The three entries below apply that rule to the tables; cb_tables_scan*,
 * cb_tables_compact and cb_get_many_* are unchanged and still return
 * tombstones as entries. The memtable's own tombstones are the store's, which
 * merges its memtable over these results as it does for get.
 * Range lists are cb_tables_scan_many's (bounds, bound_off, nr,
 * last_unbounded): the same format, ordering rule, cut cap and refusals; a
 * caller builds prefix bounds with cb_key_prefix_end. All three check their
 * own arguments (outputs, range list, limit, m_bits) before they look at the
 * table list, so with two errors at once they report the argument's. */
/* Counts without a result: entries[r] = the number of entries
 * cb_tables_scan(tables, lo_r, hi_r, limit = 0) returns, live[r] = how many of
 * them are not dead: SELECT COUNT(*) of a namespace (src/query.rs:341-357) is
 * live[r] for the prefix ns + ":". entries, live: host arrays of nr uint64,
 * either may be NULL, not both. The call runs the scan's cuts and merge up to
 * its select and then counts: it allocates no result, copies no key and
 * decodes no value. It waits for its own stream (one wait fewer than a
 * scan); the counts are complete on return. nr == 0 is legal and counts
 * nothing; no table with lines, or lo >= hi in every range: zeros, without
 * touching the device. CB_EINVAL: both arrays NULL (nothing written); else
 * the arrays are zeroed first and cb_tables_scan_many's refusals apply. */
int cb_tables_count(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                    const uint64_t* bound_off, uint32_t nr, int last_unbounded, void* stream,
                    uint64_t* entries /* nr, nullable */, uint64_t* live /* nr, nullable */);
/* cb_tables_scan_many's result without the dead entries (the cb_scan_*
 * accessors are unchanged; cb_scan_ranges' offsets count live entries).
 * limit > 0 is legal with nr == 1 only (CB_EINVAL otherwise): the first
 * `limit` live entries, `truncated` saying whether more live entries
 * qualified. Everything else, refusals included, as cb_tables_scan_many. */
int cb_tables_scan_live(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                        const uint64_t* bound_off, uint32_t nr, int last_unbounded, uint64_t limit,
                        void* stream, void** out /* cb_scan */);
/* cb_tables_compact's contract with the set narrowed to
 *   entries = { (k, Database::get(k)) : k in K, get(k) is Some and not dead }:
 * the file, line index, Bloom filter and zone bounds are exactly what
 * cb_tables_compact would produce from those entries; nothing live gives the
 * empty file. THE CALLER'S RULE: it is correct only when no older table of
 * the store stays outside the list (a full compaction). A dropped tombstone
 * can no longer shadow, so an older table left out would bring its deleted
 * rows back. The library cannot check this. Arguments, errors and waits as
 * cb_tables_compact; without tombstones in the inputs it does the same work. */
int cb_tables_compact_live(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, void* stream,
                           cb_table** table_out, cb_filter** bloom_out /* nullable */);
/* Where each range's entries lie: range r's are [range_off[r], range_off[r+1]),
 * range_off[0] = 0, range_off[nr] = count. range_off: nr+1 host uint64
 * (nullable); *nr (nullable) = the number of ranges. A result of
 * cb_tables_scan / _prefix reports nr = 1, {0, count}. Host only. */
int cb_scan_ranges(const void* r, uint64_t* nr, uint64_t* range_off);
/* Host only, no device: the exclusive upper bound of "starts with prefix",
 * i.e. the prefix without its trailing 0xFF bytes and its last remaining byte
 * incremented (*out_len <= len bytes into out). *has_end = 0, *out_len = 0
 * when nothing remains (an empty prefix, or all 0xFF): unbounded above. */
int cb_key_prefix_end(const uint8_t* prefix, uint64_t len, uint8_t* out /* len bytes */, uint64_t* out_len,
                      int* has_end);
/* Every output nullable. truncated: 1 only when limit > 0 and more than
 * limit entries qualified. */
int cb_scan_info(const void* r, uint64_t* count, uint64_t* key_bytes, uint64_t* val_bytes, int* truncated);
/* The result's parts, copied to host or device memory (as cb_table_lines
 * copies): entry i's key is keys[key_off[i] .. key_off[i + 1]), its value
 * vals[val_off[i] .. val_off[i + 1]). Either pointer of a pair may be NULL to
 * skip that part. Synchronous; may be called any number of times. */
int cb_scan_keys(const void* r, uint64_t* key_off /* count+1 */, uint8_t* keys);
int cb_scan_values(const void* r, uint64_t* val_off /* count+1 */, uint8_t* vals);
int cb_scan_which(const void* r, int32_t* which /* count */);
/* Retires the result's memory through the block pool, like every other
 * handle: no device-wide synchronise. */
int cb_scan_destroy(void* r);
/* ---- last-write-wins by row timestamp: tables as replicas --------------------
 * Every row the reference writes is stamped by its coordinator and stored as
 * 8 bytes of big-endian timestamp, then the payload (insert_ns_ts,
 * src/lib.rs:154-158); split_ts (src/query.rs:21-27) takes it off again:
 *   ts(value) = 0 when the decoded length is below 8, else the first 8
 *               decoded bytes as an unsigned big-endian u64.
 * Writes are forwarded with their timestamp, so a replica's arrival order,
 * and with it its table order, need not be timestamp order, and the cluster's
 * read reconciles by timestamp, not by position: it folds the replicas'
 * `key \t ts \t val` lines (exec_select_schema with meta, src/query.rs:393-410)
 * with "keep the current row if cur_ts >= ts, else replace"
 * (src/cluster.rs:405-416), and drops the rows whose val is empty only after
 * the fold (src/cluster.rs:454-459).
 * THE RULE. For tables T[0..nt), table r stands for replica r. Its answer for
 * key k is its line for k if that line's value decodes, else it has none (a
 * well-formed table has at most one line per key). The WINNER for k is the
 * answer with the greatest ts and, among equal ts, of the lowest table index;
 * a key without an answer has no winner and is absent. With drop_dead a
 * winner whose value is dead (the live-row section's rule: no payload) is
 * then absent too. It still defeated every line with ts <= its own, and a
 * tombstone that LOSES to a row with a newer ts deletes nothing, whichever
 * table is newer. That is the difference from the live-row entries above:
 * cb_tables_compact_live lets a tombstone in a newer table delete a row of an
 * older table even when the row's timestamp is the newer one; the entries
 * here do not. With timestamps that strictly descend in table order for every
 * key both rules choose the same lines.
 * THE CALLER'S RULE for drop_dead is cb_tables_compact_live's: dropping
 * winners is correct only when no table or replica of the store stays outside
 * the list; a tombstone that is dropped can no longer defeat an older row
 * held elsewhere. The library cannot check this.
 * The newest-wins entries above are unchanged. All three entries below check
 * their own arguments (outputs, range list, limit, m_bits) before they look
 * at the table list, and clear their outputs on every refusal. */
/* cb_tables_compact's contract with "newest decodable line" replaced by the
 * winner: the file is SsTable::create of { (k, winner(k)) }, with its line
 * index, Bloom filter and zone bounds; no winner at all gives the empty file.
 * Arguments, errors and waits as cb_tables_compact. Next to it the call reads
 * about 11 bytes and writes 8 per input line (the timestamps) and enqueues
 * two more launches. */
int cb_tables_compact_lww(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, int drop_dead,
                          void* stream, cb_table** table_out, cb_filter** bloom_out /* nullable */);
/* cb_tables_scan_live's call over the winners: range lists, the cut cap, the
 * refusals, "limit > 0 only with nr == 1" (`truncated` says whether more
 * winners qualified), the cb_scan_* accessors and cb_scan_ranges are the
 * same. which[i] = the winner's index in tables[]; cb_scan_ts gives its ts. */
int cb_tables_scan_lww(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                       const uint64_t* bound_off, uint32_t nr, int last_unbounded, int drop_dead,
                       uint64_t limit, void* stream, void** out /* cb_scan */);
/* cb_tables_count's contract over the winners: entries[r] = the winners in
 * range r (cb_tables_scan_lww's entries with drop_dead 0), live[r] = those of
 * them that are not dead (its entries with drop_dead 1). */
int cb_tables_count_lww(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                        const uint64_t* bound_off, uint32_t nr, int last_unbounded, void* stream,
                        uint64_t* entries /* winners */, uint64_t* live /* winners that are not dead */);
/* ts[i] = ts(value i) of a result of any cb_tables_scan* call: 0 for a value
 * below 8 bytes. ts: count uint64, host or device memory, as cb_scan_which
 * copies. Nothing is written for an empty result; a NULL ts returns CB_OK.
 * Synchronous. */
int cb_scan_ts(const void* r, uint64_t* ts /* count; host or device, as cb_scan_which */);
/* ---- rows WHERE column = value: the payload read on the device ----------------
 * SELECT COUNT(*) of a namespace is live[r] of cb_tables_count only without a
 * WHERE. With one the reference scans the namespace and, per row
 * (src/query.rs:309-362): takes the timestamp off the value (split_ts,
 * src/query.rs:21-27), skips a row without payload, parses the payload as a
 * JSON object of strings (decode_row, src/schema.rs:42-44: any error gives the
 * EMPTY map), overlays the key's `|`-separated parts as the key columns, and
 * compares every condition. The entries below apply that rule; its full text
 * (the JSON grammar accepted, escapes, UTF-8, duplicate keys) is
 * lsmt_amd/csrc/rowjson.hpp's, restated from serde_json's documented
 * behaviour and not run against it.
 * A predicate is nc conditions, ANDed: condition i is the column name
 * cols[col_off[i] .. col_off[i+1]), the value vals[val_off[i] .. val_off[i+1])
 * and part[i], the index of the key column the name is (the caller's schema:
 * key_columns()), or -1 for a column of the payload. A row's key parts are its
 * key without its first min(skip, len) bytes, split at every '|'. A row that
 * is not dead matches when for every i: if 0 <= part[i] < nparts, key part
 * part[i] equals the value bytewise (the payload is not consulted); else the
 * payload's map has the name and its last value equals the value bytewise
 * after unescaping (part[i] >= nparts falls back to the payload too). nc == 0:
 * every live row matches. A row whose conditions are all answered by its key
 * matches even when its payload is not JSON.
 * CB_EINVAL from all three entries, checked before the table list or result
 * is looked at, outputs cleared: w NULL; a NULL pointer next to a non-zero nc;
 * offsets that decrease; nc > 16; more than 4096 bytes of names and values
 * together; part[i] < -1 or > 255; a NULL `matched` / `flags` / `out`. Empty
 * names and empty values are legal. `w` is a const cb_where*. */
typedef struct cb_where {        /* host memory; conditions are ANDed */
  const uint8_t* cols; const uint64_t* col_off;  /* nc+1, non-decreasing */
  const uint8_t* vals; const uint64_t* val_off;  /* nc+1 */
  const int32_t* part;                            /* nc: key part index, or -1 */
  uint32_t nc;
} cb_where;
/* cb_tables_count's call (range lists, cut cap, refusals, one wait) with the
 * matching rows counted beside the live ones: live[r] is exactly
 * cb_tables_count's (lww != 0: cb_tables_count_lww's), matched[r] the number
 * of matching rows among them, the key parts of range r taken after skip[r]
 * bytes. The reference's COUNT(*) WHERE of namespace ns is the prefix
 * ns + ":" with skip = len(ns) + 1. No result is allocated and no value
 * decoded into memory: each surviving live line's value text is read in place. */
int cb_tables_count_where(const cb_table* const* tables, uint32_t nt, const uint8_t* bounds,
                          const uint64_t* bound_off, uint32_t nr, int last_unbounded,
                          const uint32_t* skip /* nr, nullable = zeros */, const void* w /* cb_where */, int lww,
                          void* stream, uint64_t* live /* nr, nullable */, uint64_t* matched /* nr */);
/* flags[i] = 1 when entry i of a result of any cb_tables_scan* call matches,
 * else 0 (dead entries: 0), over the decoded values the result holds; skip is
 * per range of the result (cb_scan_ranges). flags: count bytes, host or device
 * memory. Nothing is written for an empty result. Synchronous, as cb_scan_ts. */
int cb_scan_match(const void* r, const uint32_t* skip /* one per range of r, nullable */,
                  const void* w /* cb_where */, uint8_t* flags /* count; host or device, as cb_scan_which */);
/* Host only, no device: the rule for one row, e.g. a memtable row, which the
 * store merges over the tables' answer as it does for get. *out = 1 or 0. */
int cb_row_matches(const uint8_t* key, uint64_t key_len, uint32_t skip, const uint8_t* value,
                   uint64_t value_len, const void* w /* cb_where */, int* out);
/* ---- SELECT a, b: rows projected and re-encoded on the device ------------------
 * The other half of the SQL read path. For SELECT a, b FROM t WHERE pk IN (...)
 * the reference's exec_select_schema (src/query.rs:365-432) gets every key and,
 * per row: split_ts (src/query.rs:21-27); a row without payload is deleted
 * (src/query.rs:396-400); decode_row (src/schema.rs:42-44); the key's
 * `|`-separated parts laid over the map as the key columns
 * (src/query.rs:402-405); project_row with cast_simple (src/query.rs:641-662,
 * 817-827); encode_row (src/schema.rs:37-39); and joins the rows into the
 * response: a JSON array for a client (src/query.rs:411-431), `key\tts\tval`
 * lines for a coordinator (src/cluster.rs:404-421 parses and folds them). The
 * entries below write that response, byte for byte, from rows that are already
 * in device memory. The rule's full text (column lookup, the integer cast, the
 * escapes written) is lsmt_amd/csrc/rowselect.hpp's, over rowjson.hpp's
 * grammar; like it, a restatement that was not run against the reference.
 * A selection is nc <= 16 columns: column c's name cols[col_off[c] ..
 * col_off[c+1]) (at most 4096 bytes together; empty names are legal), part[c]
 * as in cb_where, cast[c] = 0 (none; Text, Varchar and Char too) or 1 (integer:
 * a value str::parse::<i64> accepts becomes its i64::to_string, any other stays
 * as it is). The names must ascend strictly, bytewise: that is the order a
 * BTreeMap writes them in, so nothing is sorted per row.
 * A row's column is its key part part[c] when 0 <= part[c] < nparts (the
 * payload is not consulted), else the last pair of that name in the payload's
 * map; a column without a value is left out, and a payload with an error
 * anywhere is the empty map. The row's object is {"name":"value",...} in
 * selection order, no spaces, strings escaped as serde_json writes them.
 * flags[i]: CB_ROW_TEXT the row has text; CB_ROW_DEAD; CB_ROW_ABSENT (which[i]
 * < 0); CB_ROW_BADJSON the payload is no valid map; CB_ROW_EXTRA a valid map
 * holds a name that is not in the selection. Every live row's payload is
 * parsed, so the last two are defined for every live row. SELECT * is exact
 * without a wildcard: pass all of the schema's columns; a row without
 * CB_ROW_EXTRA is then the reference's wildcard row, and the rows with it are
 * done again on the host from cb_scan_values.
 * CB_SELECT_JSON: a live row's text is its object, dead and absent rows have
 * none; the response is [ + the texts joined by , + ] and [] without any.
 * CB_SELECT_META: a live row's text is the key after skip, \t, ts in decimal,
 * \t, the object; a dead row's is key \t ts \t alone; absent rows have none;
 * the response is the texts joined by \n, no trailing newline, and no byte at
 * all without any (the reference's Ok(None)).
 * CB_EINVAL before any device work, *out = NULL: sel NULL; a NULL array next
 * to a non-zero count; offsets that decrease; nc > 16; more than 4096 bytes of
 * names; part[c] < -1 or > 255; cast[c] > 1; names that are not strictly
 * ascending; a mode other than 0 and 1; out NULL. `sel` is a const cb_select*. */
#define CB_SELECT_JSON 0
#define CB_SELECT_META 1
#define CB_ROW_TEXT 1
#define CB_ROW_DEAD 2
#define CB_ROW_ABSENT 4
#define CB_ROW_BADJSON 8
#define CB_ROW_EXTRA 16
typedef struct cb_select {       /* host memory */
  const uint8_t* cols; const uint64_t* col_off;  /* nc+1, non-decreasing */
  const int32_t* part;                            /* nc: key part index, or -1 */
  const uint8_t* cast;                            /* nc, nullable = zeros */
  uint32_t nc;
} cb_select;
/* The entries of a result of any cb_tables_scan* call, skip per range of the
 * result as in cb_scan_match. Synchronous, as cb_scan_match. An empty result
 * gives a valid object whose text is [] or empty. */
int cb_scan_select(const void* r, const uint32_t* skip /* one per range of r, nullable */,
                   const void* sel /* cb_select */, int mode, void** out /* cb_rows */);
/* Rows in DEVICE memory, e.g. what an enqueue-only cb_*get_many leaves (its
 * keys as a ragged batch, its which, val_off and vals): row i's key is
 * keys[key_off[i] .. key_off[i+1]), its value vals[val_off[i] ..
 * val_off[i+1]); which[i] < 0 (which nullable: all present) says there is no
 * row i. The work is enqueued on `stream`, behind whatever fills the buffers
 * there, and the call waits for it twice: for the text's total length, from
 * which the text is sized, and at the end, so the result is complete when the
 * call returns. Host pointers are refused (CB_EINVAL). n == 0 touches no
 * device. Two launches and a three-launch scan. */
int cb_rows_select(const uint8_t* keys, const uint64_t* key_off /* n+1 */, const int32_t* which /* n, nullable */,
                   const uint8_t* vals, const uint64_t* val_off /* n+1 */, uint64_t n, uint32_t skip,
                   const void* sel /* cb_select */, int mode, int device, void* stream, void** out /* cb_rows */);
/* Host only, no device: one row, e.g. a memtable row. *len = the length of the
 * row's text (0 without text), *flags (nullable) its flags; the text is
 * written to out when cap >= *len (call with out = NULL, cap = 0 to size). */
int cb_row_select(const uint8_t* key, uint64_t key_len, uint32_t skip, const uint8_t* value, uint64_t value_len,
                  const void* sel /* cb_select */, int mode, uint8_t* out, uint64_t cap, uint64_t* len,
                  uint8_t* flags);
/* Every output nullable: the rows, how many of them have text, the response's
 * bytes. Host only. */
int cb_rows_info(const void* rows, uint64_t* count, uint64_t* with_text, uint64_t* bytes);
/* The response (text, `bytes` of it) and, per row, where its text lies in it
 * (row_at, row_len: count uint64 each; row_len 0 without text) and its flags
 * (count bytes), each nullable, into host or device memory. Synchronous; may
 * be called any number of times. */
int cb_rows_text(const void* rows, uint8_t* text, uint64_t* row_at, uint64_t* row_len, uint8_t* flags);
/* Retires the result's memory through the block pool, as cb_scan_destroy. */
int cb_rows_destroy(void* rows);
/* ---- the token ring: which node holds which row ---------------------------------
 * The fold above treats tables as replicas; this is the rule that says which
 * node is a replica of which row. The reference places rows with a murmur3
 * token ring: Cluster::new (src/cluster.rs:46-54) inserts, for each node in
 * order and each v in 0 .. max(vnodes, 1), the position
 * (murmur3_32("{node}-{v}"), node) into a BTreeMap by token, a later insert
 * replacing an earlier one of the same token, and replicas_for
 * (src/cluster.rs:102-123) walks the positions with token >= t ascending, then
 * the whole ring from its first position, collecting the nodes not collected
 * yet until it holds rf = max(rf, 1) of them. It is asked about the partition
 * keys that SqlEngine::partition_keys cuts out of a statement
 * (src/query.rs:448-528, 697-713, 734-760). The rule's full text is
 * lsmt_amd/csrc/ring.hpp's; its hash is a restatement of MurmurHash3 x86_32
 * (seed 0) that was not run against the reference.
 * TOKEN of a byte string: MurmurHash3 x86_32, seed 0; bytes are unsigned.
 * PARTITION KEY of a stored key: rest = the key without its first
 * min(skip, len) bytes; with npk == 0, or when rest has at most npk
 * `|`-separated parts, all of rest; else rest up to, not including, its
 * npk-th `|` (the first npk parts joined again).
 * REPLICAS of token t: an ordered list, the primary first, of width =
 * min(rf, nodes that hold a position) node indices for every t. Lists are rf
 * wide, -1 past width. Nodes are 0 .. nnodes - 1 in the caller's order
 * (Cluster::new pushes the own node last).
 * A ring handle (`ring` below is a cb_ring, spelled void* as cb_scan is) is
 * immutable. Creating and asking it on the host touches no device; a device's
 * copy (the sorted tokens and each position's replica list) is made on that
 * device's first route or compaction. */
/* Cluster::new's ring: node i's name is names[name_off[i] .. name_off[i+1]).
 * CB_EINVAL, *out = NULL: a NULL argument; nnodes == 0 or > 4096; vnodes >
 * 4096; rf > 16; more than 2^20 positions; offsets that decrease; an empty
 * name; two equal names (replicas_for compares names: deduplicate first).
 * vnodes == 0 and rf == 0 act as 1. */
int cb_ring_create(const uint8_t* names, const uint64_t* name_off /* nnodes+1 */, uint32_t nnodes,
                   uint32_t vnodes, uint32_t rf, void** out /* cb_ring */);
/* The ring of explicit (tokens[i], owners[i]) pairs, inserted in order, a
 * later pair replacing an earlier one of the same token: for callers with
 * tokens of their own. CB_EINVAL as above, and for npos == 0 or > 2^20 and an
 * owner >= nnodes. */
int cb_ring_create_tokens(const uint32_t* tokens, const uint32_t* owners, uint64_t npos, uint32_t nnodes,
                          uint32_t rf, void** out /* cb_ring */);
/* Every output nullable. positions: the distinct tokens; width: as above. */
int cb_ring_info(const void* ring, uint32_t* nnodes, uint32_t* rf, uint64_t* positions, uint32_t* width);
/* The positions ascending by token, `positions` entries each (either nullable). */
int cb_ring_tokens(const void* ring, uint32_t* tokens, uint32_t* owners);
/* replicas_for of one key on the host: *token (nullable) the partition key's
 * token, replicas (nullable) its rf-wide list. */
int cb_ring_replicas(const void* ring, const uint8_t* key, uint64_t len, uint32_t skip, uint32_t npk,
                     uint32_t* token /* nullable */, int32_t* replicas /* rf, nullable */);
/* Retires the device copies through the block pool, like every other handle:
 * no device-wide synchronise. */
int cb_ring_destroy(void* ring);
/* The batched replicas_for on `device`: tokens[i] and replicas[i * rf ..] of
 * key i, for n keys with one skip and npk. Residency and waiting follow
 * cb_probe_*: device buffers are used in place and the call is asynchronous on
 * `stream`; host buffers are staged and the call waits. n == 0 writes nothing;
 * both outputs NULL is CB_EINVAL. */
int cb_ring_route_fixed(const void* ring, const uint8_t* keys, uint32_t key_len, uint64_t n, uint32_t skip,
                        uint32_t npk, int device, uint32_t* tokens /* n, nullable */,
                        int32_t* replicas /* n*rf, nullable */, void* stream);
int cb_ring_route_var(const void* ring, const uint8_t* bytes, const uint64_t* offsets /* n+1 */, uint64_t n,
                      uint32_t skip, uint32_t npk, int device, uint32_t* tokens /* n, nullable */,
                      int32_t* replicas /* n*rf, nullable */, void* stream);
/* The same over the keys of a result of any cb_tables_scan* call, skip and npk
 * per range of the result (cb_scan_ranges), as cb_scan_match takes its skip.
 * Synchronous; outputs to host or device memory, as cb_scan_which copies.
 * Nothing is written for an empty result. */
int cb_scan_route(const void* r /* cb_scan */, const void* ring, const uint32_t* skip /* per range, nullable */,
                  const uint32_t* npk /* per range, nullable */, uint32_t* tokens /* count, nullable */,
                  int32_t* replicas /* count*rf, nullable */);
/* Which keys are partitioned, and how: a key that starts with prefix r has
 * skip = len(prefix r) and npk[r]. The prefixes ascend and none starts with
 * another (cb_tables_scan_prefixes' ordering rule); at most 256 of them and
 * 4096 bytes together. np == 0 is legal. */
typedef struct cb_key_rules {   /* host memory */
  const uint8_t* prefixes; const uint64_t* prefix_off;   /* np+1, non-decreasing */
  const uint32_t* npk;                                   /* np */
  uint32_t np;
} cb_key_rules;
/* The compaction a node runs after the ring changed, or to cut what a joining
 * node must receive (Cassandra's cleanup; the reference never does it, as it
 * never compacts): the file is SsTable::create of { (k, v) in E : owned(k) }.
 * E is the entries of cb_tables_compact (lww == 0) or cb_tables_compact_lww
 * (lww != 0), drop_dead as in cb_tables_compact_live / _lww, and with it THE
 * CALLER'S RULE: dropping dead winners is correct only when
 * no table or replica of the store stays outside the list.
 * owned(k): a key under prefix r
 * of the rules is owned when `node` is among the first `ranks` entries of its
 * replica list (ranks == 0: all rf); a key under no prefix is owned by every
 * node, as the reference broadcasts its catalog writes to the whole ring
 * (src/cluster.rs:277-286, 313-314), so `_tables:` and `_schema:` rows stay
 * everywhere. Ownership depends on the key alone, so the filter runs behind
 * the merge's select: two more launches than the base entry. No owned entry
 * gives the empty file. Bloom filter, line index, zone bounds, waits and the
 * table-list refusals are cb_tables_compact's. Its own arguments are checked
 * before the table list, outputs cleared: a NULL table_out, ring or rules;
 * node >= nnodes; ranks > 16; rules that break the above; m_bits == 0 with a
 * filter asked for (CB_EZEROM). `rules` is a const cb_key_rules*. */
int cb_tables_compact_ring(const cb_table* const* tables, uint32_t nt, uint64_t m_bits, const void* ring,
                           uint32_t node, uint32_t ranks, const void* rules /* cb_key_rules */, int lww,
                           int drop_dead, void* stream, cb_table** table_out,
                           cb_filter** bloom_out /* nullable */);
/* Finalise a table from cb_sstable_create*: wait for its work, take its
 * results; returns its deferred error, if any. Idempotent, thread-safe. */
int cb_table_wait(const cb_table* t);
/* The zone map bounds of a table made by cb_sstable_create with n >= 1 (the
 * first / last key of the file: ZoneMap::update over the sorted entries,
 * src/sstable.rs:60-64): which = 0 min, 1 max. *len = the key's length; up to
 * cap bytes are copied to host memory out. Host only, no device access.
 * CB_EINVAL for other tables. */
int cb_table_zone(const cb_table* t, int which, uint8_t* out, uint64_t cap, uint64_t* len);
int cb_table_info(const cb_table* t, uint64_t* nlines, uint64_t* bytes);
/* SsTable::load's rebuild when the `.meta` file is missing or undecodable
 * (src/sstable.rs:109-120), on the device from the table's line index: a new
 * filter of m_bits (BloomFilter::new(1024) in the reference) holding the key
 * of every line that has a TAB (bytes before the first TAB; lines without one
 * are skipped), and the zone map over the same keys, returned as the line
 * indices of a smallest and a largest key (UINT64_MAX when no line has a
 * TAB; cb_table_lines + cb_table_copy give the bytes). CB_EUTF8 when a key is
 * not UTF-8 (the reference's load returns Err; nothing is returned then). */
int cb_table_rebuild(const cb_table* t, uint64_t m_bits, void* stream, cb_filter** bloom_out,
                     uint64_t* zone_min_line, uint64_t* zone_max_line);
/* *out = 1 when the file is well-formed (a TAB on every line, keys strictly
 * increasing — what SsTable::create writes): then any correct search gives
 * the reference's answer and the prefix/fence index is used; otherwise the
 * exact (lo+hi)/2 trajectory of src/sstable.rs:163-177 is replayed. */
int cb_table_well_formed(const cb_table* t, int* out);
/* Tests/bench: tables created while on != 0 always use the exact trajectory. */
int cb_table_force_exact(int on);
/* The read path's key buckets (136 B per line, rounded up to a power of two
 * lines: 64 MiB for 512K lines, 2.3 GiB for 2^24) are built for a table only
 * when they take at most max_bytes AND at most a quarter of the device memory
 * free when they are built; otherwise that table is searched without them
 * (same answers, ~20 % slower reads). max_bytes = 0 turns them off for tables
 * read from now on; the default is 1 GiB. Process-wide. */
int cb_table_bucket_limit(uint64_t max_bytes);
/* The line index: start offset, key length (bytes before the first TAB, or
 * UINT32_MAX when the line has none) and line length; host or device out. */
int cb_table_lines(const cb_table* t, uint64_t* start, uint32_t* key_len, uint32_t* line_len);
/* SsTable::binary_search (src/sstable.rs:161-179) for a key batch, same
 * (lo+hi)/2 trajectory: line_out[k] = matching line index or -1. */
int cb_table_search_fixed(const cb_table* t, const uint8_t* keys, uint32_t key_len, uint64_t n,
                          int64_t* line_out, void* stream);
int cb_table_search_var(const cb_table* t, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                        int64_t* line_out, void* stream);
/* Database::get's table walk (src/lib.rs:128-134) for a key batch.
 * tables[0] is the NEWEST table. hits (nullable): the per-table gate from a
 * (gated) probe, [rows][ceil(n/64)] with table t in row hit_rows[t] (hit_rows
 * NULL = row t); a table is searched for key k only where its bit is set.
 * which[k] = index of the first table whose SsTable::get returns Ok(Some) —
 * line found AND value decodes as base64 (base64 0.21.7 STANDARD; an Err
 * falls through to older tables) — or -1. val_off[n+1] = offsets of the
 * decoded values; *total = their byte count; the values are written to vals
 * only if cap >= *total (call with vals = NULL to size).
 * total = NULL: the call only enqueues the work on stream and returns without
 * waiting (keys, hits, which, val_off and vals must then be device memory;
 * val_off[n] holds the total once the stream has run, and vals is written
 * only if cap >= that total). Calls that repeat the same tables and hit_rows
 * upload nothing, so batches on two streams overlap. A well-formed table's
 * first get_many (this or cb_set_get_many) also enqueues the build of its key
 * buckets on that call's stream (device memory: 136 B per line, rounded up
 * to a power of two lines; freed with the table) when they fit the budget
 * set by cb_table_bucket_limit; later calls on any stream enqueue a wait for
 * that build (never a host wait) until it is seen complete. */
int cb_get_many_fixed(const cb_table* const* tables, uint32_t nt, const uint64_t* hits,
                      const uint32_t* hit_rows, const uint8_t* keys, uint32_t key_len, uint64_t n,
                      int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap,
                      uint64_t* total, void* stream);
int cb_get_many_var(const cb_table* const* tables, uint32_t nt, const uint64_t* hits,
                    const uint32_t* hit_rows, const uint8_t* bytes, const uint64_t* offsets,
                    uint64_t n, int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap,
                    uint64_t* total, void* stream);
/* Database::get in one launch (src/lib.rs:125-136 with SsTable::get's gate,
 * src/sstable.rs:138): the same walk and outputs as cb_get_many_*, with each
 * (key, table) gate — zone_map.contains && bloom.may_contain, exactly
 * cb_set_probe_gated_*'s bit — computed from the FilterSet inside the search
 * kernel instead of read from hit rows. Table t is set slot slots[t]
 * (slots NULL = slot t); nt <= the set's width (up to 4096 with a wide set;
 * runs of ascending or descending slots, e.g. slot = the table's position in
 * Vec<SsTable> walked newest first, take each group of 64 tables' gate from
 * one window of the set's rows, other mappings one bit per table); tables and
 * set on one device. Same async contract (total = NULL). */
int cb_set_get_many_fixed(const cb_filterset* set, const cb_table* const* tables, uint32_t nt,
                          const uint32_t* slots, const uint8_t* keys, uint32_t key_len, uint64_t n,
                          int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap, uint64_t* total,
                          void* stream);
int cb_set_get_many_var(const cb_filterset* set, const cb_table* const* tables, uint32_t nt,
                        const uint32_t* slots, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                        int32_t* which, uint64_t* val_off, uint8_t* vals, uint64_t cap, uint64_t* total,
                        void* stream);

/* ---- tiered filter sets: one gate and one fused get over mixed filter sizes ----
 * A FilterSet holds filters of one size m, which fits a store whose every
 * table is a 1024-entry flush behind BloomFilter::new(1024)
 * (src/sstable.rs:44,59). After cb_tables_compact a store also holds one or a
 * few large tables whose filter must be large to mean anything (110 808 keys
 * in 1024 bits is a saturated filter; cb_tables_compact takes m_bits for that
 * reason), in front of which sit the fresh small tables: mixed m is then the
 * normal case. These entries take an ordered table list (tables[0] the
 * newest) whose filters live in several FilterSets of different m, the
 * "tiers": table t's Bloom filter and zone map are slot slots[t] of
 * sets[tiers[t]]. The key is hashed once for all tiers.
 *
 * Gate: bit (key, t) is exactly what cb_set_probe_gated_* on sets[tiers[t]]
 * reports for slot slots[t] — zone_map.contains(key) && bloom.may_contain(key)
 * (src/sstable.rs:138) with that tier's m; gated == 0: may_contain alone.
 * hits is [nt][ceil(n/64)] uint64, row t = table t (table order, not slot
 * order), tail bits zero; host or device memory as for cb_set_probe_* (host
 * buffers are staged and the call synchronises). n == 0 writes nothing.
 *
 * Get: Database::get's newest-first walk (src/lib.rs:128-134) over those
 * gate bits in one launch, bit-identical in which / val_off / vals / *total
 * to cb_get_many_* fed the gate rows above; cb_set_get_many_*'s contract,
 * total = NULL (enqueue only, everything on the device) and the first-use
 * build of a table's key buckets included.
 *
 * Limits: 1 <= ns <= 8 sets of width 32 or 64 (no wide set), 1 <= nt <= 64,
 * tiers and slots non-NULL with tiers[t] < ns and slots[t] < that set's width,
 * all sets and tables on one device; anything else is CB_EINVAL with nothing
 * enqueued. A slot at or past a set's `used` reads as an empty filter (gate
 * bit 0); a set no table names is not read; a (tier, slot) pair may repeat.
 * A later cb_set_zone on any tier whose zone table the launch reads waits for
 * the launch, as after cb_set_get_many_*. */
int cb_tiers_probe_fixed(const cb_filterset* const* sets, uint32_t ns, const uint32_t* tiers,
                         const uint32_t* slots, uint32_t nt, const uint8_t* keys, uint32_t key_len,
                         uint64_t n, int gated, uint64_t* hits, void* stream);
int cb_tiers_probe_var(const cb_filterset* const* sets, uint32_t ns, const uint32_t* tiers,
                       const uint32_t* slots, uint32_t nt, const uint8_t* bytes, const uint64_t* offsets,
                       uint64_t n, int gated, uint64_t* hits, void* stream);
int cb_tiers_get_many_fixed(const cb_filterset* const* sets, uint32_t ns, const cb_table* const* tables,
                            uint32_t nt, const uint32_t* tiers, const uint32_t* slots,
                            const uint8_t* keys, uint32_t key_len, uint64_t n, int32_t* which,
                            uint64_t* val_off, uint8_t* vals, uint64_t cap, uint64_t* total, void* stream);
int cb_tiers_get_many_var(const cb_filterset* const* sets, uint32_t ns, const cb_table* const* tables,
                          uint32_t nt, const uint32_t* tiers, const uint32_t* slots, const uint8_t* bytes,
                          const uint64_t* offsets, uint64_t n, int32_t* which, uint64_t* val_off,
                          uint8_t* vals, uint64_t cap, uint64_t* total, void* stream);

/* ---- multi-GPU exchange ----
 * Each rank holds hit rows [rows][words] (uint64) for its filter subset; the
 * ranks all-gather them so every rank has the [total_rows][words] map that
 * Database::get's fan-out reads (src/lib.rs:129-134). At BASELINE densities
 * the rows are sparse, so a rank can ship the positions of its set bits:
 *   cb_hits_pack_words: size in uint32 of a pack for rows x words of hits and
 *     cap positions: 2 + cap + 2 * ceil(rows * words / 2048). Packs that are
 *     all-gathered must all have the size of the LARGEST shard's pack.
 *   cb_hits_compress: pack := {count, 0, positions[cap], directory}; position
 *     = row * words * 64 + bit; the rows are cut into blocks of 2048 words and
 *     directory entry b = {first slot, number} of block b's positions
 *     (ascending inside the block). One launch. count may exceed cap: the
 *     pack is then incomplete (which positions were kept is unspecified) and
 *     all ranks must fall back to the dense exchange.
 *     Requires rows * words * 64 < 2^32. Device pointers, async on stream.
 *   cb_hits_expand: full := the dense map holding the positions of packs[r]
 *     (nranks packs, all-gathered with the stride cb_hits_pack_words gives for
 *     the largest shard) at global row row_off[r] (host array, row_off[0] = 0,
 *     non-decreasing, nranks <= 64; rank r has rows up to row_off[r+1], the
 *     last up to total_rows); every word of full is written once. Bit-identical
 *     to the dense all-gather when no rank's count exceeds cap. A rank whose
 *     count exceeds cap contributes zeros and clears *ok (a device uint32, may
 *     be NULL): the overflow report is asynchronous, so the caller checks ok
 *     before using full and redoes that batch's exchange densely when it is 0. */
int cb_hits_pack_words(uint64_t rows, uint64_t words, uint64_t cap, uint64_t* out);
int cb_hits_compress(const uint64_t* hits, uint64_t rows, uint64_t words, uint32_t* pack,
                     uint64_t cap, void* stream);
int cb_hits_expand(const uint32_t* packs, uint32_t nranks, uint64_t cap, const uint64_t* row_off,
                   uint64_t words, uint64_t total_rows, uint64_t* full, uint32_t* ok, void* stream);

/* The whole exchange behind one call, over RCCL (one process per GPU, xGMI
 * between the GPUs of a node). Replaces the per-table loop of Database::get
 * (src/lib.rs:129-134) when the tables' filters are sharded over GPUs: the
 * table subset of rank r is rows [first_row, first_row + rows) of the global
 * map, as cb_comm_shard splits total_rows (contiguous, sizes differ by <= 1,
 * larger shards first).
 *   cb_comm_unique_id: rank 0 makes the 128-byte id and hands it to every
 *     rank by any channel (the Rust store: its own RPC; Python: the process
 *     group's broadcast).
 *   cb_comm_init: collective over the `world` ranks; binds to `device`. The
 *     calling thread's current device is left unchanged.
 *   cb_hits_allgather: collective. local = this rank's [rows][words] uint64
 *     hits (rows = its shard of total_rows), full = the [total_rows][words]
 *     map, both device memory on the communicator's device; async on stream.
 *     mode CB_XCHG_DENSE: one all-gather of the rows. CB_XCHG_SPARSE: compress
 *     -> all-gather of (2 + cap)-word packs -> expand (cap > 0, the same on
 *     every rank). With ok == NULL the gathered counts are read back (the
 *     stream is synchronised) and, if any rank's set bits exceed cap, every
 *     rank redoes the batch densely: full is always complete. With ok != NULL
 *     (a device uint32 holding 1) nothing is read back: ok is cleared when a
 *     rank overflowed, and the caller redoes that batch with CB_XCHG_DENSE.
 *     *sparse_used (nullable) = 1 when the map came from the packs.
 *   Exchanges on one communicator must be issued in the same order on every
 *   rank. They may come from several streams (pipelined batches): the
 *   library keeps a buffer set per stream and runs a communicator's
 *   collectives one after another in issue order (each waits for an event
 *   recorded after the previous one), so at most one collective of a
 *   communicator is in flight and no two communicators' collectives need to
 *   interleave. Use ONE communicator per rank. */
#define CB_COMM_ID_BYTES 128
#define CB_XCHG_DENSE 0
#define CB_XCHG_SPARSE 1
typedef struct cb_comm cb_comm;
int cb_comm_unique_id(uint8_t* id /* CB_COMM_ID_BYTES */);
int cb_comm_init(int rank, int world, const uint8_t* id, int device, cb_comm** out);
/* Two more transports under the same collectives (every host and device step
 * of cb_hits_allgather / cb_set_probe_allgather_fixed is shared; only the
 * all-gather of bytes differs):
 *   cb_comm_init_loopback: `world` ranks in ONE process on one device;
 *     ranks[r] (an array of world handles) is rank r's communicator. Each
 *     rank's collectives must be issued from its own host thread: a call
 *     returns once every rank has issued it. The all-gather is device copies
 *     between the ranks' buffers, ordered by events on each caller's stream.
 *     For tests of world > 1 on one GPU.
 *   cb_comm_init_host: the caller moves the bytes (its own RPC, MPI, gloo ...):
 *     the library synchronises the stream, copies this rank's `bytes` of send
 *     data to host memory, calls fn(user, send, recv, bytes) — fn must leave
 *     rank r's bytes at recv + r * bytes for every rank and return 0 — and
 *     copies recv back to the device. Not collective at init. */
typedef int (*cb_host_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes);
int cb_comm_init_loopback(int world, int device, cb_comm** ranks);
int cb_comm_init_host(int rank, int world, int device, cb_host_allgather_fn fn, void* user,
                      cb_comm** out);
int cb_comm_destroy(cb_comm* c);
/* Ends the communicator on this rank (ncclCommAbort for RCCL; a loopback
 * group wakes every rank): callable from any thread, also while another
 * thread is blocked inside a collective of c, which then returns an error.
 * Every later exchange on c fails with CB_EINVAL; cb_comm_destroy still
 * frees the handle. For a rank's watchdog: a peer that never joins a
 * collective would otherwise hold this rank forever. */
int cb_comm_abort(cb_comm* c);
int cb_comm_info(const cb_comm* c, int* rank, int* world, int* device);
int cb_comm_shard(uint64_t total_rows, int world, int rank, uint64_t* first_row, uint64_t* rows);
int cb_hits_allgather(cb_comm* c, const uint64_t* local, uint64_t rows, uint64_t words,
                      uint64_t total_rows, uint64_t* full, int mode, uint64_t cap, uint32_t* ok,
                      int* sparse_used, void* stream);

/* The probe and the exchange in one call: this rank's FilterSet probe (its
 * `used` slots must equal its shard of total_rows) of a device-resident batch
 * of fixed-length keys, writing local_hits ([used][ceil(n/64)], device), then
 * the all-gather into full. In sparse mode the probe kernel itself writes the
 * pack (no separate compress pass): positions as cb_hits_compress's, with
 * one directory entry per probe block of 16 hit words of every slot
 * (cb_set_pack_words). ok / sparse_used / overflow as cb_hits_allgather.
 * gated != 0 applies the zone gate (cb_set_probe_gated_fixed). When the
 * largest shard passes 64 rows (wide sets), sparse mode probes first and
 * then runs cb_hits_allgather's sparse exchange (a separate compress pass);
 * every rank must then hold such a shard, as the shard split guarantees. */
int cb_set_probe_allgather_fixed(cb_comm* c, const cb_filterset* set, const uint8_t* keys, uint32_t key_len,
                                 uint64_t n, int gated, uint64_t* local_hits, uint64_t total_rows,
                                 uint64_t* full, int mode, uint64_t cap, uint32_t* ok, int* sparse_used,
                                 void* stream);
/* Its pieces, for callers that move the packs themselves: the pack size for
 * a batch of n keys and cap positions (2 + cap + 2 * ceil(ceil(n/64)/16)
 * uint32); the probe writing hits and pack (device buffers, async); and the
 * expand of nranks such packs (all-gathered, each of cb_set_pack_words) into
 * the [total_rows][ceil(n/64)] map, rank r's rows starting at row_off[r]
 * (<= 64 rows per rank). A rank whose count exceeds cap clears *ok and
 * leaves its rows zero. */
int cb_set_pack_words(uint64_t n, uint64_t cap, uint64_t* out);
int cb_set_probe_pack_fixed(const cb_filterset* set, const uint8_t* keys, uint32_t key_len, uint64_t n, int gated,
                            uint64_t* hits, uint32_t* pack, uint64_t cap, void* stream);
int cb_hits_expand_set(const uint32_t* packs, uint32_t nranks, uint64_t cap, const uint64_t* row_off, uint64_t n,
                       uint64_t total_rows, uint64_t* full, uint32_t* ok, void* stream);

/* ---- the write-ahead log replayed on the device ---- */
/* What cb_log_replay saw of a log. lines counts the non-empty pieces of the
 * split on '\n', entries those of them with a TAB, keys the distinct keys
 * among the entries (the lines of the table). After CB_EUTF8 / CB_EBASE64
 * bad_line is the first failing piece's index among the non-empty pieces and
 * bad_offset its first byte's offset in the log (lines and entries then count
 * the whole log, keys is 0); UINT64_MAX otherwise. */
typedef struct {
    uint64_t lines;      /* non-empty pieces */
    uint64_t entries;    /* of those with a TAB */
    uint64_t keys;       /* distinct keys = lines of the table */
    uint64_t bad_line;   /* UINT64_MAX, or index among the non-empty pieces */
    uint64_t bad_offset; /* UINT64_MAX, or byte offset of that piece */
} cb_log_stats;
/* Database::new's replay of the write-ahead log (src/lib.rs:30-39: Wal::new's
 * parse_entries, src/wal.rs:14-31, then one memtable.insert per record in log
 * order) followed by the flush of that memtable (SsTable::create,
 * src/sstable.rs:51-87), on the device: the table holds one line per distinct
 * key, the LAST record of that key, sorted by key bytes. A record is what
 * insert_internal appends (src/lib.rs:96-102), `key \t STANDARD.encode(value)
 * \n`, byte for byte a table line, so its text is copied, never re-encoded.
 * The log is split on 0x0A; empty pieces are skipped, the last piece counts
 * without a final newline, and a non-empty piece without a TAB is skipped
 * whatever its bytes (parse_entries never looks at it). Of any other piece
 * the bytes before the first TAB are the key (it may be empty) and must be
 * UTF-8 by std::str::from_utf8, the bytes after it up to the piece's end the
 * value's text, which base64 0.21.7 STANDARD.decode must accept (empty text is
 * the empty value; a second TAB is part of the text and fails it). '\r' is a
 * byte like any other. The first failing piece in log order fails the call,
 * its key checked before its value (the `?` order of src/wal.rs:21-26):
 * CB_EUTF8 or CB_EBASE64 (tests/wal_error_test.rs:19), nothing is returned,
 * the outputs are cleared and *stats, when given, names the piece. The rule
 * is lsmt_amd/csrc/logline.hpp's. A last write that is a tombstone (8
 * timestamp bytes only) stays as a line, as it stays in the memtable.
 * log: host or device memory. *bloom_out (nullable): BloomFilter::new(m_bits)
 * with every kept key inserted (src/sstable.rs:59-63); the zone map is the
 * first and last kept key (cb_table_zone). The table is finalised and
 * well-formed, as one from cb_tables_compact; a log without an entry gives the
 * table of length 0. CB_EINVAL: table_out NULL, log NULL with len > 0, a piece
 * of 4 GiB or more, 2^32 or more entries. CB_EZEROM: m_bits == 0 with
 * bloom_out given, checked before the log is looked at. The call waits for its
 * own stream (the output's size depends on the data), never for the device. */
int cb_log_replay(const uint8_t* log, uint64_t len, uint64_t m_bits, int device, void* stream,
                  cb_table** table_out, cb_filter** bloom_out /* nullable */, void* stats /* cb_log_stats, nullable */);
/* The verdict of one piece of a log (no '\n' inside: CB_EINVAL) by the same
 * rule (parse_entries' loop body, src/wal.rs:17-28): *kind = 0 skipped (no
 * TAB, or empty), 1 an entry, CB_EUTF8 or CB_EBASE64; for an entry *key_len
 * (nullable) is the key's length and *value_len (nullable) the value's
 * decoded length, 0 both otherwise. Host only, no device access. */
int cb_log_line(const uint8_t* piece, uint64_t len, int* kind, uint64_t* key_len, uint64_t* value_len);

/* ---- the coordinator's read merge: the replicas' replies folded on the device ---- */
/* A winner's verdict (cb_fold_rows' flags, cb_reply_line's val_flags): its
 * val is copied into the response byte for byte, it is a deleted row (an
 * empty val) and left out, or the library does not decide it. */
#define CB_FOLD_TEXT 1
#define CB_FOLD_DEAD 2
#define CB_FOLD_HOST 4
/* What cb_replies_fold saw. After CB_EUTF8 bad_reply is the first reply in
 * order with a piece that is not UTF-8 and bad_offset the offset in `bytes` of
 * that reply's first such piece (every count but replies is then 0);
 * UINT64_MAX both otherwise. */
typedef struct {
    uint64_t replies;    /* nr */
    uint64_t lines;      /* lines that are not empty after the strip */
    uint64_t entries;    /* of those with two TABs */
    uint64_t others;     /* of those with fewer */
    uint64_t keys;       /* distinct keys among the entries = winners */
    uint64_t with_text;  /* winners whose val is in the response (CB_FOLD_TEXT) */
    uint64_t dead;       /* winners with an empty val (CB_FOLD_DEAD) */
    uint64_t host_rows;  /* winners the caller does again (CB_FOLD_HOST) */
    uint64_t bytes;      /* the response's length */
    uint64_t bad_reply;  /* UINT64_MAX, or the reply */
    uint64_t bad_offset; /* UINT64_MAX, or the piece's offset in bytes */
} cb_fold_stats;
/* The last step of the reference's cluster read (Cluster::execute,
 * src/cluster.rs:394-473, is_write false) over the replies of nr replicas, in
 * the caller's order (the reference's is a HashSet's): what cb_scan_select /
 * cb_rows_select write with CB_SELECT_META on every replica goes in, the
 * response bytes the client gets come out. The rule is
 * lsmt_amd/csrc/replyline.hpp's:
 *  - a reply must be UTF-8 (the reference's from_utf8_lossy replacement is left
 *    to the caller): the first reply in order with an invalid piece fails the
 *    call with CB_EUTF8, *out is NULL and *stats names it;
 *  - lines are str::lines() of each reply by itself: split at 0x0A, a piece a
 *    newline ended loses one trailing 0x0D, the last piece of a reply without
 *    a final newline keeps its 0x0D, replies are never joined, and a line that
 *    is empty after the strip is ignored;
 *  - a line with at least two TABs is an entry: key (it may be empty), the
 *    timestamp's text, val (further TABs included). The timestamp is
 *    str::parse::<u64>().unwrap_or(0): an optional single +, then ASCII digits
 *    only, at most 2^64 - 1; anything else is 0. Any other non-empty line is an
 *    "other";
 *  - per key the entry with the greatest timestamp wins, of equal ones the
 *    first in (reply, line) order;
 *  - the winners are walked ascending by key bytes. An empty val is a deleted
 *    row and left out (CB_FOLD_DEAD). A val in canonical form (an object of
 *    strings without whitespace, its names strictly ascending, every string as
 *    serde_json writes it; {} included) is copied byte for byte
 *    (CB_FOLD_TEXT): serde_json's parse and re-serialisation is the identity
 *    for it. Every other val is CB_FOLD_HOST: it may be invalid JSON, which
 *    the reference drops, or JSON that re-serialises differently; its text is
 *    left out of the response and the caller does that row again from its
 *    span (cb_fold_rows). Every row cb_scan_select writes is canonical, so a
 *    cluster of this library's nodes sees host_rows == 0;
 *  - the response: with at least one entry, [ + the CB_FOLD_TEXT texts joined
 *    by , + ]; with no entry but others, the bytewise least other line,
 *    verbatim (a forwarded COUNT(*) reply travels so); else [].
 * Where the others decide the response the call reads the pieces' verdicts
 * (and, for device input, the staged replies) back and takes the least on the
 * host: in everything the reference sends there they are one short line per
 * reply. A failed replica is simply not in the list.
 * bytes: host or device memory; reply r is bytes[off[r] .. off[r + 1]), off
 * (host memory) holds nr + 1 offsets. device == -1 folds on the host by the
 * same rule: bytes must then be host memory, no device is touched and the
 * result is the same kind of object. CB_EINVAL, *out NULL: out NULL; off NULL
 * with nr > 0; bytes NULL with a non-zero total; offsets that decrease;
 * nr > 4096; a piece of 4 GiB or more; 2^32 or more entries (the last two can
 * only occur with 4 GiB of replies or more; below that no device work is
 * needed to rule them out, above it the device finds them). nr == 0 or no
 * bytes at all gives a valid object whose text is []. The call waits for its
 * own stream wherever a size depends on the data (the pieces' count, the
 * entries' counts, the winners' totals, and at the end), never for the device,
 * and retires its blocks through the pool. The result is complete when the
 * call returns and does not depend on bytes afterwards. */
int cb_replies_fold(const uint8_t* bytes, const uint64_t* off, uint32_t nr, int device, void* stream,
                    void** out /* cb_fold */, void* stats /* cb_fold_stats, nullable */);
int cb_fold_info(const void* fold, void* stats /* cb_fold_stats */);
/* The response (stats.bytes bytes) into host or device memory. */
int cb_fold_text(const void* fold, uint8_t* text);
/* The winners in key order, stats.keys entries each, every argument nullable,
 * into host or device memory: where the key and the val lie in the caller's
 * bytes and how long they are, the parsed timestamp, the reply the winner came
 * from and its CB_FOLD_* flag. The object keeps no copy of the replies. */
int cb_fold_rows(const void* fold, uint64_t* key_at, uint64_t* key_len, uint64_t* ts, uint64_t* val_at,
                 uint64_t* val_len, uint32_t* reply, uint8_t* flags);
/* Where the least other line lies in the caller's bytes, when the others
 * decided the response (no entry at all); *at = UINT64_MAX, *len = 0 otherwise. */
int cb_fold_other(const void* fold, uint64_t* at, uint64_t* len);
int cb_fold_destroy(void* fold);
/* The verdict of one piece of a reply (no 0x0A inside: CB_EINVAL) by the same
 * rule; terminated says whether a newline of its reply followed it. *kind = 0
 * ignored (empty after the strip), 1 an entry, 2 an other, or CB_EUTF8; for an
 * entry *key_len, *ts, *val_at (the val's offset in the piece), *val_len and
 * *val_flags (its CB_FOLD_* verdict) are set, 0 all otherwise. Every output
 * but kind is nullable. Host only, no device access. */
int cb_reply_line(const uint8_t* piece, uint64_t len, int terminated, int* kind, uint64_t* key_len, uint64_t* ts,
                  uint64_t* val_at, uint64_t* val_len, uint8_t* val_flags);

/* ---- INSERT, UPDATE, DELETE: rows written to keys, values and log records on the device ---- */
/* The first step of the reference's write path for a batch of n rows of one
 * prepared statement: exec_insert + build_row (src/query.rs:162-198, 716-731),
 * exec_update (src/query.rs:201-237) or exec_delete (src/query.rs:240-261),
 * encode_row (src/schema.rs:37-39), then insert_ns_ts / insert_ts /
 * insert_internal (src/lib.rs:96-116, 154-157). The rule is
 * lsmt_amd/csrc/rowwrite.hpp's; the SQL parser stays with the caller.
 * The statement (cb_write, host memory): the namespace ns; nk <= 16 key
 * columns in the caller's order (INSERT: the statement's column order, which
 * build_row pushes; UPDATE and DELETE: the schema's key_columns()); nc <= 16
 * payload column names, strictly ascending bytewise, at most 4096 bytes
 * (cb_select's rules); set[c] = 1 the statement gives column c's value, 0 the
 * old row's is kept; op: CB_WRITE_INSERT (every set[c] is 1, no old rows),
 * CB_WRITE_UPDATE, CB_WRITE_DELETE (nc == 0, no old rows).
 * Cells: with w = nk + the number of set columns, cell (i, j) is
 * cells[cell_off[i * w + j] .. cell_off[i * w + j + 1]); a row's key cells come
 * first, then the set columns' in name order. Per row:
 *  - key: ns ':' and the key cells joined by '|' (`ns:` with nk == 0);
 *  - old map (UPDATE, old_which[i] >= 0): split_ts of old value i, its payload
 *    read as cb_rows_select reads one; an error anywhere or an empty payload (a
 *    tombstone) gives the empty map, decode_row's unwrap_or_default; of a
 *    duplicated name the last pair wins;
 *  - payload: none for DELETE; else {"name":"value",...} over the columns
 *    with a value in name order, without spaces, every string as serde_json
 *    writes it: a set column has its cell ("" for an empty one), a kept column
 *    the old map's value, a kept column without one is left out; {} is a live
 *    row, unlike DELETE's empty payload;
 *  - value: the row's timestamp (ts[i], or ts_all when ts is NULL) as 8
 *    big-endian bytes, then the payload;
 *  - log record: key \t STANDARD.encode(value) \n, what insert_internal
 *    appends and cb_log_replay reads;
 *  - flags: CB_WRITTEN_HOST the old payload is a valid map with a name outside
 *    the nc columns (names are not sorted per row on the device: the row is
 *    the caller's, as CB_ROW_EXTRA's and CB_FOLD_HOST's are; its key is
 *    written, its value and record have length 0); CB_WRITTEN_BADOLD the old
 *    payload was no valid map and counted as empty (a tombstone is not
 *    flagged); CB_WRITTEN_KEYCTL the key holds \t or \n, so its record does not
 *    replay to the same key (the row is written all the same).
 * Cell bytes are the caller's Rust Strings: UTF-8 is not checked.
 * cells, cell_off and ts: host or device memory (host inputs are staged; a
 * host cells with device offsets costs one read-back of the last offset). The
 * old arrays are device memory, as an enqueue-only cb_*get_many leaves them.
 * The work is enqueued on `stream`; the call waits for it twice (the three
 * totals size the outputs; the result is complete on return) and never for the
 * device. n == 0 gives a valid empty result and touches no device.
 * CB_EINVAL before any device work, *out NULL: out or w NULL; cb_select's
 * refusals of the columns; nk > 16; an op outside 0..2; set NULL with nc > 0,
 * a set[c] above 1, an INSERT that keeps a column, a DELETE with columns; old
 * arrays with INSERT or DELETE, or not all three of them; cells or cell_off
 * NULL with rows of at least one cell; host offsets that decrease. After the
 * size pass: a row's log record of 4 GiB or more (cb_log_replay's limit). */
#define CB_WRITE_INSERT 0
#define CB_WRITE_UPDATE 1
#define CB_WRITE_DELETE 2
#define CB_WRITTEN_HOST 1
#define CB_WRITTEN_BADOLD 2
#define CB_WRITTEN_KEYCTL 4
typedef struct cb_write {        /* host memory */
    const uint8_t* ns;           /* the namespace's bytes (NULL with ns_len == 0) */
    uint64_t ns_len;
    uint32_t nk;                 /* key columns, <= 16 */
    const uint8_t* cols;         /* the payload column names, concatenated */
    const uint64_t* col_off;     /* nc + 1 offsets into cols */
    const uint8_t* set;          /* nc flags */
    uint32_t nc;                 /* payload columns, <= 16 */
    int op;                      /* CB_WRITE_* */
} cb_write;
int cb_rows_write(const void* w /* cb_write */, const uint8_t* cells, const uint64_t* cell_off /* n * width + 1 */,
                  const uint64_t* ts /* n, nullable */, uint64_t ts_all, const int32_t* old_which /* n, nullable */,
                  const uint8_t* old_vals, const uint64_t* old_val_off /* n + 1 */, uint64_t n, int device,
                  void* stream, void** out /* cb_written */);
/* The rows, the bytes of the keys, values and log records, and the rows with
 * any flag. Every output is nullable. */
int cb_written_info(const void* written, uint64_t* count, uint64_t* key_bytes, uint64_t* val_bytes,
                    uint64_t* log_bytes, uint64_t* flagged);
/* The result's device arrays (NULL all for a batch of no rows): ragged keys
 * and values with count + 1 offsets each, the log (record i at log_off[i]),
 * and the flags. They stay valid until cb_written_destroy and are what
 * cb_sstable_create, cb_filter_insert_var, cb_ring_route_var (keys, key_off,
 * vals, val_off) and cb_log_replay (log, log_bytes) take; a table made from
 * them must be finalised (cb_table_wait) before the batch is destroyed. */
int cb_written_arrays(const void* written, const uint8_t** keys, const uint64_t** key_off, const uint8_t** vals,
                      const uint64_t** val_off, const uint8_t** log, const uint64_t** log_off,
                      const uint8_t** flags);
/* Any of the arrays into host or device memory (every output nullable). */
int cb_written_copy(const void* written, uint8_t* keys, uint64_t* key_off, uint8_t* vals, uint64_t* val_off,
                    uint8_t* log, uint64_t* log_off, uint8_t* flags);
/* Retires the result's memory through the block pool. */
int cb_written_destroy(void* written);
/* One row by the same rule on the host (a memtable-sized write; no device):
 * cell_off holds the row's width + 1 offsets; has_old != 0: old_value[0 ..
 * old_len) is the old value (UPDATE only). The three lengths are always set;
 * with out NULL nothing else happens (sizing); else, when cap holds them, out
 * receives key | value | record. */
int cb_row_write(const void* w /* cb_write */, const uint8_t* cells, const uint64_t* cell_off, uint64_t ts,
                 const uint8_t* old_value, uint64_t old_len, int has_old, uint8_t* out, uint64_t cap,
                 uint64_t* key_len, uint64_t* val_len, uint64_t* log_len, uint8_t* flags);

/* ---- tuning / introspection (bench + tests) ---- */
/* Path selection: 0 = auto, 1 = force direct (per-key atomics / gathers),
 * 2 = force tiled (LDS-staged filter tiles). Process-wide. */
int cb_set_path(int path);
/* FilterSet probes of dense batches (at least 2 keys per 128-B line of the
 * set: the C5 shape) take the region-partitioned probe, which streams the set
 * through LDS once instead of reading a random line per key; same hits.
 * mode 0 = by density (default), 1 = whenever the set allows it (32- or
 * 64-slot sets, m <= 2^32 in at most 4096 regions of 64 KiB; tests), -1 =
 * never. Never for gated probes or the fused exchange pack. Process-wide. */
int cb_set_dense(int mode);
/* Path the last insert/probe on this thread used (1 direct, 2 tiled, 3 FilterSet,
 * 4 FilterSet zero-copy: pinned host keys and hits read/written by the kernel,
 * 5 cb_may_contain answered from the host mirror, 6 FilterSet dense probe). */
int cb_last_path(void);
/* Per-kernel timing with HIP events recorded on each launch's own stream
 * (off by default). Kernel names: "k_insert_direct", "k_probe_direct",
 * "k_build_part", "k_build_tile", "k_part_probe", "k_tile_probe",
 * "k_masks_to_hits", "k_set_build", "k_set_or_slot", "k_set_put_slot",
 * "k_set_probe". cb_profile_read waits for pending events and returns the
 * accumulated milliseconds and launch count for one kernel. */
int cb_profile_enable(int on);
int cb_profile_reset(void);
int cb_profile_read(const char* kernel, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* CASSBLOOM_H */
