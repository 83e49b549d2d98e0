"""cb_tables_scan: range and prefix scans over SSTables on the device.

The reference scans its memtable alone (Database::scan / scan_ns,
src/lib.rs:144-146, 178-186), so the contract is stated the way compaction's
is: for tables T[0..nt), T[0] newest, and a byte range [lo, hi), the result is
{(k, Database::get(k))} over every key k of the inputs with lo <= k < hi for
which Database::get (src/lib.rs:128-134, over T alone) is Some, sorted by key
bytes, the values decoded. Every expectation here comes from the C oracle
(oracle.get_many over the input files for the keys of their lines; the range,
the limit and the paging are then plain filters of that sorted list), never
from the library's own read path or from cb_tables_compact; every comparison
is exact.

Shapes are the smallest at which each kernel can still go wrong: table sizes
at the directory threshold, the fence fan-out, its level edges and the tile
sizes; bounds at and between keys; keys that share 8 and 16 leading bytes;
runs of one key as long as the table count across a 256-record tile; totals
of lines and survivors around the tile sizes; values around the base64
padding and the decode's 16384-byte stage.
"""
import ctypes

import numpy as np
import pytest

from merge_help import b64, file_keys, hex_keys, named, open_tables, oracle_prefix_end, ragged, raw_file, TILE
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1
DECODE_LDS = 16384  # b64decode.hip kDecodeLds


class Ref:
    """The oracle's answer for every key of `files` (newest first), computed
    once: Database::get's walk over the files for the sorted keys of their
    lines. A scan's expectation is that list cut to the range and the limit."""

    def __init__(self, files):
        self.files = files
        self.otables = [oracle.OracleTable(f) for f in files]
        keys = sorted(set(k for f in files for k in file_keys(f)))
        self.all_keys = keys
        self.entries = []  # (key, value, which), found keys only, sorted
        if keys:
            kd, ko = ragged(keys)
            which, voff, vals = oracle.get_many(self.otables, None, kd, ko)
            self.entries = [(k, vals[int(voff[i]):int(voff[i + 1])], int(which[i]))
                            for i, k in enumerate(keys) if which[i] >= 0]

    def expect(self, lo=b"", hi=None, limit=0):
        e = [x for x in self.entries if lo <= x[0] and (hi is None or x[0] < hi)]
        more = bool(limit) and len(e) > limit
        return (e[:limit] if limit else e), more


def assert_result(r, want, truncated, what=""):
    """r holds exactly the entries `want` = [(key, value, which)]."""
    assert r.count == len(want), f"{what}: {r.count} entries against {len(want)}"
    assert r.truncated == truncated, what
    ko, kb, vo, vb = r.raw()
    eko, evo = ragged([k for k, _, _ in want])[1], ragged([v for _, v, _ in want])[1]
    assert np.array_equal(ko, eko), f"{what}: key offsets differ"
    assert kb.tobytes() == b"".join(k for k, _, _ in want), f"{what}: keys differ"
    assert np.array_equal(vo, evo), f"{what}: value offsets differ"
    assert vb.tobytes() == b"".join(v for _, v, _ in want), f"{what}: values differ"
    assert r.which().tolist() == [w for _, _, w in want], f"{what}: sources differ"
    assert (r.key_bytes, r.val_bytes) == (int(eko[-1]), int(evo[-1])), what


def check(gpu, ref, tables, lo=b"", hi=None, prefix=None, limit=0, stream=None):
    if prefix is not None:
        r = gpu.scan(tables, prefix=prefix, limit=limit, stream=stream)
        lo, hi = prefix, oracle_prefix_end(prefix)
    else:
        r = gpu.scan(tables, lo=lo, hi=hi, limit=limit, stream=stream)
    want, more = ref.expect(lo, hi, limit)
    assert_result(r, want, more, f"lo={lo[:24]!r} hi={None if hi is None else hi[:24]!r} limit={limit}")
    return r, want


# ---- bounds -------------------------------------------------------------------------

def bound_keys(rng, n):
    """n sorted keys: a third spread over the key space, a third sharing their
    first 8 bytes, a third sharing their first 16."""
    pool = set()
    while len(pool) < n:
        i = len(pool) % 3
        h = rng.integers(0, 256, 6, dtype=np.uint8).tobytes().hex().encode()
        pool.add(h if i == 0 else (b"samepfx8" + h[:int(rng.integers(0, 9))]) if i == 1
                 else b"sixteen-byte-pfx" + h[:int(rng.integers(0, 12))])
    return sorted(pool)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097])
def test_bounds_at_every_position(gpu, n):
    rng = np.random.default_rng(n)
    ks = bound_keys(rng, n)
    f = oracle.sstable_create([(k, named(0, k[-3:])) for k in ks])
    ref = Ref([f])
    tables = open_tables(gpu, [f])
    assert tables[0].well_formed and tables[0].nlines == n
    inner = ks[n // 2]
    same8 = [k for k in ks if k.startswith(b"samepfx8")]
    same16 = [k for k in ks if k.startswith(b"sixteen-byte-pfx")]
    spots = [ks[0][:-1], ks[0], ks[n // 3] + b"\0", inner, ks[-1], ks[-1] + b"\xff"]
    spots += [same8[len(same8) // 2], same8[-1] + b"\0"] if same8 else []
    spots += [same16[len(same16) // 2], same16[0][:16]] if same16 else []
    for lo in spots + [b""]:
        for hi in spots + [None]:
            r, want = check(gpu, ref, tables, lo=lo, hi=hi)
            if hi is not None and lo >= hi:
                assert r.count == 0  # lo == hi, lo > hi: empty, not an error
    full, want = check(gpu, ref, tables)
    assert full.count == n


def test_proper_prefix_keys_and_key_lengths(gpu):
    """"ab" < "ab\\0" < "aba" share one zero-padded prefix word; keys of 0, 7, 8,
    9, 15, 16, 17 and 200 bytes, the empty key the file's first line."""
    keys = [b"", b"ab", b"ab\0", b"aba", b"abcdefg", b"abcdefgh", b"abcdefgh\0", b"abcdefghi",
            b"abcdefghijklmno", b"abcdefghijklmnop", b"abcdefghijklmnop\0", b"abcdefghijklmnopq",
            b"k" * 200, b"k" * 199 + b"l"]
    assert {0, 7, 8, 9, 15, 16, 17, 200} <= {len(k) for k in keys}
    newer = oracle.sstable_create([(k, b"new:" + k[:5]) for k in sorted(keys)[::2]])
    older = oracle.sstable_create([(k, b"old:" + k[:5]) for k in sorted(keys)])
    assert older.startswith(b"\t")  # the empty key's line comes first
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    assert all(t.well_formed for t in tables)
    spots = sorted(set(keys + [k + b"\0" for k in keys] + [k[:-1] for k in keys if k] + [b"ab\1", b"l"]))
    for lo in spots:
        for hi in spots + [None]:
            check(gpu, ref, tables, lo=lo, hi=hi)


# ---- newest wins --------------------------------------------------------------------

@pytest.mark.parametrize("nt", [1, 2, 64, 65, 300])
def test_one_key_in_every_table(gpu, nt):
    """A run of nt lines of one key (300: longer than a 256-record tile), with a
    few other lines per table around it."""
    files = []
    for t in range(nt):
        e = [(b"shared-key", named(t, b"shared")), (b"own%04d" % t, named(t, b"own")),
             (b"pair%04d" % (t // 2), named(t, b"pair")), (b"z-last%d" % (t % 3), named(t, b"z"))]
        files.append(oracle.sstable_create(e))
    ref = Ref(files)
    tables = open_tables(gpu, files)
    r, want = check(gpu, ref, tables)
    got = dict(zip(r.keys(), zip(r.values(), r.which().tolist())))
    assert got[b"shared-key"] == (b"t0:shared", 0)
    assert got[b"own%04d" % (nt - 1)] == (named(nt - 1, b"own"), nt - 1)
    check(gpu, ref, tables, lo=b"pair", hi=b"shared-key\0")
    check(gpu, ref, tables, lo=b"shared-key", hi=b"shared-key\0")
    check(gpu, ref, tables, prefix=b"shared")


def test_undecodable_values_fall_through_and_drop(gpu):
    spoiled = [b"QUJD*A==", b"QUJDRA=", b"QQ=", b"QR==", b"====", b"A"]
    for s in spoiled:
        assert oracle.b64_decode(s) is None, s
    keys = [b"s%02d" % i for i in range(len(spoiled))]
    newest = raw_file([(k, s) for k, s in zip(keys, spoiled)] + [(b"t-good", b64(b"new"))])
    middle = raw_file([(k, spoiled[(i + 1) % len(spoiled)] if i % 2 else b64(b"mid" + k)) for i, k in enumerate(keys)])
    oldest = raw_file([(k, b64(b"old" + k)) for k in keys[:-1]] + [(b"t-good", b64(b"old"))], final_newline=False)
    ref = Ref([newest, middle, oldest])
    tables = open_tables(gpu, [newest, middle, oldest])
    r, want = check(gpu, ref, tables)
    got = dict(zip(r.keys(), zip(r.values(), r.which().tolist())))
    assert got[b"s00"] == (b"mids00", 1)       # newest spoiled: the middle one wins
    assert got[b"s01"] == (b"olds01", 2)       # two spoiled: the oldest wins
    assert keys[-1] not in got                 # spoiled everywhere: dropped
    assert got[b"t-good"] == (b"new", 0)
    check(gpu, ref, tables, lo=b"s01", hi=b"s05\0")
    # nothing decodes anywhere: an empty result
    files = [raw_file([(b"a", b"*"), (b"b", b"QQ=")]), raw_file([(b"a", b"A")])]
    r, want = check(gpu, Ref(files), open_tables(gpu, files))
    assert r.count == 0 and r.keys() == [] and r.values() == [] and len(r.which()) == 0


def test_empty_and_out_of_range_tables_anywhere(gpu):
    rng = np.random.default_rng(5)
    inside = [b"m" + k for k in hex_keys(rng, 120, 8)]
    below = oracle.sstable_create([(b"a%03d" % i, b"below") for i in range(20)])
    above = oracle.sstable_create([(b"z%03d" % i, b"above") for i in range(20)])

    def live(t):
        ks = [inside[i] for i in rng.choice(len(inside), 40, replace=False)]
        return oracle.sstable_create([(k, named(t, k)) for k in ks] + [(b"a000", named(t, b"lo")), (b"z019", named(t, b"hi"))])
    for files in ([b"", live(1), below, b"", b"", live(5), above, below, live(8), above],
                  [below, above, live(2), b""],
                  [live(0), b"", above, below, b"", live(5), b""],
                  [b"", b"", below]):
        ref = Ref(files)
        tables = open_tables(gpu, files)
        check(gpu, ref, tables, lo=b"m", hi=b"n")
        check(gpu, ref, tables, lo=b"m", hi=b"n", limit=7)
        check(gpu, ref, tables, prefix=b"m")
        check(gpu, ref, tables)
        check(gpu, ref, tables, lo=b"b", hi=b"c")  # between the tables' keys: empty


# ---- totals around the tiles --------------------------------------------------------

@pytest.mark.parametrize("total", [255, 256, 257, 4095, 4096, 4097])
def test_lines_inside_the_range_at_tile_sizes(gpu, total):
    """`total` lines inside [lo, hi) over three tables (with lines outside it)."""
    rng = np.random.default_rng(total)
    pool = sorted(hex_keys(rng, total, 12))
    inside = [b"m" + k for k in pool]
    n0 = total // 2
    n1 = (total - n0) // 2
    parts = [inside[:n0], inside[n0 - n1 // 2:n0 + n1 - n1 // 2], None]  # tables 0 and 1 overlap
    parts[2] = [inside[i] for i in rng.choice(total, total - n0 - n1, replace=False)]
    files = []
    for t, ks in enumerate(parts):
        out = [(b"a%d-%03d" % (t, i), b"low") for i in range(3 + t)] + [(b"q%d-%03d" % (t, i), b"high") for i in range(5)]
        files.append(oracle.sstable_create([(k, named(t, k[-4:])) for k in ks] + out))
    assert sum(len(p) for p in parts) == total
    ref = Ref(files)
    tables = open_tables(gpu, files)
    r, want = check(gpu, ref, tables, lo=b"m", hi=b"n")
    assert r.count == len(set(k for p in parts for k in p))
    check(gpu, ref, tables, prefix=b"m")


@pytest.mark.parametrize("survivors", [255, 256, 257])
def test_survivors_at_tile_sizes(gpu, survivors):
    rng = np.random.default_rng(survivors)
    ks = sorted(hex_keys(rng, survivors + 40, 12))
    dead, keep = ks[::9][:40], None
    keep = [k for k in ks if k not in set(dead)][:survivors]
    newer = raw_file(sorted([(k, b64(named(0, k[:3]))) for k in keep[::2]] + [(k, b"!bad") for k in dead]))
    older = raw_file(sorted([(k, b64(named(1, k[:3]))) for k in keep] + [(k, b"QQ=") for k in dead[::2]]))
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    r, want = check(gpu, ref, tables)
    assert r.count == survivors
    check(gpu, ref, tables, lo=keep[1], hi=keep[-1])


# ---- values -------------------------------------------------------------------------

def test_value_lengths_around_the_padding(gpu):
    rng = np.random.default_rng(3)
    sizes = [0, 1, 2, 3, 17, 18, 19]
    new = [(b"v%05d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in sizes]
    old = [(b"v%05d" % n, b"old") for n in sizes[::2]] + [(b"w", b"only-old")]
    for files in ([oracle.sstable_create(new), oracle.sstable_create(old)],
                  [oracle.sstable_create(old), oracle.sstable_create(new)]):
        ref = Ref(files)
        tables = open_tables(gpu, files)
        r, want = check(gpu, ref, tables)
        check(gpu, ref, tables, lo=b"v00002", hi=b"v00019")


@pytest.mark.parametrize("size", [DECODE_LDS, DECODE_LDS + 1])
def test_a_value_on_each_side_of_the_decode_stage(gpu, size):
    rng = np.random.default_rng(size)
    big = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    files = [oracle.sstable_create([(b"big", big)]), oracle.sstable_create([(b"big", b"older"), (b"small", b"s")])]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    r, want = check(gpu, ref, tables, lo=b"big", hi=b"big\0")  # the tile's values: `size` bytes
    assert r.val_bytes == size
    check(gpu, ref, tables)


def test_result_with_no_value_bytes(gpu):
    files = [oracle.sstable_create([(b"k%03d" % i, b"") for i in range(0, 300, 2)]),
             oracle.sstable_create([(b"k%03d" % i, b"") for i in range(300)])]
    r, want = check(gpu, Ref(files), open_tables(gpu, files))
    assert r.count == 300 and r.val_bytes == 0 and r.values() == [b""] * 300


# ---- limit --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def store(gpu):
    """Five overlapping tables of a few hundred lines: (ref, tables)."""
    rng = np.random.default_rng(21)
    pool = hex_keys(rng, 900, 10)
    files = []
    for t in range(5):
        ks = [pool[i] for i in rng.choice(len(pool), int(rng.integers(150, 400)), replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k[:int(rng.integers(0, 9))])) for k in ks]))
    return Ref(files), open_tables(gpu, files)


def test_limit_and_truncated(gpu, store):
    ref, tables = store
    lo, hi = b"3", b"c"
    count = len(ref.expect(lo, hi)[0])
    assert count > 300
    for limit in (1, count - 1, count, count + 1):
        r, want = check(gpu, ref, tables, lo=lo, hi=hi, limit=limit)
        assert r.truncated == (limit < count) and r.count == min(limit, count)
    full = len(ref.entries)
    for limit in (1, TILE, TILE + 1, full - 1, full, full + 1):
        check(gpu, ref, tables, limit=limit)


@pytest.mark.parametrize("page", [1, 100, 256, 257])
def test_paging_reproduces_the_unlimited_scan(gpu, store, page):
    ref, tables = store
    lo, hi = (b"2", b"e") if page > 1 else (b"2", b"24")
    whole = gpu.scan(tables, lo=lo, hi=hi)
    assert_result(whole, ref.expect(lo, hi)[0], False)
    got, at, pages = [], lo, 0
    while True:
        r = gpu.scan(tables, lo=at, hi=hi, limit=page)
        items = list(zip(r.keys(), r.values(), r.which().tolist()))
        got += items
        pages += 1
        if not r.truncated:
            break
        assert len(items) == page
        at = items[-1][0] + b"\0"
    assert got == ref.expect(lo, hi)[0]
    assert pages == max(1, -(-len(got) // page))
    assert got == list(zip(whole.keys(), whole.values(), whole.which().tolist()))


# ---- prefix -------------------------------------------------------------------------

def test_namespace_prefixes(gpu):
    """scan_ns(ns) is the prefix ns + ":" (src/lib.rs:179): "t" must not take
    "t2"'s rows, whose name it is a prefix of."""
    rng = np.random.default_rng(8)
    files = []
    for t in range(4):
        e = [(b"%s:%s" % (ns, k), named(t, ns)) for ns in (b"t", b"t2", b"u")
             for k in hex_keys(rng, int(rng.integers(20, 60)), 6)]
        e += [(b"t:shared", named(t, b"t")), (b"t2:shared", named(t, b"t2")), (b"t", b"bare"), (b"t;", b"after")]
        files.append(oracle.sstable_create(e))
    ref = Ref(files)
    tables = open_tables(gpu, files)
    for ns in (b"t", b"t2", b"u", b"none"):
        r, want = check(gpu, ref, tables, prefix=ns + b":")
        assert all(k.startswith(ns + b":") for k in r.keys())
        assert r.count == sum(k.startswith(ns + b":") for k, _, _ in ref.entries)
        assert gpu.prefix_end(ns + b":") == ns + b";"
    r, want = check(gpu, ref, tables, prefix=b"t")
    assert r.count == sum(k.startswith(b"t") for k, _, _ in ref.entries)
    r, want = check(gpu, ref, tables, prefix=b"")  # the empty prefix: the full scan
    assert r.count == len(ref.entries)
    check(gpu, ref, tables, prefix=b"t:", limit=5)


def test_prefix_ending_in_ff(gpu):
    keys = sorted([b"a", b"a\xfe", b"a\xfe\xff", b"a\xff", b"a\xff\x00", b"a\xff\xff", b"a\xff\xffz", b"b", b"b\x00",
                   b"\xff", b"\xff\xff", b"\xff\xff\xff", b"\xfe\xff"])
    newer = raw_file([(k, b64(b"n" + k)) for k in keys[::2]])
    older = raw_file([(k, b64(b"o" + k)) for k in keys])
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    assert all(t.well_formed for t in tables)
    for p in (b"a\xff", b"a\xff\xff", b"a\xfe\xff", b"\xff", b"\xff\xff", b"a", b"\xfe\xff"):
        r, want = check(gpu, ref, tables, prefix=p)
        assert r.keys() == [k for k in keys if k.startswith(p)], p


# ---- cross-check --------------------------------------------------------------------

def test_full_scan_has_the_keys_of_the_compacted_file(gpu, store):
    ref, tables = store
    r, want = check(gpu, ref, tables)  # (the oracle is the expectation)
    merged, _, _ = gpu.compact(tables)
    assert r.keys() == file_keys(merged.data())
    lines = [ln for ln in merged.data().split(b"\n") if ln]
    assert [k + b"\t" + b64(v) for k, v in r.items()] == lines


# ---- lifetime and residency ---------------------------------------------------------

def test_stream_inputs_unchanged_and_result_outlives_inputs(gpu):
    import torch
    rng = np.random.default_rng(31)
    pool = hex_keys(rng, 3000, 12)
    files = []
    for t in range(4):
        ks = [pool[i] for i in rng.choice(len(pool), 1200, replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k[:5])) for k in ks]))
    ref = Ref(files)
    tables = open_tables(gpu, files)
    stream = torch.cuda.Stream()
    r, want = check(gpu, ref, tables, lo=b"1", hi=b"f", stream=stream)
    assert [t.data() for t in tables] == files, "an input changed"
    # outputs copied into device tensors equal the host copies
    ko, kb, vo, vb = r.raw()
    d_ko = torch.zeros(r.count + 1, dtype=torch.int64, device="cuda")
    d_kb = torch.zeros(r.key_bytes, dtype=torch.uint8, device="cuda")
    d_vo = torch.zeros(r.count + 1, dtype=torch.int64, device="cuda")
    d_vb = torch.zeros(r.val_bytes, dtype=torch.uint8, device="cuda")
    d_w = torch.zeros(r.count, dtype=torch.int32, device="cuda")
    r.copy_keys(d_ko, d_kb)
    r.copy_values(d_vo, d_vb)
    r.copy_which(d_w)
    assert np.array_equal(d_ko.cpu().numpy().astype(np.uint64), ko) and d_kb.cpu().numpy().tobytes() == kb.tobytes()
    assert np.array_equal(d_vo.cpu().numpy().astype(np.uint64), vo) and d_vb.cpu().numpy().tobytes() == vb.tobytes()
    assert np.array_equal(d_w.cpu().numpy(), r.which())
    r.copy_keys(None, d_kb)  # either pointer of a pair may be left out
    r.copy_values(d_vo, None)
    # the result owns its memory: close every input, let the pool hand their blocks out again
    for t in tables:
        t.close()
    churn = open_tables(gpu, files)
    assert_result(r, want, False, "after the inputs were closed")
    del churn
    r.close()
    r.close()


def test_pending_inputs(gpu):
    rng = np.random.default_rng(32)
    pool = hex_keys(rng, 6000)
    entries, files = [], []
    for t in range(3):
        ks = [pool[i] for i in rng.choice(len(pool), 5000, replace=False)]  # unsorted, past 4096: the bin sort
        e = [(k, named(t, k[:6])) for k in ks]
        entries.append(e)
        files.append(oracle.sstable_create(e))
    ref = Ref(files)
    tables = [gpu.sstable_create(e, wait=False)[0] for e in entries]  # not waited on
    check(gpu, ref, tables, lo=b"4", hi=b"9")
    check(gpu, ref, tables)
    assert [t.data() for t in tables] == files


def test_refusals(gpu):
    good = gpu.Table(oracle.sstable_create([(b"a", b"1"), (b"b", b"2")]))
    unsorted = gpu.Table(raw_file([(b"b", b64(b"1")), (b"a", b64(b"2"))]))
    no_tab = gpu.Table(b"a\tQQ==\nnotab\nz\tQQ==\n")
    assert not unsorted.well_formed and not no_tab.well_formed
    for tables in ([good, unsorted], [no_tab, good]):
        for kw in ({}, {"prefix": b"a"}, {"lo": b"x", "hi": b"y"}):
            with pytest.raises(gpu._lib.CassBloomError) as ei:
                gpu.scan(tables, **kw)
            assert ei.value.code == CB_EINVAL
    L = gpu._lib.load()
    out = ctypes.c_void_p(0xDEAD)
    arr = ctypes.cast((ctypes.c_void_p * 2)(good._h.value, unsorted._h.value), ctypes.c_void_p)
    assert L.cb_tables_scan(arr, 2, b"", 0, None, 0, 0, 0, None, ctypes.byref(out)) == CB_EINVAL
    assert not out.value
    arr = ctypes.cast((ctypes.c_void_p * 1)(good._h.value), ctypes.c_void_p)
    for args in [(None, 1, b"b", 1, 1), (b"a", 1, None, 1, 1)]:  # a null bound with a length
        out.value = 0xDEAD
        assert L.cb_tables_scan(arr, 1, *args, 0, None, ctypes.byref(out)) == CB_EINVAL
        assert not out.value
    assert L.cb_tables_scan_prefix(arr, 1, None, 2, 0, None, ctypes.byref(out)) == CB_EINVAL
    # has_hi == 0: hi is ignored, NULL with a length included; a valid call still works
    assert L.cb_tables_scan(arr, 1, b"", 0, None, 7, 0, 0, None, ctypes.byref(out)) == 0
    r = gpu.ScanResult(out.value, 0)
    assert r.items() == [(b"a", b"1"), (b"b", b"2")] and r.which().tolist() == [0, 0]


def test_refusal_precedence(gpu):
    """Which refusal wins when a call earns several, straight through the ABI:
    the list's own checks, then the bounds, then the tables' contents."""
    L = gpu._lib.load()
    good = gpu.Table(oracle.sstable_create([(b"a", b"1"), (b"b", b"2")]))
    unsorted = gpu.Table(raw_file([(b"b", b64(b"1")), (b"a", b64(b"2"))]))
    assert not unsorted.well_formed

    def scan(handles, nt, lo, lo_len):
        out = ctypes.c_void_p(0xDEAD)
        arr = ctypes.cast((ctypes.c_void_p * 2)(*handles), ctypes.c_void_p)
        rc = L.cb_tables_scan(arr, nt, lo, lo_len, None, 0, 0, 0, None, ctypes.byref(out))
        assert not out.value
        return rc, L.cb_last_error().decode()

    assert scan([good._h.value, None], 2, None, 1) == (CB_EINVAL, "null table")
    assert scan([good._h.value, None], 1, None, 1) == (CB_EINVAL, "null lower bound with a length")
    assert scan([good._h.value, unsorted._h.value], 2, None, 1) == (CB_EINVAL, "null lower bound with a length")
    assert scan([good._h.value, unsorted._h.value], 2, b"", 0) == (CB_EINVAL, "an input table is not well-formed")
    assert scan([good._h.value, None], 0, None, 1) == (CB_EINVAL, "no tables")


# ---- the value tail shared with the gets --------------------------------------------

def test_results_on_each_side_of_the_raw_decode_limit(gpu):
    """262145 results are one more than the decode scans the tile sums for
    itself (sstable.hpp decode_raw_max): the full scan takes the one-block
    scan ahead of the decode, the scan limited to 262144 the decode alone, on
    the same data. The expectation is built here from the lists the file is
    written from."""
    n = 262145
    keys = [b"%08d" % i for i in range(n)]
    vals = [b"" if i % 7 == 0 else bytes([i % 251]) for i in range(n)]
    table = gpu.Table(b"".join(k + b"\t" + b64(v) + b"\n" for k, v in zip(keys, vals)))
    assert table.well_formed and table.nlines == n
    want = [(k, v, 0) for k, v in zip(keys, vals)]
    assert_result(gpu.scan([table]), want, False, "full")
    assert_result(gpu.scan([table], limit=n - 1), want[:n - 1], True, "limit 262144")


def test_get_scan_get_on_one_stream(gpu):
    """A get of 65 keys over two tables, a scan of the same tables and the get
    again, enqueued on one stream with device outputs: the scan's value tail
    has buffers of its own, so both gets answer as the oracle does."""
    import torch
    rng = np.random.default_rng(41)
    pool = hex_keys(rng, 2200)
    per = [pool[:900], pool[600:1800]]  # 300 keys in both tables
    files = [oracle.sstable_create([(k, named(t, k[:7])) for k in ks]) for t, ks in enumerate(per)]
    tables = open_tables(gpu, files)
    look = np.frombuffer(b"".join(pool[:20] + pool[600:620] + pool[1700:1720] + pool[-5:]), np.uint8).reshape(-1, 16)
    assert len(look) == 65
    d = np.ascontiguousarray(look.reshape(-1))
    offs = np.arange(0, 16 * (len(look) + 1), 16, dtype=np.uint64)
    ow, ovoff, ovals = oracle.get_many([oracle.OracleTable(f) for f in files], None, d, offs)
    assert (ow >= 0).sum() >= 60
    dk = gpu.DeviceKeys(torch.from_numpy(look.copy()).cuda())
    s = torch.cuda.Stream()

    def get():
        o = (torch.empty(65, dtype=torch.int32, device="cuda"), torch.empty(66, dtype=torch.int64, device="cuda"),
             torch.zeros(len(ovals) + 64, dtype=torch.uint8, device="cuda"))
        assert gpu.get_many(tables, dk, out=o, stream=s, wait=False)[2] is None
        return o
    first = get()
    ref = Ref(files)
    r, want = check(gpu, ref, tables, stream=s)
    assert r.count == len(ref.entries) > 1200
    second = get()
    s.synchronize()
    for w, vo, vb in (first, second):
        assert np.array_equal(w.cpu().numpy(), ow)
        assert np.array_equal(vo.cpu().numpy().view(np.uint64), ovoff)
        assert vb[:len(ovals)].cpu().numpy().tobytes() == ovals
    assert all(torch.equal(a, b) for a, b in zip(first, second))
