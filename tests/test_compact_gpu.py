"""cb_tables_compact: the newest-wins merge of SSTables on the device.

The reference has no compaction, so the contract is stated through the two
reference functions the result must be indistinguishable from: for tables
T[0..nt), T[0] newest, the merged data file is SsTable::create
(src/sstable.rs:51-87) of {(k, Database::get(k))} over every key k of the
inputs for which Database::get (src/lib.rs:128-134, over T alone) is Some.
Every expectation here comes from the C oracle (oracle.get_many over the
input files, oracle.sstable_create of the found pairs, OracleFilter over the
kept keys), never from the library's own read path; every comparison is exact.

Shapes are the smallest at which each kernel can still go wrong: runs of one
key as long as the table count across 256-record tiles and the sort's
4096-record tiles, line totals around the tile sizes, keys around the 16-byte
sort record, values around the base64 padding and the format pass's stages.
"""

import numpy as np
import pytest

from merge_help import absent_keys, b64, BAD, file_keys, hex_keys, named, ragged, raw_file, TILE
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1
SORT_TILE = 4096  # sort.hip kTile: records per block sort


def expected(files, m):
    """(file, OracleFilter, (min, max) or None, kept keys) of compacting `files` (newest first)."""
    otables = [oracle.OracleTable(f) for f in files]
    keys = sorted(set(k for f in files for k in file_keys(f)))
    filt = oracle.OracleFilter(m)
    if not keys:
        return b"", filt, None, [], otables
    kd, ko = ragged(keys)
    which, voff, vals = oracle.get_many(otables, None, kd, ko)
    entries = [(k, vals[int(voff[i]):int(voff[i + 1])]) for i, k in enumerate(keys) if which[i] >= 0]
    kept = [k for k, _ in entries]
    if kept:
        filt.insert_var(*ragged(kept))
    zone = (min(kept), max(kept)) if kept else None
    return (oracle.sstable_create(entries) if entries else b""), filt, zone, kept, otables


def check(gpu, files, m=1024, tables=None, seed=0):
    """Compacts `files` (or the given tables made from them) and checks the
    merged file, filter, zone bounds and reads against the oracle. Returns
    (merged table, bloom, zone, expected file)."""
    want, filt, zone, kept, otables = expected(files, m)
    own = tables is None
    if own:
        tables = [gpu.Table(f) for f in files]
    before = [t.data() for t in tables] if own else None
    merged, bloom, z = gpu.compact(tables, m=m)
    got = merged.data()
    assert got == want, f"merged file differs: {len(got)} bytes against {len(want)}"
    assert np.array_equal(bloom.bools(), filt.bools()), "filter bits differ from the oracle"
    if zone is None:
        assert (z.min, z.max) == (None, None)
        assert merged.nlines == 0 and merged.nbytes == 0
        with pytest.raises(gpu._lib.CassBloomError) as ei:
            merged._zone(0)
        assert ei.value.code == CB_EINVAL
    else:
        assert (z.min, z.max) == zone
        assert merged.well_formed
        assert merged.nlines == len(kept)
    if own:
        assert [t.data() for t in tables] == before, "an input changed"
    # reads of the merged table against the oracle's walk over the inputs
    rng = np.random.default_rng(seed)
    allk = sorted(set(k for f in files for k in file_keys(f)))
    look = allk + absent_keys(allk, rng)
    order = rng.permutation(len(look))
    look = [look[i] for i in order]
    kd, ko = ragged(look)
    ow, ovoff, ovals = oracle.get_many(otables, None, kd, ko)
    which, voff, vals = gpu.get_many([merged], look)
    assert np.array_equal(which >= 0, ow >= 0), "found keys differ"
    assert np.array_equal(voff, ovoff) and vals == ovals, "values differ"
    if own:
        for t in tables:
            t.close()
    return merged, bloom, z, want


def overlap_files(nt, pool, rng, lo=1, hi=256):
    """nt tables of lo..hi lines drawn from pool; each table's values name the table."""
    files = []
    for t in range(nt):
        n = int(rng.integers(lo, hi + 1))
        ks = [pool[i] for i in rng.choice(len(pool), n, replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k)) for k in ks]))
    return files


# ---- identity, one table, tiny tables ------------------------------------------------

def test_one_table_is_returned_byte_identical(gpu):
    rng = np.random.default_rng(1)
    keys = hex_keys(rng, 700)
    f = oracle.sstable_create([(k, rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()) for k in keys])
    merged, _, _, want = check(gpu, [f])
    assert want == f


def test_one_table_is_normalised(gpu):
    lines = [(b"a", b64(b"1")), (b"b", b64(b"22")), (b"c", b64(b"333")), (b"d", b"")]
    f = b"\n\n" + b"\n\n\n".join(k + b"\t" + t for k, t in lines)  # empty lines, no final newline
    merged, _, _, want = check(gpu, [f])
    assert want == raw_file(lines)


@pytest.mark.parametrize("sizes", [(1,), (3,), (1, 1), (1, 3), (3, 1, 3)])
def test_tiny_tables(gpu, sizes):
    pool = [b"k%d" % i for i in range(4)]
    files = [oracle.sstable_create([(k, named(t, k)) for k in pool[:n]]) for t, n in enumerate(sizes)]
    check(gpu, files)


# ---- overlap ------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["disjoint", "interleaved", "identical"])
def test_two_tables(gpu, kind):
    a = [b"key%04d" % (2 * i) for i in range(300)]
    b = {"disjoint": [b"zey%04d" % i for i in range(300)],
         "interleaved": [b"key%04d" % (2 * i + 1) for i in range(300)],
         "identical": a}[kind]
    files = [oracle.sstable_create([(k, named(0, k)) for k in a]), oracle.sstable_create([(k, named(1, k)) for k in b])]
    merged, _, _, want = check(gpu, files)
    if kind == "identical":
        assert want == files[0]


@pytest.mark.parametrize("nt", [3, 64, 65, 300])
def test_many_overlapping_tables(gpu, nt):
    rng = np.random.default_rng(100 + nt)
    pool = hex_keys(rng, 3000)
    check(gpu, overlap_files(nt, pool, rng), seed=nt)


# ---- runs at edges ------------------------------------------------------------------

def run_files(spoil_newest=0, spoil_all_key=False):
    """300 tables. `hot1` and `n-hot2` are in all of them: in sorted order their
    runs of 300 records cover positions 200..499 (across the 256-record tile
    and block edge) and 4000..4299 (across the sort's 4096-record tile).
    spoil_newest: the hot keys' values in the newest that-many tables do not
    decode, so the survivor sits that deep in its run."""
    nt = 300
    before = [b"a%05d" % i for i in range(200)]
    mid = [b"m%05d" % i for i in range(3500)]
    after = [b"z%05d" % i for i in range(130)]
    files = []
    for t in range(nt):
        lines = [(k, b64(named(t, k))) for k in before[t::nt] + mid[t::nt] + after[t::nt]]
        for hot in (b"hot1", b"n-hot2"):
            lines.append((hot, b"*bad*" if t < spoil_newest else b64(named(t, hot))))
        if spoil_all_key:
            lines.append((b"never", b"A" if t % 2 else b"===="))
        files.append(raw_file(sorted(lines)))
    return files


def test_run_of_300_across_tile_and_block_edges(gpu):
    files = run_files()
    allk = sorted(set(k for f in files for k in file_keys(f)))
    assert allk.index(b"hot1") == 200 and 200 < TILE < 200 + 300
    assert 200 + 300 + 3500 < SORT_TILE < 200 + 300 + 3500 + 300
    merged, _, _, want = check(gpu, files)
    assert b"hot1\t" + b64(b"t0:hot1") + b"\n" in want


@pytest.mark.parametrize("depth", [1, 63, 64, 65, 299])
def test_run_with_spoiled_newest_lines(gpu, depth):
    merged, _, _, want = check(gpu, run_files(spoil_newest=depth, spoil_all_key=True))
    assert b"n-hot2\t" + b64(b"t%d:n-hot2" % depth) + b"\n" in want
    assert b"never" not in want


@pytest.mark.parametrize("total", [255, 256, 257, 2048, 4096, 4097])
def test_line_totals_at_tile_sizes(gpu, total):
    rng = np.random.default_rng(total)
    pool = hex_keys(rng, total)
    n0 = total // 2
    f0 = oracle.sstable_create([(k, named(0, k)) for k in pool[:n0]])
    # the older table repeats a third of the newer one's keys
    older = pool[n0 - (total - n0) // 3:][:total - n0]
    f1 = oracle.sstable_create([(k, named(1, k)) for k in older])
    assert len(file_keys(f0)) + len(file_keys(f1)) == total
    check(gpu, [f0, f1], seed=total)


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_a_three_byte_tile_at_every_output_alignment(gpu, start):
    """One table of 600 lines. The second format tile (records 256 to 511)
    holds one survivor, the 3-byte line `b TAB NL` among 255 lines that do not
    decode, and begins `start` bytes past a dword of the merged file: the tile
    is all head, or all tail, or both, and has no whole dword."""
    lines = [(b"a%03d" % i + b"x" * (start if i == 7 else 0), b64(b"v")) for i in range(TILE)]
    lines += [(b"b", b"")] + [(b"b%03d" % i, BAD) for i in range(TILE - 1)]
    lines += [(b"c%03d" % i, b64(b"w%d" % i)) for i in range(88)]
    assert len(lines) == 600 and lines == sorted(lines) and lines[TILE][0] == b"b"
    merged, _, _, want = check(gpu, [raw_file(lines)], seed=start)
    assert want.index(b"\nb\t\n") + 1 == 10 * TILE + start and merged.nlines == TILE + 1 + 88


def test_70001_lines_over_five_tables(gpu):
    rng = np.random.default_rng(70001)
    pool = hex_keys(rng, 30000)
    files = []
    for t, n in enumerate([14000, 14000, 14000, 14000, 14001]):
        ks = [pool[i] for i in rng.choice(len(pool), n, replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k[:4])) for k in ks]))
    check(gpu, files, seed=5)


# ---- keys ---------------------------------------------------------------------------

def test_key_lengths_and_prefixes(gpu):
    rng = np.random.default_rng(7)
    base = b"0123456789abcdefXYZ"
    keys = [b"", b"q", base[:15], base[:16], base[:17], base + b"0123456789abcd", b"L" * 5000]
    keys += [base[:16] + b"tail-one", base[:16] + b"tail-two", base[:16] + b"tail", b"pre", b"prefix", b"prefixed"]
    keys += [b"L" * 4999 + b"M", b"L" * 4999]
    assert len(keys[5]) == 33
    files = []
    for t in range(3):
        ks = [k for i, k in enumerate(keys) if (i + t) % 3 != 0 or t == 2]
        files.append(oracle.sstable_create([(k, named(t, k[:8])) for k in ks]))
    check(gpu, files)
    text = [b"user:%s:profile" % w for w in (b"alice", b"bob", b"carol", b"dave", b"erin")] + [b"zeta", b"Alpha beta", b"~"]
    files = [oracle.sstable_create([(k, named(t, k)) for k in text[t:] + hex_keys(rng, 50)]) for t in range(3)]
    check(gpu, files)


def test_600_keys_under_one_8_byte_prefix(gpu):
    """One bin for the bin sort: its merge-sort fallback orders the batch."""
    keys = [b"sameprfx%04d" % i for i in range(600)]
    rng = np.random.default_rng(8)
    files = []
    for t in range(12):
        ks = [keys[i] for i in rng.choice(600, 450, replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k)) for k in ks]))
    assert sum(len(file_keys(f)) for f in files) > SORT_TILE
    check(gpu, files)


# ---- values -------------------------------------------------------------------------

def test_value_sizes(gpu):
    rng = np.random.default_rng(9)
    sizes = [0, 1, 2, 3, 4, 5, 6, 4095, 4097, 70001]
    new = [(b"v%05d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in sizes]
    old = [(b"v%05d" % n, b"old") for n in sizes[::2]] + [(b"w", b"only-old"), (b"v70001x", bytes(70000))]
    check(gpu, [oracle.sstable_create(new), oracle.sstable_create(old)])
    check(gpu, [oracle.sstable_create(old), oracle.sstable_create(new)])


# ---- spoiled values -----------------------------------------------------------------

SPOILED = [b"QUJD*A==", b"QUJDRA=", b"QUJDR", b"QQ=", b"QR==", b"====", b"A", b"QUJD\x80"]


def test_spoiled_values_lose_to_older_lines(gpu):
    for s in SPOILED:
        assert oracle.b64_decode(s) is None, s
    keys = [b"s%02d" % i for i in range(len(SPOILED))]
    newest = raw_file([(k, s) for k, s in zip(keys, SPOILED)] + [(b"t-good", b64(b"new"))])
    middle = raw_file([(k, SPOILED[(i + 1) % len(SPOILED)] if i % 2 else b64(b"mid" + k)) for i, k in enumerate(keys)])
    oldest = raw_file([(k, b64(b"old" + k)) for k in keys[:-1]] + [(b"t-good", b64(b"old"))], final_newline=False)
    merged, _, _, want = check(gpu, [newest, middle, oldest])
    assert b"s00\t" + b64(b"mids00") + b"\n" in want      # newest spoiled: the middle one wins
    assert b"s01\t" + b64(b"olds01") + b"\n" in want      # two spoiled: the oldest wins
    assert keys[-1] not in file_keys(want)                # spoiled everywhere: dropped
    assert b"t-good\t" + b64(b"new") + b"\n" in want


def test_result_with_no_lines(gpu):
    files = [raw_file([(b"a", b"*"), (b"b", b"QQ=")]), raw_file([(b"a", b"A")])]
    merged, bloom, z, want = check(gpu, files)
    assert want == b"" and merged.nlines == 0
    # an empty input contributes nothing; an empty result compacts again
    t = gpu.Table(oracle.sstable_create([(b"k", b"v")]))
    again, _, _ = gpu.compact([merged, t])
    assert again.data() == t.data()


# ---- refusals -----------------------------------------------------------------------

def test_refusals(gpu):
    good = gpu.Table(oracle.sstable_create([(b"a", b"1"), (b"b", b"2")]))
    unsorted = gpu.Table(raw_file([(b"b", b64(b"1")), (b"a", b64(b"2"))]))
    no_tab = gpu.Table(b"a\tQQ==\nnotab\nz\tQQ==\n")
    assert not unsorted.well_formed and not no_tab.well_formed
    for tables in ([good, unsorted], [no_tab, good], []):
        with pytest.raises(gpu._lib.CassBloomError) as ei:
            gpu.compact(tables)
        assert ei.value.code == CB_EINVAL
    # straight through the ABI: nothing is returned
    import ctypes
    L = gpu._lib.load()
    th, fh = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xbeef)
    arr = (ctypes.c_void_p * 2)(good._h.value, unsorted._h.value)
    assert L.cb_tables_compact(ctypes.cast(arr, ctypes.c_void_p), 2, 1024, None, ctypes.byref(th), ctypes.byref(fh)) == CB_EINVAL
    assert not th.value and not fh.value
    arr = (ctypes.c_void_p * 2)(good._h.value, None)
    assert L.cb_tables_compact(ctypes.cast(arr, ctypes.c_void_p), 2, 1024, None, ctypes.byref(th), ctypes.byref(fh)) == CB_EINVAL
    assert L.cb_tables_compact(ctypes.cast(arr, ctypes.c_void_p), 0, 1024, None, ctypes.byref(th), ctypes.byref(fh)) == CB_EINVAL
    with pytest.raises(ZeroDivisionError):
        gpu.compact([good], m=0)
    merged, _, _ = gpu.compact([good, good])  # a following valid call still works
    assert merged.data() == good.data()
    th = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 1)(good._h.value)
    assert L.cb_tables_compact(ctypes.cast(arr, ctypes.c_void_p), 1, 0, None, ctypes.byref(th), None) == 0  # no bloom: m unused
    t = gpu.Table._adopt(th.value, 0)
    assert t.data() == good.data()


def test_refusal_precedence(gpu):
    """Which refusal wins when a call earns several, straight through the ABI:
    the list's own checks, then m == 0, then the tables' contents."""
    import ctypes
    L = gpu._lib.load()
    good = gpu.Table(oracle.sstable_create([(b"a", b"1"), (b"b", b"2")]))
    unsorted = gpu.Table(raw_file([(b"b", b64(b"1")), (b"a", b64(b"2"))]))
    assert not unsorted.well_formed

    def compact(handles, nt, m_bits):
        th, fh = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xbeef)
        arr = ctypes.cast((ctypes.c_void_p * 2)(*handles), ctypes.c_void_p)
        rc = L.cb_tables_compact(arr, nt, m_bits, None, ctypes.byref(th), ctypes.byref(fh))
        assert not th.value and not fh.value
        return rc, L.cb_last_error().decode()

    assert compact([good._h.value, None], 2, 0) == (CB_EINVAL, "null table")
    rc, msg = compact([good._h.value, unsorted._h.value], 2, 0)
    assert rc == gpu._lib.CB_EZEROM and msg == "attempt to calculate the remainder with a divisor of zero"
    assert compact([good._h.value, unsorted._h.value], 2, 1024) == (CB_EINVAL, "an input table is not well-formed")
    assert compact([good._h.value, None], 0, 0) == (CB_EINVAL, "no tables")


# ---- lifetime -----------------------------------------------------------------------

def test_pending_inputs_and_inputs_destroyed_at_once(gpu):
    rng = np.random.default_rng(11)
    pool = hex_keys(rng, 6000)
    entries, files = [], []
    for t in range(4):
        ks = [pool[i] for i in rng.choice(len(pool), 5000, replace=False)]  # unsorted: past 4096, the bin sort
        e = [(k, named(t, k)) for k in ks]
        entries.append(e)
        files.append(oracle.sstable_create(e))
    tables = [gpu.sstable_create(e, wait=False)[0] for e in entries]  # not waited on
    want, filt, zone, kept, otables = expected(files, 1024)
    merged, bloom, z = gpu.compact(tables)
    assert [t.data() for t in tables] == files, "an input changed"
    for t in tables:
        t.close()
    del tables
    # the pool hands the inputs' blocks out again
    churn = [gpu.sstable_create(entries[0])[0] for _ in range(3)]
    assert merged.data() == want
    assert np.array_equal(bloom.bools(), filt.bools()) and (z.min, z.max) == zone
    kd, ko = ragged(kept[:2000])
    ow, ovoff, ovals = oracle.get_many(otables, None, kd, ko)
    which, voff, vals = gpu.get_many([merged], kept[:2000])
    assert np.array_equal(which >= 0, ow >= 0) and np.array_equal(voff, ovoff) and vals == ovals
    del churn


def test_compacting_in_steps_equals_compacting_at_once(gpu):
    rng = np.random.default_rng(12)
    pool = hex_keys(rng, 1500)
    files = overlap_files(6, pool, rng, lo=200, hi=700)
    files[3] = raw_file(sorted((k, b"!") for k in file_keys(files[3])[::2]) )  # spoiled lines in the old half too
    tables = [gpu.Table(f) for f in files]
    old, _, _ = gpu.compact(tables[2:])
    stepped, b1, z1 = gpu.compact(tables[:2] + [old])
    at_once, b2, z2, want = check(gpu, files, tables=tables)
    assert stepped.data() == want == at_once.data()
    assert np.array_equal(b1.bools(), b2.bools()) and z1 == z2


# ---- downstream ---------------------------------------------------------------------

def test_merged_table_downstream(gpu):
    rng = np.random.default_rng(13)
    pool = hex_keys(rng, 2500)
    files = overlap_files(9, pool, rng, lo=100, hi=256)
    m = 4096
    merged, bloom, z, want = check(gpu, files, m=m)
    _, filt, zone, kept, otables = expected(files, m)
    # in a FilterSet slot, through cb_set_get_many_var
    fset = gpu.FilterSet.from_filters([bloom])
    fset.set_zone(0, z)
    look = kept + absent_keys(kept, rng)
    kd, ko = ragged(look)
    ow, ovoff, ovals = oracle.get_many(otables, None, kd, ko)
    which, voff, vals = gpu.get_many([merged], look, filterset=fset)
    assert np.array_equal(which >= 0, ow >= 0) and np.array_equal(voff, ovoff) and vals == ovals
    # SsTable::load's rebuild of the merged file
    b2, z2 = merged.rebuild(m)
    assert np.array_equal(b2.bools(), filt.bools()) and (z2.min, z2.max) == zone
    # its .meta
    meta = gpu.TableMeta(bloom, z).encode()
    assert meta == oracle.meta_encode(filt, oracle.OracleZone(*zone))
    back = gpu.TableMeta.decode(meta)
    assert np.array_equal(back.bloom.bools(), filt.bools()) and (back.zone_map.min, back.zone_map.max) == zone
    # the line index: every line's start, key length and length
    st, kl, ll = merged.lines()
    lines = [ln for ln in want.split(b"\n") if ln]
    assert list(ll) == [len(ln) for ln in lines] and list(kl) == [len(k) for k in kept]
    assert list(st) == list(np.cumsum([0] + [len(ln) + 1 for ln in lines[:-1]]))
    assert np.array_equal(merged.search(kept[:50] + [b"nope"]), np.array(list(range(50)) + [-1]))
