"""cb_tables_scan_many / cb_tables_scan_prefixes: many disjoint ranges or
prefixes answered by one merge on the device.

The contract: for tables T[0..nt), T[0] newest, and ascending, pairwise
disjoint ranges R_0 .. R_{nr-1}, the result holds the entries of
cb_tables_scan(T, lo_r, hi_r, limit = 0) for r = 0, 1, ... one after the
other, and range_off[0..nr] says where each range's entries begin. Every
expectation here comes from the C oracle, as in tests/test_scan_gpu.py
(oracle.get_many over the input files for the sorted keys of their lines, then
a plain filter per range, concatenated, range_off from the lengths); every
comparison is exact.

Shapes are the smallest at which each changed kernel can go wrong. A block of
k_scan_bounds holds 8 cuts (256 lanes, 16 per search, two searches per cut)
and a wave 2, so the grid is tried at 1, 7, 8, 9 and 17 cuts; k_scan_sources
walks the cuts 256 at a time, so 255, 256 and 257 cuts, all of them sources
and most of them empty; k_scan_emit and k_scan_range_off at range boundaries
on both sides of the 256-record tile edge, with empty ranges at the ends and
in a row; the sort at 4096 and 4097 lines inside the ranges.
"""
import ctypes

import numpy as np
import pytest

from merge_help import b64, BAD, file_keys, hex_keys, named, open_tables, oracle_prefix_end, ragged, raw_file, TILE
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1


# ---- the reference and the checks (shared helpers: tests/merge_help.py) ----

class Ref:
    """The oracle's answer for every key of `files` (newest first), computed
    once: Database::get's walk over the files for the sorted keys of their
    lines. A range's expectation is that list cut to the range."""

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

    def expect(self, lo=b"", hi=None):
        return [x for x in self.entries if lo <= x[0] and (hi is None or x[0] < hi)]

    def expect_many(self, ranges):
        """(entries of every range one after the other, range_off)."""
        parts = [self.expect(lo, hi) for lo, hi in ranges]
        off = np.zeros(len(ranges) + 1, np.uint64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return [x for p in parts for x in p], off


def assert_result(r, want, what=""):
    """r holds exactly the entries `want` = [(key, value, which)], untruncated."""
    assert r.count == len(want), f"{what}: {r.count} entries against {len(want)}"
    assert r.truncated is False, what
    ko, kb, vo, vb = r.raw()
    eko, evo = ragged([k for k, _, _ in want])[1], ragged([v for _, v, _ in want])[1]
    assert np.array_equal(ko, eko), f"{what}: key offsets differ"
    assert kb.tobytes() == b"".join(k for k, _, _ in want), f"{what}: keys differ"
    assert np.array_equal(vo, evo), f"{what}: value offsets differ"
    assert vb.tobytes() == b"".join(v for _, v, _ in want), f"{what}: values differ"
    assert r.which().tolist() == [w for _, _, w in want], f"{what}: sources differ"
    assert (r.key_bytes, r.val_bytes) == (int(eko[-1]), int(evo[-1])), what


def brief(ranges):
    return [(lo[:12], None if hi is None else hi[:12]) for lo, hi in ranges[:8]]


def check_many(gpu, ref, tables, ranges=None, prefixes=None, stream=None):
    if prefixes is not None:
        r = gpu.scan_many(tables, prefixes=prefixes, stream=stream)
        ranges = [(p, oracle_prefix_end(p)) for p in prefixes]
    else:
        r = gpu.scan_many(tables, ranges=ranges, stream=stream)
    want, off = ref.expect_many(ranges)
    what = f"{len(ranges)} ranges {brief(ranges)}"
    assert r.nranges == len(ranges), what
    assert np.array_equal(r.range_off(), off), f"{what}: range offsets {r.range_off().tolist()} against {off.tolist()}"
    assert_result(r, want, what)
    return r, want, off


def ranges_from(bounds, last_unbounded=False):
    """Sorted bounds taken in pairs: ascending, disjoint (touching where two
    bounds are equal, empty where a pair is)."""
    b = sorted(bounds)
    out = [(b[2 * i], b[2 * i + 1]) for i in range(len(b) // 2)]
    if last_unbounded:
        out[-1] = (out[-1][0], None)
    return out


def raw_many(L, handles, parts, nr, last_unbounded=0, stream=None):
    """cb_tables_scan_many straight through the ABI: (rc, *out)."""
    out = ctypes.c_void_p(0xDEAD)
    arr = ctypes.cast((ctypes.c_void_p * len(handles))(*handles), ctypes.c_void_p)
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    rc = L.cb_tables_scan_many(arr, len(handles), b"".join(parts), off.ctypes.data, nr, last_unbounded, stream,
                               ctypes.byref(out))
    return rc, out.value


# ---- k_scan_bounds: the grid over (range, table) ----------------------------------------

def bound_spots(rng, pool, n):
    """n bounds: at keys, between keys, below the first key and above the last."""
    picks = [pool[i] for i in rng.choice(len(pool), n, replace=True)]
    spots = [k if i % 2 else k + b"\0" for i, k in enumerate(picks)]
    spots[0] = pool[0][:-1] if rng.integers(0, 2) else b""
    spots[-1] = pool[-1] + b"\xff"
    return spots


@pytest.mark.parametrize("nt,nr", [(1, 1), (7, 1), (1, 8), (3, 3), (17, 1)])
def test_bounds_grid(gpu, nt, nr):
    """nt x nr = 1, 7, 8, 9 and 17 cuts: less than a wave, a block less one
    cut, a full block, one cut into the next, three blocks."""
    rng = np.random.default_rng(100 * nt + nr)
    pool = sorted(hex_keys(rng, 200, 8))
    files = [oracle.sstable_create([(pool[i], named(t, pool[i][:3])) for i in rng.choice(len(pool), 40, replace=False)])
             for t in range(nt)]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    for trial in range(6):
        spots = bound_spots(rng, pool, 2 * nr)
        check_many(gpu, ref, tables, ranges=ranges_from(spots))
        check_many(gpu, ref, tables, ranges=ranges_from(spots, last_unbounded=True))
    r, want, off = check_many(gpu, ref, tables, ranges=ranges_from([b""] + [pool[len(pool) * i // nr] for i in range(1, nr)] * 2
                                                                  + [b"g"]))
    assert r.count == len(ref.entries)  # touching ranges that cover every key


def test_bounds_over_table_sizes(gpu):
    """3 ranges x 5 tables of 1, 15, 16, 17 and 300 lines: the fence fan-out
    and the directory threshold, a cut's table found as c % nt."""
    rng = np.random.default_rng(15)
    pool = sorted(hex_keys(rng, 500, 8))
    files = [oracle.sstable_create([(pool[i], named(t, pool[i][:4])) for i in rng.choice(len(pool), n, replace=False)])
             for t, n in enumerate([1, 15, 16, 17, 300])]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    assert [t.nlines for t in tables] == [1, 15, 16, 17, 300]
    only = file_keys(files[0])[0]
    for trial in range(8):
        spots = bound_spots(rng, pool, 6)
        check_many(gpu, ref, tables, ranges=ranges_from(spots))
        check_many(gpu, ref, tables, ranges=ranges_from(spots, last_unbounded=True))
    # the one-line table's key as a bound, a touching point and inside a range
    check_many(gpu, ref, tables, ranges=[(b"", only), (only, only + b"\0"), (only + b"\0", None)])
    check_many(gpu, ref, tables, ranges=ranges_from([b"", pool[3], pool[3], only + b"\0", pool[-2], b"g"]))


# ---- k_scan_sources: 255, 256 and 257 cuts ----------------------------------------------

def namespace_files(rng, nt, nr, per, live=lambda t, r: True):
    """nt tables, each with `per` keys under every prefix "r%02d:" for which
    live(t, r), and a line below and above every prefix. Keys repeat across
    tables (4 suffixes per prefix and table out of 12)."""
    files = []
    for t in range(nt):
        e = [(b"a-low%d" % (t % 3), named(t, b"lo")), (b"z-high%d" % (t % 2), named(t, b"hi"))]
        for r in range(nr):
            if live(t, r):
                e += [(b"r%02d:%02d" % (r, i), named(t, b"%d" % i)) for i in rng.choice(12, per, replace=False).tolist()]
        files.append(oracle.sstable_create(e))
    return files


@pytest.mark.parametrize("nt,nr", [(17, 15), (16, 16), (257, 1)])
def test_sources_every_cut_non_empty(gpu, nt, nr):
    rng = np.random.default_rng(nt * nr)
    files = namespace_files(rng, nt, nr, 2)
    ref = Ref(files)
    tables = open_tables(gpu, files)
    prefixes = [b"r%02d:" % r for r in range(nr)]
    r, want, off = check_many(gpu, ref, tables, prefixes=prefixes)
    assert all(off[i + 1] > off[i] for i in range(nr))
    assert set(r.which().tolist()) <= set(range(nt)) and 0 in r.which().tolist()


@pytest.mark.parametrize("nt,nr", [(17, 15), (16, 16), (257, 1)])
def test_sources_most_cuts_empty(gpu, nt, nr):
    """Ranges that miss most tables, and tables without lines in the list (they
    take no cut, so the cut counts stay 255, 256 and 257)."""
    rng = np.random.default_rng(nt * nr + 1)
    files = namespace_files(rng, nt, nr, 3, live=lambda t, r: ((t * 7 + r) % 16 == 3 and r % 4 != 1) or (nr == 1 and t in (0, 130, 256)))
    files = files[:5] + [b""] + files[5:] + [b"", b""]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    prefixes = [b"r%02d:" % r for r in range(nr)]
    r, want, off = check_many(gpu, ref, tables, prefixes=prefixes)
    assert 0 < r.count < 12 * nr + 1
    if nr > 1:
        assert any(off[i + 1] == off[i] for i in range(nr))  # some range has no line in any table


# ---- k_scan_emit / k_scan_range_off: where the ranges begin -----------------------------

def test_empty_ranges_first_last_and_in_a_row(gpu):
    files = namespace_files(np.random.default_rng(6), 3, 2, 5)
    ref = Ref(files)
    tables = open_tables(gpu, files)
    ranges = [(b"b", b"c"),            # no line inside, first
              (b"r00:", b"r00;"),
              (b"r00;", b"r00;"),      # lo == hi
              (b"r00<", b"r01"),       # no line inside: two empty ranges in a row
              (b"r01:", b"r01;"),
              (b"r02", b"r03")]        # no line inside, last
    r, want, off = check_many(gpu, ref, tables, ranges=ranges)
    assert [int(off[i + 1] - off[i]) > 0 for i in range(6)] == [False, True, False, False, True, False]
    # every range empty: by its bounds (no device work), and by the data
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"c", b"b"), (b"c", b"c"), (b"d", b"d")])
    assert r.count == 0 and r.range_off().tolist() == [0, 0, 0, 0]
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"b", b"c"), (b"d", b"e"), (b"r05", b"r06")])
    assert r.count == 0 and r.nranges == 3
    # no live table at all
    r, want, off = check_many(gpu, Ref([b"", b""]), open_tables(gpu, [b"", b""]), ranges=[(b"a", b"b"), (b"b", None)])
    assert r.count == 0 and r.range_off().tolist() == [0, 0, 0]


def test_a_range_whose_lines_all_fail_to_decode(gpu):
    """The middle range has cuts in both tables and no survivor; then a list
    in which no range has one."""
    newer = raw_file([(b"a:1", b64(b"n1")), (b"d:1", b"QQ="), (b"d:2", b"*"), (b"e:1", b64(b"n2"))])
    older = raw_file([(b"a:1", b64(b"o1")), (b"a:2", b64(b"o2")), (b"d:1", b"A"), (b"d:3", b"===="), (b"e:2", b64(b"o3"))])
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    r, want, off = check_many(gpu, ref, tables, prefixes=[b"a:", b"d:", b"e:"])
    assert off.tolist() == [0, 2, 2, 4]
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"d:", b"d:2"), (b"d:2", b"d;")])
    assert r.count == 0 and off.tolist() == [0, 0, 0]


def survivors_files(rng, counts):
    """Two tables; namespace j ("n%d:") ends with counts[j] survivors: the
    older table holds every key, the newer every second one and, undecodable,
    a few keys that survive through the older one or nowhere."""
    newer, older = [], []
    for j, c in enumerate(counts):
        ks = sorted(b"n%d:" % j + k for k in hex_keys(rng, c + 6, 8))[:c + 4]
        assert len(ks) == c + 4
        keep, dead = ks[:c], ks[c:]
        older += [(k, b64(named(1, k[-3:]))) for k in keep] + [(k, b"QQ=") for k in dead[::2]]
        newer += [(k, b64(named(0, k[-3:]))) for k in keep[::2]] + [(k, b"!bad") for k in dead] + \
                 [(k, b"QR==") for k in keep[1::8]]
    return [raw_file(sorted(newer)), raw_file(sorted(older))]


@pytest.mark.parametrize("first", [255, 256, 257])
def test_range_boundary_at_the_emit_tile_edge(gpu, first):
    """The second range begins at survivor rank 255, 256 and 257."""
    files = survivors_files(np.random.default_rng(first), [first, 3, 1])
    ref = Ref(files)
    tables = open_tables(gpu, files)
    assert all(t.well_formed for t in tables)
    r, want, off = check_many(gpu, ref, tables, prefixes=[b"n0:", b"n1:", b"n2:"])
    assert off.tolist() == [0, first, first + 3, first + 4]
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"n0:", b"n1:"), (b"n1:", b"n1;"), (b"n1;", None)])
    assert off.tolist() == [0, first, first + 3, first + 4]


def test_one_range_over_three_tiles_between_two_single_entries(gpu):
    files = survivors_files(np.random.default_rng(9), [1, 2 * TILE + 40, 1])
    ref = Ref(files)
    tables = open_tables(gpu, files)
    r, want, off = check_many(gpu, ref, tables, prefixes=[b"n0:", b"n1:", b"n2:"])
    assert off.tolist() == [0, 1, 2 * TILE + 41, 2 * TILE + 42]


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_a_tile_of_under_four_key_bytes_at_every_alignment(gpu, start):
    """One table of 600 lines in two ranges. The second emit tile (records 256
    to 511) holds one survivor, a key of 1 to 3 bytes among 255 lines that do
    not decode, and its keys begin `start` bytes past a dword of the result's
    keys: the tile is all head, or all tail, or both, and has no whole dword."""
    short = b"b" * (1 + start % 3)
    lines = [(b"a%03d" % i + b"x" * (start if i == 7 else 0), b64(b"v%d" % i)) for i in range(TILE)]
    lines += [(short, b64(b"short"))] + [(b"b~%03d" % i, BAD) for i in range(TILE - 1)]
    lines += [(b"c%03d" % i, b64(b"w%d" % i)) for i in range(88)]
    assert len(lines) == 600 and lines == sorted(lines) and lines[TILE][0] == short
    files = [raw_file(lines)]
    ref = Ref(files)
    r, want, off = check_many(gpu, ref, open_tables(gpu, files), ranges=[(b"", b"b~"), (b"b~", None)])
    assert off.tolist() == [0, TILE + 1, TILE + 1 + 88]
    ko = r.raw()[0]
    assert want[TILE][0] == short and int(ko[TILE]) % 4 == start and int(ko[TILE + 1] - ko[TILE]) < 4


# ---- touching ranges and runs of one key ------------------------------------------------

def test_a_key_at_a_touching_bound_in_every_table(gpu):
    """k is in all five tables and is hi of one range and lo of the next; the
    newest table's value for it does not decode, so the second newest wins. k
    appears once, in the later range."""
    k = b"m:key"
    files = [raw_file(sorted([(k, b"QQ=" if t == 0 else b64(named(t, b"k"))), (b"a:%d" % t, b64(b"a")),
                              (b"m:%d" % t, b64(b"m")), (b"z:%d" % t, b64(b"z"))])) for t in range(5)]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"a", k), (k, b"zz")])
    got = list(zip(r.keys(), r.values(), r.which().tolist()))
    assert got.count((k, b"t1:k", 1)) == 1 and [x[0] for x in got].count(k) == 1
    assert int(off[1]) <= r.keys().index(k) < int(off[2])
    # k as the first range's lo, and alone in a range between two others
    r, want, off = check_many(gpu, ref, tables, ranges=[(k, b"n"), (b"n", b"zz")])
    assert r.keys()[0] == k and r.which()[0] == 1
    r, want, off = check_many(gpu, ref, tables, ranges=[(b"", k), (k, k + b"\0"), (k + b"\0", None)])
    assert off[2] - off[1] == 1 and r.count == len(ref.entries)


# ---- long and ragged keys at the bounds -------------------------------------------------

def test_long_and_ragged_keys_at_the_bounds(gpu):
    """Keys that share 8 and 16 leading bytes (and 40), with range bounds inside
    those runs; bounds of 0, 1, 8, 16, 17 and 40 bytes."""
    rng = np.random.default_rng(77)
    pool = set()
    while len(pool) < 180:
        i = len(pool) % 4
        h = rng.integers(0, 256, 6, dtype=np.uint8).tobytes().hex().encode()
        pool.add(h if i == 0 else (b"samepfx8" + h[:int(rng.integers(0, 9))]) if i == 1
                 else (b"sixteen-byte-pfx" + h[:int(rng.integers(0, 12))]) if i == 2
                 else b"forty-bytes-of-shared-prefix-for-a-key--" + h[:int(rng.integers(0, 6))])
    ks = sorted(pool)
    files = [oracle.sstable_create([(k, named(t, k[-3:])) for k in sorted(set(ks[t::2] + ks[::5]))]) for t in range(2)]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    same8 = [k for k in ks if k.startswith(b"samepfx8")]
    same16 = [k for k in ks if k.startswith(b"sixteen-byte-pfx")]
    same40 = [k for k in ks if k.startswith(b"forty-bytes")]
    bounds = [b"", b"f", b"samepfx8", b"sixteen-byte-pfx", b"sixteen-byte-pfx5",
              b"forty-bytes-of-shared-prefix-for-a-key--",
              same8[len(same8) // 2], same8[-1] + b"\0", same16[len(same16) // 3], same16[-2], same40[1], same40[-1]]
    assert {0, 1, 8, 16, 17, 40} <= {len(b) for b in bounds}
    for trial in range(10):
        pick = [bounds[i] for i in rng.choice(len(bounds), 8, replace=False)]
        check_many(gpu, ref, tables, ranges=ranges_from(pick))
        check_many(gpu, ref, tables, ranges=ranges_from(pick, last_unbounded=True))
    check_many(gpu, ref, tables, ranges=ranges_from(bounds))
    check_many(gpu, ref, tables, ranges=[(a, b) for a, b in zip(sorted(bounds), sorted(bounds)[1:])])  # all touching


# ---- both sides of the key sort's plan --------------------------------------------------

@pytest.mark.parametrize("total", [4096, 4097])
def test_lines_inside_the_ranges_at_the_sort_threshold(gpu, total):
    """`total` lines inside 8 ranges over 4 tables (with lines outside them):
    the merge sort's last size and the bin sort's first."""
    rng = np.random.default_rng(total)
    per = [total // 4 + (1 if t < total % 4 else 0) for t in range(4)]
    pool = hex_keys(rng, 3000, 10)
    files = []
    for t, n in enumerate(per):
        ks = [b"%d:" % (i % 8) + pool[j] for i, j in enumerate(rng.choice(len(pool), n, replace=False))]
        out = [(b"8-out%d-%02d" % (t, i), b"o") for i in range(5)] + [(b"+below%d" % t, b"b")]
        files.append(oracle.sstable_create([(k, named(t, k[-4:])) for k in ks] + out))
    ref = Ref(files)
    tables = open_tables(gpu, files)
    prefixes = [b"%d:" % i for i in range(8)]
    assert sum(k[:2] in prefixes for f in files for k in file_keys(f)) == total
    r, want, off = check_many(gpu, ref, tables, prefixes=prefixes)
    assert r.count == sum(k[:2] in prefixes for k, _, _ in ref.entries) < total


# ---- equivalences -----------------------------------------------------------------------

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


def parts_of(r):
    return r.count, r.key_bytes, r.val_bytes, r.truncated, [x.tobytes() for x in r.raw()], r.which().tolist()


def test_one_range_equals_the_single_scan(gpu, store):
    ref, tables = store
    for lo, hi in [(b"3", b"c"), (b"3", None), (b"", None), (b"", b"8"), (b"c", b"3")]:
        many, want, off = check_many(gpu, ref, tables, ranges=[(lo, hi)])
        one = gpu.scan(tables, lo=lo, hi=hi)
        assert parts_of(many) == parts_of(one), (lo, hi)
        # a result of the single entry reports one range, {0, count}
        assert one.nranges == 1 and one.range_off().tolist() == [0, one.count]
        assert many.range_off().tolist() == [0, one.count]
    full, want, off = check_many(gpu, ref, tables, ranges=[(b"", None)])
    merged, _, _ = gpu.compact(tables)
    assert full.keys() == file_keys(merged.data())  # the full range: the compacted file's lines
    limited = gpu.scan(tables, lo=b"3", hi=b"c", limit=7)
    assert limited.truncated and limited.nranges == 1 and limited.range_off().tolist() == [0, 7]
    by_prefix = gpu.scan(tables, prefix=b"4")
    assert by_prefix.nranges == 1 and by_prefix.range_off().tolist() == [0, by_prefix.count]


def test_sixteen_prefixes_equal_sixteen_prefix_scans(gpu, store):
    ref, tables = store
    prefixes = sorted(b"%02x" % v for v in np.random.default_rng(2).choice(256, 16, replace=False).tolist())
    many, want, off = check_many(gpu, ref, tables, prefixes=prefixes)
    singles = [gpu.scan(tables, prefix=p) for p in prefixes]
    assert off.tolist() == np.concatenate([[0], np.cumsum([s.count for s in singles])]).tolist()
    assert many.keys() == [k for s in singles for k in s.keys()]
    assert many.values() == [v for s in singles for v in s.values()]
    assert many.which().tolist() == [w for s in singles for w in s.which().tolist()]
    assert many.count > 16


# ---- refusals with real tables ----------------------------------------------------------

def test_refusals_leave_the_stream_usable(gpu, store):
    import torch
    ref, tables = store
    L = gpu._lib.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    handles = [t._h.value for t in tables]
    refused = [("overlap", [b"1", b"5", b"4", b"9"], 2, 0),
               ("overlap by the last byte", [b"1", b"50", b"5", b"9"], 2, 0),
               ("descending", [b"5", b"9", b"1", b"4"], 2, 0),
               ("touching the unbounded last from above", [b"1", b"6", b"5", b""], 2, 1),
               ("no ranges", [], 0, 0),
               ("past the cut cap", [b""] * (2 * 65537), 65537, 0)]
    for what, parts, nr, unb in refused:
        rc, out = raw_many(L, handles[:1] if nr > 100 else handles, parts, nr, unb, s)
        assert (rc, out) == (CB_EINVAL, None), what
        assert L.cb_last_error(), what
        check_many(gpu, ref, tables, ranges=[(b"1", b"4"), (b"5", b"9")], stream=stream)
    # the cap itself passes: 65536 cuts over the one table with lines, every range empty
    rc, out = raw_many(L, handles[:1], [b""] * (2 * 65536), 65536, 0, s)
    assert rc == 0 and out
    r = gpu.ScanResult(out, 0)
    assert (r.count, r.nranges) == (0, 65536) and not r.range_off().any()
    # nested and repeated prefixes, and a prefix without an end before the last
    for prefixes in ([b"a:", b"a:b:"], [b"4", b"4"], [b"4", b"3"], [b"", b"4"], [b"\xff", b"\xff\xff"]):
        with pytest.raises(gpu._lib.CassBloomError) as ei:
            gpu.scan_many(tables, prefixes=prefixes, stream=stream)
        assert ei.value.code == CB_EINVAL, prefixes
        check_many(gpu, ref, tables, prefixes=[b"3", b"4", b"\xff"], stream=stream)
    # an input that is not well-formed is refused as the single scan refuses it
    unsorted = gpu.Table(raw_file([(b"b", b64(b"1")), (b"a", b64(b"2"))]))
    with pytest.raises(gpu._lib.CassBloomError) as ei:
        gpu.scan_many([tables[0], unsorted], ranges=[(b"1", b"4"), (b"5", b"9")])
    assert ei.value.code == CB_EINVAL


# ---- lifetime ---------------------------------------------------------------------------

def test_result_outlives_inputs_on_a_side_stream(gpu):
    import torch
    rng = np.random.default_rng(31)
    pool = hex_keys(rng, 2000, 12)
    files = []
    for t in range(4):
        ks = [pool[i] for i in rng.choice(len(pool), 800, replace=False)]
        files.append(oracle.sstable_create([(k, named(t, k[:5])) for k in ks]))
    ref = Ref(files)
    tables = open_tables(gpu, files)
    stream = torch.cuda.Stream()
    ranges = [(b"1", b"3"), (b"3", b"30"), (b"5", b"a"), (b"c", None)]
    want, off = ref.expect_many(ranges)
    r = gpu.scan_many(tables, ranges=ranges, stream=stream)
    for t in tables:  # destroyed right after the call
        t.close()
    churn = open_tables(gpu, files)  # the pool hands their blocks out again
    assert r.nranges == 4 and np.array_equal(r.range_off(), off)
    assert_result(r, want, "after the inputs were closed")
    assert [t.data() for t in churn] == files
    r.close()
    r.close()
