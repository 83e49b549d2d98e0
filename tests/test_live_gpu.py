"""cb_tables_count, cb_tables_scan_live and cb_tables_compact_live: the
reference's deleted rows (tombstones) in the tables, on the device.

The contract. A decoded value is dead when the reference's split_ts leaves no
payload (src/query.rs:21-27: lengths 0 and 8). A tombstone shadows and is then
dropped: the newest line of a key that decodes decides, dead or not. So for
tables T[0..nt), T[0] newest, and a range r,
    entries[r] = len(cb_tables_scan(T, lo_r, hi_r)),
    live[r]    = how many of those entries are not dead,
cb_tables_scan_live is cb_tables_scan_many's result without the dead entries,
and cb_tables_compact_live is SsTable::create of the live entries.

Every expectation comes from the C oracle exactly as tests/test_scan_many_gpu.py
builds it (oracle.get_many over the input files for the sorted keys of their
lines: Database::get's walk), filtered here with the split_ts restatement in
tests/liverow_ref.py. Every comparison is exact.

Tables are hand-written files, so every value's text and decoded length is
explicit. Shapes are the smallest at which each kernel can go wrong: the
select's 256-record tile edge with a key's lines on both sides of it, and
k_scan_count's runs of equal ranges at record positions 255, 256 and 257 of
the sorted order (every line inside the ranges is a record, shadowed
duplicates and undecodable lines included), with 256 and 257 runs in a row,
a run over three tiles, and empty ranges at the ends and in a row.
"""
import base64
import ctypes

import numpy as np
import pytest

from liverow_ref import is_dead
from merge_help import b64, BAD, file_keys, hex_keys, open_tables, oracle_prefix_end, ragged, raw_file, row, TILE, tomb
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1


# ---- the reference and the checks (shared helpers: tests/merge_help.py) ----

class Ref:
    """The oracle's answer for every key of `files` (newest first), computed
    once, and the live rows among them."""

    def __init__(self, files):
        self.files = files
        self.otables = [oracle.OracleTable(f) for f in files]
        self.nlines = sum(len(file_keys(f)) for f in files)
        keys = sorted(set(k for f in files for k in file_keys(f)))
        self.all_keys = keys
        self.entries = []  # (key, value, which), found keys only, sorted
        if keys:
            kd, ko = ragged(keys)
            which, voff, vals = oracle.get_many(self.otables, None, kd, ko)
            self.entries = [(k, vals[int(voff[i]):int(voff[i + 1])], int(which[i]))
                            for i, k in enumerate(keys) if which[i] >= 0]
        self.live = [x for x in self.entries if not is_dead(x[1])]

    @staticmethod
    def cut(entries, lo=b"", hi=None):
        return [x for x in entries if lo <= x[0] and (hi is None or x[0] < hi)]

    def expect_many(self, ranges, live):
        """(entries of every range one after the other, range_off)."""
        parts = [self.cut(self.live if live else self.entries, lo, hi) for lo, hi in ranges]
        off = np.zeros(len(ranges) + 1, np.uint64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return [x for p in parts for x in p], off


def assert_result(r, want, what="", truncated=False):
    """r holds exactly the entries `want` = [(key, value, which)]."""
    assert r.count == len(want), f"{what}: {r.count} entries against {len(want)}"
    assert r.truncated is truncated, what
    ko, kb, vo, vb = r.raw()
    eko, evo = ragged([k for k, _, _ in want])[1], ragged([v for _, v, _ in want])[1]
    assert np.array_equal(ko, eko), f"{what}: key offsets differ"
    assert kb.tobytes() == b"".join(k for k, _, _ in want), f"{what}: keys differ"
    assert np.array_equal(vo, evo), f"{what}: value offsets differ"
    assert vb.tobytes() == b"".join(v for _, v, _ in want), f"{what}: values differ"
    assert r.which().tolist() == [w for _, _, w in want], f"{what}: sources differ"
    assert (r.key_bytes, r.val_bytes) == (int(eko[-1]), int(evo[-1])), what


def check_ranges(gpu, ref, tables, ranges=None, prefixes=None, stream=None):
    """count and scan_live over the ranges against the oracle. Returns
    (entries per range, live per range) as lists."""
    kw = {"prefixes": prefixes} if prefixes is not None else {"ranges": ranges}
    if prefixes is not None:
        ranges = [(p, oracle_prefix_end(p)) for p in prefixes]
    what = f"{len(ranges)} ranges from {ranges[0][0][:12]!r}"
    _, eoff = ref.expect_many(ranges, live=False)
    want, loff = ref.expect_many(ranges, live=True)
    entries, live = gpu.count(tables, stream=stream, **kw)
    assert entries.dtype == np.uint64 and live.dtype == np.uint64
    assert entries.tolist() == np.diff(eoff).tolist(), f"{what}: entries"
    assert live.tolist() == np.diff(loff).tolist(), f"{what}: live"
    r = gpu.scan_live(tables, stream=stream, **kw)
    assert r.nranges == len(ranges), what
    assert np.array_equal(r.range_off(), loff), f"{what}: range offsets {r.range_off().tolist()} against {loff.tolist()}"
    assert_result(r, want, what)
    return entries.tolist(), live.tolist()


def expected_compaction(ref, m):
    """(file, OracleFilter, (min, max) or None) of the live entries."""
    filt = oracle.OracleFilter(m)
    kept = [k for k, _, _ in ref.live]
    if kept:
        filt.insert_var(*ragged(kept))
    return (oracle.sstable_create([(k, v) for k, v, _ in ref.live]) if kept else b""), filt, \
        ((min(kept), max(kept)) if kept else None)


def check_compact_live(gpu, ref, tables, m=1024):
    """compact_live's file, line count, filter, zone bounds and reads."""
    want, filt, zone = expected_compaction(ref, m)
    merged, bloom, z = gpu.compact_live(tables, m=m)
    got = merged.data()
    assert got == want, f"merged file differs: {len(got)} bytes against {len(want)}"
    assert merged.nlines == len(ref.live)
    assert np.array_equal(bloom.bools(), filt.bools()), "filter bits differ from the oracle"
    assert (z.min, z.max) == (zone if zone else (None, None))
    if ref.all_keys:
        # every live key answers as over the inputs, every other key is not found
        which, voff, vals = gpu.get_many([merged], ref.all_keys)
        live = {k: v for k, v, _ in ref.live}
        assert (which >= 0).tolist() == [k in live for k in ref.all_keys], "found keys differ"
        assert vals == b"".join(live.get(k, b"") for k in ref.all_keys), "values differ"
        assert np.diff(voff).tolist() == [len(live.get(k, b"")) for k in ref.all_keys]
    return merged


def check_all(gpu, files, ranges=None, prefixes=None):
    """All three entries over the files: the ranges (default: everything, as
    one unbounded range), and the live compaction."""
    ref = Ref(files)
    tables = open_tables(gpu, files)
    assert all(t.well_formed for t in tables)
    if ranges is None and prefixes is None:
        ranges = [(b"", None)]
    e, lv = check_ranges(gpu, ref, tables, ranges=ranges, prefixes=prefixes)
    check_compact_live(gpu, ref, tables)
    return ref, tables, e, lv


def raw_count(L, handles, parts, nr, unb=0, entries=True, live=True, stream=None):
    """cb_tables_count straight through the ABI: (rc, entries or None, live or None)."""
    arr = ctypes.cast((ctypes.c_void_p * len(handles))(*handles), ctypes.c_void_p)
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    e, lv = np.full(max(nr, 1), 0xDEAD, np.uint64), np.full(max(nr, 1), 0xDEAD, np.uint64)
    rc = L.cb_tables_count(arr, len(handles), b"".join(parts), off.ctypes.data, nr, unb, stream,
                           e.ctypes.data if entries else None, lv.ctypes.data if live else None)
    return rc, e[:nr].tolist() if entries else None, lv[:nr].tolist() if live else None


# ---- value lengths at the rule's edges --------------------------------------------------

def test_value_lengths_at_the_rules_edges(gpu):
    """Decoded lengths 0, 1, 7, 8, 9 and 16 and a text that does not decode,
    one key each in one table: 0 and 8 are dead, the undecodable one is no
    entry at all."""
    vals = {0: b"", 1: b"x", 7: b"1234567", 8: (77).to_bytes(8, "big"), 9: (77).to_bytes(8, "big") + b"p",
            16: (78).to_bytes(8, "big") + b"payload!"}
    lines = [(b"k%02d" % n, b64(v)) for n, v in sorted(vals.items())] + [(b"k99", BAD)]
    assert all(len(v) == n for n, v in vals.items())
    ref, tables, e, lv = check_all(gpu, [raw_file(lines)])
    assert (e, lv) == ([6], [4])
    assert [k for k, _, _ in ref.live] == [b"k01", b"k07", b"k09", b"k16"]
    # each key a range of its own, the undecodable one included
    e, lv = check_ranges(gpu, ref, tables, ranges=[(k, k + b"\0") for k, _ in lines])
    assert e == [1, 1, 1, 1, 1, 1, 0] and lv == [0, 1, 1, 0, 1, 1, 0]


# ---- shadowing --------------------------------------------------------------------------

def shadow_files(nt):
    """nt = 2 or 3 tables, newest first: one key per case of the shadowing rule."""
    live0, live1, live2 = row(30, b"new"), row(20, b"mid"), row(10, b"old")
    t0 = [(b"a:dead-over-live", tomb(31)), (b"b:live-over-dead", live0), (b"e:all-dead", tomb(32)),
          (b"f:all-bad", BAD), (b"g:plain", live0)]
    t1 = [(b"a:dead-over-live", live1), (b"b:live-over-dead", tomb(21)), (b"e:all-dead", b""),
          (b"f:all-bad", b"*"), (b"h:plain-older", live1)]
    if nt == 2:
        t0 += [(b"c:bad-over-dead", BAD)]
        t1 += [(b"c:bad-over-dead", tomb(22)), (b"d:dead-in-oldest", tomb(23))]
        return [raw_file(sorted(t0)), raw_file(sorted(t1))]
    t0 += [(b"c:bad-over-dead-over-live", BAD)]
    t1 += [(b"c:bad-over-dead-over-live", tomb(22))]
    t2 = [(b"a:dead-over-live", live2), (b"c:bad-over-dead-over-live", live2), (b"d:dead-in-oldest", tomb(11)),
          (b"e:all-dead", tomb(12)), (b"f:all-bad", b"===="), (b"b:live-over-dead", live2)]
    return [raw_file(sorted(t0)), raw_file(sorted(t1)), raw_file(sorted(t2))]


@pytest.mark.parametrize("nt", [2, 3])
def test_shadowing(gpu, nt):
    files = shadow_files(nt)
    ref, tables, e, lv = check_all(gpu, files)
    assert [k[:1] for k, _, _ in ref.entries] == [b"a", b"b", b"c", b"d", b"e", b"g", b"h"]
    assert [k[:1] for k, _, _ in ref.live] == [b"b", b"g", b"h"]  # no older value comes back
    assert (e, lv) == ([7], [3])
    e, lv = check_ranges(gpu, ref, tables, prefixes=[b"a:", b"b:", b"c:", b"d:", b"e:", b"f:", b"g:", b"h:"])
    assert e == [1, 1, 1, 1, 1, 0, 1, 1]  # a tombstone counts in entries; undecodable everywhere: no entry
    assert lv == [0, 1, 0, 0, 0, 0, 1, 1]
    # the existing entries on the same inputs still return the tombstones
    want, off = ref.expect_many([(b"", None)], live=False)
    assert_result(gpu.scan(tables), want, "scan")
    assert_result(gpu.scan_many(tables, prefixes=[b"a:", b"e:"]), Ref.cut(ref.entries, b"a:", b"a;") +
                  Ref.cut(ref.entries, b"e:", b"e;"), "scan_many")
    merged, _, _ = gpu.compact(tables)
    assert merged.data() == oracle.sstable_create([(k, v) for k, v, _ in ref.entries])
    assert any(is_dead(v) for _, v, _ in want)


# ---- no resurrection at the select's tile edge ------------------------------------------

@pytest.mark.parametrize("before", [TILE - 2, TILE - 1, TILE])
def test_a_dead_newest_line_at_the_select_tile_edge(gpu, before):
    """Key K has a line in each of three tables, the newest dead, the older
    two live; `before` records sort below it, so the dead record is lane 254,
    255 or 0 of a tile and the live ones follow, across the tile's edge when
    it is lane 254 or 255. K stays deleted."""
    fill = [(b"a%04d" % i, row(5, b"f%d" % i)) for i in range(before)]
    after = [(b"z%02d" % i, row(6, b"z")) for i in range(3)]
    files = [raw_file([(b"m:K", tomb(9))] + after[:1]),
             raw_file(sorted(fill[::2] + [(b"m:K", row(8, b"older"))] + after[1:])),
             raw_file(sorted(fill[1::2] + [(b"m:K", row(7, b"oldest"))]))]
    ref, tables, e, lv = check_all(gpu, files)
    assert (e, lv) == ([before + 4], [before + 3])
    assert b"m:K" not in [k for k, _, _ in ref.live] and (b"m:K", (9).to_bytes(8, "big"), 0) in ref.entries
    e, lv = check_ranges(gpu, ref, tables, ranges=[(b"", b"m:K"), (b"m:K", b"m:K\0"), (b"m:K\0", None)])
    assert (e, lv) == ([before, 1, 3], [before, 0, 3])


def test_a_run_of_300_lines_with_the_dead_line_first(gpu):
    """K in 300 tables, dead in the newest and live in all others, with 250
    records before it: the run covers records 250..549, a whole tile and parts
    of two more, and every live line must see the dead one."""
    fill = [(b"a%04d" % i, row(5, b"f")) for i in range(250)]
    files = [raw_file([(b"m:K", tomb(1000))])]
    files += [raw_file([(b"m:K", row(1000 - t, b"v%d" % t))]) for t in range(1, 299)]
    files += [raw_file(sorted(fill + [(b"m:K", row(1, b"first")), (b"z", tomb(2))]))]
    assert len(files) == 300
    ref, tables, e, lv = check_all(gpu, files)
    assert (e, lv) == ([252], [250]) and ref.nlines == 551
    # and with a live newest line the key is live, whatever lies below
    files[0] = raw_file([(b"m:K", row(1001, b"back"))])
    ref, tables, e, lv = check_all(gpu, files)
    assert (e, lv) == ([252], [251])


# ---- k_scan_count at its edges ----------------------------------------------------------

def text_of(i, newer):
    """A mix of live rows, both dead lengths and undecodable texts by line number."""
    if newer:
        return tomb(i) if i % 3 == 0 else BAD if i % 3 == 1 else row(i, b"n%d" % i)
    return tomb(i) if i % 5 == 0 else b"" if i % 7 == 0 else b"!bad" if i % 11 == 3 else row(i, b"o%d" % i)


def record_files(rng, recs):
    """Two tables; namespace j ("n%d:") holds exactly recs[j] lines: the older
    table about three quarters of them, one per key, the newer one the rest,
    on keys of the older (so those are shadowed duplicates)."""
    newer, older = [], []
    for j, total in enumerate(recs):
        dup = total // 4
        ks = sorted(b"n%d:" % j + k for k in hex_keys(rng, total + 8, 8))[:total - dup]
        assert len(ks) == total - dup
        older += [(k, text_of(i, False)) for i, k in enumerate(ks)]
        newer += [(k, text_of(i, True)) for i, k in enumerate(ks[1::3][:dup])]
        assert len(ks[1::3]) >= dup
    return [raw_file(sorted(newer)), raw_file(sorted(older))]


def check_records(gpu, recs, seed):
    files = record_files(np.random.default_rng(seed), recs)
    ref = Ref(files)
    assert ref.nlines == sum(recs)
    tables = open_tables(gpu, files)
    prefixes = [b"n%d:" % j for j in range(len(recs))]
    e, lv = check_ranges(gpu, ref, tables, prefixes=prefixes)
    # the same as touching ranges that cover every key, the last one unbounded
    ranges = [(b"" if j == 0 else prefixes[j], prefixes[j + 1] if j + 1 < len(recs) else None) for j in range(len(recs))]
    assert check_ranges(gpu, ref, tables, ranges=ranges) == (e, lv)
    return ref, tables, e, lv


@pytest.mark.parametrize("first", [TILE - 1, TILE, TILE + 1])
def test_count_range_boundary_at_the_tile_edge(gpu, first):
    """The second range's first record is record 255, 256 and 257."""
    ref, tables, e, lv = check_records(gpu, [first, 5, 2], first)
    assert all(0 < b < a for a, b in zip(e[:2], lv[:2]))  # live, dead and shadowed lines in the ranges at the edge


def test_count_one_range_over_three_tiles_between_two_single_records(gpu):
    ref, tables, e, lv = check_records(gpu, [1, 2 * TILE + 40, 1], 9)
    assert e[1] > TILE and 0 < lv[1] < e[1]


@pytest.mark.parametrize("nr", [TILE, TILE + 1])
def test_count_every_lane_ends_a_run(gpu, nr):
    """256 and 257 one-record ranges in a row, from record 0 on."""
    lines = [(b"k%03d:x" % i, text_of(i, False)) for i in range(nr)]
    files = [raw_file(lines)]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    e, lv = check_ranges(gpu, ref, tables, prefixes=[b"k%03d:" % i for i in range(nr)])
    assert set(e) == {0, 1} and set(lv) == {0, 1} and sum(lv) < sum(e) < nr


def test_count_empty_dead_and_undecodable_ranges(gpu):
    newer = raw_file([(b"a:1", row(9, b"n1")), (b"d:1", BAD), (b"d:2", b"*"), (b"e:1", tomb(9)), (b"g:1", row(9, b"g"))])
    older = raw_file([(b"a:1", tomb(1)), (b"a:2", row(1, b"o2")), (b"d:1", b"A"), (b"d:3", b"===="), (b"e:1", row(1, b"x")),
                      (b"e:2", b""), (b"g:2", tomb(2))])
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    ranges = [(b"0", b"1"),           # no line inside, first
              (b"a:", b"a;"),
              (b"b", b"b"),           # lo == hi
              (b"b", b"c"), (b"c", b"d"), (b"d", b"d"),  # three empty ranges in a row
              (b"d:", b"d;"),         # every line undecodable: 0, 0
              (b"e:", b"e;"),         # every entry dead: entries > 0, live 0
              (b"g:", b"g;"),
              (b"h", b"i")]           # no line inside, last
    e, lv = check_ranges(gpu, ref, tables, ranges=ranges)
    assert e == [0, 2, 0, 0, 0, 0, 0, 2, 2, 0] and lv == [0, 2, 0, 0, 0, 0, 0, 0, 1, 0]
    # every range empty: by its bounds (no device work), and by the data
    assert check_ranges(gpu, ref, tables, ranges=[(b"c", b"b"), (b"c", b"c"), (b"d", b"d")]) == ([0] * 3, [0] * 3)
    assert check_ranges(gpu, ref, tables, ranges=[(b"b", b"c"), (b"h", b"i")]) == ([0] * 2, [0] * 2)
    # no table with lines; no range
    empty = open_tables(gpu, [b"", b""])
    assert check_ranges(gpu, Ref([b"", b""]), empty, ranges=[(b"a", b"b"), (b"b", None)]) == ([0, 0], [0, 0])
    e0, l0 = gpu.count(tables, ranges=[])
    assert e0.shape == (0,) and l0.shape == (0,)
    # entries alone, live alone and both; one unbounded range
    L = gpu._lib.load()
    handles = [t._h.value for t in tables]
    parts = [b for r in ranges for b in r]
    assert raw_count(L, handles, parts, len(ranges)) == (0, e, lv)
    assert raw_count(L, handles, parts, len(ranges), live=False) == (0, e, None)
    assert raw_count(L, handles, parts, len(ranges), entries=False) == (0, None, lv)
    assert raw_count(L, handles, [b"", b""], 1, unb=1) == (0, [len(ref.entries)], [len(ref.live)])
    assert (len(ref.entries), len(ref.live)) == (6, 3)
    check_compact_live(gpu, ref, tables)


# ---- agreement with the existing entries ------------------------------------------------

STORE_PREFIXES = [b"0", b"3", b"4", b"7f", b"a", b"f"]


@pytest.fixture(scope="module")
def store(gpu):
    """17 tables x 300 hex-key lines, about a quarter tombstones and some
    undecodable values: (ref, tables)."""
    rng = np.random.default_rng(1207)
    pool = hex_keys(rng, 1600, 10)
    files = []
    for t in range(17):
        lines = []
        for i in rng.choice(len(pool), 300, replace=False).tolist():
            u = rng.random()
            text = tomb(1000 - t) if u < 0.22 else b"" if u < 0.25 else BAD if u < 0.30 else \
                row(1000 - t, b"t%d:" % t + pool[i][:int(rng.integers(0, 9))])
            lines.append((pool[i], text))
        files.append(raw_file(sorted(lines)))
    ref = Ref(files)
    key_sets = [set(file_keys(f)) for f in files]
    # the oracle leaves live, dead and shadowed keys in every tested range
    for p in STORE_PREFIXES:
        ents = Ref.cut(ref.entries, p, oracle_prefix_end(p))
        dead = [k for k, v, _ in ents if is_dead(v)]
        assert len(ents) > len(dead) > 0, p
        assert any(sum(k in s for s in key_sets) > 1 for k in dead), p  # a dead key that shadows older lines
        assert any(w > 0 for _, _, w in ents), p  # an entry whose newer lines did not decode or are absent
    return ref, open_tables(gpu, files)


def test_store_has_resurrection_candidates(store):
    """(CPU) Some key's newest decodable line is dead while an older table
    holds a live value for it: the case a drop-then-select merge gets wrong."""
    ref, _ = store
    live_somewhere = set()
    for f in ref.files:
        for ln in f.split(b"\n"):
            if ln:
                k, t = ln.split(b"\t", 1)
                try:
                    v = base64.b64decode(t, validate=True)
                except Exception:
                    continue
                if not is_dead(v):
                    live_somewhere.add(k)
    dead = [k for k, v, _ in ref.entries if is_dead(v)]
    assert sum(k in live_somewhere for k in dead) > 50


def test_agreement_with_scan_many(gpu, store):
    ref, tables = store
    entries, live = gpu.count(tables, prefixes=STORE_PREFIXES)
    many = gpu.scan_many(tables, prefixes=STORE_PREFIXES)
    lv = gpu.scan_live(tables, prefixes=STORE_PREFIXES)
    assert entries.tolist() == np.diff(many.range_off()).tolist()
    assert live.tolist() == np.diff(lv.range_off()).tolist()
    # scan_live is scan_many filtered on the host
    keep = [i for i, v in enumerate(many.values()) if not is_dead(v)]
    assert lv.keys() == [many.keys()[i] for i in keep]
    assert lv.values() == [many.values()[i] for i in keep]
    assert lv.which().tolist() == many.which()[keep].tolist()
    assert 0 < lv.count < many.count
    check_ranges(gpu, ref, tables, prefixes=STORE_PREFIXES)
    check_ranges(gpu, ref, tables, ranges=[(b"", None)])
    check_ranges(gpu, ref, tables, ranges=[(b"1", b"2"), (b"2", b"2"), (b"5", b"9"), (b"c", None)])


def test_agreement_of_compact_live(gpu, store):
    ref, tables = store
    merged = check_compact_live(gpu, ref, tables, m=1 << 14)
    assert 0 < merged.nlines < len(ref.entries)
    # the live compaction scans as the live scan of its inputs
    assert gpu.scan([merged]).keys() == gpu.scan_live(tables, ranges=[(b"", None)]).keys()
    # the existing compaction keeps the tombstones
    plain, _, _ = gpu.compact(tables)
    assert plain.data() == oracle.sstable_create([(k, v) for k, v, _ in ref.entries])
    assert plain.nlines == len(ref.entries)


# ---- scan_live with a limit -------------------------------------------------------------

def test_scan_live_with_a_limit(gpu, store):
    ref, tables = store
    lo, hi = b"2", b"6"
    want = Ref.cut(ref.live, lo, hi)
    ents = Ref.cut(ref.entries, lo, hi)
    n = len(want)
    # a cut with dead entries before it: two live entries past the first dead one
    mid = sum(not is_dead(v) for _, v, _ in ents[:[is_dead(v) for _, v, _ in ents].index(True)]) + 2
    assert 1 < mid < n - 1 < len(ents)
    for limit, trunc in [(1, True), (mid, True), (n - 1, True), (n, False), (n + 1, False), (10 * n, False)]:
        r = gpu.scan_live(tables, ranges=[(lo, hi)], limit=limit)
        assert_result(r, want[:limit], f"limit {limit}", truncated=trunc)
        assert r.nranges == 1 and r.range_off().tolist() == [0, min(limit, n)]
    # the last live entry followed by dead ones only: not truncated
    tail = raw_file([(b"a", row(1, b"x")), (b"b", row(1, b"y")), (b"c", tomb(2)), (b"d", b"")])
    t = open_tables(gpu, [tail])
    r = gpu.scan_live(t, ranges=[(b"", None)], limit=2)
    assert_result(r, [(b"a", (1).to_bytes(8, "big") + b"x", 0), (b"b", (1).to_bytes(8, "big") + b"y", 0)], "tail")
    r = gpu.scan_live(t, prefixes=[b""], limit=1)
    assert r.truncated and r.keys() == [b"a"]
    with pytest.raises(gpu._lib.CassBloomError) as ei:
        gpu.scan_live(tables, prefixes=[b"1", b"2"], limit=3)
    assert ei.value.code == CB_EINVAL


# ---- nothing live -----------------------------------------------------------------------

def test_nothing_live(gpu):
    files = [raw_file([(b"a", tomb(3)), (b"b", b""), (b"c", BAD)]), raw_file([(b"a", row(1, b"old")), (b"c", tomb(1))])]
    ref, tables, e, lv = check_all(gpu, files)
    assert (e, lv) == ([3], [0]) and ref.live == []
    merged, bloom, z = gpu.compact_live(tables)
    empty, ebloom, _ = gpu.sstable_create([], m=1024)
    assert merged.data() == empty.data() == b"" and merged.nlines == 0 and merged.nbytes == 0
    assert np.array_equal(bloom.bools(), ebloom.bools()) and not bloom.bools().any()
    assert (z.min, z.max) == (None, None)
    r = gpu.scan_live(tables, prefixes=[b"a", b"b"])
    assert r.count == 0 and r.range_off().tolist() == [0, 0, 0]
    # the empty result is usable downstream
    assert gpu.count([merged], ranges=[(b"", None)])[0].tolist() == [0]


# ---- a side stream ----------------------------------------------------------------------

def test_results_on_a_side_stream_outlive_their_inputs(gpu):
    import torch
    files = record_files(np.random.default_rng(31), [700, 900, 300])
    ref = Ref(files)
    tables = open_tables(gpu, files)
    stream = torch.cuda.Stream()
    prefixes = [b"n0:", b"n1:", b"n2:"]
    ranges = [(p, oracle_prefix_end(p)) for p in prefixes]
    want, off = ref.expect_many(ranges, live=True)
    _, eoff = ref.expect_many(ranges, live=False)
    r = gpu.scan_live(tables, prefixes=prefixes, stream=stream)
    entries, live = gpu.count(tables, prefixes=prefixes, stream=stream)
    merged, _, _ = gpu.compact_live(tables, stream=stream)
    for t in tables:  # destroyed right after the calls
        t.close()
    churn = open_tables(gpu, files)  # the pool hands their blocks out again
    assert (entries.tolist(), live.tolist()) == (np.diff(eoff).tolist(), np.diff(off).tolist())
    assert np.array_equal(r.range_off(), off)
    assert_result(r, want, "after the inputs were closed")
    assert merged.data() == expected_compaction(ref, 1024)[0]
    assert [t.data() for t in churn] == files
    r.close()
    r.close()
