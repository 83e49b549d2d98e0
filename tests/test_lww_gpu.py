"""cb_tables_compact_lww, cb_tables_scan_lww, cb_tables_count_lww and
cb_scan_ts: the reference's last-write-wins read over the tables, on the
device.

The contract. Table r of the list stands for replica r; its answer for a key
is its line for the key if that line's value decodes. The winner of a key is
the fold of src/cluster.rs:405-416 over the answers, r = 0, 1, ...: the
greatest split_ts timestamp (src/query.rs:21-27) and, among equal ones, the
lowest table index. With drop_dead a winner without payload is then absent
(src/cluster.rs:454-459); it has still defeated every line it beat.

Every expectation comes from the C oracle per single table
(oracle.get_many([OracleTable(f_r)], ...) is replica r's answer), folded with
tests/lww_ref.py. Every comparison is exact.

Tables are hand-written files, so every value's text, timestamp and decoded
length is explicit. Shapes are the smallest at which each kernel can go wrong:
runs of equal keys across the select's 256-record tile edge with the winner on
either side of it, runs longer than one and two tiles, two long runs back to
back, keys that differ past their 16th byte only, and ranges that begin and
end at a run.
"""
import ctypes

import numpy as np
import pytest

import lww_ref
from liverow_ref import is_dead
from merge_help import (ALL, b64, BAD, file_keys, hex_keys, open_tables, oracle_prefix_end, ragged,
                        raw_file, row, table_lines, TILE, tomb)
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1


# ---- the reference and the checks (shared helpers: tests/merge_help.py) ----

class Ref:
    """Every table's own answers from the oracle (table r alone is replica r),
    computed once, and their fold."""

    def __init__(self, files):
        self.files = files
        self.answers = []
        for f in files:
            keys = file_keys(f)
            rows = {}
            if keys:
                kd, ko = ragged(keys)
                which, voff, vals = oracle.get_many([oracle.OracleTable(f)], None, kd, ko)
                rows = {k: vals[int(voff[i]):int(voff[i + 1])] for i, k in enumerate(keys) if which[i] >= 0}
            self.answers.append(rows)
        self.all_keys = sorted(set(k for f in files for k in file_keys(f)))
        self.nlines = sum(len(file_keys(f)) for f in files)
        self.w = {False: lww_ref.winners(self.answers), True: lww_ref.winners(self.answers, drop_dead=True)}

    def winner(self, key):
        """(value, which, ts) of the key's winner, or None."""
        hit = [x for x in self.w[False] if x[0] == key]
        return hit[0][1:] if hit else None

    def expect_many(self, ranges, drop):
        """(winners of every range one after the other, range_off)."""
        parts = [[x for x in self.w[drop] if lo <= x[0] and (hi is None or x[0] < hi)] for lo, hi in ranges]
        off = np.zeros(len(ranges) + 1, np.uint64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return [x for p in parts for x in p], off


def assert_result(r, want, what="", truncated=False):
    """r holds exactly the entries `want` = [(key, value, which, ts)]."""
    assert r.count == len(want), f"{what}: {r.count} entries against {len(want)}"
    assert r.truncated is truncated, what
    ko, kb, vo, vb = r.raw()
    eko, evo = ragged([x[0] for x in want])[1], ragged([x[1] for x in want])[1]
    assert np.array_equal(ko, eko), f"{what}: key offsets differ"
    assert kb.tobytes() == b"".join(x[0] for x in want), f"{what}: keys differ"
    assert np.array_equal(vo, evo), f"{what}: value offsets differ"
    assert vb.tobytes() == b"".join(x[1] for x in want), f"{what}: values differ"
    assert r.which().tolist() == [x[2] for x in want], f"{what}: sources differ"
    ts = r.ts()
    assert ts.dtype == np.uint64 and ts.tolist() == [x[3] for x in want], f"{what}: timestamps differ"
    assert (r.key_bytes, r.val_bytes) == (int(eko[-1]), int(evo[-1])), what


def expected_compaction(ref, drop, m):
    """(file, its lines' (start, key_len, line_len), OracleFilter, (min, max) or None) of the winners."""
    w = ref.w[drop]
    filt = oracle.OracleFilter(m)
    kept = [x[0] for x in w]
    if kept:
        filt.insert_var(*ragged(kept))
    data = oracle.sstable_create([(x[0], x[1]) for x in w]) if kept else b""
    lines = [ln for ln in data.split(b"\n") if ln]
    starts = np.cumsum([0] + [len(ln) + 1 for ln in lines])[:-1].tolist()
    return data, (starts, [len(k) for k in kept], [len(ln) for ln in lines]), filt, \
        ((min(kept), max(kept)) if kept else None)


def check_compact(gpu, ref, tables, drop, m=1024, stream=None):
    """compact_lww's file, line index, filter, zone bounds and reads."""
    want, lines, filt, zone = expected_compaction(ref, drop, m)
    merged, bloom, z = gpu.compact_lww(tables, m=m, drop_dead=drop, stream=stream)
    got = merged.data()
    assert got == want, f"drop_dead={drop}: merged file differs: {len(got)} bytes against {len(want)}"
    assert merged.nlines == len(ref.w[drop]) and merged.nbytes == len(want)
    assert table_lines(gpu, merged) == lines, "line index differs"
    assert np.array_equal(bloom.bools(), filt.bools()), "filter bits differ from the oracle"
    assert (z.min, z.max) == (zone if zone else (None, None))
    if ref.all_keys:
        # every kept key answers with its winner's value, every other key is not found
        which, voff, vals = gpu.get_many([merged], ref.all_keys)
        kept = {x[0]: x[1] for x in ref.w[drop]}
        assert (which >= 0).tolist() == [k in kept for k in ref.all_keys], "found keys differ"
        assert vals == b"".join(kept.get(k, b"") for k in ref.all_keys), "values differ"
    return merged


def check_ranges(gpu, ref, tables, ranges=None, prefixes=None, stream=None):
    """scan_lww with drop_dead 0 and 1 and count_lww over the ranges against
    the fold. Returns (entries per range, live per range) as lists."""
    kw = {"prefixes": prefixes} if prefixes is not None else {"ranges": ranges}
    if prefixes is not None:
        ranges = [(p, oracle_prefix_end(p)) for p in prefixes]
    what = f"{len(ranges)} ranges from {ranges[0][0][:12]!r}"
    sizes = {}
    for drop in (False, True):
        want, off = ref.expect_many(ranges, drop)
        r = gpu.scan_lww(tables, drop_dead=drop, stream=stream, **kw)
        assert r.nranges == len(ranges), what
        assert np.array_equal(r.range_off(), off), \
            f"{what}, drop_dead={drop}: range offsets {r.range_off().tolist()} against {off.tolist()}"
        assert_result(r, want, f"{what}, drop_dead={drop}")
        sizes[drop] = np.diff(off).tolist()
    entries, live = gpu.count_lww(tables, stream=stream, **kw)
    assert entries.dtype == np.uint64 and live.dtype == np.uint64
    assert entries.tolist() == sizes[False], f"{what}: entries"
    assert live.tolist() == sizes[True], f"{what}: live"
    return sizes[False], sizes[True]


def check_all(gpu, files, ranges=None, prefixes=None, m=1024):
    """Every entry over the files, each with drop_dead 0 and 1: the ranges
    (default: everything, as one unbounded range) and the compaction."""
    ref = Ref(files)
    tables = open_tables(gpu, files)
    assert all(t.well_formed for t in tables if t.nlines)
    if ranges is None and prefixes is None:
        ranges = ALL
    e, lv = check_ranges(gpu, ref, tables, ranges=ranges, prefixes=prefixes)
    for drop in (False, True):
        check_compact(gpu, ref, tables, drop, m=m)
    return ref, tables, e, lv


def per_table(lines_by_key, nt):
    """lines_by_key = {key: {table: text}} -> nt files."""
    return [raw_file(sorted((k, by[t]) for k, by in lines_by_key.items() if t in by)) for t in range(nt)]


# ---- where the winner stands in its run -------------------------------------------------

def test_winner_position_and_timestamp_order(gpu):
    """Five tables; the winner is the first, a middle and the last record of
    its run, with timestamps that ascend, descend and are shuffled against
    table order, and keys that only some tables hold."""
    stamps = {b"k:ascending": [1, 2, 3, 4, 5],      # the last record wins
              b"k:descending": [9, 8, 7, 6, 5],     # the first
              b"k:middle": [3, 4, 9, 2, 1],
              b"k:second": [3, 9, 4, 2, 1],
              b"k:fourth": [6, 1, 5, 8, 7],
              b"k:some": [None, 7, None, 8, 2],
              b"k:one": [None, None, 4, None, None]}
    keys = {k: {t: row(s, b"%s@%d" % (k, t)) for t, s in enumerate(ss) if s is not None} for k, ss in stamps.items()}
    ref, tables, e, lv = check_all(gpu, per_table(keys, 5))
    assert [x[2] for x in ref.w[False]] == [4, 0, 3, 2, 2, 1, 3]  # (sorted by key)
    assert (e, lv) == ([7], [7])
    check_ranges(gpu, ref, tables, prefixes=[b"k:a", b"k:d", b"k:f", b"k:m", b"k:o", b"k:s"])


# ---- ties -------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_table_index(gpu):
    """Equal timestamps in tables 2 and 5: table 2 wins. Decoded lengths 0..7
    all have timestamp 0, whatever their bytes: the lowest index wins."""
    short = [bytes([0xF0 + n]) * n for n in (5, 0, 7, 3, 1, 6, 2, 4)]  # table r holds length len(short[r])
    keys = {b"t:tie": {0: row(10, b"zero"), 1: row(20, b"one"), 2: row(50, b"TWO"), 3: row(49, b"three"),
                       4: row(7, b"four"), 5: row(50, b"five")},
            b"t:tie-last": {6: row(50, b"six"), 7: row(50, b"seven")},
            b"t:short": {t: b64(v) for t, v in enumerate(short)},
            b"t:short-from-3": {t: b64(v) for t, v in enumerate(short) if t >= 3},
            b"t:short-against-zero-ts": {1: b64(b"abc"), 4: tomb(0), 6: row(0, b"live")}}
    ref, tables, e, lv = check_all(gpu, per_table(keys, 8))
    assert ref.winner(b"t:tie")[1:] == (2, 50) and ref.winner(b"t:tie-last")[1:] == (6, 50)
    assert ref.winner(b"t:short") == (short[0], 0, 0) and ref.winner(b"t:short-from-3") == (short[3], 3, 0)
    assert ref.winner(b"t:short-against-zero-ts") == (b"abc", 1, 0)
    assert (e, lv) == ([5], [5])


# ---- timestamp values -------------------------------------------------------------------

def test_timestamps_compare_unsigned_and_to_the_last_byte(gpu):
    hi, lo = 2 ** 63, 2 ** 63 - 1
    a, b = 0x1122334455667700, 0x1122334455667701
    keys = {b"u:sign-new": {0: row(hi, b"2^63"), 1: row(lo, b"2^63-1")},
            b"u:sign-old": {0: row(lo, b"2^63-1"), 1: row(hi, b"2^63")},
            b"u:max": {0: row(0, b"zero"), 1: row(2 ** 64 - 1, b"max"), 2: row(2 ** 64 - 2, b"max-1")},
            b"u:last-byte-new": {0: row(b, b"b"), 1: row(a, b"a")},
            b"u:last-byte-old": {0: row(a, b"a"), 1: row(b, b"b")},
            b"u:low-bits": {t: row(0x7700 | 1 << t, b"bit%d" % t) for t in range(3)},
            b"u:plus-and-slash": {0: row(0xFBEFBEFBEFBEFBEF, b"+"), 1: row(0xFFFFFFFFFFFFFFF0, b"/"),
                                  2: row(0xFBEFBEFBEFBEFBEE, b"+-1")}}
    ref, tables, e, lv = check_all(gpu, per_table(keys, 3))
    assert ref.winner(b"u:sign-new")[1:] == (0, hi) and ref.winner(b"u:sign-old")[1:] == (1, hi)
    assert ref.winner(b"u:max")[1:] == (1, 2 ** 64 - 1)
    assert ref.winner(b"u:last-byte-new")[1:] == (0, b) and ref.winner(b"u:last-byte-old")[1:] == (1, b)
    assert ref.winner(b"u:low-bits")[1:] == (2, 0x7704) and ref.winner(b"u:plus-and-slash")[1] == 1


# ---- undecodable lines ------------------------------------------------------------------

# eleven characters of the greatest timestamp, then a text STANDARD.decode rejects (13 characters)
BAD_MAX = b64((2 ** 64 - 1).to_bytes(8, "big") + b"x") + b"="


def test_undecodable_lines_take_no_part(gpu):
    assert len(BAD_MAX) == 13 and oracle.b64_decode(BAD_MAX) is None and oracle.b64_decode(BAD_MAX[:12]) is not None
    keys = {b"x:bad-newest": {0: BAD_MAX, 1: row(5, b"five"), 2: row(6, b"six")},
            b"x:bad-between": {0: row(3, b"three"), 1: BAD_MAX, 2: row(2, b"two")},
            b"x:bad-last": {0: row(1, b"one"), 2: BAD},
            b"x:nowhere": {0: BAD, 1: BAD_MAX, 2: b"*"},
            b"x:only-bad": {1: b"===="},
            b"x:bad-over-tombstone": {0: BAD_MAX, 1: tomb(9), 2: row(8, b"older")}}
    ref, tables, e, lv = check_all(gpu, per_table(keys, 3))
    assert [x[0][2:] for x in ref.w[False]] == [b"bad-between", b"bad-last", b"bad-newest", b"bad-over-tombstone"]
    assert ref.winner(b"x:bad-newest")[1:] == (2, 6) and ref.winner(b"x:bad-between")[1:] == (0, 3)
    assert (e, lv) == ([4], [3])
    e, lv = check_ranges(gpu, ref, tables, prefixes=[b"x:bad-n", b"x:n", b"x:o"])
    assert (e, lv) == ([1, 0, 0], [1, 0, 0])


def test_nothing_decodes(gpu):
    files = [raw_file([(b"a", BAD), (b"b", BAD_MAX)]), b"", raw_file([(b"a", b"*"), (b"c", b"====")])]
    ref, tables, e, lv = check_all(gpu, files, ranges=[(b"", b"b"), (b"b", None)])
    assert (e, lv) == ([0, 0], [0, 0]) and ref.w[False] == []
    for drop in (False, True):
        merged, bloom, z = gpu.compact_lww(tables, drop_dead=drop)
        empty, ebloom, _ = gpu.sstable_create([], m=1024)
        assert merged.data() == empty.data() == b"" and merged.nlines == 0 and merged.nbytes == 0
        assert np.array_equal(bloom.bools(), ebloom.bools()) and not bloom.bools().any()
        assert (z.min, z.max) == (None, None)
        # the empty result is usable downstream
        assert gpu.count_lww([merged], ranges=ALL)[0].tolist() == [0]


# ---- tombstones -------------------------------------------------------------------------

def test_tombstones_win_and_lose_by_timestamp(gpu):
    keys = {b"d:tomb-wins": {0: row(20, b"older write"), 1: tomb(30)},
            b"d:tomb-loses": {0: tomb(5), 3: row(9, b"newer write")},   # T[0] is the newer TABLE
            b"d:tomb-loses-below": {1: row(9, b"newer write"), 2: tomb(5)},
            b"d:tomb-ties-first": {0: tomb(7), 1: row(7, b"same stamp")},
            b"d:tomb-ties-second": {0: row(7, b"same stamp"), 1: tomb(7)},
            b"d:len0-then-len8": {0: b"", 1: tomb(0)},    # both ts 0: table 0, the empty value
            b"d:len8-then-len0": {0: tomb(0), 1: b""},    # both ts 0: table 0, the 8 zero bytes
            b"d:len0-against-tomb": {0: b"", 1: tomb(7)},  # ts 7 beats ts 0
            b"d:all-dead": {0: tomb(1), 1: b"", 2: tomb(3), 3: tomb(2)}}
    files = per_table(keys, 4)
    ref, tables, e, lv = check_all(gpu, files)
    kept = {False: [x[0][2:] for x in ref.w[False]], True: [x[0][2:] for x in ref.w[True]]}
    assert len(kept[False]) == 9  # with drop_dead 0 every key stays, a winning tombstone as a tombstone
    assert kept[True] == [b"tomb-loses", b"tomb-loses-below", b"tomb-ties-second"]
    assert ref.winner(b"d:tomb-wins") == ((30).to_bytes(8, "big"), 1, 30)
    assert ref.winner(b"d:tomb-loses")[1:] == (3, 9)
    assert ref.winner(b"d:len0-then-len8") == (b"", 0, 0) and ref.winner(b"d:len8-then-len0") == (bytes(8), 0, 0)
    assert ref.winner(b"d:len0-against-tomb") == ((7).to_bytes(8, "big"), 1, 7)
    assert ref.winner(b"d:all-dead")[1:] == (2, 3)
    assert (e, lv) == ([9], [3])
    # where LWW differs from the live-row entries: compact_live lets T[0]'s old tombstone delete the newer row
    live, _, _ = gpu.compact_live(tables)
    live_keys = file_keys(live.data())
    assert b"d:tomb-loses" not in live_keys and b"d:tomb-loses-below" in live_keys
    lww, _, _ = gpu.compact_lww(tables, drop_dead=True)
    assert b"d:tomb-loses" in file_keys(lww.data())


# ---- tile edges -------------------------------------------------------------------------

@pytest.mark.parametrize("winner", [0, 1, 2, 4])
def test_a_run_across_the_select_tile_edge(gpu, winner):
    """K has a line in each of five tables and 254 records sort below it, so
    its run is records 254..258: the head and one more in the first tile,
    three in the second. The winner is record 254 + winner."""
    fill = [(b"a%04d" % i, row(5, b"f%d" % i)) for i in range(TILE - 2)]
    after = [(b"z%02d" % i, row(6, b"z")) for i in range(3)]
    stamps = [10, 11, 12, 13, 14]
    stamps[winner] = 99
    files = [raw_file(sorted(fill[t::5] + [(b"m:K", row(stamps[t], b"t%d" % t))] + after[t:t + 1])) for t in range(5)]
    ref, tables, e, lv = check_all(gpu, files)
    assert ref.nlines == TILE - 2 + 5 + 3 and ref.winner(b"m:K")[1:] == (winner, 99)
    assert (e, lv) == ([TILE + 2], [TILE + 2])
    e, lv = check_ranges(gpu, ref, tables, ranges=[(b"", b"m:K"), (b"m:K", b"m:K\0"), (b"m:K\0", None)])
    assert (e, lv) == ([TILE - 2, 1, 3], [TILE - 2, 1, 3])


def test_a_dead_winner_across_the_tile_edge(gpu):
    """The same run with a tombstone as the winner in the second tile: the key
    stays a tombstone, or leaves with drop_dead, and no older row comes back."""
    fill = [(b"a%04d" % i, row(5, b"f%d" % i)) for i in range(TILE - 2)]
    texts = [row(10, b"t0"), row(11, b"t1"), row(12, b"t2"), tomb(99), row(98, b"t4")]
    files = [raw_file(sorted(fill[t::5] + [(b"m:K", texts[t])])) for t in range(5)]
    ref, tables, e, lv = check_all(gpu, files)
    assert ref.winner(b"m:K") == ((99).to_bytes(8, "big"), 3, 99)
    assert (e, lv) == ([TILE - 1], [TILE - 2])


def test_runs_of_300_and_520_back_to_back(gpu):
    """520 tables of one or two lines: J in the first 300 (records 0..299), K
    in all of them (records 300..819, over three tiles and into a fourth).
    Timestamps are shuffled against table order; J's winner is its last
    record, K's a tombstone in the run's last tile."""
    rng = np.random.default_rng(520)
    nt = 520
    tj, tk = rng.permutation(300) + 1, rng.permutation(nt) + 1
    files = []
    for t in range(nt):
        lines = [(b"m:K", tomb(10 ** 6) if t == 515 else row(int(tk[t]), b"K%d" % t))]
        if t < 300:
            lines = [(b"k:J", row(10 ** 6 if t == 299 else int(tj[t]), b"J%d" % t))] + lines
        files.append(raw_file(lines))
    ref, tables, e, lv = check_all(gpu, files, m=4096)
    assert ref.nlines == 820
    assert ref.winner(b"k:J")[1:] == (299, 10 ** 6) and ref.winner(b"m:K") == ((10 ** 6).to_bytes(8, "big"), 515, 10 ** 6)
    assert (e, lv) == ([2], [1])
    # every line undecodable but one, deep in the run: it wins from anywhere
    files = [raw_file([(b"m:K", row(3, b"only") if t == 401 else BAD)]) for t in range(nt)]
    ref, tables, e, lv = check_all(gpu, files)
    assert ref.winner(b"m:K")[1:] == (401, 3) and (e, lv) == ([1], [1])


def test_keys_that_differ_past_their_16th_byte(gpu):
    """Runs whose keys share their first 16 bytes and their length: same_key
    has to read the batch, and adjacent runs must not merge."""
    stem = b"0123456789abcdef"
    keys = {stem: {0: row(1, b"stem0"), 2: row(2, b"stem2")},
            stem + b"-A": {0: row(9, b"A0"), 1: row(3, b"A1"), 2: row(4, b"A2")},
            stem + b"-B": {0: row(1, b"B0"), 1: row(9, b"B1"), 2: row(4, b"B2")},
            stem + b"-C": {0: row(1, b"C0"), 1: row(3, b"C1"), 2: row(9, b"C2")},
            stem + b"-C" + b"x" * 40: {1: tomb(5), 2: row(4, b"long")},
            stem + b"-D": {0: tomb(9), 1: row(9, b"D1")}}
    ref, tables, e, lv = check_all(gpu, per_table(keys, 3))
    assert [x[2] for x in ref.w[False]] == [2, 0, 1, 2, 1, 0]
    assert (e, lv) == ([6], [4])
    check_ranges(gpu, ref, tables, prefixes=[stem + b"-A", stem + b"-B", stem + b"-C", stem + b"-D"])


# ---- table lists ------------------------------------------------------------------------

def test_empty_tables_anywhere_and_a_single_table(gpu):
    t1 = raw_file([(b"a", row(5, b"a1")), (b"b", row(9, b"b1")), (b"c", tomb(4))])
    t3 = raw_file([(b"a", row(7, b"a3")), (b"b", row(2, b"b3")), (b"c", row(3, b"c3")), (b"d", BAD)])
    ref, tables, e, lv = check_all(gpu, [b"", t1, b"", t3, b""])
    assert [x[2] for x in ref.w[False]] == [3, 1, 1] and (e, lv) == ([3], [2])
    ref, _, e, lv = check_all(gpu, [b"", b""], ranges=[(b"a", b"b"), (b"b", None)])
    assert (e, lv) == ([0, 0], [0, 0])
    # one table: its own decodable lines, byte for byte
    lines = [(b"a", row(5, b"a")), (b"b", BAD), (b"c", tomb(4)), (b"d", b""), (b"e", BAD_MAX), (b"f", b64(b"short"))]
    ref, tables, e, lv = check_all(gpu, [raw_file(lines)])
    merged, _, _ = gpu.compact_lww(tables)
    assert merged.data() == raw_file([ln for ln in lines if ln[1] not in (BAD, BAD_MAX)])
    assert (e, lv) == ([4], [2])


# ---- properties over a store ------------------------------------------------------------

STORE_PREFIXES = [b"0", b"3", b"4", b"7f", b"a", b"f"]


def store_files(stamp, nt=9, seed=1311):
    """nt tables x 200 hex-key lines over a pool of 700 keys, about a fifth
    tombstones and some undecodable values; stamp(t, key number) = the line's
    timestamp."""
    rng = np.random.default_rng(seed)
    pool = hex_keys(rng, 700, 10)
    files = []
    for t in range(nt):
        lines = []
        for i in rng.choice(len(pool), 200, replace=False).tolist():
            u = rng.random()
            ts = stamp(t, i)
            text = tomb(ts) if u < 0.20 else BAD if u < 0.26 else row(ts, b"t%d:" % t + pool[i][:int(rng.integers(0, 9))])
            lines.append((pool[i], text))
        files.append(raw_file(sorted(lines)))
    return files


@pytest.fixture(scope="module")
def shuffled_store(gpu):
    """Timestamps shuffled against table order, distinct within a key: (ref, tables)."""
    order = np.random.default_rng(77).permuted(np.tile(np.arange(9), (700, 1)), axis=1)
    files = store_files(lambda t, i: 1000 + int(order[i, t]))
    ref = Ref(files)
    newest = {}  # the key's first table with an answer: newest-wins' choice
    for r, rows in enumerate(ref.answers):
        for k in rows:
            newest.setdefault(k, r)
    # the rule matters here: many winners are not the newest decodable line, and tombstones both win and lose
    assert sum(newest[x[0]] != x[2] for x in ref.w[False]) > 100
    assert 20 < len(ref.w[False]) - len(ref.w[True]) < len(ref.w[False]) / 2
    return ref, open_tables(gpu, files)


def test_descending_timestamps_agree_with_newest_wins(gpu):
    """With timestamps strictly descending in table order for every key, LWW
    chooses the newest decodable line: the existing entries' answers, byte for
    byte."""
    files = store_files(lambda t, i: 5000 - 10 * t)
    ref = Ref(files)
    tables = open_tables(gpu, files)
    plain, pbloom, pz = gpu.compact(tables, m=8192)
    lww, bloom, z = gpu.compact_lww(tables, m=8192)
    assert lww.data() == plain.data() and lww.nlines == plain.nlines == len(ref.w[False])
    assert np.array_equal(bloom.bools(), pbloom.bools()) and (z.min, z.max) == (pz.min, pz.max)
    live, _, _ = gpu.compact_live(tables)
    assert gpu.compact_lww(tables, drop_dead=True)[0].data() == live.data()
    many, lw = gpu.scan_many(tables, prefixes=STORE_PREFIXES), gpu.scan_lww(tables, prefixes=STORE_PREFIXES)
    for a, b in zip(many.raw(), lw.raw()):
        assert np.array_equal(a, b)
    assert np.array_equal(many.which(), lw.which()) and np.array_equal(many.range_off(), lw.range_off())
    sl, ld = gpu.scan_live(tables, prefixes=STORE_PREFIXES), gpu.scan_lww(tables, prefixes=STORE_PREFIXES, drop_dead=True)
    assert sl.keys() == ld.keys() and sl.values() == ld.values() and np.array_equal(sl.which(), ld.which())
    assert 0 < sl.count < many.count
    assert [np.asarray(x).tolist() for x in gpu.count(tables, prefixes=STORE_PREFIXES)] == \
        [np.asarray(x).tolist() for x in gpu.count_lww(tables, prefixes=STORE_PREFIXES)]
    check_compact(gpu, ref, tables, False, m=8192)
    check_ranges(gpu, ref, tables, prefixes=STORE_PREFIXES)


def test_the_store_against_the_fold(gpu, shuffled_store):
    ref, tables = shuffled_store
    for drop in (False, True):
        check_compact(gpu, ref, tables, drop, m=1 << 14)
    check_ranges(gpu, ref, tables, prefixes=STORE_PREFIXES)
    check_ranges(gpu, ref, tables, ranges=ALL)


def test_reversing_the_table_list_changes_nothing_but_which(gpu, shuffled_store):
    """All timestamps of a key are distinct, so the winner does not depend on
    the order of the list."""
    ref, tables = shuffled_store
    nt, rev = len(tables), tables[::-1]
    for drop in (False, True):
        a, b = gpu.compact_lww(tables, drop_dead=drop)[0], gpu.compact_lww(rev, drop_dead=drop)[0]
        assert a.data() == b.data() and a.nlines == len(ref.w[drop])
        ra, rb = gpu.scan_lww(tables, ranges=ALL, drop_dead=drop), gpu.scan_lww(rev, ranges=ALL, drop_dead=drop)
        assert ra.keys() == rb.keys() and ra.values() == rb.values() and np.array_equal(ra.ts(), rb.ts())
        assert rb.which().tolist() == [nt - 1 - w for w in ra.which().tolist()]
        assert len(set(ra.which().tolist())) == nt


# ---- batched ranges, a limit, count against scan ----------------------------------------

def test_runs_at_range_boundaries_and_empty_ranges(gpu, shuffled_store):
    ref, tables = shuffled_store
    # a key held by many tables, so a run begins exactly at a range's bound and ends at the next one's
    held = {}
    for rows in ref.answers:
        for k in rows:
            held[k] = held.get(k, 0) + 1
    k = max((k for k in held if b"2" < k < b"e"), key=lambda k: (held[k], k))
    assert held[k] >= 5
    ranges = [(b"", b""),                  # lo == hi, first
              (b"", b"0"),                 # no key below "0"
              (b"0", k), (k, k + b"\0"), (k + b"\0", b"f"),
              (b"f", b"f"), (b"g", b"h"),  # empty ranges at the end: lo == hi, and no line inside
              (b"h", None)]
    e, lv = check_ranges(gpu, ref, tables, ranges=ranges)
    assert e[0] == e[1] == e[5] == e[6] == e[7] == 0 and e[3] == 1 and e[2] > 0 and e[4] > 0
    assert sum(e) == len([x for x in ref.w[False] if x[0] < b"f"])
    # every range empty: by its bounds (no device work), and by the data
    assert check_ranges(gpu, ref, tables, ranges=[(b"c", b"b"), (b"c", b"c")]) == ([0, 0], [0, 0])
    assert check_ranges(gpu, ref, tables, ranges=[(b"g", b"h"), (b"x", None)]) == ([0, 0], [0, 0])
    e0, l0 = gpu.count_lww(tables, ranges=[])
    assert e0.shape == (0,) and l0.shape == (0,)


def test_scan_lww_with_a_limit(gpu, shuffled_store):
    ref, tables = shuffled_store
    lo, hi = b"2", b"9"
    for drop in (False, True):
        want, _ = ref.expect_many([(lo, hi)], drop)
        n = len(want)
        assert n > 40
        for limit, trunc in [(1, True), (n // 2, True), (n - 1, True), (n, False), (n + 1, False)]:
            r = gpu.scan_lww(tables, ranges=[(lo, hi)], limit=limit, drop_dead=drop)
            assert_result(r, want[:limit], f"limit {limit}, drop_dead={drop}", truncated=trunc)  # truncated counts winners
            assert r.nranges == 1 and r.range_off().tolist() == [0, min(limit, n)]
    with pytest.raises(gpu._lib.CassBloomError) as ei:
        gpu.scan_lww(tables, prefixes=[b"1", b"2"], limit=3)
    assert ei.value.code == CB_EINVAL


# ---- cb_scan_ts on any result -----------------------------------------------------------

def test_scan_ts_of_plain_and_empty_results(gpu, shuffled_store):
    import torch
    ref, tables = shuffled_store
    r = gpu.scan(tables, lo=b"1", hi=b"c")  # cb_tables_scan: newest-wins entries, tombstones among them
    vals = r.values()
    want = [lww_ref.ts_of(v) for v in vals]
    assert r.count > 100 and any(len(v) == 8 for v in vals) and len(set(want)) > 5
    assert r.ts().tolist() == want  # a host output
    dev = torch.full((r.count,), -1, dtype=torch.int64, device="cuda")
    r.copy_ts(dev)                  # a device output
    assert dev.cpu().numpy().view(np.uint64).tolist() == want
    # values below 8 bytes have timestamp 0
    short = open_tables(gpu, [raw_file([(b"a", b64(b"1234567")), (b"b", b""), (b"c", row(2 ** 64 - 1, b"")),
                                        (b"d", row(258, b"x"))])])
    assert gpu.scan(short).ts().tolist() == [0, 0, 2 ** 64 - 1, 258]
    assert gpu.scan_many(short, prefixes=[b"c", b"d"]).ts().tolist() == [2 ** 64 - 1, 258]
    # an empty result: nothing is written, a NULL ts is fine
    for empty in (gpu.scan(tables, lo=b"x", hi=b"y"), gpu.scan_lww(tables, ranges=[(b"x", b"y")])):
        assert empty.count == 0 and empty.ts().shape == (0,)
        keep = np.full(4, 0xDEAD, np.uint64)
        empty.copy_ts(keep)
        assert keep.tolist() == [0xDEAD] * 4
        assert gpu._lib.load().cb_scan_ts(empty._h, None) == 0
    assert gpu._lib.load().cb_scan_ts(r._h, None) == 0


# ---- a side stream ----------------------------------------------------------------------

def test_results_on_a_side_stream_outlive_their_inputs(gpu):
    import torch
    order = np.random.default_rng(5).permuted(np.tile(np.arange(4), (700, 1)), axis=1)
    files = store_files(lambda t, i: 100 + int(order[i, t]), nt=4, seed=99)
    ref = Ref(files)
    tables = open_tables(gpu, files)
    stream = torch.cuda.Stream()
    ranges = [(p, oracle_prefix_end(p)) for p in STORE_PREFIXES]
    want, off = ref.expect_many(ranges, True)
    _, eoff = ref.expect_many(ranges, False)
    r = gpu.scan_lww(tables, prefixes=STORE_PREFIXES, drop_dead=True, stream=stream)
    entries, live = gpu.count_lww(tables, prefixes=STORE_PREFIXES, stream=stream)
    merged, _, _ = gpu.compact_lww(tables, stream=stream)
    for t in tables:  # destroyed right after the calls
        t.close()
    churn = open_tables(gpu, files)  # the pool hands their blocks out again
    assert (entries.tolist(), live.tolist()) == (np.diff(eoff).tolist(), np.diff(off).tolist())
    assert np.array_equal(r.range_off(), off)
    assert_result(r, want, "after the inputs were closed")
    assert merged.data() == expected_compaction(ref, False, 1024)[0]
    assert [t.data() for t in churn] == files
    r.close()
    r.close()
