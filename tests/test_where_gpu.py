"""cb_tables_count_where and cb_scan_match: the reference's SELECT COUNT(*) ...
WHERE (src/query.rs:309-362) over the tables, on the device.

The contract. For tables T[0..nt), T[0] newest, and a range r,
    live[r]    = cb_tables_count's live[r] (lww: cb_tables_count_lww's),
    matched[r] = how many of those live rows match the predicate,
by the row rule of lsmt_amd/csrc/rowjson.hpp: the payload after the 8-byte
timestamp parsed as serde_json parses a BTreeMap<String, String> (any error:
the empty map), the key's `|`-separated parts after `skip` bytes as the key
columns, every condition an equality. cb_scan_match is the same verdict per
entry of a finished scan result.

Every expectation comes from `Ref` as tests/test_live_gpu.py builds it (the C
oracle's get_many over hand-written files: Database::get's walk), filtered
with tests/rowjson_ref.py, the rule's independent restatement; the LWW case
takes its winners from tests/lww_ref.py. Every comparison is exact.

Shapes are the smallest at which the kernels can go wrong: the known answers
of tests/where_cases.py with filler in one result of more than 256 entries
(k_scan_match's block edge; k_scan_count_where's base64 reader over every
case, all three padding forms, the payload starting inside a quantum),
matching rows at sorted record positions 255, 256 and 257 behind shadowed
duplicates, undecodable lines and tombstones, 256 and 257 one-row ranges in a
row, one range over three tiles, empty ranges at both ends, and rows of 300
and 5000 bytes among short ones.
"""
import base64

import numpy as np
import pytest

import lww_ref
import rowjson_ref
from liverow_ref import is_dead
from merge_help import b64, BAD, file_keys, open_tables, oracle_prefix_end, raw_file, row, TILE, tomb
from test_live_gpu import Ref
from where_cases import CASES

pytestmark = pytest.mark.gpu

CV = [("c", "v")]
HIT, MISS = b'{"c":"v"}', b'{"c":"w"}'


# ---- expectations -----------------------------------------------------------------------

def lww_live(files):
    """The winners by timestamp that are not tombstones, as Ref.live holds the
    newest-wins ones: [(key, value, which)]."""
    answers = []
    for f in files:
        rows = {}
        for ln in f.split(b"\n"):
            if ln:
                k, t = ln.split(b"\t", 1)
                try:
                    rows[k] = base64.b64decode(t, validate=True)
                except Exception:
                    pass
        answers.append(rows)
    return [(k, v, w) for k, v, w, _ in lww_ref.winners(answers, drop_dead=True)]


def check_where(gpu, ref, tables, where, key_columns=(), ranges=None, prefixes=None, skip=None, lww=False, stream=None):
    """count_where over the ranges against the oracle's live rows filtered
    with rowjson_ref, and against count() and scan_live().match(). Returns
    (live, matched) as lists."""
    kw = {"prefixes": prefixes} if prefixes is not None else {"ranges": ranges}
    if prefixes is not None:
        ranges = [(p, oracle_prefix_end(p)) for p in prefixes]
    skips = skip if skip is not None else [len(p) for p in prefixes] if prefixes is not None else 0
    skips = [skips] * len(ranges) if isinstance(skips, int) else list(skips)
    rows = lww_live(ref.files) if lww else ref.live
    parts = [Ref.cut(rows, lo, hi) for lo, hi in ranges]
    want_live = [len(p) for p in parts]
    want = [sum(rowjson_ref.matches(k, v, where, key_columns, s) for k, v, _ in p) for p, s in zip(parts, skips)]
    live, matched = gpu.count_where(tables, where, key_columns, skip=skip, lww=lww, stream=stream, **kw)
    assert live.dtype == np.uint64 and matched.dtype == np.uint64
    assert live.tolist() == want_live, "live"
    assert matched.tolist() == want, "matched"
    # live is count()'s, and matched the per-range sums of the live scan's verdicts
    assert live.tolist() == (gpu.count_lww if lww else gpu.count)(tables, **kw)[1].tolist()
    r = gpu.scan_lww(tables, drop_dead=True, **kw) if lww else gpu.scan_live(tables, **kw)
    flags, off = r.match(where, key_columns, skip=skip if skip is not None else skips), r.range_off().tolist()
    assert flags.dtype == bool and flags.shape == (r.count,)
    assert [int(flags[off[i]:off[i + 1]].sum()) for i in range(len(ranges))] == want, "match() per range"
    return live.tolist(), matched.tolist()


# ---- the known answers, on the device ---------------------------------------------------

FILL = [HIT, MISS, b'{"c":"v","d":"e"}', b"not json", b'{"pk":"a","c":"v"}', b'{"c":"v"} ', b'{"c":"v"}x', b"{}"]


@pytest.fixture(scope="module")
def known(gpu):
    """One table: every case of tests/where_cases.py as a row under "g"
    (its key after a 6-byte prefix), 300 filler rows under "f" (5-byte
    prefixes), tombstones and an undecodable text among them; and the distinct
    predicates of the cases, each with the cases that use it."""
    lines = [(b"g%04d/" % i + c.key, b64(c.value)) for i, c in enumerate(CASES)]
    for i in range(300):
        text = tomb(i) if i % 9 == 0 else BAD if i % 13 == 5 else b"" if i % 31 == 7 else row(i, FILL[i % len(FILL)])
        lines.append((b"f%03d/" % i + (b"ns:a|b", b"ns:k", b"ns:", b"ns:a")[i % 4], text))
    files = [raw_file(sorted(lines))]
    ref = Ref(files)
    preds = {}
    for i, c in enumerate(CASES):
        preds.setdefault((tuple(c.where), c.key_columns, c.skip), []).append(i)
    return ref, open_tables(gpu, files), preds


def test_known_answers_on_the_device(gpu, known):
    """Every distinct predicate of the known answers over the whole table:
    cb_scan_match's flag of every entry (host destination; a device one for
    every tenth predicate), each case's own row against its hand-worked
    answer, and cb_tables_count_where's two ranges against the sums."""
    import torch
    ref, tables, preds = known
    r = gpu.scan_many(tables, prefixes=[b"f", b"g"])
    entries, off = ref.entries, r.range_off().tolist()
    assert r.count == len(entries) > 2 * TILE and r.keys() == [k for k, _, _ in entries]
    assert off[1] > TILE and off[2] - off[1] == len(CASES)  # both ranges cross a block edge
    assert any(is_dead(v) for _, v, _ in entries[:off[1]]) and any(is_dead(v) for _, v, _ in entries[off[1]:])
    at = {k: i for i, (k, _, _) in enumerate(entries)}
    want_live = [sum(not is_dead(v) for _, v, _ in entries[off[i]:off[i + 1]]) for i in range(2)]
    assert gpu.count(tables, prefixes=[b"f", b"g"])[1].tolist() == want_live
    dev = torch.zeros(r.count, dtype=torch.uint8, device="cuda")
    assert len(preds) > 100
    for n, ((where, kc, skip), cases) in enumerate(preds.items()):
        sk = [5 + skip, 6 + skip]
        want = [rowjson_ref.matches(k, v, where, kc, sk[i >= off[1]]) for i, (k, v, _) in enumerate(entries)]
        got = r.match(where, kc, skip=sk)
        assert got.tolist() == want, (where, kc, skip)
        for i in cases:
            assert bool(got[at[b"g%04d/" % i + CASES[i].key]]) is CASES[i].expect, CASES[i].label
        if n % 10 == 0:
            dev.fill_(7)
            r.copy_match(dev, where, kc, skip=sk)
            assert dev.cpu().numpy().tolist() == [int(x) for x in want], (where, kc, skip)
        live, matched = gpu.count_where(tables, where, kc, prefixes=[b"f", b"g"], skip=sk)
        assert live.tolist() == want_live, (where, kc, skip)
        assert matched.tolist() == [sum(want[off[i]:off[i + 1]]) for i in range(2)], (where, kc, skip)
    # one skip for every range: "g0001/ns:k" is the part "k" after 9 bytes, "f001/ns:k" the empty one
    want = [rowjson_ref.matches(k, v, {"pk": "k"}, ("pk",), 9) for k, v, _ in entries]
    assert r.match({"pk": "k"}, ("pk",), skip=9).tolist() == want and sum(want[off[1]:]) > 100 > sum(want[:off[1]])
    assert gpu.count_where(tables, {"pk": "k"}, ("pk",), prefixes=[b"f", b"g"], skip=9)[1].tolist() == \
        [sum(want[off[i]:off[i + 1]]) for i in range(2)]
    # a result of one range, an empty result, and a result of the live scan
    one = gpu.scan(tables, prefix=b"f")
    assert one.match(CV, skip=8).tolist() == [rowjson_ref.matches(k, v, CV, (), 8) for k, v, _ in entries[:off[1]]]
    none = gpu.scan(tables, prefix=b"zz")
    assert none.count == 0 and none.match(CV).shape == (0,)
    assert int(gpu.scan_live(tables, prefixes=[b"f"]).match(CV, skip=[8]).sum()) == \
        sum(rowjson_ref.matches(k, v, CV, (), 8) for k, v, _ in entries[:off[1]])


# ---- k_scan_count_where at its edges ----------------------------------------------------

def edge_files(first):
    """Two tables. Exactly `first` records sort below the matching rows m0,
    m1, m2: single lines (matching, not matching, undecodable, dead), keys with
    a tombstone in the newer table over a matching row in the older one (two
    records, no live row), and keys with an undecodable newer line over a live
    older one (two records, the older one is the row)."""
    newer, older, n, i = [], [], 0, 0
    while n < first:
        k, kind = b"a%04d" % i, i % 7
        i += 1
        if kind == 0 and n + 2 <= first:
            newer.append((k, tomb(900 + i)))
            older.append((k, row(i, HIT)))
            n += 2
            continue
        if kind == 1 and n + 2 <= first:
            newer.append((k, BAD))
            older.append((k, row(i, HIT if i % 2 else MISS)))
            n += 2
            continue
        older.append((k, row(i, HIT) if kind == 2 else BAD if kind == 3 else tomb(i) if kind == 4 else row(i, MISS)))
        n += 1
    older += [(b"m0", row(1, HIT)), (b"m1", row(2, b' {"c" : "v"} ')), (b"m2", row(3, b'{"x":"y","c":"v"}'))]
    newer += [(b"z0", row(4, MISS)), (b"z1", row(5, HIT))]
    older += [(b"z1", row(6, MISS)), (b"z2", row(7, HIT)), (b"z3", tomb(8))]
    return [raw_file(sorted(newer)), raw_file(sorted(older))]


@pytest.mark.parametrize("first", [TILE - 1, TILE, TILE + 1])
def test_matching_rows_at_the_tile_edge(gpu, first):
    """The matching rows m0, m1, m2 are records first, first + 1, first + 2 of
    the sorted order: 255..257, 256..258 and 257..259."""
    files = edge_files(first)
    ref = Ref(files)
    assert sum(k < b"m0" for f in files for k in file_keys(f)) == first
    tables = open_tables(gpu, files)
    live, matched = check_where(gpu, ref, tables, CV, ranges=[(b"", None)])
    assert 3 < matched[0] < live[0] < ref.nlines - 20
    live, matched = check_where(gpu, ref, tables, CV,
                                ranges=[(b"", b"m0"), (b"m0", b"m1"), (b"m1", b"m2\0"), (b"m2\0", None)])
    assert matched[1:] == [1, 2, 2] and live[1:] == [1, 2, 3]
    # a tombstone in the newer table over a matching row in the older one does not count
    k = b"a0000"
    assert k in file_keys(files[0]) and rowjson_ref.matches(k, (1).to_bytes(8, "big") + HIT, CV)
    assert check_where(gpu, ref, tables, CV, ranges=[(k, k + b"\0")]) == ([0], [0])


@pytest.mark.parametrize("nr", [TILE, TILE + 1])
def test_one_row_ranges_in_a_row(gpu, nr):
    """256 and 257 one-row ranges from record 0 on: every lane ends a run."""
    texts = [row(i, HIT) if i % 3 == 0 else tomb(i) if i % 3 == 1 and i % 2 else BAD if i % 7 == 2 else row(i, MISS)
             for i in range(nr)]
    files = [raw_file([(b"k%03d:x" % i, t) for i, t in enumerate(texts)])]
    ref = Ref(files)
    live, matched = check_where(gpu, ref, open_tables(gpu, files), CV, prefixes=[b"k%03d:" % i for i in range(nr)])
    assert set(live) == {0, 1} and set(matched) == {0, 1} and 0 < sum(matched) < sum(live) < nr
    assert matched[TILE - 1] == 1 and (nr == TILE or matched[TILE] == 0)


def test_one_range_over_three_tiles_and_empty_ranges_at_both_ends(gpu):
    lines = [(b"b%04d|%d" % (i, i % 4), row(i, (HIT, MISS, b"{", b'{"c":"v","c":"w"}', b'{"c":"w","c":"v"}')[i % 5]))
             for i in range(2 * TILE + 40)]
    files = [raw_file([(b"a", row(1, HIT))] + lines[1::2] + [(b"c", row(2, HIT))]), raw_file(lines[0::2])]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    ranges = [(b"0", b"1"), (b"a", b"a\0"), (b"a\0", b"b"), (b"b", b"c"), (b"c", b"d"), (b"y", b"z")]
    live, matched = check_where(gpu, ref, tables, CV, ranges=ranges)
    assert live == [0, 1, 0, 2 * TILE + 40, 1, 0] and matched[:3] == [0, 1, 0] and matched[4:] == [1, 0]
    assert matched[3] == sum(i % 5 in (0, 4) for i in range(2 * TILE + 40))
    # a key condition beside the JSON one: "b0123|3" is parts ("0123", "3") after one byte
    live, matched = check_where(gpu, ref, tables, [("c", "v"), ("ck", "3")], ("pk", "ck"), ranges=ranges, skip=1)
    assert matched[3] == sum(i % 5 in (0, 4) and i % 4 == 3 for i in range(2 * TILE + 40)) > 0
    # every range empty: by its bounds (no device work), and by the data; no range; no table with lines
    assert check_where(gpu, ref, tables, CV, ranges=[(b"c", b"b"), (b"d", b"d")]) == ([0, 0], [0, 0])
    assert check_where(gpu, ref, tables, CV, ranges=[(b"0", b"1"), (b"y", b"z")]) == ([0, 0], [0, 0])
    lv, ma = gpu.count_where(tables, CV, ranges=[])
    assert lv.shape == (0,) and ma.shape == (0,)
    empty = [b"", b""]
    assert check_where(gpu, Ref(empty), open_tables(gpu, empty), CV, ranges=[(b"a", b"b"), (b"b", None)]) == ([0, 0], [0, 0])


def test_long_rows_among_short_ones(gpu):
    """Rows of about 300 and 5000 bytes: the match before and after the long
    column, an error at the very end of a long document, and long columns that
    differ from the condition in their last byte."""
    def doc(n, where_first, tail=b""):
        pad = b'"pad":"' + b"p" * n + b'"'
        return b"{" + (b'"c":"v",' + pad if where_first else pad + b',"c":"v"') + b"}" + tail
    long_v = "v" * 1500
    rows = []
    for i, n in enumerate((300, 5000)):
        rows += [(b"r%d0" % i, doc(n, True)), (b"r%d1" % i, doc(n, False)), (b"r%d2" % i, doc(n, True, b"x")),
                 (b"r%d3" % i, doc(n, False, b",")), (b"r%d4" % i, doc(n, False, b" \n")),
                 (b"r%d5" % i, doc(n, True).replace(b'"pad":"pp', b'"pad":"\\u00e9\xc3\xa9')),
                 (b"r%d6" % i, doc(n, True).replace(b'"pad":"pp', b'"pad":"\xc3\x28'))]
    rows += [(b"s0", b'{"c":"' + long_v.encode() + b'"}'), (b"s1", b'{"c":"' + long_v.encode()[:-1] + b'w"}'),
             (b"s2", b'{"c":"' + long_v.encode() + b'v"}')]
    lines = [(k, row(7, p)) for k, p in rows] + [(b"q%03d" % i, row(i, (HIT, MISS)[i % 2])) for i in range(40)]
    files = [raw_file(sorted(lines))]
    ref = Ref(files)
    tables = open_tables(gpu, files)
    assert max(len(v) for _, v, _ in ref.live) > 5000
    live, matched = check_where(gpu, ref, tables, CV, prefixes=[b"q", b"r0", b"r1", b"s"])
    assert live == [40, 7, 7, 3] and matched == [20, 4, 4, 0]
    live, matched = check_where(gpu, ref, tables, [("c", long_v)], prefixes=[b"q", b"r0", b"r1", b"s"])
    assert matched == [0, 0, 0, 1]
    live, matched = check_where(gpu, ref, tables, [("pad", "p" * 300), ("c", "v")], prefixes=[b"r"])
    assert (live, matched) == ([14], [3])


# ---- equalities -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def store(gpu):
    """9 tables x 200 lines over 600 keys "ns%d:pk|ck": JSON rows of three
    short columns, tombstones, undecodable texts and rows that are no JSON,
    with shuffled timestamps so that the LWW winners differ from the newest."""
    rng = np.random.default_rng(4242)
    keys = [b"ns%d:p%02d|c%d" % (i % 3, i // 3 % 50, i // 150) for i in range(600)]
    files = []
    for t in range(9):
        lines = []
        for i in sorted(rng.choice(len(keys), 200, replace=False).tolist()):
            u, ts = rng.random(), int(rng.integers(1, 50))
            payload = b'{"c":"%s","city":"x%d","n":"%d"}' % ((b"v", b"w", b"v\\u0076")[int(rng.integers(0, 3))], i % 7, t)
            text = tomb(ts) if u < 0.2 else BAD if u < 0.25 else row(ts, b"no json") if u < 0.3 else row(ts, payload)
            lines.append((keys[i], text))
        files.append(raw_file(sorted(lines)))
    return Ref(files), open_tables(gpu, files)


def test_no_condition_counts_every_live_row(gpu, store):
    ref, tables = store
    prefixes = [b"ns0:", b"ns1:", b"ns2:"]
    for lww in (False, True):
        live, matched = check_where(gpu, ref, tables, [], prefixes=prefixes, lww=lww)
        assert matched == live and all(x > 50 for x in live)
        assert live == (gpu.count_lww if lww else gpu.count)(tables, prefixes=prefixes)[1].tolist()
    assert lww_live(ref.files) != ref.live


def test_store_predicates(gpu, store):
    """JSON conditions, key conditions and both, newest-wins and LWW, over
    prefixes (the reference's COUNT(*) WHERE: prefix ns + ":", skip its
    length), ranges, and a side stream."""
    import torch
    ref, tables = store
    prefixes = [b"ns0:", b"ns1:", b"ns2:"]
    kc = ("pk", "ck")
    for where in (CV, {"c": "vv"}, {"city": "x3", "c": "v"}, {"pk": "p07"}, {"ck": "c2", "c": "v"},
                  [("pk", "p07"), ("ck", "c1"), ("n", "4")], {"absent": ""}):
        for lww in (False, True):
            live, matched = check_where(gpu, ref, tables, where, kc, prefixes=prefixes, lww=lww)
            assert all(m < lv for m, lv in zip(matched, live))
    assert sum(check_where(gpu, ref, tables, CV, kc, prefixes=prefixes)[1]) > 30
    assert sum(check_where(gpu, ref, tables, {"pk": "p07"}, kc, prefixes=prefixes)[1]) > 3  # rows that are no JSON among them
    check_where(gpu, ref, tables, {"ck": "c2", "c": "v"}, kc, ranges=[(b"ns0:p10", b"ns0:p30"), (b"ns1:", None)], skip=4)
    check_where(gpu, ref, tables, CV, kc, prefixes=prefixes, stream=torch.cuda.Stream())


# ---- tables and order -------------------------------------------------------------------

def test_lww_counts_the_older_tables_matching_row(gpu):
    """Timestamps against table order: the older table's matching row has the
    greater timestamp than the newer table's tombstone (a) and non-matching
    row (b); c is the other way round; d's tombstone wins by timestamp."""
    newer = raw_file([(b"n:a", tomb(5)), (b"n:b", row(5, MISS)), (b"n:c", row(9, HIT)), (b"n:d", row(3, HIT))])
    older = raw_file([(b"n:a", row(8, HIT)), (b"n:b", row(8, HIT)), (b"n:c", row(2, MISS)), (b"n:d", tomb(7)),
                      (b"n:e", row(1, HIT))])
    ref = Ref([newer, older])
    tables = open_tables(gpu, [newer, older])
    assert check_where(gpu, ref, tables, CV, prefixes=[b"n:"]) == ([4], [3])             # b (newer, w), c, d, e
    assert check_where(gpu, ref, tables, CV, prefixes=[b"n:"], lww=True) == ([4], [4])   # a, b (older), c, e
    ranges = [(k, k + b"\0") for k in (b"n:a", b"n:b", b"n:c", b"n:d", b"n:e")]
    assert check_where(gpu, ref, tables, CV, ranges=ranges) == ([0, 1, 1, 1, 1], [0, 0, 1, 1, 1])
    assert check_where(gpu, ref, tables, CV, ranges=ranges, lww=True) == ([1, 1, 1, 0, 1], [1, 1, 1, 0, 1])
