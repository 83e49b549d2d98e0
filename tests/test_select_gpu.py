"""cb_scan_select and cb_rows_select: the response bytes of the reference's
SELECT a, b FROM t WHERE pk IN (...) (exec_select_schema, src/query.rs:365-432),
written on the device from rows that are already there.

The contract. For rows (key, value) and a selection, the result's text is the
reference's response, byte for byte: `[` + the rows' objects joined by `,` +
`]` for a client, the `key \\t ts \\t object` lines joined by `\\n` for a
coordinator; per row, flags, row_at and row_len say what the row is and where
its text lies. The rule is lsmt_amd/csrc/rowselect.hpp's.

Every expectation comes from `Ref` as tests/test_live_gpu.py builds it (the C
oracle's get_many over hand-written files: Database::get's walk), projected
with tests/rowselect_ref.py, the rule's independent restatement; the LWW case
takes its winners from tests/lww_ref.py. Every comparison is exact.

Shapes are the smallest at which the kernels can go wrong: the known answers of
tests/select_cases.py among filler in one result of more than 256 rows (the
block of both kernels), 255, 256 and 257 rows, the only row with text as the
first and as the last of a block, no row with text, one row, dead and absent
rows first, last and in runs, rows of about 64 KiB among rows of about 30
bytes, and ranges with skips of their own.
"""
import base64
import ctypes

import numpy as np
import pytest

import lww_ref
import rowselect_ref as ref
from merge_help import b64, BAD, open_tables, raw_file, row, TILE, tomb
from select_cases import CASES, flags_of, json_text, meta_text
from test_live_gpu import Ref
from test_select_cpu import COLUMNS, S, i32s, mutated_docs, u64s
from test_where_gpu import lww_live

pytestmark = pytest.mark.gpu

BLOCK = 256  # select.hpp kSelectBlock
assert BLOCK == TILE
KC = ("pk", "ck")
ABC = ["a", "b", "pk"]


# ---- expectations -----------------------------------------------------------------------

def check_result(res, rows, sel, meta, on_device=False):
    """res (a RowsResult) against the restatement over rows = [(key, value,
    skip, absent)]: the response, every row's flags, place and text, the
    counts, and the separators around every text."""
    want = [ref.row_text(k, v, sel, s, meta, absent) for k, v, s, absent in rows]
    texts, flags = [t for t, _ in want], [f for _, f in want]
    response = ref.response(texts, meta)
    text = res.text()
    assert text == response, (len(text), len(response))
    assert (res.count, res.with_text, res.bytes) == (len(rows), sum(t is not None for t in texts), len(response))
    assert len(res) == len(rows)
    got_flags = res.flags()
    assert got_flags.dtype == np.uint8 and got_flags.tolist() == flags
    at, ln = res.spans()
    assert at.dtype == np.uint64 and ln.dtype == np.uint64
    assert res.rows() == [t or b"" for t in texts]
    end = 1 if not meta else 0  # where the next text may begin
    sep = b"," if not meta else b"\n"
    for i, t in enumerate(texts):
        assert bool(got_flags[i] & ref.TEXT) == (t is not None) == (ln[i] > 0), i
        if t is None:
            continue
        a, n = int(at[i]), int(ln[i])
        assert text[a:a + n] == t, i
        assert a == end or (a == end + 1 and text[end:a] == sep), (i, a, end)  # one separator, and none before the first
        end = a + n
    assert end + (0 if meta else 1) == len(text) or (not any(t is not None for t in texts))  # nothing behind the last
    if on_device:
        import torch
        d_text = torch.full((max(res.bytes, 1),), 0xAD, dtype=torch.uint8, device="cuda")
        d_at, d_ln = (torch.zeros(max(res.count, 1), dtype=torch.int64, device="cuda") for _ in range(2))
        d_fl = torch.full((max(res.count, 1),), 0xAD, dtype=torch.uint8, device="cuda")
        res.copy(text=d_text, row_at=d_at, row_len=d_ln, flags=d_fl)
        assert d_text[:res.bytes].cpu().numpy().tobytes() == text
        assert d_at[:res.count].cpu().numpy().view(np.uint64).tolist() == at.tolist()
        assert d_ln[:res.count].cpu().numpy().view(np.uint64).tolist() == ln.tolist()
        assert d_fl[:res.count].cpu().numpy().tolist() == flags
    return texts, flags


def check_scan(r, entries, columns, key_columns=(), casts=None, skip=None, on_device=False):
    """ScanResult.select over r, whose entries are `entries` = [(key, value,
    which)], in both modes. Returns the JSON mode's (texts, flags)."""
    sel = ref.normalize(columns, key_columns, casts)
    off = r.range_off().tolist()
    per = [0] * r.nranges if skip is None else [skip] * r.nranges if isinstance(skip, int) else list(skip)
    rows = [(k, v, per[g], False) for g in range(r.nranges) for k, v, _ in entries[off[g]:off[g + 1]]]
    assert len(rows) == r.count == len(entries)
    out = None
    for meta in (True, False):
        res = r.select(columns, key_columns, casts, skip=skip, meta=meta)
        out = check_result(res, rows, sel, meta, on_device)
        res.close()
    return out


class Got:
    """What an enqueue-only get_many of `keys` leaves in device memory."""

    def __init__(self, gpu, tables, keys, cap, stream=None):
        import torch
        data = b"".join(keys) or b"\0"
        off = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([len(k) for k in keys], out=off[1:])
        self.batch = gpu.KeyBatch(n=len(keys), data=torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda(),
                                  offsets=torch.from_numpy(off).cuda())
        n = len(keys)
        self.which = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        self.voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.vals = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fills ran on the null stream; the get may run on another)
        assert gpu.get_many(tables, self.batch, out=(self.which, self.voff, self.vals), stream=stream, wait=False)[2] is None


def check_get(gpu, ref_, tables, keys, columns, key_columns=(), casts=None, skip=0, on_device=False, stream=None,
              no_which=False):
    """select_rows over an enqueue-only get_many of `keys`, in both modes,
    with no wait between the get and the selection."""
    found = {k: v for k, v, _ in ref_.entries}
    sel = ref.normalize(columns, key_columns, casts)
    rows = [(k, found.get(k, b""), skip, k not in found) for k in keys]
    assert not no_which or all(k in found for k in keys)
    out = None
    for meta in (True, False):
        g = Got(gpu, tables, keys, sum(len(v) for v in found.values()), stream)
        res = gpu.select_rows(g.batch, None if no_which else g.which, g.voff, g.vals, columns, key_columns, casts,
                              skip=skip, meta=meta, stream=stream)
        out = check_result(res, rows, sel, meta, on_device)
        res.close()
    return out


# ---- the known answers, on the device ---------------------------------------------------

FILL = [b'{"a":"1"}', b'{"a":"2","b":"\\n"}', b'{"c":"v","d":"e"}', b"not json", b'{"pk":"a","a":"+07"}', b'{"a":"v"} ',
        b'{"a":"v"}x', b"{}"]


@pytest.fixture(scope="module")
def known(gpu):
    """One table: every case of tests/select_cases.py that is a row, under
    "g" (its key after a 6-byte prefix), 300 filler rows under "f" (5-byte
    prefixes), tombstones and an undecodable text among them; and the distinct
    selections of the cases, each with the cases that use it."""
    cases = [c for c in CASES if not c.absent]
    lines = [(b"g%04d/" % i + c.key, b64(c.value)) for i, c in enumerate(cases)]
    for i in range(300):
        text = tomb(i) if i % 9 == 0 else BAD if i % 13 == 5 else b"" if i % 31 == 7 else row(i, FILL[i % len(FILL)])
        lines.append((b"f%03d/" % i + (b"ns:a|b", b"ns:k", b"ns:", b"ns:a")[i % 4], text))
    files = [raw_file(sorted(lines))]
    sels = {}
    for i, c in enumerate(cases):
        casts = tuple(sorted(c.casts.items())) if c.casts else None
        sels.setdefault((c.columns, c.key_columns, casts, c.skip), []).append(i)
    return Ref(files), open_tables(gpu, files), cases, sels


def test_known_answers_through_a_scan_result(gpu, known):
    """Every distinct selection of the known answers over the whole table
    (two ranges, each with its own skip), both modes: the response and every
    row against the restatement, each case's own row against its hand-worked
    text and flags."""
    ref_, tables, cases, sels = known
    r = gpu.scan_many(tables, prefixes=[b"f", b"g"])
    entries, off = ref_.entries, r.range_off().tolist()
    assert r.count == len(entries) > BLOCK and off[1] > BLOCK and off[2] - off[1] == len(cases)
    at = {k: i for i, (k, _, _) in enumerate(entries)}
    assert len(sels) > 15
    for n, ((columns, kc, casts, skip), users) in enumerate(sels.items()):
        sk = [5 + skip, 6 + skip]
        sel = ref.normalize(columns, kc, dict(casts) if casts else None)
        rows = [(k, v, sk[i >= off[1]], False) for i, (k, v, _) in enumerate(entries)]
        for meta in (False, True):
            res = r.select(columns, kc, dict(casts) if casts else None, skip=sk, meta=meta)
            texts, flags = check_result(res, rows, sel, meta, on_device=n % 10 == 0)
            res.close()
            for i in users:
                c, j = cases[i], at[b"g%04d/" % i + cases[i].key]
                # (in the meta form the case's key is the row's key after its 6-byte prefix and the case's own skip)
                assert texts[j] == (meta_text(c) if meta else json_text(c)), c.label
                assert flags[j] == flags_of(c, meta), c.label


def test_known_answers_through_a_get(gpu, known):
    """The same selections over an enqueue-only get_many of the cases' keys,
    every seventh key replaced by one that no table holds (which = -1)."""
    ref_, tables, cases, sels = known
    keys = [b"g%04d/" % i + c.key for i, c in enumerate(cases)]
    keys = [k + b"?" if i % 7 == 3 else k for i, k in enumerate(keys)]
    for n, ((columns, kc, casts, skip), users) in enumerate(sels.items()):
        texts, flags = check_get(gpu, ref_, tables, keys, columns, kc, dict(casts) if casts else None, skip=6 + skip,
                                 on_device=n % 10 == 0)
        for i in users:
            c = cases[i]
            if i % 7 == 3:
                assert (texts[i], flags[i]) == (None, ref.ABSENT)
            else:
                assert (texts[i], flags[i]) == (json_text(c), flags_of(c, False)), c.label


def test_mutated_documents_on_the_device(gpu):
    """tests/test_select_cpu.py's mutated documents as the rows of one table:
    the kernels (the device compiler's reading of the rule, under divergence:
    every lane is in another state of the walker) against the restatement,
    every selection of that test over every document."""
    docs = mutated_docs()
    ts = (77).to_bytes(8, "big")
    files = [raw_file([(b"m%04d/ns:k|x" % i, b64(ts + d if i % 7 else d)) for i, d in enumerate(docs)])]
    ref_, tables = Ref(files), open_tables(gpu, files)
    r = gpu.scan(tables)
    assert r.count == len(docs)
    bad = 0
    for columns in COLUMNS:
        texts, flags = check_scan(r, ref_.entries, columns, KC, casts={"n": 1}, skip=9)
        bad += sum(bool(f & ref.BADJSON) for f in flags)
    assert bad > 2000
    check_get(gpu, ref_, tables, [k for k, _, _ in ref_.entries[::3]], COLUMNS[0], KC, casts={"n": 1}, skip=9)


# ---- the kernels' edges -----------------------------------------------------------------

def pattern_files(kinds):
    """One table of len(kinds) rows "r%04d|x": L a live row, D a tombstone,
    U an undecodable line (no entry at all)."""
    text = {"L": lambda i: row(i, b'{"a":"%d","b":"x"}' % i), "D": tomb, "U": lambda i: BAD}
    return [raw_file([(b"r%04d|x" % i, text[k](i)) for i, k in enumerate(kinds)])]


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_row_counts_around_one_block(gpu, n):
    kinds = "".join("LD"[i % 5 == 2] for i in range(n))
    files = pattern_files(kinds)
    ref_, tables = Ref(files), open_tables(gpu, files)
    r = gpu.scan(tables)
    assert r.count == n
    texts, _ = check_scan(r, ref_.entries, ABC, KC, on_device=True)
    assert sum(t is not None for t in texts) == kinds.count("L")
    check_get(gpu, ref_, tables, [k for k, _, _ in ref_.entries], ABC, KC, no_which=True)


@pytest.mark.parametrize("at", [0, BLOCK - 1, BLOCK, 2 * BLOCK + 3])
def test_the_only_row_with_text(gpu, at):
    """One live row among tombstones, as the first and the last row of a
    block: the brackets and that row alone for a client."""
    n = 2 * BLOCK + 4
    files = pattern_files("".join("L" if i == at else "D" for i in range(n)))
    ref_, tables = Ref(files), open_tables(gpu, files)
    r = gpu.scan(tables)
    texts, flags = check_scan(r, ref_.entries, ABC, KC)
    assert [i for i, t in enumerate(texts) if t is not None] == [at]
    res = r.select(ABC, KC)
    assert res.text() == b'[{"a":"%d","b":"x","pk":"r%04d"}]' % (at, at) and res.with_text == 1
    assert int(res.spans()[0][at]) == 1


def test_no_row_with_text(gpu):
    """Tombstones alone give [] for a client (and a line each for a
    coordinator); absent rows alone give [] and no byte at all; so does an
    empty result."""
    n = BLOCK + 2
    files = pattern_files("D" * n)
    ref_, tables = Ref(files), open_tables(gpu, files)
    r = gpu.scan(tables)
    check_scan(r, ref_.entries, ABC, KC)
    res = r.select(ABC, KC)
    assert (res.text(), res.with_text, res.count, res.rows()) == (b"[]", 0, n, [b""] * n)
    missing = [b"q%04d" % i for i in range(n)]
    texts, flags = check_get(gpu, ref_, tables, missing, ABC, KC, on_device=True)
    assert texts == [None] * n and flags == [ref.ABSENT] * n
    g = Got(gpu, tables, missing, 0)
    for meta, want in ((False, b"[]"), (True, b"")):
        res = gpu.select_rows(g.batch, g.which, g.voff, g.vals, ABC, KC, meta=meta)
        assert (res.text(), res.bytes, res.with_text) == (want, len(want), 0)
    none = gpu.scan(tables, prefix=b"zz")
    assert none.count == 0
    for meta, want in ((False, b"[]"), (True, b"")):
        res = none.select(ABC, KC, meta=meta)
        assert (res.text(), res.count, res.rows(), res.flags().tolist()) == (want, 0, [], [])


@pytest.mark.parametrize("kinds", ["DLLD", "DDDLDDLLDDD", "LDDDL", "D" * (BLOCK - 1) + "LL" + "D" * BLOCK + "L" + "D" * 3,
                                   "L" + "D" * (2 * BLOCK) + "L"], ids=["ends", "runs", "inside", "block-edge", "two-blocks"])
def test_separators_around_rows_without_text(gpu, kinds):
    """Dead rows (no text for a client) and absent rows (none in either mode)
    first, last and in runs: no leading, trailing or doubled separator."""
    files = pattern_files(kinds)
    ref_, tables = Ref(files), open_tables(gpu, files)
    texts, _ = check_scan(gpu.scan(tables), ref_.entries, ["a"], KC, skip=0)
    assert [t is not None for t in texts] == [k == "L" for k in kinds]
    res = gpu.scan(tables).select(["a"])
    text = res.text()
    assert text.startswith(b'[{"a"') and text.endswith(b'"}]') and b",," not in text and text.count(b"},{") == kinds.count("L") - 1
    # the same pattern with the D rows absent: a get of keys that no table holds
    keys = [k if kinds[i] == "L" else k + b"?" for i, (k, _, _) in enumerate(ref_.entries)]
    texts, flags = check_get(gpu, ref_, tables, keys, ["a"], KC)
    assert [f == ref.ABSENT for f in flags] == [k == "D" for k in kinds]
    g = Got(gpu, tables, keys, sum(len(v) for _, v, _ in ref_.entries))
    text = gpu.select_rows(g.batch, g.which, g.voff, g.vals, ["a"], KC, meta=True).text()
    assert text.count(b"\n") == kinds.count("L") - 1 and b"\n\n" not in text
    assert not text.startswith(b"\n") and not text.endswith(b"\n")


def test_long_rows_among_short_ones(gpu):
    """Rows of about 64 KiB among rows of about 30 bytes: a value whose
    escapes shrink when written (\\u0022 is 6 bytes read, 2 written), one
    whose bytes expand against what was unescaped (a control byte is 1 byte
    unescaped, 6 written) and a key part that expands (a quote is 1 byte in
    the key, 2 written); the long column first, last and not selected."""
    n = 10900
    shrink, same = b"\\u0022" * n, b"\\u0001\\n" * (n * 3 // 4)
    quotes = b'"' * 180
    rows = [(b"k00|c", b'{"a":"1","b":"2"}'),
            (b"k01|c", b'{"a":"' + shrink + b'","b":"2"}'),
            (b"k02|c", b'{"b":"2","a":"' + same + b'"}'),
            (b"k03|c", b'{"z":"' + shrink + b'","a":"1"}'),
            (b"k04|" + quotes, b'{"a":"' + same + b'","n":"' + b"0" * 60000 + b'17"}'),
            (b"k05|c", b'{"a":"' + shrink + b'"}x'),
            (b"k06|c", b'{"a":"1","a":"' + shrink + b'","a":"3"}')]
    rows += [(b"m%03d|c" % i, b'{"a":"%d","b":"y"}' % i) for i in range(40)]
    files = [raw_file(sorted((k, row(9, p)) for k, p in rows))]
    ref_, tables = Ref(files), open_tables(gpu, files)
    assert max(len(v) for _, v, _ in ref_.entries) > 65000
    texts, flags = check_scan(gpu.scan(tables), ref_.entries, ["a", "b", "ck", "n", "pk"], KC, casts={"n": 1}, on_device=True)
    assert texts[1] == b'{"a":"' + b'\\"' * n + b'","b":"2","ck":"c","pk":"k01"}'
    assert texts[4].endswith(b'","ck":"' + b'\\"' * 180 + b'","n":"17","pk":"k04"}')
    assert flags[:7] == [1, 1, 1, 17, 1, 9, 1] and texts[6].startswith(b'{"a":"3",')
    check_get(gpu, ref_, tables, [k for k, _, _ in ref_.entries], ["a", "ck", "n"], KC, casts={"n": 1})


# ---- ranges, tables and order -----------------------------------------------------------

def test_ranges_with_their_own_skips_and_empty_ranges_at_both_ends(gpu):
    lines = [(b"aa:%03d|x" % i, row(i, b'{"a":"%d"}' % i)) for i in range(BLOCK + 10)]
    lines += [(b"b:%02d|y" % i, row(i, b'{"a":"b%d","pk":"no"}' % i) if i % 4 else tomb(i)) for i in range(30)]
    lines += [(b"cccc:k|%d" % i, row(i, b"no json" if i % 3 == 0 else b'{"b":"%d"}' % i)) for i in range(9)]
    files = [raw_file(sorted(lines))]
    ref_, tables = Ref(files), open_tables(gpu, files)
    prefixes, skips = [b"0", b"aa:", b"ab", b"b:", b"cccc:", b"zz"], [7, 3, 0, 2, 5, 1]
    r = gpu.scan_many(tables, prefixes=prefixes)
    assert r.range_off().tolist() == [0, 0, BLOCK + 10, BLOCK + 10, BLOCK + 40, BLOCK + 49, BLOCK + 49]
    texts, _ = check_scan(r, ref_.entries, ["a", "b", "ck", "pk"], KC, skip=skips, on_device=True)
    assert texts[0] == b'{"a":"0","ck":"x","pk":"000"}' and texts[BLOCK + 11] == b'{"a":"b1","ck":"y","pk":"01"}'
    assert texts[-1] == b'{"b":"8","ck":"8","pk":"k"}'
    check_scan(r, ref_.entries, ["a", "pk"], KC, skip=4)   # one skip for every range
    check_scan(r, ref_.entries, ["a", "pk"], KC)           # none: the whole key is the first part
    one = gpu.scan(tables, prefix=b"b:")
    check_scan(one, Ref.cut(ref_.entries, b"b:", b"b;"), ["a", "pk"], KC, skip=[2])
    live = gpu.scan_live(tables, prefixes=[b"b:"])
    texts, _ = check_scan(live, Ref.cut(ref_.live, b"b:", b"b;"), ["a"], skip=2)
    assert all(t is not None for t in texts) and len(texts) == 22


def test_an_lww_result_projects_the_older_tables_row(gpu):
    """Timestamps against table order: the older table's row has the greater
    timestamp than the newer table's tombstone (a) and row (b); c is the other
    way round; d's tombstone wins by timestamp."""
    new, old = b'{"a":"new"}', b'{"a":"old"}'
    newer = raw_file([(b"n:a", tomb(5)), (b"n:b", row(5, new)), (b"n:c", row(9, new)), (b"n:d", row(3, new))])
    older = raw_file([(b"n:a", row(8, old)), (b"n:b", row(8, old)), (b"n:c", row(2, old)), (b"n:d", tomb(7)),
                      (b"n:e", row(1, old))])
    files = [newer, older]
    ref_, tables = Ref(files), open_tables(gpu, files)
    texts, _ = check_scan(gpu.scan_many(tables, prefixes=[b"n:"]), ref_.entries, ["a", "pk"], ("pk",), skip=2)
    assert texts == [None, b'{"a":"new","pk":"b"}', b'{"a":"new","pk":"c"}', b'{"a":"new","pk":"d"}', b'{"a":"old","pk":"e"}']
    answers = [{ln.split(b"\t")[0]: base64.b64decode(ln.split(b"\t")[1]) for ln in f.split(b"\n") if ln} for f in files]
    winners = [(k, v, w) for k, v, w, _ in lww_ref.winners(answers, drop_dead=False)]
    r = gpu.scan_lww(tables, prefixes=[b"n:"])
    assert r.keys() == [k for k, _, _ in winners] and r.which().tolist() == [1, 1, 0, 1, 1]
    texts, _ = check_scan(r, winners, ["a", "pk"], ("pk",), skip=2)
    assert texts == [b'{"a":"old","pk":"a"}', b'{"a":"old","pk":"b"}', b'{"a":"new","pk":"c"}', None, b'{"a":"old","pk":"e"}']
    res = r.select(["a"], meta=True, skip=2)
    assert res.text() == b'a\t8\t{"a":"old"}\nb\t8\t{"a":"old"}\nc\t9\t{"a":"new"}\nd\t7\t\ne\t1\t{"a":"old"}'
    live = gpu.scan_lww(tables, prefixes=[b"n:"], drop_dead=True)
    assert check_scan(live, lww_live(files), ["a"], skip=2)[0] == [b'{"a":"old"}'] * 2 + [b'{"a":"new"}', b'{"a":"old"}']


def test_rows_from_host_arrays_a_side_stream_and_fixed_keys(gpu):
    """select_rows copies host arrays to the device itself; which=None means
    every row is present; fixed-length keys are a ragged batch of equal
    lengths; a side stream orders the selection behind the get."""
    import torch
    lines = [(b"ns:%05d" % i, row(i, b'{"a":"%d","n":"%+04d"}' % (i, i - 150))) for i in range(300)]
    files = [raw_file(lines)]
    ref_, tables = Ref(files), open_tables(gpu, files)
    keys = [k for k, _, _ in ref_.entries]
    sel = ref.normalize(["a", "n", "pk"], ("pk",), {"n": 1})
    rows = [(k, v, 3, False) for k, v, _ in ref_.entries]
    voff = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(v) for _, v, _, _ in rows], out=voff[1:])
    vals = np.frombuffer(b"".join(v for _, v, _, _ in rows), np.uint8)
    fixed = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 8)
    for batch in (keys, fixed, gpu.DeviceKeys(torch.from_numpy(fixed.copy()).cuda())):
        res = gpu.select_rows(batch, None, voff, vals, ["pk", "n", "a"], ("pk",), {"n": 1}, skip=3)
        texts, _ = check_result(res, rows, sel, False)
        assert texts[0] == b'{"a":"0","n":"-150","pk":"00000"}' and texts[151] == b'{"a":"151","n":"1","pk":"00151"}'
    which = np.zeros(len(rows), np.int32)
    which[[0, 5, 6, 299]] = -1
    res = gpu.select_rows(keys, which, voff, vals, ["a"], skip=3, meta=True)
    check_result(res, [(k, v, 3, i in (0, 5, 6, 299)) for i, (k, v, _, _) in enumerate(rows)], ref.normalize(["a"]), True)
    check_get(gpu, ref_, tables, keys[::-1] + [b"ns:nope"], ["a", "n", "pk"], ("pk",), {"n": 1}, skip=3,
              stream=torch.cuda.Stream())
    # rows in host memory are refused by the C entry itself
    s, h = S(b"a", u64s(0, 1), i32s(-1), None, 1), ctypes.c_void_p()
    with pytest.raises(gpu._lib.CassBloomError) as ei:
        gpu._lib.check(gpu._lib.load().cb_rows_select(b"kk", u64s(0, 1, 2), None, b"vv", u64s(0, 1, 2), 2, 0,
                                                      ctypes.addressof(s), 0, 0, None, ctypes.byref(h)))
    assert ei.value.code == -1 and "device memory" in str(ei.value)
