"""The LWW entries' surface (cb_tables_compact_lww, cb_tables_scan_lww,
cb_tables_count_lww, cb_scan_ts; lsmt_amd.compact_lww, scan_lww, count_lww,
ScanResult.ts), checked without a GPU: the header's declarations, the ctypes
prototypes, the integration document and the Python signatures; the argument
errors that are refused before any device is touched, each leaving its outputs
cleared; and the timestamp rule (lsmt_amd/csrc/rowts.hpp) under the address
and undefined-behaviour sanitizers, through a stand-alone driver
(tests/cpp/rowts_driver.cpp), against the restatement of the reference's fold
in tests/lww_ref.py.
"""
import base64
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import lww_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL, CB_EZEROM = 0, -1, -2

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_tables_compact_lww": ["tables", "nt", "m_bits", "drop_dead", "stream", "table_out", "bloom_out"],
    "cb_tables_scan_lww": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "drop_dead", "limit",
                           "stream", "out"],
    "cb_tables_count_lww": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "stream", "entries",
                            "live"],
    "cb_scan_ts": ["r", "ts"],
}
# name -> (parameters, the defaults of all but `tables`)
PYTHON = {
    "compact_lww": (["tables", "m", "drop_dead", "stream"], [1024, False, None]),
    "scan_lww": (["tables", "ranges", "prefixes", "limit", "drop_dead", "stream"], [None, None, 0, False, None]),
    "count_lww": (["tables", "ranges", "prefixes", "stream"], [None, None, None]),
}


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the LWW entries exist."""
    import lsmt_amd
    from lsmt_amd import _lib
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        raw_header = fh.read()
    header = re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        integration = fh.read()
    for name, names in SYMBOLS.items():
        assert name in _lib.header_symbols()
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name}: no prototype"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        fn = getattr(_lib.load(), name)  # (raises if the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params)
        assert fn.restype is ctypes.c_int
        assert re.search(r"pub fn %s\(" % name, integration), name
    # the new section follows the live-row one and cites the reference lines the rule comes from
    assert raw_header.index("cb_tables_compact_live(") < raw_header.index("cb_tables_compact_lww(")
    for cite in ("src/cluster.rs:405-416", "src/cluster.rs:454-459", "src/query.rs:21-27", "src/query.rs:393-410",
                 "src/lib.rs:154-158"):
        assert cite in raw_header, cite
    # the header says where LWW differs from the live-row entries, and repeats the caller's rule
    lww = raw_header[raw_header.index("last-write-wins by row timestamp"):raw_header.index("cb_scan_ts(")]
    assert "cb_tables_compact_live" in lww and re.search(r"deletes\s+nothing", lww)
    assert re.search(r"no\s+table\s+or\s+replica\s+of\s+the\s+store\s+stays\s+outside", lww)
    assert re.search(r"no\s+table\s+or\s+replica\s+of\s+the\s+store\s+stays\s+outside", integration)
    for name, (params, defaults) in PYTHON.items():
        assert name in lsmt_amd.__all__
        sig = inspect.signature(getattr(lsmt_amd, name))
        assert list(sig.parameters) == params, name
        assert [p.default for k, p in sig.parameters.items() if k != "tables"] == defaults, name
    assert list(inspect.signature(lsmt_amd.ScanResult.ts).parameters) == ["self"]
    # the entries whose signatures other tests pin are as they were
    assert list(inspect.signature(lsmt_amd.scan_live).parameters) == ["tables", "ranges", "prefixes", "limit", "stream"]
    assert list(inspect.signature(lsmt_amd.compact_live).parameters) == ["tables", "m", "stream"]
    assert list(inspect.signature(lsmt_amd.count).parameters) == ["tables", "ranges", "prefixes", "stream"]


def test_the_rule_has_one_home():
    """rowts.hpp defines value_ts and lww_beats; every other source that
    names them includes it, and none defines them again."""
    with open(os.path.join(CSRC, "rowts.hpp")) as fh:
        text = fh.read()
    assert re.search(r"constexpr\s+uint64_t\s+value_ts\s*\(\s*const\s+uint8_t\s*\*\s*text\s*,\s*uint32_t\s+vdl\s*\)", text)
    assert re.search(r"constexpr\s+bool\s+lww_beats\s*\(\s*uint64_t\s+ts_a\s*,\s*uint64_t\s+idx_a\s*,\s*uint64_t\s+ts_b"
                     r"\s*,\s*uint64_t\s+idx_b\s*\)", text)
    for cite in ("src/cluster.rs:405-416", "src/query.rs:21-27", "src/lib.rs:154-158"):
        assert cite in text, cite
    users = []
    for fn in sorted(os.listdir(CSRC)):
        if fn == "rowts.hpp" or not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as fh:
            src = fh.read()
        code = re.sub(r"//[^\n]*", "", src)
        if re.search(r"\b(value_ts|lww_beats|decoded_ts)\s*\(", code):
            users.append(fn)
            assert '#include "rowts.hpp"' in src, fn
        # no second definition (a return type in front of the name)
        assert not re.search(r"\b(uint64_t|bool|auto)\s+(value_ts|lww_beats|decoded_ts)\s*\(", code), fn
    assert users == ["compact.hip", "scan.hip"]
    # the select lives where the dead-row rule's users are pinned
    with open(os.path.join(CSRC, "compact.hip")) as fh:
        compact = fh.read()
    for kernel in ("k_compact_ts", "k_compact_lww_runs", "k_compact_lww_tiles"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, compact), kernel
    with open(os.path.join(CSRC, "scan.hip")) as fh:
        assert re.search(r"__global__[^;{]*\bk_scan_ts\s*\(", fh.read())


# ---- argument errors --------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


def test_argument_errors_need_no_device():
    import lsmt_amd
    from lsmt_amd import _lib
    L = _lib.load()
    null_entry = ctypes.cast((ctypes.c_void_p * 2)(None, None), ctypes.c_void_p)
    off1 = (ctypes.c_uint64 * 3)(0, 1, 2)        # one range: [a, b)
    off2 = (ctypes.c_uint64 * 5)(0, 1, 2, 3, 4)  # two ranges

    def count(tables, nt, bounds, off, nr, unb=0, entries=True, live=True):
        e, lv = np.full(max(nr, 1), 0xDEAD, np.uint64), np.full(max(nr, 1), 0xDEAD, np.uint64)
        rc = L.cb_tables_count_lww(tables, nt, bounds, off, nr, unb, None, e.ctypes.data if entries else None,
                                   lv.ctypes.data if live else None)
        return rc, e[:nr].tolist(), lv[:nr].tolist()

    def scan(tables, nt, bounds, off, nr, unb=0, limit=0, drop=0):
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_tables_scan_lww(tables, nt, bounds, off, nr, unb, drop, limit, None, ctypes.byref(out))
        return rc, out.value

    def compact(tables, nt, m_bits, bloom=True, drop=0):
        th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xDEAD)
        rc = L.cb_tables_compact_lww(tables, nt, m_bits, drop, None, ctypes.byref(th),
                                     ctypes.byref(fh) if bloom else None)
        return rc, th.value, fh.value if bloom else None

    # null outputs
    assert L.cb_tables_scan_lww(null_entry, 2, b"ab", off1, 1, 0, 0, 0, None, None) == CB_EINVAL
    assert last_error(L) == "null argument"
    assert L.cb_tables_compact_lww(null_entry, 2, 1024, 0, None, None, None) == CB_EINVAL
    assert last_error(L) == "null argument"
    assert count(null_entry, 2, b"ab", off1, 1, entries=False, live=False)[0] == CB_EINVAL
    assert "null argument" in last_error(L)
    assert count(null_entry, 2, b"ab", off1, 1, entries=False) == (CB_EINVAL, [0xDEAD], [0])
    assert count(null_entry, 2, b"ab", off1, 1, live=False) == (CB_EINVAL, [0], [0xDEAD])
    # cb_scan_ts: a null result is refused, whatever ts is
    assert L.cb_scan_ts(None, None) == CB_EINVAL and last_error(L) == "null scan"
    # nt == 0 (with and without a list) and a null entry: outputs cleared
    for args, why in [((null_entry, 0), "no tables"), ((None, 0), "no tables"), ((None, 3), "no tables"),
                      ((null_entry, 2), "null table")]:
        assert count(*args, b"abcd", off2, 2) == (CB_EINVAL, [0, 0], [0, 0])
        assert last_error(L) == why
        for drop in (0, 1):
            assert scan(*args, b"ab", off1, 1, drop=drop) == (CB_EINVAL, None)
            assert last_error(L) == why
            assert compact(*args, 1024, drop=drop) == (CB_EINVAL, None, None)
            assert last_error(L) == why
        assert count(*args, b"", None, 0)[0] == CB_EINVAL  # no range is legal, no table is not
    # limit > 0 takes exactly one range
    assert scan(null_entry, 2, b"abcd", off2, 2, limit=5) == (CB_EINVAL, None)
    assert last_error(L) == "a limit takes exactly one range"
    assert scan(null_entry, 2, b"ab", off1, 1, limit=5) == (CB_EINVAL, None)
    assert last_error(L) == "null table"  # (one range: the limit is fine)
    # the range list: cb_tables_scan_many's rule through the same check, before the table list
    bad_lists = [("overlapping", b"adbe", off2, 2, 0),                      # [a, d) and [b, e)
                 ("descending", b"cdab", off2, 2, 0),                       # [c, d) then [a, b)
                 ("unbounded from inside", b"adb", (ctypes.c_uint64 * 5)(0, 1, 2, 3, 3), 2, 1),
                 ("offsets that decrease", b"abcd", (ctypes.c_uint64 * 5)(0, 2, 1, 3, 4), 2, 0)]
    for what, bounds, off, nr, unb in bad_lists:
        assert count(null_entry, 2, bounds, off, nr, unb) == (CB_EINVAL, [0] * nr, [0] * nr), what
        assert "ascending and disjoint" in last_error(L), what
        assert scan(null_entry, 2, bounds, off, nr, unb) == (CB_EINVAL, None), what
        assert "ascending and disjoint" in last_error(L), what
    assert scan(null_entry, 2, b"", None, 0) == (CB_EINVAL, None) and last_error(L) == "no ranges"
    assert scan(null_entry, 2, b"ab", None, 1) == (CB_EINVAL, None) and last_error(L) == "null bound offsets"
    assert count(null_entry, 2, b"ab", None, 1)[0] == CB_EINVAL and last_error(L) == "null bound offsets"
    assert count(null_entry, 2, None, off1, 1)[0] == CB_EINVAL and "null bounds" in last_error(L)
    # m_bits == 0 with a filter asked for: before the table list
    assert compact(null_entry, 2, 0) == (CB_EZEROM, None, None)
    assert last_error(L) == "attempt to calculate the remainder with a divisor of zero"
    assert compact(null_entry, 2, 0, bloom=False) == (CB_EINVAL, None, None)  # (no filter: m is not used)
    assert last_error(L) == "null table"
    # the Python entries
    with pytest.raises(ValueError):
        lsmt_amd.count_lww([], ranges=[(b"a", b"b")], prefixes=[b"a"])
    with pytest.raises(ValueError):
        lsmt_amd.scan_lww([])
    with pytest.raises(ValueError):
        lsmt_amd.count_lww([], ranges=[(b"a", None), (b"b", b"c")])
    with pytest.raises(ValueError):
        lsmt_amd.scan_lww([], prefixes=[b"", b"a"])  # a prefix without an end before the last
    for call in (lambda: lsmt_amd.count_lww([], prefixes=[b"a"]), lambda: lsmt_amd.scan_lww([], ranges=[(b"a", b"b")]),
                 lambda: lsmt_amd.compact_lww([]), lambda: lsmt_amd.compact_lww([], drop_dead=True)):
        with pytest.raises(_lib.CassBloomError) as ei:
            call()  # no tables
        assert ei.value.code == CB_EINVAL
    with pytest.raises(ZeroDivisionError):
        lsmt_amd.compact_lww([], m=0)


# ---- the restatement --------------------------------------------------------------------

def test_fold_restated():
    """tests/lww_ref.py against the reference's own words: `cur_ts >= ts`
    keeps the current row, so the first of equal timestamps stays; the empty
    rows leave after the fold."""
    ts = lambda t, p=b"": t.to_bytes(8, "big") + p  # noqa: E731
    answers = [{b"a": ts(5, b"x"), b"b": ts(7), b"c": b"short"},
               {b"a": ts(5, b"y"), b"b": ts(6, b"live"), b"c": b"", b"d": ts(1, b"d")},
               {b"a": ts(6, b"z"), b"b": ts(8, b"newer")}]
    assert lww_ref.winners(answers) == [(b"a", ts(6, b"z"), 2, 6), (b"b", ts(8, b"newer"), 2, 8),
                                        (b"c", b"short", 0, 0), (b"d", ts(1, b"d"), 1, 1)]
    assert lww_ref.winners(answers[:2]) == [(b"a", ts(5, b"x"), 0, 5), (b"b", ts(7), 0, 7), (b"c", b"short", 0, 0),
                                            (b"d", ts(1, b"d"), 1, 1)]
    # the tombstone b@7 wins over the live b@6 and is dropped afterwards: b does not come back
    assert [k for k, _, _, _ in lww_ref.winners(answers[:2], drop_dead=True)] == [b"a", b"c", b"d"]
    assert lww_ref.winners([]) == [] and lww_ref.winners([{}, {}]) == []


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rowts") / "rowts_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rowts_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def run_driver(driver, requests):
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.split()
    assert len(got) == len(requests)
    return [int(x) for x in got]


TIMESTAMPS = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 0x0102030405060708, 0x0102030405060709, 0xFFFFFFFFFFFFFF00,
              0xFFFFFFFFFFFFFF01, 0xFBEFBEFBEFBEFBEF, 0xFFEFFEFFEFFEFFEF]  # (the last two spell '+' and '/')


def test_value_ts_under_sanitizers(driver):
    values = []
    for n in range(21):  # decoded lengths 0..20, every byte set so a misread shows
        values.append(bytes((0xA5 + 17 * i) & 0xFF for i in range(n)))
    for t in TIMESTAMPS:
        for tail in (b"", b"p", b"pa", b"pay", b"payload-of-12"):
            values.append(t.to_bytes(8, "big") + tail)
    # pairs that differ in the lowest byte only, bit by bit: the 11th character carries its low 6 bits
    for bit in range(8):
        values.append((0x1122334455667700 | 1 << bit).to_bytes(8, "big") + b"x")
    want = [lww_ref.ts_of(v) for v in values]
    assert want[:8] == [0] * 8 and want[8] != 0 and len(set(want[-8:])) == 8
    text = [base64.b64encode(v).decode() for v in values]
    assert all(len(t) >= 12 for v, t in zip(values, text) if len(v) >= 8)
    got = run_driver(driver, ["T %d %s" % (len(v), t or "-") for v, t in zip(values, text)])
    assert got == want
    got = run_driver(driver, ["D %s" % (v.hex() or "-") for v in values])
    assert got == want


def test_lww_beats_under_sanitizers(driver):
    grid = [(t, i) for t in (0, 1, 5, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1) for i in (0, 2, 5, 2 ** 32 - 1)]
    pairs = [(a, b) for a in grid for b in grid if a[1] != b[1]]
    got = run_driver(driver, ["B %d %d %d %d" % (a + b) for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        # the fold meets the lower index first and replaces it only for a strictly greater timestamp
        first, second = (a, b) if a[1] < b[1] else (b, a)
        winner = second if second[0] > first[0] else first
        assert g == int(winner == a), (a, b)
    # exactly one of a pair wins
    by = dict(zip(pairs, got))
    assert all(by[(a, b)] + by[(b, a)] == 1 for a, b in pairs)
