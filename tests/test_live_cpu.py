"""The live-row entries' surface (cb_tables_count, cb_tables_scan_live,
cb_tables_compact_live; lsmt_amd.count, scan_live, compact_live), checked
without a GPU: the header's declarations, the ctypes prototypes, the
integration document and the Python signatures; the argument errors that are
refused before any device is touched, each leaving its outputs cleared; and
the dead-row rule (lsmt_amd/csrc/liverow.hpp) under the address and
undefined-behaviour sanitizers, through a stand-alone driver
(tests/cpp/liverow_driver.cpp), against the restatement of the reference's
split_ts in tests/liverow_ref.py.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import liverow_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_EINVAL, CB_EZEROM = -1, -2
K_BAD_VALUE = 0xFFFFFFFF  # sstable.hpp kBadValue: a value that does not decode

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_tables_count": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "stream", "entries", "live"],
    "cb_tables_scan_live": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "limit", "stream", "out"],
    "cb_tables_compact_live": ["tables", "nt", "m_bits", "stream", "table_out", "bloom_out"],
}
# name -> (parameters, the defaults of all but `tables`)
PYTHON = {
    "count": (["tables", "ranges", "prefixes", "stream"], [None, None, None]),
    "scan_live": (["tables", "ranges", "prefixes", "limit", "stream"], [None, None, 0, None]),
    "compact_live": (["tables", "m", "stream"], [1024, None]),
}


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the live-row entries exist."""
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
    # the header cites the reference lines the rule comes from, and states the caller's rule
    for cite in ("src/query.rs:240-261", "src/query.rs:21-27", "343-346", "395-398"):
        assert cite in raw_header, cite
    assert re.search(r"no\s+older\s+table", raw_header) and re.search(r"no\s+OLDER\s+table", integration)
    for name, (params, defaults) in PYTHON.items():
        assert name in lsmt_amd.__all__
        sig = inspect.signature(getattr(lsmt_amd, name))
        assert list(sig.parameters) == params, name
        assert [p.default for k, p in sig.parameters.items() if k != "tables"] == defaults, name
    # the three functions whose signatures other tests pin are as they were
    assert list(inspect.signature(lsmt_amd.scan_many).parameters) == ["tables", "ranges", "prefixes", "stream"]
    assert list(inspect.signature(lsmt_amd.compact).parameters) == ["tables", "m", "stream"]


def test_the_rule_is_stated_once_in_the_library():
    """liverow.hpp holds the predicate; every other source asks it by name."""
    with open(os.path.join(CSRC, "liverow.hpp")) as fh:
        text = fh.read()
    assert re.search(r"constexpr\s+bool\s+value_dead\s*\(\s*uint32_t\s+vdl\s*\)", text)
    assert "src/query.rs:21-27" in text
    users = []
    for fn in sorted(os.listdir(CSRC)):
        if fn == "liverow.hpp" or not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as fh:
            src = fh.read()
        if "value_dead" in src:
            users.append(fn)
            assert '#include "liverow.hpp"' in src, fn
        # no second spelling of "length 0 or 8" next to a vdl
        assert not re.search(r"vdl\s*==\s*(0|8)\b", src), fn
    assert users == ["compact.hip", "scan.hip"]


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
        rc = L.cb_tables_count(tables, nt, bounds, off, nr, unb, None, e.ctypes.data if entries else None,
                               lv.ctypes.data if live else None)
        return rc, e[:nr].tolist(), lv[:nr].tolist()

    def scan_live(tables, nt, bounds, off, nr, unb=0, limit=0):
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_tables_scan_live(tables, nt, bounds, off, nr, unb, limit, None, ctypes.byref(out))
        return rc, out.value

    def compact_live(tables, nt, m_bits, bloom=True):
        th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xDEAD)
        rc = L.cb_tables_compact_live(tables, nt, m_bits, None, ctypes.byref(th), ctypes.byref(fh) if bloom else None)
        return rc, th.value, fh.value if bloom else None

    # null outputs
    assert L.cb_tables_scan_live(null_entry, 2, b"ab", off1, 1, 0, 0, None, None) == CB_EINVAL
    assert L.cb_tables_compact_live(null_entry, 2, 1024, None, None, None) == CB_EINVAL
    # both count arrays NULL; one of them is enough to get as far as the table list
    assert count(null_entry, 2, b"ab", off1, 1, entries=False, live=False)[0] == CB_EINVAL
    assert "null argument" in last_error(L)
    assert count(null_entry, 2, b"ab", off1, 1, entries=False) == (CB_EINVAL, [0xDEAD], [0])
    assert count(null_entry, 2, b"ab", off1, 1, live=False) == (CB_EINVAL, [0], [0xDEAD])
    # nt == 0 (with and without a list) and a null entry: outputs cleared
    for args, why in [((null_entry, 0), "no tables"), ((None, 0), "no tables"), ((None, 3), "no tables"),
                      ((null_entry, 2), "null table")]:
        assert count(*args, b"abcd", off2, 2) == (CB_EINVAL, [0, 0], [0, 0])
        assert last_error(L) == why
        assert scan_live(*args, b"ab", off1, 1) == (CB_EINVAL, None)
        assert last_error(L) == why
        assert compact_live(*args, 1024) == (CB_EINVAL, None, None)
        assert last_error(L) == why
        assert count(*args, b"", None, 0)[0] == CB_EINVAL  # no range is legal, no table is not
    # limit > 0 takes exactly one range
    assert scan_live(null_entry, 2, b"abcd", off2, 2, limit=5) == (CB_EINVAL, None)
    assert last_error(L) == "a limit takes exactly one range"
    assert scan_live(null_entry, 2, b"ab", off1, 1, limit=5) == (CB_EINVAL, None)
    assert last_error(L) == "null table"  # (one range: the limit is fine)
    # the range list: cb_tables_scan_many's rule through the same check
    bad_lists = [("overlapping", b"adbe", off2, 2, 0),                      # [a, d) and [b, e)
                 ("descending", b"cdab", off2, 2, 0),                       # [c, d) then [a, b)
                 ("unbounded from inside", b"adb", (ctypes.c_uint64 * 5)(0, 1, 2, 3, 3), 2, 1),
                 ("offsets that decrease", b"abcd", (ctypes.c_uint64 * 5)(0, 2, 1, 3, 4), 2, 0)]
    for what, bounds, off, nr, unb in bad_lists:
        assert count(null_entry, 2, bounds, off, nr, unb) == (CB_EINVAL, [0] * nr, [0] * nr), what
        assert "ascending and disjoint" in last_error(L), what
        assert scan_live(null_entry, 2, bounds, off, nr, unb) == (CB_EINVAL, None), what
        assert "ascending and disjoint" in last_error(L), what
    assert scan_live(null_entry, 2, b"", None, 0) == (CB_EINVAL, None) and last_error(L) == "no ranges"
    assert scan_live(null_entry, 2, b"ab", None, 1) == (CB_EINVAL, None) and last_error(L) == "null bound offsets"
    assert count(null_entry, 2, b"ab", None, 1)[0] == CB_EINVAL and last_error(L) == "null bound offsets"
    assert count(null_entry, 2, None, off1, 1)[0] == CB_EINVAL and "null bounds" in last_error(L)
    # m_bits == 0 with a filter asked for
    assert compact_live(null_entry, 2, 0) == (CB_EZEROM, None, None)
    assert last_error(L) == "attempt to calculate the remainder with a divisor of zero"
    assert compact_live(null_entry, 2, 0, bloom=False) == (CB_EINVAL, None, None)  # (no filter: m is not used)
    assert last_error(L) == "null table"
    # the Python entries
    with pytest.raises(ValueError):
        lsmt_amd.count([], ranges=[(b"a", b"b")], prefixes=[b"a"])
    with pytest.raises(ValueError):
        lsmt_amd.scan_live([])
    with pytest.raises(ValueError):
        lsmt_amd.count([], ranges=[(b"a", None), (b"b", b"c")])
    with pytest.raises(ValueError):
        lsmt_amd.scan_live([], prefixes=[b"", b"a"])  # a prefix without an end before the last
    for call in (lambda: lsmt_amd.count([], prefixes=[b"a"]), lambda: lsmt_amd.scan_live([], ranges=[(b"a", b"b")]),
                 lambda: lsmt_amd.compact_live([])):
        with pytest.raises(_lib.CassBloomError) as ei:
            call()  # no tables
        assert ei.value.code == CB_EINVAL
    with pytest.raises(ZeroDivisionError):
        lsmt_amd.compact_live([], m=0)


# ---- the dead rule under the sanitizers -------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("liverow") / "liverow_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "liverow_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def test_split_ts_restated():
    """The restatement against the reference's own words: below 8 bytes the
    value is the payload; from 8 on the first 8 are the timestamp."""
    assert liverow_ref.split_ts(b"") == (0, b"")
    assert liverow_ref.split_ts(b"1234567") == (0, b"1234567")
    assert liverow_ref.split_ts(b"\0\0\0\0\0\0\1\2") == (258, b"")  # exec_delete's tombstone
    assert liverow_ref.split_ts(b"\0\0\0\0\0\0\1\2x") == (258, b"x")
    for n in range(21):
        v = bytes(range(n))
        assert liverow_ref.payload_len(n) == len(liverow_ref.split_ts(v)[1])
        assert liverow_ref.is_dead(v) == (n in (0, 8))


def test_dead_rule_under_sanitizers(driver):
    lengths = list(range(21)) + [2 ** 32 - 2, K_BAD_VALUE]
    r = subprocess.run([driver], input="".join("%d\n" % v for v in lengths), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(a) for a, _ in got] == lengths
    for (a, dead), v in zip(got, lengths):
        # kBadValue is no length: such a line is no entry, and the predicate calls it not dead
        want = False if v == K_BAD_VALUE else liverow_ref.payload_len(v) == 0
        assert (dead == "1") == want, v
    assert [v for (_, d), v in zip(got, lengths) if d == "1"] == [0, 8]
