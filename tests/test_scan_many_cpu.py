"""The batched scan's surface (cb_tables_scan_many, cb_tables_scan_prefixes,
cb_scan_ranges; lsmt_amd.scan_many), checked without a GPU: the header's
declarations, the ctypes prototypes and the integration document, the
argument errors that are refused before any device is touched, and the
ordering rule of a range list (ascending, pairwise disjoint, only the last
unbounded) under the address and undefined-behaviour sanitizers, through a
stand-alone driver of the host-only code behind it
(tests/cpp/rangelist_driver.cpp over lsmt_amd/csrc/keyrange.hpp), against a
brute-force restatement of the rule written here.
"""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_EINVAL = -1

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_tables_scan_many": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "stream", "out"],
    "cb_tables_scan_prefixes": ["tables", "nt", "prefixes", "prefix_off", "np", "stream", "out"],
    "cb_scan_ranges": ["r", "nr", "range_off"],
}


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry point in one: the
    test that cannot pass before the batched scan exists."""
    import lsmt_amd
    from lsmt_amd import _lib
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        header = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
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
    assert "scan_many" in lsmt_amd.__all__
    sig = inspect.signature(lsmt_amd.scan_many)
    assert list(sig.parameters) == ["tables", "ranges", "prefixes", "stream"]
    assert all(p.default is None for k, p in sig.parameters.items() if k != "tables")
    assert callable(lsmt_amd.ScanResult.range_off)
    assert "nranges" in inspect.getsource(lsmt_amd.ScanResult.__init__)


def test_argument_errors_need_no_device():
    import lsmt_amd
    from lsmt_amd import _lib
    L = _lib.load()
    out = ctypes.c_void_p(0xDEAD)
    null_entry = (ctypes.c_void_p * 2)(None, None)
    tables = ctypes.cast(null_entry, ctypes.c_void_p)
    off = (ctypes.c_uint64 * 3)(0, 1, 2)
    poff = (ctypes.c_uint64 * 2)(0, 1)
    # out NULL
    assert L.cb_tables_scan_many(tables, 2, b"ab", off, 1, 0, None, None) == CB_EINVAL
    assert L.cb_tables_scan_prefixes(tables, 2, b"a", poff, 1, None, None) == CB_EINVAL
    # nt == 0 (with and without a list), a null entry: nothing returned
    for args in [(tables, 0), (None, 0), (None, 3), (tables, 2)]:
        out.value = 0xDEAD
        assert L.cb_tables_scan_many(*args, b"ab", off, 1, 0, None, ctypes.byref(out)) == CB_EINVAL
        assert out.value is None
        assert L.cb_last_error()
        out.value = 0xDEAD
        assert L.cb_tables_scan_prefixes(*args, b"a", poff, 1, None, ctypes.byref(out)) == CB_EINVAL
        assert out.value is None
    n = ctypes.c_uint64()
    assert L.cb_scan_ranges(None, ctypes.byref(n), None) == CB_EINVAL
    assert L.cb_scan_ranges(None, None, None) == CB_EINVAL
    # the Python entry: exactly one of ranges and prefixes; hi=None on the last range only
    with pytest.raises(ValueError):
        lsmt_amd.scan_many([], ranges=[(b"a", b"b")], prefixes=[b"a"])
    with pytest.raises(ValueError):
        lsmt_amd.scan_many([])
    with pytest.raises(ValueError):
        lsmt_amd.scan_many([], ranges=[(b"a", None), (b"b", b"c")])
    for kw in ({"ranges": [(b"a", b"b")]}, {"prefixes": [b"a"]}):
        with pytest.raises(_lib.CassBloomError) as ei:
            lsmt_amd.scan_many([], **kw)  # no tables
        assert ei.value.code == CB_EINVAL


# ---- the ordering rule, restated ----------------------------------------------------------

def first_bad(ranges):
    """The first r whose successor starts below lo_r or hi_r (bytes compare as
    Rust's `Ord for [u8]` does), or -1. ranges = [(lo, hi)]; the last hi is
    not part of the rule."""
    for r in range(len(ranges) - 1):
        lo, hi = ranges[r]
        if lo > ranges[r + 1][0] or hi > ranges[r + 1][0]:
            return r
    return -1


ALPHA = b"abc"
UNIVERSE = sorted(bytes(k) for n in range(4) for k in itertools.product(ALPHA, repeat=n))  # every key of <= 3 letters


def members(lo, hi):
    return [k for k in UNIVERSE if lo <= k and (hi is None or k < hi)]


def random_lists(seed, n):
    """Lists of 1-6 ranges whose bounds are 0-2 letters of a 3-letter alphabet:
    sorted bounds (mostly legal: touches, empties, equal bounds), the same
    with two bounds swapped, and unsorted ones."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nr = int(rng.integers(1, 7))
        b = [bytes(ALPHA[i] for i in rng.integers(0, 3, int(rng.integers(0, 3)))) for _ in range(2 * nr)]
        mode = int(rng.integers(0, 3))
        if mode < 2:
            b.sort()
        if mode == 1:
            i, j = rng.integers(0, 2 * nr, 2)
            b[i], b[j] = b[j], b[i]
        out.append(([(b[2 * r], b[2 * r + 1]) for r in range(nr)], int(rng.integers(0, 2))))
    return out


# (ranges, last_unbounded, the first bad range)
FIXED_RANGES = [
    ([(b"a", b"b"), (b"b", b"c")], 0, -1),                                 # touching
    ([(b"a", b"b"), (b"b", b"c\x01"), (b"c\x00", b"d")], 0, 1),            # an overlap by one byte
    ([(b"a", b"b\x00"), (b"b", b"c")], 0, 0),
    ([(b"b", b"c"), (b"a", b"b")], 0, 0),                                  # descending
    ([(b"a", b"b"), (b"c", b"d"), (b"b", b"b")], 0, 1),                    # a descending lo, nothing overlaps
    ([(b"a", b"b"), (b"c", b"c"), (b"c", b"d")], 0, -1),                   # an empty range in the middle
    ([(b"a", b"b"), (b"d", b"c"), (b"d", b"e")], 0, -1),                   # lo > hi: empty, the next from lo on
    ([(b"a", b"b"), (b"d", b"c"), (b"c", b"e")], 0, 1),
    ([(b"", b""), (b"", b""), (b"", b"a")], 0, -1),                        # equal, empty bounds
    ([(b"a", b"b"), (b"b", b"")], 1, -1),                                  # the last one unbounded: its hi is not read
    ([(b"a", b"z"), (b"b", b"")], 1, 0),
    ([(b"a:", b"a;"), (b"a:b:", b"a:b;")], 0, 0),                          # nested prefixes, as ranges
    ([(b"k" * 40, b"k" * 40 + b"\x00"), (b"k" * 40 + b"\x00", b"l")], 0, -1),
]

# (prefixes, refused prefix or -1, last_unbounded, first bad range of the result)
FIXED_PREFIXES = [
    ([b"a:", b"b:", b"c:"], -1, 0, -1),
    ([b"a:", b"a:"], -1, 0, 0),                       # a repeated prefix
    ([b"a:", b"a:b:"], -1, 0, 0),                     # nested
    ([b"a", b"a:b"], -1, 0, 0),
    ([b"b:", b"a:"], -1, 0, 0),                       # descending
    ([b"a", b"\xff\xff"], -1, 1, -1),                 # all 0xFF: legal as the last one
    ([b"\xff\xff", b"a"], 0, None, None),             # and nowhere else
    ([b"a", b"\xff", b"\xff\xff"], 1, None, None),
    ([b"a", b""], -1, 1, 0),                          # the empty prefix last: unbounded, but below "a"
    ([b"", b"a"], 0, None, None),                     # a missing hi before the last range
    ([b""], -1, 1, -1),
    ([b"a\xff", b"b"], -1, 0, -1),                    # "a\xff"'s end is "b": touching
    ([b"a\xff", b"a\xff\xff"], -1, 0, 0),
]

# raw offsets that decrease: (kind, last_unbounded, n, bytes, offsets, answer)
FIXED_RAW = [
    ("o", 0, 2, b"abcd", [0, 1, 2, 1, 4], "r 1"),     # the second range's lo
    ("o", 0, 2, b"abcd", [0, 1, 2, 3, 2], "r 1"),     # the second range's hi
    ("o", 0, 2, b"abcd", [2, 1, 2, 3, 4], "r 0"),
    ("o", 0, 2, b"abcd", [0, 2, 1, 3, 4], "r 0"),
    ("o", 1, 1, b"ab", [0, 2, 1], "r 0"),             # (the last hi's bytes are ignored, not its offsets)
    ("o", 0, 2, b"abcd", [0, 1, 2, 3, 4], "r -1"),
    ("q", 0, 2, b"ab", [0, 2, 1], "p 1"),
    ("q", 0, 2, b"ab", [1, 0, 2], "p 0"),
]


def test_the_restated_rule_means_disjoint_and_ascending():
    """What the rule is for: in a list it accepts, every key lies in at most
    one range and the ranges' keys ascend with the ranges, so a table's cuts
    are disjoint runs of lines in order (brute force over every key of up to
    three letters)."""
    seen = set()
    for ranges, unb in random_lists(3, 3000):
        ok = first_bad(ranges) < 0
        seen.add(ok)
        if not ok:
            continue
        sets = [members(lo, None if unb and r == len(ranges) - 1 else hi) for r, (lo, hi) in enumerate(ranges)]
        flat = [k for s in sets for k in s]
        assert flat == sorted(set(flat)), (ranges, unb)
    assert seen == {True, False}


# ---- the host-only code under the sanitizers --------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rangelist") / "rangelist_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rangelist_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def hexs(b: bytes) -> str:
    return b.hex() if b else "-"


def run(driver, lines):
    r = subprocess.run([driver], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def range_line(ranges, unb):
    return "r %d %d %s" % (unb, len(ranges), " ".join(hexs(lo) + " " + hexs(hi) for lo, hi in ranges))


def test_range_lists_under_sanitizers(driver):
    cases = random_lists(17, 4000)
    got = run(driver, [range_line(r, u) for r, u in cases])
    seen = set()
    for (ranges, unb), ln in zip(cases, got):
        want = first_bad(ranges)
        assert ln == f"r {want}", (ranges, unb, ln)
        seen.add(want < 0)
    assert seen == {True, False}  # both outcomes of the ordering rule
    got = run(driver, [range_line(r, u) for r, u, _ in FIXED_RANGES])
    for (ranges, unb, want), ln in zip(FIXED_RANGES, got):
        assert first_bad(ranges) == want, ranges  # (the restatement agrees with the cases as written down)
        assert ln == f"r {want}", (ranges, unb, ln)


def expected_ranges(prefixes):
    """(refused, last_unbounded, [(lo, hi)]) of a prefix list, worked out here:
    a prefix's end is its last non-0xFF byte incremented."""
    ranges = []
    for i, p in enumerate(prefixes):
        q = p.rstrip(b"\xff")
        if not q:
            if i + 1 != len(prefixes):
                return i, None, None
            ranges.append((p, b""))
            return -1, 1, ranges
        ranges.append((p, q[:-1] + bytes([q[-1] + 1])))
    return -1, 0, ranges


def check_prefix_line(prefixes, ln):
    refused, unb, ranges = expected_ranges(prefixes)
    if refused >= 0:
        assert ln == f"p {refused}", (prefixes, ln)
        return None
    parts = [b for r in ranges for b in r]
    offs = np.concatenate([[0], np.cumsum([len(b) for b in parts])]).tolist()
    bad = first_bad(ranges)
    want = "p -1 %d %d %s %s" % (unb, bad, hexs(b"".join(parts)), " ".join(str(o) for o in offs))
    assert ln == want, (prefixes, ln, want)
    return bad < 0


def test_prefix_lists_under_sanitizers(driver):
    rng = np.random.default_rng(19)
    alpha = [0x61, 0x62, 0xFF]
    cases = []
    for _ in range(3000):
        ps = [bytes(alpha[i] for i in rng.integers(0, 3, int(rng.integers(0, 4)))) for _ in range(int(rng.integers(1, 6)))]
        if rng.integers(0, 3):
            ps.sort()
        cases.append(ps)
    got = run(driver, ["p %d %s" % (len(ps), " ".join(hexs(p) for p in ps)) for ps in cases])
    seen = {check_prefix_line(ps, ln) for ps, ln in zip(cases, got)}
    assert seen == {True, False, None}  # accepted, refused by the rule, refused for a missing end
    got = run(driver, ["p %d %s" % (len(ps), " ".join(hexs(p) for p in ps)) for ps, _, _, _ in FIXED_PREFIXES])
    for (ps, refused, unb, bad), ln in zip(FIXED_PREFIXES, got):
        assert expected_ranges(ps)[:2] == (refused, unb), ps
        assert check_prefix_line(ps, ln) == (None if refused >= 0 else bad < 0), ps
        if refused < 0:
            assert first_bad(expected_ranges(ps)[2]) == bad, ps


def test_decreasing_offsets_under_sanitizers(driver):
    lines = ["%s %s%d %s %s" % (k, "%d " % unb if k == "o" else "", n, hexs(b), " ".join(map(str, offs)))
             for k, unb, n, b, offs, _ in FIXED_RAW]
    for (_, _, _, _, offs, want), ln in zip(FIXED_RAW, run(driver, lines)):
        assert ln == want, (offs, ln)
