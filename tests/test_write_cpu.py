"""The writing entries' surface (cb_rows_write, cb_row_write and the
cb_written_* accessors; lsmt_amd.write), checked without a GPU: the header's
declarations, the ctypes prototypes, the integration document and the Python
signatures; the argument errors that are refused before any device is touched,
each leaving its result cleared; and the rule (lsmt_amd/csrc/rowwrite.hpp over
rowjson.hpp's one grammar walker and rowselect.hpp's one escaper) under the
address and undefined-behaviour sanitizers, through a stand-alone driver
(tests/cpp/rowwrite_driver.cpp), against the restatement in
tests/rowwrite_ref.py: known answers from the reference's own tests, the old
documents of tests/select_cases.py as they are and mutated, on which the
driver, cb_row_write and the restatement must agree, with Python's json module
reading every payload back as a second witness.
"""
import base64
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rowjson_ref
import rowwrite_ref as ref
from select_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL = 0, -1

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_rows_write": ["w", "cells", "cell_off", "ts", "ts_all", "old_which", "old_vals", "old_val_off", "n", "device",
                      "stream", "out"],
    "cb_written_info": ["written", "count", "key_bytes", "val_bytes", "log_bytes", "flagged"],
    "cb_written_arrays": ["written", "keys", "key_off", "vals", "val_off", "log", "log_off", "flags"],
    "cb_written_copy": ["written", "keys", "key_off", "vals", "val_off", "log", "log_off", "flags"],
    "cb_written_destroy": ["written"],
    "cb_row_write": ["w", "cells", "cell_off", "ts", "old_value", "old_len", "has_old", "out", "cap", "key_len",
                     "val_len", "log_len", "flags"],
}
EMPTY = inspect.Parameter.empty


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the writing entries exist."""
    import lsmt_amd
    import lsmt_amd.write as wr
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
    # the statement's struct, field by field, and its ctypes mirror
    m = re.search(r"typedef\s+struct\s+cb_write\s*\{(.*?)\}\s*cb_write\s*;", header, re.S)
    assert m, "no cb_write"
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == ["ns", "ns_len", "nk", "cols", "col_off", "set", "nc", "op"]
    assert [n for n, _ in wr._CbWrite._fields_] == fields
    assert ctypes.sizeof(wr._CbWrite) == 56
    assert [getattr(wr._CbWrite, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 48, 52]
    for name, value in [("CB_WRITE_INSERT", 0), ("CB_WRITE_UPDATE", 1), ("CB_WRITE_DELETE", 2), ("CB_WRITTEN_HOST", 1),
                        ("CB_WRITTEN_BADOLD", 2), ("CB_WRITTEN_KEYCTL", 4)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(_lib, name[3:]) == value
    section = raw_header[raw_header.index("INSERT, UPDATE, DELETE: rows written"):raw_header.index("cb_row_write(")]
    for cite in ("src/query.rs:162-198", "716-731", "src/query.rs:201-237", "src/query.rs:240-261", "src/schema.rs:37-39",
                 "src/lib.rs:96-116", "154-157"):
        assert cite in section, cite
    assert "rowwrite.hpp" in section and "UTF-8 is not checked" in section
    # the Python surface: reached as lsmt_amd.write, nothing added to the package's own
    with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as fh:
        assert sorted(lsmt_amd.__all__) == sorted(json.load(fh))
    assert not hasattr(wr, "__all__")
    sig = lambda f: [(k, p.default) for k, p in inspect.signature(f).parameters.items()]  # noqa: E731
    assert sig(wr.write_rows) == [("ns", EMPTY), ("rows", EMPTY), ("nk", EMPTY), ("columns", ()), ("keep", ()),
                                  ("op", 0), ("ts", 0), ("old", None), ("device", None), ("stream", None)]
    assert sig(wr.row_write) == [("ns", EMPTY), ("row", EMPTY), ("nk", EMPTY), ("columns", ()), ("keep", ()), ("op", 0),
                                 ("ts", 0), ("old", None)]
    for method in ("keys", "values", "records", "log", "flags", "arrays", "to_table", "replay", "copy", "close"):
        assert callable(getattr(wr.Written, method)), method
    assert (wr.INSERT, wr.UPDATE, wr.DELETE) == (0, 1, 2)


def test_imports_alone():
    """lsmt_amd.write imports first in a fresh process."""
    r = subprocess.run([os.sys.executable, "-c", "import lsmt_amd.write as w; print(w.Written.__name__)"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "Written", r.stderr[-2000:]


def test_the_rule_has_one_home():
    """rowwrite.hpp holds the rule over rowjson.hpp's walker and rowselect.hpp's
    escaper and first-pass sink; write.hip holds the two kernels and restates
    none of it; the Makefile builds the new sources."""
    code = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp", ".cpp")):
            with open(os.path.join(CSRC, fn)) as fh:
                code[fn] = re.sub(r"//[^\n]*", "", fh.read())
    rule, hip = code["rowwrite.hpp"], code["write.hip"]
    assert "hip_runtime" not in rule and '#include "rowselect.hpp"' in rule
    assert "SelectSizeSink<" in rule and "esc_put(" in rule and "kKeyPartSep" in rule
    assert len(re.findall(r"\bjson_walk\s*\(", rule)) == 2  # the old map, and a kept string
    for text in (rule, hip, code["write.hpp"], code["capi_write.cpp"]):
        assert "switch" not in text
    users = [fn for fn, c in code.items() if fn != "rowwrite.hpp" and re.search(r"\b(write_size|write_emit)\s*\(", c)]
    assert users == ["capi_write.cpp", "write.hip"]
    users = [fn for fn, c in code.items() if re.search(r"\bb64_char\s*\(", c)]
    assert users == ["rowts.hpp", "rowwrite.hpp"]
    for kernel in ("k_write_size", "k_write_emit"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, hip), kernel
    assert re.findall(r'ProfScope ps\("(\w+)"', hip) == ["k_write_size", "k_write_emit"]
    with open(os.path.join(CSRC, "rowwrite.hpp")) as fh:
        raw = fh.read()
    assert re.search(r"NOT\s+run\s+against\s+the\s+reference", raw) and re.search(r"UTF-8\s+is\s+NOT\s+checked", raw)
    for cite in ("src/query.rs:162-198", "src/query.rs:201-237", "src/query.rs:240-261", "src/schema.rs:37-39",
                 "src/lib.rs:96-116"):
        assert cite in raw, cite
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    for fn in ("write.hip", "capi_write.cpp", "write.hpp", "rowwrite.hpp"):
        assert re.search(r"\b%s\b" % re.escape(fn), make), fn


# ---- argument errors --------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


class W(ctypes.Structure):
    _fields_ = [("ns", ctypes.c_char_p), ("ns_len", ctypes.c_uint64), ("nk", ctypes.c_uint32),
                ("cols", ctypes.c_char_p), ("col_off", ctypes.POINTER(ctypes.c_uint64)),
                ("set", ctypes.POINTER(ctypes.c_uint8)), ("nc", ctypes.c_uint32), ("op", ctypes.c_int)]


def u64s(*xs):
    return (ctypes.c_uint64 * len(xs))(*xs)


def u8s(*xs):
    return (ctypes.c_uint8 * len(xs))(*xs)


def good_write(op=0):
    if op == 2:
        return W(b"ns", 2, 1, None, None, None, 0, 2)
    return W(b"ns", 2, 1, b"cd", u64s(0, 1, 2), u8s(1, 1), 2, op)


def bad_writes():
    """(why, statement or None, a part of the message)."""
    big = b"".join(b"%04d" % i for i in range(1025))
    yield "w NULL", None, "null statement"
    yield "op 3", W(b"ns", 2, 1, None, None, None, 0, 3), "none of insert"
    yield "op -1", W(b"ns", 2, 1, None, None, None, 0, -1), "none of insert"
    yield "17 key columns", W(b"ns", 2, 17, None, None, None, 0, 0), "too many key columns"
    yield "null ns with a length", W(None, 2, 1, None, None, None, 0, 0), "null namespace"
    yield "null col_off", W(b"", 0, 1, b"c", None, u8s(1), 1, 0), "null column offsets"
    yield "null cols with bytes", W(b"", 0, 1, None, u64s(0, 1), u8s(1), 1, 0), "null names"
    yield "col_off decreases", W(b"", 0, 1, b"cd", u64s(1, 0), u8s(1), 1, 0), "offsets decrease"
    yield "17 columns", W(b"", 0, 1, b"abcdefghijklmnopq", u64s(*range(18)), u8s(*[1] * 17), 17, 0), "too many columns"
    yield "4097 bytes of names", W(b"", 0, 1, big, u64s(0, 4097), u8s(1), 1, 0), "too many bytes"
    yield "names descend", W(b"", 0, 1, b"dc", u64s(0, 1, 2), u8s(1, 1), 2, 0), "strictly ascending"
    yield "a name twice", W(b"", 0, 1, b"cc", u64s(0, 1, 2), u8s(1, 1), 2, 1), "strictly ascending"
    yield "null set", W(b"", 0, 1, b"c", u64s(0, 1), None, 1, 0), "null set flags"
    yield "set 2", W(b"", 0, 1, b"cd", u64s(0, 1, 2), u8s(1, 2), 2, 1), "neither 0 nor 1"
    yield "an insert that keeps", W(b"", 0, 1, b"cd", u64s(0, 1, 2), u8s(1, 0), 2, 0), "insert that keeps"
    yield "a delete with columns", W(b"", 0, 1, b"c", u64s(0, 1), u8s(1), 1, 2), "delete with payload"


def test_argument_errors_need_no_device():
    import lsmt_amd.write as wr
    from lsmt_amd import _lib
    L = _lib.load()

    def ref_of(s):
        return ctypes.addressof(s) if s is not None else None

    def rows_write(s, n=2, cells=b"kxykxy", cell_off=u64s(0, 1, 2, 3, 4, 5, 6), old=(None, None, None)):
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_rows_write(ref_of(s), cells, ctypes.cast(cell_off, ctypes.c_void_p) if cell_off is not None else None,
                             None, 7, old[0], old[1], old[2], n, 0, None, ctypes.byref(out))
        return rc, out.value

    def row_write(s, cells=b"kxy", cell_off=u64s(0, 1, 2, 3), old=None, cap=256, with_len=True):
        out = ctypes.create_string_buffer(b"\xAD" * 256, 256)
        kl, vl, rl, f = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD), ctypes.c_uint8(0xAD)
        rc = L.cb_row_write(ref_of(s), cells, ctypes.cast(cell_off, ctypes.c_void_p) if cell_off is not None else None,
                            7, old, len(old or b""), int(old is not None), out if cap else None, cap,
                            ctypes.byref(kl) if with_len else None, ctypes.byref(vl), ctypes.byref(rl), ctypes.byref(f))
        return rc, (kl.value, vl.value, rl.value), f.value, out.raw

    # every refusal of the statement, from both entries, before the cells or the result are looked at
    for why, s, msg in bad_writes():
        assert rows_write(s) == (CB_EINVAL, None), why
        assert msg in last_error(L), (why, last_error(L))
        assert row_write(s) == (CB_EINVAL, (0, 0, 0), 0, b"\xAD" * 256), why
        assert msg in last_error(L), (why, last_error(L))
    good = good_write()
    assert L.cb_rows_write(ref_of(good), None, None, None, 0, None, None, None, 0, 0, None, None) == CB_EINVAL
    assert last_error(L) == "null argument"
    assert row_write(good, with_len=False)[0] == CB_EINVAL and last_error(L) == "null argument"
    # old rows with INSERT or DELETE, or not all three arrays
    three = (ctypes.cast(u64s(0), ctypes.c_void_p), b"x", ctypes.cast(u64s(0, 0, 0), ctypes.c_void_p))
    for op in (0, 2):
        cells, off = (b"kk", u64s(0, 1, 2)) if op == 2 else (b"kxykxy", u64s(0, 1, 2, 3, 4, 5, 6))
        assert rows_write(good_write(op), cells=cells, cell_off=off, old=three) == (CB_EINVAL, None)
        assert "old rows with an insert or a delete" in last_error(L)
        assert row_write(good_write(op), old=b"")[0] == CB_EINVAL and "old rows with an insert" in last_error(L)
    assert rows_write(good_write(1), old=(three[0], None, three[2])) == (CB_EINVAL, None)
    assert "without all three" in last_error(L)
    # the cells: null with rows of at least one cell, host offsets that decrease
    for kw in ({"cells": None}, {"cell_off": None}):
        assert rows_write(good, **kw) == (CB_EINVAL, None) and last_error(L) == "null cells with a non-zero count"
        assert row_write(good, **kw)[0] == CB_EINVAL and last_error(L) == "null cells with a non-zero count"
    assert rows_write(good, cell_off=u64s(0, 1, 2, 3, 2, 5, 6)) == (CB_EINVAL, None)
    assert last_error(L) == "cell offsets decrease"
    assert row_write(good, cell_off=u64s(0, 2, 1, 3))[0] == CB_EINVAL and last_error(L) == "cell offsets decrease"
    # no rows: a valid result without a device
    for s in (good, good_write(1), good_write(2), W(None, 0, 0, None, None, None, 0, 0)):
        h = ctypes.c_void_p()
        assert L.cb_rows_write(ref_of(s), None, None, None, 0, None, None, None, 0, 0, None, ctypes.byref(h)) == CB_OK
        v = [ctypes.c_uint64(9) for _ in range(5)]
        assert L.cb_written_info(h, *[ctypes.byref(x) for x in v]) == CB_OK and [x.value for x in v] == [0] * 5
        p = [ctypes.c_void_p(0xDEAD) for _ in range(7)]
        assert L.cb_written_arrays(h, *[ctypes.byref(x) for x in p]) == CB_OK and [x.value for x in p] == [None] * 7
        off = u64s(9)
        assert L.cb_written_copy(h, None, ctypes.cast(off, ctypes.c_void_p), None, None, None, None, None) == CB_OK
        assert off[0] == 0
        assert L.cb_written_destroy(h) == CB_OK
    r = wr.write_rows("ns", [], 1, ["c"])
    assert (r.count, r.flagged, r.keys(), r.values(), r.records(), r.log(), r.flags().tolist()) == (0, 0, [], [], [], b"", [])
    assert set(r.arrays().values()) == {0}
    r.close()
    assert L.cb_written_info(None, None, None, None, None, None) == CB_EINVAL
    assert L.cb_written_arrays(None, None, None, None, None, None, None, None) == CB_EINVAL
    assert L.cb_written_copy(None, None, None, None, None, None, None, None) == CB_EINVAL
    assert L.cb_written_destroy(None) == CB_OK
    # one row on the host: sizing with out NULL, an exact capacity, one byte too few (nothing is written)
    want = ref.write_row(b"ns", [b"k"], [b"c", b"d"], {b"c": b"x", b"d": b"y"}, ref.INSERT, 7)
    total = sum(len(x) for x in want[:3])
    assert row_write(good, cap=0)[:3] == (CB_OK, tuple(len(x) for x in want[:3]), 0)
    rc, lens, f, raw = row_write(good, cap=total)
    assert rc == CB_OK and raw == b"".join(want[:3]) + b"\xAD" * (256 - total)
    assert row_write(good, cap=total - 1) == (CB_OK, lens, 0, b"\xAD" * 256)
    # the Python entries: columns in any order, a row of the wrong width
    assert wr.row_write("ns", ["k", "y", "x"], 1, ["d", "c"], ts=7) == want
    with pytest.raises(ValueError):
        wr.row_write("ns", ["k", "y"], 1, ["d", "c"])
    with pytest.raises(ValueError):
        wr.row_write("ns", ["k", "y", "x"], 1, ["c", "c"])
    with pytest.raises(_lib.CassBloomError) as ei:
        wr.row_write("ns", ["k"] * 17, 17)
    assert ei.value.code == CB_EINVAL and "too many key columns" in str(ei.value)


# ---- known answers ----------------------------------------------------------------------

def test_known_answers():
    """The reference's own tests (tests/query_advanced_test.rs): a table kv
    with the key column id and the column val. INSERT ('a', '1'), then UPDATE
    kv SET val = '2' WHERE id = 'a' leaves the row {"val":"2"}; DELETE leaves a
    tombstone, the timestamp alone. And what the statement's shape decides."""
    import lsmt_amd.write as wr
    ts = 0x0102030405060708
    stamp = bytes(range(1, 9))
    key, value, rec, f = wr.row_write("kv", ["a", "1"], 1, ["val"], op="insert", ts=ts)
    assert (key, value, f) == (b"kv:a", stamp + b'{"val":"1"}', 0)
    assert rec == b"kv:a\t" + base64.b64encode(value) + b"\n"
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], op="update", ts=ts, old=value)[:2] == (b"kv:a", stamp + b'{"val":"2"}')
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], op="update", ts=ts)[:2] == (b"kv:a", stamp + b'{"val":"2"}')
    key, value, rec, f = wr.row_write("kv", ["a"], 1, op="delete", ts=ts)
    assert (key, value, rec, f) == (b"kv:a", stamp, b"kv:a\tAQIDBAUGBwg=\n", 0)
    # an UPDATE keeps what it does not set, and leaves out what the old row does not have
    old = b"\0" * 8 + b'{ "val" : "1" , "w" : "x\\ty" }'
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], ["w", "z"], "update", 1, old)[1] == b"\0" * 7 + b'\x01{"val":"2","w":"x\\ty"}'
    # a name outside the statement's columns: the caller's row, the key alone
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], [], "update", 1, old) == (b"kv:a", None, None, wr.WRITTEN_HOST)
    # an old value that is no map counts as empty and says so; a tombstone does not
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], ["w"], "update", 1, b"\0" * 8 + b"{")[1::2] == (b"\0" * 7 + b'\x01{"val":"2"}', 2)
    assert wr.row_write("kv", ["a", "2"], 1, ["val"], ["w"], "update", 1, b"\0" * 8)[1::2] == (b"\0" * 7 + b'\x01{"val":"2"}', 0)
    # no key column, no namespace, no payload column: `:` and {} (a live row)
    assert wr.row_write("", [], 0, ts=0)[:2] == (b":", b"\0" * 8 + b"{}")
    assert wr.row_write("", [], 0, op="delete", ts=0)[:2] == (b":", b"\0" * 8)
    # key cells are joined in the caller's order; a tab in one is flagged, and the row is written
    key, value, rec, f = wr.row_write("n", ["b", "x", "a\tc"], 2, ["v"], ts=0)
    assert (key, f) == (b"n:b|x", 0) and value == b"\0" * 8 + b'{"v":"a\\tc"}'
    key, value, rec, f = wr.row_write("n", ["b\t", "x"], 2, ts=0)
    assert (key, f) == (b"n:b\t|x", wr.WRITTEN_KEYCTL) and rec.startswith(b"n:b\t|x\t")
    assert wr.row_write("n\n", [], 0)[3] == wr.WRITTEN_KEYCTL


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rowwrite") / "rowwrite_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rowwrite_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def hx(b) -> str:
    return bytes(b).hex() or "-"


def request(ns, row, nk, columns, keep, op, ts, old) -> str:
    """The driver's line for a row in the caller's order (columns sorted here)."""
    names = sorted(list(columns) + list(keep))
    given = dict(zip(columns, row[nk:]))
    cells = list(row[:nk]) + [given[c] for c in names if c in given]
    return " ".join(["W", str(op), str(nk), str(ts), str(int(old is not None)), hx(ns), hx(old or b""), str(len(names))] +
                    ["%s %d" % (hx(c), c in given) for c in names] + [str(len(cells))] + [hx(c) for c in cells])


def run_driver(driver, requests):
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(requests)
    return got


def answer(key, value, rec, flags) -> str:
    return "%d %s %s %s" % (flags, hx(key), hx(value or b""), hx(rec or b""))


ALPHABET = b'{}",:\\u \t\n\r[]0123456789abcdefnulltrue\x00\x1f\x7f\x80\xbf\xc3\xa9\xe2\xed\xa0\xf0\xf4\xff' + b"+-vcdD8"
STATEMENTS = (  # (set columns in the caller's order, kept columns)
    ([b"a"], [b"b", b"d", b"n", b"name"]), ([b"n", b"a"], []), ([], [b"a", b"a\nb", b"d", b"e", b"n", b"name", b"pk"]),
    ([b"zz", b""], [b"a", b"b", b"c", b"ck", b"d", b"e", b"n", b"name", b"pk", b"a\nb", b'a"\n\x01', b"ab", b"x", b"y"]),
)


def old_values(n=3000, seed=20261021):
    """The values of tests/select_cases.py as they are, then each after none, one
    or two of: a byte replaced or one of its bits flipped, a byte inserted, a
    byte deleted, the tail cut off."""
    rng = np.random.default_rng(seed)
    base = [c.value for c in CASES]
    out = list(base)
    for i in range(n):
        d = bytearray(base[i % len(base)])
        for _ in range(int(rng.integers(0, 3))):
            kind, at = int(rng.integers(0, 7)), int(rng.integers(0, len(d) + 1))
            b = ALPHABET[int(rng.integers(0, len(ALPHABET)))] if rng.random() < 0.7 else int(rng.integers(0, 256))
            if kind in (0, 1, 2) and at < len(d):
                d[at] = b if rng.random() < 0.5 else d[at] ^ (1 << int(rng.integers(0, 8)))
            elif kind in (3, 4):
                d.insert(at, b)
            elif kind == 5 and at < len(d):
                del d[at]
            elif kind == 6:
                del d[at:]
        out.append(bytes(d))
    return out


def update_rows():
    """(ns, row, nk, columns, keep, op, ts, old) per old value: every value
    meets every statement; the cells carry what the escaper must handle."""
    cells = [b"", b"v", b'q"\\\n\x00\x1f\x7f', "é€😀".encode(), b"\xff\xc3", bytes(range(0x80))]
    rows = []
    for i, old in enumerate(old_values()):
        columns, keep = STATEMENTS[i % len(STATEMENTS)]
        row = [b"k%d" % i, cells[i % len(cells)]] + [cells[(i + j) % len(cells)] for j in range(len(columns))]
        rows.append((b"ns", row, 2, columns, keep, ref.UPDATE, (i * 0x9E3779B97F4A7C15) % 2 ** 64, old))
    return rows


def lib_row_write(ns, row, nk, columns, keep, op, ts, old):
    """cb_row_write through plain ctypes (not the package's wrapper)."""
    from lsmt_amd import _lib
    L = _lib.load()
    names = sorted(list(columns) + list(keep))
    given = dict(zip(columns, row[nk:]))
    cells = list(row[:nk]) + [given[c] for c in names if c in given]
    s = W(ns, len(ns), nk, b"".join(names), u64s(*np.cumsum([0] + [len(c) for c in names]).tolist()),
          u8s(*[c in given for c in names]) if names else None, len(names), op)
    off = u64s(*np.cumsum([0] + [len(c) for c in cells]).tolist())
    data = b"".join(cells) or b"\0"
    kl, vl, rl, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint8()
    args = (ctypes.addressof(s), data, ctypes.cast(off, ctypes.c_void_p), ts, old, len(old or b""), int(old is not None))
    tail = (ctypes.byref(kl), ctypes.byref(vl), ctypes.byref(rl), ctypes.byref(f))
    assert L.cb_row_write(*args, None, 0, *tail) == 0
    total = kl.value + vl.value + rl.value
    out = ctypes.create_string_buffer(b"\xAD" * (total + 1), total + 1)
    assert L.cb_row_write(*args, out, total, *tail) == 0
    assert out.raw[total:] == b"\xAD"
    k, v = kl.value, vl.value
    if f.value & ref.HOST:
        assert (v, rl.value) == (0, 0)
        return out.raw[:k], None, None, f.value
    return out.raw[:k], out.raw[k:k + v], out.raw[k + v:total], f.value


def ref_row(ns, row, nk, columns, keep, op, ts, old):
    return ref.write_row(ns, list(row[:nk]), list(columns) + list(keep), dict(zip(columns, row[nk:])), op, ts, old)


def test_old_documents_agree(driver):
    """About 3000 old values under four statements: the driver, cb_row_write
    and the restatement agree on every row's key, value, record and flags;
    every payload written reads back through Python's json module as the dict
    model's map, and every record through base64 as its value; the
    restatement's reading of the old map is tests/rowjson_ref.py's too."""
    rows = update_rows()
    want = [ref_row(*r) for r in rows]
    got = run_driver(driver, [request(*r) for r in rows])
    for r, g, w in zip(rows, got, want):
        assert g == answer(*w), (r, g, answer(*w))
        assert lib_row_write(*r) == w, r
        old_payload = rowjson_ref.payload(r[7])
        assert (ref.decode_row(old_payload) or {}) == (rowjson_ref.json_map(old_payload) if old_payload else {}), r[7]
        key, value, rec, flags = w
        if value is None:
            continue
        payload = value[8:]
        m = ref.decode_row(old_payload) or {} if old_payload else {}
        m.update(dict(zip(r[3], r[1][r[2]:])))
        try:  # (a cell that is not UTF-8 gives a payload no reader accepts: the header says so)
            model = {k.decode(): v.decode() for k, v in m.items()}
        except UnicodeDecodeError:
            model = None
        if model is not None:
            assert json.loads(payload.decode(), strict=True) == model, payload
        assert rec == key + b"\t" + base64.b64encode(value) + b"\n" and base64.b64decode(rec[len(key) + 1:-1]) == value
    flags = [w[3] for w in want]
    counts = (sum(f == ref.HOST for f in flags), sum(f == ref.BADOLD for f in flags), sum(f == 0 for f in flags))
    assert counts[0] > 100 and counts[1] > 300 and counts[2] > 300, counts  # (a property of the generator)
    kept = sum(1 for r, w in zip(rows, want) if w[1] is not None and r[4] and
               any(k in (ref.decode_row(rowjson_ref.payload(r[7])) or {}) for k in r[4]))
    assert kept > 300, kept  # (rows that carry an old value over)


def test_statement_shapes_under_sanitizers(driver):
    """INSERT and DELETE, every count of key columns, empty cells and names, a
    value of every length mod 3, a 70 KB cell; and what the driver refuses."""
    rows = []
    for nk in (0, 1, 2, 16):
        keyc = [b"p%d" % j if j % 3 else b"" for j in range(nk)]
        rows.append((b"ns", keyc, nk, [], [], ref.DELETE, 2 ** 64 - 1, None))
        rows.append((b"", keyc + [b""], nk, [b""], [], ref.INSERT, 0, None))
        for pad in range(4):
            rows.append((b"n|s", keyc + [b"x" * pad, bytes(range(0x80)) + "é€😀".encode()], nk, [b"b", b"a"], [], ref.INSERT, pad, None))
    rows.append((b"big", [b"k", b"\x01" * 70000], 1, [b"c"], [], ref.INSERT, 1, None))
    rows.append((b"big", [b"k", b"z"], 1, [b"c"], [b"d"], ref.UPDATE, 1, b"\0" * 8 + b'{"d":"' + b"\\n" * 35000 + b'"}'))
    got = run_driver(driver, [request(*r) for r in rows])
    for r, g in zip(rows, got):
        w = ref_row(*r)
        assert g == answer(*w), (r[:7], g[:200])
        assert lib_row_write(*r) == w, r[:7]
    refused = ["W 3 1 0 0 - - 0 1 6b", "W 0 17 0 0 - - 0 0", "W 0 0 0 0 - - 2 62 1 61 1 2 - -", "W 0 0 0 0 - - 1 61 0 0",
               "W 2 0 0 0 - - 1 61 1 1 -", "W 0 1 0 1 - - 0 1 6b", "W 0 1 0 0 - - 0 2 6b 6b"]
    assert run_driver(driver, refused) == ["E"] * len(refused)
