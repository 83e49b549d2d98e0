"""The selecting entries' surface (cb_scan_select, cb_rows_select, cb_row_select
and the cb_rows_* accessors; lsmt_amd.select_rows, ScanResult.select,
row_select, RowsResult), checked without a GPU: the header's declarations, the
ctypes prototypes, the integration document and the Python signatures; the
argument errors that are refused before any device is touched, each leaving
its result cleared; and the selection rule (lsmt_amd/csrc/rowselect.hpp over
rowjson.hpp's one grammar walker) under the address and undefined-behaviour
sanitizers, through a stand-alone driver (tests/cpp/rowselect_driver.cpp),
against the restatement in tests/rowselect_ref.py: the known answers of
tests/select_cases.py and a seeded run of mutated documents, on which the
driver, cb_row_select and the restatement must agree, with Python's json
module as a second witness for the restatement's objects.
"""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rowjson_ref
import rowselect_ref as ref
from select_cases import CASES, flags_of, json_text, meta_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL = 0, -1

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_scan_select": ["r", "skip", "sel", "mode", "out"],
    "cb_rows_select": ["keys", "key_off", "which", "vals", "val_off", "n", "skip", "sel", "mode", "device", "stream",
                       "out"],
    "cb_row_select": ["key", "key_len", "skip", "value", "value_len", "sel", "mode", "out", "cap", "len", "flags"],
    "cb_rows_info": ["rows", "count", "with_text", "bytes"],
    "cb_rows_text": ["rows", "text", "row_at", "row_len", "flags"],
    "cb_rows_destroy": ["rows"],
}
EMPTY = inspect.Parameter.empty
PYTHON = {
    "select_rows": (["keys", "which", "val_off", "vals", "columns", "key_columns", "casts", "skip", "meta", "device",
                     "stream"], [EMPTY, EMPTY, EMPTY, EMPTY, EMPTY, (), None, 0, False, None, None]),
    "row_select": (["key", "value", "columns", "key_columns", "casts", "skip", "meta"],
                   [EMPTY, EMPTY, EMPTY, (), None, 0, False]),
}


def csrc_code():
    """{file: its text without // comments} of every source in csrc/."""
    code = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp", ".cpp")):
            with open(os.path.join(CSRC, fn)) as fh:
                code[fn] = re.sub(r"//[^\n]*", "", fh.read())
    return code


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the selecting entries exist."""
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
    # the selection's struct, field by field, and its ctypes mirror
    m = re.search(r"typedef\s+struct\s+cb_select\s*\{(.*?)\}\s*cb_select\s*;", header, re.S)
    assert m, "no cb_select"
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == ["cols", "col_off", "part", "cast", "nc"]
    from lsmt_amd.rows import _CbSelect
    assert [n for n, _ in _CbSelect._fields_] == fields
    assert ctypes.sizeof(_CbSelect) == 40
    assert [getattr(_CbSelect, f).offset for f in fields] == [0, 8, 16, 24, 32]
    # the constants, in the header and in the package
    for name, value in [("CB_SELECT_JSON", 0), ("CB_SELECT_META", 1), ("CB_ROW_TEXT", 1), ("CB_ROW_DEAD", 2),
                        ("CB_ROW_ABSENT", 4), ("CB_ROW_BADJSON", 8), ("CB_ROW_EXTRA", 16)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(_lib, name[3:]) == value
    # the new section follows the WHERE one, cites the reference lines and names the rule's header
    assert raw_header.index("cb_row_matches(") < raw_header.index("cb_scan_select(") < raw_header.index("cb_rows_destroy(")
    section = raw_header[raw_header.index("SELECT a, b: rows projected"):raw_header.index("cb_rows_destroy(")]
    for cite in ("src/query.rs:365-432", "src/query.rs:402-405", "src/query.rs:641-662", "817-827",
                 "src/schema.rs:37-39", "src/query.rs:411-431", "src/query.rs:396-400", "src/cluster.rs:404-421"):
        assert cite in section, cite
    assert "rowselect.hpp" in section and "cb_scan_values" in section
    for name, (params, defaults) in PYTHON.items():
        assert name in lsmt_amd.__all__
        sig = inspect.signature(getattr(lsmt_amd, name))
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values()] == defaults, name
    assert "RowsResult" in lsmt_amd.__all__
    sig = inspect.signature(lsmt_amd.ScanResult.select)
    assert list(sig.parameters) == ["self", "columns", "key_columns", "casts", "skip", "meta"]
    assert [p.default for p in sig.parameters.values()] == [EMPTY, EMPTY, (), None, None, False]
    for method in ("text", "rows", "flags", "close"):
        assert callable(getattr(lsmt_amd.RowsResult, method))
    # the entries whose signatures other tests pin are as they were
    assert list(inspect.signature(lsmt_amd.ScanResult.match).parameters) == ["self", "where", "key_columns", "skip"]
    assert list(inspect.signature(lsmt_amd.row_matches).parameters) == ["key", "value", "where", "key_columns", "skip"]


def test_the_grammar_and_the_rule_have_one_home():
    """rowjson.hpp holds the grammar's one walker and the key-part locator,
    rowselect.hpp the selection over them; select.hip holds the two kernels
    and restates neither."""
    code = csrc_code()
    # the walker's escape table, its UTF-8 lead-byte bounds, its surrogate test and its whitespace: once in csrc/
    # (the three-byte and four-byte leads: the two-byte test is also the key check's of SsTable::load, sstable.hip)
    for token in ("c == 'b'", "c >= 0xE0 && c <= 0xEF", "c >= 0xF0 && c <= 0xF4", "cp >= 0xD800 && cp <= 0xDBFF",
                  "c == ' ' || c == '\\t'"):
        assert {fn: c.count(token) for fn, c in code.items() if token in c} == {"rowjson.hpp": 1}, token
    # the writer's escape table: once, in rowselect.hpp
    for token in ("b == 8 ? 'b'", "out.put('u')"):
        assert {fn: c.count(token) for fn, c in code.items() if token in c} == {"rowselect.hpp": 1}, token
    rowjson, rowselect, select = code["rowjson.hpp"], code["rowselect.hpp"], code["select.hip"]
    assert len(re.findall(r"\binline\s+bool\s+json_walk\s*\(", rowjson)) == 1
    for fn in ("key_part_count", "key_part_at"):
        assert re.search(r"\binline\s+uint64_t\s+%s\s*\(" % fn, rowjson), fn
        assert re.search(r"\b%s\s*\(" % fn, rowselect), fn
    # where_json_conditions keeps its signature and is a sink over the walker; where_key_conditions uses the locator
    m = re.search(r"template <class Src>\s*CB_ROW_HD inline uint32_t where_json_conditions\(const WherePred& w, "
                  r"uint32_t ask, Src& src\) \{(.*?)\n\}", rowjson, re.S)
    assert m and "json_walk(" in m.group(1) and "switch" not in m.group(1)
    m = re.search(r"inline uint32_t where_key_conditions\(.*?\n\}", rowjson, re.S)
    assert m and "key_part_at(" in m.group(0) and "key_part_count(" in m.group(0) and "'|'" not in m.group(0)
    assert rowjson.count("switch (st)") == 1
    # the selection reads strings through the walker only: no state machine, no key split of its own
    assert len(re.findall(r"\bjson_walk\s*\(", rowselect)) == 3  # the map, and a winning string as text or as an integer
    for text in (rowselect, select, code["select.hpp"], code["capi_select.cpp"]):
        assert "'|'" not in text and "switch" not in text
    assert "hip_runtime" not in rowselect and '#include "rowjson.hpp"' in rowselect
    with open(os.path.join(CSRC, "rowselect.hpp")) as fh:
        raw = fh.read()
    assert re.search(r"NOT\s+run\s+against\s+the\s+reference", raw)
    assert re.search(r"done\s+again\s+from\s+their\s+values\s+\(cb_scan_values\)", raw)  # what EXTRA asks of the caller
    for cite in ("src/query.rs:365-432", "src/query.rs:402-405", "src/query.rs:641-662", "src/schema.rs:37-39"):
        assert cite in raw, cite
    for kernel in ("k_select_size", "k_select_write"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, select), kernel
    assert re.findall(r'ProfScope ps\("(\w+)"', select) == ["k_select_size", "k_select_write"]
    assert "last_le(" in select  # the range lookup is k_scan_match's
    users = [fn for fn, c in code.items() if fn != "rowselect.hpp" and re.search(r"\b(select_size|select_write)\s*\(", c)]
    assert users == ["capi_select.cpp", "select.hip"]
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    for fn in ("select.hip", "capi_select.cpp", "select.hpp", "rowselect.hpp"):
        assert re.search(r"\b%s\b" % re.escape(fn), make), fn


# ---- argument errors --------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


class S(ctypes.Structure):
    _fields_ = [("cols", ctypes.c_char_p), ("col_off", ctypes.POINTER(ctypes.c_uint64)),
                ("part", ctypes.POINTER(ctypes.c_int32)), ("cast", ctypes.POINTER(ctypes.c_uint8)),
                ("nc", ctypes.c_uint32)]


def u64s(*xs):
    return (ctypes.c_uint64 * len(xs))(*xs)


def i32s(*xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def u8s(*xs):
    return (ctypes.c_uint8 * len(xs))(*xs)


def good_select():
    return S(b"cd", u64s(0, 1, 2), i32s(-1, 0), u8s(0, 1), 2)


def bad_selects():
    """(why, selection or None, mode, a part of the message)."""
    big = b"".join(b"%04d" % i for i in range(1025))  # 4100 bytes, ascending four by four
    yield "sel NULL", None, 0, "null selection"
    yield "null col_off", S(b"c", None, i32s(-1), None, 1), 0, "null column offsets"
    yield "null part", S(b"c", u64s(0, 1), None, None, 1), 0, "null column offsets"
    yield "null cols with bytes", S(None, u64s(0, 1), i32s(-1), None, 1), 0, "null names"
    yield "col_off decreases", S(b"cd", u64s(1, 0), i32s(-1), None, 1), 0, "offsets decrease"
    yield "col_off decreases later", S(b"cd", u64s(0, 2, 1), i32s(-1, -1), None, 2), 0, "offsets decrease"
    yield "17 columns", S(b"abcdefghijklmnopq", u64s(*range(18)), i32s(*[-1] * 17), None, 17), 0, "too many columns"
    yield "4097 bytes of names", S(big, u64s(0, 4097), i32s(-1), None, 1), 0, "too many bytes"
    yield "a huge total", S(big, u64s(0, 2 ** 64 - 1), i32s(-1), None, 1), 0, "too many bytes"
    yield "part -2", S(b"c", u64s(0, 1), i32s(-2), None, 1), 0, "key part index"
    yield "part 256", S(b"cd", u64s(0, 1, 2), i32s(255, 256), None, 2), 0, "key part index"
    yield "cast 2", S(b"cd", u64s(0, 1, 2), i32s(-1, -1), u8s(1, 2), 2), 0, "neither 0 nor 1"
    yield "names descend", S(b"dc", u64s(0, 1, 2), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "a name twice", S(b"cc", u64s(0, 1, 2), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "a name after its extension", S(b"abca", u64s(0, 3, 4), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "the empty name twice", S(b"", u64s(0, 0, 0), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "the empty name last", S(b"a", u64s(0, 1, 1), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "names compare as unsigned bytes", S(b"\xc3\xa9z", u64s(0, 2, 3), i32s(-1, -1), None, 2), 0, "strictly ascending"
    yield "mode 2", good_select(), 2, "neither 0 nor 1"
    yield "mode -1", good_select(), -1, "neither 0 nor 1"


def test_argument_errors_need_no_device():
    import lsmt_amd
    from lsmt_amd import _lib
    L = _lib.load()

    def ref_of(s):
        return ctypes.addressof(s) if s is not None else None

    def scan_select(s, mode, r=None):
        out = ctypes.c_void_p(0xDEAD)
        return L.cb_scan_select(r, None, ref_of(s), mode, ctypes.byref(out)), out.value

    def rows_select(s, mode, n=4, keys=b"kkkk", key_off=u64s(0, 1, 2, 3, 4), vals=b"vvvv", val_off=u64s(0, 1, 2, 3, 4)):
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_rows_select(keys, ctypes.cast(key_off, ctypes.c_void_p) if key_off is not None else None, None, vals,
                              ctypes.cast(val_off, ctypes.c_void_p) if val_off is not None else None, n, 0, ref_of(s),
                              mode, 0, None, ctypes.byref(out))
        return rc, out.value

    def row_select(s, mode, key=b"ns:k", value=b"12345678{}", cap=64, with_len=True):
        out, n, f = ctypes.create_string_buffer(b"\xAD" * 64, 64), ctypes.c_uint64(0xDEAD), ctypes.c_uint8(0xAD)
        rc = L.cb_row_select(key, len(key) if key else 4, 3, value, len(value) if value else 4, ref_of(s), mode,
                             out if cap else None, cap, ctypes.byref(n) if with_len else None, ctypes.byref(f))
        return rc, n.value, f.value, out.raw

    # every refusal of the selection and the mode, from all three entries, before the rows or the result are looked at
    for why, s, mode, msg in bad_selects():
        assert scan_select(s, mode) == (CB_EINVAL, None), why
        assert msg in last_error(L), (why, last_error(L))
        assert rows_select(s, mode) == (CB_EINVAL, None), why
        assert msg in last_error(L), (why, last_error(L))
        assert row_select(s, mode) == (CB_EINVAL, 0, 0, b"\xAD" * 64), why
        assert msg in last_error(L), (why, last_error(L))
    good = good_select()
    # out NULL
    assert L.cb_scan_select(None, None, ref_of(good), 0, None) == CB_EINVAL and last_error(L) == "null argument"
    assert L.cb_rows_select(None, None, None, None, None, 0, 0, ref_of(good), 0, 0, None, None) == CB_EINVAL
    assert last_error(L) == "null argument"
    assert row_select(good, 0, with_len=False)[0] == CB_EINVAL and last_error(L) == "null argument"
    # a good selection: the rows are next
    assert scan_select(good, 1) == (CB_EINVAL, None) and last_error(L) == "null scan"
    for kw in ({"keys": None}, {"key_off": None}, {"vals": None}, {"val_off": None}):
        assert rows_select(good, 0, **kw) == (CB_EINVAL, None), kw
        assert last_error(L) == "null rows with a non-zero count"
    assert row_select(good, 0, key=None)[:3] == (CB_EINVAL, 0, 0)
    assert row_select(good, 0, value=None)[:3] == (CB_EINVAL, 0, 0)
    # legal selections: no column (all pointers null), an empty name, cast NULL, names that share a prefix
    for s in (S(None, None, None, None, 0), S(None, u64s(0, 0), i32s(255), None, 1),
              S(b"aab", u64s(0, 0, 1, 3), i32s(-1, -1, 0), u8s(1, 0, 1), 3)):
        assert scan_select(s, 0) == (CB_EINVAL, None) and last_error(L) == "null scan"
    # no rows: a valid result without a device, [] for a client and no byte for a coordinator
    for mode, want in ((0, b"[]"), (1, b"")):
        h = ctypes.c_void_p()
        assert L.cb_rows_select(None, None, None, None, None, 0, 3, ref_of(good), mode, 0, None, ctypes.byref(h)) == CB_OK
        n, wt, nb = ctypes.c_uint64(9), ctypes.c_uint64(9), ctypes.c_uint64(9)
        assert L.cb_rows_info(h, ctypes.byref(n), ctypes.byref(wt), ctypes.byref(nb)) == CB_OK
        assert (n.value, wt.value, nb.value) == (0, 0, len(want))
        text = ctypes.create_string_buffer(b"\xAD" * 4, 4)
        assert L.cb_rows_text(h, text, None, None, None) == CB_OK and text.raw == want + b"\xAD" * (4 - len(want))
        assert L.cb_rows_destroy(h) == CB_OK
        r = lsmt_amd.select_rows([], None, np.zeros(1, np.uint64), np.zeros(1, np.uint8), ["c"], meta=bool(mode))
        assert (r.count, r.with_text, r.text(), r.rows(), r.flags().tolist()) == (0, 0, want, [], [])
        r.close()
    assert L.cb_rows_info(None, None, None, None) == CB_EINVAL and L.cb_rows_text(None, None, None, None, None) == CB_EINVAL
    assert L.cb_rows_destroy(None) == CB_OK
    # one row on the host: sizing, an exact capacity, one byte too few (nothing is written)
    s = S(b"a", u64s(0, 1), i32s(-1), None, 1)
    value = b"\0" * 7 + b"\x05" + b'{"a":"1"}'
    assert row_select(s, 0, value=value, cap=0)[:3] == (CB_OK, 9, 1)
    rc, n, f, raw = row_select(s, 0, value=value, cap=9)
    assert (rc, n, f) == (CB_OK, 9, 1) and raw == b'{"a":"1"}' + b"\xAD" * 55
    assert row_select(s, 0, value=value, cap=8) == (CB_OK, 9, 1, b"\xAD" * 64)
    assert row_select(s, 1, value=value)[3][:14] == b'k\t5\t{"a":"1"}\xAD'
    # the Python entries: columns in any order, the last cast of a repeated name
    assert lsmt_amd.row_select(b"ns:k", value, ["b", "a", "pk"], ("pk",), skip=3) == (b'{"a":"1","pk":"k"}', 1)
    value = b"\0" * 8 + b'{"a":"07"}'
    assert lsmt_amd.row_select(b"k", value, ["a", "a"], casts=[1, 0])[0] == b'{"a":"07"}'
    assert lsmt_amd.row_select(b"k", value, ["a", "a"], casts=[0, 1])[0] == b'{"a":"7"}'
    assert lsmt_amd.row_select(b"k", value, ["a"], casts={"a": True}, meta=True) == (b'k\t0\t{"a":"7"}', 1)
    assert lsmt_amd.row_select(b"k", b"\0" * 8, ["a"]) == (None, 2)
    assert lsmt_amd.row_select(b"k", b"\0" * 8, ["a"], meta=True) == (b"k\t0\t", 3)
    with pytest.raises(_lib.CassBloomError) as ei:
        lsmt_amd.row_select(b"k", value, ["c%02d" % i for i in range(17)])
    assert ei.value.code == CB_EINVAL and "too many columns" in str(ei.value)
    with pytest.raises(ValueError):
        lsmt_amd.row_select(b"k", value, ["a", "b"], casts=[1])


# ---- the restatement --------------------------------------------------------------------

def selection(c):
    return ref.normalize(c.columns, c.key_columns, c.casts)


def test_known_answers_restated():
    """tests/rowselect_ref.py gives the hand-worked text and flags of every
    case, in both modes."""
    assert len(CASES) > 80 and len(set(c.label for c in CASES)) == len(CASES)
    for c in CASES:
        for meta in (False, True):
            want = (meta_text(c) if meta else json_text(c), flags_of(c, meta))
            assert ref.row_text(c.key, c.value, selection(c), c.skip, meta, c.absent) == want, (c.label, meta)
    seen = 0
    for c in CASES:
        seen |= c.flags
    assert seen == 31  # every flag occurs
    assert ref.cast_int(b"-0") == b"0" and ref.cast_int(b"+") == b"+" and ref.cast_int(b"1" * 5000) == b"1" * 5000
    assert ref.escape(bytes(range(0x30))) == (rb'\u0000\u0001\u0002\u0003\u0004\u0005\u0006\u0007\b\t\n\u000b\f\r\u000e\u000f'
                                              rb'\u0010\u0011\u0012\u0013\u0014\u0015\u0016\u0017\u0018\u0019\u001a\u001b'
                                              rb'\u001c\u001d\u001e\u001f !\"#$%&' + b"'()*+,-./")
    assert ref.response([None, b"{}", None, b'{"a":"1"}', None]) == b'[{},{"a":"1"}]'
    assert ref.response([None, None]) == b"[]" and ref.response([]) == b"[]"
    assert ref.response([None, b"k\t1\t", None, b"l\t2\t{}"], meta=True) == b"k\t1\t\nl\t2\t{}"
    assert ref.response([None], meta=True) == b""


# ---- mutated documents ------------------------------------------------------------------

BASES = [b'{"a":"1","name":"Ada","n":"+007"}', b'{ "name" : "Ada" , "a" : "x\\ty" }', b'{"a":"\\u0076\\n","d":"\\ud83d\\ude00"}',
         b'{"a":"x","a":"v","n":"-0"}', b'{"d":"\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80","a":"v"}', b'{"n":"9223372036854775807"}',
         b'{"a\\nb":"\\"q\\"","a":"v","e":""}', b'{"a":"v","name":"\\\\","pk":"zz"}', b'{"n":"12","name":"\\u0000\\u001f/"}']
ALPHABET = b'{}",:\\u \t\n\r[]0123456789abcdefnulltrue\x00\x1f\x7f\x80\xbf\xc3\xa9\xe2\xed\xa0\xf0\xf4\xff' + b"+-vcdD8"
COLUMNS = (["a", "d", "n", "name", "pk"], ["a", "n"], ["name"], ["a", "a\nb", "d", "e", "n", "name", "pk"])


def mutated_docs(n=4000, seed=20261021):
    """Each a valid row after none, one or two of: a byte replaced or one of
    its bits flipped, a byte inserted, a byte deleted, the tail cut off."""
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        d = bytearray(BASES[i % len(BASES)])
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
        docs.append(bytes(d))
    return docs


def mutated_rows():
    """(key, value, selection, skip) per document: every base meets every
    selection; one value in seven is its own payload."""
    ts = (77).to_bytes(8, "big")
    return [(b"ns:k|x", (ts + d) if i % 7 else d, ref.normalize(COLUMNS[i // len(BASES) % len(COLUMNS)], ("pk", "ck"), {"n": 1}), 3)
            for i, d in enumerate(mutated_docs())]


def witness_object(p: bytes):
    """The whole map re-encoded by Python's json module, or None when the
    payload is no valid map of strings by its reading (test_where_cpu.py's
    witness_map states the known differences that are filtered here)."""
    try:
        text = p.decode("utf-8", "strict")
        pairs = json.loads(text, strict=True, object_pairs_hook=list)
    except (UnicodeDecodeError, ValueError, RecursionError):
        return None
    if not text.lstrip(" \t\n\r").startswith("{") or not isinstance(pairs, list):
        return None
    m = {}
    for pair in pairs:
        if not (isinstance(pair, tuple) and len(pair) == 2 and isinstance(pair[1], str)):
            return None
        if any(0xD800 <= ord(ch) <= 0xDFFF for ch in pair[0] + pair[1]):
            return None
        m[pair[0]] = pair[1]
    return json.dumps(m, ensure_ascii=False, separators=(",", ":"), sort_keys=True).encode()


def test_python_json_is_a_second_witness():
    """For every payload that is a valid map, the restatement's object over ALL
    of the map's names, no key column and no cast, equals json.dumps of the
    map with sorted keys: its escapes and its lower-case \\u00xx are
    serde_json's, and code-point order is UTF-8 byte order."""
    docs = [rowjson_ref.payload(c.value) for c in CASES] + mutated_docs()
    valid = 0
    for p in docs:
        want = witness_object(p)
        m = rowjson_ref.json_map(p)
        if want is None:
            if p:  # (an empty payload is a deleted row, not a document)
                assert m == {} and ref.row_map(b"k", p, [], 0)[1] & ref.BADJSON, p
            continue
        sel = ref.normalize(list(m))
        got, flags = ref.row_map(b"k", p, sel, 0)
        assert ref.encode(got) == want and flags == ref.TEXT, p
        valid += bool(m)
    assert valid > 1500


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rowselect") / "rowselect_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rowselect_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def hx(b) -> str:
    return bytes(b).hex() or "-"


def request(key, value, sel, skip=0, meta=False, absent=False) -> str:
    return " ".join(["S", str(int(meta)), str(skip), str(int(absent)), hx(key), hx(value), str(len(sel))] +
                    ["%s %d %d" % (hx(c), p, k) for c, p, k in sel])


def run_driver(driver, requests):
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(requests)
    return got


def answer(text, flags) -> str:
    return "%d %d %s" % (flags, len(text or b""), hx(text) if text is not None else "-")


def lib_row_select(key, value, sel, skip=0, meta=False):
    """cb_row_select through plain ctypes (not the package's wrapper)."""
    from lsmt_amd import _lib
    L = _lib.load()
    s = S(b"".join(c for c, _, _ in sel), u64s(*np.cumsum([0] + [len(c) for c, _, _ in sel]).tolist()),
          i32s(*[p for _, p, _ in sel]), u8s(*[k for _, _, k in sel]), len(sel))
    n, f = ctypes.c_uint64(), ctypes.c_uint8()
    assert L.cb_row_select(key, len(key), skip, value, len(value), ctypes.addressof(s), int(meta), None, 0,
                           ctypes.byref(n), ctypes.byref(f)) == 0
    if not f.value & ref.TEXT:
        return None, f.value
    out = ctypes.create_string_buffer(b"\xAD" * (n.value + 1), n.value + 1)
    assert L.cb_row_select(key, len(key), skip, value, len(value), ctypes.addressof(s), int(meta), out, n.value,
                           ctypes.byref(n), ctypes.byref(f)) == 0
    assert out.raw[n.value:] == b"\xAD"
    return out.raw[:n.value], f.value


def test_known_answers_under_sanitizers(driver):
    import lsmt_amd
    for meta in (False, True):
        got = run_driver(driver, [request(c.key, c.value, selection(c), c.skip, meta, c.absent) for c in CASES])
        for c, g in zip(CASES, got):
            want = (meta_text(c) if meta else json_text(c), flags_of(c, meta))
            assert g == answer(*want), f"{c.label}: driver {g!r} against {answer(*want)!r}"
            if c.absent:
                continue  # (the host entries take a row that is there)
            assert lib_row_select(c.key, c.value, selection(c), c.skip, meta) == want, c.label
            assert lsmt_amd.row_select(c.key, c.value, c.columns, c.key_columns, c.casts, c.skip, meta) == want, c.label


def test_driver_refuses_what_the_library_refuses(driver):
    k, v = b"k", b"\0" * 8 + b"{}"
    got = run_driver(driver, [request(k, v, [(b"c%02d" % i, -1, 0) for i in range(17)]),
                              request(k, v, [(b"c" * 4097, -1, 0)]), request(k, v, [(b"b", -1, 0), (b"a", -1, 0)]),
                              request(k, v, [(b"a", 256, 0)]), request(k, v, [(b"a", -1, 2)]),
                              request(k, b"\0" * 8 + b'{"%s":"1"}' % (b"c" * 4096), [(b"c" * 4096, -1, 0)])])
    assert got[:5] == ["E"] * 5 and got[5] == answer(b'{"%s":"1"}' % (b"c" * 4096), 1)


def test_mutated_documents_agree(driver):
    """About 4000 documents: the driver, cb_row_select and the restatement
    agree on every one's text and flags, in both modes."""
    rows = mutated_rows()
    # a property of the generator, asserted from the restatement alone: at least a quarter of the documents
    # are valid maps that yield a selected column (from the payload, not the key)
    yielding = 0
    for key, value, sel, skip in rows:
        m = rowjson_ref.json_map(rowjson_ref.payload(value))
        yielding += any(part < 0 and col in m for col, part, _ in sel)
    assert yielding * 4 >= len(rows), (yielding, len(rows))
    bad = sum(bool(ref.row_text(*r)[1] & ref.BADJSON) for r in rows)
    assert bad > 500, bad  # (and errors are well represented too)
    for meta in (False, True):
        want = [ref.row_text(key, value, sel, skip, meta) for key, value, sel, skip in rows]
        got = run_driver(driver, [request(key, value, sel, skip, meta) for key, value, sel, skip in rows])
        for r, g, w in zip(rows, got, want):
            assert g == answer(*w), (r[1], r[2], g, answer(*w))
            assert lib_row_select(r[0], r[1], r[2], r[3], meta) == w, (r[1], r[2])
    assert sum(bool(w[1] & ref.EXTRA) for w in want) > 300 and sum(w[1] == ref.TEXT for w in want) > 300
