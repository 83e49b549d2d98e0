"""The WHERE entries' surface (cb_tables_count_where, cb_scan_match,
cb_row_matches; lsmt_amd.count_where, ScanResult.match, row_matches), checked
without a GPU: the header's declarations, the ctypes prototypes, the
integration document and the Python signatures; the argument errors that are
refused before any device is touched, each leaving its outputs cleared; and
the row rule (lsmt_amd/csrc/rowjson.hpp) under the address and
undefined-behaviour sanitizers, through a stand-alone driver
(tests/cpp/rowjson_driver.cpp) that takes it through both of its readers
(decoded bytes, and base64 text decoded on the fly), against the restatement in
tests/rowjson_ref.py: the known answers of tests/where_cases.py and a seeded
run of mutated documents, on which the driver, cb_row_matches and the
restatement must agree, and Python's json module as a second witness for the
restatement's map.
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
from where_cases import CASES, TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL = 0, -1

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_tables_count_where": ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "skip", "w", "lww",
                              "stream", "live", "matched"],
    "cb_scan_match": ["r", "skip", "w", "flags"],
    "cb_row_matches": ["key", "key_len", "skip", "value", "value_len", "w", "out"],
}
EMPTY = inspect.Parameter.empty
# name -> (parameters, their defaults)
PYTHON = {
    "count_where": (["tables", "where", "key_columns", "ranges", "prefixes", "skip", "lww", "stream"],
                    [EMPTY, EMPTY, (), None, None, None, False, None]),
    "row_matches": (["key", "value", "where", "key_columns", "skip"], [EMPTY, EMPTY, EMPTY, (), 0]),
}


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the WHERE entries exist."""
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
    # the predicate's struct, field by field, and its ctypes mirror
    m = re.search(r"typedef\s+struct\s+cb_where\s*\{(.*?)\}\s*cb_where\s*;", header, re.S)
    assert m, "no cb_where"
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == ["cols", "col_off", "vals", "val_off", "part", "nc"]
    from lsmt_amd.rows import _CbWhere
    assert [n for n, _ in _CbWhere._fields_] == fields
    assert ctypes.sizeof(_CbWhere) == 48 and _CbWhere.nc.offset == 40
    # the new section follows the last-write-wins one and cites the reference lines the rule comes from
    assert raw_header.index("cb_scan_ts(") < raw_header.index("cb_tables_count_where(")
    section = raw_header[raw_header.index("rows WHERE column = value"):raw_header.index("cb_row_matches(")]
    for cite in ("src/query.rs:309-362", "src/query.rs:21-27", "src/schema.rs:42-44"):
        assert cite in section, cite
    assert "rowjson.hpp" in section
    for name, (params, defaults) in PYTHON.items():
        assert name in lsmt_amd.__all__
        sig = inspect.signature(getattr(lsmt_amd, name))
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values()] == defaults, name
    sig = inspect.signature(lsmt_amd.ScanResult.match)
    assert list(sig.parameters) == ["self", "where", "key_columns", "skip"]
    assert [p.default for p in sig.parameters.values()] == [EMPTY, EMPTY, (), None]
    # the entries whose signatures other tests pin are as they were
    assert list(inspect.signature(lsmt_amd.count).parameters) == ["tables", "ranges", "prefixes", "stream"]
    assert list(inspect.signature(lsmt_amd.count_lww).parameters) == ["tables", "ranges", "prefixes", "stream"]
    assert list(inspect.signature(lsmt_amd.scan_live).parameters) == ["tables", "ranges", "prefixes", "limit", "stream"]
    assert list(inspect.signature(lsmt_amd.scan_lww).parameters) == ["tables", "ranges", "prefixes", "limit",
                                                                     "drop_dead", "stream"]
    assert list(inspect.signature(lsmt_amd.ScanResult.ts).parameters) == ["self"]
    for name, names in [("cb_tables_count", ["tables", "nt", "bounds", "bound_off", "nr", "last_unbounded", "stream",
                                             "entries", "live"]),
                        ("cb_scan_ts", ["r", "ts"])]:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == names


def test_the_rule_has_one_home():
    """rowjson.hpp defines the rule; the sources that apply it include it, and
    no other source parses a payload or splits a key."""
    with open(os.path.join(CSRC, "rowjson.hpp")) as fh:
        text = fh.read()
    for fn in ("row_matches", "where_json_conditions", "where_key_conditions", "where_check", "where_pack"):
        assert re.search(r"\binline\s+[\w:\s\*]+\b%s\s*\(" % fn, text), fn
    for cite in ("src/query.rs:309-362", "src/query.rs:21-27", "src/schema.rs:42-44", "src/schema.rs:27-33"):
        assert cite in text, cite
    assert re.search(r"NOT\s+run\s+against\s+the\s+reference", text)
    assert "hip_runtime" not in text  # no HIP dependency: the driver builds it with a host compiler
    users = []
    for fn in sorted(os.listdir(CSRC)):
        if fn == "rowjson.hpp" or not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as fh:
            src = fh.read()
        code = re.sub(r"//[^\n]*", "", src)
        if re.search(r"\b(row_matches|where_check|where_pack)\s*\(", code):
            users.append(fn)
        assert not re.search(r"\b(where_json_conditions|where_key_conditions)\b", code), fn
        assert "'|'" not in code, fn  # no second split of a key into parts
    assert users == ["capi_scan.cpp", "scan.hip"]
    with open(os.path.join(CSRC, "scan.hip")) as fh:
        scan = fh.read()
    for kernel in ("k_scan_count_where", "k_scan_match", "k_scan_count"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, scan), kernel


def test_the_merge_kernels_repeated_steps_have_one_home():
    """The steps that k_scan_count / k_scan_count_where, k_scan_emit /
    k_compact_format and k_compact_select / k_compact_lww_tiles share are each
    written once in csrc/, and both kernels of each pair go through that one body."""
    code = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp", ".cpp")):
            with open(os.path.join(CSRC, fn)) as fh:
                code[fn] = re.sub(r"//[^\n]*", "", fh.read())
    homes = {"s_off[i + 1]) ++i": "compact.hpp",       # the dword-assembly walk of the tile copier
             "s_rid[mid] < rid": "scan.hip",            # the search for a run's first lane
             "tkeys[blockIdx.x] = tk": "compact.hip"}   # the three-sum tile write
    for token, home in homes.items():
        assert {fn: c.count(token) for fn, c in code.items() if token in c} == {home: 1}, token
    scan, compact = code["scan.hip"], code["compact.hip"]
    assert [len(re.findall(r"\bcopy_tile_bytes\s*\(", c)) for c in (scan, compact, code["compact.hpp"])] == [1, 1, 1]
    assert len(re.findall(r"\bcount_runs\s*<[^>]*>\s*\(", scan)) == 2     # the two counting kernels
    assert len(re.findall(r"\bput_tile_sums\s*\(", compact)) == 3          # its definition and the two selects
    for kernel in ("k_scan_count", "k_scan_count_where", "k_scan_emit"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, scan), kernel
    for kernel in ("k_compact_format", "k_compact_select", "k_compact_lww_tiles"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, compact), kernel
    # the copier's header names nothing of the row rules
    assert not re.search(r"liverow|rowts|rowjson|value_dead|row_matches|decoded_ts", code["compact.hpp"])


# ---- argument errors --------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


class W(ctypes.Structure):
    _fields_ = [("cols", ctypes.c_char_p), ("col_off", ctypes.POINTER(ctypes.c_uint64)), ("vals", ctypes.c_char_p),
                ("val_off", ctypes.POINTER(ctypes.c_uint64)), ("part", ctypes.POINTER(ctypes.c_int32)),
                ("nc", ctypes.c_uint32)]


def u64s(*xs):
    return (ctypes.c_uint64 * len(xs))(*xs)


def i32s(*xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def good_where():
    return W(b"cd", u64s(0, 1, 2), b"vwx", u64s(0, 1, 3), i32s(-1, 0), 2)


def bad_wheres():
    """(why, predicate or None, a part of the message)."""
    big = b"x" * 5000
    yield "w NULL", None, "null predicate"
    yield "null col_off", W(b"c", None, b"v", u64s(0, 1), i32s(-1), 1), "null condition offsets"
    yield "null val_off", W(b"c", u64s(0, 1), b"v", None, i32s(-1), 1), "null condition offsets"
    yield "null part", W(b"c", u64s(0, 1), b"v", u64s(0, 1), None, 1), "null condition offsets"
    yield "null cols with bytes", W(None, u64s(0, 1), b"v", u64s(0, 1), i32s(-1), 1), "null names or values"
    yield "null vals with bytes", W(b"c", u64s(0, 1), None, u64s(0, 1), i32s(-1), 1), "null names or values"
    yield "col_off decreases", W(b"cd", u64s(1, 0), b"v", u64s(0, 1), i32s(-1), 1), "offsets decrease"
    yield "val_off decreases", W(b"cd", u64s(0, 1, 2), b"vw", u64s(0, 2, 1), i32s(-1, -1), 2), "offsets decrease"
    yield "17 conditions", W(b"", u64s(*[0] * 18), b"", u64s(*[0] * 18), i32s(*[-1] * 17), 17), "too many conditions"
    yield "4097 bytes", W(big, u64s(0, 4000), big, u64s(0, 97), i32s(-1), 1), "too many bytes"
    yield "4097 bytes of names", W(big, u64s(0, 4097), b"", u64s(0, 0), i32s(-1), 1), "too many bytes"
    yield "a huge total", W(big, u64s(0, 2 ** 64 - 1), big, u64s(0, 2), i32s(-1), 1), "too many bytes"
    yield "part -2", W(b"c", u64s(0, 1), b"v", u64s(0, 1), i32s(-2), 1), "key part index"
    yield "part 256", W(b"cd", u64s(0, 1, 2), b"v", u64s(0, 1, 1), i32s(255, 256), 2), "key part index"


def test_argument_errors_need_no_device():
    import lsmt_amd
    from lsmt_amd import _lib
    L = _lib.load()
    null_entry = ctypes.cast((ctypes.c_void_p * 2)(None, None), ctypes.c_void_p)
    off1 = u64s(0, 1, 2)        # one range: [a, b)
    off2 = u64s(0, 1, 2, 3, 4)  # two ranges
    skip2 = (ctypes.c_uint32 * 2)(1, 1)

    def ref(w):
        return ctypes.addressof(w) if w is not None else None

    def count(w, tables=null_entry, nt=2, bounds=b"abcd", off=off2, nr=2, unb=0, live=True, matched=True, lww=0):
        lv, ma = np.full(max(nr, 1), 0xDEAD, np.uint64), np.full(max(nr, 1), 0xDEAD, np.uint64)
        rc = L.cb_tables_count_where(tables, nt, bounds, off, nr, unb, skip2, ref(w), lww, None,
                                     lv.ctypes.data if live else None, ma.ctypes.data if matched else None)
        return rc, lv[:nr].tolist(), ma[:nr].tolist()

    def row(w, key=b"ns:k", value=b"12345678{}"):
        out = ctypes.c_int(0xDEAD)
        rc = L.cb_row_matches(key, len(key) if key else 4, 3, value, len(value) if value else 4, ref(w),
                              ctypes.byref(out))
        return rc, out.value

    flags = np.full(4, 0xAD, np.uint8)
    # every refusal of the predicate, from all three entries, before the table list or the result is looked at
    for why, w, msg in bad_wheres():
        for lww in (0, 1):
            assert count(w, lww=lww) == (CB_EINVAL, [0, 0], [0, 0]), why
            assert msg in last_error(L), (why, last_error(L))
        assert count(w, live=False) == (CB_EINVAL, [0xDEAD] * 2, [0, 0]), why
        assert row(w) == (CB_EINVAL, 0), why
        assert msg in last_error(L), (why, last_error(L))
        assert L.cb_scan_match(None, None, ref(w), flags.ctypes.data) == CB_EINVAL, why
        assert msg in last_error(L), (why, last_error(L))
    assert flags.tolist() == [0xAD] * 4
    # null outputs
    good = good_where()
    assert count(good, matched=False) == (CB_EINVAL, [0, 0], [0xDEAD] * 2) and last_error(L) == "null argument"
    assert L.cb_scan_match(None, None, ref(good), None) == CB_EINVAL and last_error(L) == "null argument"
    assert L.cb_row_matches(b"k", 1, 0, b"v", 1, ref(good), None) == CB_EINVAL and last_error(L) == "null argument"
    # a good predicate: the range list is next, then the table list (cb_tables_count's refusals)
    assert count(good, bounds=b"adbe") == (CB_EINVAL, [0, 0], [0, 0]) and "ascending and disjoint" in last_error(L)
    assert count(good, off=None)[0] == CB_EINVAL and last_error(L) == "null bound offsets"
    for lww in (0, 1):
        assert count(good, lww=lww) == (CB_EINVAL, [0, 0], [0, 0]) and last_error(L) == "null table"
    assert count(good, live=False) == (CB_EINVAL, [0xDEAD] * 2, [0, 0]) and last_error(L) == "null table"
    assert count(good, tables=None, nt=0)[0] == CB_EINVAL and last_error(L) == "no tables"
    assert count(good, bounds=b"ab", off=off1, nr=1)[0] == CB_EINVAL and last_error(L) == "null table"
    assert count(good, bounds=b"", off=None, nr=0)[0] == CB_EINVAL and last_error(L) == "null table"  # no range is legal
    assert L.cb_scan_match(None, None, ref(good), flags.ctypes.data) == CB_EINVAL and last_error(L) == "null scan"
    # legal predicates: no condition (all pointers null), empty names and values
    for w in (W(None, None, None, None, None, 0), W(None, u64s(0, 0), None, u64s(0, 0), i32s(-1), 1),
              W(b"", u64s(0, 0, 0), b"", u64s(0, 0, 0), i32s(255, -1), 2)):
        assert count(w) == (CB_EINVAL, [0, 0], [0, 0]) and last_error(L) == "null table"
    assert row(W(None, None, None, None, None, 0)) == (CB_OK, 1)
    assert row(W(None, u64s(0, 0), None, u64s(0, 0), i32s(-1), 1), value=b'{"":""}') == (CB_OK, 1)
    assert row(W(None, None, None, None, None, 0), key=None) == (CB_EINVAL, 0)
    assert row(W(None, None, None, None, None, 0), value=None) == (CB_EINVAL, 0)
    # the Python entries
    with pytest.raises(ValueError):
        lsmt_amd.count_where([], {"c": "v"}, ranges=[(b"a", b"b")], prefixes=[b"a"])
    with pytest.raises(ValueError):
        lsmt_amd.count_where([], {"c": "v"})
    with pytest.raises(ValueError):
        lsmt_amd.count_where([], {"c": "v"}, prefixes=[b"a", b"b"], skip=[1])
    with pytest.raises(_lib.CassBloomError) as ei:
        lsmt_amd.count_where([], {"c": "v"}, prefixes=[b"a"])  # no tables
    assert ei.value.code == CB_EINVAL
    with pytest.raises(_lib.CassBloomError) as ei:
        lsmt_amd.count_where([], [("c%d" % i, "v") for i in range(17)], prefixes=[b"a"])
    assert ei.value.code == CB_EINVAL and "too many conditions" in str(ei.value)
    with pytest.raises(_lib.CassBloomError):
        lsmt_amd.row_matches(b"k", b"v", {"c": "v" * 5000})


# ---- the restatement --------------------------------------------------------------------

def test_known_answers_restated():
    """tests/rowjson_ref.py gives the hand-worked answer of every case."""
    assert len(CASES) > 400 and len(set(c.label for c in CASES)) == len(CASES)
    assert sum(c.expect for c in CASES) > 80
    for c in CASES:
        assert rowjson_ref.matches(c.key, c.value, c.where, c.key_columns, c.skip) is c.expect, c.label
    assert rowjson_ref.payload(b"1234567") == b"1234567" and rowjson_ref.payload(b"12345678") == b""
    assert rowjson_ref.payload(b"123456789") == b"9" and rowjson_ref.payload(b"") == b""
    assert rowjson_ref.parts(b"ns:", 3) == [b""] and rowjson_ref.parts(b"ns:a||c", 3) == [b"a", b"", b"c"]
    assert rowjson_ref.parts(b"ns", 9) == [b""]
    assert rowjson_ref.json_map(b'{"a":"1","a":"2","b":"\\ud83d\\ude00"}') == {b"a": b"2", b"b": "\U0001F600".encode()}
    assert rowjson_ref.json_map(b'{"a":"1","b":2}') == {}


def witness_map(p: bytes) -> dict:
    """The map by Python's json module: strict UTF-8 decode, then
    json.loads(strict=True, object_pairs_hook=list)."""
    try:
        text = p.decode("utf-8", "strict")
        pairs = json.loads(text, strict=True, object_pairs_hook=list)
    except (UnicodeDecodeError, ValueError, RecursionError):
        return {}
    if not text.lstrip(" \t\n\r").startswith("{") or not isinstance(pairs, list):
        return {}
    out = {}
    for pair in pairs:
        if not (isinstance(pair, tuple) and len(pair) == 2 and isinstance(pair[1], str)):
            return {}
        if any(0xD800 <= ord(ch) <= 0xDFFF for ch in pair[0] + pair[1]):
            return {}
        out[pair[0].encode()] = pair[1].encode()
    return out


# ---- mutated documents ------------------------------------------------------------------

BASES = [b'{"c":"v","name":"Ada","n":"1"}', b'{ "name" : "Ada" , "c" : "v" }', b'{"c":"\\u0076","d":"\\ud83d\\ude00"}',
         b'{"c":"x","c":"v"}', b'{"d":"\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80","c":"v"}', b'{"c":"v"}',
         b'{"a\\nb":"\\"q\\"","c":"v","e":""}', b'{"c":"v","k":"\\\\"}']
ALPHABET = b'{}",:\\u \t\n\r[]0123456789abcdefnulltrue\x00\x1f\x7f\x80\xbf\xc3\xa9\xe2\xed\xa0\xf0\xf4\xff' + b"vcdD8"


def mutated_docs(n=5000, seed=20261020):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        d = bytearray(BASES[i % len(BASES)])
        for _ in range(int(rng.integers(1, 3))):
            kind, at = int(rng.integers(0, 4)), int(rng.integers(0, len(d) + 1))
            b = ALPHABET[int(rng.integers(0, len(ALPHABET)))] if rng.random() < 0.7 else int(rng.integers(0, 256))
            if kind == 0 and at < len(d):
                d[at] = b if rng.random() < 0.5 else d[at] ^ (1 << int(rng.integers(0, 8)))
            elif kind == 1:
                d.insert(at, b)
            elif kind == 2 and at < len(d):
                del d[at]
            elif kind == 3:
                del d[at:]
        docs.append(bytes(d))
    return docs


def test_python_json_is_a_second_witness():
    """On the known answers' payloads and the mutated documents,
    rowjson_ref.json_map equals the map Python's json module reads, accepted
    only when the top level is an object (a list of pairs under
    object_pairs_hook=list), every value is a str, and no code point in
    D800-DFFF occurs. Those are the known differences between json.loads and
    serde_json::from_slice::<BTreeMap<String, String>>: json.loads takes any
    top-level value, values of any type (NaN and Infinity included) and lone
    surrogate escapes, which serde_json refuses; raw UTF-8 errors and control
    bytes in strings both refuse (strict decode, strict=True)."""
    docs = [rowjson_ref.payload(c.value) for c in CASES] + mutated_docs()
    valid = 0
    for p in docs:
        got = rowjson_ref.json_map(p)
        assert got == witness_map(p), p
        valid += bool(got)
    assert 500 < valid < len(docs) - 500  # (a property of the generator: both verdicts are well represented)


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rowjson") / "rowjson_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rowjson_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def hx(b) -> str:
    b = b.encode() if isinstance(b, str) else bytes(b)
    return b.hex() or "-"


def request(key, value, where, key_columns=(), skip=0) -> str:
    conds = rowjson_ref.normalize(where, key_columns)
    return " ".join(["M", str(skip), hx(key), hx(value), base64.b64encode(value).decode() or "-", str(len(conds))] +
                    ["%s %s %d" % (hx(c), hx(v), p) for c, v, p in conds])


def run_driver(driver, requests):
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(requests)
    return got


def lib_row_matches(key, value, where, key_columns=(), skip=0) -> bool:
    """cb_row_matches through plain ctypes (not the package's wrapper)."""
    from lsmt_amd import _lib
    conds = rowjson_ref.normalize(where, key_columns)
    cols, vals = b"".join(c for c, _, _ in conds), b"".join(v for _, v, _ in conds)
    w = W(cols, u64s(*np.cumsum([0] + [len(c) for c, _, _ in conds]).tolist()), vals,
          u64s(*np.cumsum([0] + [len(v) for _, v, _ in conds]).tolist()), i32s(*[p for _, _, p in conds]), len(conds))
    out = ctypes.c_int(-1)
    assert _lib.load().cb_row_matches(key, len(key), skip, value, len(value), ctypes.addressof(w), ctypes.byref(out)) == 0
    assert out.value in (0, 1)
    return bool(out.value)


def test_known_answers_under_sanitizers(driver):
    import lsmt_amd
    got = run_driver(driver, [request(c.key, c.value, c.where, c.key_columns, c.skip) for c in CASES])
    for c, g in zip(CASES, got):
        want = "%d %d" % (c.expect, c.expect)
        assert g == want, f"{c.label}: driver {g!r} against {want!r}"
        assert lib_row_matches(c.key, c.value, c.where, c.key_columns, c.skip) is c.expect, c.label
        assert lsmt_amd.row_matches(c.key, c.value, c.where, c.key_columns, c.skip) is c.expect, c.label


def test_driver_refuses_what_the_library_refuses(driver):
    many = [("c%d" % i, "v") for i in range(17)]
    got = run_driver(driver, [request(b"k", b"v", many), request(b"k", b"v", [("c", "v" * 4096)]),
                              request(b"k", b"v", [("c", "v")], ("x",) * 256 + ("c",)),
                              request(b"k", TS + b'{"c":"%s"}' % (b"v" * 4095), [("c", "v" * 4095)])])
    assert got == ["E", "E", "E", "1 1"]


def test_mutated_documents_agree(driver):
    """About 5000 documents, each a valid row after a byte flip, an insert, a
    delete or a truncation (one or two of them): the driver's two readers,
    cb_row_matches and the restatement agree on every one."""
    docs = mutated_docs()
    wheres = [[("c", "v")], [("c", "v"), ("name", "Ada")], [("d", "\U0001F600")], [("pk", "k"), ("c", "v")]]
    # (every base document meets every predicate; one value in seven is its own payload)
    rows = [(b"ns:k|x", TS + d if i % 7 else d, wheres[i // len(BASES) % len(wheres)], ("pk",), 3)
            for i, d in enumerate(docs)]
    want = [rowjson_ref.matches(*r) for r in rows]
    got = run_driver(driver, [request(*r) for r in rows])
    for r, g, w in zip(rows, got, want):
        assert g == "%d %d" % (w, w), (r[1], r[2], g)
        assert lib_row_matches(*r) is w, (r[1], r[2])
    assert 100 < sum(want) < len(rows) - 100  # (a property of the generator: both verdicts occur often)
