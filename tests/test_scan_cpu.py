"""cb_tables_scan's surface, checked without a GPU: the Python entry points,
the header's declarations and the ctypes prototypes, the argument errors that
are refused before any device is touched, and the prefix's upper bound
(cb_key_prefix_end), both through the library and, under the address and
undefined-behaviour sanitizers, through a stand-alone driver of the host-only
code behind it (tests/cpp/keyrange_driver.cpp over lsmt_amd/csrc/keyrange.hpp).
"""
import ctypes
import inspect
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
    "cb_tables_scan": ["tables", "nt", "lo", "lo_len", "hi", "hi_len", "has_hi", "limit", "stream", "out"],
    "cb_tables_scan_prefix": ["tables", "nt", "prefix", "prefix_len", "limit", "stream", "out"],
    "cb_key_prefix_end": ["prefix", "len", "out", "out_len", "has_end"],
    "cb_scan_info": ["r", "count", "key_bytes", "val_bytes", "truncated"],
    "cb_scan_keys": ["r", "key_off", "keys"],
    "cb_scan_values": ["r", "val_off", "vals"],
    "cb_scan_which": ["r", "which"],
    "cb_scan_destroy": ["r"],
}

# prefix -> its end (None: unbounded above)
ENDS = [(b"", None), (b"a", b"b"), (b"ns:", b"ns;"), (b"a\xff", b"b"), (b"\xff\xff", None),
        (b"a\xfe\xff\xff", b"a\xff"), (b"\xff", None), (b"\x00", b"\x01"), (b"ab\xff\xff\xff", b"ac"),
        (b"\xfe\xff", b"\xff"), (b"k" * 300 + b"\xff" * 300, b"k" * 299 + b"l")]


def test_python_entry_points():
    import lsmt_amd
    assert "scan" in lsmt_amd.__all__ and "prefix_end" in lsmt_amd.__all__
    sig = inspect.signature(lsmt_amd.scan)
    assert list(sig.parameters) == ["tables", "lo", "hi", "prefix", "limit", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["lo"] == b"" and d["hi"] is None and d["prefix"] is None and d["limit"] == 0 and d["stream"] is None
    for name in ("count", "truncated"):
        assert name in inspect.getsource(lsmt_amd.ScanResult.__init__)
    for name in ("keys", "values", "which", "items", "raw", "close"):
        assert callable(getattr(lsmt_amd.ScanResult, name))
    with pytest.raises(ValueError):
        lsmt_amd.scan([], lo=b"a", prefix=b"a")
    with pytest.raises(ValueError):
        lsmt_amd.scan([], hi=b"b", prefix=b"a")


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_header_declares_it_and_ctypes_matches(name):
    from lsmt_amd import _lib
    assert name in _lib.header_symbols()
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "no prototype"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == SYMBOLS[name]
    fn = getattr(_lib.load(), name)  # (raises if the library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params)
    assert fn.restype is ctypes.c_int


def test_integration_doc_declares_it():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        text = fh.read()
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, text), name


@pytest.mark.parametrize("prefix,end", ENDS, ids=[repr(p[:8]) for p, _ in ENDS])
def test_prefix_end(prefix, end):
    import lsmt_amd
    assert lsmt_amd.prefix_end(prefix) == end


def test_prefix_end_abi_outputs():
    from lsmt_amd import _lib
    L = _lib.load()
    out = ctypes.create_string_buffer(b"\xaa" * 8, 8)
    n, has = ctypes.c_uint64(99), ctypes.c_int(99)
    assert L.cb_key_prefix_end(b"a\xff\xff", 3, out, ctypes.byref(n), ctypes.byref(has)) == 0
    assert (n.value, has.value, out.raw) == (1, 1, b"b" + b"\xaa" * 7)  # nothing past out_len is written
    assert L.cb_key_prefix_end(None, 0, None, ctypes.byref(n), ctypes.byref(has)) == 0
    assert (n.value, has.value) == (0, 0)
    assert L.cb_key_prefix_end(b"\xff", 1, out, ctypes.byref(n), ctypes.byref(has)) == 0
    assert (n.value, has.value) == (0, 0)
    assert L.cb_key_prefix_end(None, 3, out, ctypes.byref(n), ctypes.byref(has)) == CB_EINVAL
    assert L.cb_key_prefix_end(b"abc", 3, out, None, ctypes.byref(has)) == CB_EINVAL
    assert L.cb_key_prefix_end(b"abc", 3, out, ctypes.byref(n), None) == CB_EINVAL


def random_cases(seed, n):
    """(prefix, key) pairs over a 4-letter alphabet that holds 0xFF and 0x00, so
    that keys start with, follow and precede their prefixes often."""
    rng = np.random.default_rng(seed)
    alpha = np.array([0x00, 0x61, 0xFE, 0xFF], np.uint8)
    out = []
    for _ in range(n):
        p = alpha[rng.integers(0, 4, int(rng.integers(0, 5)))].tobytes()
        if rng.integers(0, 2):
            k = p[:int(rng.integers(0, len(p) + 1))] + alpha[rng.integers(0, 4, int(rng.integers(0, 4)))].tobytes()
        else:
            k = alpha[rng.integers(0, 4, int(rng.integers(0, 7)))].tobytes()
        out.append((p, k))
    return out


def test_prefix_range_is_starts_with():
    import lsmt_amd
    seen = set()
    for p, k in random_cases(7, 4000):
        end = lsmt_amd.prefix_end(p)
        inside = p <= k and (end is None or k < end)
        assert inside == k.startswith(p), (p, k, end)
        seen.add(inside)
    assert seen == {True, False}


def test_argument_errors_need_no_device():
    from lsmt_amd import _lib
    L = _lib.load()
    out = ctypes.c_void_p(0xDEAD)
    null_entry = (ctypes.c_void_p * 2)(None, None)
    tables = ctypes.cast(null_entry, ctypes.c_void_p)
    # out NULL
    assert L.cb_tables_scan(tables, 2, b"", 0, None, 0, 0, 0, None, None) == CB_EINVAL
    assert L.cb_tables_scan_prefix(tables, 2, b"", 0, 0, None, None) == CB_EINVAL
    # nt == 0 (with and without a list), a null entry: nothing returned
    for args in [(tables, 0), (None, 0), (None, 3), (tables, 2)]:
        out.value = 0xDEAD
        assert L.cb_tables_scan(*args, b"a", 1, b"b", 1, 1, 0, None, ctypes.byref(out)) == CB_EINVAL
        assert out.value is None
        assert L.cb_last_error()
        out.value = 0xDEAD
        assert L.cb_tables_scan_prefix(*args, b"a", 1, 0, None, ctypes.byref(out)) == CB_EINVAL
        assert out.value is None
    # the readers of a result refuse NULL; destroying NULL is a no-op
    n = ctypes.c_uint64()
    assert L.cb_scan_info(None, ctypes.byref(n), None, None, None) == CB_EINVAL
    assert L.cb_scan_keys(None, None, None) == CB_EINVAL
    assert L.cb_scan_values(None, None, None) == CB_EINVAL
    assert L.cb_scan_which(None, None) == CB_EINVAL
    assert L.cb_scan_destroy(None) == 0
    import lsmt_amd
    with pytest.raises(_lib.CassBloomError) as ei:
        lsmt_amd.scan([])
    assert ei.value.code == CB_EINVAL


# ---- the host-only code under the sanitizers --------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("keyrange") / "keyrange_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "keyrange_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def hexs(b: bytes) -> str:
    return b.hex() if b else "-"


def test_keyrange_under_sanitizers(driver):
    cases = random_cases(11, 3000)
    stdin = "".join(f"e {hexs(p)}\n" for p, _ in ENDS) + "".join(f"c {hexs(p)} {hexs(k)}\n" for p, k in cases)
    r = subprocess.run([driver], input=stdin, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(ENDS) + len(cases)
    for (p, end), ln in zip(ENDS, lines):
        assert ln == ("e 0" if end is None else f"e 1 {end.hex()}"), (p, ln)
    for (p, k), ln in zip(cases, lines[len(ENDS):]):
        assert ln == f"c {int(k.startswith(p))}", (p, k, ln)
