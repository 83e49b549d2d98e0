"""The token ring's surface and host half (cb_ring_*, cb_scan_route,
cb_tables_compact_ring; lsmt_amd.ring), checked without a GPU: the header's
declarations, the ctypes prototypes, the integration document and the Python
signatures; the restatement in tests/ring_ref.py against the pinned vectors;
the host entries against it; the refusals that touch no device; the rule
(lsmt_amd/csrc/ring.hpp) under the address and undefined-behaviour sanitizers
through a stand-alone driver (tests/cpp/ring_driver.cpp); and the one-home
checks of the new sources.
"""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL, CB_EZEROM = 0, -1, -2

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_ring_create": ["names", "name_off", "nnodes", "vnodes", "rf", "out"],
    "cb_ring_create_tokens": ["tokens", "owners", "npos", "nnodes", "rf", "out"],
    "cb_ring_info": ["ring", "nnodes", "rf", "positions", "width"],
    "cb_ring_tokens": ["ring", "tokens", "owners"],
    "cb_ring_replicas": ["ring", "key", "len", "skip", "npk", "token", "replicas"],
    "cb_ring_destroy": ["ring"],
    "cb_ring_route_fixed": ["ring", "keys", "key_len", "n", "skip", "npk", "device", "tokens", "replicas", "stream"],
    "cb_ring_route_var": ["ring", "bytes", "offsets", "n", "skip", "npk", "device", "tokens", "replicas", "stream"],
    "cb_scan_route": ["r", "ring", "skip", "npk", "tokens", "replicas"],
    "cb_tables_compact_ring": ["tables", "nt", "m_bits", "ring", "node", "ranks", "rules", "lww", "drop_dead",
                               "stream", "table_out", "bloom_out"],
}
CITES = ("src/cluster.rs:46-54", "src/cluster.rs:102-123", "src/query.rs:448-528", "697-713", "734-760")

# (input, token): MurmurHash3 x86_32, seed 0
VECTORS = [(b"", 0x00000000), (b"a", 0x3C2569B2), (b"ab", 0x9BBFD75F), (b"abc", 0xB3DD93FA), (b"abcd", 0x43ED676A),
           (b"hello", 0x248BFA47), (b"Hello, world!", 0xC0363E43),
           (b"The quick brown fox jumps over the lazy dog", 0x2E4FF723), (b"somekey", 0x4BC663ED),
           (b"http://n1-0", 0xC5B2908E), (b"\xff\xfe\x80", 0x12CB5F1F), ("é|ü".encode(), 0xADC5FC1A)]


RINGS, TOKEN_RINGS = ring_ref.RINGS, ring_ref.TOKEN_RINGS


def sample_keys(n=400):
    """Keys of many shapes: ASCII, high bytes, every length 0..13, parts."""
    rng = np.random.default_rng(7)
    keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8)) for _ in range(n)]
    keys += [b"x" * i for i in range(14)] + [bytes([0x80 + i] * i) for i in range(14)]
    keys += [b"user|%d|c%d" % (i, i % 5) for i in range(50)]
    return keys


def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the ring exists."""
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
    # the new section follows the SELECT one, knows no new handle type and cites the reference
    assert raw_header.index("cb_rows_destroy(") < raw_header.index("cb_ring_create(")
    assert "cb_ring*" not in header and "cb_ring *" not in header
    assert re.search(r"typedef\s+struct\s+cb_key_rules\s*\{[^}]*prefixes[^}]*prefix_off[^}]*npk[^}]*np;\s*\}", header)
    with open(os.path.join(CSRC, "ring.hpp")) as fh:
        rule = fh.read()
    for cite in CITES:
        assert cite in raw_header and cite in rule, cite
    assert "src/cluster.rs:277-286" in raw_header
    assert re.search(r"NOT\s+run\s+against\s+the\s+reference", rule)
    assert "hip_runtime" not in rule  # no HIP dependency: the driver builds it with a host compiler
    assert re.search(r"no\s+table\s+or\s+replica\s+of\s+the\s+store\s+stays\s+outside",
                     raw_header[raw_header.index("cb_key_rules"):])
    # the Python surface: reached as lsmt_amd.ring, nothing added to the package's own
    import lsmt_amd.ring as ring
    with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as fh:
        assert sorted(lsmt_amd.__all__) == sorted(json.load(fh))
    assert not hasattr(ring, "__all__")
    sig = lambda f: [(k, p.default) for k, p in inspect.signature(f).parameters.items()]  # noqa: E731
    E = inspect.Parameter.empty
    assert sig(ring.Ring.__init__)[:4] == [("self", E), ("nodes", E), ("vnodes", 8), ("rf", 1)]
    assert sig(ring.Ring.from_tokens) == [("tokens", E), ("owners", E), ("nnodes", E), ("rf", 1)]
    assert sig(ring.Ring.tokens) == [("self", E)]
    assert sig(ring.Ring.replicas) == [("self", E), ("key", E), ("skip", 0), ("npk", 0)]
    assert sig(ring.Ring.route) == [("self", E), ("keys", E), ("skip", 0), ("npk", 0), ("stream", None)]
    assert sig(ring.route_scan) == [("result", E), ("ring", E), ("skip", None), ("npk", None)]
    assert sig(ring.compact_ring) == [("tables", E), ("ring", E), ("node", E), ("rules", ()), ("m", 1024), ("ranks", 0),
                                      ("lww", False), ("drop_dead", False), ("stream", None)]
    for prop in ("nnodes", "rf", "width", "positions"):
        assert isinstance(getattr(ring.Ring, prop), property), prop
    assert re.search(r"kRingLdsPositions\s*=\s*%d\s*;" % ring.LDS_POSITIONS, rule)


def test_imports_alone():
    """lsmt_amd.ring imports first in a fresh process."""
    r = subprocess.run([os.sys.executable, "-c", "import lsmt_amd.ring as r; print(r.Ring.__name__)"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "Ring", r.stderr[-2000:]


# ---- the restatement --------------------------------------------------------------------

def test_vectors():
    for data, token in VECTORS:
        assert ring_ref.murmur3_32(data) == token, data


def test_vectors_against_sklearn():
    sk = pytest.importorskip("sklearn.utils")
    for data, _ in VECTORS + [(k, 0) for k in sample_keys(60)]:
        assert ring_ref.murmur3_32(data) == sk.murmurhash3_32(data, seed=0, positive=True), data


def test_partition_key_restated():
    pk = ring_ref.partition_key
    assert pk(b"ns:a|b|c", 3, 0) == b"a|b|c" and pk(b"ns:a|b|c", 3, 1) == b"a" and pk(b"ns:a|b|c", 3, 2) == b"a|b"
    assert pk(b"ns:a|b|c", 3, 3) == b"a|b|c" and pk(b"ns:a|b|c", 3, 9) == b"a|b|c"
    assert pk(b"ns:a|b|c", 99, 1) == b"" and pk(b"a||c", 0, 2) == b"a|" and pk(b"a||c", 0, 1) == b"a"
    assert pk(b"a|b|", 0, 2) == b"a|b" and pk(b"a|b|", 0, 3) == b"a|b|" and pk(b"", 0, 1) == b""


# ---- the host entries -------------------------------------------------------------------

def check_ring(r, ref, keys):
    assert (r.nnodes, r.rf, r.width, r.positions) == (ref.nnodes, ref.rf, ref.width, len(ref.sorted))
    t, o = r.tokens()
    assert (t.tolist(), o.tolist()) == tuple(map(list, ref.tokens()))
    for key, skip, npk in keys:
        token, reps = ref.replicas(key, skip, npk)
        assert reps[:ref.width].count(-1) == 0 and reps[ref.width:] == [-1] * (ref.rf - ref.width)
        assert r.replicas(key, skip, npk) == (token, reps[:ref.width]), (key, skip, npk)
    # the raw list is rf wide, -1 past width
    from lsmt_amd import _lib
    raw = np.full(ref.rf, 77, np.int32)
    assert _lib.load().cb_ring_replicas(r._h, b"abc", 3, 0, 0, None, raw.ctypes.data) == CB_OK
    assert raw.tolist() == ref.replicas(b"abc")[1]


def keys_for(ref):
    """Sample keys, every ring token's own neighbourhood, and keys that wrap
    past the ring's largest token and fall below its smallest."""
    keys = [(k, 0, 0) for k in sample_keys()]
    keys += [(b"ns:" + k, 3, n) for k in (b"a|b|c", b"a||c", b"a|b|", b"", b"|") for n in (0, 1, 2, 5)]
    keys += [(b"ab", 9, 1)]
    tokens = [ring_ref.murmur3_32(k) for k, _, _ in keys]
    if len(ref.sorted) < 1000 and 0 < ref.sorted[0] and ref.sorted[-1] < ring_ref.M32:
        assert any(t > ref.sorted[-1] for t in tokens) and any(t < ref.sorted[0] for t in tokens)
    return keys


@pytest.mark.parametrize("name", sorted(RINGS))
def test_ring_create(name):
    from lsmt_amd import ring
    names, vnodes, rf = RINGS[name]
    ref = ring_ref.Ring(names, vnodes, rf)
    r = ring.Ring(names, vnodes, rf)
    check_ring(r, ref, keys_for(ref))
    if name == "3 rf5":
        assert (r.width, r.rf) == (3, 5)
    if name == "zeros":
        assert (r.rf, r.positions) == (1, 4)
    if name == "64x256":
        assert r.positions > ring.LDS_POSITIONS
    r.close()


@pytest.mark.parametrize("name", sorted(TOKEN_RINGS))
def test_ring_create_tokens(name):
    from lsmt_amd import ring
    pairs, nnodes, rf = TOKEN_RINGS[name]
    ref = ring_ref.Ring(pairs=pairs, nnodes=nnodes, rf=rf)
    r = ring.Ring.from_tokens([t for t, _ in pairs], [o for _, o in pairs], nnodes, rf)
    check_ring(r, ref, keys_for(ref))
    if name == "repeat":
        assert r.tokens()[1].tolist() == [2, 1, 1] and r.width == 2
    if name == "overwritten":
        assert r.width == 2 and r.rf == 3  # node 0's only position was replaced
    if name == "edges":
        # tokens 0 and 0xFFFFFFFF are positions like any other
        assert r.tokens()[0].tolist() == [0, 0x80000000, 0xFFFFFFFF]
        assert ref.replicas_for_token(0) == [1, 2, 0] and ref.replicas_for_token(0xFFFFFFFF) == [0, 1, 2]
        assert r.replicas(b"")[1] == [1, 2, 0]  # the empty key's token is 0: range(0..) is inclusive


def test_token_equal_to_a_ring_token():
    """The key "n0-3" routed whole on a ring that has node n0: its token is a
    position's, and range(token..) includes it."""
    from lsmt_amd import ring
    names, vnodes, rf = RINGS["3x8"]
    ref, r = ring_ref.Ring(names, vnodes, rf), ring.Ring(names, vnodes, rf)
    token = ring_ref.murmur3_32(b"n0-3")
    assert token in ref.ring and ref.ring[token] == 0
    assert ref.replicas(b"n0-3")[1][0] == 0
    assert r.replicas(b"n0-3") == (token, ref.replicas(b"n0-3")[1][:ref.width])


# ---- refusals ---------------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


def test_refusals_touch_no_device():
    from lsmt_amd import _lib, ring
    L = _lib.load()

    def create(names, vnodes=8, rf=1, off=None, nn=None, null=()):
        joined = b"".join(names)
        off = np.array(off if off is not None else np.cumsum([0] + [len(x) for x in names]), np.uint64)
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_ring_create(None if "names" in null else joined + b"\0", None if "off" in null else off.ctypes.data,
                              len(names) if nn is None else nn, vnodes, rf, ctypes.byref(out))
        return rc, out.value

    def create_tokens(tokens, owners, nnodes, rf=1, npos=None, null=()):
        t, o = np.array(tokens + [0], np.uint32), np.array(owners + [0], np.uint32)
        out = ctypes.c_void_p(0xDEAD)
        rc = L.cb_ring_create_tokens(None if "tokens" in null else t.ctypes.data,
                                     None if "owners" in null else o.ctypes.data,
                                     len(tokens) if npos is None else npos, nnodes, rf, ctypes.byref(out))
        return rc, out.value

    refused = (CB_EINVAL, None)
    assert L.cb_ring_create(b"a", np.zeros(2, np.uint64).ctypes.data, 1, 1, 1, None) == CB_EINVAL
    assert L.cb_ring_create_tokens(np.zeros(1, np.uint32).ctypes.data, np.zeros(1, np.uint32).ctypes.data, 1, 1, 1,
                                   None) == CB_EINVAL
    assert create([b"a"], null=("names",)) == refused and create([b"a"], null=("off",)) == refused
    assert create([]) == refused and "1 to 4096 nodes" in last_error(L)
    assert create([b"a"], nn=4097, off=[0] * 4098) == refused and "1 to 4096 nodes" in last_error(L)
    assert create([b"a"], vnodes=4097) == refused and "vnodes" in last_error(L)
    assert create([b"a"], rf=17) == refused and "rf" in last_error(L)
    many = [b"%d" % i for i in range(300)]
    assert create(many, vnodes=4096) == refused and "positions" in last_error(L)  # 300 * 4096 > 2^20
    assert create([b"ab", b"c"], off=[0, 2, 1]) == refused and "decrease" in last_error(L)
    assert create([b"a", b"", b"b"]) == refused and "empty node name" in last_error(L)
    assert create([b"a", b"b", b"a"]) == refused and "share a name" in last_error(L)
    assert create_tokens([1], [0], 1, null=("tokens",)) == refused
    assert create_tokens([1], [0], 1, null=("owners",)) == refused
    assert create_tokens([], [], 1) == refused and "at least one position" in last_error(L)
    assert create_tokens([1], [0], 0) == refused and create_tokens([1], [0], 4097) == refused
    assert create_tokens([1], [0], 1, rf=17) == refused
    assert create_tokens([1, 2], [0, 2], 2) == refused and "owner" in last_error(L)
    assert create_tokens([1], [0], 1, npos=(1 << 20) + 1) == refused and "positions" in last_error(L)
    # the handle's entries
    assert L.cb_ring_info(None, None, None, None, None) == CB_EINVAL and last_error(L) == "null ring"
    assert L.cb_ring_tokens(None, None, None) == CB_EINVAL
    assert L.cb_ring_replicas(None, b"a", 1, 0, 0, None, None) == CB_EINVAL
    assert L.cb_ring_destroy(None) == CB_OK
    r = ring.Ring([b"a", b"b"], 4, 2)
    assert L.cb_ring_replicas(r._h, None, 3, 0, 0, None, None) == CB_EINVAL
    assert L.cb_ring_info(r._h, None, None, None, None) == CB_OK
    # routes: both outputs NULL, a null ring, null offsets; n == 0 writes nothing and needs no device
    tok = np.full(2, 0xDEAD, np.uint32)
    assert L.cb_ring_route_fixed(r._h, b"ab", 1, 2, 0, 0, 0, None, None, None) == CB_EINVAL
    assert last_error(L) == "null argument"
    assert L.cb_ring_route_fixed(None, b"ab", 1, 2, 0, 0, 0, tok.ctypes.data, None, None) == CB_EINVAL
    assert L.cb_ring_route_var(r._h, b"ab", None, 2, 0, 0, 0, tok.ctypes.data, None, None) == CB_EINVAL
    assert L.cb_ring_route_var(r._h, b"ab", np.zeros(3, np.uint64).ctypes.data, 2, 0, 0, 0, None, None,
                               None) == CB_EINVAL
    assert L.cb_ring_route_fixed(r._h, b"ab", 1, 0, 0, 0, 0, tok.ctypes.data, None, None) == CB_OK
    assert L.cb_ring_route_var(r._h, b"", np.zeros(1, np.uint64).ctypes.data, 0, 0, 0, 0, tok.ctypes.data, None,
                               None) == CB_OK
    assert tok.tolist() == [0xDEAD] * 2
    assert L.cb_scan_route(None, r._h, None, None, None, None) == CB_EINVAL and last_error(L) == "null argument"
    assert L.cb_scan_route(None, None, None, None, tok.ctypes.data, None) == CB_EINVAL and last_error(L) == "null ring"
    assert L.cb_scan_route(None, r._h, None, None, tok.ctypes.data, None) == CB_EINVAL and last_error(L) == "null scan"
    # the compaction's own arguments, before the table list, outputs cleared
    null_entry = ctypes.cast((ctypes.c_void_p * 2)(None, None), ctypes.c_void_p)

    def rules_of(pairs, np_=None, null=()):
        prefixes = b"".join(p for p, _ in pairs) + b"\0"
        off = np.array(np.cumsum([0] + [len(p) for p, _ in pairs]), np.uint64)
        npk = np.array([n for _, n in pairs] + [0], np.uint32)
        keep = (prefixes, off, npk)
        c = _lib.KeyRules(None if "prefixes" in null else ctypes.cast(ctypes.c_char_p(prefixes), ctypes.c_void_p),
                          None if "off" in null else off.ctypes.data, None if "npk" in null else npk.ctypes.data,
                          len(pairs) if np_ is None else np_)
        return c, keep

    def compact(rules, ring_h=r._h, node=0, ranks=0, m_bits=1024, bloom=True, tables=null_entry, nt=2):
        th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xDEAD)
        rc = L.cb_tables_compact_ring(tables, nt, m_bits, ring_h, node, ranks,
                                      ctypes.addressof(rules[0]) if rules else None, 0, 0, None, ctypes.byref(th),
                                      ctypes.byref(fh) if bloom else None)
        return rc, th.value, fh.value if bloom else None

    cleared = (CB_EINVAL, None, None)
    good = rules_of([(b"a:", 1), (b"b:", 2)])
    assert L.cb_tables_compact_ring(null_entry, 2, 1024, r._h, 0, 0, ctypes.addressof(good[0]), 0, 0, None, None,
                                    None) == CB_EINVAL and last_error(L) == "null argument"
    assert compact(good, ring_h=None) == cleared and last_error(L) == "null ring"
    assert compact(good, node=2) == cleared and "not a node" in last_error(L)
    assert compact(good, ranks=17) == cleared and "ranks" in last_error(L)
    assert compact(None) == cleared and last_error(L) == "null rules"
    assert compact(rules_of([(b"b:", 1), (b"a:", 1)])) == cleared and "ascending and disjoint" in last_error(L)
    assert compact(rules_of([(b"a:", 1), (b"a:b:", 1)])) == cleared and "ascending and disjoint" in last_error(L)
    assert compact(rules_of([(b"a:", 1), (b"a:", 2)])) == cleared
    assert compact(rules_of([(b"", 1), (b"a:", 1)])) == cleared and "without an end" in last_error(L)
    assert compact(rules_of([(b"a:", 1)], null=("off",))) == cleared
    assert compact(rules_of([(b"a:", 1)], null=("npk",))) == cleared
    assert compact(rules_of([(b"a:", 1)], null=("prefixes",))) == cleared
    assert compact(rules_of([(b"a:", 1)], np_=257)) == cleared and "at most 256" in last_error(L)
    assert compact(rules_of([(b"a" * 4000, 1), (b"b" * 97, 1)])) == cleared and "4096" in last_error(L)
    assert compact(good, m_bits=0) == (CB_EZEROM, None, None)
    # with its own arguments in order the table list is looked at: cb_tables_compact's refusals
    assert compact(good) == cleared and last_error(L) == "null table"
    assert compact(rules_of([])) == cleared and last_error(L) == "null table"  # np == 0 is legal
    assert compact(good, m_bits=0, bloom=False) == (CB_EINVAL, None, None) and last_error(L) == "null table"
    assert compact(good, tables=None, nt=0) == cleared and last_error(L) == "no tables"
    # the Python entries
    with pytest.raises(_lib.CassBloomError):
        ring.Ring([])
    with pytest.raises(_lib.CassBloomError):
        ring.Ring([b"a", b"a"])
    with pytest.raises(_lib.CassBloomError):
        ring.Ring.from_tokens([], [], 1)
    with pytest.raises(ValueError):
        ring.Ring.from_tokens([1, 2], [0], 1)
    with pytest.raises(_lib.CassBloomError) as ei:
        ring.compact_ring([], r, 0, rules={b"a:": 1})
    assert ei.value.code == CB_EINVAL
    with pytest.raises(ZeroDivisionError):
        ring.compact_ring([], r, 0, m=0)
    r.close()


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ring") / "ring_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ring_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def run_driver(driver, requests):
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(requests)
    return got


def hx(b):
    return b.hex() or "-"


def test_hash_and_partition_key_under_sanitizers(driver):
    keys = [k for k, _ in VECTORS] + sample_keys(100)
    got = run_driver(driver, ["H " + hx(k) for k in keys])
    assert [int(x) for x in got] == [ring_ref.murmur3_32(k) for k in keys]
    cases = [(k, s, n) for k in (b"ns:a|b|c", b"a||c", b"a|b|", b"", b"|", b"||", b"abc", b"\xff|\x80|\xfe")
             for s in (0, 1, 3, 99) for n in (0, 1, 2, 3, 7)]
    got = run_driver(driver, ["P %d %d %s" % (s, n, hx(k)) for k, s, n in cases])
    for (k, s, n), line in zip(cases, got):
        start, length = map(int, line.split())
        assert start == min(s, len(k)) and k[start:start + length] == ring_ref.partition_key(k, s, n), (k, s, n)


def test_rings_under_sanitizers(driver):
    probes = sorted({ring_ref.murmur3_32(k) for k in sample_keys(150)} | {0, 1, 99, 100, 101, 0x7FFFFFFF, 0x80000000,
                                                                           0x80000001, 0xFFFFFFFE, 0xFFFFFFFF})

    def expect(ref):
        t, o = ref.tokens()
        head = "%d %d %s" % (ref.width, len(t), " ".join("%d:%d" % p for p in zip(t, o)))
        rows = [",".join(map(str, (lambda r: r + [-1] * (ref.rf - len(r)))(ref.replicas_for_token(p)))) for p in probes]
        return [head] + rows

    requests, want = [], []
    for name in sorted(RINGS):
        names, vnodes, rf = RINGS[name]
        ref = ring_ref.Ring(names, vnodes, rf)
        requests += ["N %d %d %s" % (vnodes, rf, " ".join(hx(x) for x in names))] + ["R %d" % p for p in probes]
        want += expect(ref)
    for name in sorted(TOKEN_RINGS):
        pairs, nnodes, rf = TOKEN_RINGS[name]
        ref = ring_ref.Ring(pairs=pairs, nnodes=nnodes, rf=rf)
        requests += ["X %d %d %s" % (nnodes, rf, " ".join("%d:%d" % p for p in pairs))] + ["R %d" % p for p in probes]
        want += expect(ref)
    # one node holds all but one position: the lists come from their successors, not from long walks
    pairs = [(10 * i, 0) for i in range(1, 500)] + [(7, 1)]
    ref = ring_ref.Ring(pairs=pairs, nnodes=2, rf=2)
    requests += ["X 2 2 %s" % " ".join("%d:%d" % p for p in pairs)] + ["R %d" % p for p in probes]
    want += expect(ref)
    assert run_driver(driver, requests) == want
    # refusals
    got = run_driver(driver, ["N 1 1 61 - 62", "N 1 1 61 62 61", "N 4097 1 61", "N 1 17 61", "X 0 1 1:0", "X 2 1 1:2",
                              "X 2 1", "X 2 17 1:0"])
    assert all(g.startswith("ERR ") for g in got), got


def test_key_rules_under_sanitizers(driver):
    rules = [(b"a:", 1), (b"ab", 2), (b"b:", 1), (b"b;x", 3), (b"\xff\xff", 1)]
    assert rules == sorted(rules)
    keys = [b"", b"a", b"a:", b"a:x|y", b"a;", b"ab", b"abc", b"aa", b"b", b"b:", b"b:zz", b"b;", b"b;x", b"b;xy",
            b"c", b"\xff", b"\xff\xff", b"\xff\xff\x00", b"_tables:t"]
    spec = " ".join("%s:%d" % (hx(p), n) for p, n in rules)
    got = run_driver(driver, ["U %s %s" % (hx(k), spec) for k in keys] + ["U %s" % hx(b"abc"), "U %s -:4" % hx(b"abc")])
    want = [next((i for i, (p, _) in enumerate(rules) if k.startswith(p)), -1) for k in keys] + [-1, 0]
    assert [int(x) for x in got] == want


# ---- one home ---------------------------------------------------------------------------

def test_the_ring_has_one_home():
    new_files = ["lsmt_amd/csrc/ring.hpp", "lsmt_amd/csrc/ring.hip", "lsmt_amd/csrc/capi_ring.cpp", "lsmt_amd/ring.py",
                 "tests/ring_ref.py", "tests/cpp/ring_driver.cpp", "tests/test_ring_gpu.py", "tools/ubench_ring.py"]
    sep = "'%s'" % chr(124)  # the separator as a character literal
    text = {}
    for fn in new_files:
        with open(os.path.join(ROOT, fn)) as fh:
            text[fn] = fh.read()
        assert sep not in text[fn], fn  # no second split of a key into parts
    with open(__file__) as fh:
        assert sep not in fh.read()
    hip = re.sub(r"//[^\n]*", "", text["lsmt_amd/csrc/ring.hip"])
    for kernel in ("k_ring_route", "k_ring_keep"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, hip), kernel
    # the parts come from rowjson.hpp's two functions, and nothing else of the row rules is used
    rule = re.sub(r"//[^\n]*", "", text["lsmt_amd/csrc/ring.hpp"])
    assert "key_part_count(" in rule and "key_part_at(" in rule
    for src in (hip, rule, re.sub(r"//[^\n]*", "", text["lsmt_amd/csrc/capi_ring.cpp"])):
        assert not re.search(r"liverow|value_dead|value_ts|lww_beats|decoded_ts|row_matches|where_\w+\s*\(", src)
    # the hash is written once
    users = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".hip", ".hpp", ".cpp"))
             and "0xcc9e2d51" in open(os.path.join(CSRC, fn)).read().lower()]
    assert users == ["ring.hpp"]
    # the tile sums still have one body and its three callers
    with open(os.path.join(CSRC, "compact.hip")) as fh:
        compact = re.sub(r"//[^\n]*", "", fh.read())
    assert len(re.findall(r"\bput_tile_sums\s*\(", compact)) == 3
    assert len(re.findall(r"hipLaunchKernelGGL\(k_compact_lww_tiles\b", compact)) == 1
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    for fn in ("ring.hip", "capi_ring.cpp", "ring.hpp"):
        assert re.search(r"\b%s\b" % re.escape(fn), make), fn
