"""The log replay's surface and rule, checked without a GPU (cb_log_replay,
cb_log_line, cb_log_stats, CB_EBASE64; lsmt_amd.replay_log, log_line,
wal_bytes): the header's declarations, the library's exports, the ctypes
prototypes and the Python signatures; cb_log_line, the restatement
(tests/replay_ref.py) and the hand-worked cases (tests/replay_cases.py) held
against each other, then about 4000 mutated pieces; the same under the address
and undefined-behaviour sanitizers through a stand-alone driver
(tests/cpp/logline_driver.cpp); the writer's round trip; the argument refusals
that need no device; and, of the generated logs the device tests replay, that
they hold what they are for.
"""
import base64
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

import replay_ref as ref
import store_model as sm
from replay_cases import CASES, HOT, LINES, TOMBSTONE, generated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL, CB_EZEROM, CB_EUTF8, CB_EBASE64 = 0, -1, -2, -7, -8

SYMBOLS = {
    "cb_log_replay": ["log", "len", "m_bits", "device", "stream", "table_out", "bloom_out", "stats"],
    "cb_log_line": ["piece", "len", "kind", "key_len", "value_len"],
}
STATS_FIELDS = ["lines", "entries", "keys", "bad_line", "bad_offset"]
EMPTY = inspect.Parameter.empty


# ---- the surface ------------------------------------------------------------------------

def test_surface():
    """Header, library, ctypes, documents and Python entry points in one: the
    test that cannot pass before the replay exists."""
    import lsmt_amd
    from lsmt_amd import _lib
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        raw_header = fh.read()
    header = re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S)
    L = _lib.load()
    for name, names in SYMBOLS.items():
        assert name in _lib.header_symbols()
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name}: no prototype"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        fn = getattr(L, name)  # (raises if the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params)
        assert fn.restype is ctypes.c_int
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*cb_log_stats\s*;", header)
    assert m, "no cb_log_stats"
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    assert [f[-1] for f in fields] == STATS_FIELDS and all(f[0] == "uint64_t" for f in fields)
    assert [n for n, _ in _lib.LogStats._fields_] == STATS_FIELDS and ctypes.sizeof(_lib.LogStats) == 40
    assert re.search(r"#define\s+CB_EBASE64\s+\(-8\)", header) and _lib.CB_EBASE64 == CB_EBASE64
    assert re.search(r"#define\s+CB_EUTF8\s+\(-7\)", header) and _lib.CB_EUTF8 == CB_EUTF8
    # the header's comments cite the reference's lines and name the rule's home
    section = raw_header[raw_header.index("the write-ahead log replayed"):raw_header.index("cb_log_line(")]
    for cite in ("src/wal.rs:14-31", "src/lib.rs:30-39", "src/lib.rs:96-102", "src/sstable.rs:51-87",
                 "tests/wal_error_test.rs:19", "logline.hpp"):
        assert cite in section, cite
    for name, params, defaults in (("replay_log", ["log", "m", "device", "stream"], [EMPTY, 1024, 0, None]),
                                   ("log_line", ["piece"], [EMPTY]), ("wal_bytes", ["entries"], [EMPTY])):
        assert name in lsmt_amd.__all__
        sig = inspect.signature(getattr(lsmt_amd, name))
        assert list(sig.parameters) == params and [p.default for p in sig.parameters.values()] == defaults, name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        integration = fh.read()
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, integration), name
    assert "Database::new" in integration and "cb_log_stats" in integration
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    for fn in ("replay.hip", "capi_replay.cpp", "replay.hpp", "logline.hpp"):
        assert re.search(r"\b%s\b" % re.escape(fn), make), fn


def test_the_rule_has_one_home():
    """logline.hpp states the split's verdict and the UTF-8 check once; the
    kernels and the host entry ask there; compaction's steps have one body."""
    code = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp", ".cpp")):
            with open(os.path.join(CSRC, fn)) as fh:
                code[fn] = re.sub(r"//[^\n]*", "", fh.read())
    defs = {fn: len(re.findall(r"\binline\s+bool\s+utf8_valid\s*\(", c)) for fn, c in code.items()}
    assert {fn: n for fn, n in defs.items() if n} == {"logline.hpp": 1}
    assert "utf8_valid(" in code["sstable.hip"] and '#include "logline.hpp"' in code["sstable.hip"]
    assert "hip_runtime" not in code["logline.hpp"]
    for fn in ("replay.hip", "capi_replay.cpp"):
        assert re.search(r"\blog_line(_at)?\s*\(", code[fn]), fn
    assert re.findall(r'ProfScope ps\("(\w+)"', code["replay.hip"]) == ["k_log_mark", "k_log_gather"]
    for fn in ("format_survivors", "finish_compacted"):
        bodies = [f for f, c in code.items() if re.search(r"\bint\s+%s\s*\([^;{]*\)\s*\{" % fn, c)]
        assert bodies == ["capi_merge.cpp"], (fn, bodies)
        assert re.search(r"\b%s\s*\(" % fn, code["capi_replay.cpp"]) and re.search(r"\b%s\s*\(" % fn, code["capi_merge.hpp"])


# ---- cb_log_line, the restatement and the hand-worked cases ------------------------------

def lib_log_line(piece: bytes):
    """cb_log_line through plain ctypes, the piece in a buffer of exactly its size."""
    from lsmt_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_uint8 * max(len(piece), 1)).from_buffer_copy(piece or b"\0")
    kind, kl, vl = ctypes.c_int(99), ctypes.c_uint64(99), ctypes.c_uint64(99)
    assert L.cb_log_line(buf, len(piece), ctypes.byref(kind), ctypes.byref(kl), ctypes.byref(vl)) == CB_OK
    return kind.value, kl.value, vl.value


def test_hand_worked_cases_agree():
    import lsmt_amd
    for piece, kind, kl, vl in LINES:
        assert ref.line_verdict(piece) == (kind, kl, vl), piece
        assert lib_log_line(piece) == (kind, kl, vl), piece
        assert lsmt_amd.log_line(piece) == (kind, kl, vl), piece
    for c in CASES:
        r = ref.Replay(c.log)
        assert (r.code, r.file, r.stats) == (c.code, c.file, c.stats), c.label
        # the library's verdict of every piece, folded as the restatement folds it
        rows, first = {}, None
        for i, (at, piece) in enumerate(ref.pieces(c.log)):
            kind, kl, vl = lib_log_line(piece)
            if kind < 0 and first is None:
                first = (kind, i, at)
            if kind == ref.ENTRY:
                rows[piece[:kl]] = base64.b64decode(piece[kl + 1:])
                assert len(rows[piece[:kl]]) == vl
        assert (first[0], first[1], first[2]) == (c.code, c.stats[3], c.stats[4]) if c.code else first is None, c.label
        if not c.code:
            assert rows == r.rows, c.label


def mutated_pieces(n=4000, seed=20):
    """Records of keys of one to four-byte UTF-8 sequences and values of every
    padding, a byte flipped, dropped or added in the key or in the base64 tail
    (never a newline: a piece holds none)."""
    rng = random.Random(seed)
    keys = [b"k", b"", b"key-%d", "é".encode(), "€uro".encode(), "\U0001F600!".encode(), b"\xed\x9f\xbf", b"\xef\xbf\xbd",
            b"\xf4\x8f\xbf\xbf", b"a\rb", b"0123456789abcdefXYZ"]
    out = []
    while len(out) < n:
        key = rng.choice(keys).replace(b"%d", b"%d" % rng.randrange(100))
        text = base64.b64encode(rng.randbytes(rng.randrange(0, 12)))
        piece = bytearray(key + b"\t" + text)
        how = rng.randrange(6)
        lo, hi = (0, len(key)) if how < 3 else (len(key) + 1, len(piece))
        if how == 5:
            lo = max(lo, len(piece) - 3)  # the tail's last quad: padding and trailing bits
        if lo < hi or how % 3 == 2:
            at = rng.randrange(lo, hi) if lo < hi else lo
            byte = rng.choice([rng.randrange(256), rng.choice(b"=AB+/\t\r \x80\xbf\xc0\xe0\xed\xf0\xf4\xff")])
            if how % 3 == 0:
                piece[at] = byte
            elif how % 3 == 1:
                del piece[at]
            else:
                piece.insert(at, byte)
        out.append(bytes(piece).replace(b"\n", b"\x0b"))
    return out


def test_mutated_pieces_agree():
    pieces = mutated_pieces()
    kinds = {}
    for p in pieces:
        want = ref.line_verdict(p)
        assert lib_log_line(p) == want, p
        kinds[want[0]] = kinds.get(want[0], 0) + 1
    # a property of the generator: every kind is well represented
    assert all(kinds.get(k, 0) > 300 for k in (ref.ENTRY, ref.EUTF8, ref.EBASE64)), kinds


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("logline") / "logline_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "logline_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def run_driver(driver, pieces):
    text = "".join("L %s\n" % (p.hex() or "-") for p in pieces)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(pieces)
    return got


def test_cases_and_mutations_under_sanitizers(driver):
    pieces = [p for p, _, _, _ in LINES] + [p for c in CASES for _, p in ref.pieces(c.log)] + mutated_pieces()
    for p, g in zip(pieces, run_driver(driver, pieces)):
        assert g == ref.line_verdict(p), p


# ---- the writer ------------------------------------------------------------------------

def test_writer_round_trip():
    import lsmt_amd
    rng = random.Random(3)
    entries = [("k", b"v"), (b"", b""), ("é", TOMBSTONE), (b"k", b"second"), (b"a|b", rng.randbytes(100)), ("k2", "text")]
    entries += [(b"%x" % rng.getrandbits(40), rng.randbytes(rng.randrange(0, 40))) for _ in range(300)]
    log = lsmt_amd.wal_bytes(entries)
    as_bytes = [(k.encode() if isinstance(k, str) else k, v.encode() if isinstance(v, str) else v) for k, v in entries]
    assert log == b"".join(k + b"\t" + base64.b64encode(v) + b"\n" for k, v in as_bytes)
    r = ref.Replay(log)
    assert r.code == 0 and r.rows == dict(as_bytes) and r.stats[:3] == (len(entries), len(entries), len(dict(as_bytes)))
    assert r.rows[b"k"] == b"second"
    assert [lsmt_amd.log_line(p)[0] for _, p in ref.pieces(log)] == [1] * len(entries)
    assert lsmt_amd.wal_bytes([]) == b""


# ---- refusals that need no device ---------------------------------------------------------

def test_argument_refusals_need_no_device():
    from lsmt_amd import _lib
    L = _lib.load()

    def last_error():
        return (L.cb_last_error() or b"").decode()

    log = np.frombuffer(b"k\tdg==\n", np.uint8).copy()
    st = _lib.LogStats(1, 2, 3, 4, 5)
    fh = ctypes.c_void_p(0xBEEF)
    # table_out NULL (the filter's output and the stats are cleared all the same)
    assert L.cb_log_replay(log.ctypes.data, len(log), 1024, 0, None, None, ctypes.byref(fh), ctypes.byref(st)) == CB_EINVAL
    assert last_error() == "null argument" and fh.value is None
    assert (st.lines, st.entries, st.keys, st.bad_line, st.bad_offset) == (0, 0, 0, ref.NONE, ref.NONE)
    # m_bits == 0 with a filter asked for: before the log is looked at (a null log with a length comes after)
    for ptr in (log.ctypes.data, None):
        th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xBEEF)
        assert L.cb_log_replay(ptr, len(log), 0, 0, None, ctypes.byref(th), ctypes.byref(fh), None) == CB_EZEROM
        assert "divisor of zero" in last_error() and th.value is None and fh.value is None
    # log NULL with len > 0
    th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xBEEF)
    assert L.cb_log_replay(None, 7, 1024, 0, None, ctypes.byref(th), ctypes.byref(fh), None) == CB_EINVAL
    assert "null log" in last_error() and th.value is None and fh.value is None
    th = ctypes.c_void_p(0xDEAD)
    assert L.cb_log_replay(None, 7, 0, 0, None, ctypes.byref(th), None, None) == CB_EINVAL and th.value is None
    import lsmt_amd
    with pytest.raises(ZeroDivisionError):
        lsmt_amd.replay_log(b"k\tdg==\n", m=0)
    # cb_log_line: null outputs, a null piece with a length, a newline in the piece
    kind = ctypes.c_int(99)
    assert L.cb_log_line(log.ctypes.data, len(log) - 1, None, None, None) == CB_EINVAL
    assert L.cb_log_line(None, 3, ctypes.byref(kind), None, None) == CB_EINVAL
    assert L.cb_log_line(log.ctypes.data, len(log), ctypes.byref(kind), None, None) == CB_EINVAL and "newline" in last_error()
    assert L.cb_log_line(None, 0, ctypes.byref(kind), None, None) == CB_OK and kind.value == 0
    assert L.cb_log_line(log.ctypes.data, len(log) - 1, ctypes.byref(kind), None, None) == CB_OK and kind.value == 1


# ---- the generated logs hold what they are for --------------------------------------------

TILE = 256                            # compact.hpp kCompactTile: records per select block
SORT_TILE = sm.BIN_SORT_SIZE - 1      # sort.hip: records per LDS tile; past it the bin sort


def sorted_records(log):
    """The entries as the merge sees them after its sort: by key, then newest first."""
    keys = [p.split(b"\t", 1)[0] for _, p in ref.pieces(log) if b"\t" in p]
    n = len(keys)
    return sorted(range(n), key=lambda e: (keys[e], n - 1 - e)), keys


def test_generated_logs_hold_their_conditions():
    logs = generated()
    assert list(generated().values()) == list(logs.values())  # deterministic
    for name in ("one key 300 times", "one key 300 times, a tombstone last"):
        order, keys = sorted_records(logs[name])
        run = [i for i, e in enumerate(order) if keys[e] == HOT]
        assert len(run) == 300 and run == list(range(run[0], run[0] + 300))
        assert run[0] < TILE < run[-1], "the run crosses the select's first tile edge"
        assert run[0] > 0 and run[-1] < len(order) - 1, "and has other keys on both sides"
        assert order[run[0]] == len(keys) - 1, "the record that stands is the log's last"
        r = ref.Replay(logs[name])
        assert (r.rows[HOT] == TOMBSTONE) == ("tombstone" in name) and len(r.rows) == 201
    for name, n in (("4096 entries", SORT_TILE), ("4097 entries", SORT_TILE + 1)):
        r = ref.Replay(logs[name])
        assert r.stats[:2] == (n, n) and r.stats[2] == n - 400, "exactly n entries, 400 of them second writes"
        assert sum(v.endswith(b"second") for v in r.rows.values()) == 400, "every second write stands"
        order, keys = sorted_records(logs[name])
        assert [keys[e] for e in order] != [keys[e] for e in range(n)], "the log is not in key order"
    order, keys = sorted_records(logs["5000 entries, 4500 of one key"])
    assert len(keys) == 5000 > SORT_TILE and keys.count(HOT) == 4500 > SORT_TILE, "one key's run exceeds a sort tile"
    mixed = logs["9000 mixed lines"]
    assert not mixed.endswith(b"\n") and b"\n\n" in mixed
    ps = [p for _, p in ref.pieces(mixed)]
    r = ref.Replay(mixed)
    assert r.code == 0 and len(ps) == 9000 and 8000 < r.stats[1] < 9000 and r.stats[2] < r.stats[1] // 2
    skipped = [p for p in ps if b"\t" not in p]
    assert any(not ref.oracle.utf8_valid(p) for p in skipped) and any(ref.oracle.utf8_valid(p) for p in skipped)
    ks = r.keys
    assert b"" in ks and any(len(k) > 16 for k in ks) and any(not k.isascii() for k in ks) and b"k\r" in ks
    assert any(len(a) > 16 and a[:16] == b[:16] for a, b in zip(ks, ks[1:])), "long keys that share their first 16 bytes"
    assert any(b.startswith(a) and a for a, b in zip(ks, ks[1:])), "a key that is a prefix of the next"
    assert any(v == TOMBSTONE for v in r.rows.values()) and any(v == b"" for v in r.rows.values())
