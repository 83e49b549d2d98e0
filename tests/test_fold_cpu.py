"""The coordinator's read merge without a GPU (cb_replies_fold with device -1,
cb_reply_line; lsmt_amd.replies): the surface; the restatement in
tests/fold_ref.py against the hand-worked cases of tests/fold_cases.py; the
host fold and cb_reply_line against both, and against fold_ref.py over seeded
mutations of valid replies; the refusals, which touch no device; the rule
(lsmt_amd/csrc/replyline.hpp, replyfold.hpp) under the address and
undefined-behaviour sanitizers through a stand-alone driver
(tests/cpp/replyline_driver.cpp); and the one-home checks of the new sources.
"""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fold_cases
import fold_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CB_OK, CB_EINVAL, CB_EUTF8 = 0, -1, -7
STATS = ("replies", "lines", "entries", "others", "keys", "with_text", "dead", "host_rows", "bytes", "bad_reply",
         "bad_offset")

# name -> parameter names, as include/cassbloom.h declares them
SYMBOLS = {
    "cb_replies_fold": ["bytes", "off", "nr", "device", "stream", "out", "stats"],
    "cb_fold_info": ["fold", "stats"],
    "cb_fold_text": ["fold", "text"],
    "cb_fold_rows": ["fold", "key_at", "key_len", "ts", "val_at", "val_len", "reply", "flags"],
    "cb_fold_other": ["fold", "at", "len"],
    "cb_fold_destroy": ["fold"],
    "cb_reply_line": ["piece", "len", "terminated", "kind", "key_len", "ts", "val_at", "val_len", "val_flags"],
}


def test_surface():
    """Header, ctypes, integration document and Python entry points in one: the
    test that cannot pass before the fold exists."""
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
    assert raw_header.index("cb_log_line(") < raw_header.index("cb_replies_fold(")
    assert "cb_fold*" not in header and "cb_fold_stats*" not in header  # struct arguments are void*
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*cb_fold_stats\s*;", header)
    assert m and re.findall(r"uint64_t\s+(\w+)\s*;", m.group(1)) == list(STATS)
    assert [n for n, _ in _lib.FoldStats._fields_] == list(STATS)
    for flag, value in (("CB_FOLD_TEXT", 1), ("CB_FOLD_DEAD", 2), ("CB_FOLD_HOST", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), raw_header), flag
    with open(os.path.join(CSRC, "replyline.hpp")) as fh:
        rule = fh.read()
    assert "src/cluster.rs:394-473" in raw_header and "src/cluster.rs:394-473" in rule
    assert re.search(r"NOT\s+run\s+against\s+the\s+reference", rule)
    for fn in ("replyline.hpp", "replyfold.hpp"):  # no HIP dependency: the driver builds them with a host compiler
        with open(os.path.join(CSRC, fn)) as fh:
            assert "hip_runtime" not in fh.read(), fn
    # the Python surface: reached as lsmt_amd.replies, nothing added to the package's own
    import lsmt_amd.replies as replies
    with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as fh:
        assert sorted(lsmt_amd.__all__) == sorted(json.load(fh))
    assert not hasattr(replies, "__all__")
    sig = lambda f: [(k, p.default) for k, p in inspect.signature(f).parameters.items()]  # noqa: E731
    E = inspect.Parameter.empty
    assert sig(replies.fold_replies) == [("replies", E), ("device", 0), ("stream", None)]
    assert sig(replies.reply_line) == [("piece", E), ("terminated", True)]
    for name in ("text", "rows", "other", "close"):
        assert callable(getattr(replies.FoldResult, name)), name
    assert (replies.FOLD_TEXT, replies.FOLD_DEAD, replies.FOLD_HOST) == (fold_ref.TEXT, fold_ref.DEAD, fold_ref.HOST)
    assert re.search(r"kFoldMaxReplies\s*=\s*%d\s*;" % replies.MAX_REPLIES, rule)


def test_imports_alone():
    """lsmt_amd.replies imports first in a fresh process."""
    r = subprocess.run([os.sys.executable, "-c", "import lsmt_amd.replies as r; print(r.FoldResult.__name__)"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "FoldResult", r.stderr[-2000:]


# ---- the restatement against the hand-worked cases ------------------------------------

def expected(c):
    """A case's expectation in fold_ref's shape: (code, stats, text, rows, other)."""
    joined = b"".join(c["replies"])
    if c["text"] is None:
        st = dict.fromkeys(STATS, 0)
        st.update(replies=len(c["replies"]), bad_reply=c["bad"][0], bad_offset=c["bad"][1])
        return CB_EUTF8, st, None, [], None
    rows, at_of = [], {}
    base = np.cumsum([0] + [len(r) for r in c["replies"]]).tolist()
    for key, ts, val, reply, flags in c["rows"]:
        # the winner's line: a line of its reply that begins with key \t and ends with \t val
        hits = [base[reply] + s for s, piece, term in fold_ref.lines_of(c["replies"][reply])
                if piece.startswith(key + b"\t") and fold_ref.line_of(piece, term)[2] == ts
                and (piece[:-1] if term and piece.endswith(b"\r") else piece).endswith(b"\t" + val)]
        assert hits, (c["name"], key)
        at = hits[0]
        val_at = joined.index(b"\t", joined.index(b"\t", at) + 1) + 1
        assert joined[val_at:val_at + len(val)] == val
        rows.append((at, len(key), ts, val_at, len(val), reply, flags))
    lines, entries, others = c["counts"]
    fl = [r[6] for r in rows]
    st = dict(replies=len(c["replies"]), lines=lines, entries=entries, others=others, keys=len(rows),
              with_text=fl.count(fold_cases.T), dead=fl.count(fold_cases.D), host_rows=fl.count(fold_cases.H),
              bytes=len(c["text"]), bad_reply=fold_ref.NONE, bad_offset=fold_ref.NONE)
    return 0, st, c["text"], rows, c["other"]


def test_case_names_are_unique():
    names = [c["name"] for c in fold_cases.CASES]
    assert len(names) == len(set(names)) and len(names) >= 70


@pytest.mark.parametrize("c", fold_cases.CASES, ids=lambda c: c["name"])
def test_ref_on_the_cases(c):
    code, st, text, rows, other = expected(c)
    f = fold_ref.fold(c["replies"])
    assert (f.code, f.stats, f.text, f.rows, f.other) == (code, st, text, rows, other)


def test_ref_on_the_lines():
    for (piece, term), want in fold_cases.LINES:
        assert fold_ref.line_of(piece, term) == want, (piece, term)


def test_ref_canonical_check_against_json():
    """TEXT means exactly: parsing and re-serialising as serde_json does
    (sorted names, its escapes, no spaces) gives the bytes back."""
    def reserialised(val):
        try:
            doc = json.loads(val.decode())
        except ValueError:
            return None
        if not isinstance(doc, dict) or not all(isinstance(v, str) for v in doc.values()):
            return None
        pairs = list(json.JSONDecoder(object_pairs_hook=list).decode(val.decode()))
        if len({k for k, _ in pairs}) != len(pairs):
            return None  # (a repeated name loses a pair on the way)

        def esc(s):
            out = []
            for ch in s:
                o = ord(ch)
                short = {0x22: '\\"', 0x5C: "\\\\", 8: "\\b", 12: "\\f", 10: "\\n", 13: "\\r", 9: "\\t"}
                out.append(short.get(o) or ("\\u%04x" % o if o < 0x20 else ch))
            return '"' + "".join(out) + '"'
        items = sorted(doc.items(), key=lambda kv: kv[0].encode())
        return ("{" + ",".join(esc(k) + ":" + esc(v) for k, v in items) + "}").encode()
    vals = [r[2] for c in fold_cases.CASES for r in c["rows"] if r[2]]
    assert len(vals) > 60
    for val in vals:
        if b"\\ud800" in val:
            continue  # (Python's json takes a lone surrogate; serde_json does not)
        assert (fold_ref.val_flags(val) == fold_ref.TEXT) == (reserialised(val) == val), val


# ---- the host entries -----------------------------------------------------------------

def host_fold(replies):
    """(code, stats, text, rows, other) of cb_replies_fold with device -1."""
    from lsmt_amd import replies as rp
    try:
        f = rp.fold_replies(replies, device=-1)
    except UnicodeDecodeError as e:
        assert e.code == CB_EUTF8
        return CB_EUTF8, {n: getattr(e.stats, n) for n in STATS}, None, [], None
    out = (0, {n: getattr(f.stats, n) for n in STATS}, f.text(), [tuple(r) for r in f.rows()], f.other())
    f.close()
    return out


def ref_fold(replies):
    f = fold_ref.fold(replies)
    return f.code, f.stats, f.text, f.rows, f.other


@pytest.mark.parametrize("c", fold_cases.CASES, ids=lambda c: c["name"])
def test_host_fold_on_the_cases(c):
    assert host_fold(c["replies"]) == expected(c)


def test_reply_line_on_the_lines():
    from lsmt_amd import _lib, replies as rp
    for (piece, term), want in fold_cases.LINES:
        assert tuple(rp.reply_line(piece, term)) == want, (piece, term)
    # every piece of every case, both ways
    for c in fold_cases.CASES:
        for reply in c["replies"]:
            for _, piece, term in fold_ref.lines_of(reply):
                for t in (term, not term):
                    assert tuple(rp.reply_line(piece, t)) == fold_ref.line_of(piece, t), (piece, t)
    L = _lib.load()
    kind = ctypes.c_int(99)
    assert L.cb_reply_line(b"a\nb", 3, 1, ctypes.byref(kind), None, None, None, None, None) == CB_EINVAL
    assert L.cb_reply_line(b"ab", 2, 1, None, None, None, None, None, None) == CB_EINVAL
    assert L.cb_reply_line(None, 2, 1, ctypes.byref(kind), None, None, None, None, None) == CB_EINVAL
    assert L.cb_reply_line(None, 0, 1, ctypes.byref(kind), None, None, None, None, None) == CB_OK and kind.value == 0


def valid_replies(rng, nr, rows):
    """Replies of this library's own shape: canonical objects, decimal
    timestamps, some dead rows, repeated keys, CRLF and unterminated ends."""
    out = []
    for r in range(nr):
        lines = []
        for _ in range(rows):
            key = b"k%d" % rng.integers(0, rows)
            ts = int(rng.integers(0, 6))
            cols = sorted(set(rng.choice([b"a", b"b", b"c\\n", b"d"], int(rng.integers(0, 4))).tolist()))
            val = b"" if rng.random() < 0.15 else b"{" + b",".join(b'"%s":"%d"' % (c, ts) for c in cols) + b"}"
            lines.append(key + b"\t%d\t" % ts + val + (b"\r" if rng.random() < 0.2 else b""))
        text = b"\n".join(lines)
        out.append(text + (b"\n" if rng.random() < 0.7 else b""))
    return out


def mutations(seed, count):
    rng = np.random.default_rng(seed)
    alphabet = list(b'\t\n\r"\\{}:,+-0159 /u\x7f\x80\xc3\xa9\xff\x00\x1f')
    for i in range(count):
        replies = valid_replies(rng, int(rng.integers(1, 5)), int(rng.integers(1, 7)))
        for _ in range(int(rng.integers(1, 4))):
            r = int(rng.integers(0, len(replies)))
            b = bytearray(replies[r])
            at = int(rng.integers(0, len(b) + 1))
            how = int(rng.integers(0, 3))
            if how == 0 and at < len(b):
                b[at] = int(rng.choice(alphabet))  # a byte flipped
            elif how == 1:
                b.insert(at, int(rng.choice(alphabet)))  # inserted
            elif at < len(b):
                del b[at]  # dropped
            replies[r] = bytes(b)
        yield replies


def test_host_fold_on_mutations():
    n = kinds = 0
    seen = set()
    for replies in mutations(20, 3000):
        want = ref_fold(replies)
        assert host_fold(replies) == want, replies
        n += 1
        seen.add((want[0], bool(want[4]), want[1]["host_rows"] > 0, want[1]["dead"] > 0))
        kinds = len(seen)
    assert n == 3000 and kinds >= 5  # (errors, others, host rows and dead rows all occur)


def test_unmutated_replies_need_no_host():
    rng = np.random.default_rng(3)
    for _ in range(50):
        replies = valid_replies(rng, 3, 8)
        replies = [r if r.endswith(b"\n") or not r.endswith(b"\r") else r + b"\n" for r in replies]
        code, st, text, rows, _ = host_fold(replies)
        assert code == 0 and st["host_rows"] == 0 and (code, st, text, rows, None) == ref_fold(replies)
        assert json.loads(text.decode()) is not None


# ---- refusals ---------------------------------------------------------------------------

def last_error(L):
    msg = L.cb_last_error()
    return msg.decode() if msg else ""


@pytest.mark.parametrize("device", [-1, 0])
def test_refusals_touch_no_device(device):
    """Every refusal the arguments alone decide, for the host fold and for a
    device: *out is cleared and the stats say nothing. (A piece of 4 GiB and
    2^32 entries need 4 GiB of replies and more: no test builds them.)"""
    from lsmt_amd import _lib
    L = _lib.load()

    def fold(data, off, nr=None, null=(), want_out=True):
        off = np.array(off, np.uint64)
        out, st = ctypes.c_void_p(0xDEAD), _lib.FoldStats()
        rc = L.cb_replies_fold(None if "bytes" in null else data + b"\0", None if "off" in null else off.ctypes.data,
                               len(off) - 1 if nr is None else nr, device, None,
                               ctypes.byref(out) if want_out else None, ctypes.byref(st))
        return rc, out.value, st

    rc, out, st = fold(b"ab", [0, 2], want_out=False)
    assert rc == CB_EINVAL and last_error(L) == "null argument"
    rc, out, st = fold(b"ab", [0, 2], null=("off",))
    assert (rc, out) == (CB_EINVAL, None) and "offsets" in last_error(L)
    rc, out, st = fold(b"ab", [0, 2], null=("bytes",))
    assert (rc, out) == (CB_EINVAL, None) and "null replies" in last_error(L)
    rc, out, st = fold(b"abc", [0, 2, 1])
    assert (rc, out) == (CB_EINVAL, None) and "decrease" in last_error(L)
    rc, out, st = fold(b"", [0] * 4098)
    assert (rc, out) == (CB_EINVAL, None) and "4096" in last_error(L)
    assert (st.keys, st.bytes, st.bad_reply, st.bad_offset) == (0, 0, fold_ref.NONE, fold_ref.NONE)
    assert L.cb_replies_fold(b"a", np.zeros(2, np.uint64).ctypes.data, 1, -2, None, ctypes.byref(ctypes.c_void_p()),
                             None) == CB_EINVAL
    # nothing to fold needs no device either: a valid object whose text is []
    for data, off, null in ((b"", [0], ()), (b"", [0], ("bytes", "off")), (b"", [0, 0, 0], ("bytes",)),
                            (b"xyz", [2, 2, 2], ())):
        rc, out, st = fold(data, off, null=null)
        assert rc == CB_OK and out, (data, off)
        text = np.zeros(2, np.uint8)
        assert L.cb_fold_text(out, text.ctypes.data) == CB_OK and text.tobytes() == b"[]"
        got = _lib.FoldStats()
        assert L.cb_fold_info(out, ctypes.byref(got)) == CB_OK
        assert (got.replies, got.bytes, got.keys, got.bad_reply) == (len(off) - 1, 2, 0, fold_ref.NONE)
        assert L.cb_fold_rows(out, None, None, None, None, None, None, None) == CB_OK
        at, ln = ctypes.c_uint64(1), ctypes.c_uint64(1)
        assert L.cb_fold_other(out, ctypes.byref(at), ctypes.byref(ln)) == CB_OK
        assert (at.value, ln.value) == (fold_ref.NONE, 0)
        assert L.cb_fold_destroy(out) == CB_OK
    # the handle's entries
    assert L.cb_fold_info(None, None) == CB_EINVAL and L.cb_fold_text(None, None) == CB_EINVAL
    assert L.cb_fold_rows(None, None, None, None, None, None, None, None) == CB_EINVAL
    assert L.cb_fold_other(None, None, None) == CB_EINVAL and L.cb_fold_destroy(None) == CB_OK


def test_offsets_need_not_begin_at_zero():
    from lsmt_amd import _lib
    L = _lib.load()
    data = b"junk" + b"a\t1\t{}\n" + b"a\t2\t{\"x\":\"y\"}" + b"tail"
    off = np.array([4, 11, 24], np.uint64)
    out = ctypes.c_void_p()
    assert L.cb_replies_fold(data, off.ctypes.data, 2, -1, None, ctypes.byref(out), None) == CB_OK
    st = _lib.FoldStats()
    L.cb_fold_info(out, ctypes.byref(st))
    text, key_at, val_at, rp = np.zeros(st.bytes, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(
        1, np.uint32)
    L.cb_fold_text(out, text.ctypes.data)
    L.cb_fold_rows(out, key_at.ctypes.data, None, None, val_at.ctypes.data, None, rp.ctypes.data, None)
    assert text.tobytes() == b'[{"x":"y"}]' and (int(key_at[0]), int(val_at[0]), int(rp[0])) == (11, 15, 1)
    L.cb_fold_destroy(out)


def test_python_refusals():
    from lsmt_amd import replies as rp
    with pytest.raises(UnicodeDecodeError) as ei:
        rp.fold_replies([b"a\t1\t{}\n", b"\xff\n"], device=-1)
    assert (ei.value.code, ei.value.stats.bad_reply, ei.value.stats.bad_offset) == (CB_EUTF8, 1, 7)
    f = rp.fold_replies([], device=-1)
    assert f.text() == b"[]" and f.rows() == [] and f.other() is None
    f.close()
    f.close()


# ---- the rule under the sanitizers ------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fold") / "replyline_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "replyline_driver.cpp"),
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


def driver_fold(line):
    rc, stats, text, other, rows = [x.strip() for x in line.split("|")]
    st = dict(zip(STATS, map(int, stats.split())))
    oa, ol = map(int, other.split())
    rows = [tuple(map(int, r.split(":"))) for r in rows.split()]
    if int(rc):
        return int(rc), st, None, [], None
    return 0, st, b"" if text == "-" else bytes.fromhex(text), rows, None if oa == fold_ref.NONE else (oa, ol)


def test_lines_under_sanitizers(driver):
    pieces = [(p, t) for (p, t), _ in fold_cases.LINES]
    pieces += [(piece, t) for c in fold_cases.CASES for reply in c["replies"]
               for _, piece, term in fold_ref.lines_of(reply) for t in (term, not term)]
    got = run_driver(driver, ["L %d %s" % (t, hx(p)) for p, t in pieces])
    for (p, t), line in zip(pieces, got):
        assert tuple(map(int, line.split())) == fold_ref.line_of(p, t), (p, t)


def test_folds_under_sanitizers(driver):
    folds = [c["replies"] for c in fold_cases.CASES] + list(mutations(21, 600))
    got = run_driver(driver, [("F " + " ".join(hx(r) for r in replies)).strip() for replies in folds])
    for replies, line in zip(folds, got):
        assert driver_fold(line) == ref_fold(replies), replies
    for c, line in zip(fold_cases.CASES, got):
        assert driver_fold(line) == expected(c), c["name"]


# ---- one home ---------------------------------------------------------------------------

def test_the_fold_has_one_home():
    new_files = ["lsmt_amd/csrc/replyline.hpp", "lsmt_amd/csrc/replyfold.hpp", "lsmt_amd/csrc/fold.hpp",
                 "lsmt_amd/csrc/fold.hip", "lsmt_amd/csrc/capi_fold.cpp", "lsmt_amd/replies.py",
                 "tests/cpp/replyline_driver.cpp", "tests/test_fold_gpu.py", "tools/ubench_fold.py"]
    text = {}
    for fn in new_files:
        with open(os.path.join(ROOT, fn)) as fh:
            text[fn] = re.sub(r"//[^\n]*", "", fh.read())
    hip = text["lsmt_amd/csrc/fold.hip"]
    for kernel in ("k_reply_mark", "k_reply_gather", "k_fold_size", "k_fold_write"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, hip), kernel
    # the cuts, the strip, the timestamp and the canonical walk are written once, in replyline.hpp
    rule = text["lsmt_amd/csrc/replyline.hpp"]
    for fn_name in ("reply_strip", "reply_ts", "reply_line_at", "canon_string_end", "reply_val_flags"):
        assert len(re.findall(r"inline\s+\w+\s+%s\s*\(" % fn_name, rule)) == 1, fn_name
    for fn, src in text.items():
        if fn.endswith((".hip", ".cpp", ".hpp")) and fn != "lsmt_amd/csrc/replyline.hpp":
            assert "'\\r'" not in src, fn            # no second strip
            assert "'\\t'" not in src, fn            # no second cut at the TABs
            assert not re.search(r"\* 10\b", src), fn  # no second decimal parse
            assert "'\"'" not in src, fn             # no second walk of a string
    # the fold is rowts.hpp's and UTF-8 is logline.hpp's
    assert "lww_replaces(" in text["lsmt_amd/csrc/replyfold.hpp"] and "utf8_valid(" in rule
    assert not re.search(r"\bts_a\b|0xC2|0xED", rule)
    users = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".hip", ".hpp", ".cpp"))
             and re.search(r"\blww_(beats|replaces)\s*\(", re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, fn)).read()))]
    assert users == ["compact.hip", "replyfold.hpp", "rowts.hpp"]
    with open(os.path.join(CSRC, "rowts.hpp")) as fh:
        assert re.search(r"lww_replaces\([^)]*\)\s*\{\s*return\s+lww_beats\(ts, idx, kept_ts, kept_idx\);", fh.read())
    # the device fold runs the merge as it stands and parses no base64 timestamp
    capi = text["lsmt_amd/csrc/capi_fold.cpp"]
    for step in ("merge_alloc(", "enqueue_sort_begin(", "enqueue_key_sort(", "launch_compact_select_lww("):
        assert step in capi, step
    assert "launch_compact_ts" not in capi and "value_ts" not in hip
    # existing kernels are as they were: the tile sums still have one body and its three callers
    with open(os.path.join(CSRC, "compact.hip")) as fh:
        compact = re.sub(r"//[^\n]*", "", fh.read())
    assert len(re.findall(r"\bput_tile_sums\s*\(", compact)) == 3
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    for fn in ("fold.hip", "capi_fold.cpp", "fold.hpp", "replyline.hpp", "replyfold.hpp"):
        assert re.search(r"\b%s\b" % re.escape(fn), make), fn
