"""cb_replies_fold on the device: the coordinator's read merge
(src/cluster.rs:394-473) over the replicas' `key \\t ts \\t val` replies.

The oracle is tests/fold_ref.py, the rule's plain restatement; the host fold
(device -1) is a second witness. Every comparison is exact: the response, the
stats, every winner's place in the folded bytes, its timestamp, reply and
flag, and the least other line.

Shapes come from the kernels' edges: kCompactTile = 256 records (255, 256, 257
entries; a run of one key across a tile edge), kLineChunk = 4096 bytes (a
piece's end, a TAB, and a CRLF on the edge; a piece over two chunks), one long
val among short ones, all entries one key, all keys distinct, and one random
case of 20 000 lines. The end-to-end test closes the read path: scan and
select META on each of four replica tables, fold, and compare with
cb_scan_select(JSON) over cb_tables_scan_lww of the four tables.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import fold_cases
import fold_ref
import rowselect_ref as ref
from merge_help import ALL, b64, open_tables, raw_file, TILE
from test_fold_cpu import CB_EUTF8, STATS, expected, ref_fold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
CHUNK = 4096  # sstable.hpp kLineChunk
assert TILE == 256


def fold_on(gpu, replies, device, on_device=False, stream=None):
    """(code, stats, text, rows, other) of fold_replies: device -1 the host
    fold; on_device: the replies as uint8 device tensors."""
    from lsmt_amd import replies as rp
    src = replies
    if on_device:
        import torch
        src = [torch.from_numpy(np.frombuffer(r, np.uint8).copy()).cuda() if r else
               torch.empty(0, dtype=torch.uint8, device="cuda") for r in replies]
    try:
        f = rp.fold_replies(src, device=device, stream=stream)
    except UnicodeDecodeError as e:
        assert e.code == CB_EUTF8
        return CB_EUTF8, {n: getattr(e.stats, n) for n in STATS}, None, [], None
    out = (0, {n: getattr(f.stats, n) for n in STATS}, f.text(), [tuple(r) for r in f.rows()], f.other())
    f.close()
    return out


def check(gpu, replies, want=None):
    """The device fold of replies in host and in device memory, and the host
    fold, against the restatement. Returns the restatement's answer."""
    want = want or ref_fold(replies)
    assert fold_on(gpu, replies, 0) == want
    assert fold_on(gpu, replies, 0, on_device=True) == want
    assert fold_on(gpu, replies, -1) == want
    code, st, text, rows, other = want
    joined = b"".join(replies)
    base = np.cumsum([0] + [len(r) for r in replies]).tolist()
    for key_at, key_len, ts, val_at, val_len, reply, flags in rows:  # the spans cut from the caller's bytes
        assert base[reply] <= key_at and val_at + val_len <= base[reply + 1]
        assert joined[key_at + key_len:key_at + key_len + 1] == b"\t" and joined[val_at - 1:val_at] == b"\t"
    return want


# ---- the hand-worked cases ------------------------------------------------------------

@pytest.mark.parametrize("c", fold_cases.CASES, ids=lambda c: c["name"])
def test_the_cases_on_the_device(gpu, c):
    check(gpu, c["replies"], expected(c))


def test_device_outputs(gpu):
    """cb_fold_text and cb_fold_rows into device memory."""
    import torch
    from lsmt_amd import replies as rp
    replies = [b"b\t2\t{\"x\":\"1\"}\na\t1\t\n", b"a\t3\t{}\nc\t1\t{\"x\":1}\n"]
    f = rp.fold_replies(replies)
    n = int(f.stats.keys)
    assert n == 3 and f.text() == b'[{},{"x":"1"}]'
    text = torch.full((int(f.stats.bytes),), 0xAD, dtype=torch.uint8, device="cuda")
    u64 = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(5)]
    rp_, fl = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    f.copy(text, *u64, rp_, fl)
    assert text.cpu().numpy().tobytes() == f.text()
    got = list(zip(*(t.cpu().numpy().tolist() for t in u64), rp_.cpu().numpy().tolist(), fl.cpu().numpy().tolist()))
    assert got == [tuple(r) for r in f.rows()] == ref_fold(replies)[3]
    assert [r.flags for r in f.rows()] == [fold_ref.TEXT, fold_ref.TEXT, fold_ref.HOST]


# ---- the kernels' edges ---------------------------------------------------------------

def entry(key, ts, val=b"{}"):
    return key + b"\t%d\t" % ts + val + b"\n"


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_entry_counts_around_one_tile(gpu, n):
    lines = [entry(b"k%05d" % ((i * 7919) % n), i, b'{"i":"%d"}' % i if i % 5 else b"") for i in range(n)]
    code, st, text, rows, _ = check(gpu, [b"".join(lines[:n // 3]), b"".join(lines[n // 3:])])
    assert st["keys"] == st["entries"] == n and st["dead"] == (n + 4) // 5


@pytest.mark.parametrize("run", [3, 16, 300])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_run_of_one_key_across_a_tile_edge(gpu, run, where):
    """TILE - 2 keys sort before the run's key, so its entries lie on both
    sides of the first tile's edge; the winner is its first, a middle or its
    last entry, the others share a lower timestamp (ties: the first met)."""
    win = {"first": 0, "middle": run // 2, "last": run - 1}[where]
    before = [entry(b"a%04d" % i, 1) for i in range(TILE - 2)]
    after = [entry(b"z%04d" % i, 1) for i in range(40)]
    ones = [entry(b"m", 9 if i == win else 5, b'{"i":"%d"}' % i) for i in range(run)]
    replies = [b"".join(after[:20] + ones[:run // 2]), b"".join(before), b"".join(ones[run // 2:] + after[20:])]
    code, st, text, rows, _ = check(gpu, replies)
    assert st["keys"] == TILE - 2 + 1 + 40 and b'{"i":"%d"}' % win in text and text.count(b'"i"') == 1
    # every timestamp equal: the first met wins, wherever the run lies
    ones = [entry(b"m", 5, b'{"i":"%d"}' % i) for i in range(run)]
    code, st, text, rows, _ = check(gpu, [b"".join(before[:100]), b"".join(ones + before[100:] + after)])
    assert b'{"i":"0"}' in text and text.count(b'"i"') == 1


@pytest.mark.parametrize("edge", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK])
@pytest.mark.parametrize("what", ["newline", "tab1", "tab2", "crlf"])
def test_a_piece_on_a_chunk_edge(gpu, what, edge):
    """The line index reads the staged replies in chunks of 4096 bytes: the
    byte that ends a piece, either TAB and the CR of a CRLF each at the last
    byte of a chunk, the first of the next and beside them."""
    line = b"key\t77\t{\"a\":\"b\"}" + (b"\r" if what == "crlf" else b"")
    at = {"newline": len(line), "tab1": 3, "tab2": 6, "crlf": len(line) - 1}[what]
    pad = edge - at - len(b"f\t1\t{\"p\":\"\"}\n")
    filler = b"f\t1\t{\"p\":\"" + b"x" * pad + b"\"}\n"
    reply = filler + line + b"\n" + entry(b"tail", 2)
    assert (reply + b"\n")[edge:edge + 1] == {"newline": b"\n", "tab1": b"\t", "tab2": b"\t", "crlf": b"\r"}[what]
    code, st, text, rows, _ = check(gpu, [reply, entry(b"key", 3, b'{"late":"r"}')])
    assert st["keys"] == 3 and st["host_rows"] == 0 and text.endswith(b',{"a":"b"},{}]')
    # the same reply second, behind an unterminated one: its staged bytes lie two separators further on
    check(gpu, [b"o\t1\t{}", reply, b"", reply[:-1]])


def test_a_piece_over_two_chunks_and_a_long_val_among_short_ones(gpu):
    long_val = b'{"a":"' + b"v\\n" * 2990 + b'"}'  # about 9000 bytes: a piece spanning three chunks
    mid_val = b'{"a":"' + b"w" * 3000 + b'","b":"c"}'
    lines = [entry(b"k%03d" % i, i, b'{"s":"%d"}' % i) for i in range(300)]
    lines[7] = entry(b"k007", 7, long_val)
    lines[150] = entry(b"k150", 150, mid_val)
    lines[151] = entry(b"k151", 151, mid_val[:-1])  # truncated: a long walk that ends in CB_FOLD_HOST
    code, st, text, rows, _ = check(gpu, [b"".join(lines[:100]), b"".join(lines[100:])])
    assert (st["keys"], st["with_text"], st["host_rows"]) == (300, 299, 1) and long_val in text and mid_val in text


def test_all_entries_one_key_and_all_keys_distinct(gpu):
    one = [entry(b"the-key", (i * 37) % 601, b'{"i":"%d"}' % i) for i in range(600)]
    code, st, text, rows, _ = check(gpu, [b"".join(one[:200]), b"".join(one[200:201]), b"".join(one[201:])])
    best = max(range(600), key=lambda i: ((i * 37) % 601, -i))
    assert (st["keys"], st["entries"]) == (1, 600) and text == b'[{"i":"%d"}]' % best
    distinct = [entry(b"%05d" % ((i * 7919) % 1000), 4, b'{"i":"%d"}' % i) for i in range(1000)]
    code, st, text, rows, _ = check(gpu, [b"".join(distinct[:1]), b"".join(distinct[1:])])
    assert st["keys"] == 1000 and [r[5] for r in rows].count(0) == 1


def test_twenty_thousand_lines_over_eight_replies(gpu):
    """30 % repeated keys, 10 % dead rows, some CRLF ends, a few others and
    vals for the host among them."""
    rng = np.random.default_rng(11)
    n = 20000
    keys = rng.integers(0, int(n * 0.7), n)
    ts = rng.integers(0, 50, n)
    lines = []
    for i in range(n):
        u = rng.random()
        val = b"" if u < 0.10 else b'{"a":1}' if u < 0.11 else b'{"a":"%d","k":"%d"}' % (i, keys[i])
        lines.append(b"key%07d\t%d\t" % (keys[i], ts[i]) + val + (b"\r\n" if i % 17 == 0 else b"\n"))
        if i % 4001 == 0:
            lines.append(b"count\t%d\n" % i)
    cut = sorted(rng.integers(0, len(lines), 7).tolist())
    replies = [b"".join(lines[a:b]) for a, b in zip([0] + cut, cut + [len(lines)])]
    code, st, text, rows, _ = check(gpu, replies)
    assert st["entries"] == n and st["others"] == 5 and st["keys"] == len(set(keys.tolist()))
    assert st["dead"] > 500 and st["host_rows"] > 50


def test_others_alone_on_the_device(gpu):
    """No entry: the least other line comes back from the device's pieces."""
    replies = [b"%d\n" % (1000 - i) for i in range(300)] + [b"1000000\r\n", b"\n"]
    code, st, text, rows, other = check(gpu, replies)
    assert text == b"1000" and st["others"] == 301 and other == (0, 4)


# ---- end to end: scan, select META on each replica, fold, response ---------------------

COLS, KC, CASTS = ["a", "b", "ck", "n", "pk"], ("pk", "ck"), {"n": 1}
PAYLOADS = [b'{"a":"1"}', b'{"b":"\\n\\u0001","a":"x\\"y"}', b'{"n":"+007","a":"\xc3\xa9\x7f"}', b"not json", b"{}",
            b'{"zz":"extra","a":"/"}', b'{"a":"1","a":"2"}', b' { "a" : "sp" } ', b'{"a":"\\u00e9\\ud83d\\ude00"}']


def replica_files(prefixes, per_prefix):
    """Four replicas' files over the same keys: shuffled timestamps, equal
    timestamps on some keys, tombstones, keys missing on some replicas, UTF-8
    keys; lines = per replica {key: value}."""
    rng = np.random.default_rng(5)
    tails = ["u%04d|c%d", "é%04d|ü%d", "k%04d|\r%d", "q%04d%d"]
    lines = [dict() for _ in range(4)]
    for p in prefixes:
        for i in range(per_prefix):
            key = p + (tails[i % 4] % (i, i % 3)).encode()
            same = i % 11 == 0
            for r in range(4):
                if rng.random() < 0.25:
                    continue  # this replica never got the row
                ts = 100 + i if same else int(rng.integers(1, 1000))
                dead = rng.random() < 0.15
                payload = b"" if dead else PAYLOADS[int(rng.integers(0, len(PAYLOADS)))] if i % 3 else (
                    b'{"a":"r%d","n":"%d"}' % (r, i))
                lines[r][key] = ts.to_bytes(8, "big") + payload
    return lines


def winners_of(lines):
    """Last write wins over the replicas: the greatest timestamp, the first
    replica among equal ones."""
    best = {}
    for r, rows in enumerate(lines):
        for k, v in rows.items():
            t = int.from_bytes(v[:8], "big")
            if k not in best or t > best[k][0]:
                best[k] = (t, v)
    return {k: v for k, (t, v) in best.items()}


@pytest.mark.parametrize("nprefix", [0, 1, 16])
def test_the_read_path_closes(gpu, nprefix):
    from lsmt_amd import replies as rp
    prefixes = [b"t%02d:" % i for i in range(max(nprefix, 1))]
    lines = replica_files(prefixes, 2000 // len(prefixes))
    skip = 0 if nprefix == 16 else 4  # (with several namespaces in one answer the whole key is the row's key)
    sel = ref.normalize(COLS, KC, CASTS)
    # the condition, on the references alone: every row the select writes is canonical
    metas = [ref.response([ref.row_text(k, v, sel, skip, True)[0] for k, v in sorted(rows.items())], True)
             for rows in lines]
    want = fold_ref.fold(metas)
    win = winners_of(lines)
    response = ref.response([ref.row_text(k, win[k], sel, skip, False)[0] for k in sorted(win)], False)
    assert want.code == 0 and want.stats["host_rows"] == 0 and want.text == response
    assert want.stats["keys"] == len(win) and want.stats["dead"] > 50 and want.stats["entries"] > 1.5 * len(win)
    # on the device
    tables = open_tables(gpu, [raw_file(sorted((k, b64(v)) for k, v in rows.items())) for rows in lines])
    scan_of = {0: lambda ts: gpu.scan(ts), 1: lambda ts: gpu.scan(ts, prefix=prefixes[0]),
               16: lambda ts: gpu.scan_many(ts, prefixes=prefixes)}[nprefix]
    texts = [scan_of([t]).select(COLS, KC, CASTS, skip=skip, meta=True) for t in tables]  # left in device memory
    assert [t.text() for t in texts] == metas
    f = rp.fold_replies(texts)
    lww = {0: lambda: gpu.scan_lww(tables, ranges=ALL), 1: lambda: gpu.scan_lww(tables, prefixes=prefixes[:1]),
           16: lambda: gpu.scan_lww(tables, prefixes=prefixes)}[nprefix]()
    client = lww.select(COLS, KC, CASTS, skip=skip, meta=False)
    assert f.text() == client.text() == response
    assert f.stats.host_rows == 0 and {n: getattr(f.stats, n) for n in STATS} == want.stats
    assert [tuple(r) for r in f.rows()] == want.rows


# ---- launch lists ---------------------------------------------------------------------

def kernel_names():
    names = set()
    for fn in os.listdir(CSRC):
        if fn.endswith((".hip", ".cpp")):
            with open(os.path.join(CSRC, fn)) as fh:
                for m in re.finditer(r"ProfScope\s+\w+\(([^;]*?),\s*\w+\)\s*;", fh.read()):
                    names.update(re.findall(r'"(k_\w+)"', m.group(1)))
    return sorted(names)


def launch_list(gpu, fn):
    import torch
    L = gpu._lib.load()
    fn()  # (first use: buffers, the ring of events)
    torch.cuda.synchronize()
    L.cb_profile_enable(1)
    L.cb_profile_reset()
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for name in kernel_names():
            ms, n = ctypes.c_double(), ctypes.c_uint64()
            if L.cb_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value:
                out[name] = int(n.value)
    finally:
        L.cb_profile_enable(0)
    return out


REPLAY_1024 = {"k_line_count": 1, "k_scan_reduce": 3, "k_tile_scan": 6, "k_scan_apply": 3, "k_line_emit": 1,
               "k_line_finish": 1, "k_log_mark": 1, "k_log_gather": 1, "k_entry_sort": 1, "k_compact_select": 1,
               "k_compact_format": 1, "k_insert_lds": 1, "k_pfx_masks": 1, "k_table_dir": 1}
COMPACT_BINNED = {"k_compact_klen": 1, "k_scan_reduce": 1, "k_tile_scan": 4, "k_scan_apply": 1, "k_compact_gather": 1,
                  "k_entry_sort": 1, "k_bin_count": 1, "k_bin_offsets": 1, "k_bin_scatter": 1, "k_bin_sort": 1,
                  "k_compact_select": 1, "k_compact_format": 1, "k_insert_lds": 1, "k_pfx_masks": 1, "k_table_dir": 1}


def test_launch_lists(gpu):
    """The existing entries enqueue what they did (the lists profiles/replay_r18.json
    and profiles/lww_r13.json record): compaction 18 launches past the sort's
    4096-record tile, LWW compaction 20 (two more for the timestamps and the
    select's second half), the replay of a 1024-line log 23. And the fold's own
    list, which DESIGN.md 6.15 records."""
    assert len(kernel_names()) > 40 and "k_fold_write" in kernel_names()
    recs = [(b"%016x" % (i * 0x9E3779B97F4A7C15 % 2**64), (i).to_bytes(8, "big") + b"payload!") for i in range(1024)]
    log = gpu.wal_bytes(recs)
    got = launch_list(gpu, lambda: gpu.replay_log(log, m=1024))
    assert got == REPLAY_1024 and sum(got.values()) == 23
    tables = [gpu.sstable_create(sorted((b"%d:" % t + k, v) for k, v in recs), m=1024)[0] for t in range(5)]
    got = launch_list(gpu, lambda: gpu.compact(tables, m=1024))
    assert got == COMPACT_BINNED and sum(got.values()) == 18
    got = launch_list(gpu, lambda: gpu.compact_lww(tables, m=1024))
    want = dict(COMPACT_BINNED, k_compact_ts=1, k_compact_lww_runs=1, k_compact_lww_tiles=1)
    del want["k_compact_select"]
    assert got == want and sum(got.values()) == 20
    from lsmt_amd import replies as rp
    replies = [b"".join(entry(b"k%05d" % ((i * 31 + r) % 1500), i % 9, b'{"v":"%d"}' % i) for i in range(1024))
               for r in range(3)]
    got = launch_list(gpu, lambda: rp.fold_replies(replies))
    assert got == {"k_line_count": 1, "k_scan_reduce": 5, "k_tile_scan": 5, "k_scan_apply": 5, "k_line_emit": 1,
                   "k_line_finish": 1, "k_reply_mark": 1, "k_reply_gather": 1, "k_entry_sort": 1,
                   "k_compact_lww_runs": 1, "k_compact_lww_tiles": 1, "k_fold_size": 1, "k_fold_write": 1}, got


# ---- object lifetime -------------------------------------------------------------------

def test_a_result_outlives_its_inputs_and_its_stream(gpu):
    """Release, reuse and a second stream: the result stays readable after the
    replies are freed and after cb_stream_release of the calling stream."""
    import torch
    from lsmt_amd import replies as rp
    L = gpu._lib.load()
    replies = [b"".join(entry(b"k%04d" % ((i * 13 + r) % 700), (i * 7 + r) % 11, b'{"v":"%d.%d"}' % (r, i))
                        for i in range(600)) for r in range(3)]
    want = ref_fold(replies)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev = [torch.from_numpy(np.frombuffer(r, np.uint8).copy()).cuda() for r in replies]
    torch.cuda.synchronize()
    f1 = rp.fold_replies(dev, stream=s1)
    f2 = rp.fold_replies(replies, stream=s2)
    for t in dev:
        t.fill_(0x0A)  # the inputs change and go: the result keeps no reference to them
    del dev, t
    torch.cuda.synchronize()
    assert L.cb_stream_release(s1.cuda_stream) == 0
    for f in (f1, f2):
        assert (f.text(), [tuple(r) for r in f.rows()]) == (want[2], want[3])
    f1.close()
    f1.close()
    # the released blocks are reused by the next folds, on either stream, and the answers stay right
    for i in range(6):
        f = rp.fold_replies(replies[i % 3:] + replies[:i % 3], stream=(s1, s2)[i % 2])
        assert f.text() == ref_fold(replies[i % 3:] + replies[:i % 3])[2]
        if i % 2:
            f.close()
    assert f2.text() == want[2]
    assert L.cb_stream_release(s2.cuda_stream) == 0
    assert f2.text() == want[2] and {n: getattr(f2.stats, n) for n in STATS} == want[1]
