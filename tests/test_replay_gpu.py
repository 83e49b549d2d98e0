"""cb_log_replay on the device against the plain restatement (replay_ref.py),
the hand-worked logs (replay_cases.py) and SsTable::create on the device of
the deduplicated entries: the file's bytes, its form, the line count, the
filter's bits, the zone bounds, the stats and every get, for each of the
shapes at which a step of the replay can go wrong. Errors: the code, cleared
outputs and the first bad piece's line and offset. One short store history
beside tests/store_model.py's model adopts a replayed log as the newest table.
"""
import ctypes

import numpy as np
import pytest

import replay_ref as ref
import store_model as sm
from liverow_ref import is_dead
from merge_help import ALL, absent_keys, ragged
from oracle import oracle
from replay_cases import CASES, HOT, TOMBSTONE, generated, record, stamped

pytestmark = pytest.mark.gpu

M = 1024
GENERATED = generated()  # built once, shared
WANT = {}                # name -> Replay, computed once


def want_of(name, log):
    if name not in WANT:
        WANT[name] = ref.Replay(log)
    return WANT[name]


def stats_tuple(st):
    return (st.lines, st.entries, st.keys, st.bad_line, st.bad_offset)


def check_replay(gpu, name, log, source=None):
    """Replays `log` (from `source` when given: the same bytes in other memory)
    and holds everything the call returns against the restatement."""
    want = want_of(name, log)
    assert want.code == 0, name
    t, bloom, zone, st = gpu.replay_log(log if source is None else source, m=M)
    data = t.data()
    assert data == want.file, f"{name}: {len(data)} file bytes against the restatement's {len(want.file)}"
    assert t.well_formed == bool(want.keys), name  # (the table of length 0 has no line to be in order, as compaction's)
    assert t.nlines == len(want.keys), name
    assert stats_tuple(st) == want.stats, f"{name}: stats {st!r} against {want.stats}"
    of = oracle.OracleFilter(M)
    if want.keys:
        of.insert_var(*ragged(want.keys))
    assert np.array_equal(bloom.bools(), of.bools()), f"{name}: filter bits"
    if want.keys:
        assert (zone.min, zone.max) == want.bounds, f"{name}: zone bounds"
        # the same entries through SsTable::create on the device
        made, _, _ = gpu.sstable_create(want.items, m=M)
        assert made.data() == data, f"{name}: differs from sstable_create of the deduplicated entries"
    else:
        assert zone is None, name
    # Database::get over the replayed table alone: every key, and keys it does not hold
    keys = want.keys + absent_keys(want.keys, np.random.default_rng(7), 32)
    d, o = ragged(keys)
    which, voff, vals = gpu.get_many([t], gpu.KeyBatch(n=len(keys), data=d, offsets=o))
    exp = [want.rows.get(k) for k in keys]
    assert which.tolist() == [0 if v is not None else -1 for v in exp], f"{name}: which"
    assert np.array_equal(voff, ragged([v or b"" for v in exp])[1]), f"{name}: value offsets"
    assert vals == b"".join(v or b"" for v in exp), f"{name}: values"
    return t, bloom, zone


GOOD = [c for c in CASES if c.code == 0]
BAD = [c for c in CASES if c.code != 0]


@pytest.mark.parametrize("case", GOOD, ids=[c.label for c in GOOD])
def test_hand_worked_logs(gpu, case):
    """The empty and degenerate logs, skipped pieces, the last write, the keys
    the sort must tell apart: the literal file first, then every other check."""
    t, _, _, st = gpu.replay_log(case.log, m=M)
    assert t.data() == case.file, case.label
    assert stats_tuple(st) == case.stats, case.label
    check_replay(gpu, case.label, case.log)


@pytest.mark.parametrize("case", BAD, ids=[c.label for c in BAD])
def test_errors(gpu, case):
    """Wal::new returns Err: the code, the exception, cleared outputs and the
    first bad piece's line and offset (through plain ctypes and the package)."""
    from lsmt_amd import _lib
    L = _lib.load()
    buf = np.frombuffer(case.log, np.uint8).copy()
    th, fh, st = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xBEEF), _lib.LogStats()
    rc = L.cb_log_replay(buf.ctypes.data, len(buf), M, 0, None, ctypes.byref(th), ctypes.byref(fh), ctypes.byref(st))
    assert rc == case.code, case.label
    assert th.value is None and fh.value is None, f"{case.label}: outputs not cleared"
    assert stats_tuple(st) == case.stats, f"{case.label}: stats {st!r} against {case.stats}"
    kind = UnicodeDecodeError if case.code == ref.EUTF8 else ValueError
    with pytest.raises(kind) as e:
        gpu.replay_log(case.log, m=M)
    assert not (case.code == ref.EBASE64 and isinstance(e.value, UnicodeDecodeError))
    assert "line %d " % case.stats[3] in str(e.value), str(e.value)
    assert stats_tuple(e.value.stats) == case.stats and e.value.code == case.code
    # without a filter asked for and without stats: the same code
    th = ctypes.c_void_p(0xDEAD)
    assert L.cb_log_replay(buf.ctypes.data, len(buf), 0, 0, None, ctypes.byref(th), None, None) == case.code
    assert th.value is None


def test_a_bad_piece_late_in_a_long_log(gpu):
    """The first bad piece of many, past the first block of pieces: line and
    offset from the device, a later bad piece of the other kind ignored."""
    log = GENERATED["9000 mixed lines"] + b"\n"
    cut = log.index(b"\n", len(log) // 2) + 1
    for piece, code in ((b"late\t@@@\n", ref.EBASE64), (b"la\xffte\tMQ==\n", ref.EUTF8)):
        other = b"x\xc0\tMQ==\n" if code == ref.EBASE64 else b"x\t=\n"
        bad = log[:cut] + piece + log[cut:] + other
        want = ref.Replay(bad)
        assert want.code == code and want.stats[3] > 4000 and want.stats[4] == cut
        with pytest.raises((UnicodeDecodeError, ValueError)) as e:
            gpu.replay_log(bad, m=M)
        assert e.value.code == code and stats_tuple(e.value.stats) == want.stats


@pytest.mark.parametrize("name", ["one key 300 times", "one key 300 times, a tombstone last"])
def test_one_key_written_300_times(gpu, name):
    """The key's run crosses the select's 256-record tile (asserted on the CPU
    in test_replay_cpu.py); the last write stands, a tombstone too."""
    log = GENERATED[name]
    t, _, _ = check_replay(gpu, name, log)
    want = want_of(name, log)
    last = want.rows[HOT]
    assert is_dead(last) == ("tombstone" in name)
    assert record(HOT, last) in t.data()


@pytest.mark.parametrize("name", ["4096 entries", "4097 entries", "5000 entries, 4500 of one key", "9000 mixed lines"])
def test_sort_paths(gpu, name):
    """4096 entries: the merge sort alone; 4097: the bin sort; 5000 with 4500
    of one key: the bins cannot place it and the merge sort redoes the order;
    9000 mixed lines: every kind of piece at once, no final newline."""
    check_replay(gpu, name, GENERATED[name])


def test_host_and_device_input(gpu):
    """The log as bytes, as a numpy array and as a device tensor: one answer."""
    import torch
    name = "one key 300 times"
    log = GENERATED[name]
    arr = np.frombuffer(log, np.uint8).copy()
    check_replay(gpu, name, log, source=arr)
    # (a view one byte into a device buffer: the log need not be aligned)
    dev = torch.zeros(len(arr) + 1, dtype=torch.uint8, device="cuda")
    dev[1:] = torch.from_numpy(arr).cuda()
    check_replay(gpu, name, log, source=dev[1:])
    s = torch.cuda.Stream()
    t, bloom, zone, st = gpu.replay_log(dev[1:], m=M, stream=s)
    assert t.data() == want_of(name, log).file and st.keys == 201


def test_no_filter_asked_for(gpu):
    from lsmt_amd import _lib
    L = _lib.load()
    log = GENERATED["one key 300 times"]
    buf = np.frombuffer(log, np.uint8).copy()
    th = ctypes.c_void_p()
    assert L.cb_log_replay(buf.ctypes.data, len(buf), 0, 0, None, ctypes.byref(th), None, None) == 0
    t = gpu.Table._adopt(th.value, 0)
    assert t.data() == want_of("one key 300 times", log).file and t.well_formed


def test_a_replayed_log_is_the_stores_newest_table(gpu):
    """Two flushed tables and a log replayed as the third and newest: compact,
    scan and count over all three against the model (store_model.Model,
    imported and not edited), which is handed the replayed dict as a flush."""
    rng = np.random.default_rng(11)
    keys = [b"ns%d:k%03d" % (i % 3, i) for i in range(400)]
    model = sm.Model()
    tables = []
    for base, lo, hi in ((100, 0, 300), (200, 150, 400)):
        entries = [(k, TOMBSTONE if rng.random() < 0.1 else stamped(base + i, b'{"c":"v%d"}' % base))
                   for i, k in enumerate(keys[lo:hi])]
        model.flush(entries)
        tables.insert(0, gpu.sstable_create(entries, m=M)[0])
    # the log since the last flush: overwrites, deletes, new keys, keys written twice
    recs = []
    for i in rng.permutation(400)[:260]:
        k = keys[i] if i % 5 else b"ns9:new%03d" % i
        recs.append((k, TOMBSTONE if rng.random() < 0.2 else stamped(300 + int(i), b'{"c":"log"}')))
    recs += [(k, stamped(999, b'{"c":"again"}')) for k, _ in recs[:40]]
    log = b"".join(record(k, v) for k, v in recs)
    want = ref.Replay(log)
    assert want.code == 0 and len(want.rows) < len(recs)
    model.flush(want.items)
    t, _, _ = check_replay(gpu, "the store's log", log)
    tables.insert(0, t)
    newest = model.entries("newest")
    assert gpu.scan(tables).items() == [(k, v) for k, v, _ in newest]
    assert gpu.scan(tables).which().tolist() == [w for _, _, w in newest]
    entries, live = gpu.count(tables, ranges=ALL)
    assert (int(entries[0]), int(live[0])) == (len(newest), len(model.entries("newest", live=True)))
    ct, cb, cz = gpu.compact(tables, m=M)
    folded = sm.Model.fold(model.dicts, "newest")
    assert ct.data() == oracle.sstable_create(sorted(folded.items()))
    lt, _, _ = gpu.compact_live(tables, m=M)
    assert lt.data() == oracle.sstable_create(sorted(sm.Model.fold(model.dicts, "live").items()))
