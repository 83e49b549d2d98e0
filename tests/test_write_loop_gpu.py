"""The full loop on the device: rows written by cb_rows_write
(lsmt_amd.write) go on to the entries that take its arrays — the flush
(cb_sstable_create), the log replay (cb_log_replay), the ring's router
(cb_ring_route_var) — and come back through scan, get, compaction and select
as what a plain dict model of the statements holds.
"""
import json

import numpy as np
import pytest

import rowwrite_ref as ref

pytestmark = pytest.mark.gpu

KC = ("pk", "ck")
COLS = ["a", "b", "c"]


def insert_rows(n, tag=b"v"):
    """n rows (pk, ck, a, b, c) with distinct keys in no particular order."""
    return [[b"p%03d" % (i * 37 % n), b"c%d" % (i % 3), tag + b"%d" % i, b"x" * (i % 5), b'q"\n' if i % 4 == 0 else b"z"]
            for i in range(n)]


def model_of(rows, m=None):
    """{key: {column: value}} after the INSERT of rows, over m."""
    m = dict(m or {})
    for r in rows:
        m[b"ns:" + r[0] + b"|" + r[1]] = dict(zip(COLS, r[2:]))
    return m


def selected(result, skip=3):
    """{key: {column: value}} of a scan result selected with every column."""
    res = result.select(COLS + list(KC), KC, skip=skip)
    rows = json.loads(res.text().decode())
    assert not (res.flags() & 24).any()  # (no BADJSON, no EXTRA)
    res.close()
    out = {}
    for r in rows:
        key = b"ns:" + r.pop("pk").encode() + b"|" + r.pop("ck").encode()
        out[key] = {k: v.encode() for k, v in r.items()}
    return out


def test_the_log_replays_to_the_table_the_flush_makes(gpu):
    import lsmt_amd.write as wr
    rows = insert_rows(300)
    w = wr.write_rows("ns", rows, 2, COLS, ts=list(range(300)))
    table, bloom, zone = w.to_table(m=1024)
    keys, vals = w.keys(), w.values()
    assert table.data() == gpu.sstable_create(list(zip(keys, vals)), m=1024)[0].data()
    assert (zone.min, zone.max) == (min(keys), max(keys))
    for replayed in (gpu.replay_log(w.log(), m=1024), w.replay(m=1024)):  # from the host's copy, and where it lies
        assert replayed[0].data() == table.data() and replayed[3].keys == 300
    assert all(bloom.may_contain(k) for k in keys[:20])
    w.close()
    # repeated keys: the flush is not defined for them; the replay keeps each key's last record
    again = rows + [r[:2] + [b"second", b"", b"!"] for r in rows[:100]]
    w = wr.write_rows("ns", again, 2, COLS, ts=7)
    last = dict(zip(w.keys(), w.values()))
    assert len(last) == 300
    want = gpu.sstable_create(sorted(last.items()), m=1024)[0].data()
    assert gpu.replay_log(w.log(), m=1024)[0].data() == want and w.replay(m=1024)[0].data() == want
    w.close()


def test_insert_scan_select_returns_the_inserted_cells(gpu):
    import lsmt_amd.write as wr
    rows = insert_rows(257)
    w = wr.write_rows("ns", rows, 2, COLS, ts=1)
    table = w.to_table()[0]
    w.close()  # (the table is finalised: it no longer reads the batch)
    got = selected(gpu.scan([table], prefix=b"ns:"))
    assert got == model_of(rows)


def test_update_over_an_enqueue_only_get_then_compact(gpu):
    """A table, a get left in device memory, UPDATE SET a over it keeping b and
    c, a second table, compaction: the select equals the dict model. Half of
    the updated keys are not in the first table: their rows hold a alone."""
    import torch

    import lsmt_amd.write as wr
    rows = insert_rows(300)
    first = wr.write_rows("ns", rows, 2, COLS, ts=1).to_table()[0]
    model = model_of(rows)
    upd = [[r[0], r[1], b"new%d" % i] for i, r in enumerate(rows[:150])] + [[b"q%d" % i, b"c0", b"fresh"] for i in range(150)]
    keys = [b"ns:" + r[0] + b"|" + r[1] for r in upd]
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    batch = gpu.KeyBatch(n=len(keys), data=torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda(),
                         offsets=torch.from_numpy(off).cuda())
    which = torch.full((len(keys),), 7, dtype=torch.int32, device="cuda")
    voff = torch.zeros(len(keys) + 1, dtype=torch.int64, device="cuda")
    vals = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert gpu.get_many([first], batch, out=(which, voff, vals), stream=s, wait=False)[2] is None
    w = wr.write_rows("ns", upd, 2, ["a"], ["b", "c"], "update", ts=2, old=(which, voff, vals), stream=s)
    assert w.flagged == 0 and which.cpu().tolist() == [0] * 150 + [-1] * 150
    second = w.to_table(stream=s)[0]
    for k, r in zip(keys, upd):
        model[k] = dict(model.get(k, {}), a=r[2])
    merged = gpu.compact([second, first], m=1024)[0]
    assert selected(gpu.scan([merged], prefix=b"ns:")) == model
    assert selected(gpu.scan([second, first], prefix=b"ns:")) == model
    # and the values are the restatement's, old rows and all
    names = [c.encode() for c in COLS]
    olds = [ref.write_row(b"ns", r[:2], names, dict(zip(names, r[2:])), ref.INSERT, 1)[1] for r in rows[:150]] + [None] * 150
    assert w.values() == ref.write_batch(b"ns", upd, 2, [b"a"], [b"b", b"c"], ref.UPDATE, 2, olds)[1]
    w.close()


def test_delete_then_compact_live_drops_the_row(gpu):
    import lsmt_amd.write as wr
    rows = insert_rows(257)
    first = wr.write_rows("ns", rows, 2, COLS, ts=1).to_table()[0]
    gone = [r[:2] for r in rows[::3]]
    w = wr.write_rows("ns", gone, 2, op="delete", ts=2)
    assert set(w.values()) == {(2).to_bytes(8, "big")}
    second = w.to_table()[0]
    model = model_of(rows)
    for r in gone:
        del model[b"ns:" + r[0] + b"|" + r[1]]
    live = gpu.compact_live([second, first], m=1024)[0]
    assert live.nlines == len(model) and selected(gpu.scan([live], prefix=b"ns:")) == model
    assert gpu.compact([second, first], m=1024)[0].nlines == len(rows)  # (the plain compaction keeps the tombstones)
    w.close()


def test_written_keys_route_as_the_host_routes_them(gpu):
    import torch

    import lsmt_amd.ring as ring
    import lsmt_amd.write as wr
    rows = insert_rows(300)
    w = wr.write_rows("ns", rows, 2, COLS)
    rg = ring.Ring(["n%d" % i for i in range(5)], vnodes=8, rf=3)
    tok = torch.zeros(300, dtype=torch.int32, device="cuda")
    rep = torch.full((300, 3), -1, dtype=torch.int32, device="cuda")
    a = w.arrays()
    L = gpu._lib.load()
    torch.cuda.synchronize()
    assert L.cb_ring_route_var(rg._h, a["keys"], a["key_off"], 300, 3, 1, 0, tok.data_ptr(), rep.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want = [rg.replicas(k, skip=3, npk=1) for k in w.keys()]
    assert (tok.cpu().numpy().view(np.uint32).tolist(), rep.cpu().tolist()) == ([t for t, _ in want], [r for _, r in want])
    # and the filter takes them where they lie
    f = gpu.BloomFilter(1 << 16)
    assert L.cb_filter_insert_var(f._h, a["keys"], a["key_off"], 300, None) == 0
    assert all(f.may_contain(k) for k in w.keys())
    w.close()
