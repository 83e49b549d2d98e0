"""Whole store histories on the device beside the plain model of
tests/store_model.py: tables made by the device flush are compacted and the
result compacted again, inputs are closed at once so the pool hands their
blocks to the next flush, filter slots are cleared and reused for tables with
other key ranges, the table list changes while it stays the same list object,
zones are rewritten, tables are re-indexed from their own bytes, and after
each of these every read path and every scan is asked again.

Every comparison is exact, against the model (whose own answers
tests/test_store_model_cpu.py holds against the C oracle step by step) and
against the oracle's filters and gates. No table here is opened from a
hand-written file: every one is made by sstable_create or a compaction, or is
a reopen of such a table's own bytes.

A failing history can be rerun up to a step with replay(name, upto). The
harness catches nothing: a device error ends the history where it occurred.
"""
import numpy as np
import pytest

import store_model as sm
from merge_help import ragged
from oracle import oracle
from test_live_gpu import assert_result

pytestmark = pytest.mark.gpu

STREAM_HISTORY = "random-ns-ordered"        # every op on one torch.cuda.Stream()
DEVICE_KEYS_HISTORY = "random-hex16-replica"  # read keys travel as DeviceKeys


class Rec:
    """What the store keeps per open table beside the Table itself."""

    def __init__(self, bloom, zone, mt, settled=True):
        self.bloom, self.zone, self.mt, self.settled = bloom, zone, mt, settled


class DeviceStore:
    def __init__(self, gpu, name, stream=None, device_keys=False):
        self.gpu, self.name, self.stream, self.device_keys = gpu, name, stream, device_keys
        self.family = sm.FAMILY[name]
        self.model = sm.Model()
        self.tables = []  # the one list object every call is handed
        self.recs = []
        self.sets = [gpu.FilterSet(m, width=w) for m, w in sm.TIERS]
        self.wide = gpu.FilterSet(sm.WIDE[0], width=sm.WIDE[1])
        self.step, self.op, self.history = -1, None, []
        self.late = None  # (step, op, keys) of a gate check that waits for the read after it

    # -- plumbing --
    def what(self, note=""):
        return f"{self.name} step {self.step} {sm.describe(self.op)}: {note}"

    def batch(self, keys):
        """Fixed [n, 16] rows in the 16-byte family (on the device in one
        history), a ragged KeyBatch otherwise."""
        if self.family == "hex16" and keys and all(len(k) == 16 for k in keys):
            a = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16).copy()
            if self.device_keys:
                import torch
                return self.gpu.DeviceKeys(torch.from_numpy(a).cuda())
            return a
        d, o = ragged(keys)
        return self.gpu.KeyBatch(n=len(keys), data=d, offsets=o)

    def on_device(self, kb):
        return not isinstance(kb, np.ndarray) and hasattr(getattr(kb, "keys", None), "is_cuda")

    def rows(self, call, kb, nrows, n):
        """Hit rows of a probe call as uint64[nrows, words] (through device memory for device keys)."""
        if not self.on_device(kb):
            return call(), None
        import torch
        out = torch.full((max(nrows, 1), max((n + 63) // 64, 1)), -1, dtype=torch.int64, device="cuda")
        call(out=out)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint64)[:nrows, :(n + 63) // 64], out

    def got(self, call, kb, n, nvals):
        """(which, val_off, vals) of a get call."""
        if not self.on_device(kb):
            return call()
        import torch
        which = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
        voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        vals = torch.zeros(nvals + 64, dtype=torch.uint8, device="cuda")
        _, _, total = call(out=(which, voff, vals))
        torch.cuda.synchronize()
        return which.cpu().numpy()[:n], voff.cpu().numpy().view(np.uint64), vals[:total].cpu().numpy().tobytes()

    def tiers_slots(self):
        return (np.asarray([r.mt.tier for r in self.recs], np.uint32), np.asarray([r.mt.slot for r in self.recs], np.uint32),
                np.asarray([r.mt.wslot for r in self.recs], np.uint32))

    # -- checks --
    def check_table(self, i, bloom=None):
        """The table's file, line count and form, its filter and its zone."""
        t, rec = self.tables[i], self.recs[i]
        mt = rec.mt
        data = t.data()
        assert data == mt.file, self.what(f"table {i}: {len(data)} file bytes against the model's {len(mt.file)}")
        assert t.nlines == len(mt.keys), self.what(f"table {i}: nlines")
        assert t.well_formed, self.what(f"table {i}: not well formed")
        bloom = rec.bloom if bloom is None else bloom
        assert np.array_equal(bloom.bools(self.stream), mt.ofilter().bools()), self.what(f"table {i}: filter bits")
        assert (rec.zone.min, rec.zone.max) == mt.bounds, self.what(f"table {i}: zone bounds")
        z = self.sets[mt.tier].zone(mt.slot)
        assert (z.min, z.max) == mt.bounds, self.what(f"table {i}: the slot's zone")

    def check_gates(self, keys, now=False):
        """probe_tiers, gated and not, against the oracle; and every set's own
        rows: an occupied slot answers as its table's oracle filter and zone,
        a free one (never used, or cleared) answers nothing. At every other
        step, when a read follows, the check runs after that read, so that the
        fused gets are the first to see the changed slots and zones."""
        if not keys or not self.tables:
            return
        nxt = self.history[self.step + 1]["op"] if self.step + 1 < len(self.history) else None
        if not now and self.step % 2 and nxt == "read":
            self.late = (self.step, self.op, keys)
            return
        gpu, n, s = self.gpu, len(keys), self.stream
        kb = self.batch(keys)
        d, o = ragged(keys)
        mts = [r.mt for r in self.recs]
        tiers, slots, wslots = self.tiers_slots()
        want = {True: oracle.probe_gated([t.ofilter() for t in mts], [t.ozone() for t in mts], d, o),
                False: oracle.probe_var([t.ofilter() for t in mts], d, o)}
        wwant = {True: oracle.probe_gated([t.ofilter(sm.WIDE[0]) for t in mts], [t.ozone() for t in mts], d, o),
                 False: oracle.probe_var([t.ofilter(sm.WIDE[0]) for t in mts], d, o)}
        for gated in (True, False):
            rows, _ = self.rows(lambda **kw: gpu.probe_tiers(self.sets, tiers, slots, kb, gated=gated, stream=s, **kw),
                                kb, len(mts), n)
            assert np.array_equal(rows, want[gated]), self.what(f"probe_tiers(gated={gated}) differs from the oracle")
            for tier, st in list(enumerate(self.sets)) + [(-1, self.wide)]:
                used = st.used
                if not used:
                    continue
                exp = np.zeros((used, (n + 63) // 64), np.uint64)
                for t, mt in enumerate(mts):
                    if tier < 0:
                        exp[mt.wslot] = wwant[gated][t]
                    elif mt.tier == tier:
                        exp[mt.slot] = want[gated][t]
                rows, _ = self.rows(lambda **kw: st.probe(kb, gated=gated, stream=s, **kw), kb, used, n)
                bad = np.flatnonzero((rows != exp).any(1))
                assert not len(bad), self.what(f"{'wide set' if tier < 0 else f'tier {tier}'} gated={gated}: "
                                               f"slots {bad.tolist()} differ (a free slot must answer nothing)")

    def settle(self):
        """What a deferred flush or compaction left undone, before the first read."""
        for i, (t, rec) in enumerate(zip(self.tables, self.recs)):
            if rec.settled:
                continue
            if rec.zone is None:
                rec.zone = self.gpu.ZoneMap(t._zone(0), t._zone(1)) if t.nlines else self.gpu.ZoneMap()
            self.assign_wide(t, rec.mt)
            rec.settled = True
            self.check_table(i)

    def assign_wide(self, t, mt):
        b, z = t.rebuild(sm.WIDE[0], stream=self.stream)
        assert np.array_equal(b.bools(self.stream), mt.ofilter(sm.WIDE[0]).bools()), self.what("rebuild: filter bits")
        assert (z.min, z.max) == mt.bounds, self.what("rebuild: zone bounds")
        self.wide.assign(mt.wslot, b, stream=self.stream)
        self.wide.set_zone(mt.wslot, z, stream=self.stream)
        b.close()

    # -- ops --
    def create(self, entries, form, wait):
        gpu, s = self.gpu, self.stream
        if form == "list":
            return gpu.sstable_create(entries, m=sm.TIERS[0][0], stream=s, wait=wait)
        kd, ko = ragged([k for k, _ in entries])
        vd, vo = ragged([v for _, v in entries])
        if form == "device":  # device tensors, not waited for, used at once
            import torch
            kd, ko, vd, vo = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (kd, ko, vd, vo))
            wait = False
        kb = gpu.KeyBatch(n=len(entries), data=kd, offsets=ko)
        vb = gpu.KeyBatch(n=len(entries), data=vd, offsets=vo)
        return gpu.sstable_create((kb, vb), m=sm.TIERS[0][0], stream=s, wait=wait)

    def flush(self, op):
        s = self.stream
        mt = sm.apply(self.model, op)
        t, bloom, zone = self.create(op["entries"], op["form"], wait=not op["defer"])
        self.tables.insert(0, t)
        self.recs.insert(0, Rec(bloom, zone, mt, settled=not op["defer"]))
        st = self.sets[0]
        st.assign(mt.slot, bloom, stream=s)
        if op["defer"]:  # nothing of the table is touched: the zone comes from the keys, on the device
            st.zone_from_keys(mt.slot, [k for k, _ in op["entries"]], stream=s)
            return
        if zone is None:
            assert t.data() == mt.file, self.what("the pending table's file, read at once")
            zone = self.recs[0].zone = self.gpu.ZoneMap(t._zone(0), t._zone(1))
        st.set_zone(mt.slot, zone, stream=s)
        self.assign_wide(t, mt)
        self.check_table(0)
        self.check_gates(op["probe"])

    def compact(self, op):
        gpu, s = self.gpu, self.stream
        i, j = op["i"], op["j"]
        whole = i == 0 and j == len(self.tables) - 1
        ins = self.tables if whole else self.tables[i:j + 1]
        if op["kind"] == "newest":
            merged, bloom, zone = gpu.compact(ins, m=op["m"], stream=s)
        elif op["kind"] == "live":
            merged, bloom, zone = gpu.compact_live(ins, m=op["m"], stream=s)
        else:
            merged, bloom, zone = gpu.compact_lww(ins, m=op["m"], drop_dead=op["drop_dead"], stream=s)
        old = self.recs[i:j + 1]
        for t in self.tables[i:j + 1]:        # 1: the inputs are closed before anything else
            t.close()
        for r in old:
            r.bloom.close()
        self.tables[i] = merged               # the same list object: one element replaced, the rest popped
        for _ in range(j - i):
            self.tables.pop(i + 1)
        for r in old:                         # 2: their slots are cleared
            self.sets[r.mt.tier].clear_slot(r.mt.slot, stream=s)
            self.wide.clear_slot(r.mt.wslot, stream=s)
        _, mt = sm.apply(self.model, op)
        self.recs[i:j + 1] = [Rec(bloom, zone, mt, settled=not op["defer"])]
        st = self.sets[mt.tier]               # 3: the merged filter and zone go into the next tier
        st.assign(mt.slot, bloom, stream=s)
        st.set_zone(mt.slot, zone, stream=s)
        if op["defer"]:
            return
        self.assign_wide(merged, mt)          # 4: the wide slot, from the merged table's own bytes
        self.check_table(i)
        self.check_gates(op["probe"])

    def reopen(self, op):
        gpu, s, i = self.gpu, self.stream, op["i"]
        t, rec = self.tables[i], self.recs[i]
        new = gpu.Table(t.data(), stream=s)
        meta = gpu.TableMeta(rec.bloom, rec.zone).encode()
        assert meta == oracle.meta_encode(rec.mt.ofilter(), rec.mt.ozone() if rec.mt.keys else oracle.OracleZone()), \
            self.what("the table's .meta")
        self.tables[i] = new                  # the list keeps its length
        t.close()
        self.sets[rec.mt.tier].load_meta(rec.mt.slot, meta, stream=s)  # the restart path
        self.assign_wide(new, rec.mt)
        loaded, zone = gpu.TableMeta.load(meta)
        assert (zone.min, zone.max) == rec.mt.bounds, self.what("the decoded zone")
        self.check_table(i, bloom=loaded)
        self.check_gates(op["probe"])

    def churn(self, op):
        made = [self.gpu.sstable_create(e, stream=self.stream) for e in op["entries"]]
        for (t, b, _), e in zip(made, op["entries"]):
            assert t.nlines == len(e), self.what("a throw-away table")
            t.close()
            b.close()

    def read(self, op):
        gpu, s, keys = self.gpu, self.stream, op["keys"]
        n = len(keys)
        ew, evoff, evals = self.model.get(keys)
        kb = self.batch(keys)
        tiers, slots, wslots = self.tiers_slots()
        tables = self.tables

        def same(path, res):
            which, voff, vals = res
            bad = np.flatnonzero(np.asarray(which) != ew)
            assert not len(bad), self.what(f"{path}: which differs at {bad[:8].tolist()} ({[keys[b] for b in bad[:3]]}): "
                                           f"{np.asarray(which)[bad[:8]].tolist()} against {ew[bad[:8]].tolist()}")
            assert np.array_equal(np.asarray(voff, np.uint64), evoff), self.what(f"{path}: val_off differs")
            assert vals == evals, self.what(f"{path}: values differ")

        same("get_many", self.got(lambda **kw: gpu.get_many(tables, kb, stream=s, **kw), kb, n, len(evals)))
        rows, dev = self.rows(lambda **kw: gpu.probe_tiers(self.sets, tiers, slots, kb, gated=True, stream=s, **kw),
                              kb, len(tables), n)
        hits = rows if dev is None else dev
        same("get_many(hits=probe_tiers)",
             self.got(lambda **kw: gpu.get_many(tables, kb, hits=hits, stream=s, **kw), kb, n, len(evals)))
        same("get_many_tiers",
             self.got(lambda **kw: gpu.get_many_tiers(tables, self.sets, tiers, slots, kb, stream=s, **kw), kb, n, len(evals)))
        same("get_many(filterset=wide)",
             self.got(lambda **kw: gpu.get_many(tables, kb, filterset=self.wide, hit_rows=wslots, stream=s, **kw),
                      kb, n, len(evals)))
        for i, (t, rec) in enumerate(zip(tables, self.recs)):
            want = np.asarray([rec.mt.line.get(k, -1) for k in keys], np.int64)
            if self.on_device(kb):
                import torch
                out = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
                t.search(kb, out=out, stream=s)
                torch.cuda.synchronize()
                found = out.cpu().numpy()[:n]
            else:
                found = t.search(kb, stream=s)
            assert np.array_equal(found, want), self.what(f"table {i}: search differs from the line numbers of its file")
        if self.late is not None:
            here, (self.step, self.op, late_keys), self.late = (self.step, self.op), self.late, None
            self.check_gates(late_keys, now=True)
            self.step, self.op = here

    def scan(self, op):
        gpu, s = self.gpu, self.stream
        want, off = sm.cut(self.model.entries(op["rule"], live=op["live"]), sm.op_ranges(op))
        truncated = False
        if op["limit"]:
            truncated, want = len(want) > op["limit"], want[:op["limit"]]
            off = np.asarray([0, len(want)], np.uint64)
        kw = sm.range_kw(op)
        if op["rule"] == "lww":
            r = gpu.scan_lww(self.tables, drop_dead=op["live"], limit=op["limit"], stream=s, **kw)
        elif op["live"]:
            r = gpu.scan_live(self.tables, limit=op["limit"], stream=s, **kw)
        else:
            r = gpu.scan_many(self.tables, stream=s, **kw)
        assert r.nranges == len(sm.op_ranges(op)), self.what("nranges")
        assert_result(r, want, self.what(), truncated=truncated)
        assert np.array_equal(r.range_off(), off), self.what(f"range_off {r.range_off().tolist()} against {off.tolist()}")
        if op["rule"] == "lww":
            assert r.ts().tolist() == [int.from_bytes(v[:8], "big") for _, v, _ in want], self.what("timestamps")

    def count(self, op):
        fn = self.gpu.count_lww if op["rule"] == "lww" else self.gpu.count
        entries, live = fn(self.tables, stream=self.stream, **sm.range_kw(op))
        for got, lv in ((entries, False), (live, True)):
            _, off = sm.cut(self.model.entries(op["rule"], live=lv), sm.op_ranges(op))
            assert got.tolist() == np.diff(off.astype(np.int64)).tolist(), self.what("live" if lv else "entries")

    def count_where(self, op):
        gpu, s = self.gpu, self.stream
        kw = sm.range_kw(op)
        rows, off = sm.cut(self.model.entries("lww" if op["lww"] else "newest", live=True), sm.op_ranges(op))
        verdicts = sm.where_verdicts(op, rows, off)
        o = [int(x) for x in off]
        live, matched = gpu.count_where(self.tables, op["where"], op["key_columns"], skip=op["skip"], lww=op["lww"],
                                        stream=s, **kw)
        assert live.tolist() == np.diff(o).tolist(), self.what("live")
        assert matched.tolist() == [sum(verdicts[o[r]:o[r + 1]]) for r in range(len(o) - 1)], self.what("matched")
        r = gpu.scan_lww(self.tables, drop_dead=True, stream=s, **kw) if op["lww"] else gpu.scan_live(self.tables, stream=s, **kw)
        assert_result(r, rows, self.what("the live scan"))
        flags = r.match(op["where"], op["key_columns"], skip=sm.where_skips(op))
        assert flags.tolist() == verdicts, self.what("ScanResult.match differs entry by entry")

    def run(self, history):
        self.history = history
        for self.step, self.op in enumerate(history):
            op = self.op
            if not op.get("defer") and op["op"] != "churn":
                self.settle()
            getattr(self, op["op"])(op)
        self.settle()
        if self.late is not None:  # (a history cut before the read that the check waited for)
            (self.step, self.op, late_keys), self.late = self.late, None
            self.check_gates(late_keys, now=True)
        return self


def replay(name, upto=None, gpu=None):
    """Runs history[:upto] of that name on the device beside the model (a
    failing prefix, alone). Returns the DeviceStore."""
    if gpu is None:
        import lsmt_amd as gpu
    stream = None
    if name == STREAM_HISTORY:
        import torch
        stream = torch.cuda.Stream()
    return DeviceStore(gpu, name, stream=stream, device_keys=name == DEVICE_KEYS_HISTORY).run(sm.build(name)[:upto])


@pytest.mark.parametrize("name", sm.NAMES)
def test_history(gpu, name):
    store = replay(name, gpu=gpu)
    assert store.step == len(sm.build(name)) - 1
    assert [len(r.mt.keys) for r in store.recs] == [t.nlines for t in store.tables]
