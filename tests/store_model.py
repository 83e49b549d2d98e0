"""A plain model of the LSM store and the histories it is driven through.

The model is a list of dict[bytes, bytes], newest first: key -> decoded value,
a value being the 8-byte big-endian timestamp plus a payload and a tombstone
the 8 bytes alone. It adds no rule of its own; it composes what the suite
already trusts:

    a table's file      oracle.sstable_create of the dict's sorted items
    get                 the newest-first walk (src/lib.rs:128-134)
    live rows           liverow_ref.is_dead
    LWW winners         lww_ref.winners
    WHERE verdicts      rowjson_ref.matches
    prefix ends         merge_help.oracle_prefix_end
    compact(i, j)       the run's dicts replaced by their newest, live or LWW fold

The model also hands out the filter slots (lowest free first, so a slot is
reused as early as possible), because which slot a table lands in is part of
what the histories are about; tests/test_store_model_cpu.py checks on the CPU
that every history really exercises reuse, and tests/test_store_gpu.py replays
the same histories on the device beside this model.

A history is a list of ops (plain dicts of plain data) built entirely on the
CPU from a name and a seed, so it can be printed, cut (history[:k]) and
replayed. A plain module: no test, no fixture, nothing collected.
"""
import bisect

import numpy as np

import lww_ref
import rowjson_ref
from liverow_ref import is_dead
from merge_help import oracle_prefix_end, ragged
from oracle import oracle

TIERS = [(1024, 64), (16384, 32), (100_003, 32)]  # (m, width): flushed tables, then two compaction tiers
WIDE = (1024, 128)                                # every open table's Table.rebuild(1024) filter and zone
FLUSH_SIZES = [1, 15, 16, 17, 255, 256, 257, 300, 1000]
BIN_SORT_SIZE = 4097                              # shuffled: past sort.hip's 4096-record tile, the bin sort
READ_SIZES = [1, 63, 64, 65, 257, 1000]
FAMILIES = ("hex16", "ns", "long")
REGIMES = ("ordered", "replica")
MUTATING = ("flush", "compact", "reopen")
OP_KINDS = ("flush", "read", "compact", "scan", "count", "count_where", "reopen", "churn")
PAYLOADS = [b'{"c":"v"}', b'{"c":"w"}', b'{"c":"v","d":"e"}', b"not json", b'{"d":"e","c":"v"}', b"{}",
            b'{"c":"v"}x', b"x"]
KEY_COLUMNS = ("pk", "ck")                        # the ns family's keys are ns%d:pk|ck


def tier_of(m: int) -> int:
    return [tm for tm, _ in TIERS].index(m)


# ---- the model ------------------------------------------------------------------------

class MTable:
    """One table of the model: its dict, where its filter sits, and the
    oracle's view of it (file, filter at any m, zone), each built once."""

    def __init__(self, rows, tier, slot, wslot):
        self.rows, self.tier, self.slot, self.wslot = rows, tier, slot, wslot
        self.keys = sorted(rows)
        self.line = {k: i for i, k in enumerate(self.keys)}
        self._file, self._filters, self._otable = None, {}, None

    @property
    def m(self) -> int:
        return TIERS[self.tier][0]

    @property
    def bounds(self):
        return (self.keys[0], self.keys[-1]) if self.keys else (None, None)

    @property
    def file(self) -> bytes:
        if self._file is None:
            self._file = oracle.sstable_create([(k, self.rows[k]) for k in self.keys]) if self.keys else b""
        return self._file

    @property
    def otable(self):
        if self._otable is None:
            self._otable = oracle.OracleTable(self.file)
        return self._otable

    def ofilter(self, m=None):
        m = m or self.m
        if m not in self._filters:
            f = oracle.OracleFilter(m)
            if self.keys:
                f.insert_var(*ragged(self.keys))
            self._filters[m] = f
        return self._filters[m]

    def ozone(self):
        return oracle.OracleZone(*self.bounds)

    def excludes(self, key) -> bool:
        """The table's zone map rejects the key (src/zonemap.rs:37-42)."""
        return bool(self.keys) and not self.keys[0] <= key <= self.keys[-1]


class Model:
    def __init__(self):
        self.tables = []                                   # MTable, newest first
        self.free = [set(range(w)) for _, w in TIERS]
        self.wfree = set(range(WIDE[1]))
        self.former = {}                                   # (tier, slot) -> keys of the table that last left it
        self.left = []                                     # [(tier, slot, keys)] in the order tables left
        self.reuses = []                                   # [(former keys, MTable)] whenever a slot is taken again

    @property
    def dicts(self):
        return [t.rows for t in self.tables]

    def _place(self, rows, tier):
        slot, wslot = min(self.free[tier]), min(self.wfree)
        self.free[tier].remove(slot)
        self.wfree.remove(wslot)
        mt = MTable(rows, tier, slot, wslot)
        if (tier, slot) in self.former:
            self.reuses.append((self.former[(tier, slot)], mt))
        return mt

    def _release(self, mt):
        self.free[mt.tier].add(mt.slot)
        self.wfree.add(mt.wslot)
        self.former[(mt.tier, mt.slot)] = mt.keys
        self.left.append((mt.tier, mt.slot, mt.keys))

    def flush(self, entries):
        rows = dict(entries)
        assert len(rows) == len(entries), "a memtable holds a key once"
        mt = self._place(rows, 0)
        self.tables.insert(0, mt)
        return mt

    @staticmethod
    def positions(dicts, kind):
        """{key: (value, position in dicts of the line that wins)} under the
        compaction kind's rule, dead winners included."""
        if kind == "lww":
            return {k: (v, r) for k, v, r, _ in lww_ref.winners(dicts)}
        out = {}
        for k in set().union(*dicts):
            r = next(i for i, d in enumerate(dicts) if k in d)  # the newest-first walk
            out[k] = (dicts[r][k], r)
        return out

    @classmethod
    def fold(cls, dicts, kind, drop_dead=False):
        drop = kind == "live" or (kind == "lww" and drop_dead)
        return {k: v for k, (v, _) in cls.positions(dicts, kind).items() if not (drop and is_dead(v))}

    def compact(self, i, j, kind, m, drop_dead=False):
        ins = self.tables[i:j + 1]
        rows = self.fold([t.rows for t in ins], kind, drop_dead)
        for t in ins:
            self._release(t)
        mt = self._place(rows, tier_of(m))
        self.tables[i:j + 1] = [mt]
        return ins, mt

    def get(self, keys):
        """(which int32[n], val_off uint64[n + 1], vals) of the newest-first walk."""
        dicts = self.dicts
        which, vals = [], []
        for k in keys:
            t = next((i for i, d in enumerate(dicts) if k in d), -1)
            which.append(t)
            vals.append(dicts[t][k] if t >= 0 else b"")
        voff = np.zeros(len(keys) + 1, np.uint64)
        np.cumsum([len(v) for v in vals], out=voff[1:])
        return np.asarray(which, np.int32).reshape(-1), voff, b"".join(vals)

    def entries(self, rule, live=False):
        """[(key, value, which)] sorted by key: every key's newest line, or its
        LWW winner; `live` leaves out the tombstones."""
        if rule == "lww":
            out = [(k, v, r) for k, v, r, _ in lww_ref.winners(self.dicts)]
        else:
            out = [(k, v, r) for k, (v, r) in sorted(self.positions(self.dicts, "newest").items())] if self.tables else []
        return [x for x in out if not is_dead(x[1])] if live else out


def apply(model, op):
    """Advance the model by one op; what a mutating op made or replaced is returned."""
    if op["op"] == "flush":
        return model.flush(op["entries"])
    if op["op"] == "compact":
        return model.compact(op["i"], op["j"], op["kind"], op["m"], op["drop_dead"])
    return None


def op_ranges(op):
    """The op's ranges as (lo, hi) pairs, prefixes turned into ranges."""
    if op.get("prefixes") is not None:
        return [(p, oracle_prefix_end(p)) for p in op["prefixes"]]
    return [tuple(r) for r in op["ranges"]]


def range_kw(op):
    return {"prefixes": op["prefixes"]} if op.get("prefixes") is not None else {"ranges": [tuple(r) for r in op["ranges"]]}


def cut(entries, ranges):
    """(entries of every range one after the other, range_off)."""
    keys = [x[0] for x in entries]
    parts = []
    for lo, hi in ranges:
        a = bisect.bisect_left(keys, lo)
        b = len(keys) if hi is None else bisect.bisect_left(keys, hi)
        parts.append(entries[a:max(a, b)])
    off = np.zeros(len(ranges) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return [x for p in parts for x in p], off


def where_skips(op):
    """count_where's skip per range: the op's, or the default (a prefix's length, 0 for ranges)."""
    nr = len(op_ranges(op))
    if op["skip"] is not None:
        return [op["skip"]] * nr
    return [len(p) for p in op["prefixes"]] if op.get("prefixes") is not None else [0] * nr


def where_verdicts(op, entries, off):
    """rowjson_ref's verdict for every entry of cut()'s result."""
    out, off = [], [int(x) for x in off]
    for r, s in enumerate(where_skips(op)):
        out += [rowjson_ref.matches(k, v, op["where"], op["key_columns"], s) for k, v, _ in entries[off[r]:off[r + 1]]]
    return out


def describe(op) -> str:
    """One line for an assertion message."""
    o = op["op"]
    if o == "flush":
        return f"flush({len(op['entries'])} entries, {op['order']}, {op['form']}{', deferred' if op['defer'] else ''})"
    if o == "read":
        return f"read({len(op['keys'])} keys)"
    if o == "compact":
        return (f"compact({op['i']}..{op['j']}, {op['kind']}, m={op['m']}, drop_dead={op['drop_dead']}"
                f"{', deferred' if op['defer'] else ''})")
    if o in ("scan", "count", "count_where"):
        what = f"{len(op_ranges(op))} {'prefixes' if op.get('prefixes') is not None else 'ranges'}"
        rest = {k: v for k, v in op.items() if k not in ("op", "ranges", "prefixes")}
        return f"{o}({what}, {rest})"
    if o == "reopen":
        return f"reopen({op['i']})"
    return f"churn({len(op['entries'])} tables)"


# ---- keys -----------------------------------------------------------------------------

def make_pool(family, rng, n=7000):
    """n distinct keys of the family, sorted (Rust str order = byte order)."""
    out = set()
    if family == "hex16":       # the fixed-16 kernels
        while len(out) < n:
            out.add(b"%016x" % int(rng.integers(0, 1 << 62)))
    elif family == "ns":        # ns%d:pk|ck, ragged
        pks = sorted({b"%x" % int(rng.integers(0, 16 ** int(rng.integers(1, 10)))) for _ in range(150)})
        while len(out) < n:
            out.add(b"ns%d:%s|%d" % (int(rng.integers(0, 5)), pks[int(rng.integers(0, len(pks)))],
                                    int(rng.integers(0, 10 ** int(rng.integers(1, 4))))))
    else:                       # 17 to 40 bytes, 40 stems of 16 bytes shared by many keys
        stems = [b"stem-%02d-%08x" % (i, int(rng.integers(0, 1 << 32))) for i in range(40)]
        assert all(len(s) == 16 for s in stems)
        while len(out) < n:
            ln = int(rng.integers(1, 25))
            out.add(stems[int(rng.integers(0, 40))] + (b"%024x" % int(rng.integers(0, 1 << 62)))[-ln:])
    return sorted(out)


def prefix_choices(family, pool):
    """Lists of candidate prefixes, each list of one length (so none nests in another)."""
    if family == "hex16":
        return [sorted({k[:1] for k in pool}), sorted({k[:2] for k in pool})]
    if family == "ns":
        return [sorted({k[:4] for k in pool})]
    return [sorted({k[:16] for k in pool})]


# ---- building a history ---------------------------------------------------------------

class Builder:
    """Emits ops and advances a model with them, so that every op can be
    drawn against the store's state at that point."""

    def __init__(self, name, family, regime, seed):
        self.name, self.family, self.regime = name, family, regime
        self.rng = np.random.default_rng(seed)
        self.model = Model()
        self.ops = []
        self.pool = make_pool(family, self.rng)
        self.clock = 0
        self.nflush = 0
        self.witness = []   # keys the next read must hold
        self.kinds = []     # compaction kinds still to come, in this history's order

    # -- values --
    def stamp(self):
        if self.regime == "ordered":  # timestamps rise with write order
            self.clock += 1
            return self.clock
        return int(self.rng.integers(1, 1 << 40)) * 256 + self.nflush  # shuffled; distinct within a key

    def put(self, key, payload=None, ts=None):
        p = PAYLOADS[int(self.rng.integers(0, len(PAYLOADS)))] if payload is None else payload
        return key, (self.stamp() if ts is None else ts).to_bytes(8, "big") + p

    def delete(self, key, ts=None):
        return key, (self.stamp() if ts is None else ts).to_bytes(8, "big")

    def held(self, key):
        return any(key in d for d in self.model.dicts)

    def _emit(self, op):
        self.ops.append(op)
        return apply(self.model, op)

    def _probe(self, n=200):
        """Keys for the gate checks after a mutating op: of the newest table, of
        tables that have left their slots, of the rest of the store, absent ones."""
        return self.auto_keys(n, forced=False)

    # -- flush --
    def draw_entries(self, n, lo=None, width=None):
        """A memtable's content: n keys from a window of the sorted pool (so
        zones differ between tables), a quarter of them keys that older tables
        hold in that window; held keys are overwritten or deleted."""
        rng, P = self.rng, len(self.pool)
        w = min(P, max(3 * n, 60)) if width is None else width
        lo = int(rng.integers(0, P - w + 1)) if lo is None else lo
        keys = dict.fromkeys(self.pool[lo + int(i)] for i in rng.choice(w, min(n, w), replace=False))
        a, b = self.pool[lo], self.pool[lo + w - 1]
        older = [k for t in self.model.tables for k in t.keys[bisect.bisect_left(t.keys, a):bisect.bisect_right(t.keys, b)]]
        if older and n >= 4:
            take = dict.fromkeys(older[int(i)] for i in rng.choice(len(older), min(len(older), n // 4), replace=False))
            keys = dict.fromkeys(list(take) + [k for k in keys if k not in take])
        keys = list(keys)[:n]
        self.nflush += 1
        out = []
        for k in keys:
            dead = rng.random() < (0.4 if self.held(k) else 0.03)
            out.append(self.delete(k) if dead else self.put(k))
        return out

    def flush(self, entries=None, n=None, order="sorted", form="list", defer=False, **draw):
        if entries is None:
            entries = self.draw_entries(n, **draw)
        else:
            self.nflush += 1
        entries = sorted(entries)
        if order == "shuffled":
            entries = [entries[int(i)] for i in self.rng.permutation(len(entries))]
        op = {"op": "flush", "entries": entries, "order": order, "form": form, "defer": defer, "probe": None}
        mt = self._emit(op)
        op["probe"] = [] if defer else self._probe()
        return mt

    # -- read --
    def near(self, k, ragged_ok):
        """A near miss of a key: cut short, a byte appended, or (where the
        batch must stay 16 bytes wide) its last byte changed."""
        c = int(self.rng.integers(0, 3 if ragged_ok else 1))
        if c == 1:
            return k[:-1]
        if c == 2:
            return k + b"!"
        return k[:-1] + (b"g" if k[-1:] != b"g" else b"h")

    def auto_keys(self, n, forced=True, ragged_ok=None):
        """n keys over every class a read can fall in (the CPU test checks that
        each history's reads really hit them)."""
        rng, model = self.rng, self.model
        if ragged_ok is None:
            ragged_ok = self.family != "hex16" or (n > 1 and rng.random() < 0.3)
        out = []
        if forced:
            out, self.witness = self.witness[:n], self.witness[n:]
        tables = [t for t in model.tables if t.keys]
        newest = model.entries("newest") if tables else []
        tombs = [k for k, v, _ in newest if is_dead(v)]
        left = [ks for _, _, ks in model.left[-6:] if ks]
        left += [ks for ks in ([k for k in former if mt.excludes(k)] for former, mt in model.reuses[-4:]) if ks]

        def pick(seq):
            return seq[int(rng.integers(0, len(seq)))]
        while len(out) < n:
            c = rng.random()
            if c < 0.45 and tables:
                out.append(pick(pick(tables).keys))
            elif c < 0.55 and tombs:
                out.append(pick(tombs))
            elif c < 0.67 and left:
                out.append(pick(pick(left)))
            elif c < 0.80 and tables:
                out.append(self.near(pick(pick(tables).keys), ragged_ok))
            else:
                out.append(pick(self.pool))  # held somewhere, or absent everywhere
        return [out[int(i)] for i in rng.permutation(len(out))]

    def read(self, n=None, keys=None, **kw):
        if keys is None:
            keys = self.auto_keys(n, **kw)
        self._emit({"op": "read", "keys": list(keys)})

    # -- compact --
    def compact(self, i, j, kind, m=None, drop_dead=False, defer=False):
        ins = self.model.tables[i:j + 1]
        if kind == "live" or drop_dead:
            assert j == len(self.model.tables) - 1, "dead rows may only be dropped down to the oldest table"
        if m is None:
            m = TIERS[min(2, max(t.tier for t in ins) + 1)][0]
        # one key per input position whose line wins and stays, for the next read
        drop = kind == "live" or drop_dead
        seen = {}
        for k, (v, r) in sorted(Model.positions([t.rows for t in ins], kind).items()):
            pos = "first" if r == 0 else "last" if r == len(ins) - 1 else "inner"
            if not (drop and is_dead(v)):
                seen.setdefault(pos, []).append(k)
        self.witness += [ks[int(self.rng.integers(0, len(ks)))] for _, ks in sorted(seen.items())]
        op = {"op": "compact", "i": i, "j": j, "kind": kind, "m": m, "drop_dead": drop_dead, "defer": defer,
              "probe": None}
        out = self._emit(op)
        op["probe"] = [] if defer else self._probe()
        return out

    # -- scans --
    def draw_ranges(self, one=False, cover=False):
        """{"ranges": ...} or {"prefixes": ...}: ascending and pairwise disjoint."""
        rng = self.rng
        if cover:  # everything, in a few pieces
            if self.family == "ns" or rng.random() < 0.5:
                return {"ranges": None, "prefixes": prefix_choices(self.family, self.pool)[0]}
            cuts = sorted(self.pool[int(i)] for i in rng.choice(len(self.pool), 2, replace=False))
            return {"ranges": [(b"", cuts[0]), (cuts[0], cuts[1]), (cuts[1], None)], "prefixes": None}
        nr = 1 if one else int(rng.choice([1, 2, 3, 6]))
        if rng.random() < 0.4:
            cand = prefix_choices(self.family, self.pool)
            cand = cand[int(rng.integers(0, len(cand)))]
            idx = np.sort(rng.choice(len(cand), min(nr, len(cand)), replace=False))
            return {"ranges": None, "prefixes": [cand[int(i)] for i in idx]}
        cuts = sorted(self.pool[int(i)] for i in rng.choice(len(self.pool), 2 * nr, replace=False))
        ranges = [(cuts[2 * r], cuts[2 * r + 1]) for r in range(nr)]
        if rng.random() < 0.3:
            ranges[-1] = (ranges[-1][0], None)
        if rng.random() < 0.3:
            ranges[0] = (b"", ranges[0][1])
        return {"ranges": ranges, "prefixes": None}

    def rule(self):
        return "lww" if self.regime == "replica" or self.rng.random() < 0.5 else "newest"

    def scan(self, rule=None, live=None, limit=None, **where):
        rng = self.rng
        rule = self.rule() if rule is None else rule
        live = bool(rng.random() < 0.5) if live is None else live
        if limit is None:
            limit = int(rng.choice([0, 0, 1, 7, 300]))
        if rule == "newest" and not live:
            limit = 0  # scan_many has no limit
        if not where:
            where = self.draw_ranges(one=limit > 0)
        self._emit({"op": "scan", "rule": rule, "live": live, "limit": limit, **where})

    def count(self, rule=None, **where):
        self._emit({"op": "count", "rule": self.rule() if rule is None else rule, **(where or self.draw_ranges())})

    def count_where(self, where=None, key_columns=(), skip=None, lww=None, **rng_kw):
        rng = self.rng
        if lww is None:
            lww = self.rule() == "lww"
        if not rng_kw:
            rng_kw = self.draw_ranges(cover=True)
        if where is None:
            where = [("c", "v")]
            if self.family == "ns" and rng_kw["prefixes"] is not None:
                live = self.model.entries("lww" if lww else "newest", live=True)
                pk = live[int(rng.integers(0, len(live)))][0].split(b":", 1)[1].split(b"|")[0]
                where, key_columns = ([("pk", pk.decode())] if rng.random() < 0.5 else where + [("pk", pk.decode())]), KEY_COLUMNS
        self._emit({"op": "count_where", "where": [tuple(w) for w in where], "key_columns": tuple(key_columns),
                    "skip": skip, "lww": bool(lww), **rng_kw})

    # -- the rest --
    def reopen(self, i=None):
        i = int(self.rng.integers(0, len(self.model.tables))) if i is None else i
        op = {"op": "reopen", "i": i, "probe": None}
        self._emit(op)
        op["probe"] = self._probe()

    def churn(self, k=None):
        k = int(self.rng.integers(2, 5)) if k is None else k
        sizes = [int(self.rng.choice([17, 256, 300, 1000])) for _ in range(k)]
        nf = self.nflush
        entries = [sorted(self.draw_entries(n)) for n in sizes]  # thrown away: they never join the store
        self.nflush = nf
        self._emit({"op": "churn", "entries": entries})

    def next_kind(self):
        if not self.kinds:
            kinds = ["lww", "lww_drop"] if self.regime == "replica" else ["newest", "live", "lww", "lww_drop"]
            at = FAMILIES.index(self.family) % len(kinds)  # each family starts the cycle elsewhere
            self.kinds = (kinds[at:] + kinds[:at])[::-1]
        return self.kinds.pop()

    def auto_compact(self):
        """A run of 3 to 5 tables, contiguous in age; a kind that drops dead rows runs down to the oldest."""
        nt = len(self.model.tables)
        kind = self.next_kind()
        run = int(self.rng.integers(3, min(nt, 5) + 1))
        drop = kind in ("live", "lww_drop")
        i = nt - run if drop else int(self.rng.integers(0, nt - run + 1))
        self.compact(i, i + run - 1, "lww" if kind == "lww_drop" else kind, drop_dead=kind == "lww_drop")

    def tail(self):
        """Whatever op kind the history lacks so far, then reads that cover the classes."""
        while sum(op["op"] == "compact" for op in self.ops) < 2:
            while len(self.model.tables) < 3:
                self.flush(n=300)
            self.auto_compact()
            self.read(n=65)
        have = {op["op"] for op in self.ops}
        for kind in ("scan", "count", "count_where", "reopen", "churn"):
            if kind not in have:
                getattr(self, kind)()
        self.flush(n=300, order="shuffled")  # takes the lowest slot a compaction has cleared
        self.read(n=257, ragged_ok=True)   # keys cut short and keys with a byte appended: a ragged batch
        self.read(n=1000, ragged_ok=False)  # every key as long as its source: fixed rows in the 16-byte family
        return self.ops


# ---- the histories --------------------------------------------------------------------

def random_history(name, family, regime, seed):
    b = Builder(name, family, regime, seed)
    rng = b.rng
    forms = ["list", "host", "device"]

    def flush(n=None):
        n = int(rng.choice(FLUSH_SIZES)) if n is None else n
        b.flush(n=n, order="shuffled" if rng.random() < 0.5 else "sorted", form=forms[int(rng.integers(0, 3))])

    for n in (300, int(rng.choice([255, 256, 257])), 1000):
        flush(n)
    b.read(n=257)
    target, big_at, big_done = int(rng.integers(14, 18)), int(rng.integers(5, 10)), False
    while len(b.ops) < target:
        nt = len(b.model.tables)
        if not big_done and len(b.ops) >= big_at:  # once per history: the bin sort
            b.flush(n=BIN_SORT_SIZE, order="shuffled", form=forms[int(rng.integers(0, 3))])
            big_done = True
            continue
        c = rng.random()
        if nt >= 8 or (c < 0.12 and nt >= 3):
            b.auto_compact()
            b.read(n=int(rng.choice([63, 64, 65, 257, 1000])))
        elif c < 0.40:
            flush()
        elif c < 0.62:
            b.read(n=int(rng.choice(READ_SIZES)))
        elif c < 0.72:
            b.scan()
        elif c < 0.79:
            b.count()
        elif c < 0.86:
            b.count_where()
        elif c < 0.93:
            b.reopen()
        else:
            b.churn()
    return b.tail()


def slot_reuse_across_tiers(name, seed):
    """Scripted 1. A goes into tier 0 slot 5 with its zone; the run holding A
    is compacted into tier 1 and slot 5 cleared; B, whose keys and zone lie
    wholly above A's, takes slot 5; A's keys must then come from the merged
    table and B's from B."""
    b = Builder(name, "hex16", "ordered", seed)
    P = len(b.pool)
    for i in range(5):                                   # slots 0 .. 4
        b.flush(n=[17, 256, 16, 300, 255][i], lo=2600 + 400 * i, width=1200, form=["list", "host", "device"][i % 3])
    a = b.flush(n=300, lo=200, width=900, order="shuffled")            # A: slot 5, low keys
    assert (a.tier, a.slot) == (0, 5)
    a_keys = list(a.keys)
    b.read(keys=a_keys[:200] + b.auto_keys(57))
    b.flush(n=257, lo=100, width=1500, form="host")                    # slot 6
    b.flush(n=300, lo=600, width=1500, order="shuffled", form="device")  # slot 7
    b.read(n=65)
    ins, merged = b.compact(0, 2, "newest")                            # the run holding A -> tier 1; slots 5, 6, 7 cleared
    assert a in ins and merged.tier == 1
    bt = b.flush(n=300, lo=P - 1000, width=900)                        # B: slot 5 again, keys above all of A's
    assert (bt.tier, bt.slot) == (0, 5) and bt.keys[0] > a_keys[-1]
    b.read(keys=a_keys[:150] + bt.keys[:150] + b.auto_keys(700))
    b.scan(rule="newest", live=True, limit=0, ranges=[(a_keys[0], a_keys[-1] + b"0")], prefixes=None)
    return b.tail()


def one_list_object(name, seed):
    """Scripted 2. The table list is one object for every call; between calls
    it changes in place by insert (flush), pop (compact) and element
    replacement (reopen, which keeps its length), with a read after each."""
    b = Builder(name, "ns", "ordered", seed)
    for n in (300, 257, 255):
        b.flush(n=n, form="host")
    b.read(n=257)
    b.reopen(1)                # same length, another table at [1]
    b.read(n=257)
    b.reopen(0)
    b.reopen(2)
    b.read(n=64)
    b.flush(n=300)             # insert at the front: every index shifts
    b.read(n=257)
    b.compact(1, 3, "newest")  # [1] replaced, two popped
    b.read(n=257)
    b.flush(n=256, order="shuffled")
    b.flush(n=17)
    b.read(n=65)
    b.compact(0, 2, "lww")     # three tables become one: the length a past call saw comes back
    b.flush(n=300, form="device")
    b.flush(n=255)
    b.read(n=257)
    b.count()
    b.compact(0, 3, "live")    # down to the oldest: one table left
    b.read(n=63)
    b.flush(n=300)
    b.read(n=257)
    return b.tail()


def nothing_waited_for(name, seed):
    """Scripted 3. Three flushes that are not waited for, a compaction over
    those pending tables, the inputs closed, a churn, a fourth flush, and only
    then the first read."""
    b = Builder(name, "long", "ordered", seed)
    b.flush(n=300, order="shuffled", defer=True, lo=1000, width=1500)
    b.flush(n=1000, order="shuffled", defer=True, lo=1500, width=2500)
    b.flush(n=257, order="sorted", defer=True, lo=1200, width=1000)
    b.compact(0, 2, "newest", defer=True)
    b.churn(3)
    b.flush(n=300, order="shuffled", defer=True, lo=4000, width=1000)
    b.read(n=257)
    b.flush(n=256, lo=1100, width=900)
    b.flush(n=300, lo=1400, width=900, form="device")
    b.read(n=1000)
    return b.tail()


def a_tombstones_life(name, seed):
    """Scripted 4. Put, flush, delete, flush; a newest-wins compaction keeps
    the tombstone and get returns its 8 bytes; compact_live down to the
    oldest table drops the key; then (timestamps no longer following table
    order) a newer table re-puts the key with an older timestamp than a
    tombstone below it, so newest-wins and LWW answers differ for that key."""
    b = Builder(name, "ns", "replica", seed)
    key = b.pool[len(b.pool) // 2]
    around = dict(lo=len(b.pool) // 2 - 450, width=900)

    def others(n):
        return [e for e in b.draw_entries(n, **around) if e[0] != key][:n - 1]
    b.flush(entries=others(300) + [b.put(key, b'{"c":"v"}', ts=1000)])
    b.read(keys=[key] + b.auto_keys(63))
    b.flush(entries=others(257) + [b.delete(key, ts=2000)])
    b.flush(entries=others(256))
    b.read(keys=[key] + b.auto_keys(63))
    b.compact(0, 2, "newest")                      # the tombstone stays
    assert is_dead(b.model.tables[0].rows[key])
    b.read(keys=[key] + b.auto_keys(64))           # get returns the 8 bytes
    b.flush(entries=others(300))
    b.flush(entries=others(255))
    b.compact(0, 2, "live")                        # down to the oldest: the key is gone
    assert not b.held(key)
    b.read(keys=[key] + b.auto_keys(64))
    b.flush(entries=others(300) + [b.delete(key, ts=5000)])
    b.flush(entries=others(257))
    b.flush(entries=others(300) + [b.put(key, b'{"c":"v"}', ts=4000)])  # newer table, older timestamp
    b.read(keys=[key] + b.auto_keys(64))
    one = dict(ranges=[(key, key + b"\0")], prefixes=None)
    pre = dict(ranges=None, prefixes=[key[:4]])
    for rule in ("newest", "lww"):                 # live under newest-wins, dead under LWW
        b.count(rule=rule, **one)
        b.scan(rule=rule, live=True, limit=0, **one)
        b.scan(rule=rule, live=False if rule == "lww" else True, limit=0, **pre)
        b.count_where(where=[("c", "v")], lww=rule == "lww", **pre)
    b.compact(0, 3, "lww", drop_dead=True)         # the LWW fold drops it for good
    assert not b.held(key)
    b.read(keys=[key] + b.auto_keys(64))
    return b.tail()


SEEDS = {}
HISTORIES = {}
for _f in FAMILIES:
    for _r in REGIMES:
        _n = f"random-{_f}-{_r}"
        SEEDS[_n] = 1000 + 10 * FAMILIES.index(_f) + REGIMES.index(_r)
        HISTORIES[_n] = (lambda name, seed, f=_f, r=_r: random_history(name, f, r, seed))
for _n, _fn, _s in (("slot-reuse-across-tiers", slot_reuse_across_tiers, 21), ("one-list-object", one_list_object, 22),
                    ("nothing-waited-for", nothing_waited_for, 23), ("a-tombstones-life", a_tombstones_life, 24)):
    SEEDS[_n], HISTORIES[_n] = _s, _fn
NAMES = list(HISTORIES)
RANDOM = [n for n in NAMES if n.startswith("random-")]
FAMILY = {n: n.split("-")[1] for n in RANDOM}
FAMILY.update({"slot-reuse-across-tiers": "hex16", "one-list-object": "ns", "nothing-waited-for": "long",
               "a-tombstones-life": "ns"})
REGIME = {n: n.split("-")[2] for n in RANDOM}
REGIME.update({"slot-reuse-across-tiers": "ordered", "one-list-object": "ordered", "nothing-waited-for": "ordered",
               "a-tombstones-life": "replica"})


def build(name, seed=None):
    """The history of that name: a list of ops, the same for the same name and seed."""
    return HISTORIES[name](name, SEEDS[name] if seed is None else seed)
