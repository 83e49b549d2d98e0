"""The store model (tests/store_model.py) against independent witnesses, and
the conditions that keep tests/test_store_gpu.py from hiding a failure. No GPU.

Witnesses, for every history and after every op: the model's get equals the
C oracle's walk (oracle.get_many) over the model's files, ungated and gated
with oracle.probe_gated rows from OracleFilters at each table's own m and its
OracleZone; a newest-wins compaction's file equals oracle.sstable_create of
the oracle's walk over the inputs' files (the way test_compact_gpu.expected
computes it).

Conditions, each computed from the history and the oracle alone: if a seed
loses one, the seed or the generator changes until this test passes again;
the GPU test's strength rests on them.
"""
import functools

import numpy as np
import pytest

import store_model as sm
from liverow_ref import is_dead
from merge_help import file_keys, ragged
from oracle import oracle

CLASSES = ("newest", "fell-through", "zone-rejected", "tombstone", "absent")


def bits(rows, n):
    h = np.ascontiguousarray(rows, dtype="<u8")
    return np.unpackbits(h.view(np.uint8).reshape(h.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def check_get(model, keys, what):
    """model.get against the oracle's walk, ungated and gated; returns the
    model's which and the oracle's (bloom bits, gate bits) as bool[nt, n]."""
    which, voff, vals = model.get(keys)
    d, o = ragged(keys)
    otables = [t.otable for t in model.tables]
    filters, zones = [t.ofilter() for t in model.tables], [t.ozone() for t in model.tables]
    ou, og = oracle.probe_var(filters, d, o), oracle.probe_gated(filters, zones, d, o)
    for gate in (None, og):
        ow, ovoff, ovals = oracle.get_many(otables, gate, d, o)
        assert np.array_equal(which, ow) and np.array_equal(voff, ovoff) and vals == ovals, \
            f"{what}: the model's get differs from the oracle's walk ({'gated' if gate is not None else 'ungated'})"
    return which, bits(ou, len(keys)), bits(og, len(keys))


def check_newest_compaction(ins, merged, what):
    files = [t.file for t in ins]
    keys = sorted(set(k for f in files for k in file_keys(f)))
    kd, ko = ragged(keys)
    which, voff, vals = oracle.get_many([oracle.OracleTable(f) for f in files], None, kd, ko)
    entries = [(k, vals[int(voff[i]):int(voff[i + 1])]) for i, k in enumerate(keys) if which[i] >= 0]
    assert merged.file == (oracle.sstable_create(entries) if entries else b""), f"{what}: the model's fold differs"


@functools.lru_cache(maxsize=None)
def walk(name, drop_class=None):
    """Replays the history through the model, checking the witnesses at every
    step, and returns what the conditions need. drop_class: leave the read
    keys of that class out (to show that a condition notices)."""
    history = sm.build(name)
    model = sm.Model()
    st = {"kinds": set(), "classes": set(), "reuse_open": [], "reuse_read": 0, "compactions": [],
          "lww_not_newest": False, "where": [], "compact_kinds": set(), "bin_sort": 0, "nops": len(history),
          "max_tables": 0, "ragged16": set()}
    keys = None
    for step, op in enumerate(history):
        what = f"{name} step {step} {sm.describe(op)}"
        st["kinds"].add(op["op"])
        before = list(model.tables)
        nreuse = len(model.reuses)
        made = sm.apply(model, op)
        st["max_tables"] = max(st["max_tables"], len(model.tables))
        if op["op"] == "flush":
            st["bin_sort"] += len(op["entries"]) == sm.BIN_SORT_SIZE and op["order"] == "shuffled"
            assert op["order"] == "shuffled" or op["entries"] == sorted(op["entries"]), what
        if op["op"] == "compact":
            ins, merged = made
            assert op["j"] - op["i"] >= 2, f"{what}: a run needs an inner table"
            if op["kind"] == "live" or op["drop_dead"]:
                assert before[-1] is ins[-1], f"{what}: dead rows dropped above the oldest table"
            if op["kind"] == "newest":
                check_newest_compaction(ins, merged, what)
            st["compact_kinds"].add(op["kind"] + ("_drop" if op["drop_dead"] else ""))
            need = {}
            for k, (v, r) in sm.Model.positions([t.rows for t in ins], op["kind"]).items():
                if k in merged.rows:
                    need.setdefault("first" if r == 0 else "last" if r == len(ins) - 1 else "inner", set()).add(k)
            st["compactions"].append([what, need, set()])
        for former, mt in model.reuses[nreuse:]:  # a slot taken again: which of its former keys the new zone excludes
            st["reuse_open"].append({k for k in former if mt.excludes(k)})
        if op["op"] == "read":
            keys = op["keys"]
        elif op.get("probe"):
            keys = op["probe"]
        if keys and model.tables:
            which, ou, og = check_get(model, keys, what)
        if op["op"] == "read":
            nt = len(model.tables)
            newer = np.arange(nt)[:, None] < np.where(which >= 0, which, nt)[None, :]
            dead = np.array([w >= 0 and is_dead(model.tables[w].rows[k]) for k, w in zip(keys, which)])
            cls = {"newest": which == 0, "fell-through": (which > 0) & (og & newer).any(0),
                   "zone-rejected": (ou & ~og & newer).any(0), "tombstone": dead, "absent": which < 0}
            keep = np.ones(len(keys), bool) if drop_class is None else ~cls[drop_class]
            st["classes"] |= {c for c, mask in cls.items() if (mask & keep).any()}
            got = {k for k, ok in zip(keys, keep) if ok}
            st["reuse_read"] += sum(1 for s in st["reuse_open"] if s & got)
            st["reuse_open"] = [s for s in st["reuse_open"] if not s & got]
            for c in st["compactions"]:
                c[2] |= {pos for pos, ks in c[1].items() if ks & got}
            if sm.FAMILY[name] == "hex16":
                st["ragged16"].add(any(len(k) != 16 for k in keys))
        if op["op"] in ("scan", "count", "count_where") or op["op"] == "compact":
            new = {k: r for k, _, r in model.entries("newest")}
            st["lww_not_newest"] |= any(new[k] != r for k, _, r in model.entries("lww"))
        if op["op"] == "count_where":
            rows, off = sm.cut(model.entries("lww" if op["lww"] else "newest", live=True), sm.op_ranges(op))
            st["where"].append((what, len(rows), sum(sm.where_verdicts(op, rows, off))))
        if op["op"] in ("scan", "count", "count_where"):
            r = sm.op_ranges(op)
            assert all(lo <= hi for lo, hi in r[:-1]) and all(a[1] <= b[0] for a, b in zip(r, r[1:])), \
                f"{what}: ranges must ascend and be disjoint"
            if sm.REGIME[name] == "replica" and name in sm.RANDOM:
                assert op.get("rule", "lww") == "lww" and op.get("lww", True), f"{what}: a replica history merges by LWW only"
    return st


@pytest.mark.parametrize("name", sm.NAMES)
def test_model_agrees_with_its_witnesses_and_the_history_is_sound(name):
    st = walk(name)  # (the witnesses are asserted inside, step by step)
    assert st["kinds"] == set(sm.OP_KINDS), f"op kinds missing: {set(sm.OP_KINDS) - st['kinds']}"
    assert st["max_tables"] <= 12
    if name in sm.RANDOM:
        assert 20 <= st["nops"] <= 30 and st["bin_sort"] == 1


@pytest.mark.parametrize("name", sm.NAMES)
def test_reads_fall_in_every_class(name):
    st = walk(name)
    assert st["classes"] == set(CLASSES), f"no read key is {set(CLASSES) - st['classes']}"
    if sm.FAMILY[name] == "hex16":  # both key forms travel: fixed [n, 16] rows and ragged batches
        assert st["ragged16"] == {False, True}


@pytest.mark.parametrize("name", sm.NAMES)
def test_a_reused_slots_former_keys_are_read(name):
    """A slot is taken again by a table whose zone excludes a key of the
    slot's former table, and that key is read afterwards."""
    assert walk(name)["reuse_read"] >= 1


@pytest.mark.parametrize("name", sm.NAMES)
def test_every_input_position_of_every_compaction_is_read(name):
    for what, need, read in walk(name)["compactions"]:
        assert set(need) == {"first", "inner", "last"}, f"{what}: no surviving winner from {set(need)}"
        assert read == set(need), f"{what}: winners from {set(need) - read} are never read"


@pytest.mark.parametrize("name", sm.NAMES)
def test_where_counts_are_neither_nothing_nor_everything(name):
    counts = walk(name)["where"]
    assert any(0 < matched < live for _, live, matched in counts), counts


@pytest.mark.parametrize("name", [n for n in sm.NAMES if sm.REGIME[n] == "replica"])
def test_replica_histories_have_a_winner_that_is_not_the_newest_line(name):
    assert walk(name)["lww_not_newest"]


def test_every_compaction_kind_occurs_in_an_ordered_history():
    kinds = set().union(*(walk(n)["compact_kinds"] for n in sm.NAMES if sm.REGIME[n] == "ordered"))
    assert kinds >= {"newest", "live", "lww", "lww_drop"}, kinds


def test_histories_are_deterministic():
    for name in sm.NAMES:
        assert sm.build(name) == sm.build(name), name
    assert sm.build(sm.NAMES[0], seed=5) != sm.build(sm.NAMES[0], seed=6)


def test_the_class_condition_notices_a_missing_class():
    """Without its false-positive fall-throughs a history no longer passes."""
    assert "fell-through" not in walk(sm.NAMES[0], drop_class="fell-through")["classes"]
