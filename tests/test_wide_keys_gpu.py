"""Wide filter sets (more than 64 slots) with the product's keys and at the
row edges: the zone gate's byte-compare branch, the 16-byte compare against
bounds of every length, the fused walk with ragged and fixed-length batches,
a window in a row's last word, mixed group kinds, 4096 slots, the zero-copy
probe, the restart path and the probe kernel's edges.

The reference's keys are strings "ns:pk|ck" (ragged, long shared prefixes);
every table's filter is m = 1024 and Database::get walks the tables newest
first, each behind zone_map.contains && bloom.may_contain. Every GPU test
compares the HIP path with the C oracle bit for bit; no comparison here is a
tolerance. The workload (helpers below, one seed) is checked for non-vacuity
on the CPU by test_wide_workload_is_not_vacuous, and the GPU tests use the
same cached workload object.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle

SEED = 102464
NT, PER, M = 130, 256, 1024
NS = (b"users", b"events", b"warehouses")
LONG16 = b"warehouses:pk999"  # the 16 bytes the long keys share
PAD = b"|ck0123456789abcdefghijklmnop"  # what a short key is continued with in a fixed-length batch


def _ragged(keys):
    offs = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=offs[1:])
    data = np.frombuffer(b"".join(keys), np.uint8).copy() if offs[-1] else np.zeros(1, np.uint8)
    return data, offs


def _fixed(keys, length, exact=False):
    """keys as one fixed-length batch: (uint8[n, length], its bytes, its offsets).
    exact: only the keys of that length; else every key continued or cut to it."""
    rows = [k for k in keys if len(k) == length] if exact else [(k + PAD)[:length] for k in keys]
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, length).copy()
    return a, np.ascontiguousarray(a.reshape(-1)), np.arange(0, length * (len(a) + 1), length, dtype=np.uint64)


def _pool():
    """(the special keys, the whole pool): ~36K distinct keys shaped like the
    product's, so most share 8 or more leading bytes."""
    special = [b"", b"a", b"users:", b"users:pk"]
    special += [s.encode() for s in ("users:ключ|ck001", "événements:pk00007|ck", "日本:pk00001|値", "users:pk00001|ñ",
                                     "warehouses:pk00002|ÿ", "ünïcode")]
    special += [LONG16 + b"%02d|ck%03d/" % (i, i) + b"x" * (20 + i) for i in range(20)]  # 45..64 bytes
    keys = [ns + b":" + b"pk%05d" % pk + b"|" + (b"ck%03d" % (pk * 7 % 1000))[:cut]
            for ns in NS for pk in range(2000) for cut in range(6)]
    return special, special + keys


@functools.lru_cache(maxsize=None)
def _workload():
    """130 tables of 256 entries (values of 0..29 bytes) and 6500 lookups, with
    the oracle's filter, zone and table of each; built once per process."""
    rng = np.random.default_rng(SEED)
    special, pool = _pool()
    assert len(set(pool)) == len(pool) and not any(b"\t" in k or b"\n" in k for k in pool)
    entries = []
    for t in range(NT):
        keys = [pool[i] for i in rng.choice(len(pool), PER, replace=False)]
        if t % 4 == 0 and t // 4 < len(special) and special[t // 4] not in keys:
            keys[0] = special[t // 4]  # every special key lives in some table
        vlen = rng.integers(0, 30, PER)
        entries.append(sorted((k, bytes(rng.integers(0, 256, int(n), dtype=np.uint8))) for k, n in zip(keys, vlen)))
    zones = [(e[0][0], e[-1][0]) for e in entries]
    bounds = [b for z in zones for b in z]
    present = special + bounds
    present += [pool[i] for i in rng.integers(0, len(pool), 5000 - len(present))]
    nul = [present[i] + b"\0" for i in rng.choice(5000, 500, replace=False)]
    cut = [present[i][:-1] for i in rng.choice(5000, 500, replace=False)]
    absent = [(b"accounts", b"users", b"zones")[i % 3] + b":pk%05d|" % (20000 + i) + (b"ck%03d" % (i % 1000))[: i % 6]
              for i in range(500)]
    assert not {k for e in entries for k, _ in e} & set(absent)
    look = present + nul + cut + absent
    look = [look[i] for i in rng.permutation(len(look))]
    data, offs = _ragged(look)
    ofs, ozs, files, ots = [], [], [], []
    for t, e in enumerate(entries):
        o = oracle.OracleFilter(M)
        o.insert_var(*_ragged([k for k, _ in e]))
        ofs.append(o)
        ozs.append(oracle.OracleZone(*zones[t]))
        files.append(oracle.sstable_create(e))
        ots.append(oracle.OracleTable(files[-1]))
    return SimpleNamespace(special=special, pool=pool, entries=entries, zones=zones, look=look, absent=absent,
                           data=data, offs=offs, ofs=ofs, ozs=ozs, files=files, ots=ots)


def _expect_walk(w, order, data, offs, gated=True):
    """The oracle's Database::get over the tables `order` (ids, newest first):
    the gate rows (zone && bloom; `gated`: one flag, or one per position, says
    which tables have a zone), then the newest-first walk."""
    on = [gated] * len(order) if isinstance(gated, bool) else list(gated)
    gate = oracle.probe_gated([w.ofs[t] for t in order], [w.ozs[t] if g else None for t, g in zip(order, on)],
                              data, offs)
    return gate, oracle.get_many([w.ots[t] for t in order], gate, data, offs)


def _popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


def test_wide_workload_is_not_vacuous():
    """The helpers and the oracle only: what keeps the GPU tests below
    meaningful. Figures of this workload: 3376 of 6500 lookups found, 3050
    found keys with an earlier gate candidate the search rejected, 11309 bits
    between the gated and the plain rows; the floors sit well under them."""
    w = _workload()
    assert w is _workload()  # one cached object: the GPU tests see these seeds' tables and lookups
    n = len(w.look)
    assert n == 6500 and len(w.entries) == NT and all(len(e) == PER for e in w.entries)
    vl = {len(v) for e in w.entries for _, v in e}
    assert vl == set(range(30))  # both sides of the 18-byte small decode, and length 0
    order = list(range(NT))[::-1]
    gate, (which, voff, vals) = _expect_walk(w, order, w.data, w.offs)
    found = which >= 0
    print("found", int(found.sum()), "of", n)
    assert found.sum() * 4 >= n
    assert set(np.unique(which[found] // 64)) == {0, 1, 2}  # every group of 64 holds a found key
    bits = np.unpackbits(gate.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    first = np.where(bits.any(axis=0), bits.argmax(axis=0), NT)  # the newest table whose gate passes
    walked = int((found & (first < which)).sum())
    print("found behind a rejected candidate", walked)
    assert walked >= 1000
    differ = _popcount(gate ^ oracle.probe_var([w.ofs[t] for t in order], w.data, w.offs))
    print("gated rows differ from the plain ones in", differ, "bits")
    assert differ >= 1000
    assert any(0 < len(k) < 8 for k in w.look) and b"" in w.look
    # the fixed-length cases of the walk have keys to find: lookups of exactly 16 and 24 bytes
    for length in (16, 24):
        a, d, o = _fixed(w.look, length, exact=True)
        assert len(a) >= 200 and (_expect_walk(w, order, d, o)[1][0] >= 0).sum() >= 50
    # every table's largest and smallest key is looked up and found (the gate's <= and >= at equality)
    pos = {k: i for i, k in enumerate(w.look)}
    assert all(which[pos[b]] >= 0 for z in w.zones for b in z)


@pytest.fixture(scope="module")
def lsm(gpu):
    """The workload's tables created on the device; the data file and the zone
    bounds are the oracle's."""
    w = _workload()
    tables, blooms = [], []
    for t, e in enumerate(w.entries):
        tb, bloom, zone = gpu.sstable_create(e, m=M)
        assert tb.data() == w.files[t] and (zone.min, zone.max) == w.zones[t]
        tables.append(tb)
        blooms.append(bloom)
    return SimpleNamespace(w=w, tables=tables, blooms=blooms)


def _check_get(gpu, s, tabs, slots, keys, expect):
    which, voff, vals = gpu.get_many(tabs, keys, filterset=s, hit_rows=np.asarray(slots, dtype=np.uint32))
    ow, ovoff, ovals = expect
    assert np.array_equal(np.asarray(which), ow)
    assert np.array_equal(np.asarray(voff, dtype=np.uint64), ovoff) and vals == ovals


# ---- the gate ------------------------------------------------------------------------

_CLASSES = ("own", "prefix", "halfopen", "emptylo", "single", "long")
_EDGE_CLASS = {0: "own", 63: "long", 64: "prefix", 127: "single", 128: "emptylo", 129: "own"}  # all gated


def _gate_zones(w):
    longs = sorted(w.special[-20:])
    zones = []
    for f in range(NT):
        cls = _EDGE_CLASS.get(f, _CLASSES[f % 6])
        lo, hi = w.zones[f]  # the table's own min and max
        if cls == "prefix":
            lo = lo[:1]
        elif cls == "halfopen":  # one bound missing: the slot is not gated (zonemap.rs:40)
            lo, hi = (None, hi) if f % 12 < 6 else (lo, None)
        elif cls == "emptylo":  # a lower bound that is present but empty
            lo, hi = b"", b"\xff"
        elif cls == "single":
            lo = hi = w.entries[f][PER // 2][0]
        elif cls == "long":  # longer than 16 bytes, the first 16 shared with lookups
            lo, hi = longs[f % 7], longs[7 + f % 13]
        zones.append((lo, hi))
    return zones


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1024, 100003])
def test_wide_gate_ragged_keys(gpu, m):
    """wide_zone_ok's byte-compare branch (KEY_VAR, KEY_FIXED) and cmp16 on a
    wide set, with zones of every class on slots below and above 64. Each
    slot's filter also holds the keys next to its own bounds, so the gate's
    answer there shows in the rows whatever the Bloom bits of the table say."""
    import torch
    w = _workload()
    zones = _gate_zones(w)
    assert {_EDGE_CLASS.get(f, _CLASSES[f % 6]) for f in range(64, NT)} == set(_CLASSES)
    edges = [[e for b in z if b is not None for e in (b, b + b"\0", b[:-1])] for z in zones]
    look = w.look + [e for es in edges for e in es]
    filters, refs = [], []
    for f in range(NT):
        keys = [k for k, _ in w.entries[f]] + edges[f] + [(e + PAD)[:ln] for e in edges[f] for ln in (7, 16, 24)]
        kd, ko = _ragged(keys)
        b = gpu.BloomFilter(m)
        b.insert_batch(gpu.KeyBatch(n=len(keys), data=kd, offsets=ko))
        o = oracle.OracleFilter(m)
        o.insert_var(kd, ko)
        filters.append(b)
        refs.append(o)
    s = gpu.FilterSet.from_filters(filters, width=192)
    for i, z in enumerate(zones):
        s.set_zone(i, z)
    ozs = [oracle.OracleZone(lo, hi) for lo, hi in zones]
    data, offs = _ragged(look)
    kb = gpu.KeyBatch(n=len(look), data=data, offsets=offs)
    exp = oracle.probe_gated(refs, ozs, data, offs)
    plain = oracle.probe_var(refs, data, offs)
    assert _popcount(exp ^ plain) >= 1000 and _popcount(exp) >= 1000
    assert np.array_equal(s.probe(kb, gated=True), exp)
    assert np.array_equal(s.probe(kb), plain)
    for length in (7, 24, 16):  # KEY_FIXED twice, then KEY_FIXED16
        a, d, o = _fixed(look, length)
        exp = oracle.probe_gated(refs, ozs, d, o)
        assert _popcount(exp ^ oracle.probe_var(refs, d, o)) >= 100, length
        assert np.array_equal(s.probe(a, gated=True), exp), length
    # the same 16-byte batch behind a data pointer that is not 16-aligned (KEY_FIXED again)
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    buf[1:1 + a.size] = torch.from_numpy(d).cuda()
    dk = buf[1:1 + a.size].view(-1, 16)
    assert dk.data_ptr() % 16 == 1
    out = torch.zeros((NT, (len(a) + 63) // 64), dtype=torch.int64, device="cuda")
    s.probe(gpu.DeviceKeys(dk), out=out, gated=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), exp)


@pytest.mark.gpu
def test_wide_gate_fixed16_bound_lengths(gpu):
    """test_zone_gate_fixed16_bound_lengths's construction on a wide set: 16-byte
    keys against bounds of every length class (empty, inside one word,
    word-aligned, 16, longer than the key), the prefixes and the gated bits
    read from the wide zone table."""
    rng = np.random.default_rng(17)
    alpha = np.frombuffer(b"ab", np.uint8)
    m, nt = 4099, 128
    lens = [0, 1, 3, 4, 5, 8, 11, 15, 16, 17, 20]
    keys = [alpha[rng.integers(0, 2, (3000, 16))] for _ in range(nt)]
    filters, refs, zones = [], [], []
    for f in range(nt):
        b = gpu.BloomFilter(m)
        b.insert_batch(keys[f])
        o = oracle.OracleFilter(m)
        o.insert_fixed(keys[f])
        filters.append(b)
        refs.append(o)
        r = [bytes(x) for x in keys[f][:2]]
        lo = (r[0] + b"abab")[: lens[f % len(lens)]]  # (continued, so 17 and 20 are real lengths)
        hi = (r[1] + b"baba")[: lens[(f * 7 + 3) % len(lens)]]
        if lo > hi:
            lo, hi = hi, lo
        zones.append((lo, hi))
    # every length class also on a slot >= 64 (the smaller bound of a pair is the lower one: no empty upper bound)
    assert {len(lo) for lo, _ in zones[64:]} == set(lens) and {len(hi) for _, hi in zones[64:]} == set(lens) - {0}
    s = gpu.FilterSet(m, width=128)
    s.assign_all(filters)
    for i, z in enumerate(zones):
        s.set_zone(i, z)
    look = alpha[rng.integers(0, 2, (12_000, 16))]
    look[: 2 * nt] = [np.frombuffer((b + b"a" * 16)[:16], np.uint8) for z in zones for b in z]
    d = np.ascontiguousarray(look.reshape(-1))
    offs = np.arange(0, 16 * (len(look) + 1), 16, dtype=np.uint64)
    exp = oracle.probe_gated(refs, [oracle.OracleZone(lo, hi) for lo, hi in zones], d, offs)
    assert exp.any() and not np.array_equal(exp, oracle.probe_fixed(refs, look))
    assert np.array_equal(s.probe(look, gated=True), exp)


# ---- the fused walk ------------------------------------------------------------------

def _slots_of(mapping):
    """The slot of each table position (newest first) of a 192-slot set."""
    rng = np.random.default_rng(SEED + 4)
    if mapping == "descending":  # slot = age, walked .rev(): the LSM's own order
        return np.arange(NT)[::-1].copy()
    if mapping == "ascending":
        return np.arange(NT)
    if mapping == "scattered":
        return rng.permutation(192)[:NT]
    # mixed: group 0 descending (slots 133..70: a window across two words), group 1
    # scattered, the short last group ascending in the row's last word (slots 190, 191)
    g0, g2 = 133 - np.arange(64), np.array([190, 191])
    g1 = rng.permutation(np.setdiff1d(np.arange(192), np.concatenate([g0, g2])))[:64]
    return np.concatenate([g0, g1, g2])


@pytest.mark.gpu
@pytest.mark.parametrize("mapping,batch", [("descending", "ragged"), ("ascending", "ragged"), ("scattered", "ragged"),
                                           ("mixed", "ragged"), ("mixed", "fixed")])
def test_wide_get_many_ragged_keys(gpu, lsm, mapping, batch):
    """k_wide_get_many<KEY_VAR> (and, batch == "fixed", <KEY_FIXED16> and
    <KEY_FIXED> with the lookups of exactly 16 and 24 bytes) over the 130
    tables, every table's zone set, for each table -> slot mapping; one call
    mixes the three group kinds. Twice: the second call reuses the screen."""
    w = lsm.w
    order = list(range(NT))[::-1]  # table NT - 1 is the newest
    slots = _slots_of(mapping)
    assert len(set(slots.tolist())) == NT and slots.max() < 192
    s = gpu.FilterSet(M, width=192)
    for p, t in enumerate(order):
        s.assign(int(slots[p]), lsm.blooms[t])
        s.set_zone(int(slots[p]), w.zones[t])
    tabs = [lsm.tables[t] for t in order]
    if batch == "ragged":
        batches = [(gpu.KeyBatch(n=len(w.look), data=w.data, offsets=w.offs), w.data, w.offs)]
    else:
        batches = [_fixed(w.look, 16, exact=True), _fixed(w.look, 24, exact=True)]
    for keys, data, offs in batches:
        gate, expect = _expect_walk(w, order, data, offs)
        assert (expect[0] >= 0).sum() >= 50
        for _ in range(2):
            _check_get(gpu, s, tabs, slots, keys, expect)
    if batch == "ragged":  # the gate the walk computed inside, as rows
        got = s.probe(batches[0][0], gated=True)
        assert np.array_equal(got[slots], gate)


@pytest.mark.gpu
def test_wide_window_in_the_last_word(gpu, lsm):
    """wide_window's last-word branch: a window that starts inside the row's
    last word (30 tables on slots 290..319 of a 320-slot set, ascending and
    descending), and an aligned one that is the last word (64 tables on slots
    256..319), gated and without zones, 16-byte and ragged lookups. Every slot
    of the set holds some table's filter, so a window taken from the wrong
    place gives another table's bits."""
    w = lsm.w
    width = 320
    table_of = [sl % NT for sl in range(width)]
    sets = {}
    for gated in (True, False):
        s = gpu.FilterSet(M, width=width)
        s.assign_all([lsm.blooms[t] for t in table_of])
        if gated:
            for sl, t in enumerate(table_of):
                s.set_zone(sl, w.zones[t])
        sets[gated] = s
    ragged = (gpu.KeyBatch(n=len(w.look), data=w.data, offsets=w.offs), w.data, w.offs)
    for slots in (list(range(290, 320)), list(range(319, 289, -1)), list(range(319, 255, -1))):
        order = [table_of[sl] for sl in slots]
        tabs = [lsm.tables[t] for t in order]
        for keys, data, offs in (ragged, _fixed(w.look, 16, exact=True)):
            for gated in (True, False):
                _, expect = _expect_walk(w, order, data, offs, gated=gated)
                assert (expect[0] >= 0).sum() >= 20
                _check_get(gpu, sets[gated], tabs, slots, keys, expect)


@pytest.mark.gpu
def test_wide_4096_slots(gpu, lsm):
    """The widest set (R = 64 words per row): the probe's loop over 64 words,
    the walk over 64 groups to the last one (a quarter of the lookups are in
    no table), zones on every fifth slot; then 200 tables on the set's last
    slots."""
    w = lsm.w
    width, nd = 4096, 128
    table_of = [sl % nd for sl in range(width)]
    s = gpu.FilterSet(M, width=width)
    s.assign_all([lsm.blooms[t] for t in table_of])
    assert s.used == width
    for sl in range(0, width, 5):
        s.set_zone(sl, w.zones[table_of[sl]])
    absent = set(w.absent)
    look = w.absent + [k for k in w.look if k not in absent][:1500]
    data, offs = _ragged(look)
    kb = gpu.KeyBatch(n=len(look), data=data, offsets=offs)
    slots = list(range(width))[::-1]
    order = [table_of[sl] for sl in slots]
    gate, expect = _expect_walk(w, order, data, offs, gated=[sl % 5 == 0 for sl in slots])
    assert (expect[0] >= 0).sum() >= 500 and (expect[0] < 0).sum() >= 500
    _check_get(gpu, s, [lsm.tables[t] for t in order], slots, kb, expect)
    assert np.array_equal(s.probe(kb, gated=True), gate[::-1])
    slots = list(range(4095, 3895, -1))
    order = [table_of[sl] for sl in slots]
    _, expect = _expect_walk(w, order, data, offs, gated=[sl % 5 == 0 for sl in slots])
    _check_get(gpu, s, [lsm.tables[t] for t in order], slots, kb, expect)


# ---- the probe's edges, the zero-copy probe, the restart path ----------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 33, 1024])
def test_wide_probe_edges(gpu, m):
    """k_wide_probe and k_wide_build at their edges: used at a word of slots
    and one past it, n across the 64-key hit word and the 1024-key workgroup,
    m of 1 and 33 (a last group of 32 positions with one valid row). The hit
    buffer is followed by two more rows and one more word, all pre-filled: the
    probe writes the used rows' ceil(n/64) words and nothing else. (The C ABI's
    row stride is ceil(n/64), so the extra word cannot sit between the rows.)"""
    import torch
    rng = np.random.default_rng(m)
    filters, refs, some = [], [], []
    for f in range(128):
        nk = 0 if f % 5 == 0 else (200 if m == 1024 else 1 + f % 3)
        keys = rng.integers(0, 256, (nk, 16), dtype=np.uint8)
        b = gpu.BloomFilter(m)
        o = oracle.OracleFilter(m)
        if nk:
            b.insert_batch(keys)
            o.insert_fixed(keys)
        filters.append(b)
        refs.append(o)
        some.append(keys[:4])
    look = np.concatenate(some + [rng.integers(0, 256, (1025, 16), dtype=np.uint8)])
    look = np.ascontiguousarray(look[rng.permutation(len(look))[:1025]])
    dlook = torch.from_numpy(look).cuda()
    fill = 0x5A5A5A5A5A5A5A5A
    for used in (64, 65, 127, 128):
        s = gpu.FilterSet(m, width=128)
        s.assign_all(filters[:used])
        assert s.used == used
        for n in (1, 63, 64, 65, 1023, 1024, 1025):
            nw = (n + 63) // 64
            out = torch.full(((used + 2) * nw + 1,), fill, dtype=torch.int64, device="cuda")
            s.probe(gpu.DeviceKeys(dlook[:n]), out=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            exp = oracle.probe_fixed(refs[:used], look[:n])
            assert np.array_equal(got[: used * nw].reshape(used, nw), exp), (used, n)
            assert (got[used * nw:] == np.uint64(fill)).all(), (used, n)
        assert exp.any() and (exp == 0).any()


@pytest.mark.gpu
def test_wide_zero_copy(gpu, lsm):
    """Pinned keys in, pinned hit rows out on a wide set (the probe kernel reads
    and writes them in place): plain and gated, 16-byte keys and another
    length, a last hit word that is not full."""
    import torch
    w = lsm.w
    nf = 128
    s = gpu.FilterSet.from_filters(lsm.blooms[:nf], width=128)
    for f in range(nf):
        s.set_zone(f, w.zones[f])
    for length in (16, 24):
        a, d, o = _fixed(w.look, length)
        n = len(a)
        assert n % 64
        keys = torch.from_numpy(a).pin_memory()
        out = torch.zeros((nf, (n + 63) // 64), dtype=torch.int64).pin_memory()
        s.probe(gpu.KeyBatch(n=n, key_len=length, keys=keys), out=out)
        assert gpu.last_path() == 4
        plain = oracle.probe_fixed(w.ofs[:nf], a)
        assert np.array_equal(out.numpy().view(np.uint64), plain)
        out.zero_()
        s.probe(gpu.KeyBatch(n=n, key_len=length, keys=keys), out=out, gated=True)
        assert gpu.last_path() == 4
        exp = oracle.probe_gated(w.ofs[:nf], w.ozs[:nf], d, o)
        assert _popcount(exp ^ plain) >= 100
        assert np.array_equal(out.numpy().view(np.uint64), exp)


@pytest.mark.gpu
def test_wide_load_meta(gpu):
    """The restart path into a wide set: every slot, those from 64 up included,
    filled from a table's .meta as the oracle encodes it (filter bits and zone
    map; some tables without a zone map). A truncated .meta leaves the set as
    it was."""
    w = _workload()
    nf = 128
    s = gpu.FilterSet(M, width=128)
    ozs = [None if f % 9 == 4 else w.ozs[f] for f in range(nf)]
    for f in range(nf):
        s.load_meta(f, oracle.meta_encode(w.ofs[f], ozs[f]))
    assert s.used == nf
    kb = gpu.KeyBatch(n=len(w.look), data=w.data, offsets=w.offs)
    exp = oracle.probe_gated(w.ofs[:nf], ozs, w.data, w.offs)
    plain = oracle.probe_var(w.ofs[:nf], w.data, w.offs)
    assert _popcount(exp ^ plain) >= 1000
    assert np.array_equal(s.probe(kb, gated=True), exp)
    assert np.array_equal(s.probe(kb), plain)
    meta = oracle.meta_encode(w.ofs[3], w.ozs[3])
    for slot in (5, 100):
        with pytest.raises(ValueError):
            s.load_meta(slot, meta[: len(meta) // 2])
        with pytest.raises(ValueError):
            s.load_meta(slot, b"\x0a\x05\x0a\x03\x01")
    assert np.array_equal(s.probe(kb, gated=True), exp)
    assert np.array_equal(s.probe(kb), plain)
