"""Tiered filter sets on the GPU: cb_tiers_probe_* (probe_tiers) and
cb_tiers_get_many_* (get_many_tiers) over FilterSets of different m, every
check an exact comparison with the C oracle (oracle.probe_gated /
oracle.probe_var with each table's filter at its own m, oracle.get_many over
those gate rows).

The shape is the store after a compaction: small m = 1024 filters that are
nearly saturated (so false positives are certain), a large power-of-two
filter standing in for a compacted table, and a non-power-of-two one that
forces the 64-bit hash state.
"""
import base64
import ctypes

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

ALPHA = np.frombuffer(b"0123456789abcdef", np.uint8)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def ragged(items):
    offs = np.zeros(len(items) + 1, np.uint64)
    if items:
        np.cumsum([len(x) for x in items], out=offs[1:])
    data = np.frombuffer(b"".join(items), np.uint8).copy() if offs[-1] else np.zeros(1, np.uint8)
    return data, offs


def make_keys(rng, n, kind):
    """n distinct keys, sorted (Rust str order = bytes order)."""
    out = set()
    while len(out) < n:
        ln = 16 if kind == "k16" else 11 if kind == "k11" else int(rng.integers(1, 25))
        out.add(bytes(ALPHA[rng.integers(0, 16, ln)]))
    return sorted(out)


def batch(gpu, keys, kind):
    """A key list the way its kind travels: fixed rows or a ragged batch."""
    if kind == "ragged":
        d, o = ragged(keys)
        return gpu.KeyBatch(n=len(keys), data=d, offsets=o)
    kl = 16 if kind == "k16" else 11
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), kl).copy()


def table_file(keys, t):
    return b"".join(k + b"\t" + base64.b64encode(b"%d:" % t + k[::-1]) + b"\n" for k in keys)


def bits(rows, n):
    """uint64[nt, words] -> bool[nt, n]."""
    h = np.ascontiguousarray(rows, dtype="<u8")
    return np.unpackbits(h.view(np.uint8).reshape(h.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


class Case:
    """Tables (newest first) over tiered sets, with their oracle twins."""

    def __init__(self, gpu, kind, tier_shapes, table_tiers, slots, sizes, seed, pool_n, windows):
        rng = np.random.default_rng(seed)
        self.gpu, self.kind = gpu, kind
        self.pool = make_keys(rng, pool_n, kind)
        self.tiers = np.asarray(table_tiers, np.uint32)
        self.slots = np.asarray(slots, np.uint32)
        self.nt = len(table_tiers)
        self.sets = [gpu.FilterSet(m, width=w) for m, w in tier_shapes]
        self.keys, self.tables, self.otables, self.ofilters, self.ozones = [], [], [], [], []
        for t in range(self.nt):
            m = tier_shapes[table_tiers[t]][0]
            lo = int(rng.integers(0, pool_n - windows[t] + 1))
            idx = np.sort(rng.choice(windows[t], sizes[t], replace=False)) + lo
            ks = [self.pool[i] for i in idx]
            self.keys.append(ks)
            f = table_file(ks, t)
            self.tables.append(gpu.Table(f))
            self.otables.append(oracle.OracleTable(f))
            of = oracle.OracleFilter(m)
            for k in ks:
                of.insert(k)
            self.ofilters.append(of)
            b = gpu.BloomFilter(m)
            b.insert_batch(batch(gpu, ks, kind))
            st = self.sets[table_tiers[t]]
            st.assign(int(slots[t]), b)
            if t % 2 == 0:  # every other table carries a zone, the rest accept every key
                st.set_zone(int(slots[t]), (ks[0], ks[-1]))
                self.ozones.append(oracle.OracleZone(ks[0], ks[-1]))
            else:
                self.ozones.append(None)
        self.keysets = [set(ks) for ks in self.keys]
        absent = [k for k in make_keys(rng, 1500, kind) if not any(k in s for s in self.keysets)]
        look = [self.pool[i] for i in rng.choice(pool_n, 2500, replace=False)] + absent
        if kind == "ragged":  # the empty key and keys cut short
            look += [b""] + [k[: len(k) // 2] for k in look[:300]]
        rng.shuffle(look)
        self.look = look

    def oracle_gate(self, look, gated=True, zones=None):
        d, o = ragged(look)
        if gated:
            return oracle.probe_gated(self.ofilters, zones or self.ozones, d, o)
        return oracle.probe_var(self.ofilters, d, o)

    def oracle_get(self, look, gate):
        d, o = ragged(look)
        return oracle.get_many(self.otables, gate, d, o)

    def probe(self, look, gated=True, **kw):
        return self.gpu.probe_tiers(self.sets, self.tiers, self.slots, batch(self.gpu, look, self.kind), gated=gated,
                                    **kw)

    def get(self, look, **kw):
        return self.gpu.get_many_tiers(self.tables, self.sets, self.tiers, self.slots,
                                       batch(self.gpu, look, self.kind), **kw)


BASE_TIERS = [(1024, 32), (1_000_003, 64), (1 << 20, 32)]
BASE_TABLE_TIERS = [0, 1, 0, 2, 0, 1, 0, 0]          # the table order interleaves the tiers
BASE_SLOTS = [7, 63, 3, 17, 30, 5, 0, 12]            # permuted slots
BASE_SIZES = [300, 1500, 310, 1500, 290, 1480, 305, 295]
BASE_WINDOWS = [2500, 5000, 2500, 5000, 2500, 5000, 2500, 2500]


@pytest.fixture(scope="module", params=["k16", "k11", "ragged"])
def base(request, gpu):
    return Case(gpu, request.param, BASE_TIERS, BASE_TABLE_TIERS, BASE_SLOTS, BASE_SIZES, seed=31,
                pool_n=8000, windows=BASE_WINDOWS)


@pytest.fixture(scope="module")
def base16(gpu):
    return Case(gpu, "k16", BASE_TIERS, BASE_TABLE_TIERS, BASE_SLOTS, BASE_SIZES, seed=32, pool_n=8000,
                windows=BASE_WINDOWS)


def test_gate_exact(base):
    """probe_tiers equals the oracle's gate row for row (gated and not), and
    each row equals the matching slot row of its own tier's FilterSet.probe;
    16-byte, fixed 11-byte and ragged keys."""
    c, n = base, len(base.look)
    og, ou = c.oracle_gate(c.look), c.oracle_gate(c.look, gated=False)
    # the oracle rows are not vacuous: set and clear bits in every tier, the
    # zone removes Bloom candidates, and some gate bits are false positives
    bg, bu = bits(og, n), bits(ou, n)
    for tier in range(len(c.sets)):
        rows = bg[c.tiers == tier]
        assert rows.any() and not rows.all(), tier
    assert (bu & ~bg).any()
    member = np.array([[k in s for k in c.look] for s in c.keysets])
    assert (bg & ~member).any()
    assert (bg[c.tiers == 0] & ~member[c.tiers == 0]).sum() > 50  # the saturated m = 1024 tier
    assert np.array_equal(c.probe(c.look, gated=True), og)
    assert np.array_equal(c.probe(c.look, gated=False), ou)
    kb = batch(c.gpu, c.look, c.kind)
    for gated, want in ((True, og), (False, ou)):
        own = [s.probe(kb, gated=gated) for s in c.sets]
        for t in range(c.nt):
            assert np.array_equal(own[c.tiers[t]][c.slots[t]], want[t]), (gated, t)


def test_fused_get_exact(base):
    """get_many_tiers equals the oracle's walk over the oracle's gate rows, and
    get_many fed probe_tiers' rows."""
    c, n = base, len(base.look)
    og = c.oracle_gate(c.look)
    ow, ovoff, ovals = c.oracle_get(c.look, og)
    bg = bits(og, n)
    member = np.array([[k in s for k in c.look] for s in c.keysets])
    for tier in range(len(c.sets)):  # keys found in a table of each tier
        assert np.isin(ow, np.flatnonzero(c.tiers == tier)).any(), tier
    assert (ow < 0).any()
    # keys that fall through a false positive to an older table
    newer_fp = np.array([(bg[:w, k] & ~member[:w, k]).any() if w > 0 else False for k, w in enumerate(ow)])
    assert newer_fp.any()
    which, voff, vals = c.get(c.look)
    assert np.array_equal(which, ow) and np.array_equal(voff, ovoff) and vals == ovals
    w2, v2, vals2 = c.gpu.get_many(c.tables, batch(c.gpu, c.look, c.kind), hits=c.probe(c.look))
    assert np.array_equal(w2, ow) and np.array_equal(v2, ovoff) and vals2 == ovals


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_batch_edges(base16, n):
    """The wave, get-block and probe-block edges, consecutive calls on one
    stream; tail bits of the last hit word are zero in a pre-filled buffer."""
    c = base16
    look = c.look[:n]
    og = c.oracle_gate(look)
    out = np.full(og.shape, ALL, np.uint64)
    got = c.probe(look, out=out)
    assert got is out and np.array_equal(out, og)
    if n % 64:
        assert not (out[:, -1] >> np.uint64(n % 64)).any()
    ow, ovoff, ovals = c.oracle_get(look, og)
    which, voff, vals = c.get(look)
    assert np.array_equal(which, ow) and np.array_equal(voff, ovoff) and vals == ovals


@pytest.fixture(scope="module", params=["k16", "ragged"])
def small(request, gpu):
    """Two tiers of the product's filter size and its odd neighbour."""
    return Case(gpu, request.param, [(1000, 32), (1024, 64)], [0, 1, 0, 1], [3, 40, 31, 63], [60, 60, 60, 60],
                seed=33, pool_n=3000, windows=[300, 300, 300, 300])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_host_keys_into_device_hits(small, n):
    """Host keys (staged by the library) with the gate rows written in place
    to device memory: the call returns only once the staged keys have been
    read, so the caller may reuse its key buffer at once."""
    import torch
    c = small
    look = c.look[:n]
    for gated in (True, False):
        want = c.oracle_gate(look, gated=gated)
        kb = batch(c.gpu, look, c.kind)
        hits = torch.full((c.nt, (n + 63) // 64), -1, dtype=torch.int64, device="cuda")
        c.gpu.probe_tiers(c.sets, c.tiers, c.slots, kb, gated=gated, out=hits)
        for a in (kb.data, kb.offsets) if c.kind == "ragged" else (kb,):
            a[:] = 0
        torch.cuda.synchronize()
        assert np.array_equal(hits.cpu().numpy().view(np.uint64), want), gated


def test_one_tier_equals_the_set_calls(gpu, base16):
    """ns = 1: bit for bit cb_set_probe_gated_* / cb_set_get_many_* on that set."""
    c = base16
    sel = [t for t in range(c.nt) if c.tiers[t] == 0]
    st, slots = c.sets[0], c.slots[sel]
    tables = [c.tables[t] for t in sel]
    kb = batch(gpu, c.look, "k16")
    zeros = np.zeros(len(sel), np.uint32)
    for gated in (True, False):
        rows = gpu.probe_tiers([st], zeros, slots, kb, gated=gated)
        assert np.array_equal(rows, st.probe(kb, gated=gated)[slots]) and rows.any()
    a = gpu.get_many_tiers(tables, [st], zeros, slots, kb)
    b = gpu.get_many(tables, kb, filterset=st, hit_rows=slots)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert (a[0] >= 0).any() and (a[0] < 0).any()


@pytest.fixture(scope="module")
def eight(gpu):
    ms = [1024, 4096, 1_000_003, 1 << 16, 1024, 4096, 1_000_003, 1 << 16]
    shapes = [(m, 32 if i % 2 else 64) for i, m in enumerate(ms)]
    rng = np.random.default_rng(8)
    table_tiers = [int(x) for x in rng.permutation(np.repeat(np.arange(8), 8))]
    slots = np.zeros(64, np.int64)
    for i in range(8):
        mine = [t for t in range(64) if table_tiers[t] == i]
        slots[mine] = rng.permutation(shapes[i][1])[:8]
    return Case(gpu, "k16", shapes, table_tiers, slots, [100] * 64, seed=88, pool_n=4000, windows=[800] * 64)


def test_eight_tiers_sixty_four_tables(eight):
    """ns = 8, nt = 64 (the 64-bit hash state: two tiers are not powers of two)."""
    c = eight
    og = c.oracle_gate(c.look)
    assert np.array_equal(c.probe(c.look), og)
    assert np.array_equal(c.probe(c.look, gated=False), c.oracle_gate(c.look, gated=False))
    ow, ovoff, ovals = c.oracle_get(c.look, og)
    which, voff, vals = c.get(c.look)
    assert np.array_equal(which, ow) and np.array_equal(voff, ovoff) and vals == ovals
    assert len(set(ow[ow >= 0])) > 32 and (ow < 0).any()


def test_hash_state_modes_and_unreferenced_set(gpu, eight):
    """The power-of-two tiers alone (the 32-bit state), then with the tables of
    one non-power-of-two tier added (the 64-bit state): both exact on the same
    keys. A set that no table names changes nothing."""
    c = eight
    kb = batch(gpu, c.look, "k16")
    d, o = ragged(c.look)

    def run(keep_tiers, sets, remap):
        sel = [t for t in range(c.nt) if c.tiers[t] in keep_tiers]
        tiers = np.asarray([remap[c.tiers[t]] for t in sel], np.uint32)
        slots = c.slots[sel]
        og = oracle.probe_gated([c.ofilters[t] for t in sel], [c.ozones[t] for t in sel], d, o)
        ow, ovoff, ovals = oracle.get_many([c.otables[t] for t in sel], og, d, o)
        assert np.array_equal(gpu.probe_tiers(sets, tiers, slots, kb), og)
        which, voff, vals = gpu.get_many_tiers([c.tables[t] for t in sel], sets, tiers, slots, kb)
        assert np.array_equal(which, ow) and np.array_equal(voff, ovoff) and vals == ovals
        return og, which

    pow2 = [0, 1, 3, 4, 5, 7]
    remap = {tier: i for i, tier in enumerate(pow2)}
    g32, w32 = run(pow2, [c.sets[i] for i in pow2], remap)
    plus = pow2 + [2]
    run(plus, [c.sets[i] for i in plus], {tier: i for i, tier in enumerate(plus)})
    # all eight sets passed, the two non-power-of-two ones named by no table
    g8, w8 = run(pow2, c.sets, {tier: tier for tier in range(8)})
    assert np.array_equal(g8, g32) and np.array_equal(w8, w32)


def test_async_form(gpu, base16):
    """total = NULL with device buffers: val_off[n] and the values equal the
    synchronous call's once the stream has run."""
    import torch
    from lsmt_amd import _lib
    c = base16
    ew, evoff, evals = c.get(c.look)
    n = len(c.look)
    dk = torch.from_numpy(batch(gpu, c.look, "k16")).cuda()
    which = torch.zeros(n, dtype=torch.int32, device="cuda")
    voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    vals = torch.zeros(len(evals) + 64, dtype=torch.uint8, device="cuda")
    out = gpu.get_many_tiers(c.tables, c.sets, c.tiers, c.slots, gpu.DeviceKeys(dk), out=(which, voff, vals),
                             wait=False)
    assert out[2] is None
    assert _lib.load().cb_stream_synchronize(None) == _lib.CB_OK
    tot = int(voff[-1].item())
    assert tot == len(evals)
    assert np.array_equal(which.cpu().numpy(), ew)
    assert np.array_equal(voff.cpu().numpy().view(np.uint64), evoff)
    assert vals[:tot].cpu().numpy().tobytes() == evals
    # device hit rows from the probe, in place
    hits = torch.full((c.nt, (n + 63) // 64), -1, dtype=torch.int64, device="cuda")
    gpu.probe_tiers(c.sets, c.tiers, c.slots, gpu.DeviceKeys(dk), out=hits)
    assert _lib.load().cb_stream_synchronize(None) == _lib.CB_OK
    assert np.array_equal(hits.cpu().numpy().view(np.uint64), c.oracle_gate(c.look))


def test_zone_update_ordering(gpu):
    """Get, set_zone on one tier's slot to a range that newly excludes keys,
    get again on the same stream: the second answer is the oracle's with the
    new zone."""
    c = Case(gpu, "k16", BASE_TIERS, BASE_TABLE_TIERS, BASE_SLOTS, BASE_SIZES, seed=33, pool_n=8000,
             windows=BASE_WINDOWS)
    og = c.oracle_gate(c.look)
    ow, ovoff, ovals = c.oracle_get(c.look, og)
    which, voff, vals = c.get(c.look)
    assert np.array_equal(which, ow) and vals == ovals
    t = 3  # the large power-of-two tier's table (no zone so far)
    ks = c.keys[t]
    lo, hi = ks[len(ks) // 3], ks[2 * len(ks) // 3]
    c.sets[c.tiers[t]].set_zone(int(c.slots[t]), (lo, hi))
    zones = list(c.ozones)
    zones[t] = oracle.OracleZone(lo, hi)
    og2 = c.oracle_gate(c.look, zones=zones)
    ow2, ovoff2, ovals2 = c.oracle_get(c.look, og2)
    assert ((ow == t) & (ow2 != t)).any()  # the new zone shuts keys out of table t
    assert np.array_equal(c.probe(c.look), og2)
    which, voff, vals = c.get(c.look)
    assert np.array_equal(which, ow2) and np.array_equal(voff, ovoff2) and vals == ovals2


def test_refusals(gpu, base16):
    """Every violation of the limits is CB_EINVAL and writes nothing."""
    from lsmt_amd import _lib
    L = _lib.load()
    c = base16
    wide = gpu.FilterSet(1024, width=128)
    n = 100
    keys = batch(gpu, c.look[:n], "k16")
    tables = (ctypes.c_void_p * 65)(*([t._h.value for t in c.tables] + [c.tables[0]._h.value] * (65 - c.nt)))

    def arr(sets):
        return (ctypes.c_void_p * max(len(sets), 1))(*[s._h.value for s in sets])

    def both(sets, ns, tiers, slots, nt):
        sa = ctypes.cast(arr(sets), ctypes.c_void_p)
        tp = None if tiers is None else np.asarray(tiers, np.uint32)
        sp = None if slots is None else np.asarray(slots, np.uint32)
        tpp = None if tp is None else tp.ctypes.data
        spp = None if sp is None else sp.ctypes.data
        hits = np.full((65, 2), 7, np.uint64)
        assert L.cb_tiers_probe_fixed(sa, ns, tpp, spp, nt, keys.ctypes.data, 16, n, 1, hits.ctypes.data,
                                      None) == _lib.CB_EINVAL
        assert L.cb_last_error()
        assert (hits == 7).all()
        which = np.full(n, 7, np.int32)
        voff = np.full(n + 1, 7, np.uint64)
        vals = np.full(64, 7, np.uint8)
        tot = ctypes.c_uint64(7)
        assert L.cb_tiers_get_many_fixed(sa, ns, ctypes.cast(tables, ctypes.c_void_p), nt, tpp, spp,
                                         keys.ctypes.data, 16, n, which.ctypes.data, voff.ctypes.data,
                                         vals.ctypes.data, 64, ctypes.byref(tot), None) == _lib.CB_EINVAL
        assert (which == 7).all() and (voff == 7).all() and (vals == 7).all() and tot.value == 7

    tiers, slots = list(c.tiers), list(c.slots)
    both(c.sets, 0, tiers, slots, c.nt)
    both(c.sets * 3, 9, tiers, slots, c.nt)
    both(c.sets, 3, tiers, slots, 0)
    both(c.sets, 3, [0] * 65, [0] * 65, 65)
    both(c.sets, 3, [3] + tiers[1:], slots, c.nt)        # tiers[t] >= ns
    both(c.sets, 3, tiers, [32] + slots[1:], c.nt)       # table 0's tier is 32 slots wide
    both(c.sets[:2] + [wide], 3, tiers, slots, c.nt)     # a wide set
    both(c.sets, 3, None, slots, c.nt)
    both(c.sets, 3, tiers, None, c.nt)
    # and the same arguments are accepted once they are within the limits
    assert np.array_equal(gpu.probe_tiers(c.sets, c.tiers, c.slots, keys), c.oracle_gate(c.look[:n]))


def test_tiers_get_many_follows_the_tier_list_between_calls(gpu):
    """Two calls in a row on one stream over the same four tables and keys,
    the second after two of the tables swapped the tier they name: the views
    stay as the workspace holds them (nothing to upload) while the tier list
    changes, and each answer must come from the call's own list. Two tiers
    (m = 1024 and a non-power-of-two m); overlapping tables whose values name
    their table; 65 keys, some absent. Every result is compared exactly with a
    plain Python newest-first walk over the tables' dicts; each run's filters
    sit only in that run's tier and slot."""
    ms = [1024, 1_000_003]
    pool = [b"tier-%011d" % i for i in range(40)]          # 16-byte keys; 14 .. 39 are in no table
    members = [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [6, 7, 8, 9, 10], [1, 5, 9, 12, 13]]
    keys = [sorted(pool[i] for i in m) for m in members]
    tables = [gpu.Table(table_file(ks, t)) for t, ks in enumerate(keys)]
    dicts = [{k: b"%d:" % t + k[::-1] for k in ks} for t, ks in enumerate(keys)]
    look = [pool[(7 * i) % 40] for i in range(65)]
    which_e, lens, vals_e = [], [], []
    for k in look:
        t = next((i for i, d in enumerate(dicts) if k in d), -1)
        v = dicts[t][k] if t >= 0 else b""
        which_e.append(t)
        lens.append(len(v))
        vals_e.append(v)
    voff_e = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert set(which_e) == {-1, 0, 1, 2, 3}
    slots = [3, 5, 7, 2]
    for tiers in ([0, 1, 0, 1], [1, 0, 0, 1]):             # tables 0 and 1 swap tiers
        sets = [gpu.FilterSet(m, width=32) for m in ms]
        for t in range(4):
            b = gpu.BloomFilter(ms[tiers[t]])
            b.insert_batch(batch(gpu, keys[t], "k16"))
            sets[tiers[t]].assign(slots[t], b)
        which, voff, vals = gpu.get_many_tiers(tables, sets, tiers, slots, batch(gpu, look, "k16"))
        assert np.array_equal(np.asarray(which), np.asarray(which_e, np.int32)), tiers
        assert np.array_equal(np.asarray(voff, dtype=np.uint64), voff_e), tiers
        assert vals == b"".join(vals_e), tiers
