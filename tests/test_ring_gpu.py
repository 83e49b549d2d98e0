"""cb_ring_route_*, cb_scan_route and cb_tables_compact_ring on the device,
against the plain restatement of the reference's ring in tests/ring_ref.py
(Cluster::new, src/cluster.rs:46-54; replicas_for, src/cluster.rs:102-123).
Every comparison is exact.

Routes: every ring of tests/ring_ref.py (the 3x8 one is searched in LDS,
the 64x256 one in global memory behind its bucket table), batches of 0 to 5000
keys that cross the block's 2048 keys, fixed 16-byte keys and ragged keys of 0
to 40 bytes >= 0x80 (every tail length and every misalignment of the aligned
dword reads), host and device buffers, either output left out. Compaction:
the file, line count, zone bounds and Bloom bits of cb_tables_compact_ring
against the base entry's output filtered by ring_ref and written again by
cb_sstable_create, with sorted-record counts at the edges of the select's
256-record tile.
"""
import ctypes

import numpy as np
import pytest
import torch

import ring_ref
from merge_help import BAD, b64, open_tables, raw_file, row, TILE, tomb
from ring_ref import RINGS, TOKEN_RINGS

pytestmark = pytest.mark.gpu

CB_OK, CB_EINVAL = 0, -1
SIZES = [0, 1, 63, 64, 65, 257, 5000]
ALL_RINGS = sorted(RINGS) + sorted(TOKEN_RINGS)


def make_ring(gpu, name):
    from lsmt_amd import ring
    if name in RINGS:
        names, vnodes, rf = RINGS[name]
        return ring.Ring(names, vnodes, rf), ring_ref.Ring(names, vnodes, rf)
    pairs, nnodes, rf = TOKEN_RINGS[name]
    return (ring.Ring.from_tokens([t for t, _ in pairs], [o for _, o in pairs], nnodes, rf),
            ring_ref.Ring(pairs=pairs, nnodes=nnodes, rf=rf))


@pytest.fixture(scope="module")
def fixed_keys():
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 256, (max(SIZES), 16), dtype=np.uint8)
    keys[5, :4] = np.frombuffer(b"n0-3", np.uint8)  # (never routed whole: 16 bytes)
    return keys, [ring_ref.murmur3_32(k.tobytes()) for k in keys]


@pytest.fixture(scope="module")
def ragged_keys():
    """Lengths 0..40 in turn, bytes >= 0x80, a separator here and there; then
    the keys whose tokens sit on, above and below the 3x8 ring's."""
    rng = np.random.default_rng(12)
    keys = []
    for i in range(max(SIZES) - 4):
        k = bytearray(rng.integers(0x80, 256, i % 41, dtype=np.uint8).tobytes())
        for j in range(len(k)):
            if rng.integers(0, 9) == 0:
                k[j] = ord(b"|")
        keys.append(bytes(k))
    keys[3:3] = [b"n0-3", b"n1-0", b"", b"|"]
    return keys


def expect(ref, keys, skip=0, npk=0):
    got = [ref.replicas(k, skip, npk) for k in keys]
    return (np.array([t for t, _ in got], np.uint32),
            np.array([r for _, r in got], np.int32).reshape(len(keys), ref.rf))


def pack(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"".join(keys), np.uint8).copy() if off[-1] else np.zeros(1, np.uint8)
    return data, off


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def check_route(gpu, r, b, want, skip=0, npk=0):
    from lsmt_amd import ring
    tok, rep = ring._route(r, b, skip, npk, None, True, True)
    torch.cuda.synchronize()
    assert np.array_equal(host(tok), want[0]), "tokens differ"
    assert np.array_equal(host(rep), want[1]), "replicas differ"


@pytest.mark.parametrize("name", ALL_RINGS)
def test_route_fixed(gpu, name, fixed_keys):
    from lsmt_amd import ring
    r, ref = make_ring(gpu, name)
    keys, tokens = fixed_keys
    rows = {t: ref.replicas_for_token(t) for t in set(tokens)}
    want_all = (np.array(tokens, np.uint32),
                np.array([rows[t] + [-1] * (ref.rf - len(rows[t])) for t in tokens], np.int32).reshape(-1, ref.rf))
    dkeys = torch.from_numpy(keys).cuda()
    for n in SIZES:
        want = (want_all[0][:n], want_all[1][:n])
        check_route(gpu, r, gpu.KeyBatch(n=n, key_len=16, keys=keys), want)
        check_route(gpu, r, gpu.KeyBatch(n=n, key_len=16, keys=dkeys), want)
    # either output left out, host and device; an unaligned device base (byte loads of a 16-byte key)
    n = 257
    for b in (gpu.KeyBatch(n=n, key_len=16, keys=keys), gpu.KeyBatch(n=n, key_len=16, keys=dkeys)):
        tok, rep = ring._route(r, b, 0, 0, None, True, False)
        assert rep is None and np.array_equal(host(tok), want_all[0][:n])
        tok, rep = ring._route(r, b, 0, 0, None, False, True)
        assert tok is None and np.array_equal(host(rep), want_all[1][:n])
    flat = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), keys[:n].reshape(-1)])).cuda()
    check_route(gpu, r, gpu.KeyBatch(n=n, key_len=16, keys=flat[3:]), (want_all[0][:n], want_all[1][:n]))
    # the public form
    tok, rep = r.route(keys[:65])
    assert tok.dtype == np.uint32 and rep.dtype == np.int32 and rep.shape == (65, ref.rf)
    assert np.array_equal(tok, want_all[0][:65]) and np.array_equal(rep, want_all[1][:65])
    r.close()


@pytest.mark.parametrize("name", ALL_RINGS)
def test_route_ragged(gpu, name, ragged_keys):
    r, ref = make_ring(gpu, name)
    cases = [(0, 0), (0, 1), (3, 2), (1, 0), (50, 1)]
    wants = {c: expect(ref, ragged_keys, *c) for c in cases[:3]}
    for n in SIZES:
        data, off = pack(ragged_keys[:n])
        b = gpu.KeyBatch(n=n, data=data, offsets=off)
        for c in cases[:3]:
            check_route(gpu, r, b, (wants[c][0][:n], wants[c][1][:n]), *c)
        d = gpu.KeyBatch(n=n, data=torch.from_numpy(data).cuda(), offsets=torch.from_numpy(off.view(np.int64)).cuda())
        check_route(gpu, r, d, (wants[(0, 0)][0][:n], wants[(0, 0)][1][:n]))
        check_route(gpu, r, d, (wants[(3, 2)][0][:n], wants[(3, 2)][1][:n]), 3, 2)
    sub = ragged_keys[:300]
    data, off = pack(sub)
    for c in cases[3:]:
        check_route(gpu, r, gpu.KeyBatch(n=len(sub), data=data, offsets=off), expect(ref, sub, *c), *c)
    r.close()


def test_both_search_paths_are_taken(gpu):
    """The 3x8 ring is searched in LDS and the 64x256 one is not; keys that
    hit a ring token exactly, wrap past the largest and fall below the smallest."""
    from lsmt_amd import ring
    small, sref = make_ring(gpu, "3x8")
    big, bref = make_ring(gpu, "64x256")
    assert small.positions <= ring.LDS_POSITIONS < big.positions
    for r, ref, names in ((small, sref, RINGS["3x8"][0]), (big, bref, RINGS["64x256"][0])):
        exact = [nm + b"-%d" % v for nm in names[:3] for v in range(8)]
        keys = exact + [b"w%d" % i for i in range(3000)]
        tokens = [ring_ref.murmur3_32(k) for k in keys]
        assert all(t in ref.ring for t in tokens[:len(exact)])
        if r is small:
            assert any(t > ref.sorted[-1] for t in tokens) and any(t < ref.sorted[0] for t in tokens)
        tok, rep = r.route(keys)
        want = expect(ref, keys)
        assert np.array_equal(tok, want[0]) and np.array_equal(rep, want[1])
        assert [int(x) for x in rep[:len(exact), 0]] == [i // 8 for i in range(len(exact))]  # inclusive
    # the extremes of an explicit ring: tokens 0 and 0xFFFFFFFF are positions, the search wraps above the last
    r, ref = make_ring(gpu, "repeat")
    keys = [b"k%d" % i for i in range(500)] + [b""]
    tok, rep = r.route(keys)
    want = expect(ref, keys)
    assert np.array_equal(tok, want[0]) and np.array_equal(rep, want[1]) and (tok > 300).any()
    for x in (small, big, r):
        x.close()


# ---- the tables of the scan and compaction tests ----------------------------------------

RULES = [(b"ev:", 2), (b"u:", 1)]


def store_files(rng, per=300):
    """Three data files of about `per` lines over two namespaces (u: one
    partition column, ev: two, a clustering part behind them) and a few
    catalog rows: overlapping keys, undecodable values, tombstones whose
    timestamps are out of table order."""
    pool = [b"u:user%d|c%d" % (i // 3, i % 3) for i in range(240)]
    pool += [b"ev:%d|%c|e%d" % (i // 8, 65 + (i // 2) % 4, i % 2) for i in range(240)]
    pool += [b"u:solo", b"ev:only|one", b"u:|", b"ev:||"]
    catalog = [b"_tables:ev", b"_tables:u", b"_schema:u"]
    files = []
    for t in range(3):
        picked = sorted(set(pool[i] for i in rng.choice(len(pool), per - 3, replace=False)) | set(catalog))
        lines = []
        for k in picked:
            ts = int(rng.integers(1, 1000))  # (out of table order on purpose)
            kind = 9 if k in catalog else rng.integers(0, 10)  # (the catalog rows are live in every table)
            text = BAD if kind == 0 else tomb(ts) if kind <= 2 else row(ts, b'{"v":"%d"}' % t)
            lines.append((k, text))
        files.append(raw_file(lines))
    return files


BASES = {(False, False): lambda g, t: g.compact(t), (False, True): lambda g, t: g.compact_live(t),
         (True, False): lambda g, t: g.compact_lww(t), (True, True): lambda g, t: g.compact_lww(t, drop_dead=True)}


@pytest.fixture(scope="module")
def store(gpu):
    files = store_files(np.random.default_rng(5))
    tables = open_tables(gpu, files)
    bases = {}
    for rule, entry in BASES.items():
        merged = entry(gpu, tables)[0]
        bases[rule] = gpu.scan([merged]).items() if merged.nlines else []
        merged.close()
    return tables, bases


def expect_file(gpu, entries):
    """(file bytes, lines, Bloom bits, zone bounds) of cb_sstable_create over the entries."""
    t, bloom, z = gpu.sstable_create(entries, m=1024)
    out = (t.data(), t.nlines, bloom.bools().copy(), (z.min, z.max))
    t.close()
    return out


def compacted(gpu, tables, r, node, rules, ranks=0, lww=False, drop=False):
    from lsmt_amd import ring
    t, bloom, z = ring.compact_ring(tables, r, node, rules=rules, ranks=ranks, lww=lww, drop_dead=drop)
    out = (t.data(), t.nlines, bloom.bools().copy(), (z.min, z.max))
    assert t.nbytes == len(out[0]) and (not t.nlines or t.well_formed)
    t.close()
    return out


def same(got, want, what):
    assert got[0] == want[0], f"{what}: file differs ({len(got[0])} bytes against {len(want[0])})"
    assert got[1] == want[1] and got[3] == want[3], what
    assert np.array_equal(got[2], want[2]), f"{what}: Bloom bits differ"


@pytest.mark.parametrize("lww,drop", sorted(BASES))
def test_compact_ring(gpu, store, lww, drop):
    tables, bases = store
    base = bases[(lww, drop)]
    r, ref = make_ring(gpu, "3x8")
    partitioned = [k for k, _ in base if k.startswith((b"u:", b"ev:"))]
    assert len(partitioned) > 300 and len(base) - len(partitioned) == 3
    for ranks in (0, 1, 2):
        held = {k: 0 for k, _ in base}
        for node in range(3):
            kept = [(k, v) for k, v in base if ref.owned(k, node, RULES, ranks)]
            got = compacted(gpu, tables, r, node, RULES, ranks, lww, drop)
            same(got, expect_file(gpu, kept), f"lww={lww} drop={drop} ranks={ranks} node={node}")
            for k, _ in kept:
                held[k] += 1
        copies = {1: 1, 2: 2, 0: ref.width}[ranks]
        assert all(held[k] == copies for k in partitioned), ranks
        assert all(held[k] == 3 for k in held if k.startswith(b"_")), "catalog rows stay everywhere"
    r.close()


def test_compact_ring_edges(gpu, store):
    from lsmt_amd import ring
    tables, bases = store
    base = bases[(False, False)]
    want_all = expect_file(gpu, base)
    # a one-node ring: cb_tables_compact's file byte for byte
    one = ring.Ring([b"n0"], 4, 1)
    t = gpu.compact(tables)[0]
    assert compacted(gpu, tables, one, 0, RULES)[0] == t.data() == want_all[0]
    # no prefix: everything is kept, by every node
    r, ref = make_ring(gpu, "3x8")
    for node in range(3):
        same(compacted(gpu, tables, r, node, ()), want_all, "np == 0")
    # one rule only: the other namespace is every node's
    kept = [(k, v) for k, v in base if ref.owned(k, 1, RULES[1:], 1)]
    assert any(k.startswith(b"ev:") for k, _ in kept)
    same(compacted(gpu, tables, r, 1, RULES[1:], 1), expect_file(gpu, kept), "one rule")
    # a node that owns nothing: the table of length 0
    lone = ring.Ring.from_tokens([5, 9], [0, 0], 2, 1)
    only = open_tables(gpu, [raw_file([(b"u:a|1", b64(b"x")), (b"u:b|2", b64(b"y"))])])
    got = compacted(gpu, only, lone, 1, RULES)
    assert got[0] == b"" and got[1] == 0 and not got[2].any() and got[3] == (None, None)
    assert compacted(gpu, only, lone, 0, RULES)[1] == 2
    # without a filter
    L = gpu._lib.load()
    arr = (ctypes.c_void_p * 1)(only[0]._h.value)
    rules = ring._Rules(RULES)
    th = ctypes.c_void_p()
    assert L.cb_tables_compact_ring(arr, 1, 0, lone._h, 0, 0, rules.ref(), 0, 0, None, ctypes.byref(th), None) == CB_OK
    assert L.cb_table_destroy(th) == CB_OK
    # refusals that need a real table list: the own arguments still come first, then the list's
    th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xDEAD)
    assert L.cb_tables_compact_ring(arr, 1, 1024, lone._h, 2, 0, rules.ref(), 0, 0, None, ctypes.byref(th),
                                    ctypes.byref(fh)) == CB_EINVAL
    assert (th.value, fh.value) == (None, None) and b"not a node" in L.cb_last_error()
    bad = gpu.Table(b"b\tQQ==\na\tQQ==\n")  # keys out of order: not well-formed
    arr2 = (ctypes.c_void_p * 2)(only[0]._h.value, bad._h.value)
    th, fh = ctypes.c_void_p(0xDEAD), ctypes.c_void_p(0xDEAD)
    assert L.cb_tables_compact_ring(arr2, 2, 1024, lone._h, 0, 0, rules.ref(), 0, 0, None, ctypes.byref(th),
                                    ctypes.byref(fh)) == CB_EINVAL
    assert (th.value, fh.value) == (None, None) and b"not well-formed" in L.cb_last_error()
    for x in (one, r, lone, t, bad, only[0]):
        x.close()


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 700])
def test_compact_ring_tile_edges(gpu, n):
    """n sorted records in all, from two tables that share keys: the tile sums
    are taken again after the filter, and a wrong one shows at a tile's edge."""
    shared = n // 4
    keys = [b"u:p%03d|c" % i for i in range(n - shared)]  # sorted as written
    half = (len(keys) - shared) // 2
    first, second = keys[:half + shared], keys[half:]     # `shared` keys lie in both
    files = [raw_file([(k, row(7, b"new")) for k in first]), raw_file([(k, row(3, b"old")) for k in second])]
    assert sum(f.count(b"\n") for f in files) == n
    tables = open_tables(gpu, files)
    merged = gpu.compact(tables)[0]
    base = gpu.scan([merged]).items()
    r, ref = make_ring(gpu, "3x8")
    total = 0
    for node in range(3):
        kept = [(k, v) for k, v in base if ref.owned(k, node, RULES, 1)]
        total += len(kept)
        same(compacted(gpu, tables, r, node, RULES, 1), expect_file(gpu, kept), f"n={n} node={node}")
    assert total == len(base)
    for x in tables + [merged, r]:
        x.close()


def test_scan_route(gpu, store):
    from lsmt_amd import ring
    tables, _ = store
    r, ref = make_ring(gpu, "3x8")
    res = gpu.scan_many(tables, prefixes=[b"ev:", b"u:"])
    keys, off = res.keys(), res.range_off().tolist()
    assert res.nranges == 2 and 0 < off[1] < off[2] == res.count
    rule = lambda i: (3, 2) if i < off[1] else (2, 1)  # noqa: E731
    want = [ref.replicas(k, *rule(i)) for i, k in enumerate(keys)]
    tok, rep = ring.route_scan(res, r, skip=[3, 2], npk=[2, 1])
    assert tok.tolist() == [t for t, _ in want] and rep.tolist() == [x for _, x in want]
    # one number for every range, and nothing taken off at all
    tok, rep = ring.route_scan(res, r, skip=2, npk=1)
    assert tok.tolist() == [ref.replicas(k, 2, 1)[0] for k in keys]
    tok, rep = ring.route_scan(res, r)
    assert tok.tolist() == [ref.replicas(k)[0] for k in keys] and rep.tolist() == [ref.replicas(k)[1] for k in keys]
    # device outputs, either left out
    L = gpu._lib.load()
    dtok = torch.zeros(res.count, dtype=torch.int32, device="cuda")
    assert L.cb_scan_route(res._h, r._h, None, None, dtok.data_ptr(), None) == CB_OK
    assert dtok.cpu().numpy().view(np.uint32).tolist() == tok.tolist()
    rep2 = np.zeros((res.count, ref.rf), np.int32)
    assert L.cb_scan_route(res._h, r._h, None, None, None, rep2.ctypes.data) == CB_OK and rep2.tolist() == rep.tolist()
    # an empty result: nothing is written
    empty = gpu.scan_many(tables, prefixes=[b"nothing:", b"zzz:"])
    assert empty.count == 0
    tok, rep = ring.route_scan(empty, r, skip=[1, 2], npk=[1, 1])
    assert len(tok) == 0 and rep.shape == (0, ref.rf)
    canary = np.full(4, 0xDEAD, np.uint32)
    assert L.cb_scan_route(empty._h, r._h, None, None, canary.ctypes.data, None) == CB_OK
    assert canary.tolist() == [0xDEAD] * 4
    for x in (res, empty, r):
        x.close()
