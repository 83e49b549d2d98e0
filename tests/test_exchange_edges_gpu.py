"""The sparse hit exchange at its block, capacity and rank edges: the places
where cb_hits_compress, the pack writer inside the fused FilterSet probe,
cb_hits_expand and cb_hits_expand_set branch, which tests/test_exchange_gpu.py
reaches with a few mid-sized shapes only.

- A: cb_hits_compress from 16-byte aligned and from 8-byte aligned bases at
  one word either side of a 2048-word block; with cap == count, count - 1 and
  1; and seven launches queued back to back on one stream (many blocks, one
  block, no rows, an overflow, the fused probe) so the alternating claim
  words meet every kind of predecessor, also on two streams at once.
- B: cb_hits_expand over rank layouts with leading, trailing and adjacent
  empty ranks, 64 ranks, slices at the block edges, and packs a kernel really
  truncated.
- C: FilterSet.probe_pack at widths 32 and 64 with 1..64 used slots, both
  kinds of m, gated, unaligned and odd-length keys and gaps in the slots, at
  batch sizes around one probe block; cb_hits_expand_set over ranks of up to
  64 rows; both through the communicator at world size 1.
- D: one CPU test that pins the numpy restatements to a per-bit loop and
  shows that the inputs of A-C are not vacuous.

Every comparison is bit-exact against numpy (the set-bit positions of each
block in ascending order; the concatenation of the ranks' rows) or the C
oracle's probe, never against another GPU path. Every output buffer is
pre-filled with ones and carries guard words that must survive. Nothing here
runs on more than one GPU: RCCL at world > 1 stays unmeasured.
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import pytest

from lsmt_amd import workload
from lsmt_amd.shard import PACK_BLOCK_WORDS
from oracle import oracle

BW = PACK_BLOCK_WORDS  # words per compress block
PW = 16                # hit words per probe block (filterset.hpp kSetWords): 1024 keys
GUARD = 16             # words behind every pack
FILL = 0xFFFFFFFF
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
TOP = np.uint64(1 << 63)


# ---- the plain reference ----------------------------------------------------------

def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


def positions(h):
    """The set-bit positions of h (uint64, any shape) in row-major order, ascending."""
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(h).reshape(-1).view(np.uint8),
                                        bitorder="little")).astype(np.uint32)


def compress_blocks(h):
    """cb_hits_compress's blocks: the positions of each 2048 words of h."""
    pos = positions(h)
    blk = (pos >> 6) // BW
    return [pos[blk == b] for b in range(-(-h.size // BW))]


def probe_blocks(rows, n):
    """The fused probe's blocks: block b holds, slot-major, the positions
    slot * hwords * 64 + key of the keys [1024 b, 1024 (b + 1))."""
    hwords = (n + 63) // 64
    assert rows.shape[1] == hwords
    pos = positions(rows)
    blk = ((pos >> 6) % hwords) // PW
    return [pos[blk == b] for b in range(-(-hwords // PW))]


def kept(base, c, cap):
    """How many of a block's c positions, claimed at slots [base, base + c),
    a pack of cap slots stores: those at slots below cap, a prefix."""
    return int(min(max(cap - base, 0), c))


def check_pack_strict(pk, blocks, cap):
    """pk: the whole uint32 buffer {count, 0, positions[cap], dir[2 * blocks],
    GUARD words}, pre-filled with ones. Exact under overflow too: the count,
    every directory pair (the bases tile [0, count)), each block's stored
    prefix, and that nothing else in the buffer was written."""
    nblk = len(blocks)
    count = sum(len(b) for b in blocks)
    assert len(pk) == 2 + cap + 2 * nblk + GUARD
    assert pk[0] == count and pk[1] == 0
    dirs = pk[2 + cap:2 + cap + 2 * nblk].reshape(nblk, 2).astype(np.int64)
    assert np.array_equal(dirs[:, 1], [len(b) for b in blocks])
    assert (dirs[:, 0] <= count).all()  # an empty block's base is wherever the claims stood
    used = dirs[dirs[:, 1] > 0]
    used = used[np.argsort(used[:, 0], kind="stable")]
    ends = np.cumsum(used[:, 1])
    assert np.array_equal(used[:, 0], ends - used[:, 1])  # the blocks tile [0, count)
    written = np.zeros(cap, bool)
    for b in range(nblk):
        base, c = dirs[b]
        k = kept(base, c, cap)
        assert np.array_equal(pk[2 + base:2 + base + k], blocks[b][:k]), b
        written[base:base + k] = True
    assert written[:min(count, cap)].all() and int(written.sum()) == min(count, cap)
    assert (pk[2:2 + cap][~written] == FILL).all()       # slots nobody claimed
    assert (pk[2 + cap + 2 * nblk:] == FILL).all()       # the guard words


def pack_words_hits(nw, cap):
    return 2 + cap + 2 * (-(-nw // BW))


def pack_words_set(n, cap):
    return 2 + cap + 2 * (-(-((n + 63) // 64) // PW))


def bits_to_words(bits, shape):
    return np.packbits(bits.astype(np.uint8), bitorder="little").view(np.uint64).reshape(shape).copy()


def random_hits(rng, rows, words, density):
    return bits_to_words(rng.random(rows * words * 64) < density, (rows, words))


# ---- A: inputs --------------------------------------------------------------------

A1_SHAPES = [(1, 1), (1, 8), (1, 2047), (1, 2048), (1, 2049), (3, 683), (2, 2048)]


def a1_patterns(rows, words):
    nw = rows * words
    rng = np.random.default_rng(1000 * rows + words)
    out = {"random": random_hits(rng, rows, words, 0.02), "zero": np.zeros((rows, words), np.uint64)}
    top = np.zeros(nw, np.uint64)
    top[-1] = TOP
    out["top"] = top.reshape(rows, words)
    edge = np.zeros(nw, np.uint64)
    for b in range(-(-nw // BW)):
        edge[b * BW] = ONES
        edge[min((b + 1) * BW, nw) - 1] = ONES
    out["edges"] = edge.reshape(rows, words)
    return out


def a2_input():
    return random_hits(np.random.default_rng(21), 3, 1700, 0.02)  # 5100 words: three blocks


def a2_caps(h):
    count = popcount(h)
    return [count, count - 1, 1]


def a3_compress_steps(seed):
    """The standalone launches of the A3 sequence, (name, hits, cap) in issue
    order; the fused probe goes between "many2" and "one2"."""
    rng = np.random.default_rng(seed)
    many = random_hits(rng, 1, 40 * BW, 0.005)
    one = random_hits(rng, 1, 100, 0.05)
    over = random_hits(rng, 3, 1700, 0.02)
    many2 = random_hits(rng, 5, 8 * BW, 0.005)
    return [("many", many, popcount(many) + 3), ("one", one, popcount(one)),
            ("norows", np.zeros((0, 100), np.uint64), 4), ("over", over, popcount(over) // 2),
            ("many2", many2, popcount(many2)), ("one2", np.full((1, 1), ONES), 64)]


# ---- B: inputs --------------------------------------------------------------------

SPARSE64 = [0 if r in (0, 31, 63) else 1 for r in range(64)]
B1_LAYOUTS = {"lead": [0, 3, 2], "trail": [3, 2, 0], "mid2": [2, 0, 0, 3], "one_of_4": [0, 0, 4, 0], "single": [5],
              "r64": SPARSE64}
B1_WORDS = 700
B2_CASES = [([2, 3, 1], w) for w in (1, 1024, 2047, 2048, 2049)] + [([1] * 64, 2049)]
B3_LAYOUT, B3_WORDS = [2, 3, 1], 1500


def make_parts(sizes, words, seed, density=0.02):
    """One uint64 [rows, words] slice per rank; every slice that has rows
    starts with an all-ones word and ends with bit 63 set."""
    rng = np.random.default_rng(seed)
    parts = []
    for r in sizes:
        p = random_hits(rng, r, words, density)
        if r:
            p[0, 0] = ONES
            p[-1, -1] |= TOP
        parts.append(p)
    return parts


def b3_parts():
    return make_parts(B3_LAYOUT, B3_WORDS, 33)


# ---- C: pools, cases and the oracle's answers ----------------------------------------

KPF = 500
# Which key of its filter lookup j takes. Chosen on the CPU so that the gated
# cases' key 0 and key 1024 lie inside their tables' zones (with 3 the gated
# n = 1 case had no hit): test_edge_inputs_and_reference_are_sound checks it.
IDX_MUL, IDX_ADD = 7, 19
POOLS = {"pow2": (1 << 16, 64, 16, 4000), "generic": (100_003, 64, 16, 5000),
         "rand7": (1 << 16, 40, 7, 6000), "rand24": (100_003, 20, 24, 7000)}
NMAX = 2049


@functools.lru_cache(maxsize=None)
def _pool(name):
    """nf filters' keys K [nf, KPF, key_len], NMAX absent keys, and each
    filter's oracle twin; built once per process."""
    m, nf, klen, seed = POOLS[name]
    if klen == 16:
        K = np.stack([workload.key_range(seed + f, KPF) for f in range(nf)])
        absent = workload.key_range(seed + 999, NMAX)
    else:  # random bytes 0..255
        rng = np.random.default_rng(seed)
        K = rng.integers(0, 256, (nf, KPF, klen), dtype=np.uint8)
        absent = rng.integers(0, 256, (NMAX, klen), dtype=np.uint8)
    ofs = []
    for f in range(nf):
        o = oracle.OracleFilter(m)
        o.insert_fixed(K[f])
        ofs.append(o)
    return SimpleNamespace(name=name, m=m, nf=nf, klen=klen, K=K, absent=absent, ofs=ofs, empty=oracle.OracleFilter(m))


def _zone(pool, f):
    """Half-width zone of filter f: the gate rejects a quarter of its keys at either end."""
    srt = workload.sort_keys16(pool.K[f])
    return bytes(srt[KPF // 4]), bytes(srt[3 * KPF // 4])


def _lookups(pool, live, n):
    """Even i: a key of filter live[(len(live) - 1 + 23 j) % len(live)], j =
    i / 2, so key 0 belongs to the highest live slot and the slots take turns;
    odd i: an absent key."""
    i = np.arange(n)
    j = i // 2
    f = np.asarray(live)[(len(live) - 1 + 23 * j) % len(live)]
    out = pool.K[f, (IDX_MUL * j + IDX_ADD) % KPF].copy()
    out[i % 2 == 1] = pool.absent[:n][i % 2 == 1]
    return np.ascontiguousarray(out)


class Case(NamedTuple):
    id: str
    pool: str
    width: int
    slots: tuple          # slot -> filter of the pool, or None for a slot never assigned
    n: int
    gated: bool = False
    offset4: bool = False  # 16-byte keys at a base 4 bytes off alignment
    cleared: tuple = ()    # (slot, filter) pairs assigned and then cleared: they raise `used` only
    slack: int = 3         # cap = count + slack

    @property
    def used(self):
        return max([len(self.slots)] + [s + 1 for s, _ in self.cleared])

    def filter_of(self, slot):
        return self.slots[slot] if slot < len(self.slots) else None

    @property
    def live(self):
        return [f for f in self.slots if f is not None]


C1_N = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
GAPS = tuple({0: 10, 3: 11, 4: 12, 17: 13, 32: 14, 40: 15}.get(s) for s in range(41))
C1_CASES = (
    [Case(f"w64u64-n{n}", "pow2", 64, tuple(range(64)), n) for n in C1_N]
    + [Case(f"w32u31gated-n{n}", "generic", 32, tuple(range(5, 36)), n, gated=True, slack=0) for n in C1_N]
    + [Case("w32u1", "pow2", 32, (9,), 1025),
       Case("w32u32", "generic", 32, tuple(range(32, 64)), 1025),
       Case("w64u33", "generic", 64, tuple(range(33)), 1025),
       Case("w64u63", "pow2", 64, tuple(range(1, 64)), 1025),
       Case("w64offset4", "pow2", 64, tuple(range(63, -1, -1)), 1025, offset4=True),
       Case("w64len7", "rand7", 64, tuple(range(40)), 1025),
       Case("w32len24", "rand24", 32, tuple(range(20)), 1025),
       Case("w64gaps", "pow2", 64, GAPS, 1025, cleared=((45, 16),))])
A3_PROBE = Case("a3probe", "pow2", 64, tuple(range(64)), 2049, slack=0)


@functools.lru_cache(maxsize=None)
def _case_data(case, look_live=None):
    """(lookups, the oracle's [used, hwords] rows) of a case. look_live: the
    filters the present lookups are drawn from (default: the case's own)."""
    pool = _pool(case.pool)
    look = _lookups(pool, list(look_live) if look_live else case.live, case.n)
    ofs = [pool.empty if case.filter_of(s) is None else pool.ofs[case.filter_of(s)] for s in range(case.used)]
    if case.gated:
        zones = [oracle.OracleZone(*_zone(pool, case.filter_of(s))) for s in range(case.used)]
        offs = np.arange(0, pool.klen * (case.n + 1), pool.klen, dtype=np.uint64)
        rows = oracle.probe_gated(ofs, zones, np.ascontiguousarray(look.reshape(-1)), offs)
    else:
        rows = oracle.probe_fixed(ofs, look)
    assert rows.shape == (case.used, (case.n + 63) // 64)
    return look, rows


C2_LAYOUTS = {"64_0_1_33": [64, 0, 1, 33], "0_64_64": [0, 64, 64]}
C2_SLOTS = {"64_0_1_33": [tuple(range(64)), (), (7,), tuple(range(20, 53))],
            "0_64_64": [(), tuple(range(64)), tuple(range(63, -1, -1))]}
C2_N = [1025, 2049, 64]


def c2_ranks(layout, n):
    """The 'ranks' of a layout: one Case each over the pow2 pool, probing one
    shared batch drawn from all 64 filters."""
    return [Case(f"c2-{layout}-r{r}", "pow2", 32 if len(sl) <= 32 else 64, sl, n)
            for r, sl in enumerate(C2_SLOTS[layout])]


def c2_rows(layout, n):
    return [_case_data(c, tuple(range(64)))[1] for c in c2_ranks(layout, n)]


C3_CASE = Case("c3", "pow2", 64, tuple(range(64)), 2049)


# ---- D: the reference and the inputs, on the CPU ----------------------------------------

def _brute_positions(h):
    out = []
    for i, w in enumerate(int(x) for x in h.reshape(-1)):
        for b in range(64):
            if (w >> b) & 1:
                out.append(i * 64 + b)
    return out


def _brute_pack(blocks, cap, order):
    """A pack as the kernels must write it, slot by slot: the blocks claim
    their slots in `order`, and a position is stored only at a slot < cap."""
    nblk = len(blocks)
    pk = np.full(2 + cap + 2 * nblk + GUARD, FILL, np.uint32)
    slot = 0
    for b in order:
        pk[2 + cap + 2 * b], pk[2 + cap + 2 * b + 1] = slot, len(blocks[b])
        for p in blocks[b]:
            if slot < cap:
                pk[2 + slot] = p
            slot += 1
    pk[0], pk[1] = slot, 0
    return pk


def test_edge_inputs_and_reference_are_sound():
    """CPU only. The numpy restatements against per-bit loops, the strict
    checker against packs written slot by slot (and against wrong ones), and
    the conditions that keep the GPU cases meaningful, from the same seeds."""
    # positions and the per-block split of both pack writers, on three blocks
    h = random_hits(np.random.default_rng(5), 1, 2 * BW + 1, 0.01)
    h[0, -1] |= TOP
    brute = _brute_positions(h)
    assert positions(h).tolist() == brute and len(brute) > 100
    blocks = compress_blocks(h)
    assert len(blocks) == 3 and [b.tolist() for b in blocks] == [
        [p for p in brute if p // 64 // BW == k] for k in range(3)]
    n = 2049
    rows = random_hits(np.random.default_rng(6), 3, 33, 0.01)
    rows[:, -1] &= np.uint64(1)  # keys past n are never probed
    rows[2, -1] |= np.uint64(1)
    pb = probe_blocks(rows, n)
    brute = _brute_positions(rows)
    assert len(pb) == 3 and [b.tolist() for b in pb] == [
        [p for p in brute if (p % (33 * 64)) // 1024 == k] for k in range(3)]
    assert all(np.all(np.diff(b.astype(np.int64)) > 0) for b in pb) and len(pb[2]) >= 1
    # the truncation rule and the strict checker
    assert [kept(0, 5, 5), kept(3, 5, 5), kept(5, 5, 5), kept(9, 5, 5), kept(0, 0, 0)] == [5, 2, 0, 0, 0]
    count = sum(len(b) for b in blocks)
    for cap in (count + 2, count, count - 1, 1):
        for order in ([0, 1, 2], [2, 0, 1]):
            pk = _brute_pack(blocks, cap, order)
            check_pack_strict(pk, blocks, cap)
            for bad in ("dir0", "short", "guard", "count"):
                w = pk.copy()
                if bad == "dir0":    # a position stored at slot == cap lands on the first base
                    w[2 + cap] = blocks[order[-1]][-1]
                elif bad == "short":  # the last stored position missing
                    w[2 + min(count, cap) - 1] = FILL
                elif bad == "guard":
                    w[-GUARD] = 0
                else:
                    w[0] = min(count, cap)
                if not np.array_equal(w, pk):
                    with pytest.raises(AssertionError):
                        check_pack_strict(w, blocks, cap)
    check_pack_strict(_brute_pack([], 4, []), [], 4)  # no rows: count 0, nothing else
    # A1: every shape sees an empty block and a block whose last word has bit 63
    for rows_, words in A1_SHAPES:
        pats = a1_patterns(rows_, words)
        assert set(pats) == {"random", "zero", "top", "edges"}
        assert popcount(pats["zero"]) == 0 and popcount(pats["top"]) == 1
        assert any(len(b) == 0 for p in pats.values() for b in compress_blocks(p))
        for name in ("top", "edges"):
            flat = pats[name].reshape(-1)
            assert flat[-1] & TOP and compress_blocks(pats[name])[-1][-1] == flat.size * 64 - 1
        nblk = -(-rows_ * words // BW)
        assert popcount(pats["edges"]) == sum(64 if min((b + 1) * BW, rows_ * words) - b * BW == 1 else 128
                                              for b in range(nblk))
    assert popcount(a1_patterns(1, 2049)["random"]) > 1000
    # A2: three blocks, all with positions; cap == count, count - 1 (count == cap + 1), and 1 << count
    h2 = a2_input()
    caps = a2_caps(h2)
    b2 = compress_blocks(h2)
    assert len(b2) == 3 and all(len(b) > 500 for b in b2)
    assert caps[0] == popcount(h2) and caps[1] + 1 == popcount(h2) and caps[2] == 1 and popcount(h2) > 5000
    # A3: block counts of the queued launches
    for seed in (71, 72):
        steps = {name: (hh, cap) for name, hh, cap in a3_compress_steps(seed)}
        assert -(-steps["many"][0].size // BW) == 40 and -(-steps["many2"][0].size // BW) == 40
        assert steps["one"][0].size <= BW and steps["one"][1] == popcount(steps["one"][0]) > 0
        assert steps["norows"][0].size == 0 and popcount(steps["over"][0]) > steps["over"][1] > 0
        assert popcount(steps["one2"][0]) == steps["one2"][1] == 64
    # B: slices at the block edges; B3's counts
    for sizes, words in B2_CASES:
        for p in make_parts(sizes, words, 7):
            assert p[0, 0] == ONES and p[-1, -1] & TOP
    assert sorted({r * w for r, w in [(2, 1024), (3, 1024), (1, 2047), (1, 2048), (1, 2049)]}) == [
        2047, 2048, 2049, 3072]
    counts = [popcount(p) for p in b3_parts()]
    big = int(np.argmax(counts))
    assert big == 1 and sorted(counts)[-2] < counts[big] - 1  # the others fit cap = counts[big] - 1
    # C1: count > 0; a slot >= 32 at width 64; a position in the last probe block
    assert len({c.id for c in C1_CASES}) == len(C1_CASES) == 24
    for c in C1_CASES + [A3_PROBE]:
        look, rows = _case_data(c)
        pool = _pool(c.pool)
        assert look.shape == (c.n, pool.klen) and rows.shape[0] == c.used <= c.width
        pos = positions(rows)
        hwords = (c.n + 63) // 64
        assert len(pos) > 0, c.id
        if c.width == 64:
            assert (pos // (hwords * 64) >= 32).any(), c.id
        pbs = probe_blocks(rows, c.n)
        if len(pbs) > 1:
            assert len(pbs[-1]) > 0, c.id
        assert (pos % (hwords * 64) < c.n).all()
    gaps = next(c for c in C1_CASES if c.id == "w64gaps")
    assert gaps.used == 46 and len(gaps.live) == 6 and not _case_data(gaps)[1][[1, 2, 41, 45]].any()
    gated = next(c for c in C1_CASES if c.id == "w32u31gated-n2049")
    ungated = oracle.probe_fixed([_pool("generic").ofs[f] for f in gated.slots], _case_data(gated)[0])
    assert 0 < popcount(_case_data(gated)[1]) < popcount(ungated) - 100  # the gate rejects
    assert _pool("rand7").K.max() > 250 and _pool("rand24").K.min() < 5
    # C2: ranks of 64, 33, 1 and 0 rows with rows >= 32 hit; the truncated rank is the only one past cap
    for layout, sizes in C2_LAYOUTS.items():
        for n in C2_N:
            rws = c2_rows(layout, n)
            assert [r.shape[0] for r in rws] == sizes
            hw = (n + 63) // 64
            assert any((positions(r) // (hw * 64) >= 32).any() for r in rws)
    counts = [popcount(r) for r in c2_rows("64_0_1_33", 1025)]
    assert counts[0] - 1 >= max(counts[1:]) and counts[2] > 0 and counts[3] > 0
    assert popcount(_case_data(C3_CASE)[1]) > 1000


# ---- GPU helpers --------------------------------------------------------------------------

def _dev_hits(h, misalign=False):
    """h on the device: a fresh tensor (16-byte aligned base), or a view that
    starts one int64 into a larger one (8-byte aligned only)."""
    import torch
    flat = torch.from_numpy(h.view(np.int64).reshape(-1).copy())
    if misalign:
        big = torch.zeros(h.size + 3, dtype=torch.int64, device="cuda")
        big[1:1 + h.size] = flat
        t = big[1:1 + h.size].view(h.shape)
        assert t.data_ptr() % 16 == 8
    else:
        t = flat.cuda().view(h.shape)
        assert h.size == 0 or t.data_ptr() % 16 == 0
    return t


def _dev_pack(words):
    import torch
    return torch.full((words + GUARD,), -1, dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev_keys(look, offset4=False):
    import torch
    n, klen = look.shape
    if not offset4:
        return torch.from_numpy(look).cuda()
    buf = torch.zeros(n * klen + 16, dtype=torch.uint8, device="cuda")
    buf[4:4 + n * klen] = torch.from_numpy(look.reshape(-1))
    t = buf[4:4 + n * klen].view(n, klen)
    assert t.data_ptr() % 16 == 4
    return t


@pytest.fixture(scope="module")
def gpu_filters(gpu):
    """name -> the pool's filters on the GPU, built on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            pool = _pool(name)
            fs = []
            for f in range(pool.nf):
                b = gpu.BloomFilter(pool.m)
                b.insert_batch(pool.K[f])
                fs.append(b)
            cache[name] = fs
        return cache[name]
    return get


def _build_set(gpu, gpu_filters, case):
    pool = _pool(case.pool)
    gf = gpu_filters(case.pool)
    s = gpu.FilterSet(pool.m, case.width)
    if case.slots and None not in case.slots and not case.cleared:
        s.assign_all([gf[f] for f in case.slots])
    else:
        for slot, f in enumerate(case.slots):
            if f is not None:
                s.assign(slot, gf[f])
        for slot, f in case.cleared:
            s.assign(slot, gf[f])
            s.clear_slot(slot)
    if case.gated:
        for slot in range(case.used):
            s.set_zone(slot, _zone(pool, case.filter_of(slot)))
    assert s.used == case.used
    return s


def _dev_rows(rows, fill=-1):
    """(the [rows + 1, words] tensor filled with ones, its first `rows` rows):
    the last row is the guard."""
    import torch
    r, w = rows
    big = torch.full((r + 1, w), fill, dtype=torch.int64, device="cuda")
    return big, big[:r]


def _check_rows(big, want):
    got = big.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:-1], want)
    assert (got[-1] == ONES).all()  # the guard row


def _dev_ok():
    import torch
    buf = torch.tensor([1, -1, -1, -1], dtype=torch.int32, device="cuda")
    return buf, buf[:1]


def _check_ok(buf, want):
    assert buf.cpu().tolist() == [want, -1, -1, -1]


# ---- A: cb_hits_compress ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("rows,words", A1_SHAPES)
def test_compress_alignment(gpu, rows, words, misalign):
    """Both load forms of k_hits_compress (16-byte vector loads need a 16-byte
    aligned base) at one word either side of a block."""
    for name, h in a1_patterns(rows, words).items():
        cap = popcount(h) + 2
        pack = _dev_pack(pack_words_hits(h.size, cap))
        gpu.hits_compress(_dev_hits(h, misalign), pack, cap)
        check_pack_strict(_u32(pack), compress_blocks(h), cap)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2], ids=["cap=count", "cap=count-1", "cap=1"])
def test_compress_capacity(gpu, which):
    """The slot < cap guard: the directory sits directly behind the positions,
    so a store at slot == cap would land on the first block's base."""
    h = a2_input()
    cap = a2_caps(h)[which]
    pack = _dev_pack(pack_words_hits(h.size, cap))
    gpu.hits_compress(_dev_hits(h), pack, cap)
    pk = _u32(pack)
    assert pk[0] == popcount(h)
    check_pack_strict(pk, compress_blocks(h), cap)


def _queue_sequence(gpu, fset, seed, stream):
    """Queue the A3 launches on `stream` without a host sync; returns what to
    check after the final sync. Yields after every launch, so two sequences
    can be interleaved."""
    case = A3_PROBE
    look, rows = _case_data(case)
    steps = a3_compress_steps(seed)
    hwords = (case.n + 63) // 64
    cap_p = popcount(rows)
    todo = []
    inputs = [(name, _dev_hits(h), _dev_pack(pack_words_hits(h.size, cap)), h, cap) for name, h, cap in steps]
    keys = _dev_keys(look)
    hbig, hits = _dev_rows((case.used, hwords))
    ppack = _dev_pack(pack_words_set(case.n, cap_p))
    yield None  # everything is uploaded: the caller syncs once, then nothing waits
    for name, dh, pack, h, cap in inputs:
        if name == "one2":
            fset.probe_pack(keys, hits, ppack, cap=cap_p, stream=stream)
            todo.append(("probe", ppack, probe_blocks(rows, case.n), cap_p))
            yield None
        gpu.hits_compress(dh, pack, cap, stream=stream)
        todo.append((name, pack, compress_blocks(h), cap))
        yield None
    yield todo, hbig, rows


@pytest.mark.gpu
@pytest.mark.parametrize("nstreams", [1, 2])
def test_compress_claim_words_back_to_back(gpu, gpu_filters, nstreams):
    """The claim words alternate by launch parity on a stream and block 0
    clears the other word: many blocks, one block, no rows (no launch, no
    flip), an overflow, many blocks, the fused probe (same state) and one
    block, queued with no host sync; also interleaved over two streams, each
    with its own state."""
    import torch
    fset = _build_set(gpu, gpu_filters, A3_PROBE)
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    gens = [_queue_sequence(gpu, fset, 71 + i, st) for i, st in enumerate(streams)]
    for g in gens:
        next(g)
    torch.cuda.synchronize()
    results = [None] * nstreams
    live = list(range(nstreams))
    while live:
        for i in list(live):
            r = next(gens[i])
            if r is not None:
                results[i] = r
                live.remove(i)
    for st in streams:
        st.synchronize()
    for todo, hbig, rows in results:
        assert [t[0] for t in todo] == ["many", "one", "norows", "over", "many2", "probe", "one2"]
        for name, pack, blocks, cap in todo:
            check_pack_strict(_u32(pack), blocks, cap)
        _check_rows(hbig, rows)


# ---- B: cb_hits_expand ----------------------------------------------------------------------

def _compress_ranks(gpu, parts, cap):
    """Every rank's pack from a real cb_hits_compress at the shared cap and
    the largest shard's stride; (packs with guard words, stride)."""
    words = parts[0].shape[1]
    stride = pack_words_hits(max(p.shape[0] for p in parts) * words, cap)
    packs = _dev_pack(len(parts) * stride)
    for r, p in enumerate(parts):
        gpu.hits_compress(_dev_hits(p), packs[r * stride:(r + 1) * stride], cap)
    return packs, stride


def _expand_and_check(gpu, parts, cap, packs, stride, zero_ranks=(), with_ok=True):
    sizes = [p.shape[0] for p in parts]
    words = parts[0].shape[1]
    row_off = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    want = np.concatenate(parts, 0).copy()
    for r in zero_ranks:
        want[row_off[r]:row_off[r] + sizes[r]] = 0
    big, full = _dev_rows((sum(sizes), words))
    okbuf, ok = _dev_ok()
    before = _u32(packs)
    gpu.hits_expand(packs, len(parts), row_off, full, cap, ok=ok if with_ok else None)
    _check_rows(big, want)
    _check_ok(okbuf, 1 if not with_ok or not zero_ranks else 0)
    assert np.array_equal(_u32(packs), before) and (before[len(parts) * stride:] == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(B1_LAYOUTS))
def test_expand_rank_layouts(gpu, layout):
    """k_hits_expand finds its rank as the last r with blk_off[r] <=
    blockIdx.x: leading, trailing and adjacent empty ranks, one rank, and 64."""
    parts = make_parts(B1_LAYOUTS[layout], B1_WORDS, 11)
    cap = max(popcount(p) for p in parts) + 4
    packs, stride = _compress_ranks(gpu, parts, cap)
    for r, p in enumerate(parts):
        check_pack_strict(np.r_[_u32(packs)[r * stride:r * stride + pack_words_hits(p.size, cap)],
                                np.full(GUARD, FILL, np.uint32)], compress_blocks(p), cap)
    _expand_and_check(gpu, parts, cap, packs, stride)


@pytest.mark.gpu
def test_expand_refuses_bad_layouts(gpu):
    """65 ranks, and offsets that run past total_rows, are errors in both
    expand forms, and nothing is launched: full keeps its fill."""
    import torch
    words, n = 4, 256
    packs = torch.zeros(65 * (2 + 8 + 2) + 65 * 8, dtype=torch.int32, device="cuda")
    big, full = _dev_rows((5, words))
    bad = [(65, [0] * 65), (2, [0, 6]), (3, [0, 7, 2]), (2, [1, 2])]
    for world, row_off in bad:
        with pytest.raises(Exception):
            gpu.hits_expand(packs, world, row_off, full, 8)
        with pytest.raises(Exception):
            gpu.hits_expand_set(packs, world, row_off, n, full, 8)
    torch.cuda.synchronize()
    assert (big.cpu().numpy().view(np.uint64) == ONES).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,words", B2_CASES, ids=[f"{len(s)}ranks-w{w}" for s, w in B2_CASES])
def test_expand_block_edges(gpu, sizes, words):
    """Rank slices of exactly one block, one and a half, and one word either
    side of a block; 64 ranks of two blocks each."""
    parts = make_parts(sizes, words, 7)
    cap = max(popcount(p) for p in parts)  # the fullest rank fits exactly
    packs, stride = _compress_ranks(gpu, parts, cap)
    _expand_and_check(gpu, parts, cap, packs, stride)


@pytest.mark.gpu
@pytest.mark.parametrize("with_ok", [True, False], ids=["ok", "no_ok"])
@pytest.mark.parametrize("truncated", [False, True], ids=["count=cap", "count=cap+1"])
def test_expand_capacity(gpu, truncated, with_ok):
    """count == cap is a complete pack; a pack the kernel truncated (count ==
    cap + 1) clears ok and leaves that rank's rows zero, the others exact."""
    parts = b3_parts()
    counts = [popcount(p) for p in parts]
    big = int(np.argmax(counts))
    cap = counts[big] - (1 if truncated else 0)
    packs, stride = _compress_ranks(gpu, parts, cap)
    pk = _u32(packs)
    assert [int(pk[r * stride]) for r in range(len(parts))] == counts
    p = parts[big]
    check_pack_strict(np.r_[pk[big * stride:big * stride + pack_words_hits(p.size, cap)],
                            np.full(GUARD, FILL, np.uint32)], compress_blocks(p), cap)
    _expand_and_check(gpu, parts, cap, packs, stride, zero_ranks=(big,) if truncated else (), with_ok=with_ok)


# ---- C: the fused probe + pack, cb_hits_expand_set, the communicator ---------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", C1_CASES, ids=[c.id for c in C1_CASES])
def test_probe_pack_matches_oracle(gpu, gpu_filters, case):
    look, rows = _case_data(case)
    hwords = (case.n + 63) // 64
    cap = popcount(rows) + case.slack
    fset = _build_set(gpu, gpu_filters, case)
    hbig, hits = _dev_rows((case.used, hwords))
    pack = _dev_pack(pack_words_set(case.n, cap))
    assert gpu.FilterSet.pack_words(case.n, cap) + GUARD == pack.numel()
    fset.probe_pack(_dev_keys(look, case.offset4), hits, pack, cap=cap, gated=case.gated)
    _check_rows(hbig, rows)
    pk = _u32(pack)
    assert pk[0] == popcount(rows)
    check_pack_strict(pk, probe_blocks(rows, case.n), cap)


def _probe_ranks(gpu, gpu_filters, ranks, n, cap):
    """Every rank's probe_pack into its slice of one packs buffer; each rank's
    hit rows are checked against the oracle on the way."""
    stride = pack_words_set(n, cap)
    hwords = (n + 63) // 64
    packs = _dev_pack(len(ranks) * stride)
    look = _case_data(ranks[0], tuple(range(64)))[0]
    keys = _dev_keys(look)
    for r, c in enumerate(ranks):
        rows = _case_data(c, tuple(range(64)))[1]
        hbig, hits = _dev_rows((max(c.used, 1), hwords))
        _build_set(gpu, gpu_filters, c).probe_pack(keys, hits, packs[r * stride:(r + 1) * stride], cap=cap)
        if c.used:
            _check_rows(hbig, rows)
        else:
            assert (hbig.cpu().numpy().view(np.uint64) == ONES).all()
        check_pack_strict(np.r_[_u32(packs)[r * stride:(r + 1) * stride], np.full(GUARD, FILL, np.uint32)],
                          probe_blocks(rows, n), cap)
    return packs, stride


def _expand_set_and_check(gpu, rows, n, cap, packs, zero_ranks=(), with_ok=True):
    sizes = [r.shape[0] for r in rows]
    row_off = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    want = np.concatenate(rows, 0).copy()
    for r in zero_ranks:
        want[row_off[r]:row_off[r] + sizes[r]] = 0
    big, full = _dev_rows((sum(sizes), (n + 63) // 64))
    okbuf, ok = _dev_ok()
    gpu.hits_expand_set(packs, len(rows), row_off, n, full, cap, ok=ok if with_ok else None)
    _check_rows(big, want)
    _check_ok(okbuf, 1 if not with_ok or not zero_ranks else 0)
    assert (_u32(packs)[-GUARD:] == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", C2_N)
@pytest.mark.parametrize("layout", list(C2_LAYOUTS))
def test_expand_set_rank_layouts(gpu, gpu_filters, layout, n):
    """k_hits_expand_blocks with ranks of 64, 33, 1 and 0 rows; hwords of 17,
    33 and 1, so the last probe block is one word or the only block."""
    rows = c2_rows(layout, n)
    cap = max(popcount(r) for r in rows)  # the fullest rank fits exactly
    packs, _ = _probe_ranks(gpu, gpu_filters, c2_ranks(layout, n), n, cap)
    _expand_set_and_check(gpu, rows, n, cap, packs)


@pytest.mark.gpu
@pytest.mark.parametrize("with_ok", [True, False], ids=["ok", "no_ok"])
def test_expand_set_truncated_rank(gpu, gpu_filters, with_ok):
    """Rank 0's probe really truncated its pack (cap = count - 1): ok is
    cleared, its 64 rows are zero, the other ranks' rows are exact."""
    layout, n = "64_0_1_33", 1025
    rows = c2_rows(layout, n)
    cap = popcount(rows[0]) - 1
    packs, _ = _probe_ranks(gpu, gpu_filters, c2_ranks(layout, n), n, cap)
    _expand_set_and_check(gpu, rows, n, cap, packs, zero_ranks=(0,), with_ok=with_ok)


@pytest.fixture(scope="module")
def comm1():
    from lsmt_amd.shard import Comm
    c = Comm(0, 1, 0, Comm.unique_id())
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fits", "overflow_sync", "overflow_async"])
@pytest.mark.parametrize("form", ["probe_allgather", "allgather"])
def test_comm_world1_at_capacity(gpu, gpu_filters, comm1, form, mode):
    """Sparse mode at world size 1 with cap == count (the packs are used) and
    cap == count - 1 (the synchronous form redoes it densely; the asynchronous
    form clears ok and leaves the rows zero)."""
    import torch
    case = C3_CASE
    look, rows = _case_data(case)
    nf, hwords = rows.shape
    cap = popcount(rows) - (0 if mode == "fits" else 1)
    big, full = _dev_rows((nf, hwords))
    okbuf, ok = _dev_ok()
    use_ok = ok if mode != "overflow_sync" else None
    if form == "probe_allgather":
        lbig, local = _dev_rows((nf, hwords))
        fset = _build_set(gpu, gpu_filters, case)
        used = comm1.probe_allgather(fset, _dev_keys(look), nf, local, full, sparse=True, cap=cap, ok=use_ok)
        torch.cuda.synchronize()
        _check_rows(lbig, rows)
    else:
        used = comm1.allgather(_dev_hits(rows), nf, full, sparse=True, cap=cap, ok=use_ok)
        torch.cuda.synchronize()
    assert used == (mode != "overflow_sync")
    _check_rows(big, np.zeros_like(rows) if mode == "overflow_async" else rows)
    _check_ok(okbuf, 0 if mode == "overflow_async" else 1)
