"""The per-filter probe and build at large m and past 32 filters, and the
dense FilterSet probe at its shape limit, bit for bit against the CPU oracle
or a numpy restatement of the same operation.

Reference semantics: BloomFilter::hashes / insert / may_contain
(/root/reference/src/bloom.rs:26-51) for every table of Database::get's
fan-out (src/lib.rs:129-134).

What the shapes reach (lsmt_amd/csrc/tileprobe.hip, tilebuild.hip, direct.hip, capi_filter.cpp, capi_set.cpp,
densefs.hip):
  * k_tile_probe<8,4,2>, the 2^18-bit tile with the two-deep register ring
    (plan_probe picks it for m >= 2^27 and n <= m/64): P1, P2, P6, P7, P8;
  * k_tile_probe<8,2,4> (tb = 17) with generic m, ragged keys, a partial last
    tile and a tile count that is no multiple of 8: P3, P4;
  * the second group of 32 filters (blockIdx.y == 1, masks + g*n, km[1]) and
    the second launch past 64 filters: P5, P6;
  * the tiled<->direct hand-offs at T = kMaxTiles = 4096: m = 2^30 for the
    probe (P8), m = 2^31 for the build (B1), and m up to 2^32, the top of
    MOD_POW2_32 (B2);
  * the dense probe's kDenseMaxRegions = 4096 at widths 64 and 32 and the
    refusal just past it (D1, D2).

Two references, no tolerances:
  1. the C oracle (oracle.OracleFilter, probe_fixed, probe_var) wherever its
     byte-per-bit array is affordable (.bools() is never taken of these);
  2. a numpy restatement (np_hashes / NpRef below): h1, h2 as wrapping uint64
     folds over the key bytes, % m, a filter's state the sorted array of its
     inserted positions, hit iff np.isin(a, S) & np.isin(b, S). It needs no
     array of size m and stands in where the oracle would hold several GiB
     (P6, B1, B2). The CPU test pins it to the oracle.

The CPU test also checks, from the reference alone, that no probe case is
vacuous: each expected map holds present hits and at least MIN_A_ONLY (key,
filter) pairs whose bit a is set and bit b clear (the `&&` branch that gathers
b, src/bloom.rs:50). Two shapes needed more keys per filter than the smallest
that reaches their branch to clear that bar: P7 at m = 2^27 builds 2^20 keys
per filter (20 000 gave about 5 pairs) and P2's ragged filters take 2^18
further ragged keys each (the half batch alone gave about 55). The build
cases' follow-up probes (B1, B2: one filter of 50 000 keys in 2^28..2^32
bits, 70 001 lookups) cannot reach it at the sizes that make the case (about
13 pairs at 2^28, under 1 at 2^32): their check is the position set, and the
CPU test asserts present hits only for them.

Plan values in the comments come from plan_probe / plan_build (tileplan.cpp);
tests/tileplan_ref.py restates them and the CPU test asserts each comment's
values against it (tests/test_tileplan_cpu.py asserts them against the C++).
"""
import functools

import numpy as np
import pytest

import tileplan_ref
from lsmt_amd import workload
from oracle import oracle

DIRECT, TILED, AUTO = 1, 2, 0
SET_PATH, DENSE_PATH = 3, 6
MIN_A_ONLY = 100
U64 = np.uint64


# ---- the numpy restatement -------------------------------------------------------

def var_batch(data, offs):
    return (np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offs, np.uint64))


def var_take(batch, idx):
    """The ragged batch of keys idx (in that order) of a ragged batch."""
    data, offs = batch
    o = offs.astype(np.int64)
    idx = np.asarray(idx, np.int64)
    lens = o[idx + 1] - o[idx]
    out = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=out[1:])
    src = np.repeat(o[idx] - out[:-1], lens) + np.arange(out[-1])
    return var_batch(data[src] if out[-1] else np.zeros(1, np.uint8), out)


def batch_len(b):
    return len(b[1]) - 1 if isinstance(b, tuple) else len(b)


def np_hashes(b):
    """(h1, h2) of src/bloom.rs:29-34 for every key of a batch (uint8 [n, L]
    rows, or ragged (data, offsets)): u64 wrapping folds, h1 from 5381 by 33,
    h2 from 0 by 31."""
    n = batch_len(b)
    h1 = np.full(n, 5381, U64)
    h2 = np.zeros(n, U64)
    with np.errstate(over="ignore"):
        if isinstance(b, tuple):
            data, offs = b
            o = offs.astype(np.int64)
            lens = np.diff(o)
            for j in range(int(lens.max(initial=0))):
                act = np.flatnonzero(lens > j)
                c = data[o[act] + j].astype(U64)
                h1[act] = h1[act] * U64(33) + c
                h2[act] = h2[act] * U64(31) + c
        else:
            for j in range(b.shape[1]):
                c = b[:, j].astype(U64)
                h1 = h1 * U64(33) + c
                h2 = h2 * U64(31) + c
    return h1, h2


@functools.lru_cache(maxsize=None)
def _seed_hashes(seed, n):
    h1, h2 = np_hashes(workload.key_range(seed, n))
    h1.setflags(write=False)
    h2.setflags(write=False)
    return h1, h2


class Range:
    """key_range(seed, n), optionally cut to its first `cut` bytes; the raw
    hashes of the uncut 16-byte keys are computed once per seed."""

    def __init__(self, seed, n, cut=16):
        assert n <= 1 << 20
        self.seed, self.n, self.cut = seed, n, cut

    def keys(self):
        k = workload.key_range(self.seed, self.n)
        return k if self.cut == 16 else np.ascontiguousarray(k[:, :self.cut])

    def hashes(self):
        if self.cut != 16:
            return np_hashes(self.keys())
        # (the five seeds of the large cases are folded once, at their longest)
        h1, h2 = _seed_hashes(self.seed, 1 << 20 if self.seed < SEED + 5 else self.n)
        return h1[:self.n], h2[:self.n]


def keys_of(b):
    return b.keys() if isinstance(b, Range) else b


def hashes_of(b):
    return b.hashes() if isinstance(b, Range) else np_hashes(b)


def positions(hs, m):
    return hs[0] % U64(m), hs[1] % U64(m)


def position_set(batches, m):
    """A filter's state: the sorted positions its inserted keys set."""
    return np.unique(np.concatenate([p for b in batches for p in positions(hashes_of(b), m)]))


def pack_bits(hit):
    """bool[n] -> uint64[ceil(n/64)], bit k%64 of word k/64 = hit[k]."""
    by = np.packbits(hit, bitorder="little")
    out = np.zeros((len(hit) + 63) // 64 * 8, np.uint8)
    out[:len(by)] = by
    return out.view("<u8").astype(np.uint64)


class Case:
    """ms[f] bits and builds[f] (a list of key batches) per filter; one lookup batch."""

    def __init__(self, ms, builds, look):
        assert len(ms) == len(builds)
        self.ms, self.builds, self.look = list(ms), [list(b) for b in builds], look

    @property
    def n(self):
        return batch_len(self.look)

    def np_ref(self, nf=None):
        """(hit words [nf, ceil(n/64)], present hits, a-set/b-clear pairs) by
        the numpy restatement, over the first nf filters."""
        lh = hashes_of(self.look)
        rows, hits, a_only, pos = [], 0, 0, {}
        for m, bs in list(zip(self.ms, self.builds))[:nf]:
            if m not in pos:
                pos[m] = positions(lh, m)
            a, b = pos[m]
            S = position_set(bs, m)
            ina, inb = np.isin(a, S), np.isin(b, S)
            rows.append(pack_bits(ina & inb))
            hits += int((ina & inb).sum())
            a_only += int((ina & ~inb).sum())
        return np.stack(rows), hits, a_only

    def oracle_filters(self):
        refs = []
        for m, bs in zip(self.ms, self.builds):
            o = oracle.OracleFilter(m)
            for b in bs:
                k = keys_of(b)
                if isinstance(k, tuple):
                    o.insert_var(*k)
                else:
                    o.insert_fixed(k)
            refs.append(o)
        return refs

    def oracle_ref(self, refs=None, threads=1):
        refs = self.oracle_filters() if refs is None else refs
        if isinstance(self.look, tuple):
            return oracle.probe_var(refs, *self.look, threads=threads)
        return oracle.probe_fixed(refs, self.look, threads=threads)

    def gpu_filters(self, gpu):
        fs = []
        for m, bs in zip(self.ms, self.builds):
            f = gpu.BloomFilter(m)
            for b in bs:
                f.insert_batch(as_gpu_batch(gpu, keys_of(b)))
            fs.append(f)
        return fs

    def gpu_look(self, gpu):
        return as_gpu_batch(gpu, self.look)


def as_gpu_batch(gpu, k):
    if isinstance(k, tuple):
        return gpu.KeyBatch(n=batch_len(k), data=k[0], offsets=k[1])
    return k


# ---- the shapes ----------------------------------------------------------------------
# Filter f of the key_range cases is built from key_range(SEED + f, ...): the
# seeds are shared so that one fold per seed serves every case on the CPU.

SEED = 1100
K19, K20 = 1 << 19, 1 << 20


def _ranges(nf, kpf, cut=16):
    return [[Range(SEED + f, kpf, cut)] for f in range(nf)]


def _lookups(n, nf, kpf, absent):
    return workload.probe_lookups(n, nf, kpf, seed_base=SEED, absent_seed=absent)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "P1":  # tb 18, T 512, kpt 4: k_tile_probe<8,4,2>
        return Case([1 << 27] * 3, _ranges(3, K19), _lookups(100_000, 3, K19, 981))
    if name == "P2":  # tb 18, T 513 (partial last tile, T % 8 != 0), kpt 4, MOD_GENERIC
        return Case([(1 << 27) + 12345] * 3, _ranges(3, K19), _lookups(70_001, 3, K19, 982))
    if name == "P2_fixed7":  # the same plan, KEY_FIXED
        look = np.ascontiguousarray(_lookups(70_001, 3, K19, 982)[:, :7])
        return Case([(1 << 27) + 12345] * 3, _ranges(3, K19, cut=7), look)
    if name == "P2_var":  # the same plan, KEY_VAR: the first half of the lookups is in every filter
        rng = np.random.default_rng(27)
        look = var_batch(*workload.var_keys(rng, 70_001, max_len=40))
        half = var_take(look, np.arange(35_000))
        extra = [var_batch(*workload.var_keys(rng, 1 << 18, max_len=40)) for _ in range(3)]
        return Case([(1 << 27) + 12345] * 3, [[half, e] for e in extra], look)
    if name == "P3":  # tb 17, T 513, kpt 8, MOD_GENERIC; n % 64 != 0, n % 2048 != 0
        return Case([(1 << 26) + 9] * 5, _ranges(5, K19), _lookups(K20 + 777, 5, K19, 983))
    if name == "P4":  # tb 17 (held down by density, not by m), T 1024, kpt 8
        return Case([1 << 27] * 3, _ranges(3, K19), _lookups(3_000_000, 3, K19, 984))
    if name == "P5":  # tb 16, T 16, kpt 4; rows [:nf] serve nf = 33, 37, 64, 65, 70
        return Case([1 << 20] * 70, _ranges(70, 3000), _lookups(70_001, 70, 3000, 985))
    if name == "P5_mixed":  # 40 filters of 2^20 bits interleaved with 35 of 2^20 + 5
        ms = [(1 << 20) + 5 if (f % 2 and f < 70) else 1 << 20 for f in range(75)]
        assert ms.count(1 << 20) == 40
        return Case(ms, _ranges(75, 3000), _lookups(70_001, 75, 3000, 986))
    if name == "P6":  # tb 18, T 512, kpt 4, D = 2; rows [:33] serve nf = 33
        return Case([1 << 27] * 34, _ranges(34, 1 << 17), _lookups(100_000, 34, 1 << 17, 987))
    if name in ("P7_20", "P7_27"):  # tb 16, T 16 / tb 18, T 512; kpt 4, 208 blocks
        m, kpf = (1 << 20, 20_000) if name == "P7_20" else (1 << 27, K20)
        look = np.concatenate([np.repeat(workload.key_range(SEED + 3, 1), 200_000, axis=0),
                               np.repeat(workload.key_range(999_999, 1), 9000, axis=0),
                               workload.key_range(SEED + 1, 3000)])
        return Case([m] * 5, _ranges(5, kpf), look)
    if name in ("P8_30", "P8_30p1"):  # 2^30: tb 18, T 4096 = kMaxTiles, kpt 4; 2^30 + 1: direct
        m = (1 << 30) + (name == "P8_30p1")
        return Case([m] * 2, _ranges(2, K20), _lookups(70_001, 2, K20, 988))
    if name.startswith("B_"):  # one filter: 40 000 keys, then 10 000 others; half the lookups absent
        m = int(name[2:])
        return Case([m], [[Range(SEED, 40_000), Range(SEED + 1, 10_000)]], _lookups(70_001, 2, 10_000, 989))
    if name == "D1_var":  # ragged lookups, their first half dealt over the filters
        rng = np.random.default_rng(64)
        look = var_batch(*workload.var_keys(rng, 60_000, max_len=40))
        c = Case([D1_TAIL] * 37, _ranges(37, 9000), look)
        for f in range(37):
            c.builds[f].append(var_take(look, np.arange(f, 30_000, 37)))
        return c
    if name.startswith("D1_"):  # width 64: 37 filters of 9000 keys
        m = int(name[3:])
        builds = case("D1_var").builds if m == D1_TAIL else _ranges(37, 9000)
        return Case([m] * 37, builds, _lookups(120_000, 37, 9000, 990))
    if name.startswith("D2_"):  # width 32: 7 filters of 9000 keys
        return Case([int(name[3:])] * 7, _ranges(7, 9000), _lookups(120_000, 7, 9000, 991))
    raise KeyError(name)


D1_TAIL = (1 << 25) - 5  # R = 4096 regions of 8192 rows, the last one partial
B1_MS = [(1 << 28) + 7, 1 << 30, (1 << 31) - 12345, 1 << 31]
B2_MS = [(1 << 31) + 1, (1 << 32) - 5, 1 << 32]
D1_MS = [1 << 25, D1_TAIL, (1 << 25) + 1]
D2_MS = [1 << 26, (1 << 26) + 1]

# (case, filters the smallest run of it takes)
PROBE_CASES = [("P1", None), ("P2", None), ("P2_fixed7", None), ("P2_var", None), ("P3", None), ("P4", None),
               ("P5", 33), ("P5_mixed", None), ("P6", 33), ("P7_20", None), ("P7_27", None), ("P8_30", None),
               ("P8_30p1", None), ("D1_var", None)] + [(f"D1_{m}", None) for m in D1_MS] + \
              [(f"D2_{m}", None) for m in D2_MS]


def _plan_probe(m, n):
    """plan_probe (tileplan.cpp) by its restatement: (tb, T, kpt, partition blocks)."""
    p = tileplan_ref.plan_probe(m, n)
    return p.tb, p.T, p.kpt, p.nblk


# ---- the CPU test -----------------------------------------------------------------------

def test_numpy_reference_matches_oracle_and_cases_are_not_vacuous():
    # (1) the restatement against the C oracle: positions and whole hit maps
    rng = np.random.default_rng(5)
    fixed16 = workload.key_range(77, 3000)
    fixed7 = rng.integers(0, 256, size=(3000, 7), dtype=np.uint8)
    ragged = var_batch(*workload.var_keys(rng, 3000, max_len=40))
    absent = {id(fixed16): workload.key_range(78, 3000),
              id(fixed7): rng.integers(0, 256, size=(3000, 7), dtype=np.uint8),
              id(ragged): var_batch(*workload.var_keys(rng, 3000, max_len=40))}
    for m in (1000, 100_003, (1 << 27) + 12345, 1 << 30, (1 << 32) - 5, 1 << 32):
        for b in (fixed16, fixed7, ragged):
            a, bb = positions(np_hashes(b), m)
            for k in range(0, 3000, 10):
                key = bytes(b[0][int(b[1][k]):int(b[1][k + 1])]) if isinstance(b, tuple) else bytes(b[k])
                h1, h2 = oracle.raw_hashes(key)
                assert (int(a[k]), int(bb[k])) == (h1 % m, h2 % m), (m, k)
            o = oracle.OracleFilter(m)
            if isinstance(b, tuple):
                o.insert_var(*b)
                look = var_batch(np.concatenate([b[0][:int(b[1][-1])], absent[id(b)][0]]),
                                 np.concatenate([b[1], absent[id(b)][1][1:] + b[1][-1]]))
                exp = oracle.probe_var([o], *look)
            else:
                o.insert_fixed(b)
                look = np.concatenate([b, absent[id(b)]])
                exp = oracle.probe_fixed([o], look)
            got, hits, _ = Case([m], [[b]], look).np_ref()
            assert np.array_equal(got, exp), m
            assert hits >= 3000
            del o

    # (2) the plan values the cases' comments state
    assert _plan_probe(1 << 27, 100_000) == (18, 512, 4, 98)                   # P1, P6
    assert _plan_probe((1 << 27) + 12345, 70_001) == (18, 513, 4, 69)          # P2
    assert _plan_probe((1 << 26) + 9, K20 + 777) == (17, 513, 8, 513)          # P3
    assert _plan_probe(1 << 27, 3_000_000) == (17, 1024, 8, 1465)              # P4
    assert _plan_probe(1 << 20, 70_001) == (16, 16, 4, 69)                     # P5
    assert _plan_probe((1 << 20) + 5, 70_001) == (16, 17, 4, 69)               # P5_mixed
    assert _plan_probe(1 << 20, 212_000) == (16, 16, 4, 208)                   # P7
    assert _plan_probe(1 << 27, 212_000) == (18, 512, 4, 208)                  # P7
    assert _plan_probe(1 << 30, 70_001) == (18, 4096, 4, 69)                   # P8, B1
    assert _plan_probe((1 << 28) + 7, 70_001) == (18, 1025, 4, 69)             # B1
    assert [-(-m // (1 << 19)) for m in B1_MS] == [513, 2048, 4096, 4096]      # plan_build: tb 19
    assert case("P3").n % 64 and case("P3").n % 2048

    # (3) no probe case is vacuous, judged from the reference alone
    for name, nf in PROBE_CASES:
        _, hits, a_only = case(name).np_ref(nf)
        assert hits > 0, name
        assert a_only >= MIN_A_ONLY, (name, a_only)
    for m in B1_MS + B2_MS:
        _, hits, _ = case(f"B_{m}").np_ref()
        assert hits >= 35_000, m


# ---- GPU cases: the per-filter probe --------------------------------------------------------

gpu_test = pytest.mark.gpu


@pytest.fixture
def auto_path(gpu):
    gpu.set_path(AUTO)
    yield gpu
    gpu.set_path(AUTO)


@pytest.fixture
def dense(gpu):
    gpu.set_dense(1)
    yield gpu
    gpu.set_dense(0)


@pytest.fixture(scope="module")
def c2_filters(gpu):
    """Three filters of 2^27 bits, 2^19 keys each (P1, P4), with their oracles."""
    c = case("P1")
    return c.gpu_filters(gpu), c.oracle_filters()


@gpu_test
def test_p1_tb18_two_deep_ring(auto_path, c2_filters):
    gpu = auto_path
    filters, refs = c2_filters
    c = case("P1")
    exp = c.oracle_ref(refs)
    assert np.array_equal(gpu.probe(filters, c.look), exp)
    assert gpu.last_path() == TILED
    one = filters[0].may_contain_batch(c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(one, gpu.unpack_hits(exp[:1], c.n)[0])


@gpu_test
@pytest.mark.parametrize("name", ["P2", "P2_fixed7", "P2_var"])
def test_p2_tb18_generic_m_partial_last_tile(auto_path, name):
    gpu = auto_path
    c = case(name)
    got = gpu.probe(c.gpu_filters(gpu), c.gpu_look(gpu))
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref())


@gpu_test
def test_p3_tb17_generic_m_ragged_n(auto_path):
    gpu = auto_path
    c = case("P3")
    got = gpu.probe(c.gpu_filters(gpu), c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref(threads=8))


@gpu_test
def test_p4_tb17_by_density(auto_path, c2_filters):
    gpu = auto_path
    filters, refs = c2_filters
    c = case("P4")
    got = gpu.probe(filters, c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref(refs, threads=8))


@pytest.fixture(scope="module")
def p5(gpu):
    c = case("P5")
    return c, c.gpu_filters(gpu), c.oracle_ref()


@gpu_test
@pytest.mark.parametrize("path", [AUTO, TILED], ids=["auto", "tiled"])
@pytest.mark.parametrize("nf", [33, 37, 64, 65, 70])
def test_p5_second_mask_plane_and_second_launch(auto_path, p5, nf, path):
    gpu = auto_path
    c, filters, exp = p5
    gpu.set_path(path)
    got = gpu.probe(filters[:nf], c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, exp[:nf])


@gpu_test
def test_p5_rows_land_by_argument_order(auto_path):
    gpu = auto_path
    c = case("P5_mixed")
    got = gpu.probe(c.gpu_filters(gpu), c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref())


@pytest.fixture(scope="module")
def p6(gpu):
    c = case("P6")
    return c, c.gpu_filters(gpu), c.np_ref()[0]


@gpu_test
@pytest.mark.parametrize("nf", [33, 34])
def test_p6_second_group_in_the_two_deep_ring(auto_path, p6, nf):
    gpu = auto_path
    c, filters, exp = p6
    got = gpu.probe(filters[:nf], c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, exp[:nf])


@gpu_test
@pytest.mark.parametrize("name", ["P7_20", "P7_27"])
def test_p7_every_entry_in_one_tile(auto_path, name):
    # 200 000 copies of one key: one tile takes every entry of every partition
    # block (the cbase multi-chunk loop, seg_find over runs as long as a block)
    gpu = auto_path
    c = case(name)
    got = gpu.probe(c.gpu_filters(gpu), c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref())


@gpu_test
def test_p8_tiled_limit_then_direct(auto_path):
    gpu = auto_path
    c = case("P8_30")
    got = gpu.probe(c.gpu_filters(gpu), c.look)
    assert gpu.last_path() == TILED
    assert np.array_equal(got, c.oracle_ref())
    c = case("P8_30p1")
    filters, exp = c.gpu_filters(gpu), c.oracle_ref()
    for path in (AUTO, TILED):  # past probe_tiled_ok even the forced path is direct
        gpu.set_path(path)
        got = gpu.probe(filters, c.look)
        assert gpu.last_path() == DIRECT
        assert np.array_equal(got, exp)


# ---- GPU cases: builds -------------------------------------------------------------------------

def packed_positions(words):
    """The positions of the set bits of a filter's packed uint32 words."""
    nz = np.flatnonzero(words)
    bits = np.unpackbits(np.ascontiguousarray(words[nz]).astype("<u4").view(np.uint8).reshape(-1, 4),
                         axis=1, bitorder="little")
    w, b = np.nonzero(bits)
    return nz[w].astype(U64) * U64(32) + b.astype(U64)


def _build_case(gpu, m, tiled_build, tiled_probe):
    c = case(f"B_{m}")
    first, second = c.builds[0]
    f = gpu.BloomFilter(m)
    f.insert_batch(first.keys())  # n = 40 000 >= 2^15: AUTO builds tiled wherever build_tiled_ok
    assert gpu.last_path() == (TILED if tiled_build else DIRECT)
    assert np.array_equal(packed_positions(f.packed()), position_set([first], m))
    # the second batch ORs into the non-empty filter (under 2^15 keys AUTO is
    # direct: the tiled cases force the tile pass that loads the tile first)
    gpu.set_path(TILED if tiled_build else AUTO)
    f.insert_batch(second.keys())
    assert gpu.last_path() == (TILED if tiled_build else DIRECT)
    gpu.set_path(AUTO)
    assert np.array_equal(packed_positions(f.packed()), position_set([first, second], m))
    got = f.may_contain_batch(c.look)
    assert gpu.last_path() == (TILED if tiled_probe else DIRECT)
    assert np.array_equal(got, gpu.unpack_hits(c.np_ref()[0], c.n)[0])


@gpu_test
@pytest.mark.parametrize("m", B1_MS)
def test_b1_tiled_build_up_to_its_limit(auto_path, m):
    # tb 19: T = 513 (partial last tile), 2048, 4096, 4096 = kMaxTiles, the last
    # value the packed entry's 12-bit tile field holds; kpt 1, 40 blocks
    _build_case(auto_path, m, tiled_build=True, tiled_probe=m <= 1 << 30)


@gpu_test
@pytest.mark.parametrize("m", B2_MS)
def test_b2_direct_build_up_to_2_pow_32(auto_path, m):
    # past build_tiled_ok; 2^32 is the top of MOD_POW2_32 (the mask is all ones)
    _build_case(auto_path, m, tiled_build=False, tiled_probe=False)


# ---- GPU cases: the dense probe's shape limit ------------------------------------------------------

def _dense_case(gpu, name, width, path):
    c = case(name)
    s = gpu.FilterSet.from_filters(c.gpu_filters(gpu), width=width)
    got = s.probe(c.gpu_look(gpu))
    assert gpu.last_path() == path
    assert np.array_equal(got, c.oracle_ref())


@gpu_test
@pytest.mark.parametrize("m,path", [(D1_MS[0], DENSE_PATH), (D1_MS[1], DENSE_PATH), (D1_MS[2], SET_PATH)])
def test_d1_width64_region_limit(dense, m, path):
    # R = 4096, 4096 with a partial last region, 4097: refused, k_set_probe answers
    _dense_case(dense, f"D1_{m}", 64, path)


@gpu_test
def test_d1_width64_ragged_keys_at_the_limit(dense):
    _dense_case(dense, "D1_var", 64, DENSE_PATH)


@gpu_test
@pytest.mark.parametrize("m,path", [(D2_MS[0], DENSE_PATH), (D2_MS[1], SET_PATH)])
def test_d2_width32_region_limit(dense, m, path):
    _dense_case(dense, f"D2_{m}", 32, path)
