"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the
golden fixtures. Bit-exact for every bit array and every hit bitmap.

Reference semantics: /root/reference/src/bloom.rs:17-77; callers
src/sstable.rs:59-65,138 and src/lib.rs:129-134.
"""
import hashlib

import numpy as np
import pytest

from lsmt_amd import workload
from oracle import oracle

pytestmark = pytest.mark.gpu

DIRECT, TILED, AUTO = 1, 2, 0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(params=[DIRECT, TILED], ids=["direct", "tiled"])
def path(request, gpu):
    gpu.set_path(request.param)
    yield request.param
    gpu.set_path(AUTO)


def build_pair(gpu, m, keys):
    g = gpu.BloomFilter(m)
    g.insert_batch(keys)
    o = oracle.OracleFilter(m)
    if isinstance(keys, np.ndarray):
        o.insert_fixed(keys)
    else:
        for k in keys:
            o.insert(k.encode() if isinstance(k, str) else k)
    return g, o


# ---- the reference's own tests, through the GPU path ----------------------------

def test_reference_bloom_test(gpu):
    # tests/bloom_test.rs:3-8
    b = gpu.BloomFilter.new(128)
    b.insert("hello")
    assert b.may_contain("hello")
    assert list(np.flatnonzero(b.bools())) == [25, 82]


def test_reference_scenarios(gpu, golden):
    for name, s in golden["scenarios"].items():
        b = gpu.BloomFilter(s["m"])
        for k in s["insert_hex"]:
            b.insert(bytes.fromhex(k))  # queued, flushed as one batch
        assert [b.may_contain(bytes.fromhex(k)) for k in s["probe_hex"]] == s["probe"], name
        assert list(np.flatnonzero(b.bools())) == s["set_bits"], name
        assert b.to_bytes().hex() == s["to_bytes_hex"], name


def test_sstable_local_roundtrip(gpu):
    # tests/sstable_local_test.rs:12 — loaded.bloom.to_bytes() == table.bloom.to_bytes()
    b = gpu.BloomFilter(1024)
    b.insert("k")
    data = b.to_bytes()
    assert gpu.BloomFilter.from_bytes(data).to_bytes() == data
    p = b.to_proto()
    assert gpu.BloomFilter.from_proto(p).to_bytes() == data


# ---- build parity ---------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 64, 1000, 1024, 4097, 100003, 1 << 17, (1 << 20) + 7,
                               1 << 21, 3 << 20, 1 << 22])
def test_build_fixed16(gpu, path, m):
    keys = workload.key_range(1, 20_000)
    g, o = build_pair(gpu, m, keys)
    assert np.array_equal(g.bools(), o.bools())


@pytest.mark.parametrize("key_len", [0, 1, 7, 15, 17, 33])
def test_build_fixed_other_lengths(gpu, path, key_len):
    rng = np.random.default_rng(key_len)
    keys = rng.integers(0, 256, size=(5000, key_len), dtype=np.uint8)
    for m in (4099, 1 << 20):
        g, o = build_pair(gpu, m, keys)
        assert np.array_equal(g.bools(), o.bools()), (key_len, m)


def test_build_var(gpu, path):
    rng = np.random.default_rng(7)
    data, offs = workload.var_keys(rng, 30_000, max_len=64)
    keys = [bytes(data[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    for m in (100003, 1 << 20, (1 << 21) + 1):
        g = gpu.BloomFilter(m)
        g.insert_batch(gpu.KeyBatch(n=len(keys), data=data, offsets=offs))
        o = oracle.OracleFilter(m)
        o.insert_var(data, offs)
        assert np.array_equal(g.bools(), o.bools()), m
        # the list-of-bytes form builds the same ragged batch
        h = gpu.BloomFilter(m)
        h.insert_batch(keys)
        assert np.array_equal(h.bools(), o.bools())


def test_build_unaligned_fixed16(gpu, path):
    keys = workload.key_range(9, 10_001)
    raw = np.zeros(16 * 10_001 + 3, np.uint8)
    view = raw[3:].reshape(10_001, 16)  # 3-byte misaligned rows
    view[:] = keys
    g = gpu.BloomFilter(1 << 20)
    g.insert_batch(gpu.KeyBatch(n=10_001, key_len=16, keys=view))
    o = oracle.OracleFilter(1 << 20)
    o.insert_fixed(keys)
    assert np.array_equal(g.bools(), o.bools())


def test_build_incremental_and_idempotent(gpu, path):
    a = workload.key_range(11, 50_000)
    b = workload.key_range(12, 70_000)
    m = 1 << 21
    g1 = gpu.BloomFilter(m)
    g1.insert_batch(a)
    g1.insert_batch(b)  # second batch ORs into a non-empty filter
    g2 = gpu.BloomFilter(m)
    g2.insert_batch(np.concatenate([b, a]))
    g2.insert_batch(a)  # idempotent
    o = oracle.OracleFilter(m)
    o.insert_fixed(a)
    o.insert_fixed(b)
    assert np.array_equal(g1.bools(), o.bools())
    assert np.array_equal(g2.packed(), g1.packed())


def test_build_skewed_runs(gpu, path):
    # Duplicate keys pile every entry of a partition block into two tiles, so
    # runs exceed one wave (64 entries) and one tile takes most of the batch.
    base = workload.key_range(31, 3000)
    keys = np.concatenate([np.repeat(base[:1], 200_000, axis=0), base,
                           np.repeat(base[7:8], 70_001, axis=0)])
    for m in (1 << 20, 1 << 27, 100003):
        g, o = build_pair(gpu, m, keys)
        assert np.array_equal(g.bools(), o.bools()), m


@pytest.mark.parametrize("m", [(1 << 32) + 15, 1 << 33])
def test_build_64bit_modes(gpu, m):
    # m > 2^32: 64-bit state (mask or exact 64-bit fastmod). Checked by set positions.
    keys = workload.key_range(21, 4000)
    g = gpu.BloomFilter(m)
    g.insert_batch(keys)
    pos = set()
    for k in keys:
        h1, h2 = oracle.raw_hashes(bytes(k))
        pos.add(h1 % m)
        pos.add(h2 % m)
    words = g.packed()
    nz = np.flatnonzero(words)
    got = set()
    for w in nz:
        v = int(words[w])
        while v:
            lsb = v & -v
            got.add(int(w) * 32 + lsb.bit_length() - 1)
            v ^= lsb
    assert got == pos
    assert g.may_contain_batch(keys).all()


def test_c2_build_golden(gpu, golden, path):
    g = golden["c2"]
    f = gpu.BloomFilter(g["m"])
    f.insert_batch(workload.c2_build_keys(g["n"]))
    assert sha(f.bools()) == g["bools_sha256"]
    assert sha(f.packed().view(np.uint8)) == g["packed_sha256"]


# ---- probe parity ------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 70_001])
def test_probe_sizes(gpu, path, n):
    m = 1 << 20
    filters, refs = [], []
    for f in range(5):
        g, o = build_pair(gpu, m, workload.key_range(100 + f, 30_000))
        filters.append(g)
        refs.append(o)
    look = workload.probe_lookups(n, 5, 30_000, seed_base=100, absent_seed=999)
    assert np.array_equal(gpu.probe(filters, look), oracle.probe_fixed(refs, look))


def test_probe_mixed_m_and_many_filters(gpu, path):
    ms = [1024, 100003, 1 << 20, (1 << 20) + 5, 1 << 21]
    filters, refs = [], []
    for f in range(70):  # > 64 filters: several launches per size group
        m = ms[f % len(ms)]
        g, o = build_pair(gpu, m, workload.key_range(300 + f, 3000))
        filters.append(g)
        refs.append(o)
    look = workload.probe_lookups(100_000, 70, 3000, seed_base=300, absent_seed=998)
    assert np.array_equal(gpu.probe(filters, look), oracle.probe_fixed(refs, look))


def test_probe_var_keys(gpu, path):
    rng = np.random.default_rng(3)
    data, offs = workload.var_keys(rng, 80_000, max_len=40)
    half = 40_000
    filters, refs = [], []
    for m in (4099, 1 << 20, 1 << 21):
        g = gpu.BloomFilter(m)
        g.insert_batch(gpu.KeyBatch(n=half, data=data, offsets=offs[: half + 1]))
        o = oracle.OracleFilter(m)
        o.insert_var(data, offs[: half + 1])
        filters.append(g)
        refs.append(o)
    hits = gpu.probe(filters, gpu.KeyBatch(n=80_000, data=data, offsets=offs))
    assert np.array_equal(hits, oracle.probe_var(refs, data, offs))


def test_probe_empty_and_zero(gpu):
    f = gpu.BloomFilter(1 << 20)
    f.insert_batch(workload.key_range(1, 10))
    h = gpu.probe([f], np.zeros((0, 16), np.uint8))
    assert h.shape == (1, 0)
    z = gpu.BloomFilter(0)
    with pytest.raises(ZeroDivisionError):
        z.insert("x")
    with pytest.raises(ZeroDivisionError):
        z.may_contain("x")
    with pytest.raises(ZeroDivisionError):
        gpu.probe([f, z], workload.key_range(1, 3))
    assert z.to_bytes() == b""
    assert gpu.BloomFilter.from_bytes(b"").m == 0


def test_c3_probe_golden(gpu, golden, path):
    g = golden["c3"]
    filters = []
    for f in range(g["nf"]):
        b = gpu.BloomFilter(g["m"])
        b.insert_batch(workload.c3_filter_keys(f, g["keys_per_filter"]))
        filters.append(b)
    look = workload.c3_lookups(g["n_lookups"], g["nf"], g["keys_per_filter"])
    hits = gpu.probe(filters, look)
    assert sha(hits.astype("<u8")) == g["hits_sha256"]


# ---- codec -------------------------------------------------------------------------

def test_codec_matches_oracle(gpu):
    for m in (1, 127, 128, 129, 16384, 100003):
        g, o = build_pair(gpu, m, workload.key_range(4, 500))
        data = g.to_bytes()
        assert data == o.to_bytes()
        back = gpu.BloomFilter.from_bytes(data)
        assert back.m == m and np.array_equal(back.bools(), o.bools())
    unpacked = bytes([0x08, 0x01, 0x08, 0x00, 0x08, 0x05, 0x10, 0x07, 0x0A, 0x03, 0x00, 0x81, 0x01])
    f = gpu.BloomFilter.from_bytes(unpacked)
    assert list(f.bools()) == list(oracle.OracleFilter.from_bytes(unpacked).bools())
    for bad in (b"\x0a", b"\x0a\x05\x01", b"\x00", b"\x0d\x00\x00\x00\x00", b"\xff" * 11):
        with pytest.raises(ValueError):
            gpu.BloomFilter.from_bytes(bad)


def test_codec_pinned_to_the_protobuf_wire_format(gpu):
    """BloomFilter.to_bytes / from_bytes on the device against wire bytes
    written from the protobuf encoding spec (tests/test_oracle.py _wire)."""
    from tests.test_oracle import _wire
    for m in (1, 10, 127, 128, 130, 300, 16384):
        rng = np.random.default_rng(m)
        bits = [int(x) for x in rng.integers(0, 2, m)]
        wire = _wire(bits)
        f = gpu.BloomFilter.from_bytes(wire)
        assert f.m == m and list(f.bools()) == bits
        assert f.to_bytes() == wire


def test_packed_import_masks_tail(gpu):
    f = gpu.BloomFilter(40)
    f.load_packed(np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint32))
    assert int(f.bools().sum()) == 40
    assert f.packed()[1] == 0xFF


# ---- device-resident buffers and streams ----------------------------------------

def test_device_resident_keys_and_hits(gpu):
    import torch
    dev = torch.device("cuda:0")
    keys = workload.key_range(100, 200_000)
    dk = torch.from_numpy(keys).to(dev)
    s = torch.cuda.Stream()
    f = gpu.BloomFilter(1 << 22)
    with torch.cuda.stream(s):
        f.insert_batch(gpu.DeviceKeys(dk), stream=s)
        look = torch.from_numpy(workload.probe_lookups(300_000, 1, 200_000, 100, 999)).to(dev)
        out = torch.zeros((1, (300_000 + 63) // 64), dtype=torch.int64, device=dev)
        gpu.probe([f], gpu.DeviceKeys(look), out=out, stream=s)
    s.synchronize()
    o = oracle.OracleFilter(1 << 22)
    o.insert_fixed(keys)
    expect = oracle.probe_fixed([o], look.cpu().numpy())
    assert np.array_equal(out.cpu().numpy().view(np.uint64), expect)


# ---- bit-sliced filter sets ----------------------------------------------------------

@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("m", [1, 1000, 100003, 1 << 20, (1 << 21) + 3])
def test_filterset_probe_matches_oracle(gpu, width, m):
    nf = 5 if width == 32 else 37
    filters, refs = [], []
    for f in range(nf):
        g, o = build_pair(gpu, m, workload.key_range(500 + f, 4000))
        filters.append(g)
        refs.append(o)
    s = gpu.FilterSet.from_filters(filters, width=width)
    assert s.used == nf
    look = workload.probe_lookups(50_001, nf, 4000, seed_base=500, absent_seed=997)
    expect = oracle.probe_fixed(refs, look)
    assert np.array_equal(s.probe(look), expect)
    # the per-filter multi-probe agrees with the set
    assert np.array_equal(gpu.probe(filters, look), expect)


@pytest.mark.parametrize("width", [32, 64])
def test_filterset_zero_copy_host_buffers(gpu, width):
    # Pinned host keys and hits take the zero-copy path (the kernel reads keys
    # and writes hit rows over PCIe); a ragged last word; plain and zone-gated
    # answers must match the oracle / the device-resident path bit for bit.
    import torch
    m, nf, kpf = 1 << 20, (7 if width == 32 else 40), 3000
    filters, refs = [], []
    for f in range(nf):
        g, o = build_pair(gpu, m, workload.key_range(600 + f, kpf))
        filters.append(g)
        refs.append(o)
    s = gpu.FilterSet.from_filters(filters, width=width)
    n = 4 * (1 << 18) + 12_345
    look = workload.probe_lookups(n, nf, kpf, seed_base=600, absent_seed=996)
    expect = oracle.probe_fixed(refs, look)
    keys = torch.from_numpy(look).pin_memory()
    out = torch.zeros((nf, (n + 63) // 64), dtype=torch.int64).pin_memory()
    s.probe(gpu.KeyBatch(n=n, key_len=16, keys=keys), out=out)
    assert gpu.last_path() == 4
    assert np.array_equal(out.numpy().view(np.uint64), expect)
    # gated: zones from each table's keys (every present key lies inside its zone)
    for f in range(nf):
        s.zone_from_keys(f, workload.key_range(600 + f, kpf))
    out.zero_()
    s.probe(gpu.KeyBatch(n=n, key_len=16, keys=keys), out=out, gated=True)
    dev = s.probe(look, gated=True)
    assert np.array_equal(out.numpy().view(np.uint64), dev)
    # buffers from the C ABI's own pinned allocator (what the Rust shim uses)
    import ctypes
    from lsmt_amd import _lib
    L = _lib.load()
    kp, hp = ctypes.c_void_p(), ctypes.c_void_p()
    hbytes = nf * ((n + 63) // 64) * 8
    assert L.cb_host_alloc(look.nbytes, ctypes.byref(kp)) == 0
    assert L.cb_host_alloc(hbytes, ctypes.byref(hp)) == 0
    try:
        kh = np.ctypeslib.as_array((ctypes.c_uint8 * look.nbytes).from_address(kp.value)).reshape(n, 16)
        hh = np.ctypeslib.as_array((ctypes.c_uint64 * (hbytes // 8)).from_address(hp.value)).reshape(nf, -1)
        kh[:] = look
        s.probe(kh, out=hh)
        assert gpu.last_path() == 4
        assert np.array_equal(hh, expect)
    finally:
        assert L.cb_host_free(kp) == 0 and L.cb_host_free(hp) == 0


def test_filterset_assign_slots_and_var_keys(gpu):
    m = (1 << 20) + 17
    filters, refs = [], []
    for f in range(6):
        g, o = build_pair(gpu, m, workload.key_range(600 + f, 5000))
        filters.append(g)
        refs.append(o)
    s = gpu.FilterSet(m, width=32)
    for i in (0, 3, 1):  # sparse path: empty slots
        s.assign(i, filters[i])
    assert s.used == 4
    look = workload.probe_lookups(40_000, 6, 5000, seed_base=600, absent_seed=996)
    exp = oracle.probe_fixed([refs[0], refs[1], oracle.OracleFilter(m), refs[3]], look)
    assert np.array_equal(s.probe(look), exp)
    s.assign(3, filters[5])  # dense path: slot already holds bits
    s.clear_slot(1)
    exp = oracle.probe_fixed([refs[0], oracle.OracleFilter(m), oracle.OracleFilter(m), refs[5]], look)
    assert np.array_equal(s.probe(look), exp)
    rng = np.random.default_rng(11)
    data, offs = workload.var_keys(rng, 20_000, max_len=30)
    exp = oracle.probe_var([refs[0], oracle.OracleFilter(m), oracle.OracleFilter(m), refs[5]], data, offs)
    assert np.array_equal(s.probe(gpu.KeyBatch(n=20_000, data=data, offsets=offs)), exp)


def test_filterset_c3_golden(gpu, golden):
    g = golden["c3"]
    filters = []
    for f in range(g["nf"]):
        b = gpu.BloomFilter(g["m"])
        b.insert_batch(workload.c3_filter_keys(f, g["keys_per_filter"]))
        filters.append(b)
    s = gpu.FilterSet.from_filters(filters)
    look = workload.c3_lookups(g["n_lookups"], g["nf"], g["keys_per_filter"])
    assert sha(s.probe(look).astype("<u8")) == g["hits_sha256"]
    # incremental: the same set built slot by slot into empty slots
    s2 = gpu.FilterSet(g["m"])
    for i, b in enumerate(filters):
        s2.assign(i, b)
    assert sha(s2.probe(look).astype("<u8")) == g["hits_sha256"]


@pytest.mark.parametrize("nf0", [3, 37], ids=["w32", "w64"])
def test_filterset_updates_match_oracle(gpu, nf0):
    # every way a set's words change (the transpose build, the sparse OR into
    # an empty slot, the dense rewrite of a slot that holds bits, clear_slot)
    # leaves the probe equal to the oracle; m = 2^20 + 9: a ragged last group.
    # nf0 = 3 takes the 32-slot kernels, nf0 = 37 the 64-slot ones.
    m = (1 << 20) + 9
    nf = nf0 + 2
    fs, rs = [], []
    for f in range(nf):
        g, o = build_pair(gpu, m, workload.key_range(700 + f, 6000))
        fs.append(g)
        rs.append(o)
    look = workload.probe_lookups(30000, nf, 6000, seed_base=700, absent_seed=995)
    s = gpu.FilterSet.from_filters(fs[:nf0])  # the transpose
    assert s.width == (32 if nf0 <= 32 else 64)
    assert np.array_equal(s.probe(look), oracle.probe_fixed(rs[:nf0], look))
    s.assign(nf0, fs[nf0])  # the sparse OR into empty slots
    s.assign(nf0 + 1, fs[nf0 + 1])
    assert np.array_equal(s.probe(look), oracle.probe_fixed(rs, look))
    s.clear_slot(0)
    s.assign(1, fs[nf - 1])  # the dense rewrite
    exp = [oracle.OracleFilter(m), rs[nf - 1]] + rs[2:]
    assert np.array_equal(s.probe(look), oracle.probe_fixed(exp, look))


@pytest.mark.parametrize("m", [100003, 1 << 20, 1 << 25])
def test_insert_many_matches_oracle(gpu, path, m):
    # concurrent flush builds (C4 shape, scaled down): 40 filters, ragged counts
    counts = [0, 1, 5000] + [3000 + 97 * i for i in range(37)]
    keys = [workload.key_range(800 + i, c) for i, c in enumerate(counts)]
    fs = [gpu.BloomFilter(m) for _ in counts]
    fs[5].insert_batch(workload.key_range(5, 100))  # one filter already holds bits
    gpu.insert_many(fs, keys)
    for i, (f, k) in enumerate(zip(fs, keys)):
        o = oracle.OracleFilter(m)
        if i == 5:
            o.insert_fixed(workload.key_range(5, 100))
        o.insert_fixed(k)
        assert np.array_equal(f.bools(), o.bools()), i


