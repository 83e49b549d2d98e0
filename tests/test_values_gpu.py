"""Value bytes end to end: what SsTable::get decodes and SsTable::create
encodes must be bit-exact (src/sstable.rs:57-72, 133-153), at the sizes where
the hand-written branches change.

Read path (b64decode.hip): k_b64_decode's one-wait path (1..18 bytes) and its
8-chars-per-step loop, each into the 16 KiB LDS stage or, when a block's 256
values exceed it, into direct byte stores; b64_len's verdict on values that
STANDARD.decode rejects (Database::get then falls through to an older table);
the key buckets' 12-bit limits. Flush (flush.hip): k_format's word and byte
paths, its 16 KiB and 32 KiB stages and the direct stores past them.

The reference is the C oracle throughout, and every comparison is exact. The
one CPU test pins the oracle's decoder to Python on the corpus the GPU tests
use, and checks that the block plans land on the limits they are built for.
"""
import base64
import binascii
import functools

import numpy as np
import pytest

from oracle import oracle

ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
BAD_CHARS = b"=-_ \t\r\x00\x80\xff"  # each outside the STANDARD alphabet
DECODE_STAGE = 16384              # b64decode.hip kDecodeLds
FORMAT_STAGES = (16384, 32768)    # flush.hip kFormatLdsSmall / kFormatLdsLarge
TILE = 256                        # lookups / lines per block
INLINE_TILES = 64                 # flush.hpp kFormatInlineTiles
SMALL_B64 = 18                    # b64decode.hip kSmallB64Bytes


def rand_bytes(rng, n) -> bytes:
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def all_byte_values(rng) -> bytes:
    return rng.permutation(256).astype(np.uint8).tobytes()


def ragged(items):
    offs = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(x) for x in items], out=offs[1:])
    data = np.frombuffer(b"".join(items), np.uint8).copy() if offs[-1] else np.zeros(1, np.uint8)
    return data, offs


def canonical(s: bytes):
    """What base64 0.21.7's STANDARD.decode accepts: strict alphabet,
    canonical padding, zero trailing bits (as tests/test_oracle.py)."""
    try:
        d = base64.b64decode(s, validate=True)
    except (binascii.Error, ValueError):
        return None
    return d if base64.b64encode(d) == s else None


def line_len(kl: int, vl: int) -> int:
    return kl + 2 + 4 * ((vl + 2) // 3)


# ---- A. the corpus and the plans ---------------------------------------------------

CORPUS_LENGTHS = list(range(41)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 300]


@functools.lru_cache(maxsize=None)
def invalid_corpus():
    """Valid encodings and their mutations. Returns (strings, info): strings
    in a fixed order without repeats, info[s] = (mutated, j, kind) for the
    first way s was made: j the replaced position or -1, kind one of 'orig',
    'cut', 'bad' (a char outside the alphabet at j), 'alpha' (another
    alphabet char at j), 'trail' (the last body char replaced)."""
    rng = np.random.default_rng(1470)
    encs = []
    for n in CORPUS_LENGTHS:
        v = all_byte_values(rng) if n == 256 else rand_bytes(rng, n)
        encs.append(base64.b64encode(v))
    info = {}

    def add(s, j, kind):
        info.setdefault(bytes(s), (j, kind))

    for e in encs:
        add(e, -1, "orig")
    for e, n in zip(encs, CORPUS_LENGTHS):
        for s in (e[:-1], e + b"=", e + b"A", e + b"====", e.rstrip(b"=")):
            add(s, -1, "cut")
        for j in range(len(e)):
            for c in BAD_CHARS:
                add(e[:j] + bytes([c]) + e[j + 1:], j, "bad")
            add(e[:j] + bytes([ALPHABET[rng.integers(0, 64)]]) + e[j + 1:], j, "alpha")
        if n % 3:
            j = len(e.rstrip(b"=")) - 1
            for c in ALPHABET:
                add(e[:j] + bytes([c]) + e[j + 1:], j, "trail")
    origs = set(encs)
    strings = list(info)
    return strings, {s: (s not in origs, j, kind) for s, (j, kind) in info.items()}


def corpus_counts():
    strings, info = invalid_corpus()
    ok = [canonical(s) is not None for s in strings]
    rejected = len(ok) - sum(ok)
    mutated_ok = sum(1 for s, o in zip(strings, ok) if o and info[s][0])
    return sum(ok), rejected, mutated_ok


def decode_plan(small: bool):
    """B2: value lengths per lookup (-1: an absent key), 256 lookups per
    decode block. Block totals run 16383 (staged), 16385 (direct), 16384
    (staged) three times, each round behind a block of one odd-sized value, so
    the bases of the staged blocks fall on 1, 2 and 3 mod 4; a short last
    block ends the batch. small: every value is at most 18 bytes (the one-wait
    path) but one filler per block that carries the total to the limit; else
    every value is at least 19 bytes (the 8-char loop)."""
    rng = np.random.default_rng(1471 + small)
    lens = []
    for _ in range(3):
        odd = [-1] * TILE
        odd[int(rng.integers(0, TILE))] = 5 if small else 21  # 1 mod 4
        lens += odd
        for target in (DECODE_STAGE - 1, DECODE_STAGE + 1, DECODE_STAGE):
            if small:
                blk = [int(x) for x in rng.integers(0, SMALL_B64 + 1, TILE)]
                f = int(rng.integers(0, TILE))
                blk[f] = 0
                blk[f] = target - sum(blk)
            else:
                blk = [19 + int(x) for x in rng.multinomial(target - 19 * TILE, [1.0 / TILE] * TILE)]
            lens += blk
    lens += [int(x) for x in (rng.integers(0, SMALL_B64 + 1, 100) if small else rng.integers(19, 60, 100))]
    return lens


def block_totals(lens):
    return [sum(max(x, 0) for x in lens[i:i + TILE]) for i in range(0, len(lens), TILE)]


def format_plan(stage: int, many_tiles: bool):
    """C2: (key length, value length) per line of a sorted batch, 256 lines per
    k_format block. For each base & 3 in 0..3 and each of the two limits
    (total + (base & 3) == stage: staged; stage + 1: direct) one heavy block,
    each behind a light block whose one longer key moves the base. The 16 KiB
    plan is light on average (empty values, 8-byte lines) with heavy blocks of
    ~64-byte lines; the 32 KiB plan's lines average past 51 bytes. many_tiles
    pads to more than 64 tiles (the k_tile_scan launch) and ends in a short
    block; else the batch stays at 64 tiles or fewer (the inline scan)."""
    rng = np.random.default_rng(1480 + stage // 16384 + 2 * many_tiles)
    light_vl = 0 if stage == FORMAT_STAGES[0] else 60
    vmax = 80 if stage == FORMAT_STAGES[0] else 176
    lines, base = [], 0
    for edge in (0, 1):
        for want in range(4):
            light = [[6, light_vl] for _ in range(TILE)]
            light[int(rng.integers(0, TILE))][0] += (want - base - sum(line_len(*x) for x in light)) % 4
            lines += light
            base += sum(line_len(*x) for x in light)
            assert base % 4 == want
            target = stage + edge - want
            while True:
                blk = [[6, int(v)] for v in rng.integers(0, vmax + 1, TILE)]
                d = target - sum(line_len(*x) for x in blk)
                if 0 <= d <= 20 * TILE:
                    break
            for x in blk:  # the deficit as key bytes: keys of 6..26 bytes
                add = min(d, 20)
                x[0] += add
                d -= add
            rng.shuffle(blk)
            lines += blk
            base += target
    tiles = INLINE_TILES + 3 if many_tiles else len(lines) // TILE + 2
    lines += [[6, light_vl] for _ in range(tiles * TILE - len(lines) - (TILE - 100 if many_tiles else 0))]
    return [tuple(x) for x in lines]


def format_blocks(lines):
    """(base & 3, total) of each 256-line block."""
    out, base = [], 0
    for i in range(0, len(lines), TILE):
        tot = sum(line_len(kl, vl) for kl, vl in lines[i:i + TILE])
        out.append((base & 3, tot))
        base += tot
    return out


def format_stage(lines):
    """The stage launch_format picks: cap_bytes / n * 256 * 5 / 4 against 16 KiB
    (tablehost.hpp flush_file_bound: K + 2n + (4V + 8n) / 3 + 17)."""
    n = len(lines)
    K, V = sum(kl for kl, _ in lines), sum(vl for _, vl in lines)
    cap = K + 2 * n + (4 * V + 8 * n) // 3 + 17
    return FORMAT_STAGES[0] if cap // n * 320 <= FORMAT_STAGES[0] else FORMAT_STAGES[1]


def test_corpus_and_plans():
    """Oracle decoder == Python's canonical decode on the whole corpus
    (35 746 strings, 3 596 accepted of which 3 545 mutated, 32 150 rejected;
    no disagreement when written); the corpus holds what B3 needs; the B2
    and C2 plans land on the limits they name."""
    strings, info = invalid_corpus()
    assert len(strings) == len(set(strings))
    n_ok, n_rej, n_mut_ok = corpus_counts()
    print(f"corpus: {len(strings)} strings, {n_ok} accepted ({n_mut_ok} mutated), {n_rej} rejected")
    for s in strings:
        assert oracle.b64_decode(s) == canonical(s), s
    assert n_rej >= 1000 and n_mut_ok >= 500
    # a rejected char at every offset of an 8-char step of b64_len, in a first,
    # a middle and a last step (of the body: the chars before the padding)
    seen = set()
    trail = {1: [0, 0], 2: [0, 0]}  # pad -> [accepted, rejected]
    for s in strings:
        _, j, kind = info[s]
        pad = (2 if s[-2:] == b"==" else 1) if s[-1:] == b"=" else 0
        body = len(s) - pad
        if kind == "bad" and len(s) % 4 == 0 and j < body and canonical(s) is None:
            steps = (body + 7) // 8
            if steps >= 3:
                where = "first" if j < 8 else "last" if j // 8 == steps - 1 else "middle"
                seen.add((where, j % 8))
        if kind == "trail" and len(s) > 40:  # past one 8-char step
            trail[pad][canonical(s) is None] += 1
    assert seen >= {(w, o) for w in ("first", "middle") for o in range(8)}
    # (a last step holds 8 body chars only without padding: offsets 0..5 under
    # "==", 0..6 under "=", all 8 for lengths divisible by 3)
    assert {o for w, o in seen if w == "last"} == set(range(8))
    assert all(a > 0 and r > 0 for a, r in trail.values()), trail

    for small in (False, True):
        lens = decode_plan(small)
        tot = block_totals(lens)
        edge = [DECODE_STAGE - 1, DECODE_STAGE + 1, DECODE_STAGE]
        assert tot[:-1] == 3 * ([5 if small else 21] + edge) and len(lens) % TILE == 100
        bases = np.concatenate([[0], np.cumsum(tot)])[:-1]
        for t in (DECODE_STAGE - 1, DECODE_STAGE):  # the staged blocks: off a dword at 1, 2 and 3
            assert {int(b) & 3 for b, x in zip(bases, tot) if x == t} >= {1, 2, 3}
        found = [x for x in lens if x >= 0]
        if small:
            assert sum(x > SMALL_B64 for x in found) == 9 and 0 in found and SMALL_B64 in found
        else:
            assert min(found) >= SMALL_B64 + 1

    for stage in FORMAT_STAGES:
        for many in (False, True):
            lines = format_plan(stage, many)
            assert format_stage(lines) == stage
            blocks = format_blocks(lines)
            assert (len(blocks) > INLINE_TILES) == many
            at = {(sh, tot + sh - stage) for sh, tot in blocks if tot + sh >= stage}
            assert at == {(sh, e) for sh in range(4) for e in (0, 1)}, (stage, many)
            # every other block is far inside the stage
            assert all(tot + sh < stage * 3 // 4 for sh, tot in blocks if tot + sh < stage)
            assert any(kl > 16 and vl > 16 for kl, vl in lines) and any(kl <= 16 and vl <= 16 for kl, vl in lines)
    # C1's two batches under sorted input: the full one writes directly, the
    # one of values up to 100 bytes is staged (32 KiB stage for both)
    for vmax, direct in ((200, True), (100, False)):
        ents = sorted(c1_entries(vmax))
        lines = [(len(k), len(v)) for k, v in ents]
        assert format_stage(lines) == FORMAT_STAGES[1]
        full = format_blocks(lines)[:-1]
        assert all((tot + sh > FORMAT_STAGES[1]) == direct for sh, tot in full)


# ---- B. read path -------------------------------------------------------------------

def table_file(keys, encs, final_newline=True) -> bytes:
    data = b"".join(k + b"\t" + e + b"\n" for k, e in zip(keys, encs))
    return data if final_newline else data[:-1]


def check_get(gpu, tables, otables, look, hits=None, **kw):
    """get_many == the oracle's walk: which, val_off and the value bytes."""
    d, o = ragged(look)
    ow, ovoff, ovals = oracle.get_many(otables, hits, d, o)
    which, voff, vals = gpu.get_many(tables, gpu.KeyBatch(n=len(look), data=d, offsets=o), **kw)
    assert np.array_equal(which, ow)
    assert np.array_equal(voff, ovoff)
    assert vals == ovals
    return ow, ovoff, ovals


@functools.lru_cache(maxsize=None)
def b1_table():
    """Values of every length 0..200 whose encoded chars start at every
    address mod 16: line i holds a value of i % 201 bytes and a key of 5..20
    bytes chosen so that the value's first char sits at (i // 201) mod 16."""
    rng = np.random.default_rng(1472)
    keys, vals, off = [], [], 0
    for i in range(201 * 16):
        kl = 5 + (i // 201 - off - 6) % 16
        keys.append(b"%05d" % i + bytes(rng.integers(97, 123, kl - 5, dtype=np.uint8)))
        vals.append(all_byte_values(rng)[:i % 201] if i % 7 else rand_bytes(rng, i % 201))
        assert (off + kl + 1) % 16 == i // 201
        off += line_len(kl, len(vals[-1]))
    assert len(set(b"".join(vals))) == 256
    return keys, vals, table_file(keys, [base64.b64encode(v) for v in vals])


def b1_lookups(rng, keys, n_absent):
    absent = [k[:5] + b"~" for k in keys[:n_absent:2]] + [rand_bytes(rng, rng.integers(0, 20))
                                                          for _ in range(n_absent // 2)]
    look = list(keys) + absent
    return [look[i] for i in rng.permutation(len(look))]


@pytest.mark.gpu
def test_read_every_length_and_alignment(gpu):
    """B1, one table: the two-step form without hits and the fused form
    (filterset=). Blocks of 256 shuffled lookups of 0..200-byte values decode
    to ~25 KB: the direct branch of the RAW decode, small and long lanes
    mixed."""
    keys, vals, data = b1_table()
    rng = np.random.default_rng(1473)
    look = b1_lookups(rng, keys, 600)
    t, ot = gpu.Table(data), oracle.OracleTable(data)
    ow, ovoff, ovals = check_get(gpu, [t], [ot], look)
    pos = {k: i for i, k in enumerate(keys)}
    for j, k in enumerate(look):  # and against the values themselves
        want = vals[pos[k]] if k in pos else b""
        assert ovals[ovoff[j]:ovoff[j + 1]] == want and (ow[j] == 0) == (k in pos)
    # staged blocks of the same table: runs of 256 lookups of short values
    short = [k for k, v in zip(keys, vals) if len(v) <= 60]
    check_get(gpu, [t], [ot], [short[i] for i in rng.permutation(len(short))])
    b = gpu.BloomFilter(1 << 16)
    d, o = ragged(keys)
    b.insert_batch(gpu.KeyBatch(n=len(keys), data=d, offsets=o))
    s = gpu.FilterSet(1 << 16)
    s.assign(0, b)
    d, o = ragged(look)
    hits = s.probe(gpu.KeyBatch(n=len(look), data=d, offsets=o), gated=True)[:1].copy()
    check_get(gpu, [t], [ot], look, hits=hits, filterset=s)


@pytest.mark.gpu
def test_read_wide_set_values_past_slot_64(gpu):
    """B1 through a wide set (128 slots, 66 tables, newest first): 64 small
    tables in slots 0..63; slot 64 holds every fifth B1 key with an
    undecodable value (the walk falls through), every seventh with a value of
    4096..5000 bytes and one of 70 000; slot 65 is the B1 table."""
    keys, vals, data = b1_table()
    rng = np.random.default_rng(1474)
    strings, _ = invalid_corpus()
    bad = [s for s in strings if canonical(s) is None]
    files, keysets = [], []
    for t in range(64):
        ks = sorted({keys[i] for i in rng.integers(0, len(keys), 12) if i != 7} | {b"t%02d-%d" % (t, j) for j in range(5)})
        files.append(table_file(ks, [base64.b64encode(rand_bytes(rng, rng.integers(0, 90))) for _ in ks]))
        keysets.append(ks)
    k64, e64 = [], []
    for i, k in enumerate(keys):
        if i % 5 == 0:
            k64.append(k)
            e64.append(bad[int(rng.integers(0, len(bad)))])
        elif i % 7 == 0:
            k64.append(k)
            e64.append(base64.b64encode(rand_bytes(rng, 70_000 if i == 7 else rng.integers(4096, 5001))))
    files += [table_file(k64, e64), data]
    keysets += [k64, keys]
    tables = [gpu.Table(f) for f in files]
    otables = [oracle.OracleTable(f) for f in files]
    s = gpu.FilterSet(1 << 14, width=128)
    for slot, ks in enumerate(keysets):
        b = gpu.BloomFilter(1 << 14)
        d, o = ragged(ks)
        b.insert_batch(gpu.KeyBatch(n=len(ks), data=d, offsets=o))
        s.assign(slot, b)
    assert s.used == 66
    look = b1_lookups(rng, keys, 600) + [b"t07-3", b"t63-0"]
    d, o = ragged(look)
    hits = s.probe(gpu.KeyBatch(n=len(look), data=d, offsets=o), gated=True)[:66].copy()
    ow, ovoff, ovals = check_get(gpu, tables, otables, look, hits=hits, filterset=s)
    fell = {k for i, k in enumerate(keys) if i % 5 == 0}
    assert (ow == 64).sum() > 200 and (ow == 65).sum() > 1500 and ((ow >= 0) & (ow < 64)).sum() > 300
    assert sum(1 for k, w in zip(look, ow) if k in fell and w == 65) > 400
    assert max(np.diff(ovoff.astype(np.int64))) == 70_000


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["loop19plus", "small18"])
def test_read_decode_stage_limit(gpu, small):
    """B2: decode blocks of exactly 16383, 16385 and 16384 bytes (staged,
    direct, staged; decode_plan), host outputs and device outputs at +0..+3
    bytes with guard bytes around them."""
    import torch
    lens = decode_plan(small)
    rng = np.random.default_rng(1475 + small)
    look, keys, vals = [], [], []
    for i, n in enumerate(lens):
        if n < 0:
            look.append(b"k%06d-absent" % i)
        else:
            keys.append(b"k%06d" % i)
            vals.append(all_byte_values(rng)[:n] if i % 3 == 0 and n <= 256 else rand_bytes(rng, n))
            look.append(keys[-1])
    assert len(set(b"".join(vals))) == 256
    data = table_file(keys, [base64.b64encode(v) for v in vals])
    t, ot = gpu.Table(data), oracle.OracleTable(data)
    ow, ovoff, ovals = check_get(gpu, [t], [ot], look)
    assert ovals == b"".join(vals)
    n, total = len(look), len(ovals)
    d, o = ragged(look)
    kb = gpu.KeyBatch(n=n, data=d, offsets=o)
    for shift in range(4):
        which = torch.empty(n, dtype=torch.int32, device="cuda")
        voff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        guard = torch.from_numpy(np.frombuffer(rand_bytes(rng, total + 64), np.uint8).copy()).cuda()
        before = guard.cpu().numpy().copy()
        out = guard[16 + shift:16 + shift + total]
        assert out.data_ptr() % 4 == shift
        _, _, tot = gpu.get_many([t], kb, out=(which, voff, out))
        got = guard.cpu().numpy()
        assert tot == total
        assert got[16 + shift:16 + shift + total].tobytes() == ovals, shift
        assert np.array_equal(got[:16 + shift], before[:16 + shift]), shift
        assert np.array_equal(got[16 + shift + total:], before[16 + shift + total:]), shift
        assert np.array_equal(which.cpu().numpy(), ow)
        assert np.array_equal(voff.cpu().numpy().view(np.uint64), ovoff)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["indexed", "force_exact"])
def test_read_rejected_values_fall_through(gpu, exact):
    """B3: the newer table holds one line per corpus string (keys of 1..24
    bytes: the chars at every alignment), the older a valid value for every
    key. A value STANDARD.decode rejects is Err in the newer table, so
    Database::get answers from the older one (src/lib.rs:128-134)."""
    strings, _ = invalid_corpus()
    n_ok, n_rej, _ = corpus_counts()
    rng = np.random.default_rng(1476)
    keys = set()
    while len(keys) < len(strings):
        keys.add(bytes(rng.integers(97, 123, rng.integers(1, 25), dtype=np.uint8)))
    keys = sorted(keys)
    order = rng.permutation(len(strings))
    newer = table_file(keys, [strings[i] for i in order])
    older = table_file(keys, [base64.b64encode(rand_bytes(rng, rng.integers(0, 31))) for _ in keys])
    gpu.Table.force_exact(exact)
    try:
        t0 = gpu.Table(newer)
    finally:
        gpu.Table.force_exact(False)
    assert t0.well_formed != exact
    tables = [t0, gpu.Table(older)]
    otables = [oracle.OracleTable(newer), oracle.OracleTable(older)]
    absent = [k + b"-" for k in keys[::50]]
    look = keys + absent
    look = [look[i] for i in rng.permutation(len(look))]
    ow, ovoff, ovals = check_get(gpu, tables, otables, look)
    assert (ow == 0).sum() == n_ok and (ow == 1).sum() == n_rej and (ow < 0).sum() == len(absent)
    want = {k: canonical(strings[i]) for k, i in zip(keys, order)}
    for j, k in enumerate(look):
        if ow[j] == 0:
            assert ovals[ovoff[j]:ovoff[j + 1]] == want[k]
        elif ow[j] == 1:
            assert want[k] is None


@functools.lru_cache(maxsize=None)
def b4_file():
    rng = np.random.default_rng(1477)
    ents = {b"a%04d" % i: rand_bytes(rng, rng.integers(0, 50)) for i in range(700)}
    for i, vl in enumerate((4094, 4095, 4096, 5000, 70_000)):  # the buckets keep decoded lengths <= 4095
        ents[b"b%04d" % i] = all_byte_values(rng) + rand_bytes(rng, vl - 256)
    for kl in (4094, 4095, 4096):  # and keys shorter than 4095
        ents[b"m" + bytes(rng.integers(97, 123, kl - 1, dtype=np.uint8))] = rand_bytes(rng, 30 + kl % 7)
    ents[b"zz-last"] = rand_bytes(rng, 70_000)
    keys = sorted(ents)
    assert keys[-1] == b"zz-last"
    return keys, ents, table_file(keys, [base64.b64encode(ents[k]) for k in keys], final_newline=False)


@pytest.mark.gpu
def test_read_large_values_and_bucket_limits(gpu):
    """B4: values of 4094..70 000 bytes and keys of 4094..4096 bytes (both
    sides of what the key buckets hold), the file ending in a 70 000-byte
    value without a final newline: the call that builds the buckets, a second
    call, and a table read with no buckets at all."""
    keys, ents, data = b4_file()
    rng = np.random.default_rng(1478)
    longk = [k for k in keys if len(k) > 4000]
    assert sorted(len(k) for k in longk) == [4094, 4095, 4096]
    near = [k[:-1] for k in longk] + [k + b"a" for k in longk] + [k[:-1] + b"{" for k in longk]
    look = keys + near + [b"a9999", b"", b"zz-last\x00", b"zz-las"]
    look = [look[i] for i in rng.permutation(len(look))]
    ot = oracle.OracleTable(data)
    assert ot.nlines == len(keys)
    t = gpu.Table(data)
    for _ in range(2):
        ow, ovoff, ovals = check_get(gpu, [t], [ot], look)
    for j, k in enumerate(look):
        assert ovals[ovoff[j]:ovoff[j + 1]] == ents.get(k, b"") and (ow[j] == 0) == (k in ents)
    try:
        gpu.Table.bucket_limit(0)
        check_get(gpu, [gpu.Table(data)], [ot], look)
    finally:
        gpu.Table.bucket_limit(1 << 30)


@pytest.mark.gpu
def test_read_scanned_decode_direct(gpu):
    """B5: 262 145 lookups (one past the RAW decode's limit: k_tile_scan, then
    k_b64_decode<false>) of 0..200-byte values, ~25 KB a block: the scanned
    decode's direct branch. The whole output against the oracle."""
    keys, vals, data = b1_table()
    rng = np.random.default_rng(1479)
    pick = rng.integers(0, len(keys) + 200, 262_145)
    look = [keys[i] if i < len(keys) else b"absent-%d" % i for i in pick]
    check_get(gpu, [gpu.Table(data)], [oracle.OracleTable(data)], look)


# ---- C. flush -----------------------------------------------------------------------

def check_flush(gpu, entries, batches=None):
    """The created file == the oracle's, and every value reads back."""
    t, _, _ = gpu.sstable_create(batches if batches is not None else entries)
    want = oracle.sstable_create(entries)
    got = t.data()
    assert len(got) == len(want)
    assert got == want
    d, o = ragged([k for k, _ in entries])
    which, voff, vals = gpu.get_many([t], gpu.KeyBatch(n=len(entries), data=d, offsets=o))
    assert (which == 0).all()
    _, vo = ragged([v for _, v in entries])
    assert np.array_equal(voff, vo)
    assert vals == b"".join(v for _, v in entries)
    return t


@functools.lru_cache(maxsize=None)
def c1_entries(vmax=200):
    """Distinct keys of 0..40 bytes (no TAB or newline) against values of
    0..200 bytes: entry i pairs i % 41 with i % 201 (coprime: every pair once;
    the empty key once). In input order, which is not key order."""
    rng = np.random.default_rng(1481)
    kbytes = np.array([b for b in range(256) if b not in (9, 10)], np.uint8)
    seen, ents = set(), []
    for i in range(41 * 201):
        kl, vl = i % 41, i % 201
        if kl == 0 and i:
            continue
        k = kbytes[rng.integers(0, len(kbytes), kl)].tobytes()
        while k in seen:
            k = kbytes[rng.integers(0, len(kbytes), kl)].tobytes()
        seen.add(k)
        v = all_byte_values(rng)[:vl] if i % 5 == 0 else rand_bytes(rng, vl)
        if vl <= vmax:
            ents.append((k, v))
    return tuple(ents)


@pytest.mark.gpu
@pytest.mark.parametrize("sorted_input", [True, False], ids=["sorted", "unsorted"])
def test_flush_byte_path_combinations(gpu, sorted_input):
    """C1: keys of 0..40 bytes against values of 0..200 bytes: the word path
    and the byte path's four key/value combinations, lane by lane in one
    block. The full batch writes directly (~40 KB a block), the one of values
    up to 100 bytes through the 32 KiB stage."""
    for vmax in (200, 100):
        ents = list(c1_entries(vmax))
        if sorted_input:
            ents.sort()
        combos = {(len(k) <= 16, len(v) <= 16) for k, v in ents}
        assert len(combos) == 4 and len(set(b"".join(v for _, v in ents))) == 256
        t = check_flush(gpu, ents)
        assert t.well_formed


def plan_entries(lines, seed):
    rng = np.random.default_rng(seed)
    ents = []
    for i, (kl, vl) in enumerate(lines):
        k = b"%06d" % i + bytes(rng.integers(97, 123, kl - 6, dtype=np.uint8))
        ents.append((k, all_byte_values(rng)[:vl] if i % 4 == 0 else rand_bytes(rng, vl)))
    return ents


@pytest.mark.gpu
@pytest.mark.parametrize("many_tiles", [False, True], ids=["inline_scan", "tile_scan"])
@pytest.mark.parametrize("stage", FORMAT_STAGES)
def test_flush_stage_limits(gpu, stage, many_tiles):
    """C2: sorted batches whose blocks sit at total + (base & 3) == stage
    (staged) and stage + 1 (direct) for every base & 3 (format_plan), for the
    16 KiB stage (a batch light on average with heavy blocks) and the 32 KiB
    one, with the tile sums scanned inline and by k_tile_scan."""
    ents = plan_entries(format_plan(stage, many_tiles), stage + many_tiles)
    assert ents == sorted(ents)
    t = check_flush(gpu, ents)
    assert t.well_formed and t.nlines == len(ents)


@functools.lru_cache(maxsize=None)
def c3_entries():
    rng = np.random.default_rng(1482)
    ents = [(b"%016x" % int(rng.integers(0, 1 << 62)), rand_bytes(rng, rng.integers(0, 41))) for _ in range(5000)]
    for i, vl in zip((11, 1500, 2600, 4999), (4095, 4096, 70_000, 1 << 20)):
        ents[i] = (ents[i][0], all_byte_values(rng) + rand_bytes(rng, vl - 256))
    assert len({k for k, _ in ents}) == len(ents)
    return tuple(ents)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("sorted_input", [True, False], ids=["sorted", "unsorted"])
def test_flush_large_values(gpu, sorted_input, on_device):
    """C3: values of 4095, 4096, 70 000 bytes and 1 MiB among 5000 short ones
    (direct stores in their blocks, the 32 KiB stage elsewhere), from host and
    from HBM inputs; unsorted input takes the value spans from the bin sort."""
    import torch
    ents = list(c3_entries())
    if sorted_input:
        ents.sort()
    batches = None
    if on_device:
        kd, ko = ragged([k for k, _ in ents])
        vd, vo = ragged([v for _, v in ents])
        dev = [torch.from_numpy(x).cuda() for x in (kd, ko.view(np.int64), vd, vo.view(np.int64))]
        batches = (gpu.KeyBatch(n=len(ents), data=dev[0], offsets=dev[1]),
                   gpu.KeyBatch(n=len(ents), data=dev[2], offsets=dev[3]))
    check_flush(gpu, ents, batches)
