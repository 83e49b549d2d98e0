"""The three makers of a table in HBM produce the same table from the same
content: A = cb_sstable_create of the entries (sstable_enqueue, finalised on
first use), B = cb_table_create of A's file (index_table) and C =
cb_tables_compact of A alone. They share their steps (file and index
allocation, the sort plan, the directory, the index entry's writer), so
their files, line indexes, flags, zone bounds, filters and reads must agree
with each other, and every expectation comes from the C oracle
(oracle.sstable_create, OracleFilter, oracle.get_many over the oracle's file),
never from another maker; every comparison is exact.

Line counts: 1; 15 / 16 / 17 around the first table with a directory; 256 /
257 around the format and compaction tile; 4096 / 4097 around the sort plan's
switch from the merge sort to the bin sort. Key families: random 16-hex-digit
keys, and keys under one 8-byte prefix, which past 4096 lines leave the bin
sort one bin and so run its merge-sort fallback.
"""
import numpy as np
import pytest

from merge_help import absent_keys, ragged
from oracle import oracle

pytestmark = pytest.mark.gpu

CB_EINVAL = -1
NO_TAB = 0xFFFFFFFF  # sstable.hpp kNoSep: a line without a TAB
M = 1024


def make_entries(family, n, rng):
    if family == "hex":
        ids = np.unique(rng.integers(0, 1 << 63, 2 * n + 8, dtype=np.uint64))[:n]
        keys = [b"%016x" % int(i) for i in ids]
    else:  # one 8-byte prefix, different after it
        ids = np.unique(rng.integers(0, 1 << 40, 2 * n + 8, dtype=np.uint64))[:n]
        keys = [b"sameprfx%x" % int(i) for i in ids]
    assert len(set(keys)) == n
    entries = [(k, rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes()) for k in keys]
    return [entries[i] for i in rng.permutation(n)]  # shuffled: the create sorts


def split_file(data):
    """Starts, key lengths and line lengths of a file's non-empty lines, as
    SsTable::get splits it (src/sstable.rs:142-146): the key ends at the
    line's first TAB."""
    st, kl, ll, at = [], [], [], 0
    for ln in data.split(b"\n"):
        if ln:
            st.append(at)
            kl.append(ln.index(b"\t") if b"\t" in ln else NO_TAB)
            ll.append(len(ln))
        at += len(ln) + 1
    return np.array(st, np.uint64), np.array(kl, np.uint32), np.array(ll, np.uint32)


def check_makers(gpu, entries, well_formed, seed):
    """Makes A and B (and C when the content is well-formed), checks each
    against the oracle, and returns them."""
    want = oracle.sstable_create(entries)
    keys = [k for k, _ in entries]
    a, a_bloom, a_zone = gpu.sstable_create(entries, m=M)
    b = gpu.Table(a.data())
    made = [("create", a), ("index", b)]
    if well_formed:
        c, c_bloom, c_zone = gpu.compact([a], m=M)
        made.append(("compact", c))
    index = split_file(want)
    rng = np.random.default_rng(seed)
    look = keys + absent_keys(sorted(keys), rng)
    look = [look[i] for i in rng.permutation(len(look))]
    kd, ko = ragged(look)
    ow, ovoff, ovals = oracle.get_many([oracle.OracleTable(want)], None, kd, ko)
    assert (ow >= 0).sum() >= (len(keys) if well_formed else 1)
    for name, t in made:
        assert t.data() == want, f"{name}: the file differs from the oracle's"
        assert t.nlines == len(index[0]), name
        assert t.well_formed == well_formed, name
        for got, exp, what in zip(t.lines(), index, ("starts", "key lengths", "line lengths")):
            assert np.array_equal(got, exp), f"{name}: {what} differ from the oracle file's"
        which, voff, vals = gpu.get_many([t], look)
        assert np.array_equal(which >= 0, ow >= 0), f"{name}: found keys differ"
        assert np.array_equal(voff, ovoff) and vals == ovals, f"{name}: values differ"
    for (_, x), (_, y) in zip(made, made[1:]):
        for p, q in zip(x.lines(), y.lines()):
            assert np.array_equal(p, q)
    # SsTable::create's filter and zone bounds (src/sstable.rs:59-63)
    filt = oracle.OracleFilter(M)
    filt.insert_var(*ragged(keys))
    blooms, zones = [a_bloom], [a_zone]
    if well_formed:
        blooms.append(c_bloom)
        zones.append(c_zone)
    for bloom, zone in zip(blooms, zones):
        assert np.array_equal(bloom.bools(), filt.bools()), "filter bits differ from the oracle"
        assert (zone.min, zone.max) == (min(keys), max(keys))
    return [t for _, t in made]


@pytest.mark.parametrize("family", ["hex", "prefix"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 256, 257, 4096, 4097])
def test_makers_agree(gpu, n, family):
    rng = np.random.default_rng(1000 * n + len(family))
    made = check_makers(gpu, make_entries(family, n, rng), True, seed=n)
    assert [t.nlines for t in made] == [n, n, n]


def test_makers_agree_on_a_key_with_a_tab(gpu):
    """A key with '\\t' inside: the create re-indexes its file at finalisation
    (its own index is dropped and the file indexed as cb_table_create does).
    `dup\\tone` and `dup\\ttwo` both read as the key `dup`, so the file's keys
    are not strictly increasing: not well-formed, and compaction refuses it."""
    rng = np.random.default_rng(17)
    entries = make_entries("hex", 15, rng) + [(b"dup\tone", b"1"), (b"dup\ttwo", b"22")]
    assert len(entries) == 17
    entries = [entries[i] for i in rng.permutation(17)]
    a, b = check_makers(gpu, entries, False, seed=17)
    assert a.nlines == b.nlines == 17
    for tables in ([a], [b]):
        with pytest.raises(gpu._lib.CassBloomError) as ei:
            gpu.compact(tables)
        assert ei.value.code == CB_EINVAL
