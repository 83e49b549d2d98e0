"""Every object that owns a C handle closes twice without error and leaves a
fresh null handle object; get_many notices a closed table by that. Nothing
here calls into the library with a closed handle."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = (7).to_bytes(8, "big")


def test_close_twice_and_drop_for_every_handle_owner(gpu):
    bloom = gpu.BloomFilter(64)
    fset = gpu.FilterSet(64, 32)
    fset.assign(0, bloom)
    table = gpu.Table(gpu.wal_bytes([(b"a", TS + b'{"c":"1"}'), (b"b", TS + b'{"c":"2"}')]))
    result = gpu.scan([table])
    assert result.keys() == [b"a", b"b"]
    rows = result.select(["c"])
    assert rows.text() == b'[{"c":"1"},{"c":"2"}]'
    owners = [rows, result, table, fset, bloom]
    while owners:
        x = owners.pop(0)
        live = x._h
        assert live.value
        x.close()
        null = x._h
        assert null is not live and null.value is None
        x.close()
        assert x._h is null
        del x
        gc.collect()


def test_get_many_takes_a_fresh_handle_array_after_a_table_closes(gpu):
    first = gpu.Table(gpu.wal_bytes([(b"a", b"1")]))
    second = gpu.Table(gpu.wal_bytes([(b"a", b"2"), (b"b", b"3")]))
    tables = [first, second]
    which, off, vals = gpu.get_many(tables, [b"a", b"b"])
    assert which.tolist() == [0, 1] and vals == b"13"
    first.close()
    tables[0] = gpu.Table(gpu.wal_bytes([(b"b", b"4")]))  # the same list, the closed table's slot refilled
    which, off, vals = gpu.get_many(tables, [b"a", b"b"])
    assert which.tolist() == [1, 0] and vals == b"24" and np.array_equal(off, [0, 1, 2])
    tables[0].close()
    del tables[0]  # the same list again, now holding the open table alone
    which, off, vals = gpu.get_many(tables, [b"a", b"b"])
    assert which.tolist() == [0, 0] and vals == b"23"
