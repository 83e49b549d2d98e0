"""lsmt_amd — MI355X-native Bloom-filter path for the `cass` LSM store
(mweiden/lsmt, /root/reference/src/bloom.rs).

The HIP extension (lsmt_amd/libcassbloom.so, C ABI in include/cassbloom.h) is
loaded at import; there is no CPU fallback.
"""
from . import _lib

_lib.load()  # fail loudly if the gfx950 extension is not built

from .bloom import (  # noqa: E402
    BloomFilter,
    BloomProto,
    DeviceKeys,
    FilterSet,
    KeyBatch,
    device_count,
    insert_many,
    last_path,
    probe,
    set_dense,
    set_path,
    unpack_hits,
    Table,
    TableMeta,
    get_many,
    get_many_tiers,
    probe_tiers,
    sstable_create,
    compact,
    replay_log,
    log_line,
    wal_bytes,
    LogStats,
    scan,
    scan_many,
    count,
    scan_live,
    compact_live,
    compact_lww,
    scan_lww,
    count_lww,
    count_where,
    row_matches,
    select_rows,
    row_select,
    RowsResult,
    prefix_end,
    ScanResult,
    zone_bounds,
    ZoneMap,
    hits_compress,
    hits_expand,
    hits_expand_set,
)

__all__ = ["BloomFilter", "BloomProto", "DeviceKeys", "FilterSet", "insert_many", "KeyBatch", "device_count", "last_path",
           "probe", "set_dense", "set_path", "unpack_hits", "zone_bounds", "ZoneMap", "TableMeta", "Table", "get_many", "sstable_create",
           "compact", "replay_log", "log_line", "wal_bytes", "LogStats", "scan", "scan_many", "count", "scan_live", "compact_live", "compact_lww", "scan_lww", "count_lww", "count_where", "row_matches", "select_rows", "row_select", "RowsResult", "prefix_end", "ScanResult", "probe_tiers", "get_many_tiers", "hits_compress", "hits_expand", "hits_expand_set"]
__version__ = "0.1.0"
