"""lsmt_amd — MI355X-native Bloom-filter path for the `cass` LSM store
(mweiden/lsmt, /root/reference/src/bloom.rs).

The HIP extension (lsmt_amd/libcassbloom.so, C ABI in include/cassbloom.h) is
loaded at import; there is no CPU fallback. The ctypes binding is split by
subject (DESIGN.md has the module map); every public name is exported here.
"""
from . import _lib

_lib.load()  # fail loudly if the gfx950 extension is not built

from ._ffi import DeviceKeys, KeyBatch  # noqa: E402
from .bloom import (BloomFilter, BloomProto, device_count, insert_many, last_path, probe, set_path,  # noqa: E402
                    unpack_hits)
from .exchange import hits_compress, hits_expand, hits_expand_set  # noqa: E402
from .filterset import FilterSet, probe_tiers, set_dense  # noqa: E402
from .get import get_many, get_many_tiers  # noqa: E402
from .rows import RowsResult, row_matches, row_select, select_rows  # noqa: E402
from .scan import (ScanResult, count, count_lww, count_where, prefix_end, scan, scan_live, scan_lww,  # noqa: E402
                   scan_many)
from .table import Table, compact, compact_live, compact_lww, sstable_create  # noqa: E402
from .wal import LogStats, log_line, replay_log, wal_bytes  # noqa: E402
from .zone import TableMeta, ZoneMap, zone_bounds  # noqa: E402

__all__ = [
    # key batches
    "DeviceKeys", "KeyBatch",
    # one filter
    "BloomFilter", "BloomProto", "device_count", "insert_many", "last_path", "probe", "set_path", "unpack_hits",
    # zone maps and .meta files
    "TableMeta", "ZoneMap", "zone_bounds",
    # filter sets and tiers
    "FilterSet", "probe_tiers", "set_dense",
    # tables, flush and compaction
    "Table", "compact", "compact_live", "compact_lww", "sstable_create",
    # the write-ahead log
    "LogStats", "log_line", "replay_log", "wal_bytes",
    # rows: WHERE and SELECT
    "RowsResult", "row_matches", "row_select", "select_rows",
    # scans and counts
    "ScanResult", "count", "count_lww", "count_where", "prefix_end", "scan", "scan_live", "scan_lww", "scan_many",
    # the read path
    "get_many", "get_many_tiers",
    # the multi-GPU hit exchange
    "hits_compress", "hits_expand", "hits_expand_set",
]
__version__ = "0.1.0"
