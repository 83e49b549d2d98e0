"""The reference's last-write-wins read, restated for the tests (the library's
one statement of it is lsmt_amd/csrc/rowts.hpp).

The coordinator asks every replica for `key \\t ts \\t val` lines
(exec_select_schema with meta, src/query.rs:393-410), where ts is
split_ts(value).0 (src/query.rs:21-27), and folds them replica by replica
(src/cluster.rs:405-416):

    if let Some((cur_ts, _)) = merged.get(&key) { if *cur_ts >= ts { continue; } }
    merged.insert(key, (ts, val));

so the greatest timestamp wins and, among equal ones, the replica asked
first. Rows whose val is empty are dropped only after the fold
(src/cluster.rs:454-459). This module is that fold over per-table answers and
the drop afterwards; it uses liverow_ref.split_ts and nothing from the library.
"""
from liverow_ref import is_dead, split_ts


def ts_of(value: bytes) -> int:
    return split_ts(value)[0]


def fold(answers):
    """answers[r] = {key: decoded value}: replica r's answers (a key it cannot
    answer is not in the map). Returns {key: (ts, value, r)} of the winners."""
    merged = {}
    for r, rows in enumerate(answers):
        for key, val in rows.items():
            ts = ts_of(val)
            if key in merged and merged[key][0] >= ts:
                continue
            merged[key] = (ts, val, r)
    return merged


def winners(answers, drop_dead=False):
    """[(key, value, which, ts)] sorted by key: the fold, then (drop_dead) the
    post-fold drop of the rows without payload."""
    out = [(k, v, r, ts) for k, (ts, v, r) in sorted(fold(answers).items())]
    return [x for x in out if not is_dead(x[1])] if drop_dead else out
