"""The reference's dead-row rule, restated for the tests (the library's one
statement of it is lsmt_amd/csrc/liverow.hpp).

exec_delete writes the 8-byte timestamp with an empty payload
(src/query.rs:240-261); every reader of a scan does
`let (_, data) = split_ts(&bytes); if data.is_empty() { continue; }`
(src/query.rs:343-346, 395-398). This module is split_ts (src/query.rs:21-27)
and that test, nothing else: tests/test_live_cpu.py holds the library's
predicate against it and tests/test_live_gpu.py filters the oracle's answers
with it.
"""


def split_ts(value: bytes):
    """src/query.rs:21-27: (timestamp, payload)."""
    if len(value) < 8:
        return 0, value
    return int.from_bytes(value[:8], "big"), value[8:]


def is_dead(value: bytes) -> bool:
    """The readers' `if data.is_empty() { continue; }`."""
    return len(split_ts(value)[1]) == 0


def payload_len(length: int) -> int:
    """len(split_ts(v)[1]) for any v of `length` bytes (split_ts looks at the
    length alone), for lengths too large to build."""
    return length if length < 8 else length - 8
