"""What the GPU tests of the device merge share (compaction, scans, counts,
live rows, LWW, WHERE, the table makers): hand-written data files, their keys
and value texts, and the tile size their edges sit on. A plain module: no
test, no fixture, nothing collected."""
import base64

import numpy as np

TILE = 256  # compact.hpp kCompactTile = scan.hip kNT = sstable.hpp kDecodeTile
BAD = b"QQ="  # a text STANDARD.decode rejects
ALL = [(b"", None)]  # everything, as one unbounded range


def ragged(items):
    offs = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(x) for x in items], out=offs[1:])
    data = np.frombuffer(b"".join(items), np.uint8).copy() if offs[-1] else np.zeros(1, np.uint8)
    return data, offs


def b64(v: bytes) -> bytes:
    return base64.b64encode(v)


def raw_file(lines, final_newline=True) -> bytes:
    """A hand-written data file: lines = [(key, value text)] in file order."""
    body = b"\n".join(k + b"\t" + t for k, t in lines)
    return body + (b"\n" if final_newline and lines else b"")


def file_keys(data: bytes):
    """The keys of a file's lines, as SsTable::get splits it (src/sstable.rs:142-146)."""
    return [ln.split(b"\t", 1)[0] for ln in data.split(b"\n") if ln]


def absent_keys(keys, rng, n=64):
    have = set(keys)
    out = [k + b"!" for k in keys[:n]] + [k[:-1] for k in keys[:n] if k] + [b"", b"\xff" * 9]
    out += [rng.integers(0, 256, int(rng.integers(1, 24)), dtype=np.uint8).tobytes().replace(b"\n", b"n").replace(b"\t", b"t")
            for _ in range(n)]
    return [k for k in dict.fromkeys(out) if k not in have]


def named(t, k):
    return b"t%d:" % t + k


def hex_keys(rng, n, kl=16):
    h = rng.integers(0, 256, (n, kl // 2), dtype=np.uint8).tobytes().hex().encode()
    return list(dict.fromkeys(h[i * kl:(i + 1) * kl] for i in range(n)))


def oracle_prefix_end(p: bytes):
    """The least byte string above every string that starts with p, worked out
    here (not by the library): the first key k > p, in a brute-force sense,
    that does not start with p is p's last non-0xFF byte incremented."""
    q = p.rstrip(b"\xff")
    return q[:-1] + bytes([q[-1] + 1]) if q else None


def tomb(ts: int) -> bytes:
    """exec_delete's value text: the 8-byte timestamp, no payload (src/query.rs:240-261)."""
    return b64(ts.to_bytes(8, "big"))


def row(ts: int, payload: bytes) -> bytes:
    """A live row's value text: timestamp, then the payload."""
    return b64(ts.to_bytes(8, "big") + payload)


def open_tables(gpu, files):
    return [gpu.Table(f) for f in files]


def table_lines(gpu, t):
    """cb_table_lines: (start, key_len, line_len) of every line."""
    n = t.nlines
    start, kl, ll = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    gpu._lib.check(gpu._lib.load().cb_table_lines(t._h, start.ctypes.data, kl.ctypes.data, ll.ctypes.data))
    return start[:n].tolist(), kl[:n].tolist(), ll[:n].tolist()
