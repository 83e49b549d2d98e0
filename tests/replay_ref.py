"""A plain restatement of the log replay (cb_log_replay, logline.hpp) over the
C oracle's verdicts: Wal::new's parse_entries (src/wal.rs:14-31), one
memtable.insert per record in log order (src/lib.rs:35-39), then the flush of
that memtable (SsTable::create, src/sstable.rs:51-87).

The split rules are written out here; whether a key is UTF-8 and whether a
text is STANDARD base64 are oracle.utf8_valid's and oracle.b64_decode's
answers (the oracle is read, not changed). A plain module: no test, no
fixture, nothing collected.
"""
from oracle import oracle

SKIPPED, ENTRY, EUTF8, EBASE64 = 0, 1, -7, -8
NONE = 2 ** 64 - 1  # UINT64_MAX: no bad piece


def pieces(log: bytes):
    """[(offset, piece)] of the non-empty pieces of log.split(b'\\n'); the last
    piece counts without a final newline."""
    out, at = [], 0
    for piece in bytes(log).split(b"\n"):
        if piece:
            out.append((at, piece))
        at += len(piece) + 1
    return out


def line(piece: bytes):
    """(kind, key, value) of one piece: SKIPPED without a TAB, whatever its
    bytes; else the key is checked first, then the text; key and value are None
    unless the piece is an ENTRY."""
    tab = piece.find(b"\t")
    if tab < 0:
        return SKIPPED, None, None
    key, text = piece[:tab], piece[tab + 1:]
    if not oracle.utf8_valid(key):
        return EUTF8, None, None
    value = oracle.b64_decode(text)
    if value is None:
        return EBASE64, None, None
    return ENTRY, key, value


def line_verdict(piece: bytes):
    """(kind, key_len, value_len) as cb_log_line answers."""
    kind, key, value = line(piece)
    return (kind, len(key), len(value)) if kind == ENTRY else (kind, 0, 0)


class Replay:
    """What a replay of `log` gives: code 0 with the dict (log order, last write
    stands), the file and the stats, or the error's code with the first bad
    piece; stats = (lines, entries, keys, bad_line, bad_offset)."""

    def __init__(self, log: bytes):
        ps = pieces(log)
        self.code, self.rows, self.file = 0, {}, None
        lines, entries, bad = len(ps), 0, None
        for i, (at, piece) in enumerate(ps):
            kind, key, value = line(piece)
            entries += kind != SKIPPED
            if kind < 0 and bad is None:
                bad = (kind, i, at)
            if kind == ENTRY and bad is None:
                self.rows.pop(key, None)  # (a dict in log order: the key moves to its last write)
                self.rows[key] = value
        if bad is not None:
            self.code, self.rows = bad[0], None
            self.stats = (lines, entries, 0, bad[1], bad[2])
            return
        self.keys = sorted(self.rows)
        self.items = [(k, self.rows[k]) for k in self.keys]
        self.file = oracle.sstable_create(self.items) if self.items else b""
        self.stats = (lines, entries, len(self.keys), NONE, NONE)

    @property
    def bounds(self):
        return (self.keys[0], self.keys[-1]) if self.keys else None
