"""A plain Python restatement of the coordinator's read merge (the tail of
Cluster::execute for a read, src/cluster.rs:394-473), independent of
lsmt_amd/csrc/replyline.hpp: dicts, sorted keys and Python's own string
methods. It states Rust's and serde_json's documented behaviour; it was not
run against the reference.

fold(replies) -> Fold: stats (a dict named as cb_fold_stats), rows (the
winners in key order as places in b"".join(replies)), text (the response) and
other ((at, len) of the least other line where it is the response).
"""
import json
import re

ENTRY, OTHER, IGNORED, BAD_UTF8 = 1, 2, 0, -7
TEXT, DEAD, HOST = 1, 2, 4
NONE = 0xFFFFFFFFFFFFFFFF

_TS = re.compile(rb"\+?[0-9]+\Z")
# a string as serde_json writes one: the bytes that need an escape never stand raw, the short
# escapes only for the bytes that have one, \u00xx in lower-case hex for the other controls
_STR = rb'"(?:[^"\\\x00-\x1f]|\\["\\bfnrt]|\\u00(?:0[0-7b]|0[ef]|1[0-9a-f]))*"'
_OBJ = re.compile(rb"\{(?:%s:%s(?:,%s:%s)*)?\}\Z" % (_STR, _STR, _STR, _STR))
_NAME = re.compile(rb"(?:\{|,)(%s):%s" % (_STR, _STR))


def lines_of(reply: bytes):
    """str::lines() of one reply as (start, bytes, terminated) per piece that
    is not empty before the strip; the strip itself is line_of's."""
    out, i = [], 0
    while i < len(reply):
        e = reply.find(b"\n", i)
        end, term = (e, True) if e >= 0 else (len(reply), False)
        if end > i:
            out.append((i, reply[i:end], term))
        i = end + 1
    return out


def parse_ts(text: bytes) -> int:
    if not _TS.match(text):
        return 0
    v = int(text)
    return v if v < 1 << 64 else 0


def val_flags(val: bytes) -> int:
    """DEAD, TEXT (serde_json's parse and re-serialisation is the identity) or
    HOST (anything else that is not empty)."""
    if not val:
        return DEAD
    if not _OBJ.match(val):
        return HOST
    # the names as strings, in document order: strictly ascending by their UTF-8 bytes
    names = [json.loads(m.group(1).decode()).encode() for m in _NAME.finditer(val)]
    return TEXT if all(a < b for a, b in zip(names, names[1:])) else HOST


def line_of(piece: bytes, terminated: bool):
    """(kind, key_len, ts, val_at, val_len, val_flags) of one piece."""
    try:
        piece.decode("utf-8")
    except UnicodeDecodeError:
        return (BAD_UTF8, 0, 0, 0, 0, 0)
    line = piece[:-1] if terminated and piece.endswith(b"\r") else piece
    if not line:
        return (IGNORED, 0, 0, 0, 0, 0)
    cut = line.split(b"\t", 2)
    if len(cut) < 3:
        return (OTHER, 0, 0, 0, 0, 0)
    key, ts, val = cut
    return (ENTRY, len(key), parse_ts(ts), len(key) + len(ts) + 2, len(val), val_flags(val))


class Fold:
    def __init__(self):
        self.stats = dict(replies=0, lines=0, entries=0, others=0, keys=0, with_text=0, dead=0, host_rows=0, bytes=0,
                          bad_reply=NONE, bad_offset=NONE)
        self.rows, self.text, self.other, self.code = [], b"[]", None, 0


def fold(replies) -> Fold:
    f = Fold()
    f.stats["replies"] = len(replies)
    best, others, base = {}, [], 0
    for r, reply in enumerate(replies):
        for at, piece, term in lines_of(reply):
            kind, klen, ts, val_at, val_len, flags = line_of(piece, term)
            if kind == BAD_UTF8:
                f.stats.update(lines=0, entries=0, others=0, bad_reply=r, bad_offset=base + at)
                f.code, f.text = BAD_UTF8, None
                return f
            if kind == IGNORED:
                continue
            f.stats["lines"] += 1
            if kind == OTHER:
                line = piece[:-1] if term and piece.endswith(b"\r") else piece
                others.append((line, base + at))
                continue
            f.stats["entries"] += 1
            key = piece[:klen]
            row = (base + at, klen, ts, base + at + val_at, val_len, r, flags)
            if key not in best or ts > best[key][2]:  # (of equal timestamps the first met stays)
                best[key] = row
        base += len(reply)
    f.stats["others"] = len(others)
    joined = b"".join(replies)
    if not best:
        if others:
            line, at = min(others)  # (bytewise; of equal lines the first met)
            f.text, f.other = line, (at, len(line))
        f.stats["bytes"] = len(f.text)
        return f
    f.rows = [best[k] for k in sorted(best)]
    texts = [joined[r[3]:r[3] + r[4]] for r in f.rows if r[6] == TEXT]
    f.text = b"[" + b",".join(texts) + b"]"
    f.stats.update(keys=len(f.rows), with_text=len(texts), dead=sum(r[6] == DEAD for r in f.rows),
                   host_rows=sum(r[6] == HOST for r in f.rows), bytes=len(f.text))
    return f
