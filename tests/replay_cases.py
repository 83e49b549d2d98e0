"""Hand-worked logs for the replay (cb_log_replay, cb_log_line): each with the
file a replay plus flush writes, or the error and the first bad piece, written
out literally. Worked from src/wal.rs:14-31, src/lib.rs:35-39 and
src/sstable.rs:51-87 by hand: "dg==" is base64 of b"v", "eA==" of b"x",
"eQ==" of b"y", "MQ==" / "Mg==" / "Mw==" of b"1" / b"2" / b"3", "YWI=" of b"ab",
"YWJj" of b"abc", "AAAAAAAAAAA=" of eight zero bytes (a tombstone: the timestamp
alone). A plain module: no test, no fixture, nothing collected.
"""
from collections import namedtuple

EUTF8, EBASE64 = -7, -8
NONE = 2 ** 64 - 1

# file: the expected table file (None for an error); code: 0 or the error;
# stats: (lines, entries, keys, bad_line, bad_offset)
Case = namedtuple("Case", "label log file code stats")


def ok(label, log, file, lines, entries, keys):
    return Case(label, log, file, 0, (lines, entries, keys, NONE, NONE))


def bad(label, log, code, lines, entries, bad_line, bad_offset):
    return Case(label, log, None, code, (lines, entries, 0, bad_line, bad_offset))


K17A, K17B = b"0123456789abcdefX", b"0123456789abcdefY"  # 17 bytes, the first 16 shared

CASES = [
    # ---- empty and degenerate logs
    ok("the empty log", b"", b"", 0, 0, 0),
    ok("only newlines", b"\n\n\n", b"", 0, 0, 0),
    ok("one record", b"k\tdg==\n", b"k\tdg==\n", 1, 1, 1),
    ok("one record without a final newline", b"k\tdg==", b"k\tdg==\n", 1, 1, 1),
    ok("an empty key", b"\tdg==\n", b"\tdg==\n", 1, 1, 1),
    ok("an empty text is the empty value", b"k\t\n", b"k\t\n", 1, 1, 1),
    ok("an empty key and an empty text", b"\t\n", b"\t\n", 1, 1, 1),
    ok("empty pieces between records", b"\n\nb\tMQ==\n\n\na\tMg==\n\n", b"a\tMg==\nb\tMQ==\n", 2, 2, 2),
    ok("\\r is a byte of the key", b"k\r\tdg==\nk\tdg==\n", b"k\tdg==\nk\r\tdg==\n", 2, 2, 2),
    # ---- skipped pieces
    ok("only TAB-less pieces", b"hello\nworld", b"", 2, 0, 0),
    ok("TAB-less pieces between records", b"junk\nb\tMQ==\nmore junk\na\tMg==\nend", b"a\tMg==\nb\tMQ==\n", 5, 2, 2),
    ok("a TAB-less piece that is not UTF-8 is skipped", b"\xff\xfe\xc0\nk\tdg==\n\xed\xa0\x80\n", b"k\tdg==\n", 3, 1, 1),
    ok("a TAB-less piece of bad base64 is skipped", b"@@\nk\tdg==\n", b"k\tdg==\n", 2, 1, 1),
    # ---- the last write stands; the file is sorted
    ok("sorted by key bytes", b"b\tMQ==\nc\tMg==\na\tMw==\n", b"a\tMw==\nb\tMQ==\nc\tMg==\n", 3, 3, 3),
    ok("the last write of a key stands", b"k\tMQ==\nk\tMg==\nk\tMw==\n", b"k\tMw==\n", 3, 3, 1),
    ok("the last write stands among others", b"a\tMQ==\nb\tMg==\na\tMw==\nc\teA==\nb\teQ==\n",
       b"a\tMw==\nb\teQ==\nc\teA==\n", 5, 5, 3),
    ok("a tombstone last stays as a line", b"k\tdg==\nk\tAAAAAAAAAAA=\n", b"k\tAAAAAAAAAAA=\n", 2, 2, 1),
    ok("a write after a tombstone stands", b"k\tAAAAAAAAAAA=\nk\tdg==\n", b"k\tdg==\n", 2, 2, 1),
    ok("the empty value last stands", b"k\tdg==\nk\t\n", b"k\t\n", 2, 2, 1),
    ok("texts of every padding", b"a\tYWI=\nb\tYWJj\nc\teA==\n", b"a\tYWI=\nb\tYWJj\nc\teA==\n", 3, 3, 3),
    # ---- keys the sort must tell apart
    ok("keys that share their first 16 bytes", K17B + b"\tMQ==\n" + K17A + b"\tMg==\n" + K17B + b"\tMw==\n",
       K17A + b"\tMg==\n" + K17B + b"\tMw==\n", 3, 3, 2),
    ok("a key that is a prefix of another", b"abc\tMQ==\nab\tMg==\nabcd\tMw==\na\teA==\n",
       b"a\teA==\nab\tMg==\nabc\tMQ==\nabcd\tMw==\n", 4, 4, 4),
    ok("keys compare as unsigned bytes", b"\xc3\xa9\tMQ==\nz\tMg==\nZ\tMw==\n", b"Z\tMw==\nz\tMg==\n\xc3\xa9\tMQ==\n", 3, 3, 3),
    # ---- errors: the reference's own, then each kind
    bad("the reference's own bad log", b"bad\t@@\n", EBASE64, 1, 1, 0, 0),
    bad("an overlong key", b"a\tMQ==\n\xc0\xaf\tMQ==\n", EUTF8, 2, 2, 1, 7),
    bad("a surrogate in the key", b"\xed\xa0\x80\tMQ==\n", EUTF8, 1, 1, 0, 0),
    bad("a key cut at the TAB", b"\n\nab\xe2\x82\tMQ==\n", EUTF8, 1, 1, 0, 2),
    bad("a byte above U+10FFFF", b"\xf4\x90\x80\x80\tMQ==", EUTF8, 1, 1, 0, 0),
    bad("a bad character", b"k\te@==\n", EBASE64, 1, 1, 0, 0),
    bad("bad padding: too short", b"k\teA=\n", EBASE64, 1, 1, 0, 0),
    bad("bad padding: '=' inside", b"k\te=A=\n", EBASE64, 1, 1, 0, 0),
    bad("bad padding: three '='", b"k\te===\n", EBASE64, 1, 1, 0, 0),
    bad("non-zero trailing bits, two '='", b"k\teB==\n", EBASE64, 1, 1, 0, 0),
    bad("non-zero trailing bits, one '='", b"k\tYWJ=\n", EBASE64, 1, 1, 0, 0),
    bad("length 1 mod 4", b"k\teA==Q\n", EBASE64, 1, 1, 0, 0),
    bad("no padding at all", b"k\teA\n", EBASE64, 1, 1, 0, 0),
    bad("a TAB in the text", b"k\tAAA\t\n", EBASE64, 1, 1, 0, 0),
    bad("a second record on the line", b"k\tMQ==\tMg==\n", EBASE64, 1, 1, 0, 0),
    bad("\\r before the newline is part of the text", b"k\tMQ==\r\n", EBASE64, 1, 1, 0, 0),
    bad("two bad pieces: the earlier wins (value, then key)", b"a\tMQ==\nskip\nb\t@@@@\n\xff\tMQ==\n", EBASE64, 4, 3, 2, 12),
    bad("two bad pieces: the earlier wins (key, then value)", b"a\tMQ==\n\xff\tMQ==\nb\t@@@@\n", EUTF8, 3, 3, 1, 7),
    bad("bad in both key and value: the key is checked first", b"\xff\t@@\n", EUTF8, 1, 1, 0, 0),
    bad("good records after the bad one do not help", b"k\t@\nk\tMQ==\n", EBASE64, 2, 2, 0, 0),
]

# (piece, kind, key_len, value_len): cb_log_line's answers
LINES = [
    (b"", 0, 0, 0),
    (b"no tab", 0, 0, 0),
    (b"\xff\xff", 0, 0, 0),
    (b"k\tdg==", 1, 1, 1),
    (b"\t", 1, 0, 0),
    (b"key\t", 1, 3, 0),
    (b"\tYWJj", 1, 0, 3),
    (b"k\tAAAAAAAAAAA=", 1, 1, 8),
    (b"\xc3\xa9\tYWI=", 1, 2, 2),
    (b"k\r\tdg==", 1, 2, 1),
    (b"bad\t@@", EBASE64, 0, 0),
    (b"k\tdg==\r", EBASE64, 0, 0),
    (b"k\tdg=\t", EBASE64, 0, 0),
    (b"\xc0\xaf\tdg==", EUTF8, 0, 0),
    (b"\xff\t@@", EUTF8, 0, 0),
]


# ---- generated logs for the device tests (their conditions are asserted on the CPU, tests/test_replay_cpu.py)

def record(key: bytes, value: bytes) -> bytes:
    """insert_internal's record with Wal::append's newline (src/lib.rs:96-102, src/wal.rs:63-72)."""
    import base64
    return key + b"\t" + base64.b64encode(value) + b"\n"


TOMBSTONE = b"\0" * 8
HOT = b"m-hot"  # sorts after the 100 keys "a..." and before the 100 keys "z..." of the hot-key logs


def stamped(i: int, payload: bytes) -> bytes:
    return i.to_bytes(8, "big") + payload


def hot_key_log(writes: int, others: int, last: bytes, seed: int) -> bytes:
    """`writes` records of HOT spread among 2 * others records of distinct keys,
    half sorting before HOT and half after; HOT's last value is `last`."""
    import random
    rng = random.Random(seed)
    recs = [(b"a%04d" % i, stamped(i, b"lo")) for i in range(others)] + [(b"z%04d" % i, stamped(i, b"hi")) for i in range(others)]
    recs += [(HOT, stamped(1000 + i, b"w%d" % i)) for i in range(writes - 1)]
    rng.shuffle(recs)
    recs.append((HOT, last))
    return b"".join(record(k, v) for k, v in recs)


def distinct_log(entries: int, repeats: int, seed: int) -> bytes:
    """`entries` records in random order: entries - repeats distinct 16-hex-digit
    keys, `repeats` of them (first written in the log's first half) written a
    second time somewhere in its second half."""
    import random
    rng = random.Random(seed)
    keys = [b"%016x" % rng.getrandbits(64) for _ in range(entries - repeats)]
    assert len(set(keys)) == len(keys)
    recs = [(k, stamped(i, b"first")) for i, k in enumerate(keys)]
    half = len(recs) // 2
    for i, (k, _) in enumerate(rng.sample(recs[:half], repeats)):
        recs.insert(rng.randrange(half, len(recs) + 1), (k, stamped(i, b"second")))
    return b"".join(record(k, v) for k, v in recs)


def mixed_log(lines: int, seed: int) -> bytes:
    """About `lines` non-empty pieces of every kind a good log holds: keys of 0 to
    40 bytes (long ones sharing their first 20), values of 0 to 60 bytes,
    tombstones, repeated keys, TAB-less pieces (some not UTF-8), empty pieces,
    and no final newline."""
    import random
    rng = random.Random(seed)
    pool = [b"%x" % rng.getrandbits(4 * rng.randrange(1, 17)) for _ in range(lines // 3)]
    pool += [b"shared-prefix-of-20b:" + b"%x" % rng.getrandbits(4 * rng.randrange(1, 20)) for _ in range(lines // 6)]
    pool += [b"", "é|ü".encode(), b"k\r", b" "]
    out = []
    for i in range(lines):
        r = rng.random()
        if r < 0.03:
            out.append(rng.choice([b"junk", b"\xff\xfe", b"@@@@", b"\xed\xa0\x80 not a key"]) + b"\n")
        elif r < 0.06:
            out.append(b"\n" * rng.randrange(1, 4))
            out.append(record(rng.choice(pool), stamped(i, b"after blanks")))
        elif r < 0.12:
            out.append(record(rng.choice(pool), TOMBSTONE))
        else:
            out.append(record(rng.choice(pool), rng.randbytes(rng.randrange(0, 61))))
    return b"".join(out)[:-1]


def generated():
    """{name: log} of the device tests' generated inputs."""
    return {
        "one key 300 times": hot_key_log(300, 100, stamped(9999, b"the last write"), 1),
        "one key 300 times, a tombstone last": hot_key_log(300, 100, TOMBSTONE, 2),
        "4096 entries": distinct_log(4096, 400, 3),
        "4097 entries": distinct_log(4097, 400, 4),
        "5000 entries, 4500 of one key": hot_key_log(4500, 250, stamped(9999, b"the last write"), 5),
        "9000 mixed lines": mixed_log(9000, 6),
    }
