"""Hand-worked replies for the coordinator's read merge (cb_replies_fold) with
what the fold must make of them, worked out from the rule's text
(include/cassbloom.h; src/cluster.rs:394-473) and not from any implementation.

A case: name, replies (bytes, in order), text (the response; None: CB_EUTF8),
rows (the winners in key order as (key, ts, val, reply, flags)), counts
(lines, entries, others) and, for CB_EUTF8, bad = (reply, offset in the
joined replies). LINES holds single pieces for cb_reply_line.
"""
T, D, H = 1, 2, 4  # CB_FOLD_TEXT, CB_FOLD_DEAD, CB_FOLD_HOST
U64 = 18446744073709551615


def case(name, replies, text, rows=(), counts=None, bad=None, other=None):
    return dict(name=name, replies=list(replies), text=text, rows=list(rows), counts=counts, bad=bad, other=other)


def ts_case(name, ts_text, ts):
    """One entry whose timestamp text is ts_text against an entry of ts 1 for
    the same key behind it: the first wins unless it parsed to 0."""
    first = b"k\t" + ts_text + b"\t{\"a\":\"1\"}\n"
    rows = [(b"k", ts, b'{"a":"1"}', 0, T)] if ts >= 1 else [(b"k", 1, b'{"b":"2"}', 1, T)]
    return case("ts " + name, [first, b"k\t1\t{\"b\":\"2\"}\n"], b"[" + rows[0][2] + b"]", rows, (2, 2, 0))


CASES = [
    # ---- ts ----
    ts_case("plain", b"5", 5),
    ts_case("max", b"18446744073709551615", U64),
    ts_case("max + 1", b"18446744073709551616", 0),
    ts_case("20 nines", b"99999999999999999999", 0),
    ts_case("plus", b"+5", 5),
    ts_case("minus", b"-5", 0),
    ts_case("plus alone", b"+", 0),
    ts_case("two plus", b"++5", 0),
    ts_case("empty", b"", 0),
    ts_case("25 leading zeros", b"0" * 25 + b"7", 7),
    ts_case("30 zeros", b"0" * 30, 0),
    ts_case("space before", b" 5", 0),
    ts_case("space behind", b"5 ", 0),
    ts_case("arabic-indic five", "٥".encode(), 0),
    ts_case("hex", b"0x10", 0),
    ts_case("float", b"5.0", 0),
    ts_case("plus max", b"+18446744073709551615", U64),
    # ---- \r ----
    case("crlf is stripped", [b"k\t1\t{}\r\n"], b"[{}]", [(b"k", 1, b"{}", 0, T)], (1, 1, 0)),
    case("an unterminated last line keeps its cr", [b"k\t1\t{}\r"], b"[]", [(b"k", 1, b"{}\r", 0, H)], (1, 1, 0)),
    case("a lone crlf is no line", [b"\r\n"], b"[]", [], (0, 0, 0)),
    case("a lone cr at the end is an other", [b"\r"], b"\r", [], (1, 0, 1), other=(0, 1)),
    case("only one cr goes", [b"k\t1\t{}\r\r\n"], b"[]", [(b"k", 1, b"{}\r", 0, H)], (1, 1, 0)),
    case("crlf dead row", [b"k\t1\t\r\n"], b"[]", [(b"k", 1, b"", 0, D)], (1, 1, 0)),
    case("cr inside", [b"k\t1\t{}\rx\n"], b"[]", [(b"k", 1, b"{}\rx", 0, H)], (1, 1, 0)),
    # ---- reply edges ----
    case("two unterminated replies stay two lines", [b"a\t1\t{}", b"b\t1\t{}"], b"[{},{}]",
         [(b"a", 1, b"{}", 0, T), (b"b", 1, b"{}", 1, T)], (2, 2, 0)),
    case("joined they would be one entry", [b"a\t1", b"\t{}"], b"\t{}", [], (2, 0, 2), other=(3, 3)),
    case("an unterminated cr before the next reply", [b"a\t1\t{}\r", b"\nb\t2\t{}\n"], b"[{}]",
         [(b"a", 1, b"{}\r", 0, H), (b"b", 2, b"{}", 1, T)], (2, 2, 0)),
    case("empty replies around", [b"", b"a\t1\t{}\n", b"", b"", b"b\t1\t{}", b""], b"[{},{}]",
         [(b"a", 1, b"{}", 1, T), (b"b", 1, b"{}", 4, T)], (2, 2, 0)),
    case("one reply", [b"b\t1\t{}\na\t2\t{\"x\":\"y\"}\n"], b'[{"x":"y"},{}]',
         [(b"a", 2, b'{"x":"y"}', 0, T), (b"b", 1, b"{}", 0, T)], (2, 2, 0)),
    case("sixteen replies", [b"k%02d\t%d\t{\"r\":\"%d\"}\n" % (i % 4, i, i) for i in range(16)],
         b'[{"r":"12"},{"r":"13"},{"r":"14"},{"r":"15"}]',
         [(b"k%02d" % j, 12 + j, b'{"r":"%d"}' % (12 + j), 12 + j, T) for j in range(4)], (16, 16, 0)),
    case("no reply", [], b"[]", [], (0, 0, 0)),
    case("empty replies only", [b"", b""], b"[]", [], (0, 0, 0)),
    case("newlines only", [b"\n\n", b"\n"], b"[]", [], (0, 0, 0)),
    # ---- entry cuts ----
    case("an empty key", [b"\t3\t{}\n"], b"[{}]", [(b"", 3, b"{}", 0, T)], (1, 1, 0)),
    case("a val with further tabs", [b"k\t3\t{}\t\tx\n"], b"[]", [(b"k", 3, b"{}\t\tx", 0, H)], (1, 1, 0)),
    case("one tab is an other", [b"k\t3\n"], b"k\t3", [], (1, 0, 1), other=(0, 3)),
    case("others are ignored once an entry exists", [b"count\t3\n", b"zz\nk\t1\t{}\nnote\n"], b"[{}]",
         [(b"k", 1, b"{}", 1, T)], (4, 1, 3)),
    case("an empty key and an empty ts and an empty val", [b"\t\t\n"], b"[]", [(b"", 0, b"", 0, D)], (1, 1, 0)),
    # ---- ties and order ----
    case("equal timestamps across replies: the first", [b"k\t5\t{\"a\":\"0\"}\n", b"k\t5\t{\"a\":\"1\"}\n"],
         b'[{"a":"0"}]', [(b"k", 5, b'{"a":"0"}', 0, T)], (2, 2, 0)),
    case("equal timestamps within a reply: the first", [b"k\t5\t{\"a\":\"0\"}\nk\t5\t{\"a\":\"1\"}\n"],
         b'[{"a":"0"}]', [(b"k", 5, b'{"a":"0"}', 0, T)], (2, 2, 0)),
    case("a later greater one wins", [b"k\t5\t{\"a\":\"0\"}\n", b"x\t1\t{}\nk\t6\t{\"a\":\"1\"}\n"],
         b'[{"a":"1"},{}]', [(b"k", 6, b'{"a":"1"}', 1, T), (b"x", 1, b"{}", 1, T)], (3, 3, 0)),
    case("a bad ts against a real 0: the first", [b"k\tzz\t{\"a\":\"0\"}\n", b"k\t0\t{\"a\":\"1\"}\n"],
         b'[{"a":"0"}]', [(b"k", 0, b'{"a":"0"}', 0, T)], (2, 2, 0)),
    case("a real 0 against a bad ts: the first", [b"k\t0\t{\"a\":\"1\"}\n", b"k\tzz\t{\"a\":\"0\"}\n"],
         b'[{"a":"1"}]', [(b"k", 0, b'{"a":"1"}', 0, T)], (2, 2, 0)),
    case("a dead winner over a live loser", [b"k\t5\t{\"a\":\"0\"}\n", b"k\t9\t\n"], b"[]",
         [(b"k", 9, b"", 1, D)], (2, 2, 0)),
    case("a live winner over a dead loser", [b"k\t9\t{\"a\":\"0\"}\n", b"k\t5\t\n"], b'[{"a":"0"}]',
         [(b"k", 9, b'{"a":"0"}', 0, T)], (2, 2, 0)),
    case("keys ascend bytewise", [b"b\t1\t{}\n\xc3\xa9\t1\t{}\nB\t1\t{}\nab\t1\t{}\na\t1\t{}\n"], b"[{},{},{},{},{}]",
         [(k, 1, b"{}", 0, T) for k in (b"B", b"a", b"ab", b"b", b"\xc3\xa9")], (5, 5, 0)),
    # ---- canonical edges ----
    case("names equal", [b'k\t1\t{"a":"1","a":"2"}\n'], b"[]", [(b"k", 1, b'{"a":"1","a":"2"}', 0, H)], (1, 1, 0)),
    case("names descending", [b'k\t1\t{"b":"1","a":"2"}\n'], b"[]", [(b"k", 1, b'{"b":"1","a":"2"}', 0, H)], (1, 1, 0)),
    case("names ascending", [b'k\t1\t{"a":"1","ab":"","b":"2"}\n'], b'[{"a":"1","ab":"","b":"2"}]',
         [(b"k", 1, b'{"a":"1","ab":"","b":"2"}', 0, T)], (1, 1, 0)),
    case("names ascend as unescaped", [b'k\t1\t{"\\n":"1","!":"2"}\n'], b'[{"\\n":"1","!":"2"}]',
         [(b"k", 1, b'{"\\n":"1","!":"2"}', 0, T)], (1, 1, 0)),
    case("names descend as unescaped", [b'k\t1\t{"!":"2","\\n":"1"}\n'], b"[]",
         [(b"k", 1, b'{"!":"2","\\n":"1"}', 0, H)], (1, 1, 0)),
    case("a space after the colon", [b'k\t1\t{"a": "1"}\n'], b"[]", [(b"k", 1, b'{"a": "1"}', 0, H)], (1, 1, 0)),
    case("a space before the end", [b'k\t1\t{"a":"1"} \n'], b"[]", [(b"k", 1, b'{"a":"1"} ', 0, H)], (1, 1, 0)),
    case("an escaped solidus", [b'k\t1\t{"a":"\\/"}\n'], b"[]", [(b"k", 1, b'{"a":"\\/"}', 0, H)], (1, 1, 0)),
    case("a raw solidus", [b'k\t1\t{"a":"/"}\n'], b'[{"a":"/"}]', [(b"k", 1, b'{"a":"/"}', 0, T)], (1, 1, 0)),
    case("u0041", [b'k\t1\t{"a":"\\u0041"}\n'], b"[]", [(b"k", 1, b'{"a":"\\u0041"}', 0, H)], (1, 1, 0)),
    case("u001F upper", [b'k\t1\t{"a":"\\u001F"}\n'], b"[]", [(b"k", 1, b'{"a":"\\u001F"}', 0, H)], (1, 1, 0)),
    case("u001f lower", [b'k\t1\t{"a":"\\u001f"}\n'], b'[{"a":"\\u001f"}]',
         [(b"k", 1, b'{"a":"\\u001f"}', 0, T)], (1, 1, 0)),
    case("u000a has a short form", [b'k\t1\t{"a":"\\u000a"}\n'], b"[]", [(b"k", 1, b'{"a":"\\u000a"}', 0, H)],
         (1, 1, 0)),
    case("the short escapes", [b'k\t1\t{"a":"\\"\\\\\\b\\f\\n\\r\\t\\u0000"}\n'],
         b'[{"a":"\\"\\\\\\b\\f\\n\\r\\t\\u0000"}]', [(b"k", 1, b'{"a":"\\"\\\\\\b\\f\\n\\r\\t\\u0000"}', 0, T)],
         (1, 1, 0)),
    case("a raw 0x7f and non-ascii", ['k\t1\t{"a":"\x7fé€😀"}\n'.encode()], '[{"a":"\x7fé€😀"}]'.encode(),
         [(b"k", 1, '{"a":"\x7fé€😀"}'.encode(), 0, T)], (1, 1, 0)),
    case("a raw control byte", [b'k\t1\t{"a":"\x01"}\n'], b"[]", [(b"k", 1, b'{"a":"\x01"}', 0, H)], (1, 1, 0)),
    case("a number value", [b'k\t1\t{"a":1}\n'], b"[]", [(b"k", 1, b'{"a":1}', 0, H)], (1, 1, 0)),
    case("a nested object", [b'k\t1\t{"a":{}}\n'], b"[]", [(b"k", 1, b'{"a":{}}', 0, H)], (1, 1, 0)),
    case("an array", [b"k\t1\t[]\n"], b"[]", [(b"k", 1, b"[]", 0, H)], (1, 1, 0)),
    case("truncated json", [b'k\t1\t{"a":"1\n'], b"[]", [(b"k", 1, b'{"a":"1', 0, H)], (1, 1, 0)),
    case("a brace inside the last string", [b'k\t1\t{"a":"}\n'], b"[]", [(b"k", 1, b'{"a":"}', 0, H)], (1, 1, 0)),
    case("a trailing comma", [b'k\t1\t{"a":"1",}\n'], b"[]", [(b"k", 1, b'{"a":"1",}', 0, H)], (1, 1, 0)),
    case("a lone surrogate escape", [b'k\t1\t{"a":"\\ud800"}\n'], b"[]", [(b"k", 1, b'{"a":"\\ud800"}', 0, H)],
         (1, 1, 0)),
    case("a backslash at the end", [b'k\t1\t{"a":"\\\n'], b"[]", [(b"k", 1, b'{"a":"\\', 0, H)], (1, 1, 0)),
    case("one brace", [b"k\t1\t{\n"], b"[]", [(b"k", 1, b"{", 0, H)], (1, 1, 0)),
    case("host rows stay out of the text", [b'a\t1\t{"x":"1"}\nb\t1\t{"x":1}\nc\t1\t{}\nd\t1\t\n'], b'[{"x":"1"},{}]',
         [(b"a", 1, b'{"x":"1"}', 0, T), (b"b", 1, b'{"x":1}', 0, H), (b"c", 1, b"{}", 0, T), (b"d", 1, b"", 0, D)],
         (4, 4, 0)),
    # ---- the three responses ----
    case("the least other wins", [b"5\n", b"12\n", b"3\n"], b"12", [], (3, 0, 3), other=(2, 2)),
    case("a prefix sorts before its extension", [b"ab\nabc\n", b"a\nab"], b"a", [], (4, 0, 4), other=(7, 1)),
    case("of equal others the first", [b"7\n", b"7\n"], b"7", [], (2, 0, 2), other=(0, 1)),
    case("a crlf other", [b"9\r\n", b"10\r\n"], b"10", [], (2, 0, 2), other=(3, 2)),
    case("nothing at all", [b"", b"\n", b"\r\n"], b"[]", [], (0, 0, 0)),
    # ---- UTF-8 ----
    case("a bad byte in reply 0's key", [b"a\t1\t{}\n\xff\t1\t{}\n", b"b\t1\t{}\n"], None, bad=(0, 7)),
    case("a bad byte in reply 2's val", [b"a\t1\t{}\n", b"", b"b\t1\t{}\nc\t1\t{\"a\":\"\xc3\"}\n"], None, bad=(2, 14)),
    case("a bad byte in an other line", [b"a\t1\t{}\n", b"x\xed\xa0\x80\n"], None, bad=(1, 7)),
    case("bad bytes in two replies: the first in order", [b"ok\n", b"\xc0\x80\n", b"\xff\n"], None, bad=(1, 3)),
    case("a bad ts text", [b"a\t\x80\t{}\n"], None, bad=(0, 0)),
    case("a truncated sequence at a reply's end", [b"a\t1\t{}\n\xe2\x82", b"\xac\n"], None, bad=(0, 7)),
]

# (piece, terminated) -> (kind, key_len, ts, val_at, val_len, val_flags)
LINES = [
    ((b"", True), (0, 0, 0, 0, 0, 0)),
    ((b"\r", True), (0, 0, 0, 0, 0, 0)),
    ((b"\r", False), (2, 0, 0, 0, 0, 0)),
    ((b"k\t1\t{}\r", True), (1, 1, 1, 4, 2, T)),
    ((b"k\t1\t{}\r", False), (1, 1, 1, 4, 3, H)),
    ((b"k\t1\t\r", True), (1, 1, 1, 4, 0, D)),
    ((b"key\t+42\tv\tw", True), (1, 3, 42, 8, 3, H)),
    ((b"\t\t", True), (1, 0, 0, 2, 0, D)),
    ((b"k\t1", True), (2, 0, 0, 0, 0, 0)),
    ((b"k\t\r", True), (2, 0, 0, 0, 0, 0)),
    ((b"\xffk\t1\t{}", True), (-7, 0, 0, 0, 0, 0)),
    ((b"k\t18446744073709551615\t{}", True), (1, 1, U64, 23, 2, T)),
    ((b"k\t18446744073709551616\t{}", True), (1, 1, 0, 23, 2, T)),
]
