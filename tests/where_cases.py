"""The known-answer rows of the WHERE rule (lsmt_amd/csrc/rowjson.hpp), shared
by tests/test_where_cpu.py (driver, cb_row_matches) and tests/test_where_gpu.py
(cb_scan_match, cb_tables_count_where). Every case carries the answer worked
out by hand from the rule's text; the tests also hold tests/rowjson_ref.py to it.

A case: (label, key, value, where, key_columns, skip, expect).
"""
from collections import namedtuple

Case = namedtuple("Case", "label key value where key_columns skip expect")

TS = (1_700_000_000_123_456).to_bytes(8, "big")
CV = [("c", "v")]
CASES = []


def add(label, payload, expect, where=CV, key=b"ns:k", key_columns=(), skip=3, raw=False):
    """payload follows the 8-byte timestamp unless raw (then it is the value)."""
    CASES.append(Case(label, key, payload if raw else TS + payload, list(where), tuple(key_columns), skip, expect))


def q(s: bytes) -> bytes:
    return b'{"c":"' + s + b'"}'


# ---- escapes ----
for esc, byte in [(b'\\"', b'"'), (b"\\\\", b"\\"), (b"\\/", b"/"), (b"\\b", b"\b"), (b"\\f", b"\f"), (b"\\n", b"\n"),
                  (b"\\r", b"\r"), (b"\\t", b"\t")]:
    add("escape %r in a value" % esc, q(b"a" + esc + b"z"), True, [("c", b"a" + byte + b"z")])
    add("escape %r in a name" % esc, b'{"' + esc + b'":"v"}', True, [(byte, "v")])
    add("escape %r is not its letter" % esc, q(esc), False, [("c", esc[1:])] if esc[1:] not in b'"\\/' else [("c", esc)])
add("an escaped slash equals a plain one", q(b"a\\/b"), True, [("c", "a/b")])
for bad in (b"\\a", b"\\N", b"\\0", b"\\x41", b"\\'", b"\\U0041", b"\\ "):
    add("unknown escape %r" % bad, q(bad), False, [("c", bad)])
    add("unknown escape %r in another pair" % bad, b'{"c":"v","d":"' + bad + b'"}', False)
add("\\u lower case", q(b"\\u00e9"), True, [("c", "\u00e9")])
add("\\u upper case", q(b"\\u00E9"), True, [("c", "\u00e9")])
add("\\u mixed case", q(b"\\u20aC"), True, [("c", "\u20ac")])
add("\\u ascii", q(b"\\u0041\\u007a"), True, [("c", "Az")])
add("\\u in a name", b'{"\\u0063":"v"}', True)
add("\\u two bytes edge", q(b"\\u0080\\u07ff"), True, [("c", "\u0080\u07ff")])
add("\\u three bytes edge", q(b"\\u0800\\uffff"), True, [("c", "\u0800\uffff")])
add("\\u three hex digits", q(b"\\u041"), False, [("c", "A")])
add("\\u bad hex digit", q(b"\\u00g9"), False, [("c", "\u00e9")])
add("\\u with a sign", q(b"\\u+041"), False, [("c", "A")])
add("\\u0000", q(b"a\\u0000b"), True, [("c", b"a\0b")])
add("\\u0000 is not the empty string", q(b"\\u0000"), False, [("c", b"")])
add("surrogate pair lower", q(b"\\ud83d\\ude00"), True, [("c", "\U0001F600")])
add("surrogate pair upper", q(b"\\uD83D\\uDE00"), True, [("c", "\U0001F600")])
add("surrogate pair lowest", q(b"\\ud800\\udc00"), True, [("c", "\U00010000")])
add("surrogate pair highest", q(b"\\udbff\\udfff"), True, [("c", "\U0010FFFF")])
add("lone high surrogate at the string's end", q(b"\\ud83d"), False, [("c", b"\xed\xa0\xbd")])
add("lone high surrogate before a letter", q(b"\\ud83dx"), False, [("c", b"\xed\xa0\xbdx")])
add("lone high surrogate before another escape", q(b"\\ud83d\\n"), False, [("c", b"\xed\xa0\xbd\n")])
add("high surrogate before a non-surrogate \\u", q(b"\\ud83d\\u0041"), False, [("c", b"\xed\xa0\xbdA")])
add("two high surrogates", q(b"\\ud83d\\ud83d"), False, [("c", b"\xed\xa0\xbd\xed\xa0\xbd")])
add("lone low surrogate", q(b"\\ude00"), False, [("c", b"\xed\xb8\x80")])
add("low before high", q(b"\\ude00\\ud83d"), False, [("c", "\U0001F600")])
add("a lone surrogate in another pair", b'{"c":"v","d":"\\udc00"}', False)
add("high surrogate cut off by the end of input", b'{"c":"\\ud83d', False, [("c", "")])
add("high surrogate then a cut-off escape", b'{"c":"\\ud83d\\ud', False, [("c", "")])

# ---- raw bytes ----
for b in range(0x20):
    add("raw control byte %02x" % b, q(b"a" + bytes([b]) + b"z"), False, [("c", b"a" + bytes([b]) + b"z")])
add("raw control byte in a name", b'{"\x01":"v"}', False, [(b"\x01", "v")])
add("raw control byte in another pair", b'{"c":"v","d":"\x1f"}', False)
add("DEL is legal", q(b"a\x7fz"), True, [("c", b"a\x7fz")])
add("space is legal", q(b" "), True, [("c", " ")])
for good in (b"\xc2\x80", b"\xc3\xa9", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xe2\x82\xac", b"\xec\xbf\xbf", b"\xed\x9f\xbf",
             b"\xee\x80\x80", b"\xef\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf0\x9f\x98\x80", b"\xf3\xbf\xbf\xbf",
             b"\xf4\x8f\xbf\xbf"):
    add("well-formed UTF-8 %s" % good.hex(), q(b"a" + good + b"z"), True, [("c", b"a" + good + b"z")])
    add("well-formed UTF-8 %s as a name" % good.hex(), b'{"' + good + b'":"v"}', True, [(good, "v")])
UTF8_BAD = {
    "overlong two bytes": [b"\xc0\x80", b"\xc0\xaf", b"\xc1\xbf"],
    "overlong three bytes": [b"\xe0\x80\x80", b"\xe0\x9f\xbf"],
    "overlong four bytes": [b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf"],
    "encoded surrogate": [b"\xed\xa0\x80", b"\xed\xad\xbf", b"\xed\xb0\x80", b"\xed\xbf\xbf"],
    "above U+10FFFF": [b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf7\xbf\xbf\xbf"],
    "five and six byte forms": [b"\xf8\x88\x80\x80\x80", b"\xfc\x84\x80\x80\x80\x80"],
    "never a UTF-8 byte": [b"\xfe", b"\xff"],
    "lone continuation": [b"\x80", b"\xbf", b"\xc3\xa9\xa9"],
    "bad continuation": [b"\xc3\x28", b"\xc3\xc3", b"\xe2\x28\xac", b"\xe2\x82\x28", b"\xf0\x28\x98\x80",
                         b"\xf0\x9f\x28\x80", b"\xf0\x9f\x98\x28"],
    "cut off by the end of the string": [b"\xc3", b"\xe2", b"\xe2\x82", b"\xf0", b"\xf0\x9f", b"\xf0\x9f\x98"],
}
for klass, seqs in UTF8_BAD.items():
    for s in seqs:
        add("%s %s" % (klass, s.hex()), q(b"v" + s), False, [("c", b"v" + s)])
        add("%s %s in another pair" % (klass, s.hex()), b'{"c":"v","d":"' + s + b'"}', False)
for s in (b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98"):
    add("UTF-8 cut off by the end of input %s" % s.hex(), b'{"c":"v","d":"' + s, False)
add("bad UTF-8 outside a string", b'{"c":"v"}\xff', False)
add("bad UTF-8 before the object", b'\xc3{"c":"v"}', False)

# ---- whitespace and structure ----
add("no whitespace", b'{"c":"v"}', True)
add("whitespace in every position", b' \t\n\r{ \t"c"\n\r: \t"v"\r\n,\t "d" : "e" \n} \r\n\t', True)
add("whitespace in every position, the second pair", b' {\n"d" :\t"e"\r, "c"\t:\n"v" } ', True)
add("whitespace inside a string is data", b'{"c":" v"}', False)
add("whitespace inside a name is data", b'{" c":"v"}', False)
for ws in (b"\x0b", b"\x0c", b"\xc2\xa0", b"\x00", b"\xe2\x80\x8b"):
    add("not whitespace: %s" % ws.hex(), b'{"c":' + ws + b'"v"}', False)
    add("not whitespace after the object: %s" % ws.hex(), b'{"c":"v"}' + ws, False)
add("a BOM", b'\xef\xbb\xbf{"c":"v"}', False)
add("a trailing comma", b'{"c":"v",}', False)
add("a trailing comma after two pairs", b'{"c":"v","d":"e" , }', False)
add("a leading comma", b'{,"c":"v"}', False)
add("two commas", b'{"c":"v",,"d":"e"}', False)
add("a missing comma", b'{"c":"v" "d":"e"}', False)
add("a missing colon", b'{"c" "v"}', False)
add("a missing colon in another pair", b'{"c":"v","d" "e"}', False)
add("two colons", b'{"c"::"v"}', False)
add("a comma for the colon", b'{"c","v"}', False)
add("a missing value", b'{"c":}', False)
add("a missing value at the end", b'{"c":"v","d":}', False)
add("a name alone", b'{"c"}', False)
for k in (b"1", b"c", b"null", b"true", b"'c'", b"[]", b"{}"):
    add("a non-string key %r" % k, b"{" + k + b':"v"}', False)
    add("a non-string key %r in another pair" % k, b'{"c":"v",' + k + b':"v"}', False)
for v in (b"1", b"-1.5e3", b"null", b"true", b"false", b"v", b"'v'", b'["v"]', b"[]", b'{"c":"v"}', b"{}", b"NaN"):
    add("a non-string value %r" % v, b'{"c":' + v + b"}", False)
    add("a non-string value %r in another pair" % v, b'{"c":"v","d":' + v + b"}", False)
    add("a non-string value %r before the pair" % v, b'{"d":' + v + b',"c":"v"}', False)
add("a nested object that holds the pair", b'{"x":{"c":"v"}}', False)
for top in (b"null", b"[]", b'["c","v"]', b'[{"c":"v"}]', b'"c"', b"1", b"true", b'"c":"v"'):
    add("the top level is %r" % top, top, False)
add("the empty object", b"{}", False)
add("the empty object with whitespace", b" { } ", False)
add("only whitespace", b" \t\n\r", False)
add("one space", b" ", False)
add("garbage after a matching pair", b'{"c":"v"}x', False)
add("a second object", b'{"c":"v"}{}', False)
add("a comma after the object", b'{"c":"v"} ,', False)
add("a second closing brace", b'{"c":"v"}}', False)
add("a quote after the object", b'{"c":"v"}"', False)
for cut in (b"{", b'{"', b'{"c', b'{"c"', b'{"c":', b'{"c":"', b'{"c":"v', b'{"c":"v"', b'{"c":"v",', b'{"c":"v\\',
            b'{"c":"\\u00', b'{"c":"v","d'):
    add("cut off: %r" % cut, cut, False)
add("single quotes", b"{'c':'v'}", False)

# ---- duplicates, prefixes, empties ----
add("duplicate keys, the last one matches", b'{"c":"x","c":"v"}', True)
add("duplicate keys, the last one does not", b'{"c":"v","c":"x"}', False)
add("three duplicates, match in the middle", b'{"c":"x","c":"v","c":"y"}', False)
add("three duplicates with others between", b'{"c":"x","d":"v","c":"y","e":"v","c":"v"}', True)
add("a duplicate through an escape", b'{"c":"v","\\u0063":"x"}', False)
add("the value is a prefix of the condition", q(b"v"), False, [("c", "vv")])
add("the condition is a prefix of the value", q(b"vv"), False)
add("the empty value against a condition", q(b""), False)
add("the name is a prefix of the column", b'{"c":"v"}', False, [("cc", "v")])
add("the column is a prefix of the name", b'{"cc":"v"}', False)
add("the column is absent", b'{"d":"v"}', False)
add("name and value swapped", b'{"v":"c"}', False)
add("an empty name and an empty value", b'{"":""}', True, [("", "")])
add("an empty name", b'{"":"v"}', True, [("", "v")])
add("an empty value", b'{"c":""}', True, [("c", "")])
add("an empty name against a name", b'{"":"v"}', False)
add("an empty condition value against a value", q(b"v"), False, [("c", "")])
add("case matters", b'{"C":"v"}', False)
add("two conditions, both hold", b'{"a":"1","b":"2"}', True, [("a", "1"), ("b", "2")])
add("two conditions, pairs reversed", b'{"b":"2","a":"1"}', True, [("a", "1"), ("b", "2")])
add("two conditions, one fails", b'{"a":"1","b":"2"}', False, [("a", "1"), ("b", "3")])
add("two conditions, one absent", b'{"a":"1"}', False, [("a", "1"), ("b", "2")])
add("one column twice, the same value", b'{"a":"1"}', True, [("a", "1"), ("a", "1")])
add("one column twice, two values", b'{"a":"1","a":"2"}', False, [("a", "1"), ("a", "2")])
add("two columns with one value", b'{"a":"1","b":"1"}', True, [("a", "1"), ("b", "1")])
add("sixteen conditions", b"{" + b",".join(b'"k%d":"%d"' % (i, i) for i in range(16)) + b"}", True,
    [("k%d" % i, "%d" % i) for i in range(16)])
add("sixteen conditions, the last fails", b"{" + b",".join(b'"k%d":"%d"' % (i, i) for i in range(16)) + b"}", False,
    [("k%d" % i, "%d" % (i if i < 15 else 0)) for i in range(16)])
add("no condition, a JSON row", b'{"c":"v"}', True, [])
add("no condition, not JSON", b"not json", True, [])
add("no condition, one byte", b"x", True, [])

# ---- split_ts's 8: whole values of 0 to 9 bytes, and payload lengths mod 3 ----
for n in range(10):
    v = (b'{"":""}' + b"  ")[:n]
    # 7 bytes: below 8, the value is its own payload and a document; 8 bytes: no payload left (dead);
    # 9 bytes: one space of payload, no document
    add("a value of %d bytes" % n, v, n == 7, [("", "")], raw=True)
    add("a value of %d bytes, no condition" % n, v, n not in (0, 8), [], raw=True)
add("exactly the timestamp", b"", False)
add("exactly the timestamp, no condition", b"", False, [])
add("a short value is its own payload", b'{"c":1}', False, raw=True)
for pad in range(3):
    add("payload length %d mod 3" % ((9 + pad) % 3), b'{"c":"v"}' + b" " * pad, True)
    add("payload length %d mod 3, garbage last" % ((10 + pad) % 3), b'{"c":"v"}' + b" " * pad + b"x", False)
    add("payload length %d mod 3, the match last" % ((12 + pad) % 3), b'{"c":"' + b"w" * pad + b'v"}', True,
        [("c", "w" * pad + "v")])

# ---- key conditions ----
KC = ("pk", "ck")
add("a key condition alone, payload not JSON", b"not json", True, [("pk", "a")], b"ns:a|b", KC)
add("a key condition fails", b'{"pk":"b"}', False, [("pk", "b")], b"ns:a|b", KC)
add("the second key part", b"\xff", True, [("ck", "b")], b"ns:a|b", KC)
add("both key parts", b"{", True, [("pk", "a"), ("ck", "b")], b"ns:a|b", KC)
add("both key parts, one fails", b'{"ck":"c"}', False, [("pk", "a"), ("ck", "c")], b"ns:a|b", KC)
add("the key part overrides the map", b'{"pk":"zzz"}', True, [("pk", "a")], b"ns:a|b", KC)
add("the map does not answer for a key part", b'{"pk":"zzz"}', False, [("pk", "zzz")], b"ns:a|b", KC)
add("a key condition and a JSON one", b'{"c":"v"}', True, [("pk", "a"), ("c", "v")], b"ns:a|b", KC)
add("a key condition and a JSON one, bad JSON", b'{"c":"v"', False, [("pk", "a"), ("c", "v")], b"ns:a|b", KC)
add("a key condition and a JSON one, the key fails", b'{"c":"v"}', False, [("pk", "b"), ("c", "v")], b"ns:a|b", KC)
add("fewer parts than key columns: the JSON answers", b'{"ck":"b"}', True, [("ck", "b")], b"ns:a", KC)
add("fewer parts than key columns: the JSON differs", b'{"ck":"c"}', False, [("ck", "b")], b"ns:a", KC)
add("fewer parts than key columns: not JSON", b"not json", False, [("ck", "b")], b"ns:a", KC)
add("fewer parts than key columns: the first still answers", b"not json", True, [("pk", "a")], b"ns:a", KC)
add("more parts than key columns", b"x", True, [("pk", "a"), ("ck", "b")], b"ns:a|b|c", KC)
add("more parts than key columns: the rest is no part of ck", b"x", False, [("ck", "b|c")], b"ns:a|b|c", KC)
add("a key equal to its prefix is one empty part", b"x", True, [("pk", "")], b"ns:", KC)
add("a key equal to its prefix: ck falls back", b'{"ck":""}', True, [("pk", ""), ("ck", "")], b"ns:", KC)
add("a key equal to its prefix against a value", b"x", False, [("pk", "a")], b"ns:", KC)
add("skip past the key's end", b"x", True, [("pk", "")], b"ns", KC, skip=9)
add("skip zero: the prefix is in the part", b"x", True, [("pk", "ns:a")], b"ns:a|b", KC, skip=0)
add("an empty part in the middle", b"x", True, [("pk", "a"), ("ck", ""), ("c3", "c")], b"ns:a||c", ("pk", "ck", "c3"))
add("an empty last part", b"x", True, [("ck", "")], b"ns:a|", KC)
add("an empty last part against a value", b"x", False, [("ck", "b")], b"ns:a|", KC)
add("the part is a prefix of the condition", b"x", False, [("pk", "ab")], b"ns:a|b", KC)
add("the condition is a prefix of the part", b"x", False, [("pk", "a")], b"ns:ab|b", KC)
add("a bar in the condition never equals a part", b"x", False, [("pk", "a|b")], b"ns:a|b", KC)
add("a dead row with a matching key", b"", False, [("pk", "a")], b"ns:a|b", KC)
add("the empty key", b"x", True, [("pk", "")], b"", KC, skip=0)
add("a key column far past the parts", b'{"k9":"z"}', True, [("k9", "z")], b"ns:a|b", tuple("k%d" % i for i in range(10)))
