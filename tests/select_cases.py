"""Hand-worked answers of the selection rule (lsmt_amd/csrc/rowselect.hpp): one
row each, with the object the reference's exec_select_schema would write for
it. A plain module: no test, no fixture, nothing collected.

Every key is `ns:` + its parts, read with skip = 3 unless the case says
otherwise; no key holds a tab or a newline, so every case can also be a line of
a data file. A case's `obj` is written out by hand; its two texts follow from
it: the object itself for a client, `key \\t ts \\t object` for a coordinator.
"""
from collections import namedtuple

TEXT, DEAD, ABSENT, BADJSON, EXTRA = 1, 2, 4, 8, 16
TS = (5).to_bytes(8, "big")
KC = ("pk", "ck")

Case = namedtuple("Case", "label key value columns key_columns casts skip obj flags ts absent")
CASES = []


def case(label, payload, columns, obj, flags=TEXT, key=b"ns:k1|c2", key_columns=KC, casts=None, skip=3, ts=TS,
         absent=False):
    """payload None: the value is `ts` alone (a deleted row). ts: the value's
    first bytes as they are (b"" for a value that is its own payload)."""
    value = ts if payload is None else ts + payload
    stamp = int.from_bytes(ts, "big") if len(value) >= 8 else 0
    CASES.append(Case(label, key, value, tuple(columns), tuple(key_columns), casts, skip, obj, flags, stamp, absent))


def json_text(c):
    return c.obj if c.flags & TEXT and not c.flags & DEAD else None


def meta_text(c):
    if c.flags & ABSENT:
        return None
    head = c.key[min(c.skip, len(c.key)):] + b"\t%d\t" % c.ts
    return head if c.flags & DEAD else head + c.obj


def flags_of(c, meta):
    return c.flags | TEXT if meta and c.flags & DEAD else c.flags


# ---- strings ----
case("every escape read and written", rb'{"a":"q\"b\\s\/\b\f\n\r\t"}', ["a"], rb'{"a":"q\"b\\s/\b\f\n\r\t"}')
case("raw bytes that need no escape", b'{"a":"x/y\x7f z"}', ["a"], b'{"a":"x/y\x7f z"}')
case("u0000", rb'{"a":"x\u0000y"}', ["a"], rb'{"a":"x\u0000y"}')
case("control escapes come back in lower-case hex", rb'{"a":"\u001F\u001f\u0001\u000B\u000e"}', ["a"],
     rb'{"a":"\u001f\u001f\u0001\u000b\u000e"}')
case("u escapes of the short forms come back short", rb'{"a":"\u0008\u000c\u000A\u000d\u0009\u0022\u005c\u002f"}', ["a"],
     rb'{"a":"\b\f\n\r\t\"\\/"}')
case("a surrogate pair becomes four raw bytes", rb'{"a":"\ud83d\ude00!"}', ["a"], b'{"a":"\xf0\x9f\x98\x80!"}')
case("u escapes of non-ASCII become raw UTF-8", rb'{"a":"\u00e9\u20AC\u007f"}', ["a"], b'{"a":"\xc3\xa9\xe2\x82\xac\x7f"}')
case("raw UTF-8 is copied", '{"a":"é€😀"}'.encode(), ["a"], '{"a":"é€😀"}'.encode())
case("a name that needs escapes", rb'{"a\"\n\u0001":"1"}', [b'a"\n\x01'], rb'{"a\"\n\u0001":"1"}')
case("a name matched through its escapes", rb'{"\u0061b":"1"}', ["ab"], b'{"ab":"1"}')
case("whitespace around everything", b' \t{ "a" :\n"1" ,\r"b" : "2" } \n', ["a", "b"], b'{"a":"1","b":"2"}')

# ---- column lookup ----
case("the last of a duplicate name wins", b'{"a":"1","b":"x","a":"2"}', ["a", "b"], b'{"a":"2","b":"x"}')
case("the last of a duplicate name wins even when shorter", b'{"a":"long value","a":""}', ["a"], b'{"a":""}')
case("a name that is a prefix of another", b'{"ab":"1","a":"2","abc":"3"}', ["a", "ab"], b'{"a":"2","ab":"1"}',
     TEXT | EXTRA)
case("a longer name is not its prefix", b'{"ab":"1"}', ["a"], b"{}", TEXT | EXTRA)
case("an empty name and an empty value", b'{"":"","a":""}', ["", "a"], b'{"":"","a":""}')
case("an empty name that the map lacks", b'{"a":"1"}', ["", "a"], b'{"a":"1"}')
case("a key part overrides the payload", b'{"pk":"zz","a":"1"}', ["a", "pk"], b'{"a":"1","pk":"k1"}')
case("both key parts, the payload empty", b"{}", ["ck", "pk"], b'{"ck":"c2","pk":"k1"}')
case("part >= nparts falls back to the payload", b'{"ck":"pay"}', ["ck", "pk"], b'{"ck":"pay","pk":"k1"}', key=b"ns:k1")
case("part >= nparts and no pair: left out", b'{"a":"1"}', ["a", "ck"], b'{"a":"1"}', key=b"ns:k1")
case("key parts that need escaping", b"{}", ["ck", "pk"], rb'{"ck":"c\\d\u0001","pk":"a\"b"}', key=b'ns:a"b|c\\d\x01')
case("an empty key part", b'{"ck":"pay"}', ["ck", "pk"], b'{"ck":"","pk":"k"}', key=b"ns:k|")
case("skip past the key's end", b'{"pk":"pay"}', ["ck", "pk"], b'{"pk":""}', skip=40)
case("skip 0 takes the namespace into the part", b"{}", ["pk"], b'{"pk":"ns:k1"}', skip=0)
case("a third part nobody names", b'{"a":"1"}', ["a", "ck"], b'{"a":"1","ck":"c2"}', key=b"ns:k1|c2|x3")
case("selection order is name order, not the document's", b'{"z":"1","m":"2","a":"3"}', ["a", "m", "z"],
     b'{"a":"3","m":"2","z":"1"}')
case("no column selected", b'{"a":"1"}', [], b"{}", TEXT | EXTRA)
case("no column selected, empty map", b"{}", [], b"{}")

# ---- payload and row state ----
case("a payload that is no JSON: key columns only", b"not json", ["a", "pk"], b'{"pk":"k1"}', TEXT | BADJSON)
case("a payload that is no JSON: nothing", b"not json", ["a"], b"{}", TEXT | BADJSON)
case("an error after the last brace voids every pair", b'{"a":"1"}x', ["a", "pk"], b'{"pk":"k1"}', TEXT | BADJSON)
case("a value that is no string voids every pair", b'{"a":"1","b":2}', ["a"], b"{}", TEXT | BADJSON)
case("a truncated document", b'{"a":"1"', ["a"], b"{}", TEXT | BADJSON)
case("a lone surrogate voids the document", rb'{"a":"1","b":"\ud83d"}', ["a"], b"{}", TEXT | BADJSON)
case("bad UTF-8 in an unselected value voids the document", b'{"a":"1","b":"\xc3\x28"}', ["a"], b"{}", TEXT | BADJSON)
case("a value under 8 bytes is its own payload", b'{"":""}', [""], b'{"":""}', ts=b"")
case("a value under 8 bytes: the empty map", b"{}", ["pk"], b'{"pk":"k1"}', ts=b"")
case("a value under 8 bytes that is no JSON", b"1234567", ["a"], b"{}", TEXT | BADJSON, ts=b"")
case("a deleted row", None, ["a", "pk"], None, DEAD)
case("a value of no bytes is a deleted row", None, ["a"], None, DEAD, ts=b"")
case("a deleted row with an empty rest of the key", None, ["a"], None, DEAD, key=b"ns:")
case("no row at all", b'{"a":"1"}', ["a"], None, ABSENT, absent=True)

# ---- integer casts ----
N = {"n": 1}
for text, want in [("+7", "7"), ("-0", "0"), ("007", "7"), ("9223372036854775807", "9223372036854775807"),
                   ("9223372036854775808", "9223372036854775808"), ("-9223372036854775808", "-9223372036854775808"),
                   ("-9223372036854775809", "-9223372036854775809"), ("+9223372036854775807", "9223372036854775807"),
                   ("", ""), ("+", "+"), ("-", "-"), ("1 ", "1 "), (" 1", " 1"), ("+-1", "+-1"), ("--1", "--1"),
                   ("0000", "0"), ("-007", "-7"), ("+0", "0"), ("1_0", "1_0"), ("1e3", "1e3"), ("0x10", "0x10"),
                   ("12a", "12a"), ("1.0", "1.0"), ("000000000000000000000000000000000005", "5"),
                   ("00009223372036854775808", "00009223372036854775808"), ("18446744073709551616", "18446744073709551616"),
                   ("99999999999999999999999999", "99999999999999999999999999"), ("42", "42"), ("-1", "-1")]:
    case("cast %r" % text, b'{"n":"%s"}' % text.encode(), ["n"], b'{"n":"%s"}' % want.encode(), casts=N)
case("cast of digits behind escapes", rb'{"n":"\u002b\u0030\u0031\u0032"}', ["n"], b'{"n":"12"}', casts=N)
case("cast refused: the value is written escaped", rb'{"n":"1\n"}', ["n"], rb'{"n":"1\n"}', casts=N)
case("cast refused: a non-ASCII digit", '{"n":"１"}'.encode(), ["n"], '{"n":"１"}'.encode(), casts=N)
case("cast of a key part", b'{"pk":"9"}', ["pk"], b'{"pk":"5"}', key=b"ns:+05|c", casts={"pk": 1})
case("cast of a key part refused", b"{}", ["ck", "pk"], b'{"ck":"-","pk":"5x"}', key=b"ns:5x|-", casts={"pk": 1, "ck": 1})
case("cast of the last duplicate", b'{"n":"1","n":"-02"}', ["n"], b'{"n":"-2"}', casts=N)
case("no cast asked: the value stays", b'{"n":"007","m":"+1"}', ["m", "n"], b'{"m":"+1","n":"007"}', casts={"n": 0})
case("one column cast, its neighbour not", b'{"n":"007","m":"+1"}', ["m", "n"], b'{"m":"+1","n":"7"}', casts=N)

# ---- flags and framing ----
case("a name outside the selection sets EXTRA", b'{"a":"1","b":"2"}', ["a"], b'{"a":"1"}', TEXT | EXTRA)
case("every name inside the selection: no EXTRA", b'{"a":"1","b":"2"}', ["a", "b", "c"], b'{"a":"1","b":"2"}')
case("a key column in the payload and in the selection: no EXTRA", b'{"pk":"zz"}', ["pk"], b'{"pk":"k1"}')
case("a key column in the payload, not selected: EXTRA", b'{"pk":"zz","a":"1"}', ["a"], b'{"a":"1"}', TEXT | EXTRA)
case("ts 0", b'{"a":"1"}', ["a"], b'{"a":"1"}', ts=bytes(8))
case("ts 2^64 - 1", b'{"a":"1"}', ["a"], b'{"a":"1"}', ts=b"\xff" * 8)
case("ts 2^64 - 1 of a deleted row", None, ["a"], None, DEAD, ts=b"\xff" * 8)
case("ts 10^19", b"{}", [], b"{}", ts=(10 ** 19).to_bytes(8, "big"))
