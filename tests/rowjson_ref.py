"""The row rule behind cb_tables_count_where, cb_scan_match and cb_row_matches,
restated in plain Python, independently of lsmt_amd/csrc/rowjson.hpp (a
recursive-descent reader over bytes where the C++ is one state machine).

What it restates (the reference's SELECT COUNT(*) ... WHERE, src/query.rs:309-362):
  payload(value)  split_ts (src/query.rs:21-27): the value below 8 bytes, else value[8:]
  json_map(p)     serde_json::from_slice::<BTreeMap<String, String>>(p).unwrap_or_default()
                  (decode_row, src/schema.rs:42-44), as a dict of bytes -> bytes
  parts(key, s)   key[min(s, len):].split("|")
  matches(...)    every condition: the key part when the row has it, else the map

The verdict never comes from json.loads; tests/test_where_cpu.py compares the
map with json.loads as a second witness.
"""
import functools

WS = b" \t\n\r"
ESCAPES = {ord('"'): b'"', ord("\\"): b"\\", ord("/"): b"/", ord("b"): b"\b", ord("f"): b"\f", ord("n"): b"\n",
           ord("r"): b"\r", ord("t"): b"\t"}
HEX = b"0123456789abcdefABCDEF"


class Bad(Exception):
    pass


def payload(value: bytes) -> bytes:
    return value if len(value) < 8 else value[8:]


def _utf8_len(b: bytes, i: int) -> int:
    """The length of the well-formed UTF-8 sequence that starts at b[i] (Rust's
    str::from_utf8 table), or Bad."""
    c = b[i]
    if c < 0x80:
        return 1
    if 0xC2 <= c <= 0xDF:
        bounds = [(0x80, 0xBF)]
    elif c == 0xE0:
        bounds = [(0xA0, 0xBF), (0x80, 0xBF)]
    elif 0xE1 <= c <= 0xEC or 0xEE <= c <= 0xEF:
        bounds = [(0x80, 0xBF)] * 2
    elif c == 0xED:
        bounds = [(0x80, 0x9F), (0x80, 0xBF)]
    elif c == 0xF0:
        bounds = [(0x90, 0xBF)] + [(0x80, 0xBF)] * 2
    elif 0xF1 <= c <= 0xF3:
        bounds = [(0x80, 0xBF)] * 3
    elif c == 0xF4:
        bounds = [(0x80, 0x8F)] + [(0x80, 0xBF)] * 2
    else:
        raise Bad("lead byte")
    for k, (lo, hi) in enumerate(bounds):
        if i + 1 + k >= len(b) or not lo <= b[i + 1 + k] <= hi:
            raise Bad("continuation byte")
    return 1 + len(bounds)


def _hex4(b: bytes, i: int) -> int:
    h = b[i:i + 4]
    if len(h) != 4 or any(c not in HEX for c in h):
        raise Bad("hex digits")
    return int(h, 16)


def _string(b: bytes, i: int):
    """b[i] is the opening quote: (the unescaped bytes, the index after the
    closing quote)."""
    out = bytearray()
    i += 1
    while True:
        if i >= len(b):
            raise Bad("unterminated string")
        c = b[i]
        if c == 0x22:
            return bytes(out), i + 1
        if c < 0x20:
            raise Bad("control byte in a string")
        if c != 0x5C:
            n = _utf8_len(b, i)
            out += b[i:i + n]
            i += n
            continue
        if i + 1 >= len(b):
            raise Bad("unterminated escape")
        e = b[i + 1]
        if e in ESCAPES:
            out += ESCAPES[e]
            i += 2
            continue
        if e != ord("u"):
            raise Bad("unknown escape")
        cp = _hex4(b, i + 2)
        i += 6
        if 0xDC00 <= cp <= 0xDFFF:
            raise Bad("lone low surrogate")
        if 0xD800 <= cp <= 0xDBFF:
            if b[i:i + 2] != b"\\u":
                raise Bad("lone high surrogate")
            low = _hex4(b, i + 2)
            if not 0xDC00 <= low <= 0xDFFF:
                raise Bad("high surrogate without a low one")
            cp = 0x10000 + ((cp - 0xD800) << 10) + (low - 0xDC00)
            i += 6
        out += chr(cp).encode("utf-8")


def _skip_ws(b: bytes, i: int) -> int:
    while i < len(b) and b[i] in WS:
        i += 1
    return i


def parse_pairs(b: bytes):
    """The document's (name, value) pairs in order, or Bad."""
    i = _skip_ws(b, 0)
    if i >= len(b) or b[i] != ord("{"):
        raise Bad("no object")
    i = _skip_ws(b, i + 1)
    pairs = []
    if i < len(b) and b[i] == ord("}"):
        i += 1
    else:
        while True:
            if i >= len(b) or b[i] != 0x22:
                raise Bad("a name must be a string")
            name, i = _string(b, i)
            i = _skip_ws(b, i)
            if i >= len(b) or b[i] != ord(":"):
                raise Bad("no colon")
            i = _skip_ws(b, i + 1)
            if i >= len(b) or b[i] != 0x22:
                raise Bad("a value must be a string")
            value, i = _string(b, i)
            pairs.append((name, value))
            i = _skip_ws(b, i)
            if i < len(b) and b[i] == ord(","):
                i = _skip_ws(b, i + 1)
                continue
            if i < len(b) and b[i] == ord("}"):
                i += 1
                break
            raise Bad("no comma or brace")
    if _skip_ws(b, i) != len(b):
        raise Bad("trailing bytes")
    return pairs


@functools.lru_cache(maxsize=None)
def json_map(b: bytes) -> dict:
    """unwrap_or_default: any error gives the empty map. The last of
    duplicate names wins. (Cached per payload: callers do not change it.)"""
    try:
        return dict(parse_pairs(b))
    except Bad:
        return {}


def parts(key: bytes, skip: int):
    return key[min(skip, len(key)):].split(b"|")


def normalize(where, key_columns=()):
    """[(column, value, part)] from a mapping or a list of (column, value)."""
    as_bytes = lambda x: x.encode() if isinstance(x, str) else bytes(x)  # noqa: E731
    pairs = list(where.items()) if hasattr(where, "items") else list(where)
    kc = [as_bytes(c) for c in key_columns]
    return [(as_bytes(c), as_bytes(v), kc.index(as_bytes(c)) if as_bytes(c) in kc else -1) for c, v in pairs]


def matches(key: bytes, value: bytes, where, key_columns=(), skip: int = 0) -> bool:
    p = payload(value)
    if not p:
        return False  # a deleted row
    kp = parts(key, skip)
    doc = None
    for col, val, part in normalize(where, key_columns):
        if 0 <= part < len(kp):
            if kp[part] != val:
                return False
            continue
        if doc is None:
            doc = json_map(p)
        if doc.get(col) != val:
            return False
    return True
