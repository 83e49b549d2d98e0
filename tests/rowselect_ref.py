"""The selection rule behind cb_scan_select, cb_rows_select and cb_row_select,
restated in plain Python, independently of lsmt_amd/csrc/rowselect.hpp: whole
maps and whole strings where the C++ sizes and writes byte by byte in two
passes. Built on rowjson_ref.json_map and rowjson_ref.parts; the escaper and
the integer cast are this file's own.

What it restates (the reference's exec_select_schema, src/query.rs:365-432):
  split_ts, the deleted row (src/query.rs:396-400), decode_row, the key parts
  laid over the map (src/query.rs:402-405), project_row with cast_simple
  (src/query.rs:641-662, 817-827), encode_row (src/schema.rs:37-39) and the two
  forms of the response (src/query.rs:411-431).

Like rowjson_ref.py this is a restatement of serde_json's and Rust's
documented behaviour and was NOT run against the reference.
tests/test_select_cpu.py compares its objects with json.dumps as a second
witness.
"""
import rowjson_ref

TEXT, DEAD, ABSENT, BADJSON, EXTRA = 1, 2, 4, 8, 16

SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def as_bytes(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


def escape(b: bytes) -> bytes:
    """A string's bytes between the quotes, as serde_json writes them."""
    out = bytearray()
    for c in b:
        if c in SHORT:
            out += SHORT[c]
        elif c < 0x20:
            out += b"\\u00%02x" % c
        else:
            out.append(c)
    return bytes(out)


def cast_int(v: bytes) -> bytes:
    """v.parse::<i64>().ok().map(|i| i.to_string()).unwrap_or(v)."""
    digits = v[1:] if v[:1] in (b"+", b"-") else v
    if not digits or any(not 0x30 <= c <= 0x39 for c in digits):
        return v
    digits = digits.lstrip(b"0") or b"0"
    if len(digits) > 19:
        return v
    n = -int(digits) if v[:1] == b"-" else int(digits)
    return str(n).encode() if -2 ** 63 <= n <= 2 ** 63 - 1 else v


def split_ts(value: bytes):
    return (0, value) if len(value) < 8 else (int.from_bytes(value[:8], "big"), value[8:])


def normalize(columns, key_columns=(), casts=None):
    """[(name, part, cast)] sorted by name, the last cast of a repeated name."""
    names = [as_bytes(c) for c in columns]
    if casts is None:
        given = [0] * len(names)
    elif hasattr(casts, "items"):
        by = {as_bytes(c): int(v) for c, v in casts.items()}
        given = [by.get(c, 0) for c in names]
    else:
        given = [int(v) for v in casts]
    chosen = {}
    for c, v in zip(names, given):
        chosen[c] = v
    kc = [as_bytes(c) for c in key_columns]
    return [(c, kc.index(c) if c in kc else -1, chosen[c]) for c in sorted(chosen)]


def row_map(key: bytes, payload: bytes, sel, skip: int):
    """(the selected columns' values as a dict in selection order, flags of a live row)."""
    doc = rowjson_ref.json_map(payload)
    valid = True
    if not doc:
        try:
            rowjson_ref.parse_pairs(payload)  # (the empty map of {} is valid; that of an error is not)
        except rowjson_ref.Bad:
            valid = False
    kp = rowjson_ref.parts(key, skip)
    names = set(c for c, _, _ in sel)
    flags = TEXT | (0 if valid else BADJSON) | (EXTRA if any(k not in names for k in doc) else 0)
    out = {}
    for col, part, cast in sel:
        if 0 <= part < len(kp):
            v = kp[part]
        elif col in doc:
            v = doc[col]
        else:
            continue
        out[col] = cast_int(v) if cast else v
    return out, flags


def encode(m: dict) -> bytes:
    return b"{" + b",".join(b'"' + escape(k) + b'":"' + escape(v) + b'"' for k, v in m.items()) + b"}"


def row_text(key: bytes, value: bytes, sel, skip: int = 0, meta: bool = False, absent: bool = False):
    """(the row's text or None, its flags)."""
    if absent:
        return None, ABSENT
    ts, payload = split_ts(value)
    head = key[min(skip, len(key)):] + b"\t" + str(ts).encode() + b"\t"
    if not payload:
        return (head, DEAD | TEXT) if meta else (None, DEAD)
    m, flags = row_map(key, payload, sel, skip)
    return (head if meta else b"") + encode(m), flags


def response(texts, meta: bool = False) -> bytes:
    have = [t for t in texts if t is not None]
    return b"\n".join(have) if meta else b"[" + b",".join(have) + b"]"
