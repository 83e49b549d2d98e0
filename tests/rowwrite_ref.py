"""A plain-Python restatement of the rule in lsmt_amd/csrc/rowwrite.hpp: the key,
value and log record an INSERT, UPDATE or DELETE stores for a row
(src/query.rs:162-261, 716-731, src/schema.rs:37-39, src/lib.rs:96-116, 154-157).

It is independent of the library and of tests/rowjson_ref.py: a dict stands for
the BTreeMap, Python's json module reads the old map, the escaper below writes
serde_json's strings, base64.b64encode the log record. Like rowselect.hpp's it
is a restatement and was NOT run against the reference, which cannot be built
here (no vendored crates).
"""
import base64
import json

INSERT, UPDATE, DELETE = 0, 1, 2
HOST, BADOLD, KEYCTL = 1, 2, 4

_SHORT = {8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t", 0x22: b'\\"', 0x5C: b"\\\\"}


def escape(s: bytes) -> bytes:
    """A string's bytes as serde_json writes them between the quotes."""
    out = bytearray()
    for b in s:
        if b in _SHORT:
            out += _SHORT[b]
        elif b < 0x20:
            out += b"\\u%04x" % b
        else:
            out.append(b)
    return bytes(out)


def encode_row(m: dict) -> bytes:
    """encode_row of a BTreeMap<String, String> given as {bytes: bytes}."""
    return b"{" + b",".join(b'"%s":"%s"' % (escape(k), escape(m[k])) for k in sorted(m)) + b"}"


def split_ts(value: bytes):
    return (0, value) if len(value) < 8 else (int.from_bytes(value[:8], "big"), value[8:])


def decode_row(payload: bytes):
    """The payload's map {bytes: bytes}, or None where serde_json's
    from_slice::<BTreeMap<String, String>> fails (the reference then takes the
    default, the empty map). Python's json module is laxer in known ways, each
    closed here: the bytes must be UTF-8, control characters inside strings are
    refused (strict), the top level must be an object written with braces,
    every value a string, and no string may hold a surrogate (serde_json
    refuses a lone one; a pair has already become one character)."""
    try:
        text = payload.decode("utf-8", "strict")
        pairs = json.loads(text, strict=True, object_pairs_hook=list)
    except (UnicodeDecodeError, ValueError, RecursionError):
        return None
    if not text.lstrip(" \t\n\r").startswith("{") or not isinstance(pairs, list):
        return None
    m = {}
    for pair in pairs:
        if not (isinstance(pair, tuple) and len(pair) == 2 and isinstance(pair[1], str)):
            return None
        if any(0xD800 <= ord(ch) <= 0xDFFF for ch in pair[0] + pair[1]):
            return None
        m[pair[0].encode()] = pair[1].encode()  # (the last pair of a name wins)
    return m


def write_row(ns: bytes, key_cells, names, given: dict, op: int, ts: int, old=None):
    """(key, value, record, flags) of one row. names: every payload column of
    the statement (any order); given: {name: cell} for the columns it sets;
    old: the old value's bytes or None. value and record are None for a row
    flagged HOST."""
    key = ns + b":" + b"|".join(key_cells)
    flags = KEYCTL if (b"\t" in key or b"\n" in key) else 0
    if op == DELETE:
        payload = b""
    else:
        row = {}
        if op == UPDATE and old is not None:
            _, data = split_ts(old)
            if data:  # (an empty payload is a tombstone: the empty map, and no error of the store's)
                m = decode_row(data)
                if m is None:
                    flags |= BADOLD
                elif set(m) - set(names):
                    return key, None, None, flags | HOST
                else:
                    row = m
        row.update(given)
        payload = encode_row(row)
    value = ts.to_bytes(8, "big") + payload
    return key, value, key + b"\t" + base64.b64encode(value) + b"\n", flags


def write_batch(ns, rows, nk, columns=(), keep=(), op=INSERT, ts=0, old=None):
    """lsmt_amd.write.write_rows over lists: rows of nk key cells then one cell
    per name of `columns`; ts an int or one per row; old a list of old values
    (None: no row). Returns (keys, values, records, flags), values and records
    b"" for HOST rows."""
    names = list(columns) + list(keep)
    keys, vals, recs, flags = [], [], [], []
    for i, row in enumerate(rows):
        t = ts if isinstance(ts, int) else int(ts[i])
        k, v, r, f = write_row(ns, list(row[:nk]), names, dict(zip(columns, row[nk:])), op, t,
                               None if old is None else old[i])
        keys.append(k)
        vals.append(v or b"")
        recs.append(r or b"")
        flags.append(f)
    return keys, vals, recs, flags
