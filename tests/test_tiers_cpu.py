"""The tiered filter sets' surface (cb_tiers_probe_* / cb_tiers_get_many_*),
checked without a GPU: the header's declarations, the exports and ctypes
prototypes, the Python entry points, the Rust declarations, and the refusals
that need no device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cb_tiers_probe_fixed", "cb_tiers_probe_var", "cb_tiers_get_many_fixed", "cb_tiers_get_many_var"]


def _header_params(name):
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"no prototype for {name}"
    return [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", SYMBOLS)
def test_header_export_and_ctypes(name):
    from lsmt_amd import _lib
    assert name in _lib.header_symbols()
    L = _lib.load()
    assert hasattr(L, name)
    assert len(getattr(L, name).argtypes) == len(_header_params(name))


def test_header_parameter_names():
    assert _header_params("cb_tiers_probe_fixed") == ["sets", "ns", "tiers", "slots", "nt", "keys", "key_len", "n",
                                                      "gated", "hits", "stream"]
    assert _header_params("cb_tiers_probe_var") == ["sets", "ns", "tiers", "slots", "nt", "bytes", "offsets", "n",
                                                    "gated", "hits", "stream"]
    assert _header_params("cb_tiers_get_many_fixed") == ["sets", "ns", "tables", "nt", "tiers", "slots", "keys",
                                                         "key_len", "n", "which", "val_off", "vals", "cap", "total",
                                                         "stream"]
    assert _header_params("cb_tiers_get_many_var") == ["sets", "ns", "tables", "nt", "tiers", "slots", "bytes",
                                                       "offsets", "n", "which", "val_off", "vals", "cap", "total",
                                                       "stream"]


def test_python_entry_points():
    import lsmt_amd
    assert "probe_tiers" in lsmt_amd.__all__ and "get_many_tiers" in lsmt_amd.__all__
    sig = inspect.signature(lsmt_amd.probe_tiers)
    assert list(sig.parameters) == ["sets", "tiers", "slots", "keys", "gated", "out", "stream"]
    assert sig.parameters["gated"].default is True
    assert sig.parameters["out"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(lsmt_amd.get_many_tiers)
    assert list(sig.parameters) == ["tables", "sets", "tiers", "slots", "keys", "stream", "out", "wait"]
    assert sig.parameters["wait"].default is True
    assert sig.parameters["out"].default is None and sig.parameters["stream"].default is None


@pytest.mark.parametrize("name", SYMBOLS)
def test_integration_doc_declares_it(name):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert re.search(r"pub fn " + name + r"\(", fh.read())


def test_null_argument_errors_without_gpu():
    from lsmt_amd import _lib
    L = _lib.load()
    one = np.zeros(1, np.uint32)
    keys = np.zeros(16, np.uint8)
    offs = np.zeros(2, np.uint64)
    hits = np.zeros(1, np.uint64)
    which = np.zeros(1, np.int32)
    voff = np.zeros(2, np.uint64)
    tot = ctypes.c_uint64(7)
    p = lambda a: a.ctypes.data  # noqa: E731
    # no sets at all
    assert L.cb_tiers_probe_fixed(None, 1, p(one), p(one), 1, p(keys), 16, 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert b"null" in L.cb_last_error()
    assert L.cb_tiers_probe_var(None, 1, p(one), p(one), 1, p(keys), p(offs), 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert L.cb_tiers_get_many_fixed(None, 1, None, 1, p(one), p(one), p(keys), 16, 1, p(which), p(voff), None, 0,
                                     ctypes.byref(tot), None) == _lib.CB_EINVAL
    assert L.cb_tiers_get_many_var(None, 1, None, 1, p(one), p(one), p(keys), p(offs), 1, p(which), p(voff), None,
                                   0, ctypes.byref(tot), None) == _lib.CB_EINVAL
    # a set array whose only entry is NULL, and missing tiers / slots / offsets
    sets = (ctypes.c_void_p * 1)(None)
    sp = ctypes.cast(sets, ctypes.c_void_p)
    assert L.cb_tiers_probe_fixed(sp, 1, p(one), p(one), 1, p(keys), 16, 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert L.cb_tiers_probe_fixed(sp, 1, None, p(one), 1, p(keys), 16, 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert L.cb_tiers_probe_fixed(sp, 1, p(one), None, 1, p(keys), 16, 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert L.cb_tiers_probe_var(sp, 1, p(one), p(one), 1, p(keys), None, 1, 1, p(hits), None) == _lib.CB_EINVAL
    # the counts are checked before any set is looked at
    for ns, nt in [(0, 1), (9, 1), (1, 0), (1, 65)]:
        assert L.cb_tiers_probe_fixed(sp, ns, p(one), p(one), nt, p(keys), 16, 1, 1, p(hits), None) == _lib.CB_EINVAL
    assert hits[0] == 0 and which[0] == 0 and tot.value == 7  # nothing was written
