"""cb_tables_compact's surface, checked without a GPU: the Python entry point,
the header's declaration and the ctypes prototype (the export and parse checks
of test_capi_cpu.py / test_integration_abi.py then cover the symbol too)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_entry_point():
    import lsmt_amd
    assert "compact" in lsmt_amd.__all__
    sig = inspect.signature(lsmt_amd.compact)
    assert list(sig.parameters) == ["tables", "m", "stream"]
    assert sig.parameters["m"].default == 1024 and sig.parameters["stream"].default is None


def test_header_declares_it_and_ctypes_matches():
    from lsmt_amd import _lib
    assert "cb_tables_compact" in _lib.header_symbols()
    with open(os.path.join(ROOT, "include", "cassbloom.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    m = re.search(r"int\s+cb_tables_compact\s*\(([^)]*)\)\s*;", text)
    assert m, "no prototype"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["tables", "nt", "m_bits", "stream", "table_out", "bloom_out"]
    fn = _lib.load().cb_tables_compact
    assert len(fn.argtypes) == len(params)


def test_integration_doc_declares_it():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert re.search(r"pub fn cb_tables_compact\(", fh.read())
