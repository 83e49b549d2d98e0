"""The package's public Python surface against a recording of it
(tests/golden/python_surface.json): the exported names, every signature,
property and method of them, their docstrings, and that the package's modules
import in any order. No device call is made here."""
import ast
import glob
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsmt_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_surface.json")


def _params(fn):
    try:
        sig = inspect.signature(fn)
    except ValueError:  # (a ctypes structure: LogStats)
        return None
    return [[p.name, p.kind.name, None if p.default is p.empty else repr(p.default)] for p in sig.parameters.values()]


def _callable(fn):
    return {"params": _params(fn), "doc": bool(fn.__doc__)}


def _member(cls, name):
    m = inspect.getattr_static(cls, name)
    if isinstance(m, property):
        return {"kind": "property", "doc": bool(m.__doc__)}
    if isinstance(m, (classmethod, staticmethod)):
        return {"kind": type(m).__name__, **_callable(m.__func__)}
    if inspect.isfunction(m):
        return {"kind": "method", **_callable(m)}
    return {"kind": "attribute"}


def surface():
    """What the fixture holds, taken from the imported package."""
    import lsmt_amd
    out = {}
    for name in lsmt_amd.__all__:
        obj = getattr(lsmt_amd, name)
        if inspect.isclass(obj):
            members = {m: _member(obj, m) for m in dir(obj) if not m.startswith("_")}
            out[name] = {"kind": "class", "doc": bool(obj.__doc__), "init": _params(obj), "members": members}
        else:
            out[name] = {"kind": "function", **_callable(obj)}
    return out


def _modules():
    return sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(PKG, "*.py")))


def test_exported_names_are_the_recorded_ones():
    import lsmt_amd
    want = json.load(open(FIXTURE))
    assert len(lsmt_amd.__all__) == len(set(lsmt_amd.__all__))
    assert set(lsmt_amd.__all__) == set(want)
    for name in want:
        assert hasattr(lsmt_amd, name), name


def test_signatures_properties_and_methods_are_unchanged():
    want, got = json.load(open(FIXTURE)), surface()
    for name, rec in want.items():
        now = got[name]
        assert now["kind"] == rec["kind"], name
        if rec["kind"] == "function":
            assert now["params"] == rec["params"], name
            continue
        assert now["init"] == rec["init"], name
        assert set(now["members"]) == set(rec["members"]), name
        for m, mrec in rec["members"].items():
            mnow = now["members"][m]
            assert mnow["kind"] == mrec["kind"], (name, m)
            assert mnow.get("params") == mrec.get("params"), (name, m)


def test_what_had_a_docstring_still_has_one():
    want, got = json.load(open(FIXTURE)), surface()
    for name, rec in want.items():
        assert got[name]["doc"] or not rec["doc"], name
        for m, mrec in rec.get("members", {}).items():
            assert got[name]["members"][m].get("doc") or not mrec.get("doc"), (name, m)


def test_every_module_imports_in_a_fresh_process_shard_first():
    mods = ["shard"] + [m for m in _modules() if m not in ("shard", "__init__")]
    code = "import importlib\nfor m in %r:\n    importlib.import_module('lsmt_amd.' + m)\n" % (mods,)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _taken_by_init():
    """module -> the names lsmt_amd/__init__.py imports from it."""
    tree = ast.parse(open(os.path.join(PKG, "__init__.py")).read())
    taken = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module:
            taken.setdefault(node.module, set()).update(a.name for a in node.names)
    return taken


def test_no_module_keeps_an_export_list_that_disagrees_with_the_package():
    import importlib

    import lsmt_amd
    taken = _taken_by_init()
    assert set().union(*taken.values()) >= set(lsmt_amd.__all__)
    for m in _modules():
        if m == "__init__":
            continue
        mod = importlib.import_module("lsmt_amd." + m)
        if hasattr(mod, "__all__"):
            assert set(mod.__all__) == taken.get(m, set()) & set(lsmt_amd.__all__), m
