"""The host-only arithmetic behind the SSTable entries
(lsmt_amd/csrc/tablehost.hpp), checked without a GPU: the carver of
16-byte-aligned parts, the wide walk's group classification, a scan result's
layout, the flush's file bound and its staged block. The code runs in a
stand-alone driver (tests/cpp/tablehost_driver.cpp) built under the address
and undefined-behaviour sanitizers; every expectation is worked out here.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tablehost") / "tablehost_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tablehost_driver.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


def ask(driver, requests):
    """One answer line (split into words, the request's letter dropped) per request line."""
    r = subprocess.run([driver], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    return [ln.split()[1:] for ln in lines]


def up16(x):
    return (x + 15) // 16 * 16


def test_header_has_no_hip_include():
    with open(os.path.join(CSRC, "tablehost.hpp")) as fh:
        text = fh.read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text


# ---- the wide walk's groups ---------------------------------------------------------

NTS = [1, 63, 64, 65, 128, 129, 300]
BASE = 37


def scattered(n, seed):
    return [int(x) for x in np.random.default_rng(seed).permutation(n)]


def mapping(kind, nt):
    """The slots of nt tables (None: no slot list)."""
    if kind == "identity":
        return None
    if kind == "ascending":
        return [BASE + t for t in range(nt)]
    if kind == "descending":
        return [BASE + nt - 1 - t for t in range(nt)]
    if kind == "scattered":
        return scattered(nt, nt)
    if kind == "mixed":  # group 0 descending, group 1 scattered, group 2 (and later ones) ascending
        g0 = [500 + 63 - i for i in range(64)]
        g1 = [1000 + x for x in scattered(64, 5)]
        return (g0 + g1 + [2000 + i for i in range(max(0, nt - 128))])[:nt]
    if kind == "last_one":  # full descending groups, then a group of one table
        full = nt // 64 * 64
        return [BASE + full - 1 - t for t in range(full)] + [4000]
    raise AssertionError(kind)


def expect_groups(slots, nt):
    """(need_slots, [(kind, lo, gn, pad)]) by wideset's rule: ascending runs are
    kind 0 from their first slot, descending ones kind 1 from their last,
    anything else kind 2; one table alone is ascending."""
    groups, need = [], False
    for t0 in range(0, nt, 64):
        gn = min(64, nt - t0)
        s = [t0 + i if slots is None else slots[t0 + i] for i in range(gn)]
        if all(s[i] == s[0] + i for i in range(gn)):
            groups.append((0, s[0], gn, 0))
        elif all(s[i] == s[0] - i for i in range(gn)):
            groups.append((1, s[-1], gn, 0))
        else:
            groups.append((2, 0, gn, 0))
            need = True
    return need, groups


@pytest.mark.parametrize("kind", ["identity", "ascending", "descending", "scattered", "mixed", "last_one"])
def test_wide_groups(driver, kind):
    cases = [(nt, mapping(kind, nt)) for nt in NTS]
    reqs = [f"i {nt}" if s is None else "g %d %s" % (len(s), " ".join(map(str, s))) for nt, s in cases]
    for (nt, slots), ans in zip(cases, ask(driver, reqs)):
        nt = nt if slots is None else len(slots)
        need, groups = expect_groups(slots, nt)
        got = [int(x) for x in ans]
        assert got[0] == int(need) and got[1] == len(groups) == (nt + 63) // 64, (kind, nt)
        got_groups = [tuple(got[2 + 4 * g:6 + 4 * g]) for g in range(len(groups))]
        assert got_groups == groups, (kind, nt)
        # what the kernel makes of a window group is the slots themselves
        for g, (k, lo, gn, _) in enumerate(got_groups):
            s = [64 * g + i if slots is None else slots[64 * g + i] for i in range(gn)]
            if k == 0:
                assert s == [lo + i for i in range(gn)]
            elif k == 1:
                assert s == [lo + gn - 1 - i for i in range(gn)]
    if kind == "mixed":
        need, groups = expect_groups(mapping(kind, 300), 300)
        assert need and [g[0] for g in groups] == [1, 2, 0, 0, 0]
    if kind == "last_one":
        for nt in NTS:
            s = mapping(kind, nt)
            assert expect_groups(s, len(s))[1][-1] == (0, 4000, 1, 0)  # the tie-break: ascending from its slot


# ---- the carver ---------------------------------------------------------------------

TWELVE = [0, 1, 15, 16, 17, 31, 32, 33, 4096, 7, 0, 1000003]


@pytest.mark.parametrize("sizes", [[0], [1], [15], [16], [17], TWELVE], ids=lambda s: "x".join(map(str, s))[:24])
def test_carver(driver, sizes):
    (ans,) = ask(driver, ["c %d %s" % (len(sizes), " ".join(map(str, sizes)))])
    offs, total = [int(x) for x in ans[:-1]], int(ans[-1])
    assert len(offs) == len(sizes)
    assert all(o % 16 == 0 for o in offs) and offs[0] == 0
    for i in range(len(sizes) - 1):
        assert offs[i] + sizes[i] <= offs[i + 1]  # no overlap
    assert offs[-1] + sizes[-1] <= total
    assert total == sum(up16(s) for s in sizes)


# ---- a scan result's layout ---------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 2, 257])
def test_scan_layout(driver, count):
    cases = [(count, kb, vb) for kb in (0, 7, 4099) for vb in (0, 3, 65537)]
    for (c, kb, vb), ans in zip(cases, ask(driver, ["s %d %d %d" % x for x in cases])):
        parts = [(c + 1) * 8, (c + 1) * 8, c * 4, kb + 16, vb + 16]  # key_off | val_off | which | keys | vals
        want, at = [], 0
        for p in parts:
            want.append(at)
            at += up16(p)
        assert [int(x) for x in ans] == want + [at], (c, kb, vb)


# ---- the flush's file bound and staged block ----------------------------------------

FLUSHES = [(0, 0, 0), (1, 1, 0), (1, 0, 1), (3, 7, 2), (1000, 16000, 999)]


def test_flush_file_bound(driver):
    for (n, K, V), ans in zip(FLUSHES, ask(driver, ["f %d %d %d" % x for x in FLUSHES])):
        bound = int(ans[0])
        assert bound == K + 2 * n + (4 * V + 8 * n) // 3 + 17, (n, K, V)
        # it holds the file (key \t base64 \n per entry) and its 16 bytes of slack,
        # however the value bytes fall: all in one entry, or spread evenly
        for vals in ([V] + [0] * (n - 1), [V // n + (i < V % n) for i in range(n)]) if n else ():
            assert sum(vals) == V
            assert K + sum(2 + 4 * ((v + 2) // 3) for v in vals) + 16 <= bound


@pytest.mark.parametrize("mask", range(16))
def test_flush_stage_layout(driver, mask):
    reqs = ["l %d %d %d %d %d" % (mask, (n + 1) * 8, (n + 1) * 8, K, V) for n, K, V in FLUSHES]
    for (n, K, V), ans in zip(FLUSHES, ask(driver, reqs)):
        sizes = [(n + 1) * 8, (n + 1) * 8, K, V]  # key offsets | value offsets | key bytes | value bytes
        want, at = [], 0
        for i, b in enumerate(sizes):
            if mask >> i & 1:
                want.append(str(at))
                at += up16(b)
            else:
                want.append("-")
        assert ans == want + [str(at)], (mask, n, K, V)
