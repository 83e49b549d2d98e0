"""The tile planner (lsmt_amd/csrc/tileplan.cpp) on the CPU, under sanitizers.

plan_build / plan_probe decide tile size, grid sizes, workspace and LDS bytes
and which kernel instantiation a tiled pass runs. The planner has no device
code in it, so a small stand-alone driver (tests/cpp/tileplan_driver.cpp) is
compiled together with tileplan.cpp with -fsanitize=address,undefined and run
as a child process: nothing is preloaded and nothing is loaded into Python.

Three checks over one run of the driver:
  (a) every field, byte count and flag equals the Python restatement
      (tests/tileplan_ref.py) on a grid of (m, n, nb);
  (b) plans worked by hand, as literals: the probe plans
      tests/test_large_m_gpu.py states for its cases, and build plans for C2,
      C4 and the three shapes of test_batched_long_run_builds;
  (c) on every grid point, the invariants the launchers and capi_filter.cpp's
      `covers` refuse a plan for at run time.
"""
import os
import subprocess
from collections import namedtuple

import pytest

import tileplan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsmt_amd", "csrc")
LDS_PER_CU = 163_840  # MI355X: 160 KiB of LDS per CU

MS = [1, 4095, 4096, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, 1 << 20, (1 << 20) + 5, 1 << 22, 3 << 23, 1 << 25,
      1 << 26, (1 << 27) + 12345, 1 << 30, (1 << 30) + 1, 1 << 31, (1 << 31) + 1, 1 << 32, 1 << 33]
NS = [1, 255, 1024, 4096, 4097, 1 << 15, 70_001, 1 << 18, 380_000, 1 << 20, 512 * 2048 - 1, 512 * 2048, 1 << 23,
      1 << 24]
NBS = [1, 7, 8, 12, 32, 64, 255, 256, 300]
GRID = [("b", m, n, nb) for m in MS for n in NS for nb in NBS] + [("p", m, n, 1) for m in MS for n in NS]

K20 = 1 << 20
# (tb, T, kpt, partition blocks): the plans test_large_m_gpu.py's cases state
PROBE_PINS = {
    (1 << 27, 100_000): (18, 512, 4, 98),            # P1, P6
    ((1 << 27) + 12345, 70_001): (18, 513, 4, 69),   # P2
    ((1 << 26) + 9, K20 + 777): (17, 513, 8, 513),   # P3
    (1 << 27, 3_000_000): (17, 1024, 8, 1465),       # P4
    (1 << 20, 70_001): (16, 16, 4, 69),              # P5
    ((1 << 20) + 5, 70_001): (16, 17, 4, 69),        # P5_mixed
    (1 << 20, 212_000): (16, 16, 4, 208),            # P7
    (1 << 27, 212_000): (18, 512, 4, 208),           # P7
    (1 << 30, 70_001): (18, 4096, 4, 69),            # P8, B1
    ((1 << 28) + 7, 70_001): (18, 1025, 4, 69),      # B1
}
# (m, n, nb) -> (tb, T, kpt, C, nblk, sub), worked by hand from plan_build
BUILD_PINS = {
    (1 << 27, 1 << 20, 1): (19, 256, 4, 4096, 256, 0),   # C2
    (1 << 25, 1 << 18, 32): (18, 128, 4, 4096, 64, 2),   # C4
    (1 << 22, 380_000, 12): (17, 32, 4, 4096, 93, 1),    # test_batched_long_run_builds
    (3 << 23, 380_000, 12): (18, 96, 4, 4096, 93, 2),
    (1 << 26, 380_000, 12): (19, 128, 4, 4096, 93, 3),
}
PINS = [("p", m, n, 1) for m, n in PROBE_PINS] + [("b", m, n, nb) for m, n, nb in BUILD_PINS]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tileplan") / "tileplan_driver")
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tileplan_driver.cpp"),
           os.path.join(CSRC, "tileplan.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return out


Row = namedtuple("Row", "plan ok seg ent lkey lds_part lds_tile long_runs")


@pytest.fixture(scope="module")
def planned(driver):
    """{(kind, m, n, nb): Row} of the real planner, over the grid and the pins."""
    points = list(dict.fromkeys(GRID + PINS))
    stdin = "".join(f"{k} {m} {n} {nb}\n" for k, m, n, nb in points)
    r = subprocess.run([driver], input=stdin, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(points)
    out = {}
    for pt, ln in zip(points, lines):
        f = ln.split()
        assert f[0] == pt[0], ln
        v = [int(x) for x in f[1:]]
        out[pt] = Row(ref.Plan(*v[:6]), bool(v[6]), *v[7:12], bool(v[12]))
    return out


def _ref_row(kind, m, n, nb):
    if kind == "b":
        p = ref.plan_build(m, n, nb)
        return Row(p, ref.plan_ok(p), ref.build_seg_bytes(p), ref.build_ent_bytes(p), 0, ref.build_part_lds(p),
                   ref.build_tile_lds(p), ref.long_runs(p.C, p.T))
    p = ref.plan_probe(m, n)
    return Row(p, ref.plan_ok(p), ref.probe_seg_bytes(p), ref.probe_ent_bytes(p), ref.probe_lkey_bytes(p),
               ref.probe_part_lds(p), ref.probe_tile_lds(p), ref.long_runs(p.C, p.T))


def test_planner_matches_the_restatement_on_the_grid(planned):
    assert len(GRID) == len(MS) * len(NS) * (len(NBS) + 1)
    for pt in GRID:
        assert planned[pt] == _ref_row(*pt), pt


def test_pinned_plans(planned):
    for (m, n), want in PROBE_PINS.items():
        p = planned[("p", m, n, 1)].plan
        assert (p.tb, p.T, p.kpt, p.nblk) == want, (m, n)
    for (m, n, nb), want in BUILD_PINS.items():
        assert tuple(planned[("b", m, n, nb)].plan) == want, (m, n, nb)


def test_plan_invariants_on_the_grid(planned):
    for pt in GRID:
        kind, m, n, _ = pt
        row = planned[pt]
        p = row.plan
        assert row.ok == (p.T <= 4096), pt
        if not row.ok:
            continue
        assert ((p.T - 1) << p.tb) < m <= (p.T << p.tb), pt
        if kind == "b":
            assert 12 <= p.tb <= 19 and p.kpt in (1, 2, 4) and p.C == 1024 * p.kpt, pt
            assert p.sub in (0, 1, 2, 3), pt
            if p.sub:
                assert p.tb == 16 + p.sub and (p.T << p.sub) <= 4096, pt
            assert row.seg == ((p.T << p.sub) + 1) * p.nblk * 4, pt
            assert row.ent == p.nblk * 2 * p.C * (2 if p.sub else 4), pt
            assert row.lkey == 0, pt
        else:
            assert 16 <= p.tb <= 18 and p.kpt in (4, 8) and p.C == 256 * p.kpt and p.sub == 0, pt
            assert row.seg == (p.T + 1) * p.nblk * 4, pt
            assert row.ent == p.nblk * p.C * 8, pt
            assert row.lkey == p.nblk * p.C * 2, pt
        assert p.nblk == -(-n // p.C), pt
        assert row.lds_part <= LDS_PER_CU and row.lds_tile <= LDS_PER_CU, pt
