"""A Python restatement of the tile planner (lsmt_amd/csrc/tileplan.cpp):
plan_build, plan_probe, the workspace bytes and the LDS bytes of each pass.

The reference of tests/test_tileplan_cpu.py, and where tests/test_large_m_gpu.py
takes the plan values its comments state. Written from the planner's rules, in
exact integers; it never calls the code under test.
"""
from collections import namedtuple

Plan = namedtuple("Plan", "tb T kpt C nblk sub")

MAX_TILES = 4096
BUILD_THREADS, PART_THREADS, TILE_PROBE_THREADS = 1024, 256, 512
FILTERS_PER_GROUP = 32


def _ceil_div(a, b):
    return -(-a // b)


def _ilog2(x):
    return x.bit_length() - 1


def _fit_tiles(m, tb, hi):
    while tb < hi and _ceil_div(m, 1 << tb) > MAX_TILES:
        tb += 1
    return tb


def long_runs(C, T):
    """More than ~3/4 of a wave of entries per (partition block, tile)."""
    return 2 * C > 48 * T


def plan_build(m, n, nb=1):
    nb = max(nb, 1)
    want_tiles = 1 if nb >= 256 else 256 // nb
    tb = min(max(_ilog2(m // want_tiles if m > want_tiles else 1), 12), 19)
    tb = _fit_tiles(m, tb, 19)
    T = _ceil_div(m, 1 << tb)
    kpt = 4
    while kpt > 1 and nb * _ceil_div(n, BUILD_THREADS * kpt) < 256:
        kpt //= 2
    C = BUILD_THREADS * kpt
    sub = 0
    if tb >= 17 and nb >= 8 and long_runs(C, T):  # batched builds of long runs: 16-bit entries
        if tb == 19 and long_runs(C, 2 * T) and T * 8 <= MAX_TILES:
            tb, T = 18, _ceil_div(m, 1 << 18)
        if T << (tb - 16) <= MAX_TILES:
            sub = tb - 16
    return Plan(tb, T, kpt, C, _ceil_div(n, C), sub)


def plan_probe(m, n):
    tb1 = _ilog2(m // 512 if m > 512 else 1)
    want = m * 4096 // n if n else m
    tb2 = _ilog2(want if want else 1)
    tb = _fit_tiles(m, min(max(min(tb1, tb2), 16), 18), 18)
    kpt = 8 if n >= 512 * 2048 else 4
    C = PART_THREADS * kpt
    return Plan(tb, _ceil_div(m, 1 << tb), kpt, C, _ceil_div(n, C), 0)


def plan_ok(p):
    return p.T <= MAX_TILES


# ---- workspace bytes -------------------------------------------------------------

def build_seg_bytes(p):  # a row of bins + 1 run starts (uint32) per partition block
    return ((p.T << p.sub) + 1) * p.nblk * 4


def build_ent_bytes(p):  # two entries per key, of 2 bytes with sub-tiles and 4 without
    return p.nblk * 2 * p.C * (2 if p.sub else 4)


def probe_seg_bytes(p):
    return (p.T + 1) * p.nblk * 4


def probe_ent_bytes(p):  # one uint2 per key
    return p.nblk * p.C * 8


def probe_lkey_bytes(p):  # one uint16 per key
    return p.nblk * p.C * 2


# ---- dynamic LDS bytes of each pass ------------------------------------------------

def _hist_words(bins):  # bins + 1 counts, padded to a multiple of 4 words
    return (bins + 4) & ~3


def build_part_lds(p):  # histogram, 4 words (the discards), 2 C staged entries
    return (_hist_words(p.T << p.sub) + 4) * 4 + 2 * p.C * (2 if p.sub else 4)


def build_tile_lds(p):  # the tile
    return (1 << p.tb) // 8


def probe_part_lds(p):  # histogram, C staged uint2, C staged uint16, 8 words of scan scratch
    return (_hist_words(p.T) + 2 * p.C + p.C // 2 + 8) * 4


def probe_tile_lds(p):  # two tiles, two run tables of nblk padded to 4, a word per wave, 32 pointers
    nbp = (p.nblk + 3) & ~3
    return (2 * ((1 << p.tb) // 32) + 2 * nbp + TILE_PROBE_THREADS // 64) * 4 + FILTERS_PER_GROUP * 8
