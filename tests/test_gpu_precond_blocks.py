"""The preconditioner's dense kernels (csrc/nk2d_precond.hip) at every block-size class.  They are written around fixed
tiles -- Gauss-Jordan panels of 32 pivots, rank-32 updates on 64 x 64 tiles, the next pivot block inverted inside whichever
tile holds it, mat-vec rows staged in chunks of 1280 columns, a wide mat-vec for even and a general one for odd block sizes
-- and the other tests meet them at m = 3 nz in {60, 63, 78, 210, 390, 1248} only.  Here the block size is walked through
the classes where such index arithmetic goes wrong:

  group 1  shifted systems (nk2d_shift_factor / nk2d_shift_solve) of a one-tracer forced module, m = nz: a single partial
           panel (2, 3, 16, 31), a single tile (33, 63), full panels and exact tiles (32, 64, 96, 128, 160), a last panel of
           ONE pivot (33, 65, 97, 129, 193), the next pivot block in either half of a tile at a ragged edge, odd m
  group 2  shifted systems of iage, m = 2 nz (two tracers in a block)
  group 3  the time-periodic system of iage (nk2d_precond_setup / nk2d_precond_apply), m = 3 nz = 6 .. 258
  group 4  the same with rows LONGER than one mat-vec chunk: m = 1281 (odd), 1284, 1536 (the largest block the library takes)

against sparse direct solves of the same operators built from the oracle's Jacobian in float64 (shifted systems: splu of
YEAR J(YEAR / 2) - sigma I, bar 1e-8 as test_phosphorus_preconditioner; time-periodic system: oracle.model.
apply_precond_stable, bar 1e-9 as test_precond_apply).  tests/test_precond_blocks_host.py asserts on the CPU that the
library's algorithm in NumPy agrees with these references to 1e-10 on every grid and shift used here (the iage shifts kept
after that run: 0.02 and 0.5).  The grids and shifts are helpers.py's, shared by both files.

One engine per grid walks the option matrix (the pc_* options are read at the next set-up; the set-up is repeated after
every change and "pc_setup_rounds" says whether one or two chains ran):

  A  defaults                                        against the reference
  B  pc_fused 2 (one-launch panel steps)             against the reference; the bits of C
  C  pc_fused 0 (two launches, fp64 MFMA update)     against the reference
  D  pc_valu 1 (round-1 VALU update, general mat-vec at every m)   against the reference
  E  pc_two_ended 1 with pc_fused 2 and 0            against the reference; the two bit for bit equal; ny // 2 + 1 rounds
  F  pc_fp32 1 with pc_refine 1, one- and two-ended  against the reference at the same bar

(No variant is dropped anywhere: D at 428 x 5 takes well under a second.)  A run of the WHOLE file writes the largest error of
every group and variant to profiles/precond_blocks_margins.json (a run of some of its cases leaves that file alone)."""
import functools
import json
import os

import numpy as np
import pytest
from scipy.sparse.linalg import splu

from helpers import (FORCED_MODELINFO, FORCED_SHIFT_GRIDS, FORCED_SHIFTS, IAGE_SHIFT_GRIDS, IAGE_SHIFTS, LONG_ROW_GRIDS,
                     PERIODIC_BAR, PERIODIC_GRIDS, SHIFT_BAR, SHIFT_TIME, YEAR, block_rhs, oracle_iage, oracle_shift_module,
                     rel_err, shifted_operator)
from oracle.model import apply_precond_stable

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "precond_blocks_margins.json")

DEFAULTS = {"pc_fused": 1, "pc_valu": 0, "pc_fp32": 0, "pc_refine": 1, "pc_two_ended": 0}
# (name, options on top of the defaults)
VARIANTS = [
    ("A_defaults", {}),
    ("B_fused_2", {"pc_fused": 2}),
    ("C_fused_0", {"pc_fused": 0}),
    ("D_valu", {"pc_valu": 1}),
    ("E_two_ended_fused_2", {"pc_two_ended": 1, "pc_fused": 2}),
    ("E_two_ended_fused_0", {"pc_two_ended": 1, "pc_fused": 0}),
    ("F_fp32_refined", {"pc_fp32": 1, "pc_refine": 1}),
    ("F_fp32_refined_two_ended", {"pc_fp32": 1, "pc_refine": 1, "pc_two_ended": 1}),
]
SAME_BITS = [("B_fused_2", "C_fused_0"), ("E_two_ended_fused_2", "E_two_ended_fused_0")]

_largest = {}
_cases_run = set()
N_CASES = len(FORCED_SHIFT_GRIDS) + len(IAGE_SHIFT_GRIDS) + len(PERIODIC_GRIDS) + len(LONG_ROW_GRIDS)


@pytest.fixture(scope="module", autouse=True)
def margins_file():
    """the largest error per group and variant, written once at the end of a run of every case of this file"""
    yield
    if len(_cases_run) == N_CASES:
        try:
            with open(MARGINS, "w") as f:
                json.dump(_largest, f, indent=1, sort_keys=True)
        except OSError as exc:      # a read-only tree: the figures were printed case by case
            print(f"{MARGINS} not written: {exc}")


def _note(group, bar, name, err, case):
    _cases_run.add(case)
    _largest[f"{group}.bar"] = bar
    key = f"{group}.{name}"
    if err >= _largest.get(key, -1.0):
        _largest[key] = err
        _largest[key + ".at"] = case


def walk(eng, ny, solve, wants, group, bar, case):
    """every variant of the option matrix on one engine: `solve()` sets up again and returns the solutions (a list, one per
    reference of `wants`).  Everything is measured and printed first, then asserted."""
    got, rounds, errs = {}, {}, {}
    for name, options in VARIANTS:
        for key, value in {**DEFAULTS, **options}.items():
            eng.set_option(key, value)
        got[name] = solve()
        rounds[name] = eng.counter("pc_setup_rounds")
        errs[name] = max(rel_err(g, w) for g, w in zip(got[name], wants))
        print(f"{case} {name}: {errs[name]:.2e} against the reference (bar {bar:.0e}), {rounds[name]} rounds")
        _note(group, bar, name, errs[name], case)
    for key, value in DEFAULTS.items():
        eng.set_option(key, value)
    for name, options in VARIANTS:
        assert rounds[name] == (ny // 2 + 1 if options.get("pc_two_ended") else ny), (name, rounds[name])
        assert errs[name] < bar, (name, errs[name])
    for a, b in SAME_BITS:
        assert all(np.array_equal(x, y) for x, y in zip(got[a], got[b])), (a, b)


@functools.lru_cache(maxsize=None)
def shifted_case(kind, nz, ny, shifts):
    """a right-hand side and the sparse direct solves of it, computed once per grid (read-only)"""
    tm = oracle_shift_module(kind, nz, ny)
    v = block_rhs(tm.tc * nz * ny)
    wants = [splu(shifted_operator(tm, sigma)).solve(v) for sigma in shifts]
    for w in wants:
        w.setflags(write=False)
    return v, wants


@functools.lru_cache(maxsize=None)
def periodic_case(nz, ny):
    _, tm = oracle_iage(nz, ny)
    v = block_rhs(2 * nz * ny)
    want = apply_precond_stable(tm, v)
    want.setflags(write=False)
    return v, [want]


def shifted_walk(kind, nz, ny, shifts, group):
    from nk_ooc_amd.engine import forced_engine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    v, wants = shifted_case(kind, nz, ny, tuple(shifts))
    grid = Grid2d.default(nz, ny)
    eng = forced_engine(grid, FORCED_MODELINFO) if kind == "forced" else iage_engine(grid)
    vd = eng.upload(v)

    def solve():
        eng.shift_factor(SHIFT_TIME, YEAR, shifts)
        return [eng.download(eng.shift_solve(i, vd)).reshape(-1) for i in range(len(shifts))]

    try:
        walk(eng, ny, solve, wants, group, SHIFT_BAR, f"{kind} {nz} x {ny} (m = {eng.tc * nz}), shifts {shifts}")
    finally:
        eng.close()


def periodic_walk(nz, ny, group):
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    v, wants = periodic_case(nz, ny)
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(v)

    def solve():
        eng.precond_setup()
        return [eng.download(eng.precond_apply(vd)).reshape(-1)]

    try:
        walk(eng, ny, solve, wants, group, PERIODIC_BAR, f"iage {nz} x {ny} (m = {3 * nz})")
    finally:
        eng.close()


@pytest.mark.parametrize("nz,ny", FORCED_SHIFT_GRIDS)
def test_forced_shifted_systems(nz, ny):
    shifted_walk("forced", nz, ny, FORCED_SHIFTS, "group1_forced_shifted_m_nz")


@pytest.mark.parametrize("nz,ny", IAGE_SHIFT_GRIDS)
def test_iage_shifted_systems(nz, ny):
    shifted_walk("iage", nz, ny, IAGE_SHIFTS, "group2_iage_shifted_m_2nz")


@pytest.mark.parametrize("nz,ny", PERIODIC_GRIDS)
def test_periodic_system(nz, ny):
    periodic_walk(nz, ny, "group3_iage_periodic_m_3nz")


@pytest.mark.parametrize("nz,ny", LONG_ROW_GRIDS)
def test_periodic_system_long_rows(nz, ny):
    periodic_walk(nz, ny, "group4_iage_periodic_long_rows")
