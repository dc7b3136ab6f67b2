"""Option "pc_panel" 64: the Gauss-Jordan inversions of the preconditioner's set-up (pc_gj_invert in csrc/nk2d_precond.hip)
in panel steps of 64 pivots -- k_pc_pivot_invert64 and k_pc_gj_step64 -- instead of 32.  The pivots are taken one by one in
the same order, but the updates between them are grouped differently, so the results differ from option 32 in rounding and
the test is against the sparse references of tests/test_gpu_precond_blocks.py, at that file's bars (SHIFT_BAR 1e-8,
PERIODIC_BAR 1e-9: tests/test_pc_panel64_host.py holds a NumPy twin of both panel widths to 1e-10 against the same
references), on the grids of helpers.py -- every block-size class of the 64-wide step: m < 64 (one partial panel in one
tile), m = 64, a last panel of ONE pivot (65, 129, 193), of 32 or 33 (96, 97, 160), of 2 and 4 (66, 258, 1284), full last
panels (128, 192) -- through

  A_defaults          k_pc_gj_step64 at every size (pc_fused 1 would take the 32-wide one-launch step from m = 1024 only)
  B_two_ended         the same launches with both chains in the grid's z
  C_fp32_refined      the single precision storage downstream of the inversion
  D_fused_0           pc_fused is not consulted: the bits of A_defaults

with the counters pc_panel_steps == ceil(m / 64) * pc_setup_rounds and pc_pivot_wave_steps == 0.  The relative difference
between the 64 and the 32 solutions of the same engine is printed, not asserted (it is rounding; no bound for it follows
from the references).  One engine per grid; everything is measured and printed first, then asserted; a run of every case
writes the largest errors to profiles/pc_panel64_margins.json (a run of some of the cases leaves that file alone)."""
import functools
import json
import os

import numpy as np
import pytest
from scipy.sparse import identity
from scipy.sparse.linalg import splu, spsolve

from helpers import (FORCED_MODELINFO, FORCED_SHIFT_GRIDS, FORCED_SHIFTS, IAGE_SHIFT_GRIDS, IAGE_SHIFTS, PERIODIC_BAR,
                     PERIODIC_GRIDS, SHIFT_BAR, SHIFT_TIME, YEAR, block_rhs, oracle_iage, oracle_shift_module, rel_err,
                     shifted_operator)
from oracle.model import apply_precond_stable

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "pc_panel64_margins.json")

DEFAULTS = {"pc_fused": 1, "pc_valu": 0, "pc_fp32": 0, "pc_refine": 1, "pc_two_ended": 0, "pc_pivot_wave": 0, "pc_panel": 32}
# (name, options on top of the defaults and of pc_panel 64)
VARIANTS = [
    ("A_defaults", {}),
    ("B_two_ended", {"pc_two_ended": 1}),
    ("C_fp32_refined", {"pc_fp32": 1, "pc_refine": 1}),
    ("D_fused_0", {"pc_fused": 0}),
]
LONG_ROW_GRID = (428, 5)        # of helpers.LONG_ROW_GRIDS: m = 1284 = 20 * 64 + 4

_largest = {}
_cases_run = set()
N_CASES = len(FORCED_SHIFT_GRIDS) + len(IAGE_SHIFT_GRIDS) + len(PERIODIC_GRIDS) + 1 + 2 + 1


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


def panel_steps(m, rounds):
    return -(-m // 64) * rounds


def set_options(eng, options):
    for key, value in {**DEFAULTS, **options}.items():
        eng.set_option(key, value)


def walk(eng, m, ny, solve, wants, group, bar, case):
    """option 32 under the defaults, then every variant with 64, on one engine: `solve()` sets up again and returns the
    solutions (a list, one per reference of `wants`)"""
    set_options(eng, {})
    got32 = solve()
    err32 = max(rel_err(g, w) for g, w in zip(got32, wants))
    steps32 = eng.counter("pc_panel_steps")
    print(f"{case} option 32: {err32:.2e} against the reference (bar {bar:.0e}), pc_panel_steps {steps32}")
    got, steps, wave_steps, rounds, errs = {}, {}, {}, {}, {}
    for name, options in VARIANTS:
        set_options(eng, {**options, "pc_panel": 64})
        got[name] = solve()
        steps[name] = eng.counter("pc_panel_steps")
        wave_steps[name] = eng.counter("pc_pivot_wave_steps")
        rounds[name] = eng.counter("pc_setup_rounds")
        errs[name] = max(rel_err(g, w) for g, w in zip(got[name], wants))
        diff = max(rel_err(g, h) for g, h in zip(got[name], got32))
        print(f"{case} {name}, panels of 64: {errs[name]:.2e} against the reference (bar {bar:.0e}), {diff:.2e} from option "
              f"32; {steps[name]} steps in {rounds[name]} rounds")
        _note(group, bar, name, errs[name], case)
    set_options(eng, {})
    assert steps32 == 0, steps32
    for name, options in VARIANTS:
        assert rounds[name] == (ny // 2 + 1 if options.get("pc_two_ended") else ny), (name, rounds[name])
        assert steps[name] == panel_steps(m, rounds[name]), (name, steps[name])
        assert wave_steps[name] == 0, (name, wave_steps[name])
        assert all(np.all(np.isfinite(g)) for g in got[name]), name
        assert errs[name] < bar, (name, errs[name])
    assert all(np.array_equal(x, y) for x, y in zip(got["A_defaults"], got["D_fused_0"]))


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
        walk(eng, eng.tc * nz, ny, solve, wants, group, SHIFT_BAR, f"{kind} {nz} x {ny} (m = {eng.tc * nz}), shifts {shifts}")
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
        walk(eng, 3 * nz, ny, solve, wants, group, PERIODIC_BAR, f"iage {nz} x {ny} (m = {3 * nz})")
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


def test_periodic_system_long_rows():
    periodic_walk(*LONG_ROW_GRID, "group4_iage_periodic_long_rows")


@pytest.mark.parametrize("two_ended", [0, 1])
def test_the_benchmarked_block(two_ended):
    """iage at 416 x 2: m = 1248 = 19 * 64 + 32, the block of the benchmarked grid, two rounds of 20 panel steps (one- and
    two-ended alike: ny // 2 + 1 = ny = 2).  The reference is the oracle's stable form itself, apply_precond_stable (a sparse
    solve of 5000 unknowns, well under a second), at PERIODIC_BAR -- not the option-32 apply"""
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz, ny = 416, 2
    v, wants = periodic_case(nz, ny)
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(v)
    eng.set_option("pc_two_ended", two_ended)
    got, steps, rounds = {}, {}, {}
    for panel in (32, 64):
        eng.set_option("pc_panel", panel)
        eng.precond_setup()
        steps[panel] = eng.counter("pc_panel_steps")
        rounds[panel] = eng.counter("pc_setup_rounds")
        got[panel] = eng.download(eng.precond_apply(vd)).reshape(-1)
    eng.close()
    case = f"iage {nz} x {ny} (m = {3 * nz}), pc_two_ended {two_ended}"
    errs = {panel: rel_err(got[panel], wants[0]) for panel in (32, 64)}
    print(f"{case}: panels of 64 {errs[64]:.2e}, of 32 {errs[32]:.2e} against the reference (bar {PERIODIC_BAR:.0e}), "
          f"{rel_err(got[64], got[32]):.2e} between them; {steps[64]} steps in {rounds[64]} rounds")
    _note("benchmarked_block_iage_416x2", PERIODIC_BAR, f"two_ended_{two_ended}", errs[64], case)
    assert rounds == {32: 2, 64: 2}, rounds
    assert steps == {32: 0, 64: 40}, steps
    assert np.all(np.isfinite(got[64]))
    assert errs[64] < PERIODIC_BAR, errs[64]


def test_the_option_is_read_at_set_up_and_the_refusals():
    """a factorisation made with 64 is applied after the option went back to 32, with the same bits; the next set-up is the
    32-wide one again; a value other than 32 or 64 is refused and leaves the value alone; a set-up with 64 and pc_valu 1 or
    pc_pivot_wave 1 is refused with both names in the message, and the context stays usable"""
    from nk_ooc_amd.engine import Nk2dError, iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz, ny = 43, 3
    m = 3 * nz
    v, wants = periodic_case(nz, ny)
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(v)

    def apply():
        return eng.download(eng.precond_apply(vd)).reshape(-1)

    try:
        assert eng.counter("pc_panel_steps") == 0
        eng.precond_setup()                                       # the engine's first set-up: option 32
        fresh32 = apply()
        assert eng.counter("pc_panel_steps") == 0
        eng.set_option("pc_panel", 64)
        eng.precond_setup()
        assert eng.counter("pc_panel_steps") == panel_steps(m, ny)
        before = apply()
        eng.set_option("pc_panel", 32)
        after = apply()
        assert eng.counter("pc_panel_steps") == panel_steps(m, ny)    # no set-up since: the last elimination's
        assert np.array_equal(before, after)
        assert rel_err(before, wants[0]) < PERIODIC_BAR
        eng.precond_setup()
        assert eng.counter("pc_panel_steps") == 0
        assert np.array_equal(apply(), fresh32)
        with pytest.raises(Nk2dError, match="pc_panel"):
            eng.set_option("pc_panel", 48)
        eng.precond_setup()                                       # the value is still 32
        assert eng.counter("pc_panel_steps") == 0
        assert np.array_equal(apply(), fresh32)
        for other in ("pc_valu", "pc_pivot_wave"):
            eng.set_option("pc_panel", 64)
            eng.set_option(other, 1)
            with pytest.raises(Nk2dError, match="pc_panel") as exc:
                eng.precond_setup()
            assert other in str(exc.value), str(exc.value)
            set_options(eng, {})
            eng.precond_setup()
            err = rel_err(apply(), wants[0])
            print(f"iage {nz} x {ny}: a default set-up after the refusal of pc_panel 64 with {other} 1: {err:.2e}")
            assert err < PERIODIC_BAR, (other, err)
    finally:
        eng.close()


def test_phosphorus_shifted_systems(golden_dir):
    """the shifted systems of the 22 x 9 phosphorus case as tests/test_gpu_phosphorus.py builds them (m = 66: one full panel
    and a last panel of two pivots, indefinite matrices), against that test's reference at its bar"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d
    from oracle.grid import default_axes
    from oracle.model import Phosphorus, Py2dModel, phosphorus_precond_matrix

    g = np.load(f"{golden_dir}/phosphorus_22x9.npz")
    nz, ny = int(g["nz"]), int(g["ny"])
    depth, ypos = default_axes(nz, ny)
    tm = Phosphorus(Py2dModel(depth, ypos))
    po4 = g["y"].reshape(3, nz, ny)[0]
    mat = phosphorus_precond_matrix(tm, po4)
    n = mat.shape[0]
    v = np.random.default_rng(21).standard_normal(n)
    shifts = [0.02, -0.03]
    wants = [spsolve((mat - sigma * identity(n, format="csc")).tocsc(), v) for sigma in shifts]
    eng = phosphorus_engine(Grid2d.default(nz, ny))
    try:
        ylin = np.zeros((3, nz, ny))
        ylin[0] = po4
        eng.set_lin_state(eng.upload(ylin))
        vd = eng.upload(v)
        got, steps = {}, {}
        for panel in (32, 64):
            eng.set_option("pc_panel", panel)
            eng.shift_factor(0.5 * YEAR, YEAR, shifts)
            steps[panel] = eng.counter("pc_panel_steps")
            got[panel] = [eng.download(eng.shift_solve(i, vd)).reshape(-1) for i in range(2)]
    finally:
        eng.close()
    case = f"phosphorus {nz} x {ny} (m = {3 * nz}), shifts {shifts}"
    errs = {panel: max(rel_err(x, w) for x, w in zip(got[panel], wants)) for panel in (32, 64)}
    diff = max(rel_err(x, y) for x, y in zip(got[64], got[32]))
    print(f"{case}: panels of 64 {errs[64]:.2e}, of 32 {errs[32]:.2e} against the reference (bar {SHIFT_BAR:.0e}), {diff:.2e} "
          f"between them; {steps[64]} steps")
    _note("phosphorus_22x9_shifted_m_66", SHIFT_BAR, "A_defaults", errs[64], case)
    assert steps == {32: 0, 64: 2 * ny}, steps
    assert errs[64] < SHIFT_BAR, errs[64]
