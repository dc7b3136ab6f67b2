"""Option "pc_pivot_wave": the 32 x 32 pivot blocks of the preconditioner's Gauss-Jordan inversions (pc_gj_invert in
csrc/nk2d_precond.hip) inverted by ONE wave in registers instead of by four waves through LDS.  The arithmetic is the same
operations in the same order, so the test is bit for bit: with the option at 1 every solution is np.array_equal to the one
with 0, on the grids of helpers.py -- the block-size classes where the index arithmetic of the wave flavours can go wrong:
fewer than 16 pivots in the block, exactly 16, 17 .. 31, exactly 32, a last panel of ONE pivot (a 1 x 1 block padded with
the identity), the next pivot block in either half of a tile at a ragged edge -- through every user of the inversion:

  pc_fused 2                    k_pc_pivot_invert<1> and k_pc_gj_step<1> at every size; also against the sparse reference
  pc_fused 0                    k_pc_gj_rows<1> ahead of the matrix-core update
  pc_valu 1                     k_pc_gj_rows<1> ahead of the VALU update
  pc_two_ended 1, pc_fused 2    the same launches with both chains in the grid's z
  pc_fp32 1 refined             the single precision storage downstream of the inversion

One engine per grid; the set-up is repeated after every option change (the pc_* options are read at the next set-up)."""
import functools

import numpy as np
import pytest
from scipy.sparse.linalg import splu

from helpers import (FORCED_MODELINFO, FORCED_SHIFT_GRIDS, FORCED_SHIFTS, IAGE_SHIFT_GRIDS, IAGE_SHIFTS, PERIODIC_BAR,
                     PERIODIC_GRIDS, SHIFT_BAR, SHIFT_TIME, YEAR, block_rhs, oracle_iage, oracle_shift_module, rel_err,
                     shifted_operator)
from oracle.model import apply_precond_stable

pytestmark = pytest.mark.gpu

DEFAULTS = {"pc_fused": 1, "pc_valu": 0, "pc_fp32": 0, "pc_refine": 1, "pc_two_ended": 0, "pc_pivot_wave": 0}
# (name, options on top of the defaults); the first one is also held to the sparse reference
VARIANTS = [
    ("fused_2", {"pc_fused": 2}),
    ("fused_0", {"pc_fused": 0}),
    ("valu", {"pc_valu": 1}),
    ("two_ended_fused_2", {"pc_two_ended": 1, "pc_fused": 2}),
    ("fp32_refined", {"pc_fp32": 1, "pc_refine": 1}),
]
LONG_ROW_GRID = (428, 5)        # of helpers.LONG_ROW_GRIDS: m = 1284, where the one-launch panel step is the default


def panel_steps(m, rounds):
    return -(-m // 32) * rounds


def walk(eng, m, ny, solve, wants, bar, case):
    """every variant on one engine with the option at 0 and at 1: `solve()` sets up again and returns the solutions (a
    list, one per reference of `wants`).  Everything is measured and printed first, then asserted."""
    got, steps, rounds, err = {}, {}, {}, None
    for name, options in VARIANTS:
        for wave in (0, 1):
            for key, value in {**DEFAULTS, **options, "pc_pivot_wave": wave}.items():
                eng.set_option(key, value)
            got[name, wave] = solve()
            steps[name, wave] = eng.counter("pc_pivot_wave_steps")
            rounds[name, wave] = eng.counter("pc_setup_rounds")
        if name == "fused_2":
            err = max(rel_err(g, w) for g, w in zip(got[name, 1], wants))
            print(f"{case} {name}, one-wave pivot blocks: {err:.2e} against the reference (bar {bar:.0e})")
        same = all(np.array_equal(x, y) for x, y in zip(got[name, 0], got[name, 1]))
        print(f"{case} {name}: {steps[name, 1]} wave steps in {rounds[name, 1]} rounds, bits {'equal' if same else 'DIFFER'}")
    for key, value in DEFAULTS.items():
        eng.set_option(key, value)
    for name, options in VARIANTS:
        assert rounds[name, 1] == rounds[name, 0] == (ny // 2 + 1 if options.get("pc_two_ended") else ny), name
        assert steps[name, 0] == 0, (name, steps[name, 0])
        assert steps[name, 1] == panel_steps(m, rounds[name, 1]), (name, steps[name, 1])
        assert all(np.array_equal(x, y) for x, y in zip(got[name, 0], got[name, 1])), name
    assert err < bar, err


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


def shifted_walk(kind, nz, ny, shifts):
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
        walk(eng, eng.tc * nz, ny, solve, wants, SHIFT_BAR, f"{kind} {nz} x {ny} (m = {eng.tc * nz}), shifts {shifts}")
    finally:
        eng.close()


def periodic_walk(nz, ny):
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    v, wants = periodic_case(nz, ny)
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(v)

    def solve():
        eng.precond_setup()
        return [eng.download(eng.precond_apply(vd)).reshape(-1)]

    try:
        walk(eng, 3 * nz, ny, solve, wants, PERIODIC_BAR, f"iage {nz} x {ny} (m = {3 * nz})")
    finally:
        eng.close()


@pytest.mark.parametrize("nz,ny", FORCED_SHIFT_GRIDS)
def test_forced_shifted_systems_bit_for_bit(nz, ny):
    shifted_walk("forced", nz, ny, FORCED_SHIFTS)


@pytest.mark.parametrize("nz,ny", IAGE_SHIFT_GRIDS)
def test_iage_shifted_systems_bit_for_bit(nz, ny):
    shifted_walk("iage", nz, ny, IAGE_SHIFTS)


@pytest.mark.parametrize("nz,ny", PERIODIC_GRIDS + [LONG_ROW_GRID])
def test_periodic_system_bit_for_bit(nz, ny):
    periodic_walk(nz, ny)


@pytest.mark.parametrize("two_ended", [0, 1])
def test_the_benchmarked_block(two_ended):
    """iage at 416 x 2: m = 1248, the block of the benchmarked grid, two rounds of 39 panel steps (one- and two-ended alike:
    ny // 2 + 1 = ny = 2) -- nk2d_precond_setup + nk2d_precond_apply under defaults and under pc_two_ended 1"""
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz, ny = 416, 2
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(block_rhs(2 * nz * ny))
    eng.set_option("pc_two_ended", two_ended)
    got, steps = {}, {}
    for wave in (0, 1):
        eng.set_option("pc_pivot_wave", wave)
        eng.precond_setup()
        steps[wave] = eng.counter("pc_pivot_wave_steps")
        assert eng.counter("pc_setup_rounds") == 2
        got[wave] = eng.download(eng.precond_apply(vd)).reshape(-1)
    eng.close()
    assert steps == {0: 0, 1: 78}, steps
    assert np.all(np.isfinite(got[0]))
    assert np.array_equal(got[0], got[1])


def test_the_option_is_read_at_set_up():
    """a factorisation made with 1 is applied after the option went back to 0, with the same result; a value of 2 is refused
    and the context stays usable"""
    from nk_ooc_amd.engine import Nk2dError, iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz, ny = 43, 3
    v, wants = periodic_case(nz, ny)
    eng = iage_engine(Grid2d.default(nz, ny))
    vd = eng.upload(v)
    assert eng.counter("pc_pivot_wave_steps") == 0
    eng.set_option("pc_fused", 2)
    eng.set_option("pc_pivot_wave", 1)
    eng.precond_setup()
    assert eng.counter("pc_pivot_wave_steps") == panel_steps(3 * nz, ny)
    before = eng.download(eng.precond_apply(vd)).reshape(-1)
    eng.set_option("pc_pivot_wave", 0)
    after = eng.download(eng.precond_apply(vd)).reshape(-1)
    assert eng.counter("pc_pivot_wave_steps") == panel_steps(3 * nz, ny)      # no set-up since: the last elimination's
    assert np.array_equal(before, after)
    with pytest.raises(Nk2dError, match="pc_pivot_wave"):
        eng.set_option("pc_pivot_wave", 2)
    eng.precond_setup()                                                       # the value is still 0
    assert eng.counter("pc_pivot_wave_steps") == 0
    again = eng.download(eng.precond_apply(vd)).reshape(-1)
    eng.close()
    assert np.array_equal(before, again)
    assert rel_err(again, wants[0]) < PERIODIC_BAR
