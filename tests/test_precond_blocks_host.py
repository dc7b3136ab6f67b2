"""The references of tests/test_gpu_precond_blocks.py are good enough for its bars: on every grid and shift that file uses,
the library's algorithm on the host -- a dense NumPy block-tridiagonal elimination with explicit inverses in float64
(helpers.block_tridiag_solve) -- agrees with the sparse direct solve of the same operator to 1e-10, one to two decades below
the device's bars (1e-8 for the shifted systems, 1e-9 for the time-periodic system).  A grid or a shift whose operator is too
ill-conditioned for that turns this file red before anybody reads a device error against it.  The grids and shifts are
those of helpers.py, imported by both files."""
import numpy as np
import pytest
from scipy.sparse.linalg import splu

from helpers import (FORCED_SHIFT_GRIDS, FORCED_SHIFTS, IAGE_SHIFT_GRIDS, IAGE_SHIFTS, LONG_ROW_GRIDS, PERIODIC_GRIDS,
                     TWIN_BAR, block_rhs, oracle_iage, oracle_shift_module, rel_err, shifted_operator, twin_precond_apply,
                     twin_shift_solve)
from oracle.model import apply_precond_stable


def _shifted(kind, nz, ny, shifts):
    tm = oracle_shift_module(kind, nz, ny)
    v = block_rhs(tm.tc * nz * ny)
    for sigma in shifts:
        want = splu(shifted_operator(tm, sigma)).solve(v)
        err = rel_err(twin_shift_solve(tm, sigma, v), want)
        print(f"{kind} {nz} x {ny} (m = {tm.tc * nz}), shift {sigma}: host twin against splu {err:.2e}")
        assert err <= TWIN_BAR, (sigma, err)


def _periodic(nz, ny):
    _, tm = oracle_iage(nz, ny)
    v = block_rhs(2 * nz * ny)
    err = rel_err(twin_precond_apply(tm, v), apply_precond_stable(tm, v))
    print(f"iage {nz} x {ny} (m = {3 * nz}): host twin against the oracle's stable form {err:.2e}")
    assert err <= TWIN_BAR, err


@pytest.mark.parametrize("nz,ny", FORCED_SHIFT_GRIDS)
def test_twin_forced_shifted_systems(nz, ny):
    _shifted("forced", nz, ny, FORCED_SHIFTS)


@pytest.mark.parametrize("nz,ny", IAGE_SHIFT_GRIDS)
def test_twin_iage_shifted_systems(nz, ny):
    _shifted("iage", nz, ny, IAGE_SHIFTS)


@pytest.mark.parametrize("nz,ny", PERIODIC_GRIDS)
def test_twin_periodic_system(nz, ny):
    _periodic(nz, ny)


@pytest.mark.slow
@pytest.mark.parametrize("nz,ny", LONG_ROW_GRIDS)
def test_twin_periodic_system_long_rows(nz, ny):
    _periodic(nz, ny)


def test_the_twin_is_a_block_elimination():
    """the twin against a dense solve of a small random block-tridiagonal system: unequal blocks, full couplings"""
    from scipy import sparse

    from helpers import block_tridiag_solve

    rng = np.random.default_rng(11)
    sizes = [3, 5, 2, 4]
    edges = np.concatenate(([0], np.cumsum(sizes)))
    n = edges[-1]
    dense = np.zeros((n, n))
    for j, sz in enumerate(sizes):
        a, b = edges[j], edges[j + 1]
        dense[a:b, a:b] = rng.standard_normal((sz, sz)) + 8.0 * np.eye(sz)
        if j > 0:
            dense[a:b, edges[j - 1]:a] = rng.standard_normal((sz, sizes[j - 1]))
            dense[edges[j - 1]:a, a:b] = rng.standard_normal((sizes[j - 1], sz))
    rhs = rng.standard_normal(n)
    # blocks in a scrambled numbering, as the ypos columns are inside a state vector
    perm = rng.permutation(n)
    scrambled = np.zeros((n, n))
    scrambled[np.ix_(perm, perm)] = dense
    rhs_s = np.zeros(n)
    rhs_s[perm] = rhs
    blocks = [perm[edges[j]:edges[j + 1]] for j in range(len(sizes))]
    got = block_tridiag_solve(sparse.csr_matrix(scrambled), blocks, rhs_s)
    assert rel_err(got, np.linalg.solve(scrambled, rhs_s)) < 1e-13
