"""Panel width does not cost accuracy on the preconditioner's operators: a NumPy twin of the panelled Gauss-Jordan inversion
of csrc/nk2d_precond.hip (pc_gj_invert: no pivoting, one pivot after the other inside the pivot block, a rank-nb update of
everything else per panel step), with panels of 32 pivots (k_pc_gj_step) and of 64 (k_pc_gj_step64, option "pc_panel"),
takes the place of np.linalg.inv inside a copy of the elimination of helpers.block_tridiag_solve.  On every grid and shift of
helpers.py both widths are held to TWIN_BAR against the references tests/test_gpu_pc_panel64.py uses on the device: the
sparse direct solve of the shifted operators and the oracle's stable form of the time-periodic system.  Runs without the
library."""
import numpy as np
import pytest
from scipy.sparse.linalg import splu

from helpers import (FORCED_SHIFT_GRIDS, FORCED_SHIFTS, IAGE_SHIFT_GRIDS, IAGE_SHIFTS, PERIODIC_GRIDS, TWIN_BAR, block_rhs,
                     column_blocks, oracle_iage, oracle_shift_module, periodic_operator, rel_err, shifted_operator)
from oracle.model import apply_precond_stable

PANELS = (32, 64)


def invert_block(a):
    """unpivoted Gauss-Jordan inverse of a small block, pivot by pivot (pc_invert_block / pc_invert_block64)"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    for pp in range(n):
        piv = 1.0 / a[pp, pp]
        prow = a[pp].copy()
        prow[pp] = 1.0
        prow *= piv
        f = a[:, pp].copy()
        a[:, pp] = 0.0
        a -= np.outer(f, prow)
        a[pp] = prow
    return a


def panel_inverse(mat, panel):
    """the panelled in-place inversion: per step P = [p0, p0 + nb), Pinv = inverse of A[P, P], R = Pinv A[P, :] with the pivot
    columns replaced by Pinv, rows outside P: (c in P ? 0 : A[i, c]) - A[i, P] R[:, c], rows inside P: R"""
    a = np.array(mat, dtype=np.float64)
    m = a.shape[0]
    for p0 in range(0, m, panel):
        p1 = min(p0 + panel, m)
        pinv = invert_block(a[p0:p1, p0:p1])
        r = pinv @ a[p0:p1]
        r[:, p0:p1] = pinv
        f = a[:, p0:p1].copy()
        a[:, p0:p1] = 0.0
        a -= f @ r
        a[p0:p1] = r
    return a


def panel_block_tridiag_solve(mat, blocks, rhs, panel):
    """helpers.block_tridiag_solve with panel_inverse for np.linalg.inv"""
    mat = mat.tocsr()
    rows = [mat[idx] for idx in blocks]
    nb = len(blocks)
    sinv, y = [], []
    for j in range(nb):
        s = rows[j][:, blocks[j]].toarray()
        r = np.array(rhs[blocks[j]], dtype=np.float64)
        if j > 0:
            lo = rows[j][:, blocks[j - 1]]
            up = rows[j - 1][:, blocks[j]]
            s = s - lo @ (up.T @ sinv[j - 1].T).T
            r = r - lo @ (sinv[j - 1] @ y[j - 1])
        sinv.append(panel_inverse(s, panel))
        y.append(r)
    out = np.zeros(mat.shape[0])
    x_next = None
    for j in range(nb - 1, -1, -1):
        r = y[j]
        if j < nb - 1:
            r = r - rows[j][:, blocks[j + 1]] @ x_next
        x_next = sinv[j] @ r
        out[blocks[j]] = x_next
    return out


def panel_precond_apply(module, v, panel):
    """helpers.twin_precond_apply on the panelled elimination"""
    m = module.model
    n = module.tc * m.nz * m.ny
    big = periodic_operator(module)
    rhs = np.zeros(3 * n)
    rhs[:n] = v
    u = np.zeros(3 * n)
    for tr in range(module.tc):
        cells = (tr * m.nz + np.arange(m.nz)) * m.ny
        level = np.concatenate([tau * n + cells for tau in range(3)])
        u += panel_block_tridiag_solve(big, [level + j for j in range(m.ny)], rhs, panel)
    return -(u[2 * n:] + v)


def _shifted(kind, nz, ny, shifts):
    tm = oracle_shift_module(kind, nz, ny)
    v = block_rhs(tm.tc * nz * ny)
    errs = {}
    for sigma in shifts:
        op = shifted_operator(tm, sigma)
        want = splu(op).solve(v)
        for panel in PANELS:
            got = panel_block_tridiag_solve(op, column_blocks(tm.tc, nz, ny), v, panel)
            errs[sigma, panel] = rel_err(got, want)
            print(f"{kind} {nz} x {ny} (m = {tm.tc * nz}), shift {sigma}, panels of {panel}: twin against splu "
                  f"{errs[sigma, panel]:.2e}")
    for key, err in errs.items():
        assert err <= TWIN_BAR, (key, err)


@pytest.mark.parametrize("nz,ny", FORCED_SHIFT_GRIDS)
def test_panel_twin_forced_shifted_systems(nz, ny):
    _shifted("forced", nz, ny, FORCED_SHIFTS)


@pytest.mark.parametrize("nz,ny", IAGE_SHIFT_GRIDS)
def test_panel_twin_iage_shifted_systems(nz, ny):
    _shifted("iage", nz, ny, IAGE_SHIFTS)


@pytest.mark.parametrize("nz,ny", PERIODIC_GRIDS)
def test_panel_twin_periodic_system(nz, ny):
    _, tm = oracle_iage(nz, ny)
    v = block_rhs(2 * nz * ny)
    want = apply_precond_stable(tm, v)
    errs = {}
    for panel in PANELS:
        errs[panel] = rel_err(panel_precond_apply(tm, v, panel), want)
        print(f"iage {nz} x {ny} (m = {3 * nz}), panels of {panel}: twin against the oracle's stable form {errs[panel]:.2e}")
    for panel, err in errs.items():
        assert err <= TWIN_BAR, (panel, err)


@pytest.mark.parametrize("m", [1, 31, 33, 64, 65, 129])
def test_panel_inverse_is_an_inverse(m):
    """the panelled inversion against np.linalg.inv on a diagonally dominant matrix; m = 33, 65 and 129 end in a last panel
    of ONE pivot (65 and 129 under both widths), m = 1 is nothing else"""
    rng = np.random.default_rng(m)
    a = rng.standard_normal((m, m)) + (m + 2.0) * np.eye(m)
    want = np.linalg.inv(a)
    for panel in PANELS:
        assert rel_err(panel_inverse(a, panel), want) < 1e-13, panel
    # one panel that covers the matrix is the pivot-by-pivot inversion itself
    assert np.array_equal(panel_inverse(a, max(m, 1)), invert_block(a))


def test_pc_panel_is_documented():
    """an option, a counter and an environment name, no entry point: the header, the README and the engine name them"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nk2d.h")).read()
    for name in ('"pc_panel"', '"pc_panel_steps"'):
        assert name in header, name
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", header[header.index('extern "C"'):]))
    assert len(declared) == 56, len(declared)
    assert "NK2D_PC_PANEL" in open(os.path.join(root, "README.md")).read()
    assert "NK2D_PC_PANEL" in open(os.path.join(root, "newton-krylov_ooc_amd", "engine.py")).read()
