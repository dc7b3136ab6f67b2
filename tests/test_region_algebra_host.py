"""The reference of tests/test_gpu_region_algebra.py is good enough for its bars.  helpers.algebra_reference -- plain NumPy
element-wise operations in the kernels' documented order, dots in exact rational arithmetic -- is held to the oracle
(oracle.krylov, itself pinned to the reference's functions): bit for bit element-wise, within the derived bound
(N_r + 3) 2**-53 S_r for the dots.  And the inputs of the device test are such that the bound means something: on every
grid, tracer count and region layout that file uses, the smallest |term| of every regional dot is at least 100 times the
region's bound, so that one dropped, doubled or misplaced cell cannot hide inside it.  Grids, regions and inputs are
those of helpers.py, imported by both files."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import (ALGEBRA_GRIDS, ALGEBRA_HOST_SHAPES, ALGEBRA_MGS_EDGE, ALGEBRA_N_EDGE, ALGEBRA_NVEC,
                     ALGEBRA_REDUCE_SHAPES, ALGEBRA_TC, U53, algebra_coefs, algebra_reference, algebra_vectors, oracle_iage,
                     region_cases)
from oracle import krylov

CASES = ("depth_split", "patchwork", "sparse_regions", "columns")
DEVICE_SHAPES = ([(tc, nz, ny) for nz, ny in ALGEBRA_GRIDS for tc in ALGEBRA_TC] + ALGEBRA_REDUCE_SHAPES
                 + [ALGEBRA_MGS_EDGE, ALGEBRA_N_EDGE])


@pytest.mark.parametrize("nz,ny,tc", ALGEBRA_HOST_SHAPES)
def test_reference_against_the_oracle(nz, ny, tc):
    _, tm = oracle_iage(nz, ny)
    assert tm.tc == tc
    vecs = algebra_vectors(tc, nz, ny)
    a, b = vecs[0], vecs[1]
    for name, reg in region_cases(nz, ny).items():
        mod = krylov.OracleModule(tm, reg)
        ref = algebra_reference(reg, tc)
        # the normalised weights are the rows of the oracle's region mean matrix
        for r in range(reg.nreg):
            row = reg.mean_matrix[[r], :].toarray().reshape(-1)
            assert np.array_equal(np.where(ref.mask == r + 1, ref.wn, 0.0), row), (name, r)
        c1, c2 = algebra_coefs(reg.nreg, 2)
        assert np.array_equal(ref.scale(a, c1), mod.scale(a, c1)), name
        assert np.array_equal(ref.axpby(c1, a, c2, b), mod.scale(a, c1) + mod.scale(b, c2)), name
        assert np.array_equal(ref.diff_scale(a, b, c1), mod.scale(a - b, c1)), name
        assert np.array_equal(ref.mask_out(a), mod.mask_out(a)), name
        for n in (1, 2, 5):
            cf = algebra_coefs(reg.nreg, n)
            want = krylov.lin_comb([mod], cf[None], [[v] for v in vecs[1:n + 1]])[0]
            assert np.array_equal(ref.lin_comb(cf, vecs[1:n + 1]), want), (name, n)
        # the projections of mod_gram_schmidt with the oracle's own coefficients
        h_or, w_or = krylov.mod_gram_schmidt([mod], [a], [[v] for v in vecs[1:5]])
        assert np.array_equal(ref.multi_axpy(a, vecs[1:5], h_or[0], 1.0), w_or[0]), name
        # the oracle's dots (CSR rows summed in index order, tracer after tracer) are one order of the same terms
        for v in vecs[1:]:
            dref = ref.dot(a, v)
            excess = ref.dot_excess(mod.dot(a, v), dref)
            assert excess <= 1.0, (name, excess)
            assert np.array_equal(dref[2], tc * np.array([np.count_nonzero(reg.mask == r + 1) for r in range(reg.nreg)]))
        # ... and with them the two Gram-Schmidt agree as far as the propagated bound says
        h, w, hbound = ref.mgs(a, vecs[1:5])
        assert (np.abs(h - h_or[0]) <= hbound).all(), name
        assert np.max(np.abs(w - w_or[0])) <= 1e-12 * np.max(np.abs(w_or[0])), name


def test_exact_dot_is_exact():
    """the integer mantissa arithmetic of the dots against fractions.Fraction term by term, and the bound's anatomy: a
    float64 sum in index order lies inside it, the same sum with one term left out does not"""
    nz, ny, tc = 20, 3, 2
    vecs = algebra_vectors(tc, nz, ny)
    for name, reg in region_cases(nz, ny).items():
        ref = algebra_reference(reg, tc)
        exact, s, n = ref.dot(vecs[0], vecs[1])
        wn, mask = np.tile(ref.wn, tc), np.tile(ref.mask, tc)
        for r in range(reg.nreg):
            idx = np.nonzero(mask == r + 1)[0]
            terms = [Fraction(float(wn[i])) * Fraction(float(vecs[0][i])) * Fraction(float(vecs[1][i])) for i in idx]
            assert sum(terms) == exact[r] and sum(abs(t) for t in terms) == s[r] and len(terms) == n[r], (name, r)
        prod = wn * (vecs[0] * vecs[1])
        naive = np.array([np.cumsum(prod[mask == r + 1])[-1] for r in range(reg.nreg)])
        assert ref.dot_excess(naive, (exact, s, n)) <= 1.0, name
        for r in range(reg.nreg):
            idx = np.nonzero(mask == r + 1)[0]
            short = naive.copy()
            short[r] = np.sum(prod[idx[1:]]) if len(idx) > 1 else 0.0
            assert ref.dot_excess(short, (exact, s, n)) > 50.0, (name, r)


@pytest.mark.parametrize("nz,ny", sorted({(nz, ny) for _, nz, ny in DEVICE_SHAPES}))
def test_region_cases_are_what_they_say(nz, ny):
    cases = region_cases(nz, ny)
    assert tuple(cases) == CASES
    e = (nz + 63) // 64
    for name, reg in cases.items():
        assert reg.mask.shape == reg.weight.shape == (nz, ny)
        assert ((reg.mask == 0) == (reg.weight == 0.0)).all() and reg.mask.min() >= 0
        assert set(np.unique(reg.mask[reg.mask > 0])) == set(range(1, reg.nreg + 1)), name
    split = cases["depth_split"].mask
    assert cases["depth_split"].nreg == 3 and (np.diff(split, axis=0) >= 0).all()
    if nz > 2:
        first = np.array([[np.argmax(split[:, j] == r) for j in range(ny)] for r in (2, 3)])    # boundary levels
        assert (first % 64 != 0).all() and (e == 1 or (first % e != 0).all())
        assert (first[0, 1:] != first[0, :-1]).all()                                            # column to column
    assert cases["patchwork"].nreg == (5 if nz > 2 else cases["patchwork"].nreg)
    if nz * ny >= 100:
        assert 0.03 < np.mean(cases["patchwork"].mask == 0) < 0.2
    sparse = cases["sparse_regions"].mask
    assert (sparse[:, ny - 1] == 0).all()
    counts = [np.count_nonzero(sparse == r) for r in range(1, cases["sparse_regions"].nreg + 1)]
    assert 1 in counts
    assert any((sparse[:, 1:] != r).all() and (sparse[:, 0] == r).any() for r in range(1, len(counts) + 1))
    assert np.array_equal(cases["columns"].mask, np.broadcast_to(np.arange(1, ny + 1), (nz, ny)))


@pytest.mark.parametrize("tc,nz,ny", DEVICE_SHAPES)
def test_no_term_hides_inside_the_dot_bound(tc, nz, ny):
    """what the device test relies on: for every dot it takes (vector 0 against vectors 1 ... 6) the smallest |term| of
    every region is at least 100 bounds of that region"""
    vecs = algebra_vectors(tc, nz, ny)
    assert len(vecs) == ALGEBRA_NVEC
    for name, reg in region_cases(nz, ny).items():
        ref = algebra_reference(reg, tc)
        for v in vecs[1:]:
            terms, mask = ref.dot_terms(vecs[0], v)
            for r in range(reg.nreg):
                mine = terms[mask == r + 1]
                bound = (mine.size + 3) * U53 * np.sum(mine)
                assert mine.size == ref.count[r] > 0 and mine.min() >= 100.0 * bound, (name, r, mine.min(), bound)
