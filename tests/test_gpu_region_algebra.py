"""The region-weighted vector algebra every GMRES iteration runs on, at every column-depth class: k_dot, k_axpby,
k_diff_scale, k_mgs_update, k_lin_comb, k_mask and k_reduce (csrc/nk2d_api.hip, csrc/nk2d_kernels.hip), k_multi_dot,
k_multi_axpy and k_reduce_cols (csrc/nk2d_krylov.hip), through ModuleEngine and the C ABI, against helpers.algebra_reference
(plain NumPy in the kernels' documented operation order; dots in exact rational arithmetic), which
test_region_algebra_host.py holds to the oracle on the CPU.

Each kernel is a template over the levels per lane E = ceil(nz / 64) and finds its ypos column as task % ny over tc * ny
wave tasks, so the grids walk nz through every E (ragged and exact column ends, the smallest column), ny through 2, 5, 7 and
the tracer count through 1, 2, 3, and every grid carries four region layouts (helpers.region_cases): boundaries inside a
column at levels that are multiples of neither 64 nor E, a patchwork with cells of no region, regions absent from whole
columns, column regions.  Element-wise results must be the reference's bit for bit; a regional dot must lie within
(N_r + 3) 2**-53 S_r of the exact one (derived in helpers.algebra_reference, no factor on it), while the inputs keep every
single term of a dot above 100 such bounds (asserted on the CPU), so that one cell dropped, doubled or counted for the
wrong region fails the test."""
import numpy as np
import pytest

from helpers import (ALGEBRA_GRIDS, ALGEBRA_MGS_EDGE, ALGEBRA_N_EDGE, ALGEBRA_REDUCE_SHAPES, ALGEBRA_TC, algebra_coefs,
                     algebra_reference, algebra_vectors, region_cases, rel_err)

pytestmark = pytest.mark.gpu

BASIS_SCALE = 0.3       # basis vectors of the Gram-Schmidt checks: <v, v> near 1, so that projections do not grow w


def _engine(tc, nz, ny):
    """a linear module of tc tracers; phosphorus (the production module of three tracers) on the grids of five columns"""
    from nk_ooc_amd.engine import ModuleEngine, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    grid = Grid2d.default(nz, ny)
    if tc == 3 and ny == 5:
        return phosphorus_engine(grid)
    return ModuleEngine(grid, tc=tc, decay_rate=(1.0e-8,) * tc)


def _same(eng, vec, want):
    return np.array_equal(eng.download(vec).reshape(-1), want)


def _check_layout(eng, name, reg, vecs):
    tc = eng.tc
    eng.set_region(reg.mask, reg.weight)
    assert eng.nreg == reg.nreg
    ref = algebra_reference(reg, tc)
    d = [eng.upload(v) for v in vecs]
    c0, c1 = algebra_coefs(reg.nreg, 2)
    # ---- element-wise: bit for bit
    assert _same(eng, eng.scale(d[0], c0), ref.scale(vecs[0], c0)), name
    assert _same(eng, eng.axpby(c0, d[0], c1, d[1]), ref.axpby(c0, vecs[0], c1, vecs[1])), name
    assert _same(eng, eng.diff_scale(d[0], d[1], c0), ref.diff_scale(vecs[0], vecs[1], c0)), name
    assert _same(eng, eng.apply_region_mask(d[0].copy()), ref.mask_out(vecs[0])), name
    for n in (1, 2, 5):
        cf = algebra_coefs(reg.nreg, n)
        assert _same(eng, eng.lin_comb(d[1:n + 1], cf), ref.lin_comb(cf, vecs[1:n + 1])), (name, n)
    # (all coefficients zero: exactly zero in every cell of a region -- an accumulator that starts from anything but its
    # first term shows, even where what it starts from is small against the inputs)
    nothing = np.zeros((2, reg.nreg))
    assert _same(eng, eng.lin_comb(d[1:3], nothing), ref.lin_comb(nothing, vecs[1:3])), name
    for n in (1, 4):
        h = algebra_coefs(reg.nreg, n, seed=41)
        for fill in (1.0, 0.0):
            w = eng.multi_axpy(d[0].copy(), d[1:n + 1], h, fill=fill)
            assert _same(eng, w, ref.multi_axpy(vecs[0], vecs[1:n + 1], h, fill)), (name, n, fill)
    # ---- the in-place forms nk2d_gmres_solve uses: out is an input
    x = d[0].copy()
    assert _same(eng, eng.axpby(c0, x, c1, d[1], out=x), ref.axpby(c0, vecs[0], c1, vecs[1])), name
    x = d[0].copy()
    assert _same(eng, eng.scale(x, c0, out=x), ref.scale(vecs[0], c0)), name
    x = d[0].copy()
    assert _same(eng, eng.diff_scale(x, d[1], c0, out=x), ref.diff_scale(vecs[0], vecs[1], c0)), name
    # ---- dots: within the derived bound of the exact ones; the fused dots are the single ones bit for bit
    refs = [ref.dot(vecs[0], v) for v in vecs[1:]]
    got = eng.dot(d[0], d[1])
    one = eng.multi_dot(d[0], d[1:2])
    six = eng.multi_dot(d[0], d[1:7])
    stack = np.stack([eng.dot(d[0], b) for b in d[1:7]])
    excess = [ref.dot_excess(got, refs[0])] + [ref.dot_excess(row, r) for row, r in zip(six, refs)]
    print(f"{name}: nreg {reg.nreg}, cells per region {ref.count.min()} ... {ref.count.max()}, "
          f"|dot - exact| / bound at most {max(excess):.3f}")
    assert max(excess) <= 1.0, (name, excess)
    assert np.array_equal(six, stack) and np.array_equal(one, stack[:1]) and np.array_equal(got, stack[0]), name
    # ---- modified Gram-Schmidt against the reference's with the exact dots
    basis = [BASIS_SCALE * v for v in vecs[1:5]]
    h_ref, w_ref, h_bound = ref.mgs(vecs[0], basis)
    w = d[0].copy()
    h = eng.mgs(w, [eng.upload(v) for v in basis])
    w_err = rel_err(eng.download(w).reshape(-1), w_ref)
    print(f"{name}: mgs |h - h_ref| / bound at most {np.max(np.abs(h - h_ref) / h_bound):.3f}, w {w_err:.2e}")
    assert (np.abs(h - h_ref) <= h_bound).all(), name
    assert w_err < 1e-12, (name, w_err)
    # ---- cells of no region do not enter a dot, whatever they hold
    free = np.tile(ref.mask == 0, tc)
    if free.any():
        poisoned = [eng.upload(np.where(free, np.nan, v)) for v in vecs[:2]]
        assert np.array_equal(eng.dot(*poisoned), got), name
        assert np.array_equal(eng.multi_dot(poisoned[0], poisoned[1:]), one), name


def _check_grid(tc, nz, ny):
    eng = _engine(tc, nz, ny)
    assert (eng.tc, eng.nz, eng.ny) == (tc, nz, ny)
    vecs = algebra_vectors(tc, nz, ny)
    try:
        # one engine, the four layouts in turn: nk2d_set_region reallocates its partials when the region count changes
        for name, reg in region_cases(nz, ny).items():
            _check_layout(eng, name, reg, vecs)
    finally:
        eng.close()


@pytest.mark.parametrize("tc", ALGEBRA_TC)
@pytest.mark.parametrize("nz,ny", ALGEBRA_GRIDS)
def test_algebra_at_every_depth_class(nz, ny, tc):
    _check_grid(tc, nz, ny)


@pytest.mark.parametrize("tc,nz,ny", ALGEBRA_REDUCE_SHAPES)
def test_algebra_reduction_shapes(tc, nz, ny):
    """k_reduce / k_reduce_cols over 2 wave tasks (fewer than a wave of the reducing block has lanes) and over 261 (no
    multiple of the block's 256 threads: its second round is ragged)"""
    assert tc * ny in (2, 261)
    _check_grid(tc, nz, ny)


@pytest.mark.parametrize("tc,nz,ny", [(3, 65, 2), (1, 2, 2), (2, 200, 7)])
def test_padding_levels_do_not_enter(tc, nz, ny):
    """a column is padded to a multiple of 64 levels; nan in the padding of every operand (written through the zero-copy
    tensor view of the vectors) changes no dot, no projection coefficient and no owned cell of an element-wise result"""
    import torch

    eng = _engine(tc, nz, ny)
    reg = region_cases(nz, ny)["patchwork"]
    eng.set_region(reg.mask, reg.weight)
    ref = algebra_reference(reg, tc)
    vecs = algebra_vectors(tc, nz, ny)
    clean = [eng.upload(v) for v in vecs[:4]]
    dirty = [eng.upload(v) for v in vecs[:4]]
    # the packed layout of a column: lane l of the column's wave holds the levels l E ... l E + E - 1, level l E + e at
    # position 64 e + l (k_pack_state, csrc/nk2d_kernels.hip); positions whose level is >= nz are padding
    e = (nz + 63) // 64
    slot, lane = np.divmod(np.arange(64 * e), 64)
    pad = torch.from_numpy(lane * e + slot >= nz)
    assert pad.sum() == 64 * e - nz
    eng.sync()
    for vec in dirty:
        view = eng.vec_tensor(vec).view(tc * ny, 64 * e)
        view[:, pad.to(view.device)] = float("nan")
    torch.cuda.synchronize()
    for vec, host in zip(dirty, vecs):
        assert np.array_equal(eng.download(vec).reshape(-1), host)
    c0, c1 = algebra_coefs(reg.nreg, 2)
    assert np.array_equal(eng.dot(dirty[0], dirty[1]), eng.dot(clean[0], clean[1]))
    assert np.array_equal(eng.multi_dot(dirty[0], dirty[1:]), eng.multi_dot(clean[0], clean[1:]))
    assert _same(eng, eng.axpby(c0, dirty[0], c1, dirty[1]), ref.axpby(c0, vecs[0], c1, vecs[1]))
    basis = [eng.scale(v, BASIS_SCALE) for v in dirty[1:]]
    basis_clean = [eng.scale(v, BASIS_SCALE) for v in clean[1:]]
    h = eng.mgs(dirty[0], basis)
    assert np.array_equal(h, eng.mgs(clean[0], basis_clean))
    assert np.array_equal(eng.download(dirty[0]), eng.download(clean[0]))
    eng.close()


def test_mgs_capacity_edge():
    """(n + 1) nreg <= 4096 of nk2d_mgs at 64 column regions: 63 basis vectors pass and match the reference, 64 are refused
    before anything is launched, and the engine goes on answering.  The basis is 63 (64) pointers to four vectors that live
    on disjoint sets of levels, a tenth of the inputs' size: a projection then feeds the error of an earlier one back only
    through the same vector, weakly, and the propagated bound stays near 1e-13 to the last of them"""
    from nk_ooc_amd.engine import Nk2dError

    tc, nz, ny = ALGEBRA_MGS_EDGE
    eng = _engine(tc, nz, ny)
    reg = region_cases(nz, ny)["columns"]
    assert reg.nreg == 64
    eng.set_region(reg.mask, reg.weight)
    ref = algebra_reference(reg, tc)
    vecs = algebra_vectors(tc, nz, ny, n=5)
    level = np.broadcast_to(np.arange(nz)[None, :, None], (tc, nz, ny)).reshape(-1)
    four = [0.1 * vecs[1 + k] * (level % 4 == k) for k in range(4)]
    dfour = [eng.upload(v) for v in four]
    basis, dbasis = [four[i % 4] for i in range(64)], [dfour[i % 4] for i in range(64)]
    h_ref, w_ref, h_bound = ref.mgs(vecs[0], basis[:63])
    assert h_bound.max() < 1e-12 * np.abs(h_ref).max()
    w = eng.upload(vecs[0])
    h = eng.mgs(w, dbasis[:63])
    w_err = rel_err(eng.download(w).reshape(-1), w_ref)
    print(f"63 projections: |h - h_ref| / bound at most {np.max(np.abs(h - h_ref) / h_bound):.3f}, w {w_err:.2e}")
    assert (np.abs(h - h_ref) <= h_bound).all()
    assert w_err < 1e-12
    w = eng.upload(vecs[0])
    with pytest.raises(Nk2dError, match="too many basis vectors"):
        eng.mgs(w, dbasis)
    assert _same(eng, w, vecs[0])
    assert ref.dot_excess(eng.dot(w, dbasis[0]), ref.dot(vecs[0], basis[0])) <= 1.0
    eng.close()


def test_fused_calls_take_512_vectors_and_refuse_513():
    """n <= 512 of nk2d_multi_dot, nk2d_multi_axpy and nk2d_lin_comb: 512 pointers to five vectors give the reference's
    results, 513 are refused before anything is launched"""
    from nk_ooc_amd.engine import Nk2dError

    tc, nz, ny = ALGEBRA_N_EDGE
    eng = _engine(tc, nz, ny)
    reg = region_cases(nz, ny)["patchwork"]
    eng.set_region(reg.mask, reg.weight)
    ref = algebra_reference(reg, tc)
    vecs = algebra_vectors(tc, nz, ny, n=6)
    d = [eng.upload(v) for v in vecs]
    pick = [1 + i % 5 for i in range(513)]
    many, hmany = [d[i] for i in pick], [vecs[i] for i in pick]
    dots = eng.multi_dot(d[0], many[:512])
    refs = [ref.dot(vecs[0], v) for v in vecs[1:]]
    assert np.array_equal(dots, np.stack([eng.dot(d[0], d[i]) for i in pick[:512]]))
    assert max(ref.dot_excess(dots[k], refs[pick[k] - 1]) for k in range(512)) <= 1.0
    cf = algebra_coefs(reg.nreg, 513)
    assert _same(eng, eng.lin_comb(many[:512], cf[:512]), ref.lin_comb(cf[:512], hmany[:512]))
    h = 0.01 * cf
    for fill in (1.0, 0.0):
        w = eng.multi_axpy(d[0].copy(), many[:512], h[:512], fill=fill)
        assert _same(eng, w, ref.multi_axpy(vecs[0], hmany[:512], h[:512], fill)), fill
    with pytest.raises(Nk2dError, match="nk2d_multi_dot: n out of range"):
        eng.multi_dot(d[0], many)
    with pytest.raises(Nk2dError, match="nk2d_lin_comb: n out of range"):
        eng.lin_comb(many, cf)
    w = d[0].copy()
    with pytest.raises(Nk2dError, match="nk2d_multi_axpy: n out of range"):
        eng.multi_axpy(w, many, h)
    assert _same(eng, w, vecs[0])
    assert ref.dot_excess(eng.dot(d[0], d[1]), refs[0]) <= 1.0
    eng.close()
