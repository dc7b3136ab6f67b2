"""The history block (hist.fields_block_layout): hist.pack_fields_host -- every sum in the order of its
index -- against what hist.write_hist_file writes from the same samples by its NumPy reductions, a file written from blocks
against a file written the old way, and the layout.

Contract: samples, time_mean, time_anom, time_std (the square root of the same sum, by the same np.sqrt), time_delta,
depth_int and vert_mixing_coeff bit for bit.  NumPy sums the ypos axis in pairwise blocks of its own, so ypos_mean and
depth_ypos_int are held -- both NumPy's value and the block's -- to the exact sums (math.fsum) within
    ypos_mean:       (ny + 2) 2^-53 sum_j |dy_j v_j| / yspan
    depth_ypos_int:  (nz + ny + 2) 2^-53 sum_k dz_k sum_j |dy_j v|."""
import math

import numpy as np
import pytest
from scipy.io import netcdf_file

from nk_ooc_amd import hist
from nk_ooc_amd.grid import Grid2d

EXACT = ("", "_time_mean", "_time_anom", "_time_std", "_time_delta", "_depth_int")
SHAPES = [(61, 7, 5), (2, 7, 5), (3, 130, 2), (61, 40, 65)]
U = 2.0 ** -53


def _case(n, nz, ny, nvar, seed=3):
    """samples of `nvar` tracer-like variables (signs mixed, magnitudes over six decades, zeros at the start as iage has them;
    the last of four stands for an uptake) and mixing coefficients"""
    rng = np.random.default_rng(seed + 1000 * n + nz + ny)
    grid = Grid2d.default(nz, ny)
    samples = rng.standard_normal((n, nvar, nz, ny)) * 10.0 ** rng.uniform(-3, 3, (1, nvar, nz, 1))
    samples[0, 0] = 0.0
    vmix = 10.0 ** rng.uniform(-4, 1, (n, nz - 1, ny))
    names = ["po4", "dop", "pop", "po4_uptake"][:nvar] if nvar == 4 else ["iage", "iage_2"]
    tracers = {name: {"long_name": name, "units": "mmol / m^3"} for name in names}
    return grid, tracers, samples, vmix


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _read(fname):
    with netcdf_file(fname, "r", mmap=False) as fptr:
        data = {name: np.array(var[:], dtype=np.float64) for name, var in fptr.variables.items()}
        meta = {name: (var.dimensions, dict(var._attributes)) for name, var in fptr.variables.items()}
        return data, meta, list(fptr.variables), {k: v for k, v in fptr.dimensions.items()}, fptr.history


def _row_bounds(grid, vals):
    """exact row sums and the two bounds for samples `vals` [n, nz, ny]"""
    n, nz, ny = vals.shape
    dz, dy = grid.depth.delta, grid.ypos.delta
    yspan = grid.ypos.edges.max() - grid.ypos.edges.min()
    exact_mean, bound_mean = np.empty((n, nz)), np.empty((n, nz))
    exact_int, bound_int = np.empty(n), np.empty(n)
    for i in range(n):
        exact_rows, abs_rows = [], []
        for k in range(nz):
            prods = [float(dy[j]) * float(vals[i, k, j]) for j in range(ny)]
            exact_rows.append(math.fsum(prods))
            abs_rows.append(math.fsum(abs(p) for p in prods))
            exact_mean[i, k] = exact_rows[-1] / yspan
            bound_mean[i, k] = (ny + 2) * U * abs_rows[-1] / yspan
        exact_int[i] = math.fsum(float(dz[k]) * exact_rows[k] for k in range(nz))
        bound_int[i] = (nz + ny + 2) * U * math.fsum(float(dz[k]) * abs_rows[k] for k in range(nz))
    return exact_mean, bound_mean, exact_int, bound_int


def _check_row_sums(grid, vals, ypos_mean, depth_ypos_int, what):
    exact_mean, bound_mean, exact_int, bound_int = _row_bounds(grid, vals)
    err_mean = np.abs(np.asarray(ypos_mean, dtype=np.float64) - exact_mean)
    err_int = np.abs(np.asarray(depth_ypos_int, dtype=np.float64) - exact_int)
    print(f"{what}: ypos_mean worst error / bound {np.max(err_mean / np.maximum(bound_mean, 1e-300)):.3f}, "
          f"depth_ypos_int {np.max(err_int / np.maximum(bound_int, 1e-300)):.3f}")
    assert np.all(err_mean <= bound_mean), what
    assert np.all(err_int <= bound_int), what


@pytest.mark.parametrize("nvar", [2, 4])
@pytest.mark.parametrize("n,nz,ny", SHAPES)
def test_pack_fields_host_is_todays_file(n, nz, ny, nvar, tmp_path):
    grid, tracers, samples, vmix = _case(n, nz, ny, nvar)
    time = np.linspace(0.0, 365.0 * 86400.0, n)
    fname = str(tmp_path / "hist_today.nc")
    hist.write_hist_file(fname, grid, time, [(tracers, samples)], vmix, "stamp")
    today = _read(fname)[0]
    block = hist.pack_fields_host(grid, samples, vmix)
    assert block.block.dtype == np.dtype(">f8") and block.block.size == hist.fields_block_layout(n, nvar, nz, ny)["len"]
    assert np.array_equal(_bits(block.vert_mixing_coeff), _bits(today["vert_mixing_coeff"]))
    for ind, tname in enumerate(tracers):
        assert np.array_equal(_bits(block[:, ind]), _bits(samples[:, ind]))
        for suffix in EXACT:
            assert np.array_equal(_bits(block.field(ind, suffix)), _bits(today[tname + suffix])), tname + suffix
        # NumPy's own pairwise sums and the block's sequential ones: both within the bounds of the exact sums
        _check_row_sums(grid, samples[:, ind], today[tname + "_ypos_mean"], today[tname + "_depth_ypos_int"], f"numpy {tname}")
        _check_row_sums(grid, samples[:, ind], block.field(ind, "_ypos_mean"), block.field(ind, "_depth_ypos_int"), f"block {tname}")


def test_negative_zero_and_nan_pass_through():
    """the sums over time and over depth start from 0 (a mean and a depth integral of -0.0 samples are +0.0, as np.einsum and
    .sum(axis=-2) give them); a NaN sample stays a NaN with its payload in `samples`"""
    n, nz, ny = 3, 4, 2
    grid = Grid2d.default(nz, ny)
    samples = np.full((n, 1, nz, ny), -0.0)
    samples[1, 0, 2, 1] = np.uint64(0x7FF8000000ABCDEF).view(np.float64)
    vmix = np.ones((n, nz - 1, ny))
    block = hist.pack_fields_host(grid, samples, vmix)
    weights = hist.time_mean_weights(n)
    vals = samples[:, 0]
    assert np.array_equal(_bits(block.field(0, "")), _bits(vals))
    clean = np.ones((nz, ny), dtype=bool)
    clean[2, 1] = False
    assert np.array_equal(_bits(block.field(0, "_time_mean"))[clean], _bits(np.einsum("i,i...", weights, vals))[clean])
    assert np.all(_bits(block.field(0, "_time_mean"))[clean] == 0), "a mean of -0.0 samples is +0.0"
    assert np.isnan(block.field(0, "_time_mean")[2, 1])
    assert np.array_equal(_bits(block.field(0, "_depth_int"))[[0, 2]], _bits((grid.depth.delta[:, np.newaxis] * vals).sum(axis=-2))[[0, 2]])


@pytest.mark.parametrize("nvar", [2, 4])
def test_file_from_blocks_is_the_file_of_today(nvar, tmp_path):
    n, nz, ny = 61, 7, 5
    grid, tracers, samples, vmix = _case(n, nz, ny, nvar)
    time = np.linspace(0.0, 365.0 * 86400.0, n)
    old, new = str(tmp_path / "old.nc"), str(tmp_path / "new.nc")
    hist.write_hist_file(old, grid, time, [(tracers, samples)], vmix, "the stamp")
    hist.write_hist_file(new, grid, time, [(tracers, hist.pack_fields_host(grid, samples, vmix))], None, "the stamp")
    d_old, m_old, order_old, dims_old, stamp_old = _read(old)
    d_new, m_new, order_new, dims_new, stamp_new = _read(new)
    assert order_new == order_old and dims_new == dims_old and stamp_new == stamp_old
    assert m_new == m_old
    row_summed = {t + s for t in tracers for s in ("_ypos_mean", "_depth_ypos_int")}
    for name in order_old:
        if name not in row_summed:
            assert np.array_equal(_bits(d_new[name]), _bits(d_old[name])), name
    for ind, tname in enumerate(tracers):
        _check_row_sums(grid, samples[:, ind], d_new[tname + "_ypos_mean"], d_new[tname + "_depth_ypos_int"], f"file {tname}")
    # a writer fed through HistWriter serves the samples of a block as it serves an array's
    writer = hist.HistWriter()
    writer.submit(str(tmp_path / "w.nc"), grid, time, [(tracers, hist.pack_fields_host(grid, samples, vmix))], None, "s", background=False)
    first = next(iter(tracers))
    got = writer.tracer_samples(str(tmp_path / "w.nc"), [first])[first][0]
    assert np.array_equal(_bits(got), _bits(samples[:, 0]))


def test_layout_is_the_documented_order():
    """samples, time_mean, time_anom, time_std, time_delta, depth_int, ypos_mean, depth_ypos_int per variable, one variable after
    the other, vert_mixing_coeff behind the last; lengths worked out by hand"""
    for n, nvar, nz, ny in [(61, 2, 7, 5), (2, 4, 7, 5), (3, 1, 130, 2), (61, 4, 416, 416)]:
        layout = hist.fields_block_layout(n, nvar, nz, ny)
        plane = nz * ny
        want = [0, n * plane, n * plane + plane, 2 * n * plane + plane, 2 * n * plane + 2 * plane, 2 * n * plane + 3 * plane,
                2 * n * plane + 3 * plane + n * ny, 2 * n * plane + 3 * plane + n * ny + n * nz]
        assert [layout["fields"][s][0] for s in hist.FIELD_SUFFIXES] == want
        assert layout["var_len"] == want[-1] + n
        assert layout["vert_mixing_coeff"] == (nvar * layout["var_len"], (n, nz + 1, ny))
        assert layout["len"] == nvar * layout["var_len"] + n * (nz + 1) * ny
    with pytest.raises(ValueError):
        hist.FieldsBlock(np.zeros(10), 2, 1, 2, 2)
