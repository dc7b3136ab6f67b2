"""The phosphorus preconditioner behind the C ABI: nk2d_precond_setup_states on a phosphorus context (one vector, the scaled null
vector; engine.precond_set_nullspace) declares the two shifted systems of one nk2d_shift_factor call the extrapolated preconditioner, nk2d_precond_apply is then the whole apply in one call (both systems
down ONE substitution chain, nothing read back) and nk2d_gmres_solve accepts the module.  The one call against the five-call
sequence of PhosphorusPrecond.apply bit for bit at every levels-per-lane class and under the options the substitution
follows, against the oracle, the whole solve against the KrylovSolver mirror, and the refusals."""
import functools
import os

import numpy as np
import pytest

from helpers import rel_err
from oracle.grid import default_axes

pytestmark = pytest.mark.gpu
YEAR = 365.0 * 86400.0
SHIFTS = [0.02, 0.01]       # -(T J - shift I) is then a non-singular M-matrix; the code path does not depend on the sign

# nz x ny: one .. eight levels per lane; ny 4 and 5 give the two-ended chains an even and an odd meeting column; 385 x 4 has
# the odd block size m = 1155 (the narrow mat-vec), 384 is an exact multiple of 64
SHAPES = [(22, 9), (70, 12), (130, 3), (200, 4), (300, 5), (384, 3), (385, 4), (512, 3)]
OPTION_SETS = {
    "defaults": {},
    "two_ended": {"pc_two_ended": 1},
    "fp32_refine0": {"pc_fp32": 1, "pc_refine": 0},
    "fp32_refine1": {"pc_fp32": 1, "pc_refine": 1},
    "two_ended_fp32": {"pc_two_ended": 1, "pc_fp32": 1, "pc_refine": 1},
}


def sub_launches(ny, two_ended):
    """dependent mat-vec launches of one block substitution over ny columns (csrc/nk2d_precond.hip): forward over columns
    1 .. ny - 1 and backward over all of them; from both ends with the meeting column jm = ny // 2 the longer of the two
    inward chains, the left chain's correction of the meeting block, that block, and the longer way out"""
    if not two_ended:
        return 2 * ny - 1
    jm = ny // 2
    return max(jm - 1, ny - 1 - jm) + (1 if jm >= 1 else 0) + 1 + max(jm, ny - 1 - jm)


@functools.lru_cache(maxsize=None)
def case_fields(nz, ny):
    """linearisation state, right-hand side and a positive vector for e_hat, once per grid (read-only)"""
    rng = np.random.default_rng(1000 * nz + ny)
    ylin = np.zeros((3, nz, ny))
    ylin[0] = 2.0 + 0.2 * rng.random((nz, ny))
    v = rng.standard_normal((3, nz, ny))
    pos = 0.5 + rng.random((3, nz, ny))
    for a in (ylin, v, pos):
        a.setflags(write=False)
    return ylin, v, pos


def region_of(nz, ny, layout):
    depth, ypos = default_axes(nz, ny)
    weight = np.outer(depth.delta, ypos.delta)
    mask = np.ones((nz, ny), dtype=np.int32)
    if layout == "bands":           # three regions in ypos bands
        mask[:, ny // 3:2 * ny // 3] = 2
        mask[:, 2 * ny // 3:] = 3
    elif layout == "holes":         # cells of no region, and two regions around them
        mask[:, ny // 2:] = 2
        mask[::3, 1::2] = 0
        mask[nz - 2:, :] = 0
    return mask, weight


def make_case(nz, ny, options=None, layout="one", declare=True):
    """a phosphorus engine with the two shifted systems factorised, and (v, ones, e_hat) on the device"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    eng = phosphorus_engine(Grid2d.default(nz, ny))
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    eng.set_region(*region_of(nz, ny, layout))
    ylin, v, pos = case_fields(nz, ny)
    eng.set_lin_state(eng.upload(ylin))
    eng.shift_factor(0.5 * YEAR, YEAR, SHIFTS)
    ones = eng.upload(np.ones(eng.shape))
    e = eng.upload(pos)
    e_hat = eng.scale(e, 1.0 / eng.dot(e, ones))
    if declare:
        eng.precond_set_nullspace(e_hat)
    return eng, eng.upload(v), ones, e_hat


def composite(eng, v, ones, e_hat, out=None):
    """PhosphorusPrecond.apply as it is with NK2D_PHOS_PC_FUSED unset: five calls"""
    sol_full = eng.shift_solve(0, v)
    sol_half = eng.shift_solve(1, v)
    sol = eng.axpby(2.0, sol_half, -1.0, sol_full, out=sol_half)
    sol = eng.axpby(1.0, sol, -eng.dot(sol, ones), e_hat, out=sol)
    return eng.axpby(1.0, sol, -1.0, v, out=out)


def packed(eng, vec):
    """every double of a vector as it lies in HBM, the padding of the columns included"""
    eng.sync()
    return eng.vec_tensor(vec).cpu().numpy().copy()


def check_same_bits(eng, v, ones, e_hat):
    want = composite(eng, v, ones, e_hat)
    got = eng.precond_apply(v)
    assert np.array_equal(eng.download(got), eng.download(want))
    assert np.array_equal(packed(eng, got), packed(eng, want), equal_nan=True)
    assert np.all(np.isfinite(eng.download(got)))
    return got


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("nz,ny", SHAPES)
def test_one_call_is_the_five_calls_bit_for_bit(nz, ny, opts):
    options = OPTION_SETS[opts]
    eng, v, ones, e_hat = make_case(nz, ny, options)
    assert eng.counter("pc_phos_applies") == 0
    check_same_bits(eng, v, ones, e_hat)
    assert eng.counter("pc_phos_applies") == 1
    assert eng.counter("pc_sub_launches") == sub_launches(ny, options.get("pc_two_ended", 0))
    eng.close()


@pytest.mark.parametrize("layout", ["bands", "holes"])
@pytest.mark.parametrize("opts", ["defaults", "two_ended_fp32"])
def test_regions_and_cells_of_no_region(layout, opts):
    """the null-space correction region by region; a cell of no region gets half + full, + e_hat, + v (the broadcast rule
    of k_axpby: every coefficient is 1.0 there)"""
    nz, ny = 22, 9
    eng, v, ones, e_hat = make_case(nz, ny, OPTION_SETS[opts], layout=layout)
    mask, _ = region_of(nz, ny, layout)
    assert eng.nreg == mask.max()
    got = eng.download(check_same_bits(eng, v, ones, e_hat))
    if layout == "holes":
        free = np.broadcast_to(mask == 0, got.shape)
        assert free.any()
        full = eng.download(eng.shift_solve(0, v))
        half = eng.download(eng.shift_solve(1, v))
        want = ((half + full) + eng.download(e_hat)) + eng.download(v)
        assert np.array_equal(got[free], want[free])
    eng.close()


def test_in_place_repeats_and_counters():
    nz, ny = 22, 9
    for two_ended in (0, 1):
        eng, v, ones, e_hat = make_case(nz, ny, {"pc_two_ended": two_ended})
        want = eng.download(composite(eng, v, ones, e_hat))
        first = eng.download(eng.precond_apply(v))
        assert eng.counter("pc_sub_launches") == sub_launches(ny, two_ended)
        again = eng.download(eng.precond_apply(v))
        assert np.array_equal(first, want) and np.array_equal(again, want)
        x = v.copy()
        same = eng.precond_apply(x, out=x)           # out == v
        assert same is x and np.array_equal(eng.download(x), want)
        assert eng.counter("pc_phos_applies") == 3
        # a composite apply in between leaves the counter alone and the one substitution of a solve behind
        composite(eng, v, ones, e_hat)
        assert eng.counter("pc_phos_applies") == 3
        assert eng.counter("pc_sub_launches") == sub_launches(ny, two_ended)
        eng.close()
    assert sub_launches(9, 0) == 17 and sub_launches(9, 1) == 10 <= 9 + 2      # (the bound of test_gpu_precond_two_ended.py)


@pytest.mark.parametrize("tag", ["22x9", "70x12"])
def test_against_the_oracle(golden_dir, tag, monkeypatch):
    """the full preconditioner of precond_setup_state(po4) with NK2D_PHOS_PC_FUSED=1 against the oracle (sparse direct +
    ARPACK) at the bar of test_phosphorus_preconditioner"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d
    from oracle.krylov import Regions
    from oracle.model import Phosphorus, Py2dModel, apply_precond_phosphorus

    monkeypatch.setenv("NK2D_PHOS_PC_FUSED", "1")
    g = np.load(f"{golden_dir}/phosphorus_{tag}.npz")
    nz, ny = int(g["nz"]), int(g["ny"])
    eng = phosphorus_engine(Grid2d.default(nz, ny))
    assert eng.phos_pc_fused
    depth, ypos = default_axes(nz, ny)
    tm = Phosphorus(Py2dModel(depth, ypos))
    weight = np.outer(depth.delta, ypos.delta)
    mask = np.ones((nz, ny), dtype=np.int32)
    eng.set_region(mask, weight)
    po4 = g["y"].reshape(3, nz, ny)[0]
    v = np.random.default_rng(21).standard_normal(3 * nz * ny)
    pc = eng.precond_setup_state(po4)
    assert pc.fused
    want, _, shift = apply_precond_phosphorus(tm, Regions(mask, weight), po4, v)
    assert abs(pc.shift - shift) < 1e-8 * abs(shift)
    vd = eng.upload(v)
    got = eng.download(eng.precond_apply(vd)).reshape(-1)
    assert eng.counter("pc_phos_applies") == 1
    err = rel_err(got, want)
    print(f"phosphorus {tag}: one-call preconditioner against the oracle {err:.2e}")
    assert err < 1e-6
    # ... and the five calls on the same factorisation: the same bits
    assert np.array_equal(got, eng.download(composite(eng, vd, pc.ones, pc.e_hat)).reshape(-1))
    eng.close()


def test_whole_solve_against_the_krylov_solver_mirror(tmp_path, monkeypatch):
    """tracer_module_names = phosphorus, three iterations as test_phosphorus_krylov_solve sets it up: KrylovSolver.solve with
    the five-call preconditioner, then nk2d_gmres_solve with the declaration installed on the same factorisation and the
    same schedule -- the same Krylov space bit for bit, the increment to the rounding of Givens against LAPACK"""
    from nk_ooc_amd.krylov_solver import KrylovSolver
    from nk_ooc_amd.model_config import ModelConfig
    from nk_ooc_amd.model_state import ModelState
    from nk_ooc_amd.setup_solver import gen_grid_vars_file, make_config

    monkeypatch.delenv("NK2D_PHOS_PC_FUSED", raising=False)
    nz, ny, iters = 22, 9, 3
    work = str(tmp_path)
    cfg = make_config(work, nz, ny, tracer_module_names="phosphorus",
                      extra_solverinfo={"krylov_max_iter": str(iters), "krylov_rel_tol": "1e-9"})
    gen_grid_vars_file(cfg["modelinfo"])
    ModelState.reset_class()
    ModelState.model_config_obj = ModelConfig(cfg["modelinfo"])
    ModelState.write_files = True
    iterate = ModelState("gen_init_iterate")
    hist_fname = os.path.join(work, "hist_00.nc")
    fcn = iterate.comp_fcn(os.path.join(work, "fcn_00.nc"), None, hist_fname)
    solverinfo = dict(cfg["solverinfo"], krylov_workdir=os.path.join(work, "krylov_00"))
    solver = KrylovSolver(iterate, solverinfo, False, False, hist_fname)
    inc = solver.solve(os.path.join(work, "increment_00.nc"), fcn)
    state = solver._solver_state
    beta, h_mat = state.get_value_saved_state("beta"), state.get_value_saved_state("h_mat")
    eng = iterate.tracer_modules[0].eng
    pc = eng._state_precond
    assert not pc.fused and eng.counter("pc_phos_applies") == 0
    x, fx = iterate.tracer_modules[0].vec, fcn.tracer_modules[0].vec
    sched = fcn._sched["phosphorus"]
    assert len(sched) > 50
    eng.precond_set_nullspace(pc.e_hat)
    got, info = eng.gmres_solve(x, fx, 1.0e-9, 0, iters, sched=sched)
    assert info["iters"] == iters == solver.get_iteration()
    assert eng.counter("pc_phos_applies") == iters + 1      # M^-1 fcn and one apply per iteration
    assert np.array_equal(info["beta"], beta[0])
    assert np.array_equal(info["h_mat"], h_mat[0])
    assert rel_err(eng.download(got), eng.download(inc.tracer_modules[0].vec)) < 1e-10
    # stopping rule: with a loose tolerance and min_iter the loop stops where the reference's would
    _, early = eng.gmres_solve(x, fx, 0.9, 2, iters, sched=sched)
    want = next(k + 1 for k in range(iters) if k + 1 >= 2 and (info["resid_norm"][k] < 0.9 * info["beta"]).all())
    assert early["iters"] == want
    ModelState.reset_class()


def test_refusals_and_staleness():
    from nk_ooc_amd.engine import Nk2dError, iage_engine
    from nk_ooc_amd.grid import Grid2d

    iage = iage_engine(Grid2d.default(22, 9))
    some = iage.upload(np.ones(iage.shape))
    with pytest.raises(Nk2dError, match="phosphorus"):
        iage.precond_set_nullspace(some)
    iage.shift_factor(0.5 * YEAR, YEAR, SHIFTS)
    with pytest.raises(Nk2dError, match="module_kind 1"):
        iage.precond_set_nullspace(some)
    import ctypes

    one = (ctypes.c_void_p * 1)(some.ptr)           # ... and so does the library, with the refusal it always had
    assert iage._lib.nk2d_precond_setup_states(iage._ctx, one) < 0
    assert b"forcing files only" in iage._lib.nk2d_last_error(iage._ctx)
    iage.close()

    from nk_ooc_amd.engine import phosphorus_engine

    nz, ny = 22, 9
    eng = phosphorus_engine(Grid2d.default(nz, ny))
    eng.set_region(*region_of(nz, ny, "one"))
    ylin, v, pos = case_fields(nz, ny)
    vd, e_hat = eng.upload(v), eng.upload(pos)
    out = eng.new_vec()
    with pytest.raises(Nk2dError, match="nk2d_shift_factor"):        # before any factorisation
        eng.precond_set_nullspace(e_hat)
    eng.set_lin_state(eng.upload(ylin))
    eng.shift_factor(0.5 * YEAR, YEAR, SHIFTS[:1])
    with pytest.raises(Nk2dError, match="two shifts"):               # a one-system factorisation
        eng.precond_set_nullspace(e_hat)
    eng.shift_factor(0.5 * YEAR, YEAR, SHIFTS)
    with pytest.raises(Nk2dError, match="null vector"):
        eng.precond_set_nullspace(None)
    # nothing declared yet: the apply and the solve refuse and say what to call
    assert eng._lib.nk2d_precond_apply(eng._ctx, vd.ptr, out.ptr) < 0
    assert b"nk2d_precond_setup_states" in eng._lib.nk2d_last_error(eng._ctx)
    with pytest.raises(Nk2dError, match="phosphorus.*nk2d_precond_setup_states"):
        eng.gmres_solve(vd, vd, 1e-2, 0, 2)
    eng.precond_set_nullspace(e_hat)
    first = eng.download(eng.precond_apply(vd))
    assert np.all(np.isfinite(first))
    # a second factorisation takes the declaration away: a stale e_hat never meets another factorisation
    eng.shift_factor(0.5 * YEAR, YEAR, SHIFTS)
    assert eng._lib.nk2d_precond_apply(eng._ctx, vd.ptr, out.ptr) < 0
    msg = eng._lib.nk2d_last_error(eng._ctx)
    assert b"nk2d_shift_factor" in msg and b"nk2d_precond_setup_states" in msg
    with pytest.raises(Nk2dError, match="nk2d_shift_factor.*nk2d_precond_setup_states"):
        eng.gmres_solve(vd, vd, 1e-2, 0, 2)
    assert eng.counter("pc_phos_applies") == 1
    eng.precond_set_nullspace(e_hat)
    assert np.array_equal(eng.download(eng.precond_apply(vd)), first)
    eng.close()
