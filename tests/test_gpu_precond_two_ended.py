"""Option "pc_two_ended": the preconditioner's block elimination from both ends of the ypos axis at once (a twisted
factorisation, csrc/nk2d_precond.hip): two chains of half the length in the same launches, meeting in column ny // 2 --
against the oracle's stable form and sparse direct solves at the bars of the one-ended tests, the counters that say the
path ran and what it bought, and what a `Precond` does when the option changes under it."""
import functools
import os

import numpy as np
import pytest
from scipy.sparse import identity
from scipy.sparse.linalg import spsolve

from helpers import oracle_iage, rel_err
from oracle import krylov
from oracle.grid import default_axes
from oracle.model import apply_precond_stable

pytestmark = pytest.mark.gpu
YEAR = 365.0 * 86400.0


def make_engine(nz, ny, vv=0.1, kh=1000.0, two_ended=1, **options):
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    eng = iage_engine(Grid2d.default(nz, ny, vv, kh))
    eng.set_option("pc_two_ended", two_ended)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


@functools.lru_cache(maxsize=None)
def iage_case(nz, ny, vv=0.1, kh=1000.0):
    """a right-hand side and the oracle's apply of it, computed once per grid (read-only)"""
    _, tm = oracle_iage(nz, ny, vv, kh)
    v = np.random.default_rng(3).standard_normal(2 * nz * ny)
    want = apply_precond_stable(tm, v)
    v.setflags(write=False)
    want.setflags(write=False)
    return v, want


def apply(eng, v):
    return eng.download(eng.precond_apply(eng.upload(v))).reshape(-1)


# nz x ny: empty right chain; one column per chain, no inward mat-vec; unequal chains; odd m = 63 (the general mat-vec
# kernel); m = 78, partial last panel; longer chains; two levels per lane; m = 1248, where the one-launch panel step is
# the default
IAGE_CASES = [(20, 2), (20, 3), (20, 4), (21, 5), (26, 26), (70, 40), (130, 9), (416, 3)]


@pytest.mark.parametrize("nz,ny", IAGE_CASES)
def test_two_ended_apply_against_the_oracle(nz, ny):
    v, want = iage_case(nz, ny)
    eng = make_engine(nz, ny)
    got = apply(eng, v)
    err = rel_err(got, want)
    print(f"{nz} x {ny}: two-ended apply against the oracle's stable form {err:.2e}, "
          f"{eng.counter('pc_setup_rounds')} rounds, {eng.counter('pc_sub_launches')} mat-vec launches")
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    eng.close()
    assert err < 1e-9, err


def test_decoupled_columns_give_the_same_bits():
    """no lateral coupling (vv = 0, kh = 0): both orders of elimination do the same operations on every column"""
    v, want = iage_case(20, 3, 0.0, 0.0)
    got = {}
    for two_ended in (0, 1):
        eng = make_engine(20, 3, 0.0, 0.0, two_ended=two_ended)
        got[two_ended] = apply(eng, v)
        eng.close()
    assert np.array_equal(got[0], got[1])
    assert rel_err(got[1], want) < 1e-9


@pytest.mark.parametrize("nz,ny", [(26, 26), (20, 4)])
def test_the_chain_is_shorter(nz, ny):
    v, want = iage_case(nz, ny)
    eng0 = make_engine(nz, ny, two_ended=0)
    apply(eng0, v)
    assert eng0.counter("pc_setup_rounds") == ny
    assert eng0.counter("pc_sub_launches") == 2 * ny - 1
    eng0.close()
    eng = make_engine(nz, ny)
    first = apply(eng, v)
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    assert eng.counter("pc_sub_launches") <= ny + 2
    again = apply(eng, v)
    eng.close()
    assert np.array_equal(first, again)
    assert rel_err(first, want) < 1e-9


@pytest.mark.parametrize("nz,ny", [(26, 26), (130, 9)])
def test_two_ended_single_precision_storage(nz, ny):
    """"pc_fp32" with the option: refined once against the exact operator 1e-9 as with double precision storage; without the
    refinement the single precision shows"""
    v, want = iage_case(nz, ny)
    eng = make_engine(nz, ny, pc_fp32=1)
    got = apply(eng, v)
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    eng.set_option("pc_refine", 0)
    raw = apply(eng, v)
    eng.close()
    print(f"{nz} x {ny}, pc_fp32 two-ended: refined once {rel_err(got, want):.2e}, unrefined {rel_err(raw, want):.2e}")
    assert rel_err(got, want) < 1e-9, rel_err(got, want)
    assert rel_err(raw, want) > 1e-9, rel_err(raw, want)


@pytest.mark.parametrize("tag", ["22x9", "70x12"])
def test_two_ended_shifted_systems(golden_dir, tag):
    """the shifted systems of the phosphorus preconditioner (mode 1), as test_phosphorus_preconditioner sets them up"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d
    from oracle.krylov import Regions
    from oracle.model import Phosphorus, Py2dModel, apply_precond_phosphorus, phosphorus_precond_matrix

    g = np.load(f"{golden_dir}/phosphorus_{tag}.npz")
    nz, ny = int(g["nz"]), int(g["ny"])
    eng = phosphorus_engine(Grid2d.default(nz, ny))
    eng.set_option("pc_two_ended", 1)
    depth, ypos = default_axes(nz, ny)
    tm = Phosphorus(Py2dModel(depth, ypos))
    weight = np.outer(depth.delta, ypos.delta)
    mask = np.ones((nz, ny), dtype=np.int32)
    eng.set_region(mask, weight)
    po4 = g["y"].reshape(3, nz, ny)[0]
    mat = phosphorus_precond_matrix(tm, po4)
    n = mat.shape[0]
    v = np.random.default_rng(21).standard_normal(n)
    ylin = np.zeros((3, nz, ny))
    ylin[0] = po4
    eng.set_lin_state(eng.upload(ylin))
    eng.shift_factor(0.5 * YEAR, YEAR, [0.02, -0.03])
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    for i, sigma in enumerate([0.02, -0.03]):
        want = spsolve((mat - sigma * identity(n, format="csc")).tocsc(), v)
        got = eng.download(eng.shift_solve(i, eng.upload(v))).reshape(-1)
        print(f"phosphorus {tag}, shift {sigma}: two-ended solve against spsolve {rel_err(got, want):.2e}")
        assert eng.counter("pc_sub_launches") <= ny + 2
        assert rel_err(got, want) < 1e-8
    pc = eng.precond_setup_state(po4)
    want, e_vals, shift = apply_precond_phosphorus(tm, Regions(mask, weight), po4, v)
    assert abs(pc.e_vals[0]) < 1e-9
    assert abs(pc.e_vals[1].real - e_vals[1].real) < 1e-8 * abs(e_vals[1].real)
    assert abs(pc.shift - shift) < 1e-8 * abs(shift)
    got = eng.download(eng.precond_apply(eng.upload(v))).reshape(-1)
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    assert rel_err(got, want) < 1e-6
    eng.close()


def test_two_ended_state_dependent_forced_setup(golden_dir, tmp_path):
    """a forced module with a sink threshold (the Jacobian depends on the state at the three time levels) through
    nk2d_precond_setup_states, as test_forced_file_kernels builds its smallest such case"""
    from nk_ooc_amd.engine import forced_engine
    from nk_ooc_amd.grid import Grid2d
    from test_gpu_forced import _file_modelinfo
    from test_oracle_forced_file import oracle_forced

    g = np.load(f"{golden_dir}/forced_file_sink_thres_22x9.npz")
    nz, ny = int(g["nz"]), int(g["ny"])
    eng = forced_engine(Grid2d.default(nz, ny), _file_modelinfo(g, tmp_path))
    assert eng.state_dependent_precond
    eng.set_option("pc_two_ended", 1)
    eng.precond_setup_states([eng.upload(s) for s in g["precond_states"]])
    assert eng.counter("pc_setup_rounds") == ny // 2 + 1
    got = eng.download(eng.precond_apply(eng.upload(g["precond_v"]))).reshape(-1)
    assert eng.counter("pc_sub_launches") <= ny + 2
    want = apply_precond_stable(oracle_forced(g), g["precond_v"], states=list(g["precond_states"]))
    eng.close()
    assert rel_err(got, want) < 1e-9, rel_err(got, want)


def test_a_switch_after_setup():
    """a `Precond` follows the value it was factorised with, not the current option; the option is read at a set-up; the
    round-1 kernels ("pc_valu") have no two-ended form"""
    from nk_ooc_amd.engine import Nk2dError

    nz, ny = 26, 26
    v, _ = iage_case(nz, ny)
    eng = make_engine(nz, ny)
    before = apply(eng, v)
    eng.set_option("pc_two_ended", 0)
    after = apply(eng, v)
    assert np.array_equal(before, after)
    assert eng.counter("pc_sub_launches") <= ny + 2
    eng.precond_setup()
    assert eng.counter("pc_setup_rounds") == ny
    one_ended = apply(eng, v)
    assert eng.counter("pc_sub_launches") == 2 * ny - 1
    fresh = make_engine(nz, ny, two_ended=0)
    assert np.array_equal(one_ended, apply(fresh, v))
    fresh.close()
    eng.set_option("pc_valu", 1)
    eng.set_option("pc_two_ended", 1)
    with pytest.raises(Nk2dError, match="pc_valu"):
        eng.precond_setup()
    eng.close()


def test_two_ended_through_a_solve(tmp_path, monkeypatch):
    """test_krylov_26x26_vs_oracle with NK2D_PC_TWO_ENDED=1: two Krylov iterations at 26 x 26 against the oracle's Krylov
    loop with the stable preconditioner, at that test's tolerances"""
    from nk_ooc_amd.krylov_solver import KrylovSolver
    from test_gpu_krylov import _setup_run

    monkeypatch.setenv("NK2D_PC_TWO_ENDED", "1")
    cfg, ModelState = _setup_run(tmp_path, 26, 26, extra_solverinfo={"krylov_max_iter": "2", "krylov_rel_tol": "1.0e-8"})
    model, tm = oracle_iage(26, 26)
    weight = np.outer(model.depth.delta, model.ypos.delta)
    mod = krylov.OracleModule(tm, krylov.Regions(np.ones((26, 26), dtype=np.int32), weight), precond="stable")
    x_host = (np.stack([np.broadcast_to(np.interp(model.depth.mid, [55.0, 200.0], [0.0, 2.0])[:, None], (26, 26))] * 2)
              + 0.1).reshape(-1)
    fcn_host = mod.comp_fcn(x_host)
    _, trace = krylov.krylov_solve([mod], [x_host], [fcn_host], rel_tol=1e-8, max_iter=2)

    ModelState.write_files = False
    try:
        iterate = ModelState("zeros")
        eng = iterate.tracer_modules[0].eng
        eng.upload(x_host, out=iterate.tracer_modules[0].vec)
        fcn = iterate.comp_fcn(os.path.join(str(tmp_path), "fcn_00.nc"), None)
        got_fcn = fcn.tracer_modules[0].get_tracer_vals_all().reshape(-1)
        assert np.allclose(got_fcn, fcn_host, rtol=1e-3, atol=1e-6)
        solverinfo = dict(cfg["solverinfo"])
        solverinfo["Krylov_workdir"] = os.path.join(str(tmp_path), "krylov_00")
        solver = KrylovSolver(iterate, solverinfo, resume=False, rewind=False, hist_fname=None)
        solver.solve(os.path.join(str(tmp_path), "increment_00.nc"), fcn)
        st = solver._solver_state
        beta = st.get_value_saved_state("beta")
        h_mat = st.get_value_saved_state("h_mat")
        rounds, launches = eng.counter("pc_setup_rounds"), eng.counter("pc_sub_launches")
    finally:
        ModelState.write_files = True
        ModelState.reset_class()
    assert (rounds, launches) == (14, 27)          # the solve's preconditioner was the two-ended one
    assert st.get_iteration() == 2
    assert rel_err(beta, trace["beta"]) < 1e-4
    assert h_mat.shape == trace["h_mat"][-1].shape == (1, 3, 2, 1)
    assert rel_err(h_mat, trace["h_mat"][-1]) < 2e-2
