"""Frozen years replayed from a command tape (option "frozen_tape", csrc/nk2d_stream.h): the commands
of a frozen year are recorded once per schedule, put in HBM, and every frozen year of that schedule is ONE launch of the
resident kernel with no host in the loop.  The kernel runs the device functions the host-fed command stream runs, so the year
is the frozen year by launches and as a host-fed stream BIT FOR BIT -- for the recorded state, the free-running year itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _phos_state(eng, rng):
    tc, nz, ny = eng.shape
    prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                 ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    return np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, ny)))


def _iage_state(eng, seed=5):
    rng = np.random.default_rng(seed)
    tc, nz, ny = eng.shape
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    return np.stack([np.broadcast_to(col[:, None], (nz, ny))] * tc) + 0.01 * rng.standard_normal(eng.shape)


def _engine(case, golden_dir=None, tmp_path=None, two_waves=None):
    from nk_ooc_amd.engine import forced_engine, iage_engine, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    kind, size = case.split("_")[0], case.split("_")[-1]
    rng = np.random.default_rng(12)
    if kind == "iage":
        nz, ny = (int(v) for v in size.split("x"))
        eng = iage_engine(Grid2d.default(nz, ny))
        x0 = _iage_state(eng)
    elif kind == "phosphorus":
        nz, ny = (int(v) for v in size.split("x"))
        eng = phosphorus_engine(Grid2d.default(nz, ny))
        x0 = _phos_state(eng, rng)
    elif case.startswith("forced_decay"):
        eng = forced_engine(Grid2d.default(26, 26), {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"})
        bump = np.cumsum(np.cumsum(rng.standard_normal((1, 26, 26)), axis=1), axis=2)
        x0 = 1.0 + 0.3 * bump / np.max(np.abs(bump))
    else:
        from test_gpu_forced import _file_modelinfo

        g = np.load(f"{golden_dir}/{case}.npz")
        eng = forced_engine(Grid2d.default(int(g["nz"]), int(g["ny"])), _file_modelinfo(g, tmp_path))
        x0 = np.asarray(g["y0"]).reshape(eng.shape)
    if two_waves is not None:
        eng.set_option("stream_two_waves", two_waves)
    eng.set_option("stream_years", 0)
    eng.set_option("frozen_persistent", 0)
    return eng, x0


def _perturbed(x0):
    nz = x0.shape[1]
    return x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, nz))[None, :, None])


def _check_tape_years(eng, x0):
    """the recorded state and x + sigma v on the recorded schedule: by launches, as a host-fed stream, from the tape"""
    x, xp = eng.upload(x0), eng.upload(_perturbed(x0))
    fx, st, sched = eng.comp_fcn(x, record=True)
    free = eng.download(fx)
    launches = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    _, st_l = eng.comp_fcn_frozen(xp, sched)
    eng.set_option("stream_years", 2)
    stream = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("stream_years", 0)
    runs0 = eng.counter("stream_years_run")
    eng.set_option("frozen_tape", 1)
    got_x = eng.download(eng.comp_fcn_frozen(x, sched)[0])
    got_p, st_t = eng.comp_fcn_frozen(xp, sched)
    got_p = eng.download(got_p)
    assert eng.counter("tape_years_run") == 2 and eng.counter("tape_builds") == 1
    assert eng.counter("stream_timeouts") == 0 and eng.counter("tape_timeouts") == 0 and eng.frozen_fallbacks() == 0
    assert eng.counter("tape_fallbacks") == 0
    assert eng.counter("stream_years_run") == runs0 and eng.counter("frozen_persistent_years") == 0
    assert np.array_equal(got_x, free)
    assert np.array_equal(got_p, launches) and np.array_equal(got_p, stream)
    for key in ("nsteps", "nnewton", "nfev", "njev", "nlu", "nerr_checked", "nresumed"):
        assert st_t[key] == st_l[key], key
    assert st_t["max_err"] == st_l["max_err"]
    assert eng.counter("tape_bytes") > 0 and eng.counter("tape_commands") > st_t["nnewton"]
    return sched


@pytest.mark.parametrize("case", ["iage_26x26", "iage_20x3", "iage_180x8", "iage_320x8", "iage_416x8", "iage_512x6"])
def test_iage_frozen_year_from_a_tape(case):
    eng, x0 = _engine(case)
    _check_tape_years(eng, x0)
    eng.close()


@pytest.mark.parametrize("case", ["phosphorus_22x9", "phosphorus_70x12", "phosphorus_416x4", "forced_decay_26x26",
                                  "forced_file_sink_thres_22x9", "forced_file_restore_sms_22x9"])
def test_other_modules_frozen_year_from_a_tape(case, golden_dir, tmp_path):
    eng, x0 = _engine(case, golden_dir, tmp_path)
    _check_tape_years(eng, x0)
    eng.close()


def test_phosphorus_two_waves_tape():
    """seven levels per lane with the flavour of two waves to a SIMD (forced on): the tape flavour of k_stream_w2"""
    eng, x0 = _engine("phosphorus_416x8", two_waves=2)
    _check_tape_years(eng, x0)
    assert eng.counter("stream_two_waves_kernel") == 1
    eng.close()


def test_tape_is_kept_per_schedule():
    from nk_ooc_amd.engine import Nk2dScheduleMismatch

    eng, x0 = _engine("phosphorus_22x9")
    eng.set_option("frozen_tape", 1)
    x, xp = eng.upload(x0), eng.upload(_perturbed(x0))
    _, _, sched = eng.comp_fcn(x, record=True)
    a = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    b = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    assert np.array_equal(a, b) and eng.counter("tape_builds") == 1 and eng.counter("tape_years_run") == 2
    # a new schedule: a new tape
    _, _, sched2 = eng.comp_fcn(xp, record=True)
    c = eng.download(eng.comp_fcn_frozen(x, sched2)[0])
    assert eng.counter("tape_builds") == 2 and eng.counter("tape_years_run") == 3
    eng.set_option("frozen_tape", 0)
    assert np.array_equal(c, eng.download(eng.comp_fcn_frozen(x, sched2)[0]))
    # a schedule of another context (other grid): refused, as without tapes
    other, y0 = _engine("phosphorus_22x10")
    _, _, sched_o = other.comp_fcn(other.upload(y0), record=True)
    other.close()
    eng.set_option("frozen_tape", 1)
    with pytest.raises(Nk2dScheduleMismatch):
        eng.comp_fcn_frozen(x, sched_o)
    assert eng.counter("tape_builds") == 2
    eng.close()


def test_starved_schedule_is_resumed_after_a_tape_year():
    """the recipe of test_gpu_frozen_safety: Newton iterations taken away at one step; the check after the tape year finds the
    step and resumes from the checkpoint the tape wrote -- the same result and counts as the launch path"""
    from test_gpu_frozen_safety import _starved

    eng, x0 = _engine("iage_26x26")
    x = eng.upload(x0)
    _, _, sched = eng.comp_fcn(x, record=True)
    res = {}
    for tape in (0, 1):
        eng.set_option("frozen_tape", tape)
        for drop in (1, 2, 3):
            if not np.any(sched[200:, 3] >= drop + 1):
                continue
            bad, _ = _starved(sched, drop=drop)
            r0, f0 = eng.frozen_resumes(), eng.frozen_fallbacks()
            fx2, st2 = eng.comp_fcn_frozen(x, bad)
            res[(tape, drop)] = (eng.download(fx2), st2["nresumed"], eng.frozen_resumes() - r0, eng.frozen_fallbacks() - f0,
                                 st2["nsteps"])
    assert eng.counter("tape_years_run") >= 1
    for drop in (1, 2, 3):
        if (0, drop) in res:
            a, b = res[(0, drop)], res[(1, drop)]
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], drop
    eng.close()


def test_a_tape_year_that_gives_up_is_rerun():
    """time limit zero: a workgroup's first wait for a neighbour gives up; the year is rerun by the existing path, counted"""
    eng, x0 = _engine("iage_52x52")
    x, xp = eng.upload(x0), eng.upload(_perturbed(x0))
    _, _, sched = eng.comp_fcn(x, record=True)
    want = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("frozen_tape", 1)
    eng.set_option("barrier_timeout_ms", 0)
    got, st = eng.comp_fcn_frozen(xp, sched)
    assert np.array_equal(eng.download(got), want)
    assert eng.counter("tape_timeouts") >= 1 and eng.counter("tape_years_run") == 0 and st["nbarrier_timeouts"] == 1
    eng.set_option("barrier_timeout_ms", 2000)
    got = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    assert np.array_equal(got, want) and eng.counter("tape_years_run") == 1
    eng.close()


def test_a_reallocated_buffer_drops_the_tape():
    """set_region with another number of regions reallocates the norm partials the recorded Newton commands write to: the next
    frozen year records the tape again and is the launches' year bit for bit"""
    eng, x0 = _engine("phosphorus_22x9")
    tc, nz, ny = eng.shape
    weight = np.outer(eng.grid.depth.delta, eng.grid.ypos.delta)
    eng.set_region(np.ones((nz, ny), dtype=np.int32), weight)
    x, xp = eng.upload(x0), eng.upload(_perturbed(x0))
    _, _, sched = eng.comp_fcn(x, record=True)
    want = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("frozen_tape", 1)
    assert np.array_equal(eng.download(eng.comp_fcn_frozen(xp, sched)[0]), want) and eng.counter("tape_builds") == 1
    eng.set_region(np.broadcast_to(np.arange(1, ny + 1, dtype=np.int32)[None, :], (nz, ny)).copy(), weight)   # ny regions
    assert np.array_equal(eng.download(eng.comp_fcn_frozen(xp, sched)[0]), want)
    assert eng.counter("tape_builds") == 2 and eng.counter("tape_years_run") == 2 and eng.counter("tape_fallbacks") == 0
    eng.close()


def _krylov_solve(work, names, nz, ny):
    """a GMRES solve through the solver mirrors (ModelState / KrylovSolver, the modules' years in flight together): the
    increment file, beta, the Hessenberg matrix, and tape_years_run of every module"""
    import os

    from nk_ooc_amd import ncio
    from nk_ooc_amd.krylov_solver import KrylovSolver
    from nk_ooc_amd.model_config import ModelConfig
    from nk_ooc_amd.model_state import ModelState
    from nk_ooc_amd.setup_solver import gen_grid_vars_file, make_config
    from test_gpu_config4 import DECAY, _structured_dye

    os.makedirs(work)
    cfg = make_config(work, nz, ny, tracer_module_names=names, extra_modelinfo=DECAY,
                      extra_solverinfo={"krylov_max_iter": "3", "krylov_rel_tol": "1e-9"})
    gen_grid_vars_file(cfg["modelinfo"])
    ModelState.reset_class()
    ModelState.model_config_obj = ModelConfig(cfg["modelinfo"])
    ModelState.write_files = True
    try:
        iterate = ModelState("gen_init_iterate")
        if len(iterate.tracer_modules) == 3:
            _structured_dye(ModelState, iterate, nz, ny)
        hist_fname = os.path.join(work, "hist_00.nc")
        fcn = iterate.comp_fcn(os.path.join(work, "fcn_00.nc"), None, hist_fname)
        solverinfo = dict(cfg["solverinfo"], krylov_workdir=os.path.join(work, "krylov_00"))
        solver = KrylovSolver(iterate, solverinfo, False, False, hist_fname)
        inc_name = os.path.join(work, "increment_00.nc")
        solver.solve(inc_name, fcn)
        inc, _ = ncio.read_file(inc_name)
        st = solver._solver_state
        taped = {tms.name: tms.eng.counter("tape_years_run") for tms in iterate.tracer_modules}
        return inc, st.get_value_saved_state("beta"), st.get_value_saved_state("h_mat"), taped
    finally:
        ModelState.reset_class()


@pytest.mark.parametrize("names,nz,ny", [("phosphorus", 70, 12), ("iage,phosphorus,forced_{suff}:dye", 22, 9)],
                         ids=["phosphorus_70x12", "three_modules_22x9"])
def test_gmres_with_tapes(tmp_path, monkeypatch, names, nz, ny):
    """NK2D_FROZEN_TAPE=1 through the solver mirrors -- phosphorus alone, and the three modules of one ModelState whose years
    are in flight together: the default's increment, beta and Hessenberg matrix bit for bit, with the phosphorus products'
    perturbed years run from tapes (iage and the decaying forced module: the one-launch year on the cache takes them)"""
    res = {}
    for tape in ("0", "1"):
        monkeypatch.setenv("NK2D_FROZEN_TAPE", tape)
        res[tape] = _krylov_solve(str(tmp_path / f"tape{tape}"), names, nz, ny)
    a, b = res["0"], res["1"]
    assert set(a[0]) == set(b[0]) and len(a[0]) >= 3
    for name in a[0]:
        assert np.array_equal(np.asarray(a[0][name]), np.asarray(b[0][name])), name
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3]["phosphorus"] == 0 and b[3]["phosphorus"] >= 1, (a[3], b[3])
