"""Option "stream_xlane" (csrc/nk2d_stream_xl.hip, nk2d_stream_body.inc): the resident kernel of the
command-stream year in the flavour whose cross-lane moves at distances 1 and 32, and wave sums, go through the VALU (the xl_
helpers of csrc/nk2d_common.h, pinned bit for bit in test_gpu_xlane_helpers.py) instead of ds_bpermute.  The moves carry the
same bits, so the year is the same year: every case runs one year on one engine three ways -- by launches ("stream_years" 0),
as a stream with "stream_xlane" 0, as a stream with "stream_xlane" 1 -- and asks for equal results, equal schedules, equal
stats, a year counted per stream year, no timeout, and counter "stream_xlane_bits" = the option wherever the class has the
flavour (NK2D_STREAM_XLANE in csrc/nk2d_stream.h leaves out linear sources at one level per lane) and 0 where it has not."""
import numpy as np
import pytest

from test_gpu_stream import _iage, _phos_state, _state

pytestmark = pytest.mark.gpu

YEAR = 365.0 * 86400.0
NOT_THE_YEAR = ("seconds", "nlaunch")      # wall time; launches: what a stream year saves


def _has_flavour(eng, kind, two_waves=False):
    """NK2D_STREAM_XLANE(E, KIND, W2) of csrc/nk2d_stream.h"""
    levels_per_lane = (eng.shape[1] + 63) // 64
    return not (levels_per_lane == 1 and kind == 0 and not two_waves)


def _same_stats(a, b, skip=()):
    assert set(a) == set(b)
    differ = {key: (a[key], b[key]) for key in a if key not in skip and a[key] != b[key]}
    assert not differ, differ


def _three_ways(eng, year, stream_years, bits_with_1, not_by_launches=()):
    """year() -> (tuple of arrays, stats): by launches, as a stream with "stream_xlane" 0, as a stream with 1
    (not_by_launches: entries of the stats a stream year books differently from the year by launches whatever the option says;
    between the two stream years every entry but the wall time is compared always)"""
    eng.set_option("stream_years", 0)
    want, st = year()
    eng.set_option("stream_years", stream_years)
    for opt in (0, 1):
        eng.set_option("stream_xlane", opt)
        runs = eng.counter("stream_years_run")
        got, st_s = year()
        assert eng.counter("stream_years_run") == runs + 1 and eng.counter("stream_timeouts") == 0
        bits = eng.counter("stream_xlane_bits")
        print(f"stream_xlane {opt}: stream_xlane_bits {bits}, {st_s['nlaunch']} launches ({st['nlaunch']} by launches)")
        assert bits == (bits_with_1 if opt else 0)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        _same_stats(st_s, st, skip=NOT_THE_YEAR + tuple(not_by_launches))
        if opt == 0:
            st_0 = st_s
        else:
            _same_stats(st_s, st_0, skip=("seconds",))
    return want


def _free_year(eng, x):
    def year():
        fx, st, sched = eng.comp_fcn(x, record=True)
        return (eng.download(fx), sched), st
    return year


def _frozen_year(eng, xp, sched):
    def year():
        fx, st = eng.comp_fcn_frozen(xp, sched)
        return (eng.download(fx),), st
    return year


def _perturbed(x0):
    return x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, x0.shape[1]))[None, :, None])


@pytest.mark.parametrize("nz", [26, 125, 130, 250, 320, 384, 416, 512])
@pytest.mark.parametrize("mode", ["default", "scipy_decisions"])
def test_free_running_year_at_every_depth_class(nz, mode):
    """one to eight levels per lane: 26 leaves 38 lanes of identity rows that go through every level of the reduction, 125 (a
    shipped depth) and 416 have rows past nz in their last lane"""
    eng = _iage(nz, 6)
    if mode == "scipy_decisions":
        eng.set_option("jac_stage", -1)
        eng.set_option("jac_fresh", 0)
    _three_ways(eng, _free_year(eng, eng.upload(_state(eng))), 1, 1 if _has_flavour(eng, 0) else 0)
    eng.close()


def test_edge_columns_only():
    eng = _iage(416, 2)
    _three_ways(eng, _free_year(eng, eng.upload(_state(eng))), 1, 1)
    eng.close()


def test_commands_with_solves_and_no_stage_part():
    """two sweeps per solve: Newton commands without a stage part, and the sweep command of the error estimate"""
    eng = _iage(416, 6)
    eng.set_option("min_sweeps", 2)
    _three_ways(eng, _free_year(eng, eng.upload(_state(eng))), 1, 1)
    eng.close()


@pytest.mark.parametrize("nz", [130, 416])
def test_frozen_year_as_a_stream(nz):
    """the Newton command that ends a frozen step, and the pieces of an error estimate on every third step"""
    eng = _iage(nz, 6)
    eng.set_option("frozen_persistent", 0)
    eng.set_option("frozen_err_check", 3)
    x0 = _state(eng)
    _, _, sched = eng.comp_fcn(eng.upload(x0), record=True)
    _three_ways(eng, _frozen_year(eng, eng.upload(_perturbed(x0)), sched), 3, 1)
    eng.close()


@pytest.mark.parametrize("nz,ny,two_waves", [(30, 12, None), (130, 6, None), (416, 4, 2)])
def test_phosphorus(nz, ny, two_waves):
    """three waves to a workgroup, the Jacobian command of every attempt, the shifts of the sinking flux; at 416 x 4 with
    "stream_two_waves" forced on: k_stream_w2"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    eng = phosphorus_engine(Grid2d.default(nz, ny))
    if two_waves is not None:
        eng.set_option("stream_two_waves", two_waves)
    eng.set_option("frozen_persistent", 0)
    x0 = _phos_state(eng, np.random.default_rng(12))
    want = _three_ways(eng, _free_year(eng, eng.upload(x0)), 3, 1 if _has_flavour(eng, 1, two_waves is not None) else 0)
    assert eng.counter("stream_two_waves_kernel") == (1 if two_waves is not None else 0)
    _three_ways(eng, _frozen_year(eng, eng.upload(_perturbed(x0)), want[1]), 3, 1)
    eng.close()


@pytest.mark.parametrize("case", ["forced_decay_26x26", "forced_file_sink_thres_22x9"])
def test_forced(case, golden_dir, tmp_path):
    """linear sources at one level per lane (the class without the flavour: the option changes nothing and the counter says
    0), and the file-driven module with a thresholded sink (its Jacobian reads the state)"""
    from nk_ooc_amd.engine import forced_engine
    from nk_ooc_amd.grid import Grid2d

    if case == "forced_decay_26x26":
        eng = forced_engine(Grid2d.default(26, 26), {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"})
        bump = np.cumsum(np.cumsum(np.random.default_rng(12).standard_normal((1, 26, 26)), axis=1), axis=2)
        x0, kind = 1.0 + 0.3 * bump / np.max(np.abs(bump)), 0
    else:
        from test_gpu_forced import _file_modelinfo

        g = np.load(f"{golden_dir}/{case}.npz")
        eng = forced_engine(Grid2d.default(int(g["nz"]), int(g["ny"])), _file_modelinfo(g, tmp_path))
        x0, kind = np.asarray(g["y0"]).reshape(eng.shape), 2
    eng.set_option("frozen_persistent", 0)
    bits = 1 if _has_flavour(eng, kind) else 0
    want = _three_ways(eng, _free_year(eng, eng.upload(x0)), 3, bits)
    _three_ways(eng, _frozen_year(eng, eng.upload(_perturbed(x0)), want[1]), 3, bits)
    eng.close()


@pytest.mark.parametrize("stream_hist", [0, 1])
def test_year_with_history_samples(stream_hist):
    """stream_hist 0: every sample ends the kernel and the next command starts it again -- every start takes the flavour
    again; stream_hist 1: the samples are commands of the one kernel.  With stream_hist 1 a sampled step keeps its fused
    boundary command, where the year by launches ends such a step with separate launches and evaluates the Jacobian at the
    start of the next attempt: the same year, one Jacobian (and factorisation) booked differently -- njev 2633 against 2634
    here, with today's kernel as with the new flavour; tests/test_gpu_stream_hist.py compares nsteps, nrejected, nnewton and
    nfev for that reason.  Here: every entry but njev and nlu against the year by launches, every entry between the two
    stream years."""
    eng = _iage(130, 6)
    eng.set_option("stream_hist", stream_hist)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 13)

    def year():
        fx, st, hist = eng.comp_fcn_hist(x, t_eval)
        return (eng.download(fx), hist), st

    starts = eng.counter("stream_launches")
    _three_ways(eng, year, 1, 1, not_by_launches=("njev", "nlu") if stream_hist else ())
    starts = eng.counter("stream_launches") - starts
    assert starts >= (2 * 10 if stream_hist == 0 else 2)
    eng.close()


def test_a_tape_year_runs_unchanged_and_reports_0():
    eng = _iage(130, 6)
    eng.set_option("frozen_persistent", 0)
    x0 = _state(eng)
    x, xp = eng.upload(x0), eng.upload(_perturbed(x0))
    fx, _, sched = eng.comp_fcn(x, record=True)
    want, st_l = eng.comp_fcn_frozen(xp, sched)
    want = eng.download(want)
    eng.set_option("stream_xlane", 1)
    eng.set_option("stream_years", 2)
    assert np.array_equal(eng.download(eng.comp_fcn_frozen(xp, sched)[0]), want) and eng.counter("stream_xlane_bits") == 1
    eng.set_option("stream_years", 0)
    eng.set_option("frozen_tape", 1)
    got, st_t = eng.comp_fcn_frozen(xp, sched)
    assert eng.counter("tape_years_run") == 1 and eng.counter("tape_timeouts") == 0 and eng.counter("stream_timeouts") == 0
    assert eng.counter("stream_xlane_bits") == 0
    assert np.array_equal(eng.download(got), want)
    _same_stats(st_t, st_l, skip=NOT_THE_YEAR)
    eng.close()


def test_option_1_then_0_on_one_engine():
    """the option is read at every start of the kernel: the second year runs today's kernel, says so, and is the same bits"""
    eng = _iage(250, 6)
    x = eng.upload(_state(eng))
    eng.set_option("stream_years", 1)
    eng.set_option("stream_xlane", 1)
    fx_1, st_1, sched_1 = eng.comp_fcn(x, record=True)
    fx_1 = eng.download(fx_1)
    assert eng.counter("stream_xlane_bits") == 1
    eng.set_option("stream_xlane", 0)
    fx_0, st_0, sched_0 = eng.comp_fcn(x, record=True)
    assert eng.counter("stream_xlane_bits") == 0
    assert eng.counter("stream_years_run") == 2 and eng.counter("stream_timeouts") == 0
    assert np.array_equal(eng.download(fx_0), fx_1) and np.array_equal(sched_0, sched_1)
    _same_stats(st_0, st_1, skip=("seconds",))
    with pytest.raises(Exception):
        eng.set_option("stream_xlane", 2)
    eng.close()
