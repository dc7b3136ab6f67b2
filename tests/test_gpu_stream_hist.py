"""History samples as commands of the year's resident kernel (option "stream_hist", csrc/nk2d_stream.h NK2D_OP_DENSE_OUT;
DESIGN.md section 3.5.2): a sampled step keeps its boundary command, its samples are pushed behind it and wait, packed, in a
buffer in HBM until the kernel has ended.  The reference of every comparison is the same engine's year BY LAUNCHES
(stream_years 0; pinned against the CPU oracle in test_gpu_comp_fcn.py): the samples, F(x) and the counters bit for bit."""
import os

import numpy as np
import pytest

from test_gpu_stream import _iage, _phos_state, _state

pytestmark = pytest.mark.gpu

YEAR = 365.0 * 86400.0
KEYS = ("nsteps", "nrejected", "nnewton", "nfev")


def _by_launches(eng, x, t_eval):
    eng.set_option("stream_years", 0)
    fx, st, hist = eng.comp_fcn_hist(x, t_eval)
    return eng.download(fx), st, hist


def _as_commands(eng, x, t_eval, want, **opts):
    """the sampled year as a stream with stream_hist 1 against `want` (_by_launches); returns what the counters gained"""
    eng.set_option("stream_years", 1)
    eng.set_option("stream_hist", 1)
    for key, v in opts.items():
        eng.set_option(key, v)
    names = ("stream_years_run", "stream_launches", "stream_hist_samples", "stream_hist_drains")
    c0 = {k: eng.counter(k) for k in names}
    fx, st, hist = eng.comp_fcn_hist(x, t_eval)
    gained = {k: eng.counter(k) - c0[k] for k in names}
    assert np.array_equal(hist, want[2]) and np.array_equal(eng.download(fx), want[0])
    for key in KEYS:
        assert st[key] == want[1][key], key
    assert gained["stream_years_run"] == 1 and eng.counter("stream_timeouts") == 0
    return gained


@pytest.mark.parametrize("nz,ny", [(26, 26), (52, 52), (130, 20), (416, 8), (512, 6)])
def test_sampled_year_is_one_kernel_start_and_the_same_bits(nz, ny):
    """1, 1, 3, 7 and 8 levels per lane (26 and 130 leave padded lanes), 61 uniform samples: only the sample at t1 may go by
    launches, nothing is drained before the year's end, and the kernel starts as often as in a plain year of the same engine
    and state (+ 2: the last step's sample ends the kernel once more at most)"""
    eng = _iage(nz, ny)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 61)
    want = _by_launches(eng, x, t_eval)
    eng.set_option("stream_years", 1)
    l0 = eng.counter("stream_launches")
    fx, _, _ = eng.comp_fcn(x)
    plain_starts = eng.counter("stream_launches") - l0
    assert np.array_equal(eng.download(fx), want[0])
    gained = _as_commands(eng, x, t_eval, want)
    print(f"{nz}x{ny}: kernel starts plain {plain_starts}, sampled {gained['stream_launches']}; "
          f"samples by command {gained['stream_hist_samples']}, drains {gained['stream_hist_drains']}")
    assert gained["stream_hist_samples"] >= 60
    assert gained["stream_hist_drains"] == 1
    assert gained["stream_launches"] <= plain_starts + 2
    eng.close()


def test_irregular_sample_times():
    """40 samples inside the first two days (several to a step), 10 random ones over the rest of the year (many steps with
    none); neither t0 nor t1 is a sample, so every sample is a command"""
    eng = _iage(52, 52)
    x = eng.upload(_state(eng))
    rng = np.random.default_rng(17)
    t_eval = np.concatenate([np.linspace(600.0, 2.0 * 86400.0, 40), np.sort(rng.uniform(3.0 * 86400.0, YEAR - 86400.0, 10))])
    assert np.all(np.diff(t_eval) > 0) and t_eval[0] > 0.0 and t_eval[-1] < YEAR
    want = _by_launches(eng, x, t_eval)
    gained = _as_commands(eng, x, t_eval, want)
    assert gained["stream_hist_samples"] == len(t_eval) and gained["stream_hist_drains"] == 1
    eng.close()


def test_drains_of_a_small_sample_buffer():
    """one slot (stream_hist_mb 0): a drain per sample; a budget worth exactly 8 slots: 8 or 9 drains for 61 samples"""
    nz = ny = 52
    eng = _iage(nz, ny)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 61)
    want = _by_launches(eng, x, t_eval)
    gained = _as_commands(eng, x, t_eval, want, stream_hist_mb=0)
    assert gained["stream_hist_samples"] >= 60 and gained["stream_hist_drains"] >= 60
    tc, levels = eng.shape[0], -(-nz // 64)
    packed_bytes = tc * ny * levels * 64 * 8          # a packed state: 64 lanes x levels per lane to a (tracer, ypos) column
    gained = _as_commands(eng, x, t_eval, want, stream_hist_mb=8 * packed_bytes / 2.0**20)
    assert gained["stream_hist_samples"] >= 60 and 8 <= gained["stream_hist_drains"] <= 9
    eng.close()


@pytest.mark.parametrize("case", ["phosphorus_30x12", "phosphorus_416x4_two_waves", "forced_file_sink_thres_22x9"])
def test_other_module_kinds(case, golden_dir, tmp_path):
    """phosphorus (three coupled tracers; at 416 x 4 the 256-register flavour of the kernel, forced) and the forced module with
    a thresholded sink: their Jacobian reads the state, a JAC command stands between the boundary and the samples"""
    from nk_ooc_amd.engine import forced_engine, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    if case.startswith("phosphorus"):
        nz, ny = (int(v) for v in case.split("_")[1].split("x"))
        eng = phosphorus_engine(Grid2d.default(nz, ny))
        if case.endswith("two_waves"):
            eng.set_option("stream_two_waves", 2)
        x0 = _phos_state(eng, np.random.default_rng(12))
    else:
        from test_gpu_forced import _file_modelinfo

        g = np.load(f"{golden_dir}/{case}.npz")
        eng = forced_engine(Grid2d.default(int(g["nz"]), int(g["ny"])), _file_modelinfo(g, tmp_path))
        x0 = np.asarray(g["y0"]).reshape(eng.shape)
    x = eng.upload(x0)
    t_eval = np.linspace(0.0, YEAR, 13)
    want = _by_launches(eng, x, t_eval)
    gained = _as_commands(eng, x, t_eval, want)
    assert gained["stream_hist_samples"] >= 12 and gained["stream_hist_drains"] == 1
    if case.endswith("two_waves"):
        assert eng.counter("stream_two_waves_kernel") == 1
    eng.close()


def test_sample_commands_through_the_relay_wave(monkeypatch):
    """NK2D_STREAM_RELAY=1: the commands go through pinned host memory and the relay wave -- the new one as every other"""
    monkeypatch.setenv("NK2D_STREAM_RELAY", "1")
    eng = _iage(52, 52)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 61)
    want = _by_launches(eng, x, t_eval)
    gained = _as_commands(eng, x, t_eval, want)
    assert gained["stream_hist_samples"] >= 60
    eng.close()


def test_a_kernel_that_gives_up_hands_the_sampled_year_back():
    """time limit zero: the kernel's first wait gives up, the year is rerun by launches from x and produces every sample the
    old way; with the limit back the next sampled year is a stream again"""
    eng = _iage(52, 52)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 61)
    want = _by_launches(eng, x, t_eval)
    eng.set_option("stream_years", 1)
    eng.set_option("stream_hist", 1)
    eng.set_option("barrier_timeout_ms", 0)
    fx, st, hist = eng.comp_fcn_hist(x, t_eval)
    assert np.array_equal(hist, want[2]) and np.array_equal(eng.download(fx), want[0])
    assert st["nbarrier_timeouts"] == 1 and eng.counter("stream_timeouts") >= 1 and eng.counter("stream_years_run") == 0
    assert eng.counter("stream_hist_samples") == 0 and eng.counter("stream_hist_drains") == 0
    eng.set_option("barrier_timeout_ms", 2000)
    fx, st, hist = eng.comp_fcn_hist(x, t_eval)
    assert np.array_equal(hist, want[2]) and np.array_equal(eng.download(fx), want[0])
    assert eng.counter("stream_years_run") == 1 and eng.counter("stream_hist_samples") >= 60
    eng.close()


def test_option_off_is_todays_year():
    """the default: a sampled step ends the kernel for its launches, as before the option existed"""
    eng = _iage(52, 52)
    x = eng.upload(_state(eng))
    t_eval = np.linspace(0.0, YEAR, 61)
    want = _by_launches(eng, x, t_eval)
    eng.set_option("stream_years", 1)
    eng.set_option("stream_hist", 0)
    fx, st, hist = eng.comp_fcn_hist(x, t_eval)
    assert np.array_equal(hist, want[2]) and np.array_equal(eng.download(fx), want[0])
    assert eng.counter("stream_years_run") == 1 and eng.counter("stream_launches") >= 50
    assert eng.counter("stream_hist_samples") == 0 and eng.counter("stream_hist_drains") == 0
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception):
            eng.set_option("stream_hist", bad)
    with pytest.raises(Exception):
        eng.set_option("stream_hist_mb", -1)
    eng.close()


def _sampled_year_files(work, nz, ny):
    """iterate.comp_fcn with a history file through the solver mirrors: the bytes of hist_00.nc and fcn_00.nc, and the samples the
    module's engine produced by command"""
    from nk_ooc_amd.model_config import ModelConfig
    from nk_ooc_amd.model_state import ModelState
    from nk_ooc_amd.setup_solver import gen_grid_vars_file, make_config

    os.makedirs(work)
    cfg = make_config(work, nz, ny, tracer_module_names="iage")
    gen_grid_vars_file(cfg["modelinfo"])
    ModelState.reset_class()
    ModelState.model_config_obj = ModelConfig(cfg["modelinfo"])
    ModelState.write_files = True
    try:
        iterate = ModelState("gen_init_iterate")
        iterate.comp_fcn(os.path.join(work, "fcn_00.nc"), None, os.path.join(work, "hist_00.nc"))
        ModelState.flush_files()
        by_command = sum(tms.eng.counter("stream_hist_samples") for tms in iterate.tracer_modules)
        return [open(os.path.join(work, name), "rb").read() for name in ("hist_00.nc", "fcn_00.nc")], by_command
    finally:
        ModelState.reset_class()


def test_through_the_solver_mirrors(tmp_path, monkeypatch):
    """NK2D_STREAM_HIST=1 in the environment of a ModelState: the year that produces F(x) and its history file, byte for byte
    (the files carry a time stamp to the second in their history attribute: the clock stands still for the comparison)"""
    import datetime as dt

    from nk_ooc_amd import ncio

    class _Clock(dt.datetime):
        @classmethod
        def now(cls, tz=None):
            return cls(2001, 1, 1, 12, 0, 0)

    monkeypatch.setattr(ncio, "datetime", _Clock)
    monkeypatch.delenv("NK2D_STREAM_HIST", raising=False)
    off, n_off = _sampled_year_files(str(tmp_path / "work"), 26, 26)
    os.rename(tmp_path / "work", tmp_path / "work_off")       # (the same work directory for both: its name may be in a file)
    monkeypatch.setenv("NK2D_STREAM_HIST", "1")
    on, n_on = _sampled_year_files(str(tmp_path / "work"), 26, 26)
    assert n_off == 0 and n_on >= 60, (n_off, n_on)
    assert len(off[0]) > 61 * 26 * 26 * 8
    assert on[0] == off[0], "hist_00.nc"
    assert on[1] == off[1], "fcn_00.nc"
