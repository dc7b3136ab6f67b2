"""The one-launch frozen year for every file-driven forced module (option "frozen_forced").

Bit 1: a module_kind 2 context without a sink threshold at five to eight levels per lane (k_frozen_persistent<E, 2, ...> for
E = 5 ... 8), on the full and on the lean cache, slab and pieces.  Bit 2: one WITH a sink threshold at one to eight levels per
lane on the lean cache: the year forms UPR = -d sms / d c of each wave's own column, from the state at the step start and the
file source at the row's Jacobian time, at the rows where the launch-per-phase path evaluates the Jacobian anew.

Every criterion is bit for bit against the launch-per-phase year (option "frozen_persistent" 0), the path
tests/test_gpu_oracle_deep_modules.py holds to the oracle for this module: no tolerance is chosen anywhere.

Shapes as in test_gpu_frozen_lean.py: ny = 6, nz = 64 E - 3, an error estimate on every 8th step, one engine per (case, E)
for the whole file.  The thresholded inputs are asserted to exercise the threshold (test_thresholded_inputs_...): conditions on
the inputs and on the LAUNCH-PATH results, never on the code under test."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY = 6
DAY = 86400.0
THRES = 0.6      # the median of the states below: about half the cells lie under the threshold
STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
REC_TIMES = np.array([-10.0, 40.0, 95.0, 200.0, 300.0]) * DAY
T_RANGE = (0.0, 40.0 * DAY)


def _inputs(E):
    """restoring targets, file source (negative on about half the cells: a standard normal field), state, perturbed state"""
    nz = 64 * E - 3
    rng = np.random.default_rng(11)
    restore = 1.0 + 0.2 * rng.standard_normal((5, NY))
    sms = 3.0e-8 * rng.standard_normal((5, nz, NY))
    x0 = 0.6 + 0.2 * rng.standard_normal((1, nz, NY))
    v = np.random.default_rng(5).standard_normal(x0.shape)
    return restore, sms, x0, x0 + 1.0e-4 * np.abs(x0) * v


def _engine(case, E, scipy_mode=False):
    """case "linear": KIND 2 without a sink threshold; "thres": with one.  scipy_mode: SciPy's decision mode (the Jacobian is
    kept from step to step until the Newton iteration slows down), set before anything is recorded"""
    from nk_ooc_amd.engine import ModuleEngine
    from nk_ooc_amd.grid import Grid2d

    restore, sms, x0, xp0 = _inputs(E)
    eng = ModuleEngine(Grid2d.default(64 * E - 3, NY), tc=1, surf_rate=(24.0 / DAY,), module_kind=2, restore_series=(REC_TIMES, restore),
                       sms_series=(REC_TIMES, sms), sink_thres=THRES if case == "thres" else None, time_range=T_RANGE)
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    eng.set_option("frozen_err_check", 8)
    if scipy_mode:
        eng.set_option("jac_fresh", 0)
        eng.set_option("jac_stage", -1)
    return eng, x0, xp0


def _sizes(E):
    """bytes of a full row, of a lean row and of a plane of the cache of these engines (one tracer; kv_len = 2 plane + ny)"""
    plane = NY * 64 * E
    nv, ntab, kv_len = plane, NY * 14 * 64, 2 * plane + NY
    return 8 * (3 * kv_len + 5 * plane + 3 * nv + 3 * ntab), 8 * (3 * kv_len + 5 * plane), 8 * plane


_SHAPES = {}


def _shape(case, E, scipy_mode=False):
    """one engine per (case, levels per lane, mode) for the whole file: its recorded year and the launch-per-phase year of the
    perturbed state -- computed once, with the option at 0, left unchanged"""
    key = (case, E, scipy_mode)
    if key in _SHAPES:
        return _SHAPES[key]
    eng, x0, xp0 = _engine(case, E, scipy_mode)
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    ref = dict(eng=eng, x0=x0, xp0=xp0, x=x, xp=xp, sched=sched, n=len(sched), want=eng.download(fx))
    eng.set_option("frozen_persistent", 0)
    fx_l, ref["st_lpp"] = eng.comp_fcn_frozen(xp, sched)
    ref["lpp"] = eng.download(fx_l)
    eng.set_option("frozen_persistent", 1)
    _SHAPES[key] = ref
    return ref


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ref in _SHAPES.values():
        ref["eng"].close()
    _SHAPES.clear()


COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_forced_years")


def _year(ref, state="xp", sched=None):
    """one frozen year with whatever options are set: (result, stats, (one-launch, lean, forced) years it added)"""
    eng = ref["eng"]
    before = [eng.counter(k) for k in COUNTERS]
    fx, st = eng.comp_fcn_frozen(ref[state], ref["sched"] if sched is None else sched)
    return eng.download(fx), st, tuple(eng.counter(k) - b for k, b in zip(COUNTERS, before))


def _reset(eng):
    for key, val in (("frozen_forced", 0), ("frozen_cache_lean", 0), ("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0),
                     ("frozen_coef_lds", 15), ("frozen_by_column", 1), ("frozen_persistent", 1), ("frozen_cache_gb", 128.0)):
        eng.set_option(key, val)


def _check_stats(ref, st):
    for key in ("nsteps", "nnewton"):
        assert st[key] == ref["st_lpp"][key], key
    assert st["nerr_checked"] >= 2                                   # several rows carried the in-kernel estimate


# ---- 1. linear sources, five to eight levels per lane (bit 1)
@pytest.mark.parametrize("E", [5, 6, 7, 8])
def test_linear_forced_module_takes_the_one_launch_year_above_four_levels_per_lane(E):
    ref = _shape("linear", E)
    eng, n = ref["eng"], ref["n"]
    full_row, lean_row, _ = _sizes(E)
    cap = n + n // 6 + 16
    try:
        got, _, took = _year(ref)                                    # the option at 0: today's routing
        assert took == (0, 0, 0) and eng.counter("frozen_cache_bytes") == 0 and np.array_equal(got, ref["lpp"])
        eng.set_option("frozen_forced", 1)
        got, _, took = _year(ref, "x")                               # the recorded state: the recorded year
        assert took == (1, 0, 1)
        assert np.array_equal(got, ref["want"])
        full, st_full, took = _year(ref)                             # a perturbed state: the launch-per-phase year
        assert took == (1, 0, 1)
        assert np.array_equal(full, ref["lpp"])
        _check_stats(ref, st_full)
        assert eng.counter("frozen_cache_lean") == 0 and eng.counter("frozen_cache_bytes") == cap * full_row
        eng.set_option("frozen_cache_lean", 1)
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1) and np.array_equal(got, ref["want"])
        lean, st_lean, took = _year(ref)
        assert took == (1, 1, 1)
        assert np.array_equal(lean, full) and np.array_equal(lean, ref["lpp"])
        for key in STATS:
            assert st_lean[key] == st_full[key], key
        assert st_lean["nlaunch"] == st_full["nlaunch"]
        assert eng.counter("frozen_cache_lean") == 1 and eng.counter("frozen_cache_bytes") == cap * lean_row
    finally:
        _reset(eng)


# ---- 2. what lives in LDS (by column: a workgroup of ONE wave per ypos column)
@pytest.mark.parametrize("E,bits", [(E, b) for E in (5, 7) for b in (0, 3, 7, 15)])
def test_linear_whatever_lives_in_lds(E, bits):
    ref = _shape("linear", E)
    eng = ref["eng"]
    eng.set_option("frozen_forced", 1)
    eng.set_option("frozen_coef_lds", bits)
    try:
        for lean in (0, 1):
            eng.set_option("frozen_cache_lean", lean)
            got, _, took = _year(ref, "x")
            assert took == (1, lean, 1) and np.array_equal(got, ref["want"])
            got, st, took = _year(ref)
            assert took == (1, lean, 1) and np.array_equal(got, ref["lpp"])
            _check_stats(ref, st)
    finally:
        _reset(eng)


# ---- 3. a thresholded sink, one to eight levels per lane (bit 2, lean cache): the four-wave team (E = 1, 2), adjacent columns
# (3, 4), by column (5 ... 8)
@pytest.mark.parametrize("E", range(1, 9))
def test_thresholded_forced_module_takes_the_one_launch_year_on_the_lean_cache(E):
    ref = _shape("thres", E)
    eng, n = ref["eng"], ref["n"]
    _, lean_row, plane = _sizes(E)
    try:
        got, _, took = _year(ref)                                    # the option at 0: today's routing
        assert took == (0, 0, 0) and np.array_equal(got, ref["lpp"])
        eng.set_option("frozen_forced", 2)
        got, _, took = _year(ref)                                    # the full cache of such a context does not exist: as today
        assert took == (0, 0, 0) and eng.counter("frozen_cache_bytes") == 0 and np.array_equal(got, ref["lpp"])
        eng.set_option("frozen_cache_lean", 1)
        teams = eng.counter("frozen_team_years")
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1)
        assert np.array_equal(got, ref["want"])
        got, st, took = _year(ref)
        assert took == (1, 1, 1)
        assert np.array_equal(got, ref["lpp"])
        _check_stats(ref, st)
        assert eng.counter("frozen_team_years") - teams == (2 if E <= 2 else 0)
        assert eng.counter("frozen_cache_lean") == 1
        assert eng.counter("frozen_cache_bytes") == (n + n // 6 + 16) * (lean_row + plane)
        eng.set_option("frozen_cache_lean", 2)                       # for such a context always lean: the same cache, no build
        builds = eng.counter("frozen_cache_builds")
        got, _, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"]) and eng.counter("frozen_cache_builds") == builds
    finally:
        _reset(eng)


# ---- 4. the inputs exercise the threshold
def _on(state, sms_plane):
    """jac_core's condition: the sink is scaled down where the source is a sink and the tracer lies below the threshold"""
    r = state / THRES
    return (sms_plane < 0.0) & (r > 0.0) & (r < 1.0)


def _sms_at(E, t):
    _, sms, _, _ = _inputs(E)
    k = min(max(int(np.searchsorted(REC_TIMES, t)), 1), len(REC_TIMES) - 1)
    return sms[k - 1] + (sms[k] - sms[k - 1]) * ((t - REC_TIMES[k - 1]) / (REC_TIMES[k] - REC_TIMES[k - 1]))


@pytest.mark.parametrize("E", range(1, 9))
def test_thresholded_inputs_exercise_the_threshold(E):
    ref = _shape("thres", E)
    sched = ref["sched"]
    on_start = _on(ref["x0"][0], _sms_at(E, sched[0, 4]))
    on_pert = _on(ref["xp0"][0], _sms_at(E, sched[0, 4]))
    on_end = _on(ref["lpp"].reshape(ref["x0"].shape)[0], _sms_at(E, sched[-1, 4]))     # (the launch path's end-of-year state)
    for on in (on_start, on_pert, on_end):
        assert 0.10 < on.mean() < 0.90, on.mean()
    # a kernel that formed UPR once would go wrong: the on-set moves in at least half the columns
    moved = np.any(on_end != on_pert, axis=0)
    assert moved.sum() >= NY / 2, moved
    # and the Jacobian is evaluated anew along the year (the default mode: at every step start)
    assert np.all(sched[1:, 4] != sched[:-1, 4])


# ---- 5. SciPy's decision mode: rows that reuse the Jacobian -- and UPR -- of the row before
@pytest.mark.parametrize("E", [1, 7])
def test_thresholded_in_scipys_decision_mode(E):
    ref = _shape("thres", E, scipy_mode=True)
    eng, sched = ref["eng"], ref["sched"]
    reused = sched[1:, 4] == sched[:-1, 4]
    print(f"E = {E}: {int(reused.sum())} of {len(sched) - 1} rows reuse the Jacobian of the row before")
    assert reused.any(), (int(reused.sum()), len(sched))
    eng.set_option("frozen_forced", 2)
    eng.set_option("frozen_cache_lean", 1)
    try:
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1) and np.array_equal(got, ref["want"])
        got, st, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"])
        _check_stats(ref, st)
    finally:
        _reset(eng)


# ---- 6. pieces
@pytest.mark.parametrize("case,B", [(c, b) for c in ("linear", "thres") for b in (1, 7)])
def test_pieces_at_seven_levels_per_lane(case, B):
    """piece boundaries before, on and behind rows with an error estimate: the slab's results in pieces of B rows"""
    ref = _shape(case, 7)
    eng, n = ref["eng"], ref["n"]
    full_row, lean_row, plane = _sizes(7)
    eng.set_option("frozen_forced", 1 if case == "linear" else 2)
    try:
        for lean in ((0, 1) if case == "linear" else (1,)):
            eng.set_option("frozen_cache_pieces", 0)
            eng.set_option("frozen_cache_lean", lean)
            slab, st_slab, took = _year(ref)
            assert took == (1, lean, 1)
            eng.set_option("frozen_cache_pieces", 1)
            eng.set_option("frozen_cache_piece_rows", B)
            got, _, took = _year(ref, "x")
            assert took == (1, lean, 1) and np.array_equal(got, ref["want"])
            got, st, took = _year(ref)
            assert took == (1, lean, 1)
            assert np.array_equal(got, slab) and np.array_equal(got, ref["lpp"])
            for key in STATS:
                assert st[key] == st_slab[key], key
            row = (lean_row + (plane if case == "thres" else 0)) if lean else full_row
            assert eng.counter("frozen_cache_pieces") == math.ceil(n / B)
            assert eng.counter("frozen_cache_bytes") == math.ceil(n / B) * B * row
    finally:
        _reset(eng)


# ---- 7. the benchmarked depth: 416 levels, the thresholded module of tests/golden/forced_file_sink_thres_416x4.npz
def test_product_on_frozen_years_at_416_levels(golden_dir, tmp_path):
    from test_gpu_oracle_deep_modules import _case, _direction, _regions

    make, x0, _, _ = _case("forced_416x4", golden_dir, tmp_path)
    eng = make()
    try:
        _regions(eng)
        assert eng.state_dependent_precond and (eng.shape[1] + 63) // 64 == 7
        eng.set_option("stream_years", 0)
        eng.set_option("frozen_alloc_async", 0)
        x = eng.upload(x0)
        vd = eng.upload(_direction("forced", x0))
        vd = eng.scale(vd, 1.0 / np.sqrt(eng.dot(vd, vd)))
        fx, _, sched = eng.comp_fcn(x, record=True)
        eng.set_option("frozen_persistent", 0)
        w_l, sigma_l, st_l = eng.jvp(x, fx, vd, sched=sched)
        w_l = eng.download(w_l)
        eng.set_option("frozen_persistent", 1)
        eng.set_option("frozen_forced", 2)
        eng.set_option("frozen_cache_lean", 1)
        before = [eng.counter(k) for k in COUNTERS]
        products = 2
        for _ in range(products):
            w_f, sigma_f, st_f = eng.jvp(x, fx, vd, sched=sched)
            assert np.array_equal(sigma_f, sigma_l)
            assert np.array_equal(eng.download(w_f), w_l)
            assert st_f["nsteps"] == st_l["nsteps"] and st_f["nrejected"] == 0
        assert [eng.counter(k) - b for k, b in zip(COUNTERS, before)] == [products] * 3     # one perturbed year per product
        assert eng.frozen_fallbacks() == 0
    finally:
        eng.close()


# ---- 8. the safety net, and the context afterwards
def _safety_net(eng, x, sched, bad):
    """the starved schedule, then a zero barrier time-out on the good one: results and what the safety net counted"""
    res0, fb0 = eng.frozen_resumes(), eng.frozen_fallbacks()
    fx, st = eng.comp_fcn_frozen(x, bad)
    out = [eng.download(fx), st["nresumed"], eng.frozen_resumes() - res0, eng.frozen_fallbacks() - fb0]
    eng.set_option("barrier_timeout_ms", 0.0)
    fx, st = eng.comp_fcn_frozen(x, sched)
    out += [eng.download(fx), st["nbarrier_timeouts"]]
    eng.set_option("barrier_timeout_ms", 2000.0)
    return out


def test_thresholded_safety_net_and_a_clean_context():
    """Newton iterations taken away at a step in the middle of the year: the one-launch year is handed back and resumed as the
    launch-per-phase year is; so is one whose hand-over times out; and the context -- its own UPR included -- is then what
    a fresh one is"""
    ref = _shape("thres", 1)
    sched = ref["sched"]
    bad = sched.copy()
    half = len(bad) // 2
    k = half + int(np.argmax(bad[half:, 3]))          # (the step with the most iterations keeps one)
    drop = int(bad[k, 3]) - 1
    assert drop >= 1
    bad[k, 3] -= drop
    outs = {}
    for flag in (0, 2):
        eng, x0, _ = _engine("thres", 1)
        eng.set_option("frozen_forced", flag)
        eng.set_option("frozen_cache_lean", 1)
        x = eng.upload(x0)
        fx, _, sched_f = eng.comp_fcn(x, record=True)
        assert np.array_equal(sched_f, sched) and np.array_equal(eng.download(fx), ref["want"])
        outs[flag] = _safety_net(eng, x, sched, bad)
        assert eng.counter("frozen_cache_lean") == (1 if flag else 0)
        # a free-running year on the context gives the bits it gives on a fresh context, and so does a frozen year
        fx2, _, sched2 = eng.comp_fcn(x, record=True)
        assert np.array_equal(eng.download(fx2), ref["want"]) and np.array_equal(sched2, sched)
        years = eng.counter("frozen_forced_years")
        fx3, _ = eng.comp_fcn_frozen(x, sched)
        assert np.array_equal(eng.download(fx3), ref["want"])
        assert eng.counter("frozen_forced_years") - years == (1 if flag else 0)
        eng.set_option("frozen_persistent", 0)
        fx4, _ = eng.comp_fcn_frozen(x, sched)
        assert np.array_equal(eng.download(fx4), ref["want"])
        eng.close()
    off, on = outs[0], outs[2]
    assert np.array_equal(on[0], off[0]) and on[1:4] == off[1:4]
    if drop >= 2:
        assert on[1] >= 1 or on[3] >= 1                              # (the net was needed)
    assert np.array_equal(on[4], off[4]) and np.array_equal(on[4], ref["want"]) and on[5] >= 1


# ---- 9. refusals
def test_refusals():
    from nk_ooc_amd.engine import Nk2dError, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    ref = _shape("thres", 1)
    eng = ref["eng"]
    for bad in (4, -1, 1.5):
        with pytest.raises(Nk2dError, match="frozen_forced"):
            eng.set_option("frozen_forced", bad)
    # the single precision factorisation: no one-launch year, the year is the launch path's
    eng2, x0, xp0 = _engine("thres", 1)
    eng2.set_option("factor_fp32", 1)
    eng2.set_option("frozen_forced", 3)
    eng2.set_option("frozen_cache_lean", 1)
    x, xp = eng2.upload(x0), eng2.upload(xp0)
    fx, _, sched = eng2.comp_fcn(x, record=True)
    fx_p, _ = eng2.comp_fcn_frozen(xp, sched)
    assert [eng2.counter(k) for k in COUNTERS] == [0, 0, 0] and eng2.counter("frozen_cache_bytes") == 0
    eng2.set_option("frozen_persistent", 0)
    fx_l, _ = eng2.comp_fcn_frozen(xp, sched)
    assert np.array_equal(eng2.download(fx_p), eng2.download(fx_l))
    eng2.close()
    # phosphorus: bit 2 changes nothing
    ph = phosphorus_engine(Grid2d.default(61, NY), time_range=T_RANGE)
    try:
        ph.set_option("device_ctl", 0)
        ph.set_option("stream_years", 0)
        rng = np.random.default_rng(3)
        y0 = np.abs(np.stack([np.full((61, NY), 2.0), np.full((61, NY), 0.1), np.full((61, NY), 0.01)])
                    * (1.0 + 0.05 * rng.standard_normal((3, 61, NY))))
        y = ph.upload(y0)
        _, _, sched = ph.comp_fcn(y, record=True)
        a, _ = ph.comp_fcn_frozen(y, sched)
        a = ph.download(a)
        ph.set_option("frozen_forced", 2)
        ph.set_option("frozen_cache_lean", 1)
        b, _ = ph.comp_fcn_frozen(y, sched)
        assert np.array_equal(ph.download(b), a)
        assert [ph.counter(k) for k in COUNTERS] == [0, 0, 0] and ph.counter("frozen_cache_bytes") == 0
    finally:
        ph.close()
