"""The one-launch frozen year for the phosphorus module (option "frozen_phosphorus").

A module_kind 1 context at three to eight levels per lane on the lean schedule cache: the workgroup of k_frozen_persistent<E, 1, 0,
PIECES, 1> is one ypos column with its three tracers, a wave each; at the rows where the launch-per-phase path evaluates the
Jacobian anew every wave forms UPR = mu light hs / (po4 + hs)^2 of that column from tracer 0 of the state at the step start.
Values 2 and 3 of the option reach the 256-register flavour (k_frozen_persistent_w2, five to eight levels per lane).

Every criterion is bit for bit against the launch-per-phase year (option "frozen_persistent" 0), the path
tests/test_gpu_oracle_deep_modules.py holds to the oracle for this module: no tolerance is chosen anywhere.

Shapes as in test_gpu_frozen_forced.py: ny = 6, nz = 64 E - 3, a year of 40 days, an error estimate on every 8th step, one engine
per (E, mode) for the whole file.  The inputs are asserted to exercise the state dependence (test_inputs_exercise_...): conditions
on the inputs and on the LAUNCH-PATH results, never on the code under test."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY = 6
DAY = 86400.0
T_RANGE = (0.0, 40.0 * DAY)
STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_phosphorus_years")
# the po4 profile of tests/test_gpu_tape.py's _phos_state times this factor (1: that state; test_inputs_exercise_... holds the
# launch path's year of the state to the conditions it must meet)
PO4_SCALE = 1.0


def _state(grid):
    """a state like _phos_state of tests/test_gpu_tape.py (po4 depleted above 130 m, dop and pop concentrated there, 5 % noise),
    and the perturbed state x + 1e-4 |x| v"""
    nz = len(grid.depth.mid)
    prof = [np.interp(grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3 * PO4_SCALE, 4.1e0 * PO4_SCALE]),
                                                             ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]), ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    rng = np.random.default_rng(12)
    x0 = np.stack([np.broadcast_to(p[:, None], (nz, NY)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, NY)))
    v = np.random.default_rng(5).standard_normal(x0.shape)
    return x0, x0 + 1.0e-4 * np.abs(x0) * v


def _engine(nz, ny=NY, scipy_mode=False):
    """scipy_mode: SciPy's decision mode (the Jacobian is kept from step to step until the Newton iteration slows down), set
    before anything is recorded.  With the default step-size cap (a hundredth of the 40 days) that mode never evaluates the Jacobian
    a second time on this state (measured: 126 of 126 rows reuse the first one), so the mode's engines may take steps of up to a
    quarter of the time range: 47 to 50 rows then, two Jacobian times, five rows with an estimate"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    eng = phosphorus_engine(Grid2d.default(nz, ny), time_range=T_RANGE, **(dict(max_step_frac=0.25) if scipy_mode else {}))
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    eng.set_option("frozen_err_check", 8)
    if scipy_mode:
        eng.set_option("jac_fresh", 0)
        eng.set_option("jac_stage", -1)
    return eng


def _lean_row(E):
    """bytes of a row of the lean cache of these engines: KV and J, 8 (3 kv_len + 5 np) with kv_len = np = ny 64 E"""
    plane = NY * 64 * E
    return 8 * (3 * plane + 5 * plane)


_SHAPES = {}


def _shape(E, scipy_mode=False):
    """one engine per (levels per lane, mode) for the whole file: its recorded year and the launch-per-phase year of the
    perturbed state -- computed once, with the option at 0, left unchanged"""
    key = (E, scipy_mode)
    if key in _SHAPES:
        return _SHAPES[key]
    eng = _engine(64 * E - 3, scipy_mode=scipy_mode)
    x0, xp0 = _state(eng.grid)
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


def _year(ref, state="xp", sched=None):
    """one frozen year with whatever options are set: (result, stats, (one-launch, lean, phosphorus) years it added)"""
    eng = ref["eng"]
    before = [eng.counter(k) for k in COUNTERS]
    fx, st = eng.comp_fcn_frozen(ref[state], ref["sched"] if sched is None else sched)
    return eng.download(fx), st, tuple(eng.counter(k) - b for k, b in zip(COUNTERS, before))


def _reset(eng):
    for key, val in (("frozen_phosphorus", 0), ("frozen_cache_lean", 0), ("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0),
                     ("frozen_coef_lds", 15), ("frozen_by_column", 1), ("frozen_persistent", 1), ("frozen_cache_gb", 128.0),
                     ("barrier_timeout_ms", 2000.0)):
        eng.set_option(key, val)


def _check_stats(ref, st):
    for key in ("nsteps", "nnewton"):
        assert st[key] == ref["st_lpp"][key], key
    assert st["nerr_checked"] >= 2                                   # several rows carried the in-kernel estimate
    # The estimates never reach the year's bits (only the host's check of them), so they are held on their own.  The one-launch year
    # evaluates one on the sampled rows whose solves take ONE sweep, the launch path on those of up to two sweeps (3 of its 16 at
    # E = 3): a subset, row for row the same expressions on the same bits -- the tendency at the step start (tend_at_body's
    # phosphorus sources) among them.  So it cannot count more rows, its largest cannot exceed the launch path's largest, and
    # where both sample the same rows the two are equal to the bit.  (A tendency without the sources made the estimate of row 24
    # exceed 1.5 times the recorded one: such a year is refused with -7 and none of these tests would get here.)
    lpp = ref["st_lpp"]
    print(f"error estimates: {st['nerr_checked']} rows, largest {st['max_err']!r}; launch path {lpp['nerr_checked']} rows, largest {lpp['max_err']!r}")
    assert st["nerr_checked"] <= lpp["nerr_checked"]
    assert 0.0 < st["max_err"] <= lpp["max_err"]
    if st["nerr_checked"] == lpp["nerr_checked"]:
        assert st["max_err"] == lpp["max_err"]


# ---- 1. three to eight levels per lane, one wave per SIMD, on the lean cache
@pytest.mark.parametrize("E", range(3, 9))
def test_phosphorus_takes_the_one_launch_year_on_the_lean_cache(E):
    ref = _shape(E)
    eng, n = ref["eng"], ref["n"]
    try:
        eng.set_option("frozen_cache_lean", 1)
        two = eng.counter("frozen_two_waves_years")
        held = (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds"))
        got, _, took = _year(ref)                                    # the option at 0: today's routing, no cache touched
        assert took == (0, 0, 0) and np.array_equal(got, ref["lpp"])
        assert (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds")) == held
        eng.set_option("frozen_phosphorus", 1)
        got, _, took = _year(ref, "x")                               # the recorded state: the recorded year
        assert took == (1, 1, 1)
        assert np.array_equal(got, ref["want"])
        got, st, took = _year(ref)                                   # a perturbed state: the launch-per-phase year
        assert took == (1, 1, 1)
        assert np.array_equal(got, ref["lpp"])
        _check_stats(ref, st)
        assert eng.counter("frozen_cache_lean") == 1
        assert eng.counter("frozen_cache_bytes") == (n + n // 6 + 16) * _lean_row(E)
        assert eng.counter("frozen_two_waves_years") == two
        eng.set_option("frozen_cache_lean", 2)                       # for such a context always lean: the same cache, no build
        builds = eng.counter("frozen_cache_builds")
        got, _, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"]) and eng.counter("frozen_cache_builds") == builds
        eng.set_option("frozen_cache_lean", 1)
        for bits in (0, 1, 3, 7, 15):                                # whatever lives in LDS: by column all the same
            eng.set_option("frozen_coef_lds", bits)
            got, st, took = _year(ref)
            assert took == (1, 1, 1), bits
            assert np.array_equal(got, ref["lpp"]), bits
            _check_stats(ref, st)
    finally:
        _reset(eng)


# ---- 2. the 256-register flavour
@pytest.mark.parametrize("E", [5, 6, 7, 8])
def test_the_256_register_flavour(E):
    ref = _shape(E)
    eng = ref["eng"]
    eng.set_option("frozen_cache_lean", 1)
    try:
        eng.set_option("frozen_phosphorus", 3)
        two = eng.counter("frozen_two_waves_years")
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1) and np.array_equal(got, ref["want"])
        got, st, took = _year(ref)
        assert took == (1, 1, 1)
        assert np.array_equal(got, ref["lpp"])
        _check_stats(ref, st)
        assert eng.counter("frozen_two_waves_years") - two == 2
        # value 2 at six ypos columns: the flavour of one wave per SIMD is resident and is taken
        eng.set_option("frozen_phosphorus", 2)
        two = eng.counter("frozen_two_waves_years")
        got, _, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"])
        assert eng.counter("frozen_two_waves_years") == two
    finally:
        _reset(eng)


@pytest.mark.parametrize("E", [3, 4])
def test_value_3_below_five_levels_per_lane_is_the_one_wave_flavour(E):
    ref = _shape(E)
    eng = ref["eng"]
    eng.set_option("frozen_cache_lean", 1)
    eng.set_option("frozen_phosphorus", 3)
    try:
        two = eng.counter("frozen_two_waves_years")
        got, _, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"]) and eng.counter("frozen_two_waves_years") == two
    finally:
        _reset(eng)


# ---- 3. pieces
@pytest.mark.parametrize("E,value", [(3, 1), (3, 3), (7, 1), (7, 3)])
def test_pieces_of_seven_rows(E, value):
    """piece boundaries before, on and behind rows with an error estimate (every 8th row): the slab's results in pieces of 7 rows"""
    ref = _shape(E)
    eng, n = ref["eng"], ref["n"]
    B = 7
    carries = [i for i in range(1, n - 1) if i % 8 == 0]
    assert any(i % B == 0 for i in carries) and any(i % B != 0 for i in carries)      # a boundary on such a row, and not
    eng.set_option("frozen_phosphorus", value)
    eng.set_option("frozen_cache_lean", 1)
    try:
        slab, st_slab, took = _year(ref)
        assert took == (1, 1, 1)
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_piece_rows", B)
        two = eng.counter("frozen_two_waves_years")
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1) and np.array_equal(got, ref["want"])
        got, st, took = _year(ref)
        assert took == (1, 1, 1)
        assert np.array_equal(got, slab) and np.array_equal(got, ref["lpp"])
        for key in STATS:
            assert st[key] == st_slab[key], key
        assert eng.counter("frozen_two_waves_years") - two == (2 if (value == 3 and E >= 5) else 0)
        assert eng.counter("frozen_cache_pieces") == math.ceil(n / B)
        assert eng.counter("frozen_cache_bytes") == math.ceil(n / B) * B * _lean_row(E)
    finally:
        _reset(eng)


# ---- 4. SciPy's decision mode: rows that reuse the Jacobian -- and UPR -- of the row before
@pytest.mark.parametrize("E", [4, 7])
def test_scipys_decision_mode(E):
    ref = _shape(E, scipy_mode=True)
    eng, sched = ref["eng"], ref["sched"]
    reused = sched[1:, 4] == sched[:-1, 4]
    print(f"E = {E}: {int(reused.sum())} of {len(sched) - 1} rows reuse the Jacobian of the row before, "
          f"{len(np.unique(sched[:, 4]))} distinct Jacobian times")
    assert reused.sum() >= 1 and len(np.unique(sched[:, 4])) >= 2
    eng.set_option("frozen_phosphorus", 1)
    eng.set_option("frozen_cache_lean", 1)
    try:
        got, _, took = _year(ref, "x")
        assert took == (1, 1, 1) and np.array_equal(got, ref["want"])
        got, st, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"])
        _check_stats(ref, st)
    finally:
        _reset(eng)


# ---- 5. the inputs exercise the state dependence
def _upr(eng, state):
    """jac_core's plane in NumPy: d uptake / d po4 = mu light hs / (po4 + hs)^2"""
    hs, mu = eng.phos["po4_halfsat"], eng.phos["max_uptake_rate"]
    return mu * eng.light_lim * hs / (state[0] + hs) ** 2


@pytest.mark.parametrize("E", range(3, 9))
def test_inputs_exercise_the_state_dependence(E):
    ref = _shape(E)
    eng = ref["eng"]
    # lit: where the light limitation is at least a hundredth of its largest value (uptake is a term of the balance there)
    lit = eng.light_lim >= 1.0e-2 * eng.light_lim.max()
    assert lit.sum() >= NY
    start = _upr(eng, ref["x0"])
    end = _upr(eng, ref["x0"] + ref["want"].reshape(ref["x0"].shape))      # (the recorded year's end state: F(x) = y(T) - x)
    rel = np.abs(end - start)[lit] / np.abs(start)[lit]
    print(f"E = {E}: UPR moves by more than 1e-3 relative in {np.mean(rel > 1.0e-3):.3f} of {int(lit.sum())} lit cells "
          f"(median {np.median(rel):.3e})")
    # a kernel that formed UPR once would go wrong
    assert np.mean(rel > 1.0e-3) >= 0.5
    # ... and so would one that formed it from the recorded state
    assert np.any(_upr(eng, ref["xp0"])[lit] != start[lit])
    # the Jacobian is evaluated anew along the year (the default mode: at every step)
    assert np.all(ref["sched"][1:, 4] != ref["sched"][:-1, 4])


# ---- 6. hand-back
def test_a_year_handed_back_leaves_the_context_clean():
    """a zero hand-over time limit (the library's own mechanism: the first neighbour that is not there yet ends the wait): the year
    is handed back and rerun by the launch-per-phase path to the same bits, nothing is booked for the one-launch year, and the
    context's own UPR and tables are what the launch path left -- a launch-per-phase year afterwards gives the bits it gave"""
    ref = _shape(5)
    eng = ref["eng"]
    eng.set_option("frozen_phosphorus", 1)
    eng.set_option("frozen_cache_lean", 1)
    try:
        got, _, took = _year(ref)
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"])
        two, fb = eng.counter("frozen_two_waves_years"), eng.frozen_fallbacks()
        eng.set_option("barrier_timeout_ms", 0.0)
        got, st, took = _year(ref)
        eng.set_option("barrier_timeout_ms", 2000.0)
        assert np.array_equal(got, ref["lpp"])
        assert took == (0, 0, 0) and eng.counter("frozen_two_waves_years") == two
        assert st["nbarrier_timeouts"] >= 1 and eng.frozen_fallbacks() > fb
        for key in ("nsteps", "nnewton"):                            # nothing booked twice
            assert st[key] == ref["st_lpp"][key], key
        eng.set_option("frozen_persistent", 0)
        got, _, took = _year(ref)
        assert took == (0, 0, 0) and np.array_equal(got, ref["lpp"])
        got, _, _ = _year(ref, "x")
        assert np.array_equal(got, ref["want"])
        eng.set_option("frozen_persistent", 1)
        got, _, took = _year(ref)                                    # and the one-launch year is still there
        assert took == (1, 1, 1) and np.array_equal(got, ref["lpp"])
    finally:
        _reset(eng)


# ---- 7. routing
def test_not_taken_without_the_lean_cache_or_with_single_precision_factors():
    ref = _shape(5)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_phosphorus", 3)
        held = (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds"))
        got, _, took = _year(ref)                                    # "frozen_cache_lean" 0
        assert took == (0, 0, 0) and np.array_equal(got, ref["lpp"])
        assert (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds")) == held      # (no cache built or dropped)
    finally:
        _reset(eng)
    # the single precision factorisation: an engine of its own (the option belongs to the recorded year too)
    eng2 = _engine(64 * 5 - 3)
    try:
        eng2.set_option("factor_fp32", 1)
        x, xp = eng2.upload(ref["x0"]), eng2.upload(ref["xp0"])
        _, _, sched = eng2.comp_fcn(x, record=True)
        eng2.set_option("frozen_persistent", 0)
        fx_l, _ = eng2.comp_fcn_frozen(xp, sched)
        eng2.set_option("frozen_persistent", 1)
        eng2.set_option("frozen_phosphorus", 3)
        eng2.set_option("frozen_cache_lean", 1)
        fx_p, _ = eng2.comp_fcn_frozen(xp, sched)
        assert [eng2.counter(k) for k in COUNTERS] == [0, 0, 0] and eng2.counter("frozen_cache_bytes") == 0
        assert np.array_equal(eng2.download(fx_p), eng2.download(fx_l))
    finally:
        eng2.close()


def test_not_taken_by_a_year_with_history_samples():
    """The public interface has no frozen year with history samples: comp_fcn_hist always runs a free year, which never reaches the
    routing of frozen years.  So this does NOT exercise the `hist_n` clause of frozen_eligible() (it would pass without it); what it
    shows is only that a sampled year computes and counts the same with the option set."""
    ref = _shape(5)
    eng = ref["eng"]
    t_eval = np.linspace(T_RANGE[0], T_RANGE[1], 5)
    try:
        fx0, _, hist0 = eng.comp_fcn_hist(ref["x"], t_eval)
        fx0 = eng.download(fx0)
        eng.set_option("frozen_phosphorus", 3)
        eng.set_option("frozen_cache_lean", 1)
        before = [eng.counter(k) for k in COUNTERS + ("frozen_two_waves_years",)]
        fx1, _, hist1 = eng.comp_fcn_hist(ref["x"], t_eval)
        assert np.array_equal(eng.download(fx1), fx0) and np.array_equal(hist1, hist0)
        assert [eng.counter(k) for k in COUNTERS + ("frozen_two_waves_years",)] == before
    finally:
        _reset(eng)


def test_not_taken_at_one_level_per_lane():
    eng = _engine(22, ny=9)
    try:
        assert (eng.shape[1] + 63) // 64 == 1
        rng = np.random.default_rng(3)
        y0 = np.abs(np.stack([np.full((22, 9), 2.0), np.full((22, 9), 0.1), np.full((22, 9), 0.01)])
                    * (1.0 + 0.05 * rng.standard_normal((3, 22, 9))))
        y = eng.upload(y0)
        _, _, sched = eng.comp_fcn(y, record=True)
        a, _ = eng.comp_fcn_frozen(y, sched)
        a = eng.download(a)
        eng.set_option("frozen_phosphorus", 3)
        eng.set_option("frozen_cache_lean", 1)
        b, _ = eng.comp_fcn_frozen(y, sched)
        assert np.array_equal(eng.download(b), a)
        assert [eng.counter(k) for k in COUNTERS] == [0, 0, 0] and eng.counter("frozen_cache_bytes") == 0
    finally:
        eng.close()


def test_values_outside_0_to_3_are_refused():
    from nk_ooc_amd.engine import Nk2dError

    eng = _shape(5)["eng"]
    for bad in (4, -1, 1.5):
        with pytest.raises(Nk2dError, match="frozen_phosphorus"):
            eng.set_option("frozen_phosphorus", bad)
    eng.set_option("frozen_cache_lean", 1)                           # (where any non-zero value would take the one-launch year)
    try:
        assert _year(_shape(5))[2] == (0, 0, 0)                      # the option is still 0
    finally:
        _reset(eng)


ALL_COUNTERS = COUNTERS + ("frozen_two_waves_years", "frozen_forced_years", "frozen_team_years", "frozen_cache_bytes")


@pytest.mark.parametrize("kind", ["iage", "forced_thres"])
def test_other_modules_are_unaffected(kind):
    """an iage engine and a thresholded forced engine (ny = 6, E = 5): with the option at 3 the years and counters of the option at 0"""
    from nk_ooc_amd.engine import ModuleEngine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz = 64 * 5 - 3
    grid = Grid2d.default(nz, NY)
    rng = np.random.default_rng(11)
    if kind == "iage":
        eng = iage_engine(grid, time_range=T_RANGE)
        col = np.interp(grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (nz, NY))] * 2) + 0.01 * rng.standard_normal((2, nz, NY))
    else:
        rec = np.array([-10.0, 40.0, 95.0, 200.0, 300.0]) * DAY
        restore = 1.0 + 0.2 * rng.standard_normal((5, NY))
        sms = 3.0e-8 * rng.standard_normal((5, nz, NY))
        x0 = 0.6 + 0.2 * rng.standard_normal((1, nz, NY))
        eng = ModuleEngine(grid, tc=1, surf_rate=(24.0 / DAY,), module_kind=2, restore_series=(rec, restore), sms_series=(rec, sms),
                           sink_thres=0.6, time_range=T_RANGE)
    try:
        eng.set_option("device_ctl", 0)
        eng.set_option("frozen_alloc_async", 0)
        eng.set_option("frozen_err_check", 8)
        eng.set_option("frozen_cache_lean", 1)
        if kind == "forced_thres":
            eng.set_option("frozen_forced", 2)
        xp0 = x0 + 1.0e-4 * np.abs(x0) * np.random.default_rng(5).standard_normal(x0.shape)
        x, xp = eng.upload(x0), eng.upload(xp0)
        _, _, sched = eng.comp_fcn(x, record=True)
        outs = []
        for value in (0, 3):
            eng.set_option("frozen_phosphorus", value)
            before = [eng.counter(k) for k in ALL_COUNTERS[:-1]]
            fx, st = eng.comp_fcn_frozen(xp, sched)
            outs.append((eng.download(fx), [st[k] for k in STATS], [eng.counter(k) - b for k, b in zip(ALL_COUNTERS[:-1], before)],
                         eng.counter("frozen_cache_bytes")))
        assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1:] == outs[0][1:]
        assert outs[0][2][0] == 1 and outs[0][2][2] == 0 and outs[0][2][3] == 0      # (they do take the one-launch year, and book no phosphorus year)
    finally:
        eng.close()


# ---- 8. more ypos columns than one wave per SIMD holds (a workgroup of three waves takes a compute unit)
def test_a_grid_that_is_not_resident_at_one_wave_per_simd():
    """ny = 300 at five levels per lane: value 1 does not take the year and allocates no cache (the
    residency is asked before the build); value 2 takes it in the 256-register flavour, two workgroups to a compute unit"""
    ny = 300                                                         # (the MI355X has 256 compute units)
    eng = _engine(64 * 5 - 3, ny=ny)
    try:
        nz = eng.shape[1]
        prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                     ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
        x0 = np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * np.random.default_rng(12).random((3, nz, ny)))
        xp0 = x0 + 1.0e-4 * np.abs(x0) * np.random.default_rng(5).standard_normal(x0.shape)
        x, xp = eng.upload(x0), eng.upload(xp0)
        _, _, sched = eng.comp_fcn(x, record=True)
        eng.set_option("frozen_persistent", 0)
        fx_l, st_l = eng.comp_fcn_frozen(xp, sched)
        lpp = eng.download(fx_l)
        eng.set_option("frozen_persistent", 1)
        eng.set_option("frozen_cache_lean", 1)
        names = COUNTERS + ("frozen_two_waves_years",)
        eng.set_option("frozen_phosphorus", 1)
        fx, _ = eng.comp_fcn_frozen(xp, sched)
        assert np.array_equal(eng.download(fx), lpp)
        assert [eng.counter(k) for k in names] == [0, 0, 0, 0]
        assert eng.counter("frozen_cache_bytes") == 0 and eng.counter("frozen_cache_builds") == 0
        eng.set_option("frozen_phosphorus", 2)
        fx, st = eng.comp_fcn_frozen(xp, sched)
        assert np.array_equal(eng.download(fx), lpp)
        assert [eng.counter(k) for k in names] == [1, 1, 1, 1]
        for key in ("nsteps", "nnewton"):
            assert st[key] == st_l[key], key
        assert 2 <= st["nerr_checked"] <= st_l["nerr_checked"] and 0.0 < st["max_err"] <= st_l["max_err"]      # (see _check_stats)
    finally:
        eng.close()
