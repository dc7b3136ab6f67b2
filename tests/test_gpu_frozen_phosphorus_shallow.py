"""The one-launch frozen year for the phosphorus module at ONE and TWO levels per lane (option "frozen_phosphorus_shallow",
DESIGN.md section 3.6.4): up to 128 depth levels, the grids the model is shipped with.

With the option at 1 -- and "frozen_phosphorus" non-zero on the lean cache -- a module_kind 1 context at these depths runs
k_frozen_persistent<1 or 2, 1, 0, PIECES, 1>: the workgroup is one ypos column with its three tracers, a wave each and never a team,
nothing of the year in LDS; every wave forms UPR of that column at the rows where the launch-per-phase path evaluates the Jacobian
anew.  With the option at 0 nothing changes.

Every criterion is bit for bit against the launch-per-phase year (option "frozen_persistent" 0) of the same engine: no tolerance is
chosen anywhere (the one tolerance below, against the reference's own year, is test_phosphorus_comp_fcn's).

Shapes, state, engine options and helpers as in tests/test_gpu_frozen_phosphorus.py: ny = 6; nz = 61 and 125 (64 E - 3: the last
lane partly empty) and 64 and 128 (every lane full); a year of 40 days, an error estimate on every 8th step, one engine per
(shape, mode) for the whole file, options reset in `finally`."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY = 6
DAY = 86400.0
T_RANGE = (0.0, 40.0 * DAY)
T_RANGE_SCIPY = (0.0, 80.0 * DAY)
NZS = (61, 125, 64, 128)
STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_phosphorus_years")
SHALLOW = "frozen_phosphorus_shallow_years"
OTHERS = ("frozen_team_years", "frozen_two_waves_years", "frozen_lds_bits")


def _state(grid, ny=NY):
    """_state of tests/test_gpu_frozen_phosphorus.py (po4 depleted above 130 m, dop and pop concentrated there, 5 % noise), and the
    perturbed state x + 1e-4 |x| v"""
    nz = len(grid.depth.mid)
    prof = [np.interp(grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                             ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    rng = np.random.default_rng(12)
    x0 = np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, ny)))
    v = np.random.default_rng(5).standard_normal(x0.shape)
    return x0, x0 + 1.0e-4 * np.abs(x0) * v


def _engine(nz, ny=NY, scipy_mode=False, time_range=T_RANGE, err_check=8):
    """scipy_mode: SciPy's decision mode (the Jacobian is kept from step to step until the Newton iteration slows down), set before
    anything is recorded, with steps of up to a quarter of the time range.  time_range None: the full year; err_check None: the
    library's default stride"""
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    kw = dict(max_step_frac=0.25) if scipy_mode else {}
    if time_range is not None:
        kw["time_range"] = time_range
    eng = phosphorus_engine(Grid2d.default(nz, ny), **kw)
    assert (eng.shape[1] + 63) // 64 in (1, 2)
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    if err_check is not None:
        eng.set_option("frozen_err_check", err_check)
    if scipy_mode:
        eng.set_option("jac_fresh", 0)
        eng.set_option("jac_stage", -1)
    return eng


def _lean_row(nz, ny=NY):
    """bytes of a row of the lean cache: KV and J, 8 (3 kv_len + 5 np) with kv_len = np = ny 64 E"""
    plane = ny * 64 * ((nz + 63) // 64)
    return 8 * (3 * plane + 5 * plane)


def _record(eng, x0, xp0):
    """the recorded year of x0 and the launch-per-phase year of the perturbed state on its schedule -- with every option at its
    default, computed once, left unchanged"""
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    ref = dict(eng=eng, x0=x0, xp0=xp0, x=x, xp=xp, fx=fx, sched=sched, n=len(sched), want=eng.download(fx))
    eng.set_option("frozen_persistent", 0)
    fx_l, ref["st_lpp"] = eng.comp_fcn_frozen(xp, sched)
    ref["lpp"] = eng.download(fx_l)
    eng.set_option("frozen_persistent", 1)
    return ref


_SHAPES = {}


def _shape(nz, scipy_mode=False, ny=NY):
    """one engine per (nz, mode, ny) for the whole file"""
    key = (nz, scipy_mode, ny)
    if key not in _SHAPES:
        eng = _engine(nz, ny=ny, scipy_mode=scipy_mode, time_range=T_RANGE_SCIPY if scipy_mode else T_RANGE)
        _SHAPES[key] = _record(eng, *_state(eng.grid, ny))
    return _SHAPES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ref in _SHAPES.values():
        ref["eng"].close()
    _SHAPES.clear()


def _year(ref, state="xp"):
    """one frozen year with whatever options are set: (result, stats, (one-launch, lean, phosphorus) years it added, shallow years
    it added)"""
    eng = ref["eng"]
    before = [eng.counter(k) for k in COUNTERS + (SHALLOW,)]
    fx, st = eng.comp_fcn_frozen(ref[state], ref["sched"])
    took = tuple(eng.counter(k) - b for k, b in zip(COUNTERS + (SHALLOW,), before))
    return eng.download(fx), st, took[:3], took[3]


def _reset(eng):
    for key, val in (("frozen_phosphorus_shallow", 0), ("frozen_phosphorus", 0), ("frozen_cache_lean", 0), ("frozen_cache_pieces", 0),
                     ("frozen_cache_piece_rows", 0), ("frozen_coef_lds", 63), ("frozen_by_column", 1), ("frozen_team", 1),
                     ("frozen_persistent", 1), ("frozen_cache_gb", 128.0), ("barrier_timeout_ms", 2000.0)):
        eng.set_option(key, val)


def _on(eng, value=1, lean=1):
    eng.set_option("frozen_phosphorus", value)
    eng.set_option("frozen_cache_lean", lean)
    eng.set_option("frozen_phosphorus_shallow", 1)


def _check_stats(ref, st):
    """as _check_stats of tests/test_gpu_frozen_phosphorus.py: the one-launch year evaluates an estimate on the sampled rows whose
    solves take ONE sweep, the launch path on those of up to two -- a subset, row for row the same expressions on the same bits"""
    lpp = ref["st_lpp"]
    for key in ("nsteps", "nnewton"):
        assert st[key] == lpp[key], key
    print(f"error estimates: {st['nerr_checked']} rows, largest {st['max_err']!r}; launch path {lpp['nerr_checked']} rows, largest {lpp['max_err']!r}")
    assert st["nerr_checked"] >= 2
    assert st["nerr_checked"] <= lpp["nerr_checked"]
    assert 0.0 < st["max_err"] <= lpp["max_err"]
    if st["nerr_checked"] == lpp["nerr_checked"]:
        assert st["max_err"] == lpp["max_err"]


def _takes_both_years(ref, check_stats=True):
    """the recorded state gives the recorded year, the perturbed state the launch-path year; one year of every kind is booked, no
    team year, no two-waves year, nothing in LDS"""
    eng = ref["eng"]
    others = [eng.counter(k) for k in OTHERS]
    got, _, took, shallow = _year(ref, "x")
    assert took == (1, 1, 1) and shallow == 1
    assert np.array_equal(got, ref["want"])
    got, st, took, shallow = _year(ref)
    assert took == (1, 1, 1) and shallow == 1
    assert np.array_equal(got, ref["lpp"])
    assert [eng.counter(k) for k in OTHERS] == others
    if check_stats:
        _check_stats(ref, st)
    else:
        for key in ("nsteps", "nnewton"):
            assert st[key] == ref["st_lpp"][key], key
    return st


# ---- 1. the option at 0 changes nothing
@pytest.mark.parametrize("nz", NZS)
def test_option_0_changes_nothing(nz):
    ref = _shape(nz)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_phosphorus", 1)
        eng.set_option("frozen_cache_lean", 1)
        held = (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds"))
        others = [eng.counter(k) for k in OTHERS]
        got, st, took, shallow = _year(ref)
        assert took == (0, 0, 0) and shallow == 0
        assert np.array_equal(got, ref["lpp"])
        for key in STATS:
            assert st[key] == ref["st_lpp"][key], key
        assert (eng.counter("frozen_cache_bytes"), eng.counter("frozen_cache_builds")) == held
        assert [eng.counter(k) for k in OTHERS] == others
        got, _, took, shallow = _year(ref, "x")
        assert took == (0, 0, 0) and shallow == 0 and np.array_equal(got, ref["want"])
    finally:
        _reset(eng)


# ---- 2. the option at 1 takes the year
@pytest.mark.parametrize("nz", NZS)
def test_option_1_takes_the_year(nz):
    ref = _shape(nz)
    eng, n = ref["eng"], ref["n"]
    try:
        _on(eng)
        _takes_both_years(ref)
        assert eng.counter("frozen_cache_lean") == 1
        assert eng.counter("frozen_cache_bytes") == (n + n // 6 + 16) * _lean_row(nz)
        assert eng.counter("frozen_lds_bits") == 0
    finally:
        _reset(eng)


# ---- 3. cache settings and flavours
@pytest.mark.parametrize("nz", NZS)
def test_cache_settings_and_flavours(nz):
    ref = _shape(nz)
    eng, n = ref["eng"], ref["n"]
    try:
        _on(eng)
        slab, st_slab, took, shallow = _year(ref)
        assert took == (1, 1, 1) and shallow == 1 and np.array_equal(slab, ref["lpp"])
        eng.set_option("frozen_cache_lean", 2)                       # for such a context always lean: the same cache, no build
        builds = eng.counter("frozen_cache_builds")
        got, _, took, shallow = _year(ref)
        assert took == (1, 1, 1) and shallow == 1 and np.array_equal(got, ref["lpp"]) and eng.counter("frozen_cache_builds") == builds
        eng.set_option("frozen_cache_lean", 1)
        two = eng.counter("frozen_two_waves_years")
        for value in (2, 3):                                         # no 256-register flavour at these depths: the one-wave flavour
            eng.set_option("frozen_phosphorus", value)
            got, st, took, shallow = _year(ref)
            assert took == (1, 1, 1) and shallow == 1, value
            assert np.array_equal(got, ref["lpp"]), value
            _check_stats(ref, st)
        assert eng.counter("frozen_two_waves_years") == two
        eng.set_option("frozen_phosphorus", 1)
        team = eng.counter("frozen_team_years")
        for key, values, default in (("frozen_coef_lds", (0, 15, 63), 63), ("frozen_by_column", (0,), 1), ("frozen_team", (0, 1), 1)):
            for value in values:
                eng.set_option(key, value)
                got, st, took, shallow = _year(ref)
                assert took == (1, 1, 1) and shallow == 1, (key, value)
                assert np.array_equal(got, ref["lpp"]), (key, value)
                assert eng.counter("frozen_lds_bits") == 0, (key, value)
            eng.set_option(key, default)
        assert eng.counter("frozen_team_years") == team
        carries = [i for i in range(1, n - 1) if i % 8 == 0]
        eng.set_option("frozen_cache_pieces", 1)
        for B in (7, 16):          # piece boundaries before, on and behind rows with an error estimate (every 8th row)
            assert any(i % B == 0 for i in carries) and (B == 16 or any(i % B != 0 for i in carries))
            eng.set_option("frozen_cache_piece_rows", B)
            got, _, took, shallow = _year(ref, "x")
            assert took == (1, 1, 1) and shallow == 1 and np.array_equal(got, ref["want"]), B
            got, st, took, shallow = _year(ref)
            assert took == (1, 1, 1) and shallow == 1, B
            assert np.array_equal(got, slab), B
            for key in STATS:
                assert st[key] == st_slab[key], (B, key)
            assert eng.counter("frozen_cache_pieces") == math.ceil(n / B)
            assert eng.counter("frozen_cache_bytes") == math.ceil(n / B) * B * _lean_row(nz)
    finally:
        _reset(eng)


# ---- 4. SciPy's decision mode: rows that reuse the Jacobian -- and UPR -- of the row before
@pytest.mark.parametrize("nz", [61, 125, 128])
def test_scipys_decision_mode(nz):
    """a time range of 80 days: at 40 the mode never evaluates the Jacobian a second time at nz = 125 (the CPU oracle's year,
    whatever the step cap); at 80 the oracle's year has 41, 46 and 47 rows with two Jacobian times at nz = 61, 125 and 128"""
    ref = _shape(nz, scipy_mode=True)
    eng, sched = ref["eng"], ref["sched"]
    reused = sched[1:, 4] == sched[:-1, 4]
    print(f"nz = {nz}: {len(sched)} rows, {int(reused.sum())} reuse the Jacobian of the row before, "
          f"{len(np.unique(sched[:, 4]))} distinct Jacobian times")
    assert len(np.unique(sched[:, 4])) >= 2 and reused.sum() >= 1
    try:
        _on(eng)
        _takes_both_years(ref)
    finally:
        _reset(eng)


# ---- 5. the inputs exercise the state dependence (inputs and launch-path results only)
def _upr(eng, state):
    """jac_core's plane in NumPy: d uptake / d po4 = mu light hs / (po4 + hs)^2"""
    hs, mu = eng.phos["po4_halfsat"], eng.phos["max_uptake_rate"]
    return mu * eng.light_lim * hs / (state[0] + hs) ** 2


@pytest.mark.parametrize("nz", NZS)
def test_inputs_exercise_the_state_dependence(nz):
    ref = _shape(nz)
    eng = ref["eng"]
    # lit: where the light limitation is at least a hundredth of its largest value (uptake is a term of the balance there)
    lit = eng.light_lim >= 1.0e-2 * eng.light_lim.max()
    assert lit.sum() >= NY
    start = _upr(eng, ref["x0"])
    end = _upr(eng, ref["x0"] + ref["want"].reshape(ref["x0"].shape))      # (the recorded year's end state: F(x) = y(T) - x)
    rel = np.abs(end - start)[lit] / np.abs(start)[lit]
    print(f"nz = {nz}: UPR moves by more than 1e-3 relative in {np.mean(rel > 1.0e-3):.3f} of {int(lit.sum())} lit cells "
          f"(median {np.median(rel):.3e})")
    # a kernel that formed UPR once would go wrong
    assert np.mean(rel > 1.0e-3) >= 0.5
    # ... and so would one that formed it from the recorded state
    assert np.any(_upr(eng, ref["xp0"])[lit] != start[lit])
    # the Jacobian is evaluated anew along the year (the default mode: at every step)
    assert np.all(ref["sched"][1:, 4] != ref["sched"][:-1, 4])


# ---- 6. few and many columns
def test_two_columns():
    """ny = 2: every workgroup has one neighbour"""
    ref = _shape(61, ny=2)
    eng = ref["eng"]
    try:
        _on(eng)
        _takes_both_years(ref)
    finally:
        _reset(eng)


def test_the_shipped_grid_over_the_full_year():
    """depth_nlevs 40, 50 ypos columns, the full year, the library's default stride of error estimates"""
    eng = _engine(40, ny=50, time_range=None, err_check=None)
    try:
        ref = _record(eng, *_state(eng.grid, 50))
        _on(eng)
        _takes_both_years(ref, check_stats=False)
        assert eng.counter("frozen_cache_bytes") == (ref["n"] + ref["n"] // 6 + 16) * _lean_row(40, 50)
    finally:
        eng.close()


# ---- 7. products
def test_products():
    """finite-difference products on the installed schedule, a chain of three directions (each the product of the one before): the
    numbers of the option at 0, one shallow year per product"""
    ref = _shape(61)
    eng = ref["eng"]
    v0 = 1.0e-2 * np.abs(ref["x0"]) * np.random.default_rng(21).standard_normal(ref["x0"].shape)
    try:
        eng.set_option("frozen_phosphorus", 1)
        eng.set_option("frozen_cache_lean", 1)
        eng.set_frozen_schedule(ref["sched"])
        outs = []
        for value in (0, 1):
            eng.set_option("frozen_phosphorus_shallow", value)
            before = [eng.counter(k) for k in COUNTERS + (SHALLOW,)]
            v, chain = eng.upload(v0), []
            for _ in range(3):
                v, sigma, _ = eng.jvp(ref["x"], ref["fx"], v)
                chain.append((eng.download(v), sigma.copy()))
            assert [eng.counter(k) - b for k, b in zip(COUNTERS + (SHALLOW,), before)] == [3 * value] * 4
            outs.append(chain)
        for (w0, s0), (w1, s1) in zip(*outs):
            assert np.all(np.isfinite(w0)) and np.any(w0 != 0.0)
            assert np.array_equal(w1, w0) and np.array_equal(s1, s0)
    finally:
        eng.set_frozen_schedule(None)
        _reset(eng)


# ---- 8. hand-back
def test_a_year_handed_back_leaves_the_context_clean():
    """a zero hand-over time limit (the library's own mechanism: the first neighbour that is not there yet ends the wait): the year
    is handed back and rerun by the launch-per-phase path to the same bits, nothing is booked for the one-launch year, and a
    launch-per-phase year afterwards gives the bits it gave"""
    ref = _shape(125)
    eng = ref["eng"]
    try:
        _on(eng)
        got, _, took, shallow = _year(ref)
        assert took == (1, 1, 1) and shallow == 1 and np.array_equal(got, ref["lpp"])
        others, fb = [eng.counter(k) for k in OTHERS], eng.frozen_fallbacks()
        eng.set_option("barrier_timeout_ms", 0.0)
        got, st, took, shallow = _year(ref)
        eng.set_option("barrier_timeout_ms", 2000.0)
        assert np.array_equal(got, ref["lpp"])
        assert took == (0, 0, 0) and shallow == 0 and [eng.counter(k) for k in OTHERS] == others
        assert st["nbarrier_timeouts"] >= 1 and eng.frozen_fallbacks() == fb + 1
        for key in ("nsteps", "nnewton"):                            # nothing booked twice
            assert st[key] == ref["st_lpp"][key], key
        eng.set_option("frozen_persistent", 0)
        got, _, took, shallow = _year(ref)
        assert took == (0, 0, 0) and shallow == 0 and np.array_equal(got, ref["lpp"])
        got, _, _, _ = _year(ref, "x")
        assert np.array_equal(got, ref["want"])
        eng.set_option("frozen_persistent", 1)
        got, _, took, shallow = _year(ref)                           # and the one-launch year is still there
        assert took == (1, 1, 1) and shallow == 1 and np.array_equal(got, ref["lpp"])
    finally:
        _reset(eng)


# ---- 9. other modules
ALL_COUNTERS = COUNTERS + (SHALLOW, "frozen_two_waves_years", "frozen_forced_years", "frozen_team_years")


@pytest.mark.parametrize("kind", ["iage", "forced_thres"])
def test_other_modules_are_unaffected(kind):
    """an iage engine and a thresholded forced engine (ny = 6, nz = 61): with the option at 1 the years and counters of the option at 0"""
    from nk_ooc_amd.engine import ModuleEngine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz = 61
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
        eng.set_option("frozen_phosphorus", 1)
        if kind == "forced_thres":
            eng.set_option("frozen_forced", 2)
        xp0 = x0 + 1.0e-4 * np.abs(x0) * np.random.default_rng(5).standard_normal(x0.shape)
        x, xp = eng.upload(x0), eng.upload(xp0)
        _, _, sched = eng.comp_fcn(x, record=True)
        outs = []
        for value in (0, 1):
            eng.set_option("frozen_phosphorus_shallow", value)
            before = [eng.counter(k) for k in ALL_COUNTERS]
            fx, st = eng.comp_fcn_frozen(xp, sched)
            outs.append((eng.download(fx), [st[k] for k in STATS], [eng.counter(k) - b for k, b in zip(ALL_COUNTERS, before)],
                         eng.counter("frozen_cache_bytes"), eng.counter("frozen_lds_bits")))
        assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1:] == outs[0][1:]
        assert outs[0][2][0] == 1 and outs[0][2][2] == 0 and outs[0][2][3] == 0      # (they take the one-launch year, and book no phosphorus year)
    finally:
        eng.close()


# ---- 10. bad values
def test_values_other_than_0_and_1_are_refused():
    from nk_ooc_amd.engine import Nk2dError

    ref = _shape(61)
    eng = ref["eng"]
    for bad in (2, -1, 0.5):
        with pytest.raises(Nk2dError, match="frozen_phosphorus_shallow"):
            eng.set_option("frozen_phosphorus_shallow", bad)
    eng.set_option("frozen_phosphorus", 1)                           # (where the option at 1 would take the one-launch year)
    eng.set_option("frozen_cache_lean", 1)
    try:
        got, _, took, shallow = _year(ref)                           # the option is still 0
        assert took == (0, 0, 0) and shallow == 0 and np.array_equal(got, ref["lpp"])
    finally:
        _reset(eng)


# ---- 11. tie to the reference's own numbers
@pytest.mark.parametrize("tag", ["22x9", "70x12"])
def test_the_reference_year_as_one_launch(golden_dir, tag):
    """y0 of the goldens over the full year (one and two levels per lane): the year frozen on its own recorded schedule, run as one
    launch, is the recorded year bit for bit, and the recorded year meets the reference's at test_phosphorus_comp_fcn's tolerance.
    phosphorus_70x12.npz holds the state (`y`) but no year: the reference's year of that very state is phosphorus_fcn_70x12.npz
    (tests/golden/gen_phosphorus_fcn.py, the generator of phosphorus_22x9.npz's `fcn` with the fixture's own seed)"""
    g = np.load(f"{golden_dir}/phosphorus_{tag}.npz")
    nz, ny = int(g["nz"]), int(g["ny"])
    if "fcn" in g.files:
        y0, fcn = g["y0"], g["fcn"]
    else:
        year = np.load(f"{golden_dir}/phosphorus_fcn_{tag}.npz")
        assert np.array_equal(year["y0"], g["y"])
        y0, fcn = year["y0"], year["fcn"]
    eng = _engine(nz, ny=ny, time_range=None, err_check=None)
    try:
        x = eng.upload(y0)
        fx, _, sched = eng.comp_fcn(x, record=True)
        want = eng.download(fx)
        assert np.allclose(want.reshape(-1), fcn, rtol=1.0e-3, atol=1.0e-6)
        _on(eng)
        names = COUNTERS + (SHALLOW,) + OTHERS
        before = [eng.counter(k) for k in names]
        fx1, _ = eng.comp_fcn_frozen(x, sched)
        assert [eng.counter(k) - b for k, b in zip(names, before)] == [1, 1, 1, 1, 0, 0, 0]
        assert np.array_equal(eng.download(fx1), want)
    finally:
        eng.close()
