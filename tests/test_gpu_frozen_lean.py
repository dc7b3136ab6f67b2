"""The one-launch frozen year on a LEAN schedule cache (option "frozen_cache_lean"): the cache holds the
mixing and Jacobian planes only, and the first phase of every row of k_frozen_persistent<..., LEAN = 1> is the factorising
instantiation of its body (what the launch-per-phase path runs at every "LU" event), on one row's worth of factor tables.
The same device functions, so the same bits -- as the recorded year, as the launch-per-phase year and as the full-cache
one-launch year of a perturbed state -- in every flavour of the kernel (four-wave team, adjacent columns, by column; slab
and pieces; whatever lives in LDS), with a cache of the planes' size.

Shapes: ny = 6 (a column with both neighbours, both edges, an even/odd split) and nz = 64 E - 3 for E = 1 ... 8 levels per lane
(a ragged last lane at every levels-per-lane count); an error estimate on every 8th step, so that several rows carry the
in-kernel estimate on in-kernel tables.

The file-driven forced module (KIND 2) has no one-launch year above four levels per lane, lean or not ("the same modules
take it as today"): at seven levels per lane that is what is checked for it, and the one-tracer linear module that does
have one there (forced with a decay source, KIND 0) carries the lean checks."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY = 6
STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")


def _engine(kind, E):
    from nk_ooc_amd.engine import ModuleEngine, forced_engine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    nz = 64 * E - 3
    grid = Grid2d.default(nz, NY)
    rng = np.random.default_rng(11)
    if kind == "iage":
        eng = iage_engine(grid)
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (nz, NY))] * 2) + 0.01 * rng.standard_normal((2, nz, NY))
    elif kind == "forced_files":       # KIND 2, linear sources (no sink threshold)
        times = np.array([-10.0, 40.0, 95.0, 200.0, 300.0]) * 86400.0
        eng = ModuleEngine(grid, tc=1, surf_rate=(24.0 / 86400.0,), module_kind=2,
                           restore_series=(times, 1.0 + 0.2 * rng.standard_normal((5, NY))),
                           sms_series=(times, 3.0e-8 * rng.standard_normal((5, nz, NY))), time_range=(0.0, 40.0 * 86400.0))
        x0 = 0.6 + 0.2 * rng.standard_normal((1, nz, NY))
    else:                              # "forced_decay": one tracer, KIND 0
        eng = forced_engine(grid, {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"})
        x0 = 1.0 + 0.2 * rng.standard_normal((1, nz, NY))
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    eng.set_option("frozen_err_check", 8)
    v = np.random.default_rng(5).standard_normal(x0.shape)
    return eng, x0, x0 + 1.0e-4 * np.abs(x0) * v


def _sizes(eng, E):
    """bytes of a full and of a lean cache row of this engine (CachePtrs: 8 (3 kv_len + 5 np + 3 nv + 3 ntab) / 8 (3 kv_len + 5 np))"""
    tc = eng.shape[0]
    nzp = 64 * E
    plane, nv, ntab = NY * nzp, tc * NY * nzp, tc * NY * 14 * 64
    kv_len = 2 * plane + NY if eng.module_kind == 2 else plane
    return 8 * (3 * kv_len + 5 * plane + 3 * nv + 3 * ntab), 8 * (3 * kv_len + 5 * plane)


_SHAPES = {}


def _shape(kind, E):
    """one engine per (module, levels per lane) for the whole file: its recorded year and, for the perturbed state, the
    launch-per-phase year and the full-cache one-launch year with the full cache's size -- computed once, left unchanged"""
    if (kind, E) in _SHAPES:
        return _SHAPES[(kind, E)]
    eng, x0, xp0 = _engine(kind, E)
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    ref = dict(eng=eng, x=x, xp=xp, sched=sched, n=len(sched), want=eng.download(fx))
    eng.set_option("frozen_persistent", 0)
    fx_l, ref["st_lpp"] = eng.comp_fcn_frozen(xp, sched)
    ref["lpp"] = eng.download(fx_l)
    eng.set_option("frozen_persistent", 1)
    years = eng.counter("frozen_persistent_years")
    fx_f, _ = eng.comp_fcn_frozen(xp, sched)
    ref["full_took"] = eng.counter("frozen_persistent_years") - years
    fx_f, ref["st_full"] = eng.comp_fcn_frozen(xp, sched)         # (a year on the built cache: its launch count is the year's)
    ref["full"] = eng.download(fx_f)
    ref["full_bytes"] = eng.counter("frozen_cache_bytes")
    assert eng.counter("frozen_cache_lean") == 0 and eng.counter("frozen_lean_years") == 0
    _SHAPES[(kind, E)] = ref
    return ref


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ref in _SHAPES.values():
        ref["eng"].close()
    _SHAPES.clear()


def _lean_year(ref, state="xp"):
    """one frozen year with whatever options are set: (result, stats, one-launch years it added, lean years it added)"""
    eng = ref["eng"]
    years, lean = eng.counter("frozen_persistent_years"), eng.counter("frozen_lean_years")
    fx, st = eng.comp_fcn_frozen(ref[state], ref["sched"])
    return eng.download(fx), st, eng.counter("frozen_persistent_years") - years, eng.counter("frozen_lean_years") - lean


def _reset(eng):
    for key, val in (("frozen_cache_lean", 0), ("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0), ("frozen_coef_lds", 15),
                     ("frozen_by_column", 1), ("frozen_persistent", 1), ("frozen_cache_gb", 128.0)):
        eng.set_option(key, val)


def _check_against_references(ref, got, st):
    assert np.array_equal(got, ref["lpp"])                           # (a) the launch-per-phase year
    assert np.array_equal(got, ref["full"])                          # (b) the full-cache one-launch year
    for key in STATS:
        assert st[key] == ref["st_full"][key], key
    for key in ("nsteps", "nnewton"):
        assert st[key] == ref["st_lpp"][key], key
    assert st["nerr_checked"] >= 2                                   # several rows carried the in-kernel estimate


CASES = [("iage", E) for E in range(1, 9)] + [("forced_files", 1), ("forced_files", 4), ("forced_decay", 7)]


@pytest.mark.parametrize("kind,E", CASES, ids=[f"{k}-E{e}" for k, e in CASES])
def test_lean_year_is_the_full_cache_year_and_the_launch_per_phase_year(kind, E):
    ref = _shape(kind, E)
    eng, n = ref["eng"], ref["n"]
    assert ref["full_took"] == 1
    eng.set_option("frozen_cache_lean", 1)
    try:
        builds = eng.counter("frozen_cache_builds") + (0 if eng.counter("frozen_cache_lean") else 1)
        got, _, took, lean = _lean_year(ref, "x")
        assert (took, lean) == (1, 1)
        assert np.array_equal(got, ref["want"])                      # 1. the recorded year, bit for bit
        assert eng.counter("frozen_cache_builds") == builds          # (the full cache went, the lean one was built)
        got, st, took, lean = _lean_year(ref)                        # 2. a perturbed state
        assert (took, lean) == (1, 1)                                # 3. booked once, as a one-launch year and as a lean one
        assert eng.counter("frozen_cache_builds") == builds          #    (one cache per schedule)
        _check_against_references(ref, got, st)
        assert st["nlaunch"] == ref["st_full"]["nlaunch"]
        assert eng.counter("frozen_cache_lean") == 1                 # 4.
        full_row, lean_row = _sizes(eng, E)                          # 5. the planes' size, with the slab's headroom rows
        cap = n + n // 6 + 16
        assert ref["full_bytes"] == cap * full_row
        assert eng.counter("frozen_cache_bytes") == cap * lean_row < ref["full_bytes"]
    finally:
        _reset(eng)


def test_file_driven_forced_module_at_seven_levels_per_lane_routes_as_today():
    """no one-launch year for KIND 2 above four levels per lane, on either cache: the lean option leaves the year on the
    launch-per-phase path with its bits"""
    ref = _shape("forced_files", 7)
    eng = ref["eng"]
    assert ref["full_took"] == 0 and ref["full_bytes"] == 0 and np.array_equal(ref["full"], ref["lpp"])
    eng.set_option("frozen_cache_lean", 1)
    try:
        got, _, took, lean = _lean_year(ref)
        assert (took, lean) == (0, 0) and eng.counter("frozen_cache_lean") == 0 and eng.counter("frozen_cache_bytes") == 0
        assert np.array_equal(got, ref["lpp"])
    finally:
        _reset(eng)


@pytest.mark.parametrize("E,bits", [(E, b) for E in (5, 7) for b in (0, 3, 7, 15)])
def test_whatever_lives_in_lds(E, bits):
    """by column: nothing, coefficients + W, + the step block, + the pivots of the real system (bit 8: filled behind the
    factorising phase from what it wrote)"""
    ref = _shape("iage", E)
    eng = ref["eng"]
    eng.set_option("frozen_cache_lean", 1)
    eng.set_option("frozen_coef_lds", bits)
    try:
        got, _, took, lean = _lean_year(ref, "x")
        assert (took, lean) == (1, 1) and np.array_equal(got, ref["want"])
        got, st, took, lean = _lean_year(ref)
        assert (took, lean) == (1, 1)
        _check_against_references(ref, got, st)
    finally:
        _reset(eng)


def test_by_column_forced_at_three_levels_per_lane():
    ref = _shape("iage", 3)
    eng = ref["eng"]
    eng.set_option("frozen_cache_lean", 1)
    eng.set_option("frozen_by_column", 2)
    try:
        got, _, took, lean = _lean_year(ref, "x")
        assert (took, lean) == (1, 1) and np.array_equal(got, ref["want"])
        got, st, took, lean = _lean_year(ref)
        assert (took, lean) == (1, 1)
        _check_against_references(ref, got, st)
    finally:
        _reset(eng)


@pytest.mark.parametrize("E,B", [(1, 1), (1, 7), (7, 1), (7, 7)])
def test_pieces_of_a_lean_cache(E, B):
    """piece boundaries before, on and behind rows with an error estimate (every 8th row; pieces of 1 and of 7 rows): the
    slab-lean results, in pieces of B lean rows"""
    ref = _shape("iage", E)
    eng, n = ref["eng"], ref["n"]
    eng.set_option("frozen_cache_lean", 1)
    try:
        slab, st_slab, _, _ = _lean_year(ref)
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_piece_rows", B)
        got, _, took, lean = _lean_year(ref, "x")
        assert (took, lean) == (1, 1) and np.array_equal(got, ref["want"])
        got, st, took, lean = _lean_year(ref)
        assert (took, lean) == (1, 1)
        assert np.array_equal(got, slab)
        for key in STATS:
            assert st[key] == st_slab[key], key
        _check_against_references(ref, got, st)
        assert eng.counter("frozen_cache_lean") == 1 and eng.counter("frozen_cache_pieces") == math.ceil(n / B)
        assert eng.counter("frozen_cache_bytes") == math.ceil(n / B) * B * _sizes(eng, E)[1]
    finally:
        _reset(eng)


def test_mode_2_is_lean_only_where_the_full_cache_is_refused():
    ref = _shape("iage", 2)
    eng, n = ref["eng"], ref["n"]
    full_row, lean_row = _sizes(eng, 2)
    full_b, lean_b = n * full_row, n * lean_row          # (what "frozen_cache_gb" is compared with: the rows of the schedule)
    assert lean_b < full_b == ref["full_bytes"] // (n + n // 6 + 16) * n
    eng.set_option("frozen_cache_lean", 2)
    try:
        eng.set_option("frozen_cache_gb", 0.5 * (full_b + lean_b) / 1.0e9)
        got, st, took, lean = _lean_year(ref)
        assert (took, lean) == (1, 1) and eng.counter("frozen_cache_lean") == 1
        _check_against_references(ref, got, st)
        got, _, took, lean = _lean_year(ref)             # (and stays: the same cache, no build)
        assert (took, lean) == (1, 1) and np.array_equal(got, ref["lpp"])
        eng.set_option("frozen_cache_gb", 2.0 * full_b / 1.0e9)
        builds = eng.counter("frozen_cache_builds")
        got, st, took, lean = _lean_year(ref)
        assert (took, lean) == (1, 0) and eng.counter("frozen_cache_lean") == 0
        assert eng.counter("frozen_cache_builds") == builds + 1 and eng.counter("frozen_cache_bytes") == ref["full_bytes"]
        assert np.array_equal(got, ref["lpp"])
        eng.set_option("frozen_cache_gb", 0.5 * lean_b / 1.0e9)      # below both: no one-launch year
        got, _, took, lean = _lean_year(ref)
        assert (took, lean) == (0, 0) and np.array_equal(got, ref["lpp"])
    finally:
        _reset(eng)


def test_switching_lean_full_lean():
    ref = _shape("iage", 4)
    eng = ref["eng"]
    full_row, lean_row = _sizes(eng, 4)
    try:
        _lean_year(ref)                                              # (whatever was held before: the full cache now)
        assert eng.counter("frozen_cache_lean") == 0 and eng.counter("frozen_cache_bytes") == ref["full_bytes"]
        for flag in (1, 0, 1):
            eng.set_option("frozen_cache_lean", flag)
            builds = eng.counter("frozen_cache_builds")
            got, st, took, lean = _lean_year(ref)
            assert (took, lean) == (1, flag)                         # no year booked twice
            assert eng.counter("frozen_cache_builds") == builds + 1  # the other form went, this one was built
            assert eng.counter("frozen_cache_lean") == flag
            assert eng.counter("frozen_cache_bytes") % (lean_row if flag else full_row) == 0
            assert (eng.counter("frozen_cache_bytes") == ref["full_bytes"]) == (flag == 0)
            _check_against_references(ref, got, st)
    finally:
        _reset(eng)


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


def test_safety_net_as_with_the_full_cache():
    """Newton iterations taken away at a step in the middle of the year (as the safety-net test of the one-launch year does):
    the lean year is handed back and resumed exactly as the full-cache year is; so is one whose hand-over times out; and the
    context is then what a fresh one is"""
    ref = _shape("iage", 1)
    sched = ref["sched"]
    bad = sched.copy()
    half = len(bad) // 2
    k = half + int(np.argmax(bad[half:, 3]))          # (the step with the most iterations keeps one)
    drop = int(bad[k, 3]) - 1
    assert drop >= 1
    bad[k, 3] -= drop
    outs = {}
    for flag in (0, 1):
        eng, x0, _ = _engine("iage", 1)
        eng.set_option("frozen_cache_lean", flag)
        x = eng.upload(x0)
        fx, _, sched_f = eng.comp_fcn(x, record=True)
        assert np.array_equal(sched_f, sched) and np.array_equal(eng.download(fx), ref["want"])
        outs[flag] = _safety_net(eng, x, sched, bad)
        assert eng.counter("frozen_cache_lean") == flag
        # a free-running year on the context gives the bits it gives on a fresh context
        fx2, _, sched2 = eng.comp_fcn(x, record=True)
        assert np.array_equal(eng.download(fx2), ref["want"]) and np.array_equal(sched2, sched)
        fx3, _ = eng.comp_fcn_frozen(x, sched)
        assert np.array_equal(eng.download(fx3), ref["want"])
        eng.close()
    full, lean = outs[0], outs[1]
    assert np.array_equal(lean[0], full[0]) and lean[1:4] == full[1:4]
    if drop >= 2:
        assert lean[1] >= 1 or lean[3] >= 1                          # (the net was needed)
    assert np.array_equal(lean[4], full[4]) and np.array_equal(lean[4], ref["want"]) and lean[5] >= 1 and full[5] >= 1


def test_refusals():
    from nk_ooc_amd.engine import Nk2dError

    ref = _shape("iage", 1)
    eng = ref["eng"]
    for bad in (3, -1):
        with pytest.raises(Nk2dError, match="frozen_cache_lean"):
            eng.set_option("frozen_cache_lean", bad)
    # the single precision factorisation: the lean year is not taken, the year is the launch path's
    eng2, x0, xp0 = _engine("iage", 1)
    eng2.set_option("factor_fp32", 1)
    eng2.set_option("frozen_cache_lean", 1)
    x, xp = eng2.upload(x0), eng2.upload(xp0)
    fx, _, sched = eng2.comp_fcn(x, record=True)
    fx_p, _ = eng2.comp_fcn_frozen(xp, sched)
    assert eng2.counter("frozen_persistent_years") == 0 and eng2.counter("frozen_lean_years") == 0
    assert eng2.counter("frozen_cache_lean") == 0 and eng2.counter("frozen_cache_bytes") == 0
    eng2.set_option("frozen_persistent", 0)
    fx_l, _ = eng2.comp_fcn_frozen(xp, sched)
    assert np.array_equal(eng2.download(fx_p), eng2.download(fx_l))
    fx_r, _ = eng2.comp_fcn_frozen(x, sched)
    assert np.array_equal(eng2.download(fx_r), eng2.download(fx))
    eng2.close()
