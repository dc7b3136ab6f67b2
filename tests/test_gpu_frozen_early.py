"""The one-launch frozen year with the norm partials out of the way of the hand-over (option "frozen_early", DESIGN.md section
3.6): a wave that carries its column's whole own state forms the norm partial of an update part behind that part's stores of Z
(or of y_new and the next Z) and stores it behind its hand-over flag, instead of both in front of the stores its neighbours
wait for.  No operation changes: the perturbed frozen year is the same bits with 0 and 1 and on the launch-per-phase path, and
so is every norm the year's check reads -- the sums of the last two Newton iterations of every step, which decide whether the
year is accepted at all, and the sampled error estimates (`max_err`).

The state does not depend on the partials, and their rows outlive a year.  So every engine here runs with option
"frozen_sums_poison": the rows are NaN before each year, and a partial that is not stored, or stored to another place, fails
the year's check (the year is handed back: "frozen_persistent_years" does not count it) instead of passing on the sums of
the year before.  And counter "frozen_step_sums_hash" -- a hash of the bits of every step sum the check read -- must be the
same with 0, with 1 and launch by launch.

Shapes: the ones at which this code can go wrong.  ny = 6 with nz = 320, 384, 416, 512 -- five to eight levels per lane, a
ragged last lane at 416; at 512 the own state is not compiled in, the counter reports 0 and nothing changes --; two ypos
columns (one neighbour each); an error estimate on every third step, so that the phases of another kind between two
hand-overs with a pending partial run many times in a year; two sweeps per solve (a phase without an update part between two
with one, Z written in place); the forced module with a decay source; a cache in pieces of seven rows; and the own state
switched off with the option on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
EARLY = (0, 1)


def _engine(kind, nz, ny):
    from nk_ooc_amd.engine import forced_engine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    grid = Grid2d.default(nz, ny)
    rng = np.random.default_rng(23)
    if kind in ("iage", "iage_two_sweeps"):
        eng = iage_engine(grid)
        if kind == "iage_two_sweeps":       # (a few ypos columns couple too weakly to ask for a second sweep by themselves)
            eng.set_option("min_sweeps", 2)
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (nz, ny))] * 2) + 0.01 * rng.standard_normal((2, nz, ny))
    else:                              # "forced_decay": one tracer with a decay source
        eng = forced_engine(grid, {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"})
        eng.set_option("frozen_forced", 1)
        x0 = 1.0 + 0.2 * rng.standard_normal((1, nz, ny))
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    eng.set_option("frozen_err_check", 3)
    eng.set_option("frozen_sums_poison", 1)
    v = np.random.default_rng(7).standard_normal(x0.shape)
    return eng, x0, x0 + 1.0e-4 * np.abs(x0) * v


_SHAPES = {}


def _shape(kind, nz, ny):
    """one engine per shape for the whole file: its recorded year and the launch-per-phase year of the perturbed state --
    computed once, left unchanged"""
    key = (kind, nz, ny)
    if key in _SHAPES:
        return _SHAPES[key]
    eng, x0, xp0 = _engine(kind, nz, ny)
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    ref = dict(eng=eng, x=x, xp=xp, sched=sched, want=eng.download(fx))
    eng.set_option("frozen_persistent", 0)
    years = eng.counter("frozen_persistent_years")
    fx_l, ref["st_lpp"] = eng.comp_fcn_frozen(xp, sched)
    assert eng.counter("frozen_persistent_years") == years
    ref["lpp"] = eng.download(fx_l)
    ref["sums_lpp"] = eng.counter("frozen_step_sums_hash")
    eng.set_option("frozen_persistent", 1)
    _SHAPES[key] = ref
    return ref


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ref in _SHAPES.values():
        ref["eng"].close()
    _SHAPES.clear()


def _reset(eng):
    for key, val in (("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0), ("frozen_coef_lds", 63), ("frozen_early", 1),
                     ("frozen_persistent", 1)):
        eng.set_option(key, val)


def _both_ways(ref, own_state=True, min_err=2, lds_bits=63):
    """the perturbed year with the option off and on: the launch-per-phase year's bits, the same counters and norms"""
    eng = ref["eng"]
    first = None
    for early in EARLY:
        eng.set_option("frozen_early", early)
        years = eng.counter("frozen_persistent_years")
        fx, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        got = eng.download(fx)
        print(f"frozen_early {early}: in effect {eng.counter('frozen_early_bits')} (lds bits {eng.counter('frozen_lds_bits')}), "
              f"step sums hash {eng.counter('frozen_step_sums_hash'):#x} (launch path {ref['sums_lpp']:#x}), "
              f"nnewton {st['nnewton']}, nsweeps {st['nsweeps']}, nerr_checked {st['nerr_checked']}, max_err {st['max_err']!r}")
        assert eng.counter("frozen_persistent_years") == years + 1, early
        assert eng.counter("frozen_lds_bits") == lds_bits, early
        assert eng.counter("frozen_early_bits") == (early if own_state else 0), early
        assert np.array_equal(got, ref["lpp"]), early
        # the sums of the last two iterations of every step as this year's check read them: the launch path's, bit for bit
        assert eng.counter("frozen_step_sums_hash") == ref["sums_lpp"], early
        for key in ("nsteps", "nnewton"):                        # (the launch path books its sweeps and estimates its own way)
            assert st[key] == ref["st_lpp"][key], (early, key)
        first = st if first is None else first
        for key in STATS:                                        # (max_err: the largest sampled error estimate, bit for bit)
            assert st[key] == first[key], (early, key)
        assert st["nerr_checked"] >= min_err, early              # rows with an estimate: their phases ran between the others
    # the recorded state itself, with everything on: the recorded year
    eng.set_option("frozen_early", 1)
    fx, _ = eng.comp_fcn_frozen(ref["x"], ref["sched"])
    assert np.array_equal(eng.download(fx), ref["want"])


IAGE = [(320, 5), (384, 6), (416, 7), (512, 8)]


@pytest.mark.parametrize("nz,E", IAGE, ids=[f"nz{nz}" for nz, _ in IAGE])
def test_levels_per_lane(nz, E):
    ref = _shape("iage", nz, 6)
    try:
        _both_ways(ref, own_state=E != 8, lds_bits=15 if E == 8 else 63)
    finally:
        _reset(ref["eng"])


def test_two_columns():
    """each column has one neighbour: both workgroups sit at an edge of the plane"""
    ref = _shape("iage", 416, 2)
    try:
        _both_ways(ref)
    finally:
        _reset(ref["eng"])


def test_two_sweep_iterations():
    """a phase without an update part between every two with one, and the update of a two-sweep iteration writes Z in place: a
    year whose every iteration takes two sweeps"""
    ref = _shape("iage_two_sweeps", 416, 6)
    eng = ref["eng"]
    try:
        _both_ways(ref, min_err=0)           # (a year of two-sweep solves samples no estimate in the kernel)
        _, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_early_bits") == 1
        assert st["nsweeps"] > st["nnewton"]
    finally:
        _reset(eng)


def test_forced_decay():
    ref = _shape("forced_decay", 416, 4)
    try:
        _both_ways(ref)
    finally:
        _reset(ref["eng"])


@pytest.mark.parametrize("pieces", [0, 1], ids=["slab", "pieces"])
def test_slab_and_pieces(pieces):
    """the piece flavour of the kernel is an instantiation of its own: a cache in pieces of seven rows"""
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_cache_pieces", pieces)
        if pieces:
            eng.set_option("frozen_cache_piece_rows", 7)
        _both_ways(ref)
        assert (eng.counter("frozen_cache_pieces") > 0) == bool(pieces)
    finally:
        _reset(eng)


def test_own_state_off():
    """without the own state (the lower four bits of "frozen_coef_lds" alone) the body is the one from before: the counter
    reports 0 whatever the option says, the year is the same"""
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_coef_lds", 15)
        _both_ways(ref, own_state=False, lds_bits=15)
    finally:
        _reset(eng)


def test_option_is_boolean():
    """any value but 0 switches it on: the counter reports 1"""
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_early", 7)
        years = eng.counter("frozen_persistent_years")
        eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_persistent_years") == years + 1
        assert eng.counter("frozen_early_bits") == 1
    finally:
        _reset(eng)


def test_sums_are_the_years_own():
    """the hash is of the sums of the year just run, not of a leftover: another state on the same steps gives another one, and
    the first state again the first one again"""
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.comp_fcn_frozen(ref["x"], ref["sched"])
        h_x = eng.counter("frozen_step_sums_hash")
        eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_step_sums_hash") == ref["sums_lpp"] != h_x
    finally:
        _reset(eng)
