"""The one-launch frozen year with the cross-lane moves of its Newton phase in the VALU (option "frozen_xlane", DESIGN.md
section 3.6): on top of the stage-value exchange, the vertical stencil of the tendencies, the parallel cyclic reduction of the
two tridiagonal solves and the sum of the norm partial move values between lanes with DPP and v_permlane swaps instead of
ds_bpermute.  Every lane receives the 64 bits __shfl_up / __shfl_down gave it -- its own value where it has no partner, which
the reduction multiplies by a zero --, so the perturbed frozen year is the same bits with the option 0 and 1, crossed with
"frozen_stage_exchange" 0 and 1 and "frozen_early" 0 and 1, and on the launch-per-phase path; so is every norm the year's check
reads (counter "frozen_step_sums_hash") and every sampled error estimate (`max_err`).  Counter "frozen_xlane_bits" is 1
exactly where the instantiation carries the body and "frozen_stage_exchange_bits" is 1.

Every engine runs with "frozen_err_check" 3 and "frozen_sums_poison" 1; behind the perturbed years the recorded state runs on
the same engine and must give the recorded year.

Shapes: the ones at which this code can go wrong.  ny = 6 with nz = 320, 384, 416 -- five to seven levels per lane; at 416 the
last lanes hold rows past nz, identity rows that go through every level of the reduction --; nz = 512, where the body is not
compiled in: the counter reports 0 and nothing changes; two ypos columns; two sweeps per solve (a phase with solves and no
stage part); the forced module with a decay source; a cache in pieces of seven rows (an instantiation of its own: with the
body at five levels per lane, without at six and seven); and the own state switched off with the option on (the body from
before)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
# ("frozen_xlane", "frozen_stage_exchange", "frozen_early")
ARMS = tuple((xl, xc, ea) for xl in (0, 1) for xc in (0, 1) for ea in (0, 1))


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
                     ("frozen_stage_exchange", 1), ("frozen_xlane", 1), ("frozen_persistent", 1)):
        eng.set_option(key, val)


def _all_ways(ref, own_state=True, min_err=2, lds_bits=63, exchange=None, body=None):
    """the perturbed year with the option, the exchange and "frozen_early" off and on: the launch-per-phase year's bits, the same
    counters and norms; then the recorded state with everything on: the recorded year"""
    eng = ref["eng"]
    exchange = own_state if exchange is None else exchange      # (the instantiation has the body for the exchange)
    body = exchange if body is None else body                   # (... and the one with the VALU moves)
    first = None
    for arm in ARMS:
        xlane, xchg, early = arm
        eng.set_option("frozen_xlane", xlane)
        eng.set_option("frozen_stage_exchange", xchg)
        eng.set_option("frozen_early", early)
        years = eng.counter("frozen_persistent_years")
        fx, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        got = eng.download(fx)
        print(f"frozen_xlane {xlane} (in effect {eng.counter('frozen_xlane_bits')}), "
              f"frozen_stage_exchange {xchg} (in effect {eng.counter('frozen_stage_exchange_bits')}), frozen_early {early} "
              f"(in effect {eng.counter('frozen_early_bits')}), lds bits {eng.counter('frozen_lds_bits')}: "
              f"step sums hash {eng.counter('frozen_step_sums_hash'):#x} (launch path {ref['sums_lpp']:#x}), "
              f"nnewton {st['nnewton']}, nsweeps {st['nsweeps']}, nerr_checked {st['nerr_checked']}, max_err {st['max_err']!r}, "
              f"differing values {int(np.count_nonzero(got != ref['lpp']))}")
        assert eng.counter("frozen_persistent_years") == years + 1, arm        # (no year is handed back)
        assert eng.counter("frozen_lds_bits") == lds_bits, arm
        assert eng.counter("frozen_stage_exchange_bits") == (xchg if exchange else 0), arm
        assert eng.counter("frozen_xlane_bits") == (xlane if body and exchange and xchg else 0), arm
        assert eng.counter("frozen_early_bits") == (early if own_state else 0), arm
        assert np.array_equal(got, ref["lpp"]), arm
        # the sums of the last two iterations of every step as this year's check read them: the launch path's, bit for bit
        assert eng.counter("frozen_step_sums_hash") == ref["sums_lpp"], arm
        for key in ("nsteps", "nnewton"):                        # (the launch path books its sweeps and estimates its own way)
            assert st[key] == ref["st_lpp"][key], (arm, key)
        first = st if first is None else first
        for key in STATS:                                        # (max_err: the largest sampled error estimate, bit for bit)
            assert st[key] == first[key], (arm, key)
        assert st["nerr_checked"] >= min_err, arm                # rows with an estimate: their phases ran between the others
    # the recorded state itself on the same engine, a second year behind the first
    eng.set_option("frozen_xlane", 1)
    eng.set_option("frozen_stage_exchange", 1)
    eng.set_option("frozen_early", 1)
    years = eng.counter("frozen_persistent_years")
    fx, _ = eng.comp_fcn_frozen(ref["x"], ref["sched"])
    assert eng.counter("frozen_persistent_years") == years + 1
    assert eng.counter("frozen_stage_exchange_bits") == (1 if exchange else 0)
    assert eng.counter("frozen_xlane_bits") == (1 if body and exchange else 0)
    assert np.array_equal(eng.download(fx), ref["want"])


IAGE = [(320, 5), (384, 6), (416, 7), (512, 8)]


@pytest.mark.parametrize("nz,E", IAGE, ids=[f"nz{nz}" for nz, _ in IAGE])
def test_levels_per_lane(nz, E):
    """five to seven levels per lane carry the body; at eight it is not compiled in: the counter is 0, the bits the same"""
    ref = _shape("iage", nz, 6)
    try:
        _all_ways(ref, own_state=E != 8, lds_bits=15 if E == 8 else 63)
    finally:
        _reset(ref["eng"])


def test_two_columns():
    """edge columns only: each column has one neighbour"""
    ref = _shape("iage", 416, 2)
    try:
        _all_ways(ref)
    finally:
        _reset(ref["eng"])


def test_two_sweep_iterations():
    """a phase with the two solves and no stage part behind every phase with one: a year whose every iteration takes two
    sweeps"""
    ref = _shape("iage_two_sweeps", 416, 6)
    eng = ref["eng"]
    try:
        _all_ways(ref, min_err=0)           # (a year of two-sweep solves samples no estimate in the kernel)
        eng.set_option("frozen_stage_exchange", 1)
        eng.set_option("frozen_xlane", 1)
        _, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_xlane_bits") == 1
        assert st["nsweeps"] > st["nnewton"]
    finally:
        _reset(eng)


def test_forced_decay():
    ref = _shape("forced_decay", 416, 4)
    try:
        _all_ways(ref)
    finally:
        _reset(ref["eng"])


@pytest.mark.parametrize("nz,exchange", [(320, True), (384, True), (416, False)], ids=["nz320", "nz384", "nz416"])
def test_cache_in_pieces(nz, exchange):
    """the piece flavour of the kernel is an instantiation of its own: a cache in pieces of seven rows.  At seven levels per lane
    that flavour has neither the exchange nor this body: both counters report 0 whatever the options say, the year is the same;
    at six it has the exchange and not this body (with it the compiler reports a spilled register): this counter reports 0, the
    other follows its option; at five it takes both"""
    ref = _shape("iage", nz, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_piece_rows", 7)
        _all_ways(ref, exchange=exchange, body=nz == 320)
        assert eng.counter("frozen_cache_pieces") > 0
    finally:
        _reset(eng)


def test_own_state_off():
    """without the own state (the lower four bits of "frozen_coef_lds" alone) the body is the one from before: the counter
    reports 0 whatever the option says, the year is the same"""
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_coef_lds", 15)
        _all_ways(ref, own_state=False, lds_bits=15)
    finally:
        _reset(eng)
