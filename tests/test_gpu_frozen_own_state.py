"""The one-launch frozen year with a column's own state kept on its compute unit (option "frozen_coef_lds" bits 16 and 32,
DESIGN.md section 3.6): bit 16 keeps the wave's own state column Y in LDS, bit 32 hands the wave's own three stage values from
the update part of one Newton phase to the stage part of the next in registers.  Neither changes an operation: the perturbed
frozen year is the same bits with 15, 31, 47 and 63 and on the launch-per-phase path, and so is every norm the year's check
reads -- the sums of the last two Newton iterations of every step decide whether the year is accepted at all, the sampled
error estimates come back as `max_err`; the partials of earlier iterations, which nothing reads, are no longer formed.

Shapes: ny = 6 (both edge columns and interior ones) and nz = 320, 384, 416, 512, that is five to eight levels per lane with a
ragged last lane at 416; an error estimate on every third step, so that rows whose tail rewrites Y, Z and W by another path
(and the reload behind them) are exercised many times in a year.  Eight levels per lane stay what they were: a compute unit
that holds two workgroups has no room for Y there and the kernel no register room for the stage values, so both bits are
compiled out and the year runs with the lower four bits alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
BITS = (15, 31, 47, 63)


def _engine(kind, nz, ny):
    from nk_ooc_amd.engine import forced_engine, iage_engine
    from nk_ooc_amd.grid import Grid2d

    grid = Grid2d.default(nz, ny)
    rng = np.random.default_rng(23)
    if kind in ("iage", "iage_two_sweeps"):
        eng = iage_engine(grid)
        if kind == "iage_two_sweeps":       # (six ypos columns couple too weakly to ask for a second sweep by themselves)
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
    for key, val in (("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0), ("frozen_coef_lds", 63), ("frozen_persistent", 1)):
        eng.set_option(key, val)


def _in_effect(bits, E):
    """what the kernel takes of the bits asked for: everything where it fits (six workgroups: a compute unit each), at eight
    levels per lane the set from before these bits"""
    return bits & 15 if E == 8 else bits


def _five_ways(ref, E, min_err=2):
    eng = ref["eng"]
    first = None
    for bits in BITS:
        eng.set_option("frozen_coef_lds", bits)
        years = eng.counter("frozen_persistent_years")
        fx, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        got = eng.download(fx)
        print(f"frozen_coef_lds {bits}: in effect {eng.counter('frozen_lds_bits')}, nnewton {st['nnewton']}, nsweeps {st['nsweeps']}, "
              f"nerr_checked {st['nerr_checked']}, max_err {st['max_err']!r}")
        assert eng.counter("frozen_persistent_years") == years + 1, bits
        assert eng.counter("frozen_lds_bits") == _in_effect(bits, E), bits
        assert np.array_equal(got, ref["lpp"]), bits
        for key in ("nsteps", "nnewton"):                        # (the launch path books its sweeps and estimates its own way)
            assert st[key] == ref["st_lpp"][key], (bits, key)
        first = st if first is None else first
        for key in STATS:                                        # (max_err: the largest sampled error estimate, bit for bit)
            assert st[key] == first[key], (bits, key)
        assert st["nerr_checked"] >= min_err, bits               # rows with an estimate: the reload path ran
    # the recorded state itself, with everything on: the recorded year
    eng.set_option("frozen_coef_lds", 63)
    fx, _ = eng.comp_fcn_frozen(ref["x"], ref["sched"])
    assert np.array_equal(eng.download(fx), ref["want"])


IAGE = [(320, 5), (384, 6), (416, 7), (512, 8)]


@pytest.mark.parametrize("nz,E", IAGE, ids=[f"nz{nz}" for nz, _ in IAGE])
def test_iage_is_the_same_year_five_ways(nz, E):
    ref = _shape("iage", nz, 6)
    try:
        _five_ways(ref, E)
    finally:
        _reset(ref["eng"])


def test_two_sweep_iterations():
    """the update of a two-sweep iteration writes Z in place (the stage part of the same iteration has read it, the phase
    between them carries nothing): a year whose every iteration takes two sweeps, five ways"""
    ref = _shape("iage_two_sweeps", 416, 6)
    eng = ref["eng"]
    try:
        _five_ways(ref, 7, min_err=0)       # (a year of two-sweep solves samples no estimate in the kernel)
        _, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_lds_bits") == 63
        assert st["nsweeps"] > st["nnewton"]
    finally:
        _reset(eng)


def test_forced_decay_is_the_same_year_five_ways():
    ref = _shape("forced_decay", 416, 4)
    try:
        _five_ways(ref, 7)
    finally:
        _reset(ref["eng"])


@pytest.mark.parametrize("pieces", [0, 1], ids=["slab", "pieces"])
def test_slab_and_pieces(pieces):
    ref = _shape("iage", 416, 6)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_cache_pieces", pieces)
        if pieces:
            eng.set_option("frozen_cache_piece_rows", 7)
        years = eng.counter("frozen_persistent_years")
        fx, st = eng.comp_fcn_frozen(ref["xp"], ref["sched"])
        assert eng.counter("frozen_persistent_years") == years + 1
        assert eng.counter("frozen_lds_bits") == 63
        assert (eng.counter("frozen_cache_pieces") > 0) == bool(pieces)
        assert np.array_equal(eng.download(fx), ref["lpp"])
        for key in ("nsteps", "nnewton"):
            assert st[key] == ref["st_lpp"][key], key
        assert st["nerr_checked"] >= 2
    finally:
        _reset(eng)
