"""The one-launch frozen year in the kernel that carries the default year's body alone (option "frozen_dedicated", DESIGN.md
section 3.6; csrc/nk2d_frozen_d.hip): k_frozen_persistent_d compiles the text of k_frozen_persistent with the one Newton body a
year with every option at its default runs (CL 959) and with what the host guarantees for that body as constants; with value
2 its hand-over polls the neighbours' flags and the abort flag with one load.  The device functions are the same, so the year is
the same bits with the option 0, 1 and 2 and on the launch-per-phase path: the result, every norm the year's check reads
(counter "frozen_step_sums_hash" under "frozen_sums_poison") and every sampled error estimate (`max_err`, `nerr_checked`).

Every case asserts from the counters that arm 0 ran no dedicated year ("frozen_dedicated_years", "frozen_dedicated_bits") and that
arms 1 and 2 ran every year dedicated: a case that routes elsewhere fails.  Every engine runs with "frozen_err_check" 3, so that
rows with an estimate -- whose phases clear the wave's own state -- lie between the others.  Per arm the perturbed state runs
first and the recorded state behind it on the same engine: a second year behind a first.

Shapes, the smallest at which this body can go wrong: nz = 320, 384, 416 -- five, six and seven levels per lane, at 416 with
identity rows past nz in the last lanes --; one ypos column (no neighbour: nothing to wait for), two (edge columns only) and five;
iage (two tracers: two waves to a workgroup, the step block shared through LDS) and the forced module with a linear source (one
wave) -- a decay source (module kind 0) and the file-driven module without a sink threshold (kind 2, option "frozen_forced" 1:
instantiations of their own) --; the slab and a cache in pieces of seven rows (instantiations of their own; for kind 0 at five
levels per lane only: its piece flavours of six and seven are not in the set and would route to k_frozen_persistent)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("nsteps", "nnewton", "nfev", "njev", "nlu", "nsolve", "nsweeps", "nrejected", "nresumed", "nerr_checked", "max_err")
ARMS = (0, 1, 2)


def _grid(nz, ny):
    from nk_ooc_amd.grid import Grid2d

    if ny > 1:
        return Grid2d.default(nz, ny)
    # one ypos column: the stream function of the default grid vanishes on both of its edges, and its normalisation is 0 / 0.
    # A column at rest: no flow, vertical mixing only
    with np.errstate(invalid="ignore", divide="ignore"):
        grid = Grid2d.default(nz, 1)
    for field in (grid.stream, grid.vvel, grid.wvel):
        field[...] = 0.0
    assert grid.hmix_coeff.shape == (nz, 0)
    return grid


def _engine(kind, nz, ny):
    from nk_ooc_amd.engine import forced_engine, iage_engine

    grid = _grid(nz, ny)
    rng = np.random.default_rng(29)
    if kind == "iage":
        eng = iage_engine(grid)
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (nz, ny))] * 2) + 0.01 * rng.standard_normal((2, nz, ny))
    elif kind == "forced":             # one tracer with a decay source, linear in the tracer (module kind 0)
        eng = forced_engine(grid, {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"})
        eng.set_option("frozen_forced", 1)
        x0 = 1.0 + 0.2 * rng.standard_normal((1, nz, ny))
    else:                              # "forced_file": restoring targets and a source from records, no sink threshold (module kind 2), 40 days
        from nk_ooc_amd.engine import ModuleEngine

        day = 86400.0
        rec_times = np.array([-10.0, 40.0, 95.0, 200.0, 300.0]) * day
        restore = 1.0 + 0.2 * rng.standard_normal((5, ny))
        sms = 3.0e-8 * rng.standard_normal((5, nz, ny))
        eng = ModuleEngine(grid, tc=1, surf_rate=(24.0 / day,), module_kind=2, restore_series=(rec_times, restore),
                           sms_series=(rec_times, sms), sink_thres=None, time_range=(0.0, 40.0 * day))
        eng.set_option("frozen_forced", 1)
        x0 = 0.6 + 0.2 * rng.standard_normal((1, nz, ny))
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    eng.set_option("frozen_err_check", 3)
    eng.set_option("frozen_sums_poison", 1)
    v = np.random.default_rng(11).standard_normal(x0.shape)
    return eng, x0, x0 + 1.0e-4 * np.abs(x0) * v


_SHAPES = {}


def _shape(kind, nz, ny):
    """one engine per shape for the whole file: its recorded schedule and the launch-per-phase frozen year of the perturbed and of
    the recorded state -- computed once, left unchanged"""
    key = (kind, nz, ny)
    if key in _SHAPES:
        return _SHAPES[key]
    eng, x0, xp0 = _engine(kind, nz, ny)
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    ref = dict(eng=eng, sched=sched, states={"perturbed": xp, "recorded": x}, lpp={}, sums_lpp={}, st_lpp={})
    eng.set_option("frozen_persistent", 0)
    years = eng.counter("frozen_persistent_years")
    for name, state in ref["states"].items():
        fx_l, ref["st_lpp"][name] = eng.comp_fcn_frozen(state, sched)
        ref["lpp"][name] = eng.download(fx_l)
        ref["sums_lpp"][name] = eng.counter("frozen_step_sums_hash")
    assert eng.counter("frozen_persistent_years") == years
    # (the frozen year of the recorded state is the recorded year)
    assert np.array_equal(ref["lpp"]["recorded"], eng.download(fx))
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
    for key, val in (("frozen_cache_pieces", 0), ("frozen_cache_piece_rows", 0), ("frozen_dedicated", 0)):
        eng.set_option(key, val)


def _three_arms(ref):
    eng = ref["eng"]
    first = {}
    for arm in ARMS:
        eng.set_option("frozen_dedicated", arm)
        for name, state in ref["states"].items():       # the perturbed state, and the recorded one behind it
            years, dedicated = eng.counter("frozen_persistent_years"), eng.counter("frozen_dedicated_years")
            fx, st = eng.comp_fcn_frozen(state, ref["sched"])
            got = eng.download(fx)
            print(f"frozen_dedicated {arm} (in effect {eng.counter('frozen_dedicated_bits')}), {name} state: lds bits {eng.counter('frozen_lds_bits')}, "
                  f"early {eng.counter('frozen_early_bits')}, stage exchange {eng.counter('frozen_stage_exchange_bits')}, "
                  f"xlane {eng.counter('frozen_xlane_bits')}; one-launch years +{eng.counter('frozen_persistent_years') - years}, dedicated "
                  f"+{eng.counter('frozen_dedicated_years') - dedicated}; step sums hash {eng.counter('frozen_step_sums_hash'):#x} (launch path "
                  f"{ref['sums_lpp'][name]:#x}), nnewton {st['nnewton']}, nerr_checked {st['nerr_checked']}, max_err {st['max_err']!r}, "
                  f"differing values {int(np.count_nonzero(got != ref['lpp'][name]))}")
            assert eng.counter("frozen_persistent_years") == years + 1, (arm, name)        # (no year is handed back)
            assert eng.counter("frozen_dedicated_bits") == arm, (arm, name)
            assert eng.counter("frozen_dedicated_years") == dedicated + (1 if arm else 0), (arm, name)
            assert np.array_equal(got, ref["lpp"][name]), (arm, name)
            # the sums of the last two iterations of every step as this year's check read them: the launch path's, bit for bit
            assert eng.counter("frozen_step_sums_hash") == ref["sums_lpp"][name], (arm, name)
            for key in ("nsteps", "nnewton"):                        # (the launch path books its sweeps and estimates its own way)
                assert st[key] == ref["st_lpp"][name][key], (arm, name, key)
            first.setdefault(name, st)
            for key in STATS:                                        # (max_err: the largest sampled error estimate, bit for bit)
                assert st[key] == first[name][key], (arm, name, key)
            assert st["nerr_checked"] >= 1, (arm, name)              # rows with an estimate: their phases ran between the others


# (kind, nz, ny)
SLAB = [("iage", 320, 5), ("iage", 384, 5), ("iage", 416, 5), ("iage", 416, 2), ("iage", 416, 1),
        ("forced", 416, 5), ("forced", 384, 2), ("forced", 320, 1), ("forced_file", 416, 5), ("forced_file", 320, 2)]
PIECES = [("iage", 320, 5), ("forced", 320, 1), ("forced_file", 416, 5), ("forced_file", 384, 2)]


def _ids(cases):
    return [f"{kind}-nz{nz}-ny{ny}" for kind, nz, ny in cases]


@pytest.mark.parametrize("kind,nz,ny", SLAB, ids=_ids(SLAB))
def test_slab(kind, nz, ny):
    ref = _shape(kind, nz, ny)
    try:
        _three_arms(ref)
    finally:
        _reset(ref["eng"])


@pytest.mark.parametrize("kind,nz,ny", PIECES, ids=_ids(PIECES))
def test_cache_in_pieces(kind, nz, ny):
    """the piece flavour of the kernel is an instantiation of its own: a cache in pieces of seven rows"""
    ref = _shape(kind, nz, ny)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_piece_rows", 7)
        _three_arms(ref)
        assert eng.counter("frozen_cache_pieces") > 0
    finally:
        _reset(eng)


def test_option_values():
    """any value other than 0, 1 or 2 is an error, and leaves the option what it was"""
    ref = _shape("iage", 320, 5)
    eng = ref["eng"]
    try:
        eng.set_option("frozen_dedicated", 2)
        for bad in (3, -1, 0.5):
            with pytest.raises(Exception):
                eng.set_option("frozen_dedicated", bad)
        eng.comp_fcn_frozen(ref["states"]["perturbed"], ref["sched"])
        assert eng.counter("frozen_dedicated_bits") == 2
    finally:
        _reset(eng)
