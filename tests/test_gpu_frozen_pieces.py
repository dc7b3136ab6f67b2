"""The schedule cache of the one-launch frozen year as a list of equally sized pieces (option "frozen_cache_pieces", DESIGN.md
section 3.6): the piece flavours of k_frozen_persistent, k_cache_planes and k_cache_factor find a row's tables in the piece
that holds the row and do everything else as the slab flavours do -- the same bits as the slab path and as the launch-per-phase
path, wherever the piece boundaries fall; pieces are kept and only added to; the early request has them there before the
first product."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _iage(n, ny=None):
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    eng = iage_engine(Grid2d.default(n, ny or n))
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    return eng


def _state(eng, seed=3):
    rng = np.random.default_rng(seed)
    tc, nz, ny = eng.shape
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    x0 = np.stack([np.broadcast_to(col[:, None], (nz, ny))] * tc) + 0.01 * rng.standard_normal(eng.shape)
    return x0, eng.upload(x0), eng.upload(x0 * (1.0 + 1.0e-4 * rng.standard_normal(x0.shape)))


def _three_way(eng, x, xp, sched, want, piece_rows):
    """the recorded and a perturbed state on the launch-per-phase path, the slab path and the piece path: (perturbed result,
    slab stats, piece stats); asserts the bit comparisons and that every slab / piece year was a one-launch year"""
    eng.set_option("frozen_persistent", 0)
    lpp = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("frozen_persistent", 1)
    eng.set_option("frozen_cache_pieces", 0)
    years = eng.counter("frozen_persistent_years")
    fx_s, st_s = eng.comp_fcn_frozen(xp, sched)
    slab = eng.download(fx_s)
    assert eng.counter("frozen_persistent_years") == years + 1 and eng.counter("frozen_cache_pieces") == 0
    eng.set_option("frozen_cache_pieces", 1)
    eng.set_option("frozen_cache_piece_rows", piece_rows)
    fx_r, _ = eng.comp_fcn_frozen(x, sched)
    assert eng.counter("frozen_persistent_years") == years + 2
    assert np.array_equal(eng.download(fx_r), want)                      # the recorded year, bit for bit
    fx_p, st_p = eng.comp_fcn_frozen(xp, sched)
    assert eng.counter("frozen_persistent_years") == years + 3
    got = eng.download(fx_p)
    assert np.array_equal(got, slab) and np.array_equal(got, lpp)
    assert eng.counter("frozen_cache_pieces") == math.ceil(len(sched) / piece_rows)
    return got, st_s, st_p


@pytest.fixture(scope="module")
def year26():
    """iage 26 x 26 with an error estimate on every 7th step: one engine, its recorded year and the references of the
    launch-per-phase and the slab path, shared by the boundary cases"""
    eng = _iage(26)
    eng.set_option("frozen_err_check", 7)
    _, x, xp = _state(eng)
    fx, _, sched = eng.comp_fcn(x, record=True)
    want = eng.download(fx)
    eng.set_option("frozen_persistent", 0)
    lpp = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("frozen_persistent", 1)
    fx_s, st_s = eng.comp_fcn_frozen(xp, sched)
    ref = dict(eng=eng, x=x, xp=xp, sched=sched, want=want, lpp=lpp, slab=eng.download(fx_s), st_slab=st_s)
    yield ref
    eng.close()


@pytest.mark.parametrize("where", ["1", "7", "n-1", "n", "n+5"])
def test_piece_boundaries_team_flavour(year26, where):
    """every row its own piece; checked rows on the first row of a piece (row i - 1 in the piece before); a last piece of one
    row; exactly one full piece; one partial piece"""
    eng, sched = year26["eng"], year26["sched"]
    n = len(sched)
    B = {"1": 1, "7": 7, "n-1": n - 1, "n": n, "n+5": n + 5}[where]
    eng.set_option("frozen_persistent", 1)
    eng.set_option("frozen_cache_pieces", 1)
    eng.set_option("frozen_cache_piece_rows", B)
    years, team = eng.counter("frozen_persistent_years"), eng.counter("frozen_team_years")
    fx_r, _ = eng.comp_fcn_frozen(year26["x"], sched)
    assert np.array_equal(eng.download(fx_r), year26["want"])
    assert eng.counter("frozen_persistent_years") == years + 1 and eng.counter("frozen_team_years") == team + 1
    fx_p, st_p = eng.comp_fcn_frozen(year26["xp"], sched)
    got = eng.download(fx_p)
    assert np.array_equal(got, year26["slab"]) and np.array_equal(got, year26["lpp"])
    assert eng.counter("frozen_persistent_years") == years + 2 and eng.counter("frozen_team_years") == team + 2
    st_s = year26["st_slab"]
    for key in ("nsteps", "nnewton", "nerr_checked", "max_err"):
        assert st_p[key] == st_s[key], key
    assert st_p["nerr_checked"] > 0
    assert eng.counter("frozen_cache_pieces") == math.ceil(n / B)
    eng.set_option("frozen_cache_pieces", 0)


def _case(name):
    from nk_ooc_amd.engine import ModuleEngine, forced_engine
    from nk_ooc_amd.grid import Grid2d

    rng = np.random.default_rng(11)
    if name == "iage_52_two_sweeps":
        eng = _iage(52)
        eng.set_option("lin_tol", 1.0e-3)
        x0, _, _ = _state(eng)
        xp0 = x0 * (1.0 + 1.0e-4 * rng.standard_normal(x0.shape))
    elif name == "forced_decay_22x9":
        eng = forced_engine(Grid2d.default(22, 9), {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay",
                                                     "forced_sms_decay_rate": "1.0e-8"})
        x0 = 1.0 + 0.2 * rng.standard_normal((1, 22, 9))
        xp0 = x0 * (1.0 + 1.0e-5 * rng.standard_normal(x0.shape))
    elif name == "forced_files_100x11":
        nz, ny = 100, 11
        times = np.array([-10.0, 40.0, 95.0, 200.0, 300.0]) * 86400.0
        eng = ModuleEngine(Grid2d.default(nz, ny), tc=1, surf_rate=(24.0 / 86400.0,), module_kind=2,
                           restore_series=(times, 1.0 + 0.2 * rng.standard_normal((5, ny))),
                           sms_series=(times, 3.0e-8 * rng.standard_normal((5, nz, ny))), time_range=(0.0, 40.0 * 86400.0))
        x0 = 0.6 + 0.2 * rng.standard_normal((1, nz, ny))
        xp0 = x0 * (1.0 + 1.0e-5 * rng.standard_normal(x0.shape))
    else:
        nz, ny = int(name.split("_")[1]), 48
        eng = _iage(nz, ny)
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (nz, ny))] * 2).copy()
        xp0 = x0 * (1.0 + 1.0e-4 * np.outer(np.sin(3.0 * np.linspace(0.0, 1.0, nz)), np.cos(2.0 * np.linspace(0.0, 1.0, ny)))[None])
    eng.set_option("device_ctl", 0)
    eng.set_option("frozen_alloc_async", 0)
    return eng, x0, xp0


@pytest.mark.parametrize("name", ["iage_52_two_sweeps", "forced_decay_22x9", "forced_files_100x11", "nz_250", "nz_320", "nz_512"])
def test_every_flavour_once(name):
    """team with two-sweep solves; the forced module kind (planes carry the forcing bundle); four levels per lane (adjacent
    columns, coefficients and W in LDS), five and eight (by column: step block and pivots filled from the piece at a step's
    first phase) -- pieces of five rows, an error estimate on every fifth step"""
    eng, x0, xp0 = _case(name)
    eng.set_option("frozen_err_check", 5)
    x, xp = eng.upload(x0), eng.upload(xp0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    _, st_s, st_p = _three_way(eng, x, xp, sched, eng.download(fx), 5)
    for key in ("nsteps", "nnewton", "nerr_checked", "max_err"):
        assert st_p[key] == st_s[key], key
    eng.close()


def test_growth_and_reuse():
    eng = _iage(26)
    _, x, xp = _state(eng)
    B = 64
    eng.set_option("frozen_cache_pieces", 1)
    eng.set_option("frozen_cache_piece_rows", B)
    fx, _, sched = eng.comp_fcn(x, record=True)
    fx_p, _ = eng.comp_fcn_frozen(x, sched)
    assert np.array_equal(eng.download(fx_p), eng.download(fx))
    held = eng.counter("frozen_cache_pieces")
    assert held == math.ceil(len(sched) / B) == eng.counter("frozen_cache_piece_allocs") and eng.counter("frozen_cache_builds") == 1
    # a second schedule: the pieces stay, only what is missing is added
    fx2, _, sched2 = eng.comp_fcn(xp, record=True)
    allocs = eng.counter("frozen_cache_piece_allocs")
    fx2_p, _ = eng.comp_fcn_frozen(xp, sched2)
    assert eng.counter("frozen_cache_builds") == 2 and eng.counter("frozen_persistent_years") == 2
    assert eng.counter("frozen_cache_piece_allocs") - allocs == max(0, math.ceil(len(sched2) / B) - held)
    assert np.array_equal(eng.download(fx2_p), eng.download(fx2))
    # one form at a time: pieces -> slab -> pieces
    pieces_bytes = eng.counter("frozen_cache_bytes")
    assert pieces_bytes > 0 and pieces_bytes % eng.counter("frozen_cache_pieces") == 0
    row_bytes = pieces_bytes // (eng.counter("frozen_cache_pieces") * B)
    eng.set_option("frozen_cache_pieces", 0)
    eng.comp_fcn_frozen(xp, sched2)
    n2 = len(sched2)
    assert eng.counter("frozen_cache_pieces") == 0 and eng.counter("frozen_cache_bytes") == row_bytes * (n2 + n2 // 6 + 16)
    eng.set_option("frozen_cache_pieces", 1)
    fx3_p, _ = eng.comp_fcn_frozen(xp, sched2)
    assert eng.counter("frozen_cache_bytes") == row_bytes * B * math.ceil(n2 / B) == row_bytes * B * eng.counter("frozen_cache_pieces")
    assert np.array_equal(eng.download(fx3_p), eng.download(fx2)) and eng.counter("frozen_persistent_years") == 4
    eng.close()


def test_walk_through_every_form():
    """ONE store through every form in turn -- slab, pieces, slab again, lean slab, lean pieces, full slab: after every change the
    launch-per-phase year's bits, one more one-launch year, exactly one more build, the other form gone (pieces held, lean
    flag, bytes = 8 x rows held x doubles of a row of that form); a repeat year in the same form builds and allocates nothing"""
    eng = _iage(26)
    eng.set_option("frozen_err_check", 7)
    _, x, xp = _state(eng)
    _, _, sched = eng.comp_fcn(x, record=True)
    n, B = len(sched), 7
    tc = eng.shape[0]                                            # one level per lane: kv_len = np = 26 x 64, nv = tc np, ntab = tc 26 x 14 x 64
    plane, nv, ntab = 26 * 64, tc * 26 * 64, tc * 26 * 14 * 64
    row_bytes = {0: 8 * (3 * plane + 5 * plane + 3 * nv + 3 * ntab), 1: 8 * (3 * plane + 5 * plane)}
    eng.set_option("frozen_persistent", 0)
    lpp = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
    eng.set_option("frozen_persistent", 1)
    eng.set_option("frozen_cache_piece_rows", B)
    for pieces, lean in ((0, 0), (1, 0), (0, 0), (0, 1), (1, 1), (0, 0)):
        eng.set_option("frozen_cache_pieces", pieces)
        eng.set_option("frozen_cache_lean", lean)
        years, builds = eng.counter("frozen_persistent_years"), eng.counter("frozen_cache_builds")
        got = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
        assert np.array_equal(got, lpp), (pieces, lean)
        assert eng.counter("frozen_persistent_years") == years + 1 and eng.counter("frozen_cache_builds") == builds + 1, (pieces, lean)
        assert eng.counter("frozen_cache_pieces") == (math.ceil(n / B) if pieces else 0), (pieces, lean)
        assert eng.counter("frozen_cache_lean") == lean, (pieces, lean)
        rows_held = math.ceil(n / B) * B if pieces else n + n // 6 + 16
        assert eng.counter("frozen_cache_bytes") == rows_held * row_bytes[lean], (pieces, lean)
        allocs = eng.counter("frozen_cache_piece_allocs")
        again = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
        assert np.array_equal(again, lpp), (pieces, lean)
        assert eng.counter("frozen_persistent_years") == years + 2 and eng.counter("frozen_cache_builds") == builds + 1, (pieces, lean)
        assert eng.counter("frozen_cache_piece_allocs") == allocs, (pieces, lean)
        assert eng.counter("frozen_cache_bytes") == rows_held * row_bytes[lean], (pieces, lean)
    eng.close()


def test_routing():
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    # a cache larger than allowed (the limit applies to the sum of the pieces)
    eng = _iage(26)
    eng.set_option("frozen_cache_pieces", 1)
    eng.set_option("frozen_cache_piece_rows", 7)
    _, x, _ = _state(eng)
    fx, _, sched = eng.comp_fcn(x, record=True)
    eng.set_option("frozen_cache_gb", 1.0e-3)
    fx_p, _ = eng.comp_fcn_frozen(x, sched)
    assert eng.counter("frozen_persistent_years") == 0 and eng.counter("frozen_cache_pieces") == 0
    assert np.array_equal(eng.download(fx_p), eng.download(fx))
    eng.close()
    # the single precision factorisation
    eng = _iage(26)
    eng.set_option("frozen_cache_pieces", 1)
    eng.set_option("factor_fp32", 1)
    _, x, _ = _state(eng)
    fx, _, sched = eng.comp_fcn(x, record=True)
    fx_p, _ = eng.comp_fcn_frozen(x, sched)
    assert eng.counter("frozen_persistent_years") == 0 and eng.counter("frozen_cache_pieces") == 0
    assert np.array_equal(eng.download(fx_p), eng.download(fx))
    eng.close()
    # a Jacobian that reads the state
    ph = phosphorus_engine(Grid2d.default(30, 12))
    ph.set_option("frozen_cache_pieces", 1)
    ph.set_option("frozen_cache_early", 1)
    rng = np.random.default_rng(8)
    x0 = np.stack([2.0 + 0.1 * rng.standard_normal((30, 12)), 0.05 + 0.005 * rng.standard_normal((30, 12)),
                   0.01 + 0.001 * rng.standard_normal((30, 12))])
    x = ph.upload(x0)
    fx, _, sched = ph.comp_fcn(x, record=True)
    fx2, _ = ph.comp_fcn_frozen(x, sched)
    assert np.array_equal(ph.download(fx2), ph.download(fx)) and ph.counter("frozen_persistent_years") == 0
    assert ph.counter("frozen_cache_early_requests") == 0 and ph.counter("frozen_cache_pieces") == 0
    ph.close()
    # the early request is the pieces' alone
    eng = _iage(26)
    eng.set_option("frozen_cache_early", 1)
    _, x, _ = _state(eng)
    fx, _, sched = eng.comp_fcn(x, record=True)
    assert eng.counter("frozen_cache_early_requests") == 0 and eng.counter("frozen_cache_pending") == 0
    fx_p, _ = eng.comp_fcn_frozen(x, sched)
    assert eng.counter("frozen_persistent_years") == 1 and eng.counter("frozen_cache_pieces") == 0
    assert np.array_equal(eng.download(fx_p), eng.download(fx))
    eng.close()


def test_early_request():
    engs = []
    for wait in (True, False):
        eng = _iage(26)
        engs.append(eng)
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_early", 1)
        eng.set_option("frozen_cache_piece_rows", 7)
        _, x, _ = _state(eng)
        fx, _, sched = eng.comp_fcn(x, record=True)
        assert eng.counter("frozen_cache_early_requests") == 1
        if wait:
            deadline = time.monotonic() + 10.0
            while eng.counter("frozen_cache_pending") and time.monotonic() < deadline:
                time.sleep(0.005)
            assert eng.counter("frozen_cache_pending") == 0
            allocs = eng.counter("frozen_cache_piece_allocs")
            fx_p, _ = eng.comp_fcn_frozen(x, sched)
            assert eng.counter("frozen_persistent_years") == 1                # one launch, on pieces that were there:
            assert eng.counter("frozen_cache_piece_allocs") == allocs         # (booked when adopted, none allocated by the year)
            assert eng.counter("frozen_cache_pieces") == math.ceil(len(sched) / 7)
        else:
            fx_p, _ = eng.comp_fcn_frozen(x, sched)                           # whichever path it took
        assert np.array_equal(eng.download(fx_p), eng.download(fx))
    for eng in engs:
        eng.close()


def test_products():
    """nk2d_gmres_solve with a schedule installed: the same numbers on pieces and on the slab, three one-launch years each"""
    n = 26
    eng = _iage(n)
    eng.set_region(np.ones((n, n), dtype=np.int32), np.outer(eng.grid.depth.delta, eng.grid.ypos.delta))
    _, x, _ = _state(eng)
    fx, _, sched = eng.comp_fcn(x, record=True)
    out = {}
    for flag in (0, 1):
        eng.set_option("frozen_cache_pieces", flag)
        eng.set_option("frozen_cache_piece_rows", 7)
        years = eng.counter("frozen_persistent_years")
        inc, info = eng.gmres_solve(x, fx, 0.0, 0, 3, sched=sched)
        out[flag] = (eng.download(inc), info["h_mat"].copy(), info["beta"].copy())
        assert eng.counter("frozen_persistent_years") == years + 3
        assert (eng.counter("frozen_cache_pieces") > 0) == bool(flag)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    eng.close()
