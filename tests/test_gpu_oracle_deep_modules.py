"""The tracer modules of the benchmark's mix at the benchmarked depth against the CPU oracle.

bench.py's module mix and its sharded run take `phosphorus` (module kind 1: three coupled tracers, a Jacobian that reads the
state, kernels that spill, a flavour of the resident kernel with two waves to a SIMD) at 416 levels: seven levels per lane
(E = 7).  tests/test_gpu_oracle_deep.py holds iage to the oracle there; this module does the same for phosphorus and for the
file-driven `forced` module (kind 2: file restoring, file source, sink threshold), on NARROW grids of full depth, whose
oracle years (SciPy's sparse LU on the restated reference functions, oracle/radau.py) take one to a few minutes of a core:

  phosphorus 416 x 4 (E = 7)  state and reference year of tests/golden/phosphorus_416x4.npz
  phosphorus 320 x 4 (E = 5)  state of test_gpu_stream._phos_state
  forced     416 x 4 (E = 7)  options, forcing records, state and reference year of tests/golden/forced_file_sink_thres_416x4.npz

For each of them:

  (a) the accepted steps of the default mode's free-running year, replayed launch by launch (options stream_years 0,
      frozen_persistent 0), against the oracle replaying the same rows.  Bounds: the project's own for these modules,
      < 1e-9 for phosphorus (test_phosphorus_comp_fcn: its coupled shifted solves are relaxed to an inner tolerance, not
      solved exactly) and < 1e-10 for forced (test_forced_file_kernels).  The same replay at lin_tol 1e-6 and 1e-9 is
      measured beside it (margins file): an error that falls with lin_tol is the inner tolerance, a floor that does not
      move would be a kernel fault.
  (b) the finite-difference product on frozen years, eng.jvp(x, fx, v, sched=sched), by launches, as a command stream
      (stream_years 3, `stream_years_run` asserted to advance) and -- phosphorus 416 x 4 -- as a command stream of the kernel
      with two waves to a SIMD (stream_two_waves 2, `stream_two_waves_kernel` asserted): the three bit for bit the same,
      no frozen year rejected, and against the oracle's (f(x + sigma v) - f(x)) / sigma from two replays with the
      device's sigma.  Bound: the project's 2e-3 -- unless, for phosphorus, the oracle's OWN product moves by more than
      2e-4 when every step is given one more Newton iteration (the finite difference cannot be known better than its own
      truncation); then ten times that sensitivity (the factor allows for accumulation over ~2000 steps).  The sensitivity
      is computed from four oracle replays alone and never from a device result; it and the bound go to the margins file.
  (c) the free-running year of the default mode against the reference's own solve_ivp year (the fixtures' `fcn`; for
      320 x 4 an oracle free-running year) at the reference's CI tolerance in margin form: atol 1e-6, rtol 1e-3 for
      phosphorus; atol 5e-5 for the thresholded forced module (test_forced_file_kernels: the kink of the sink threshold
      makes the map less smooth than the linear modules').

The device side of every case runs first; the oracle's eleven years then run side by side in spawned worker processes that
never touch the GPU (at most 11 of them).  Every measured error and margin goes to oracle_deep_modules_margins.json in the
output directory of test_gpu_oracle_deep.py's margins (copied to profiles/)."""
import multiprocessing as mp
import os
import time

import numpy as np
import pytest

from helpers import oracle_year_job, rel_err

pytestmark = pytest.mark.gpu

CASES = ["phosphorus_416x4", "phosphorus_320x4", "forced_416x4"]
MARGINS = "oracle_deep_modules_margins.json"      # beside the margins file of test_gpu_oracle_deep.py
REPLAY_BOUND = {"phosphorus": 1e-9, "forced": 1e-10}
FREE_ATOL = {"phosphorus": 1e-6, "forced": 5e-5}
LIN_TOL_SCAN = (1e-6, 1e-9)


def _case(case, golden_dir, tmp_path):
    """(engine factory, x0 [tc, nz, ny], picklable module description of helpers.oracle_module, reference year or None)"""
    from nk_ooc_amd.engine import forced_engine, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    kind, size = case.split("_")
    nz, ny = (int(v) for v in size.split("x"))
    if kind == "phosphorus":
        make = lambda: phosphorus_engine(Grid2d.default(nz, ny))      # noqa: E731
        if size == "416x4":
            g = np.load(f"{golden_dir}/phosphorus_416x4.npz")
            return make, np.asarray(g["y0"]).reshape(3, nz, ny), {"kind": "phosphorus"}, np.asarray(g["fcn"])
        from test_gpu_stream import _phos_state

        eng = make()
        x0 = _phos_state(eng, np.random.default_rng(1000 + nz))
        eng.close()
        return make, x0, {"kind": "phosphorus"}, None
    from test_gpu_forced import _file_modelinfo

    g = np.load(f"{golden_dir}/forced_file_sink_thres_416x4.npz")
    assert (int(g["nz"]), int(g["ny"])) == (nz, ny)
    info = _file_modelinfo(g, tmp_path)
    thres = float(g["sink_thres"])
    module = {"kind": "forced",
              "params": {"surf_restore_opt": str(g["surf_restore_opt"]), "surf_restore_const": float(g["surf_restore_const"]),
                         "sms_opt": str(g["sms_opt"]), "sms_decay_rate": float(g["sms_decay_rate"]), "sms_const": 0.0,
                         "sink_thres": thres if thres > 0.0 else None},
              "forcing": {"surf_restore_series": (np.asarray(g["rec_times"]), np.asarray(g["restore_vals"])),
                          "sms_series": (np.asarray(g["rec_times"]), np.asarray(g["sms_vals"]))}}
    return (lambda: forced_engine(Grid2d.default(nz, ny), info)), np.asarray(g["y0"]).reshape(1, nz, ny), module, \
        np.asarray(g["fcn"])


def _direction(kind, x0):
    """a smooth direction: for phosphorus a smooth RELATIVE change of every tracer (x + sigma v stays positive where the
    tracers span four decades), for forced a smooth field"""
    tc, nz, ny = x0.shape
    zz = np.linspace(0.0, 1.0, nz)[None, :, None]
    yy = ((np.arange(ny) + 0.5) / ny)[None, None, :]
    kk = np.arange(tc)[:, None, None]
    smooth = np.cos(np.pi * (1.5 * zz + 0.3 * kk)) * (1.0 + 0.5 * np.sin(2.0 * np.pi * yy))
    return x0 * smooth if kind == "phosphorus" else smooth


def _regions(eng):
    nz, ny = eng.shape[1:]
    eng.set_region(np.ones((nz, ny), dtype=np.int32), np.outer(eng.grid.depth.delta, eng.grid.ypos.delta))


def _device_side(case, make, x0):
    """everything the device computes for one case (see the module docstring); host arrays only"""
    kind = case.split("_")[0]
    eng = make()
    _regions(eng)
    x = eng.upload(x0)
    vd = eng.upload(_direction(kind, x0))
    vd = eng.scale(vd, 1.0 / np.sqrt(eng.dot(vd, vd)))
    v = eng.download(vd)
    # the default mode's free-running year
    fx, st, sched = eng.comp_fcn(x, record=True)
    rows = [(r[0], r[1], r[2], int(r[3]), r[4], r[5]) for r in sched]
    rec = {"kind": kind, "E": (eng.shape[1] + 63) // 64, "steps": len(rows), "rejected_free": st["nrejected"],
           "rows": rows, "fx": eng.download(fx).reshape(-1), "free_year_streams": eng.counter("stream_years_run")}
    # (a) its steps launch by launch, with the inner tolerance of a step replay
    eng.set_option("stream_years", 0)
    eng.set_option("frozen_persistent", 0)
    rec["replayed"] = eng.download(eng.comp_fcn(x, replay=np.array(rows))[0]).reshape(-1)
    # (b) the product on frozen years: by launches, then as a command stream
    w_l, sigma, stp_l = eng.jvp(x, fx, vd, sched=sched)
    eng.set_option("stream_years", 3)
    runs0 = eng.counter("stream_years_run")
    w_s, sigma_s, stp_s = eng.jvp(x, fx, vd, sched=sched)
    rec.update(sigma=float(sigma[0]), v=v.reshape(-1), w_launches=eng.download(w_l).reshape(-1),
               w_stream=eng.download(w_s).reshape(-1), same_sigma=bool(np.array_equal(sigma, sigma_s)),
               stream_years_advanced=eng.counter("stream_years_run") - runs0, stream_timeouts=eng.counter("stream_timeouts"),
               frozen_steps=(stp_l["nsteps"], stp_s["nsteps"]), frozen_rejected=(stp_l["nrejected"], stp_s["nrejected"]),
               fallbacks=eng.frozen_fallbacks())
    # (a), measured beside it: the same replay with tighter inner solves
    eng.set_option("stream_years", 0)
    rec["replayed_scan"] = {}
    for lin_tol in LIN_TOL_SCAN:
        eng.set_option("lin_tol", lin_tol)
        rec["replayed_scan"][lin_tol] = eng.download(eng.comp_fcn(x, replay=np.array(rows))[0]).reshape(-1)
    eng.close()
    if case == "phosphorus_416x4":
        # (b) once more in a context whose resident kernel is the flavour with two waves to a SIMD (the option is taken
        # before the context's first year): its own free-running year -- the same year -- and the product on its steps
        eng = make()
        _regions(eng)
        eng.set_option("stream_two_waves", 2)
        eng.set_option("stream_years", 3)
        eng.set_option("frozen_persistent", 0)
        x2, v2 = eng.upload(x0), eng.upload(v)
        fx2, _, sched2 = eng.comp_fcn(x2, record=True)
        runs0 = eng.counter("stream_years_run")
        w_2, sigma_2, stp_2 = eng.jvp(x2, fx2, v2, sched=sched2)
        rec["two_waves"] = {"same_year": bool(np.array_equal(sched2, sched) and np.array_equal(eng.download(fx2).reshape(-1), rec["fx"])),
                            "w": eng.download(w_2).reshape(-1), "same_sigma": bool(np.array_equal(sigma_2, sigma)),
                            "kernel": eng.counter("stream_two_waves_kernel"),
                            "stream_years_advanced": eng.counter("stream_years_run") - runs0,
                            "stream_timeouts": eng.counter("stream_timeouts"), "fallbacks": eng.frozen_fallbacks(),
                            "frozen_steps": stp_2["nsteps"], "frozen_rejected": stp_2["nrejected"]}
        eng.close()
    return rec


@pytest.fixture(scope="module")
def deep(golden_dir, tmp_path_factory):
    """device side of all cases first, then the oracle's years in parallel"""
    ctx = mp.get_context("spawn")
    pool = ctx.Pool(processes=min(11, max(2, (os.cpu_count() or 4) - 2)))
    out = {}
    try:
        t0 = time.time()
        for case in CASES:
            make, x0, module, ref = _case(case, golden_dir, tmp_path_factory.mktemp(case))
            rec = _device_side(case, make, x0)
            nz, ny = x0.shape[1:]
            xf, xp = x0.reshape(-1), x0.reshape(-1) + rec["sigma"] * rec["v"]
            rec.update(x0=xf, xp=xp, ref=ref)
            rows = rec["rows"]
            jobs = {"f0": (xf, rows), "f1": (xp, rows)}
            if rec["kind"] == "phosphorus":
                # the oracle-only sensitivity of the product: one more Newton iteration in every step
                more = [(r[0], r[1], r[2], r[3] + 1, r[4], r[5]) for r in rows]
                jobs.update(f0_more=(xf, more), f1_more=(xp, more))
            if ref is None:
                jobs["free"] = (xf, None)
            rec["jobs"] = {name: pool.apply_async(oracle_year_job, ((nz, ny, xv, rws, module),)) for name, (xv, rws) in jobs.items()}
            out[case] = rec
        t1 = time.time()
        for rec in out.values():
            rec["oracle"] = {name: job.get(timeout=2000) for name, job in rec.pop("jobs").items()}
        _record("seconds.device_side", round(t1 - t0, 1))
        _record("seconds.waiting_for_the_oracle", round(time.time() - t1, 1))
        yield out
    finally:
        pool.terminate()
        pool.join()


def _record(key, value):
    from test_gpu_oracle_deep import _record as record_beside

    record_beside(key, value, fname=MARGINS)


@pytest.mark.parametrize("case", CASES)
def test_default_mode_steps_replayed_by_the_oracle(deep, case):
    rec = deep[case]
    f0 = rec["oracle"]["f0"]
    err = rel_err(rec["replayed"], f0)
    _record(f"{case}.levels_per_lane", rec["E"])
    _record(f"{case}.steps", rec["steps"])
    _record(f"{case}.replay_vs_oracle", err)
    for lin_tol, replayed in rec["replayed_scan"].items():
        _record(f"{case}.replay_vs_oracle.lin_tol_{lin_tol:g}", rel_err(replayed, f0))
    # (how far the free-running year itself, with its inexact inner solves, is from the oracle on its steps: a figure only)
    _record(f"{case}.free_running_vs_oracle_replay", rel_err(rec["fx"], f0))
    print(f"{case}: replay against the oracle {err:.3e} (bound {REPLAY_BOUND[rec['kind']]:g})")
    assert rec["free_year_streams"] == 1, "the default mode's free-running year did not run as a command stream"
    assert err < REPLAY_BOUND[rec["kind"]]


@pytest.mark.parametrize("case", CASES)
def test_frozen_product_against_the_oracle(deep, case):
    rec = deep[case]
    orc = rec["oracle"]
    # x + sigma v keeps the sign of every cell (phosphorus: stays positive)
    assert np.all(np.sign(rec["xp"]) == np.sign(rec["x0"])) and (rec["kind"] != "phosphorus" or rec["xp"].min() > 0.0)
    w_oracle = (orc["f1"] - orc["f0"]) / rec["sigma"]
    bound = 2e-3
    if rec["kind"] == "phosphorus":
        sens = rel_err((orc["f1_more"] - orc["f0_more"]) / rec["sigma"], w_oracle)
        _record(f"{case}.oracle_product_sensitivity_to_one_more_newton_iteration", sens)
        if not sens < 2e-4:
            bound = 10.0 * sens
    _record(f"{case}.frozen_product_bound", bound)
    paths = {"launches": rec["w_launches"], "stream": rec["w_stream"]}
    if case == "phosphorus_416x4":
        paths["two_waves"] = rec["two_waves"]["w"]
    errs = {name: rel_err(w, w_oracle) for name, w in paths.items()}
    for name, err in errs.items():
        _record(f"{case}.frozen_product_{name}_vs_oracle", err)
    print(f"{case}: frozen product against the oracle {errs} (bound {bound:g})")
    # every path was the path it claims to be, and every frozen year stood
    assert rec["stream_years_advanced"] >= 1 and rec["stream_timeouts"] == 0 and rec["same_sigma"]
    assert rec["fallbacks"] == 0 and rec["frozen_rejected"] == (0, 0) and rec["frozen_steps"] == (rec["steps"], rec["steps"])
    assert np.array_equal(rec["w_launches"], rec["w_stream"])
    if case == "phosphorus_416x4":
        two = rec["two_waves"]
        assert two["kernel"] == 1 and two["stream_years_advanced"] >= 1 and two["stream_timeouts"] == 0
        assert two["same_year"] and two["same_sigma"] and two["fallbacks"] == 0
        assert two["frozen_rejected"] == 0 and two["frozen_steps"] == rec["steps"]
        assert np.array_equal(two["w"], rec["w_launches"])
    for name, err in errs.items():
        assert err < bound, (name, err, bound)


@pytest.mark.parametrize("case", CASES)
def test_free_running_default_mode_against_the_reference_year(deep, case):
    rec = deep[case]
    ref = rec["ref"] if rec["ref"] is not None else rec["oracle"]["free"]
    margin = float(np.max(np.abs(rec["fx"] - ref) / (FREE_ATOL[rec["kind"]] + 1.0e-3 * np.abs(ref))))
    _record(f"{case}.free_running_vs_{'reference' if rec['ref'] is not None else 'oracle'}_ci_margin", margin)
    print(f"{case}: free-running year, margin {margin:.3f} of the CI tolerance")
    assert margin < 1.0
