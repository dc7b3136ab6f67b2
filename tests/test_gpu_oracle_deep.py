"""The benchmarked instantiation against the CPU oracle (round-3 verdict, weak 1 / next 1).

bench.py times iage at 416 x 416: seven levels per lane, the frozen years of the products in ONE launch.  A 416 x 416 year is
out of the CPU oracle's reach (days), a NARROW grid of the same depth is not: 416 x 8 runs exactly the kernels of the bench
-- E = 7, the same launches, the same one-launch year -- on 2 x 8 columns, and the oracle (SciPy's sparse LU on the restated
reference functions, oracle/radau.py after scipy/integrate/_ivp/radau.py as driven by
/root/reference/nk_ooc/py_driver_2d/model_state.py:102-121) integrates it in two to three minutes.  For 416 x 8 (E = 7),
320 x 8 (E = 5) and 512 x 6 (E = 8):

  (a) the steps of the default mode's free-running year replayed launch by launch against the oracle replaying the same
      steps: <= 1e-10;
  (b) the finite-difference product (/root/reference/nk_ooc/model_state_base.py:492-527) on frozen years with the
      one-launch year forced on -- `frozen_persistent_years` asserted -- against the oracle differencing two replays: <= 2e-3;
  (c) the free-running year of the default mode against the oracle's own free-running year (SciPy's decisions) at the
      reference's CI tolerance (atol 1e-6, rtol 1e-3).

The oracle's eleven years (nine of the deep grids, two of 52 x 52) run side by side in spawned worker processes (they never touch the GPU) while the device side of
all three sizes is long done; the margins go to gpurun_out/r04_oracle_deep_margins.json (copied to profiles/)."""
import json
import multiprocessing as mp
import os

import numpy as np
import pytest

from helpers import oracle_iage, oracle_year_job, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(416, 8), (320, 8), (512, 6)]
# ... and 52 x 52 (one level per lane; the one-launch year of a four-wave team per column): replay and product only -- its two
# oracle years ride in the same pool of worker processes instead of taking 160 s of a test of their own
# (tests/test_gpu_comp_fcn.py had them until round 4); the free-running 52 x 52 year is held against solve_ivp goldens there
SIZES_REPLAY = [(52, 52)] + SIZES          # (its oracle years are the longest: queued first)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state(nz, ny, depth_mid):
    rng = np.random.default_rng(1000 + nz)
    col = np.interp(depth_mid, [55.0, 200.0], [0.0, 2.0])
    x0 = np.stack([np.broadcast_to(col[:, None], (nz, ny))] * 2) + 0.01 * rng.standard_normal((2, nz, ny))
    v = np.cumsum(rng.standard_normal(x0.shape), axis=1)
    return x0, v


@pytest.fixture(scope="module")
def deep():
    """device side of all sizes first, then the oracle's years in parallel"""
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    ctx = mp.get_context("spawn")
    pool = ctx.Pool(processes=min(11, max(2, (os.cpu_count() or 4) - 2)))
    out = {}
    try:
        for nz, ny in SIZES_REPLAY:
            model, _ = oracle_iage(nz, ny)
            eng = iage_engine(Grid2d.default(nz, ny, 0.1, 1000.0))
            eng.set_option("device_ctl", 0)
            eng.set_option("frozen_alloc_async", 0)
            weight = np.outer(model.depth.delta, model.ypos.delta)
            eng.set_region(np.ones((nz, ny), dtype=np.int32), weight)
            x0, v = _state(nz, ny, model.depth.mid)
            x, vd = eng.upload(x0), eng.upload(v)
            vd = eng.scale(vd, 1.0 / np.sqrt(eng.dot(vd, vd)))
            v = eng.download(vd)
            fx, st, sched = eng.comp_fcn(x, record=True)
            rows = [(r[0], r[1], r[2], int(r[3]), r[4], r[5]) for r in sched]
            # (a) launch by launch, with the inner tolerance of a replay
            eng.set_option("frozen_persistent", 0)
            replayed, _, _ = eng.comp_fcn(x, replay=sched)
            # (b) the product on frozen years, the one-launch year forced on
            eng.set_option("frozen_persistent", 1)
            eng.set_option("frozen_cache_after", 0)
            years0 = eng.counter("frozen_persistent_years")
            w, sigma, stp = eng.jvp(x, fx, vd, sched=sched)
            years = eng.counter("frozen_persistent_years") - years0
            # ... and the same product launch by launch
            eng.set_option("frozen_persistent", 0)
            w_l, _, _ = eng.jvp(x, fx, vd, sched=sched)
            rec = {
                "E": (nz + 63) // 64, "steps": len(sched), "x0": x0, "fx": eng.download(fx).reshape(-1),
                "replayed": eng.download(replayed).reshape(-1), "w": eng.download(w).reshape(-1),
                "w_launches": eng.download(w_l).reshape(-1), "sigma": float(sigma[0]),
                "one_launch_years": years, "fallbacks": eng.frozen_fallbacks(), "rejected": stp["nrejected"],
                "jobs": [pool.apply_async(oracle_year_job, ((nz, ny, x0.reshape(-1), rows),)),
                         pool.apply_async(oracle_year_job, ((nz, ny, (x0 + float(sigma[0]) * v).reshape(-1), rows),))]
                        + ([pool.apply_async(oracle_year_job, ((nz, ny, x0.reshape(-1), None),))] if (nz, ny) in SIZES else []),
            }
            eng.close()
            out[(nz, ny)] = rec
        for rec in out.values():
            rec["oracle"] = [job.get(timeout=1500) for job in rec.pop("jobs")]
        yield out
    finally:
        pool.terminate()
        pool.join()


def _record(key, value, fname=None):
    """one figure into the margins file of this module -- or into `fname` beside it (test_gpu_oracle_deep_modules.py)"""
    path = os.path.join(ROOT, "gpurun_out", "r04_oracle_deep_margins.json")
    if fname is not None:
        path = os.path.join(os.path.dirname(path), fname)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("nz,ny", SIZES_REPLAY)
def test_default_mode_steps_replayed_by_the_oracle(deep, nz, ny):
    rec = deep[(nz, ny)]
    f0 = rec["oracle"][0]
    err = rel_err(rec["replayed"], f0)
    _record(f"{nz}x{ny}.replay_vs_oracle", err)
    assert err < 1e-10
    # the free-running year itself is that map to the Newton tolerance
    assert np.allclose(rec["fx"], f0, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("nz,ny", SIZES_REPLAY)
def test_one_launch_frozen_product_against_the_oracle(deep, nz, ny):
    rec = deep[(nz, ny)]
    assert rec["one_launch_years"] >= 1, "the perturbed year of the product did not take the one-launch path"
    assert rec["fallbacks"] == 0 and rec["rejected"] == 0
    f0, f1 = rec["oracle"][0], rec["oracle"][1]
    w_oracle = (f1 - f0) / rec["sigma"]
    err = rel_err(rec["w"], w_oracle)
    err_l = rel_err(rec["w_launches"], w_oracle)
    _record(f"{nz}x{ny}.frozen_product_one_launch_vs_oracle", err)
    _record(f"{nz}x{ny}.frozen_product_launches_vs_oracle", err_l)
    _record(f"{nz}x{ny}.levels_per_lane", rec["E"])
    _record(f"{nz}x{ny}.steps", rec["steps"])
    assert err < 2e-3 and err_l < 2e-3
    # the two device paths are the same discrete map
    assert np.array_equal(rec["w"], rec["w_launches"])


@pytest.mark.parametrize("nz,ny", SIZES)
def test_free_running_default_mode_against_the_oracles_year(deep, nz, ny):
    rec = deep[(nz, ny)]
    ref = rec["oracle"][2]
    margin = float(np.max(np.abs(rec["fx"] - ref) / (1.0e-6 + 1.0e-3 * np.abs(ref))))
    _record(f"{nz}x{ny}.free_running_vs_oracle_ci_margin", margin)
    assert margin < 1.0
