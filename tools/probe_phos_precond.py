"""phosphorus preconditioner: the apply as the five calls of PhosphorusPrecond.apply (two nk2d_shift_solve, three nk2d_axpby, one
nk2d_dot: two substitution chains, four stream synchronisations, one read-back) against ONE nk2d_precond_apply after
nk2d_precond_setup_states with the null vector (both systems down one chain, nothing read back).  One
phosphorus engine per size, precond_setup_state once; the two arms alternate back to back, `reps` repetitions of APPLIES applies each; then both
arms again on the same eigen-pair with pc_two_ended 1.  Medians and min - max, and pc_sub_launches per arm.  The rule, fixed
beforehand: the one call is "recommended" at a size only where its median is below the minimum of the five calls'.

Then, at the sizes given as k<nz>x<ny>: iterations per second of engine.gmres_solve against the KrylovSolver mirror on the
same problem (three iterations, the preconditioner of the mirror's solve; the mirror also writes its file trail).

    python tools/probe_phos_precond.py [reps] [sizes ...] [k<nz>x<ny> ...]      (default: 5 104 208 416 k22x9 k104x104)
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nk_ooc_amd.engine import phosphorus_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

APPLIES = 20


def stats(xs, unit, scale=1.0):
    xs = np.asarray(xs) * scale
    return f"{np.median(xs):.4g} {unit} ({xs.min():.4g} - {xs.max():.4g})"


def timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return time.perf_counter() - t0, out


def probe_apply(n, reps):
    grid = Grid2d.default(n, n)
    eng = phosphorus_engine(grid)
    eng.set_region(np.ones((n, n), dtype=np.int32), np.outer(grid.depth.delta, grid.ypos.delta))
    po4 = np.broadcast_to(np.interp(grid.depth.mid, [1.3e2, 2.6e2], [5.5e-3, 4.1e0])[:, None], (n, n)).copy()
    v = eng.upload(np.random.default_rng(0).standard_normal(eng.shape))
    eng.phos_pc_fused = False                      # the five calls are PhosphorusPrecond's own; the declaration is made below
    pc = eng.precond_setup_state(po4)
    out5, out1 = eng.new_vec(), eng.new_vec()
    for two_ended in (0, 1):
        if two_ended:
            eng.set_option("pc_two_ended", 1)      # the same eigen-pair, factorised from both ends
            eng.shift_factor(pc.t_mid, pc.scale, [pc.shift, 0.5 * pc.shift])
        eng.precond_set_nullspace(pc.e_hat)        # (the five calls do not look at it)
        pc.apply(v, out=out5)
        eng.precond_apply(v, out=out1)             # (warm)
        t5, t1, launches = [], [], {}
        for rep in range(reps):
            t5.append(timed(eng, lambda: [pc.apply(v, out=out5) for _ in range(APPLIES)])[0] / APPLIES)
            launches[5] = 2 * eng.counter("pc_sub_launches")
            t1.append(timed(eng, lambda: [eng.precond_apply(v, out=out1) for _ in range(APPLIES)])[0] / APPLIES)
            launches[1] = eng.counter("pc_sub_launches")
        same = np.array_equal(eng.download(out5), eng.download(out1))
        rule = "recommended" if np.median(t1) < np.min(t5) else "not recommended"
        print(f"phosphorus {n} x {n}, pc_two_ended={two_ended}: five calls {stats(t5, 'ms', 1e3)}, {launches[5]} dependent "
              f"mat-vec launches; one call {stats(t1, 'ms', 1e3)}, {launches[1]}; same bits: {same}; by the rule: {rule}",
              flush=True)
    eng.close()


def probe_solve(nz, ny, iters=3):
    from nk_ooc_amd.krylov_solver import KrylovSolver
    from nk_ooc_amd.model_config import ModelConfig
    from nk_ooc_amd.model_state import ModelState
    from nk_ooc_amd.setup_solver import gen_grid_vars_file, make_config

    with tempfile.TemporaryDirectory() as work:
        cfg = make_config(work, nz, ny, tracer_module_names="phosphorus",
                          extra_solverinfo={"krylov_max_iter": str(iters), "krylov_rel_tol": "1e-30"})
        gen_grid_vars_file(cfg["modelinfo"])
        ModelState.reset_class()
        ModelState.model_config_obj = ModelConfig(cfg["modelinfo"])
        ModelState.write_files = True
        iterate = ModelState("gen_init_iterate")
        hist = os.path.join(work, "hist_00.nc")
        fcn = iterate.comp_fcn(os.path.join(work, "fcn_00.nc"), None, hist)
        eng = iterate.tracer_modules[0].eng
        secs = []
        for k in range(2):      # the first solve builds the preconditioner (eigen-pair, factorisations); the second is timed
            info = dict(cfg["solverinfo"], krylov_workdir=os.path.join(work, f"krylov_{k:02d}"))
            solver = KrylovSolver(iterate, info, False, False, hist)
            secs.append(timed(eng, lambda: solver.solve(os.path.join(work, f"increment_{k:02d}.nc"), fcn))[0])
        mirror_its = solver.get_iteration()
        pc = eng._state_precond
        eng.precond_set_nullspace(pc.e_hat)
        x, fx, sched = iterate.tracer_modules[0].vec, fcn.tracer_modules[0].vec, fcn._sched["phosphorus"]
        eng.gmres_solve(x, fx, 1.0e-30, 0, iters, sched=sched)      # (warm)
        dt, (_, res) = timed(eng, lambda: eng.gmres_solve(x, fx, 1.0e-30, 0, iters, sched=sched))
        print(f"phosphorus {nz} x {ny}, {iters} GMRES iterations: KrylovSolver mirror {mirror_its / secs[1]:.3g} iterations/s "
              f"({secs[1]:.3f} s; the solve that also built the preconditioner {secs[0]:.3f} s), engine.gmres_solve "
              f"{res['iters'] / dt:.3g} iterations/s ({dt:.3f} s)", flush=True)
        ModelState.reset_class()


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[0]) if args else 5
    sizes = args[1:] or ["104", "208", "416", "k22x9", "k104x104"]
    for s in sizes:
        if s.startswith("k"):
            nz, ny = s[1:].split("x")
            probe_solve(int(nz), int(ny))
        else:
            probe_apply(int(s), reps)
