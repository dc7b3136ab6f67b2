"""preconditioner set-up: pivot blocks of the Gauss-Jordan inversions by four waves through LDS (option pc_pivot_wave 0)
against one wave in registers (1), one context per size, the two values alternating back to back:
iage set-up with pc_fused 1 and 0 and pc_two_ended 0 and 1, then the phosphorus shifted systems (shift_factor with two
shifts, one precond_setup_state).  A change of pc_two_ended is a new allocation, so every series of timed set-ups follows
an untimed one.  Medians and min - max of `reps` repetitions, the counter pc_pivot_wave_steps, and whether the applies of
the two values agree bit for bit.  The rule (fixed before the measurement): the option is recommended at a size only if
the median with 1 lies below the minimum with 0.

    python tools/probe_pc_pivot_wave.py [reps] [iage sizes ...] [p<phosphorus size> ...]      (default: 5 104 208 416 p416)
    python tools/probe_pc_pivot_wave.py trace <0|1> [size]    one iage set-up with pc_fused 1 and one with 0 at that value
                                                              (default 416), for a kernel trace of the three kernels
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nk_ooc_amd.engine import iage_engine, phosphorus_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

YEAR = 365.0 * 86400.0


def stats(xs, unit, scale=1.0):
    xs = np.asarray(xs) * scale
    return f"{np.median(xs):.4g} {unit} ({xs.min():.4g} - {xs.max():.4g})"


def verdict(t):
    return "recommended" if np.median(t[1]) < np.min(t[0]) else "NOT recommended"


def timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return time.perf_counter() - t0, out


def probe_iage(n, reps):
    eng = iage_engine(Grid2d.default(n, n))
    v = eng.upload(np.random.default_rng(0).standard_normal((2, n, n)))
    for two_ended in (0, 1):
        eng.set_option("pc_two_ended", two_ended)
        for fused in (1, 0):
            eng.set_option("pc_fused", fused)
            eng.set_option("pc_pivot_wave", 0)
            eng.precond_setup()                       # (allocates; untimed)
            setup, steps, res = {0: [], 1: []}, {}, {}
            for rep in range(reps):
                for wave in (0, 1):
                    eng.set_option("pc_pivot_wave", wave)
                    setup[wave].append(timed(eng, eng.precond_setup)[0])
                    steps[wave] = eng.counter("pc_pivot_wave_steps")
                    if rep == 0:
                        res[wave] = eng.download(eng.precond_apply(v))
            for wave in (0, 1):
                print(f"iage {n} x {n}, pc_fused={fused}, pc_two_ended={two_ended}: pc_pivot_wave={wave}: set-up "
                      f"{stats(setup[wave], 's')}, pc_pivot_wave_steps {steps[wave]}", flush=True)
            print(f"iage {n} x {n}, pc_fused={fused}, pc_two_ended={two_ended}: {verdict(setup)} by the rule; applies "
                  f"{'bit for bit equal' if np.array_equal(res[0], res[1]) else 'DIFFER'}", flush=True)
    eng.close()


def probe_phosphorus(n, reps):
    grid = Grid2d.default(n, n)
    eng = phosphorus_engine(grid)
    po4 = np.broadcast_to(np.interp(grid.depth.mid, [1.3e2, 2.6e2], [5.5e-3, 4.1e0])[:, None], (n, n)).copy()
    ylin = np.zeros(eng.shape)
    ylin[0] = po4
    eng.set_lin_state(eng.upload(ylin))
    eng.shift_factor(0.5 * YEAR, YEAR, [0.02, -0.03])     # (allocates; untimed)
    factor, state, steps = {0: [], 1: []}, {0: [], 1: []}, {}
    for rep in range(reps):
        for wave in (0, 1):
            eng.set_option("pc_pivot_wave", wave)
            factor[wave].append(timed(eng, lambda: eng.shift_factor(0.5 * YEAR, YEAR, [0.02, -0.03]))[0])
            steps[wave] = eng.counter("pc_pivot_wave_steps")
            state[wave].append(timed(eng, lambda: eng.precond_setup_state(po4))[0])
    for wave in (0, 1):
        print(f"phosphorus {n} x {n}: pc_pivot_wave={wave}: shift_factor, two shifts {stats(factor[wave], 's')}, "
              f"precond_setup_state {stats(state[wave], 's')}, pc_pivot_wave_steps {steps[wave]}", flush=True)
    print(f"phosphorus {n} x {n}: shift_factor {verdict(factor)}, precond_setup_state {verdict(state)} by the rule", flush=True)
    eng.close()


def trace(wave, n):
    eng = iage_engine(Grid2d.default(n, n))
    eng.set_option("pc_pivot_wave", wave)
    for fused in (1, 0):
        eng.set_option("pc_fused", fused)
        dt, _ = timed(eng, eng.precond_setup)
        print(f"iage {n} x {n}, pc_fused={fused}, pc_pivot_wave={wave}: set-up {dt:.4g} s (traced), pc_pivot_wave_steps "
              f"{eng.counter('pc_pivot_wave_steps')}", flush=True)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "trace":
        trace(int(args[1]), int(args[2]) if len(args) > 2 else 416)
        sys.exit(0)
    reps = int(args[0]) if args else 5
    sizes = args[1:] or ["104", "208", "416", "p416"]
    for s in sizes:
        if s.startswith("p"):
            probe_phosphorus(int(s[1:]), reps)
        else:
            probe_iage(int(s), reps)
