"""preconditioner set-up: Gauss-Jordan panel steps of 32 pivots (option pc_panel 32, the default) against 64 (DESIGN.md
section 4), one context per size, the two values alternating back to back: iage set-up with pc_two_ended 0 and 1, then the
phosphorus shifted systems (shift_factor with two shifts, one precond_setup_state).  A change of pc_two_ended is a new
allocation, so every series of timed set-ups follows an untimed one.  Medians and min - max of `reps` repetitions, the
counters pc_panel_steps and pc_setup_rounds, and the relative difference between the applies of the two factorisations
(printed, not judged: the two differ in rounding).  The rule (fixed before the measurement): 64 is recommended for a case
only if its median lies below the minimum with 32 in the same call.

    python tools/probe_pc_panel.py [reps] [iage sizes ...] [p<phosphorus size> ...]      (default: 5 104 208 416 p416)
    python tools/probe_pc_panel.py trace <32|64> [size]       one iage set-up at that value (default 416), for a kernel trace
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
PANELS = (32, 64)


def stats(xs, unit, scale=1.0):
    xs = np.asarray(xs) * scale
    return f"{np.median(xs):.4g} {unit} ({xs.min():.4g} - {xs.max():.4g})"


def verdict(t):
    return "64 recommended" if np.median(t[64]) < np.min(t[32]) else "64 NOT recommended"


def rel_diff(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


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
        eng.set_option("pc_panel", 32)
        eng.precond_setup()                       # (allocates; untimed)
        setup, steps, rounds, res = {32: [], 64: []}, {}, {}, {}
        for rep in range(reps):
            for panel in PANELS:
                eng.set_option("pc_panel", panel)
                setup[panel].append(timed(eng, eng.precond_setup)[0])
                steps[panel] = eng.counter("pc_panel_steps")
                rounds[panel] = eng.counter("pc_setup_rounds")
                if rep == 0:
                    res[panel] = eng.download(eng.precond_apply(v))
        for panel in PANELS:
            print(f"iage {n} x {n}, pc_two_ended={two_ended}: pc_panel={panel}: set-up {stats(setup[panel], 's')}, "
                  f"pc_panel_steps {steps[panel]}, pc_setup_rounds {rounds[panel]}", flush=True)
        same = np.array_equal(res[32], res[64])
        print(f"iage {n} x {n}, pc_two_ended={two_ended}: {verdict(setup)} by the rule; applies "
              f"{'bit for bit equal' if same else 'differ'}, relative difference {rel_diff(res[64], res[32]):.2e}", flush=True)
    eng.set_option("pc_panel", 32)
    eng.close()


def probe_phosphorus(n, reps):
    grid = Grid2d.default(n, n)
    eng = phosphorus_engine(grid)
    po4 = np.broadcast_to(np.interp(grid.depth.mid, [1.3e2, 2.6e2], [5.5e-3, 4.1e0])[:, None], (n, n)).copy()
    ylin = np.zeros(eng.shape)
    ylin[0] = po4
    eng.set_lin_state(eng.upload(ylin))
    shifts = [0.02, -0.03]
    v = eng.upload(np.random.default_rng(0).standard_normal(eng.shape))
    eng.shift_factor(0.5 * YEAR, YEAR, shifts)     # (allocates; untimed)
    factor, state, steps, rounds, res = {32: [], 64: []}, {32: [], 64: []}, {}, {}, {}
    for rep in range(reps):
        for panel in PANELS:
            eng.set_option("pc_panel", panel)
            factor[panel].append(timed(eng, lambda: eng.shift_factor(0.5 * YEAR, YEAR, shifts))[0])
            steps[panel] = eng.counter("pc_panel_steps")
            rounds[panel] = eng.counter("pc_setup_rounds")
            if rep == 0:
                res[panel] = [eng.download(eng.shift_solve(i, v)) for i in range(len(shifts))]
            state[panel].append(timed(eng, lambda: eng.precond_setup_state(po4))[0])
    for panel in PANELS:
        print(f"phosphorus {n} x {n}: pc_panel={panel}: shift_factor, two shifts {stats(factor[panel], 's')}, "
              f"precond_setup_state {stats(state[panel], 's')}, pc_panel_steps {steps[panel]}, pc_setup_rounds {rounds[panel]}",
              flush=True)
    diff = max(rel_diff(a, b) for a, b in zip(res[64], res[32]))
    print(f"phosphorus {n} x {n}: shift_factor {verdict(factor)}, precond_setup_state {verdict(state)} by the rule; shifted "
          f"solves differ by {diff:.2e} (relative)", flush=True)
    eng.set_option("pc_panel", 32)
    eng.close()


def trace(panel, n):
    eng = iage_engine(Grid2d.default(n, n))
    eng.set_option("pc_panel", panel)
    dt, _ = timed(eng, eng.precond_setup)
    print(f"iage {n} x {n}, pc_panel={panel}: set-up {dt:.4g} s (traced), pc_panel_steps {eng.counter('pc_panel_steps')}, "
          f"pc_setup_rounds {eng.counter('pc_setup_rounds')}", flush=True)
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
