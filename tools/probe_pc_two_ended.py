"""preconditioner: block elimination over ypos = 0 .. ny - 1 (option pc_two_ended 0) against the elimination from both ends at
once (1: two chains of half the length in the same launches), one context per size, the two values
alternating back to back: iage set-up and apply with the counters pc_setup_rounds / pc_sub_launches, then the phosphorus
shifted systems (shift_factor with two shifts, one precond_setup_state).  A change of the value is a new allocation, so
every timed set-up follows an untimed one with the same value.  Medians and min - max of `reps` repetitions.

    python tools/probe_pc_two_ended.py [reps] [iage sizes ...] [p<phosphorus size> ...]      (default: 5 104 208 416 p416)
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


def probe_iage(n, reps):
    eng = iage_engine(Grid2d.default(n, n))
    v = eng.upload(np.random.default_rng(0).standard_normal((2, n, n)))
    setup, apply, counters, res = {0: [], 1: []}, {0: [], 1: []}, {}, {}
    for rep in range(reps):
        for two_ended in (0, 1):
            eng.set_option("pc_two_ended", two_ended)
            eng.precond_setup()                       # (allocates; untimed)
            setup[two_ended].append(timed(eng, eng.precond_setup)[0])
            out = eng.precond_apply(v)                # (warm)
            dt, _ = timed(eng, lambda: [eng.precond_apply(v, out=out) for _ in range(APPLIES)])
            apply[two_ended].append(dt / APPLIES)
            counters[two_ended] = (eng.counter("pc_setup_rounds"), eng.counter("pc_sub_launches"))
            res[two_ended] = eng.download(out)
    for two_ended in (0, 1):
        print(f"iage {n} x {n}: pc_two_ended={two_ended}: set-up {stats(setup[two_ended], 's')}, apply "
              f"{stats(apply[two_ended], 'ms', 1e3)}, pc_setup_rounds {counters[two_ended][0]}, pc_sub_launches "
              f"{counters[two_ended][1]}", flush=True)
    den = np.max(np.abs(res[0]))
    print(f"iage {n} x {n}: applies of the two orders differ by {np.max(np.abs(res[1] - res[0])) / den:.2e} (relative, max norm)",
          flush=True)
    eng.close()


def probe_phosphorus(n, reps):
    grid = Grid2d.default(n, n)
    eng = phosphorus_engine(grid)
    po4 = np.broadcast_to(np.interp(grid.depth.mid, [1.3e2, 2.6e2], [5.5e-3, 4.1e0])[:, None], (n, n)).copy()
    ylin = np.zeros(eng.shape)
    ylin[0] = po4
    eng.set_lin_state(eng.upload(ylin))
    factor, state, rounds = {0: [], 1: []}, {0: [], 1: []}, {}
    for rep in range(reps):
        for two_ended in (0, 1):
            eng.set_option("pc_two_ended", two_ended)
            eng.shift_factor(0.5 * YEAR, YEAR, [0.02, -0.03])     # (allocates; untimed)
            factor[two_ended].append(timed(eng, lambda: eng.shift_factor(0.5 * YEAR, YEAR, [0.02, -0.03]))[0])
            rounds[two_ended] = eng.counter("pc_setup_rounds")
            state[two_ended].append(timed(eng, lambda: eng.precond_setup_state(po4))[0])
    for two_ended in (0, 1):
        print(f"phosphorus {n} x {n}: pc_two_ended={two_ended}: shift_factor, two shifts {stats(factor[two_ended], 's')}, "
              f"precond_setup_state {stats(state[two_ended], 's')}, pc_setup_rounds {rounds[two_ended]}", flush=True)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[0]) if args else 5
    sizes = args[1:] or ["104", "208", "416", "p416"]
    for s in sizes:
        if s.startswith("p"):
            probe_phosphorus(int(s[1:]), reps)
        else:
            probe_iage(int(s), reps)
