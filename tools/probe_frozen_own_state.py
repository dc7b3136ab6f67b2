"""one-launch frozen year: a column's own state on its compute unit (option "frozen_coef_lds" bits 16: own Y in LDS, 32: own stage
values in registers) against the set of before, 15.  One process, one engine; the arms alternate, five years each; per arm the
median and the min - max of the launch (two HIP events around it, counter "frozen_launch_us") and of the year's wall time.
With NK2D_LIB_PATH naming a library of the parent commit every arm is that library's 15 (it masks the option with 15): the arm
for the norm partials nobody reads, which the new library leaves out whatever the option says.

usage: probe_frozen_own_state.py [n ...]      (default 416)"""
import os
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from nk_ooc_amd import _lib  # noqa: E402
from nk_ooc_amd.engine import iage_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

ARMS = (15, 31, 47, 63)
ROUNDS = 5

print(f"library {os.path.relpath(_lib.LIB_PATH)}", flush=True)
for n in [int(a) for a in sys.argv[1:]] or [416]:
    eng = iage_engine(Grid2d.default(n, n))
    eng.set_option("frozen_alloc_async", 0)
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    x0 = np.stack([np.broadcast_to(col[:, None], (n, n))] * 2).copy()
    x = eng.upload(x0)
    zz = np.linspace(0.0, 1.0, n)
    xp = eng.upload(x0 * (1.0 + 1.0e-4 * np.outer(np.sin(3.0 * zz), np.cos(2.0 * zz))[None]))
    fx, st, sched = eng.comp_fcn(x, record=True)
    ref, same, in_effect = None, {}, {}
    launch = {b: [] for b in ARMS}
    wall = {b: [] for b in ARMS}
    for bits in ARMS:       # (the cache is built and every arm's code is loaded before anything is timed)
        eng.set_option("frozen_coef_lds", bits)
        got = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
        ref = got if ref is None else ref
        same[bits] = bool(np.array_equal(got, ref))
        try:
            in_effect[bits] = eng.counter("frozen_lds_bits")
        except Exception:       # (a library from before the counter)
            in_effect[bits] = -1
    for _ in range(ROUNDS):
        for bits in ARMS:
            eng.set_option("frozen_coef_lds", bits)
            us = eng.counter("frozen_launch_us")
            stats = eng.comp_fcn_frozen(xp, sched)[1]
            launch[bits].append(1.0e-3 * (eng.counter("frozen_launch_us") - us))
            wall[bits].append(1.0e3 * stats["seconds"])
    base = float(np.median(launch[ARMS[0]]))
    print(f"{n}^2: {st['nsteps']} steps, one-launch years {eng.counter('frozen_persistent_years')}; spread of the {ARMS[0]} arm "
          f"{100.0 * (max(launch[ARMS[0]]) - min(launch[ARMS[0]])) / base:.2f} % (min - max over the median)", flush=True)
    for bits in ARMS:
        med = float(np.median(launch[bits]))
        print(f"  frozen_coef_lds {bits:2d} (in effect {in_effect[bits]:2d}): launch median {med:8.3f} ms  [{min(launch[bits]):8.3f} - {max(launch[bits]):8.3f}]  "
              f"{100.0 * (base - med) / base:+.2f} % against {ARMS[0]};  year wall median {float(np.median(wall[bits])):8.3f} ms  "
              f"[{min(wall[bits]):8.3f} - {max(wall[bits]):8.3f}];  same bits {same[bits]}", flush=True)
    eng.close()
