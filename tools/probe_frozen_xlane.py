"""one-launch frozen year: the Newton phase's cross-lane moves in the VALU (option "frozen_xlane" 1) against 0.  One process, one
engine; the arms alternate, five years each (a library without the option: twice five of its one arm); per arm the median and
the min - max of the launch (two HIP events around it, counter "frozen_launch_us") and of the year's wall time, the counters
that say which path the arm took, and whether its year is the first arm's bit for bit.  With NK2D_LIB_PATH naming a library of
the parent commit the one arm is that library's year: the parent's arm of the comparison, run as a process of its own -- its
checksum of the year is to be compared with this library's.

usage: probe_frozen_xlane.py [n ...]      (default 416 208)"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from nk_ooc_amd import _lib  # noqa: E402
from nk_ooc_amd.engine import iage_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

ARMS = (0, 1)
ROUNDS = 5


def _set(eng, bits):
    try:
        eng.set_option("frozen_xlane", bits)
        return True
    except Exception:       # (a library from before the option)
        return False


print(f"library {os.path.relpath(_lib.LIB_PATH)}", flush=True)
for n in [int(a) for a in sys.argv[1:]] or [416, 208]:
    eng = iage_engine(Grid2d.default(n, n))
    eng.set_option("frozen_alloc_async", 0)
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    x0 = np.stack([np.broadcast_to(col[:, None], (n, n))] * 2).copy()
    x = eng.upload(x0)
    zz = np.linspace(0.0, 1.0, n)
    xp = eng.upload(x0 * (1.0 + 1.0e-4 * np.outer(np.sin(3.0 * zz), np.cos(2.0 * zz))[None]))
    fx, st, sched = eng.comp_fcn(x, record=True)
    known = _set(eng, 0)
    arms = ARMS if known else (0,)
    ref, same, in_effect = None, {}, {}
    launch = {b: [] for b in arms}
    wall = {b: [] for b in arms}
    for bits in arms:       # (the cache is built and every arm's code is loaded before anything is timed)
        _set(eng, bits)
        got = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
        ref = got if ref is None else ref
        same[bits] = bool(np.array_equal(got, ref))
        in_effect[bits] = eng.counter("frozen_xlane_bits") if known else -1
    for _ in range(ROUNDS * (1 if known else len(ARMS))):
        for bits in arms:
            _set(eng, bits)
            us = eng.counter("frozen_launch_us")
            stats = eng.comp_fcn_frozen(xp, sched)[1]
            launch[bits].append(1.0e-3 * (eng.counter("frozen_launch_us") - us))
            wall[bits].append(1.0e3 * stats["seconds"])
    base = float(np.median(launch[arms[0]]))
    spread = max(launch[arms[0]]) - min(launch[arms[0]])
    print(f"{n}^2: {st['nsteps']} steps, one-launch years {eng.counter('frozen_persistent_years')}, lds bits {eng.counter('frozen_lds_bits')}, "
          f"early {eng.counter('frozen_early_bits')}, stage exchange {eng.counter('frozen_stage_exchange_bits')}; "
          f"spread of the {arms[0]} arm {spread:.3f} ms = {100.0 * spread / base:.2f} % (min - max over the median); "
          f"checksum of the year {float(np.sum(ref)):.17g}, sha1 {hashlib.sha1(ref.tobytes()).hexdigest()[:16]}", flush=True)
    for bits in arms:
        med = float(np.median(launch[bits]))
        print(f"  frozen_xlane {bits} (in effect {in_effect[bits]:2d}): launch median {med:8.3f} ms  [{min(launch[bits]):8.3f} - {max(launch[bits]):8.3f}]  "
              f"{100.0 * (base - med) / base:+.2f} % against {arms[0]}, {(base - med) / spread if spread > 0 else float('inf'):+.1f} spreads;  "
              f"year wall median {float(np.median(wall[bits])):8.3f} ms  [{min(wall[bits]):8.3f} - {max(wall[bits]):8.3f}];  same bits {same[bits]}",
              flush=True)
    eng.close()
