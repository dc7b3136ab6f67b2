"""one-launch frozen year: the kernel that carries the default year's body alone (option "frozen_dedicated" 1; 2: with the hand-over's
one-load poll) against k_frozen_persistent (0).  One process, one engine; the arms alternate, five years each (a library without
the option: three times five of its one arm); per arm the median and the min - max of the launch (two HIP events around it,
counter "frozen_launch_us") and of the year's wall time, the counters that say which kernel the arm ran, and whether its year is
the first arm's bit for bit.  With NK2D_LIB_PATH naming a library of the parent commit the one arm is that library's year: the
parent's arm of the comparison, run as a process of its own -- its checksum of the year is to be compared with this library's.

The rule the numbers are read by: an arm becomes the default only if, at 416^2, its median lies below the 0
arm's minimum and its gain is at least three times the 0 arm's min - max spread; arm 2 is preferred over arm 1 only if it clears
the same bar against arm 1.  The last line of every size says what the rule gives.

usage: probe_frozen_dedicated.py [n ...]      (default 416 208)"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from nk_ooc_amd import _lib  # noqa: E402
from nk_ooc_amd.engine import iage_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

ARMS = (0, 1, 2)
ROUNDS = 5


def _set(eng, value):
    try:
        eng.set_option("frozen_dedicated", value)
        return True
    except Exception:       # (a library from before the option)
        return False


def _clears(launch, arm, against):
    """the bar: median below the other arm's minimum, gain at least three of its min - max spreads"""
    med, base = float(np.median(launch[arm])), float(np.median(launch[against]))
    spread = max(launch[against]) - min(launch[against])
    return med < min(launch[against]) and base - med >= 3.0 * spread


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
    launch = {a: [] for a in arms}
    wall = {a: [] for a in arms}
    for arm in arms:        # (the cache is built and every arm's code is loaded before anything is timed)
        _set(eng, arm)
        got = eng.download(eng.comp_fcn_frozen(xp, sched)[0])
        ref = got if ref is None else ref
        same[arm] = bool(np.array_equal(got, ref))
        in_effect[arm] = eng.counter("frozen_dedicated_bits") if known else -1
    dedicated = eng.counter("frozen_dedicated_years") if known else 0
    for _ in range(ROUNDS * (1 if known else len(ARMS))):
        for arm in arms:
            _set(eng, arm)
            us = eng.counter("frozen_launch_us")
            stats = eng.comp_fcn_frozen(xp, sched)[1]
            launch[arm].append(1.0e-3 * (eng.counter("frozen_launch_us") - us))
            wall[arm].append(1.0e3 * stats["seconds"])
    dedicated = (eng.counter("frozen_dedicated_years") - dedicated) if known else 0
    base = float(np.median(launch[0]))
    spread = max(launch[0]) - min(launch[0])
    print(f"{n}^2: {st['nsteps']} steps, one-launch years {eng.counter('frozen_persistent_years')} (timed in the dedicated kernel: {dedicated}), "
          f"lds bits {eng.counter('frozen_lds_bits')}, early {eng.counter('frozen_early_bits')}, stage exchange "
          f"{eng.counter('frozen_stage_exchange_bits')}, xlane {eng.counter('frozen_xlane_bits')}; "
          f"spread of the 0 arm {spread:.3f} ms = {100.0 * spread / base:.2f} % (min - max over the median); "
          f"checksum of the year {float(np.sum(ref)):.17g}, sha1 {hashlib.sha1(ref.tobytes()).hexdigest()[:16]}", flush=True)
    for arm in arms:
        med = float(np.median(launch[arm]))
        print(f"  frozen_dedicated {arm} (in effect {in_effect[arm]:2d}): launch median {med:8.3f} ms  [{min(launch[arm]):8.3f} - {max(launch[arm]):8.3f}]  "
              f"{100.0 * (base - med) / base:+.2f} % against 0, {(base - med) / spread if spread > 0 else float('inf'):+.1f} spreads;  "
              f"year wall median {float(np.median(wall[arm])):8.3f} ms  [{min(wall[arm]):8.3f} - {max(wall[arm]):8.3f}];  same bits {same[arm]}",
              flush=True)
    if known:
        one, two = _clears(launch, 1, 0), _clears(launch, 2, 0)
        pick = 0
        if one or two:
            pick = 2 if (two and (not one or _clears(launch, 2, 1))) else 1
        print(f"  the rule at {n}^2: arm 1 clears the bar against 0: {one}; arm 2 against 0: {two}; arm 2 against 1: "
              f"{_clears(launch, 2, 1)}  ->  value {pick}" + ("" if in_effect[1] == 1 else "  (the dedicated kernel is not taken at this size)"),
              flush=True)
    eng.close()
