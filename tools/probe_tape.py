"""one frozen year at 416 x 416 four ways (option "frozen_tape"): by launches, as a host-fed command
stream (stream_years 3), from a command tape, and -- iage only -- on the schedule cache of the one-launch year.  The same
schedule and state every time (x + sigma v on the steps recorded at x); every way is checked bit for bit against the
launches.  Best of `reps` years each; the first tape year (recording + upload + run) separately; the tape's size.
    python tools/probe_tape.py [n] [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ooc_amd.engine import iage_engine, phosphorus_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 416
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3


def state(eng, kind):
    tc, nz, ny = eng.shape
    rng = np.random.default_rng(5)
    if kind == "iage":
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        return np.stack([np.broadcast_to(col[:, None], (nz, ny))] * tc) + 0.01 * rng.standard_normal(eng.shape)
    prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                 ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    return np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, ny)))


def year(eng, xp, sched):
    eng.sync()
    t0 = time.perf_counter()
    out, st = eng.comp_fcn_frozen(xp, sched)
    eng.sync()
    return time.perf_counter() - t0, eng.download(out), st


for kind in ("iage", "phosphorus"):
    eng = (iage_engine if kind == "iage" else phosphorus_engine)(Grid2d.default(n, n))
    x0 = state(eng, kind)
    x = eng.upload(x0)
    xp = eng.upload(x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, n))[None, :, None]))
    _, st_free, sched = eng.comp_fcn(x, record=True)
    print(f"{kind} {n}x{n}: free-running year {st_free['seconds']:.3f} s, {len(sched)} steps, {st_free['nnewton']} Newton iterations",
          flush=True)
    ways = [("launches", dict(stream_years=0, frozen_persistent=0, frozen_tape=0)),
            ("stream", dict(stream_years=3, frozen_persistent=0, frozen_tape=0)),
            ("tape", dict(stream_years=0, frozen_persistent=0, frozen_tape=1))]
    if kind == "iage":
        ways.append(("cache", dict(stream_years=0, frozen_persistent=1, frozen_tape=0, frozen_cache_after=0)))
    ref = None
    for name, opts in ways:
        for k, v in opts.items():
            eng.set_option(k, v)
        first, out, _ = year(eng, xp, sched)
        times = []
        for _ in range(reps):
            t, out2, st = year(eng, xp, sched)
            times.append(t)
            assert np.array_equal(out2, out)
        if ref is None:
            ref = out
        same = np.array_equal(out, ref)
        extra = ""
        if name == "tape":
            extra = (f", first year (recording + upload + run) {first:.3f} s, tape {eng.counter('tape_bytes') / 1e6:.2f} MB in "
                     f"{eng.counter('tape_commands')} commands, builds {eng.counter('tape_builds')}, years {eng.counter('tape_years_run')}, "
                     f"timeouts {eng.counter('tape_timeouts')}")
        if name == "cache":
            extra = f", first year {first:.3f} s, cache years {eng.counter('frozen_persistent_years')}"
        print(f"  {name:9s} best {min(times):.4f} s  median {sorted(times)[len(times) // 2]:.4f} s  nlaunch {st['nlaunch']}  "
              f"bit-identical to launches: {same}{extra}", flush=True)
    eng.close()
