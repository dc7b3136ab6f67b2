"""the one-launch frozen year of the file-driven forced module (option "frozen_forced") against the other
ways to run the same frozen year, one engine per case, the ways alternating in one process:

  file-driven forced n x n WITHOUT a sink threshold (bit 1: five to eight levels per lane)
    full       the full schedule cache, one launch
    lean       the lean cache, one launch that factorises in the first phase of every step
    launches   frozen_persistent 0: a launch per phase
    tape       frozen_tape 1: the command tape
  file-driven forced n x n WITH a sink threshold (bit 2: the year forms UPR of each wave's own column; lean cache only)
    lean       the lean cache with the rows' source planes, one launch
    launches   frozen_persistent 0: a launch per phase
    stream     stream_years 3: the host-fed command stream
    tape       frozen_tape 1: the command tape

Per case: five repetitions of every way in turn (a year that allocates and builds a cache comes first and is not timed),
median and min - max of the year's wall time; which path every setting actually took, from the counters; every result checked
bit for bit against the launches; each one-launch / launch-per-phase ratio of medians from the same run.

    python tools/probe_frozen_forced.py [n ...]          (default: 416)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ooc_amd.engine import ModuleEngine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

REPS = 5
DAY = 86400.0
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_forced_years", "tape_years_run", "stream_years_run",
            "frozen_cache_builds")
BASE = dict(stream_years=0, frozen_tape=0, frozen_persistent=1, frozen_cache_after=0, frozen_cache_lean=0, frozen_cache_pieces=0,
            frozen_forced=3)


def year(eng, xp, sched):
    eng.sync()
    t0 = time.perf_counter()
    out, st = eng.comp_fcn_frozen(xp, sched)
    eng.sync()
    return time.perf_counter() - t0, eng.download(out), st


def fmt(ts):
    ts = 1.0e3 * np.asarray(ts)
    return f"median {np.median(ts):8.2f} ms  (min {ts.min():8.2f} - max {ts.max():8.2f})"


def probe(n, thres, ways):
    rng = np.random.default_rng(11)
    times_rec = np.array([-10.0, 95.0, 200.0, 300.0, 380.0]) * DAY
    eng = ModuleEngine(Grid2d.default(n, n), tc=1, surf_rate=(24.0 / DAY,), module_kind=2,
                       restore_series=(times_rec, 1.0 + 0.2 * rng.standard_normal((5, n))),
                       sms_series=(times_rec, 3.0e-9 * rng.standard_normal((5, n, n))), sink_thres=0.6 if thres else None)
    eng.set_option("frozen_alloc_async", 0)
    zz = np.linspace(0.0, 1.0, n)[:, None]
    x0 = (0.6 + 0.2 * np.cos(3.0 * np.pi * zz) * np.ones((1, n)) + 0.01 * rng.standard_normal((n, n)))[None]
    x = eng.upload(x0)
    xp = eng.upload(x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, n))[None, :, None]))
    _, st_free, sched = eng.comp_fcn(x, record=True)
    print(f"file-driven forced {n} x {n}, {'sink threshold 0.6' if thres else 'no sink threshold'}: free-running year "
          f"{st_free['seconds']:.3f} s, {len(sched)} steps, {st_free['nnewton']} Newton iterations", flush=True)
    times = {name: [] for name, _ in ways}
    took, outs = {}, {}
    for rep in range(REPS):
        for name, opts in ways:
            for k, v in dict(BASE, **opts).items():
                eng.set_option(k, v)
            year(eng, xp, sched)                                   # (allocates and builds where the cache changed form; records a tape)
            before = {k: eng.counter(k) for k in COUNTERS}
            t, out, st = year(eng, xp, sched)
            times[name].append(t)
            outs[name] = out
            took[name] = ({k: eng.counter(k) - before[k] for k in COUNTERS}, eng.counter("frozen_cache_bytes"), st["nlaunch"])
    ref = outs["launches"]
    med = {name: float(np.median(times[name])) for name, _ in ways}
    for name, _ in ways:
        d, nbytes, nlaunch = took[name]
        if d["frozen_persistent_years"]:
            path = f"one launch, {'lean' if d['frozen_lean_years'] else 'full'} cache of {nbytes / 1e9:.2f} GB" + \
                   (", by option frozen_forced" if d["frozen_forced_years"] else "")
        elif d["tape_years_run"]:
            path = "command tape"
        elif d["stream_years_run"]:
            path = "host-fed command stream"
        else:
            path = "a launch per phase"
        line = f"  {name:9s} {fmt(times[name])}  took: {path}, {nlaunch} launches; bit-identical to launches: {np.array_equal(outs[name], ref)}"
        if d["frozen_persistent_years"]:
            line += f"; one launch / launch per phase (medians): {med[name] / med['launches']:.3f}"
        print(line, flush=True)
    eng.close()


WAYS_LINEAR = [("full", {}), ("lean", dict(frozen_cache_lean=1)), ("launches", dict(frozen_persistent=0)),
               ("tape", dict(frozen_persistent=0, frozen_tape=1))]
WAYS_THRES = [("lean", dict(frozen_cache_lean=1)), ("launches", dict(frozen_persistent=0)),
              ("stream", dict(frozen_persistent=0, stream_years=3)), ("tape", dict(frozen_persistent=0, frozen_tape=1))]

if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or [416]:
        probe(n, False, WAYS_LINEAR)
        probe(n, True, WAYS_THRES)
