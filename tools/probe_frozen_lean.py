"""the one-launch frozen year on a lean schedule cache (option "frozen_cache_lean") against the other ways
to run the same frozen year of iage, one engine per size, the options alternating in one process:

    full       the full schedule cache (planes + factor tables), one launch
    lean       the lean cache (planes only), one launch that factorises in the first phase of every step
    lean+pcs   the lean cache in pieces
    launches   frozen_persistent 0: a launch per phase
    tape       frozen_tape 1: the command tape

Per size: five repetitions of every way in turn (the cache changes form between them: a year that allocates and builds
comes first and is reported on its own), median and min - max of the year's wall time; the cache's build time (the year that
rebuilds the tables in a slab that is there, minus the median year) and the wall time of its allocation (the year that
allocates and builds, minus the year that only builds); which way every setting actually took, from the counters; every
result checked bit for bit against the launches.  Then the same at 512 x 512 under the default "frozen_cache_gb", where the
full cache is expected not to fit, with "frozen_cache_lean" 0, 1 and 2.

    python tools/probe_frozen_lean.py [n ...]          (default: 208 416 512)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ooc_amd.engine import iage_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

REPS = 5
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "tape_years_run", "frozen_cache_builds")


def year(eng, xp, sched):
    eng.sync()
    t0 = time.perf_counter()
    out, st = eng.comp_fcn_frozen(xp, sched)
    eng.sync()
    return time.perf_counter() - t0, eng.download(out), st


def fmt(ts):
    ts = 1.0e3 * np.asarray(ts)
    return f"median {np.median(ts):8.2f} ms  (min {ts.min():8.2f} - max {ts.max():8.2f})"


def probe(n, ways):
    eng = iage_engine(Grid2d.default(n, n))
    eng.set_option("frozen_alloc_async", 0)
    rng = np.random.default_rng(5)
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    x0 = np.stack([np.broadcast_to(col[:, None], (n, n))] * 2) + 0.01 * rng.standard_normal(eng.shape)
    x = eng.upload(x0)
    xp = eng.upload(x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, n))[None, :, None]))
    _, st_free, sched = eng.comp_fcn(x, record=True)
    print(f"iage {n} x {n}: free-running year {st_free['seconds']:.3f} s, {len(sched)} steps, {st_free['nnewton']} Newton iterations, "
          f"frozen_cache_gb at its default", flush=True)
    times = {name: [] for name, _ in ways}
    first, rebuild, took, outs = {}, {}, {}, {}
    for rep in range(REPS):
        for name, opts in ways:
            for k, v in dict(stream_years=0, frozen_tape=0, frozen_persistent=1, frozen_cache_after=0, frozen_cache_lean=0,
                             frozen_cache_pieces=0, **opts).items():
                eng.set_option(k, v)
            before = {k: eng.counter(k) for k in COUNTERS}
            t_first, out, _ = year(eng, xp, sched)                 # (allocates and builds where the cache changed form)
            if eng.counter("frozen_cache_builds") > before["frozen_cache_builds"]:
                first.setdefault(name, []).append(t_first)
                # the tables again in the slab that is there: another estimate stride is another cache key, and back
                eng.set_option("frozen_err_check", 129)
                year(eng, xp, sched)
                eng.set_option("frozen_err_check", 128)
                t_build, out, _ = year(eng, xp, sched)
                rebuild.setdefault(name, []).append(t_build)
            before = {k: eng.counter(k) for k in COUNTERS}
            t, out2, st = year(eng, xp, sched)
            times[name].append(t)
            assert np.array_equal(out2, out)
            outs[name] = out2
            took[name] = ({k: eng.counter(k) - before[k] for k in COUNTERS}, eng.counter("frozen_cache_lean"),
                          eng.counter("frozen_cache_pieces"), eng.counter("frozen_cache_bytes"), st["nlaunch"])
    ref = outs["launches"]
    for name, _ in ways:
        d, lean, pieces, nbytes, nlaunch = took[name]
        if d["frozen_lean_years"]:
            path = "one launch, lean cache" + (f" in {pieces} pieces" if pieces else "")
        elif d["frozen_persistent_years"]:
            path = "one launch, full cache" + (f" in {pieces} pieces" if pieces else "")
        elif d["tape_years_run"]:
            path = "command tape"
        else:
            path = "a launch per phase"
        line = f"  {name:9s} {fmt(times[name])}  took: {path}, {nlaunch} launches"
        if d["frozen_persistent_years"]:
            line += f", cache {nbytes / 1e9:.2f} GB"
        line += f"; bit-identical to launches: {np.array_equal(outs[name], ref)}"
        print(line, flush=True)
        if name in first:
            med = float(np.median(times[name]))
            build = np.asarray(rebuild[name]) - med
            alloc = np.asarray(first[name]) - np.asarray(rebuild[name])
            print(f"            cache build ({'k_cache_planes alone' if d['frozen_lean_years'] else 'k_cache_planes + k_cache_factor'}): {fmt(build)}"
                  f";  allocation (wall): {fmt(alloc)}", flush=True)
    med = {name: float(np.median(times[name])) for name, _ in ways}
    if "lean" in med and "full" in med and took["full"][0]["frozen_persistent_years"] and took["lean"][0]["frozen_lean_years"]:
        print(f"  lean / full (medians): {med['lean'] / med['full']:.3f};  lean median {1e3 * med['lean']:.2f} ms against the launches' "
              f"minimum {1e3 * min(times['launches']):.2f} ms", flush=True)
    eng.close()


WAYS = [("full", {}), ("lean", dict(frozen_cache_lean=1)), ("lean+pcs", dict(frozen_cache_lean=1, frozen_cache_pieces=1)),
        ("launches", dict(frozen_persistent=0)), ("tape", dict(frozen_persistent=0, frozen_tape=1))]
WAYS_512 = [("lean=0", {}), ("lean=1", dict(frozen_cache_lean=1)), ("lean=2", dict(frozen_cache_lean=2)),
            ("lean+pcs", dict(frozen_cache_lean=1, frozen_cache_pieces=1)),
            ("launches", dict(frozen_persistent=0)), ("tape", dict(frozen_persistent=0, frozen_tape=1))]

if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [208, 416, 512]
    for n in sizes:
        probe(n, WAYS_512 if n >= 512 else WAYS)
