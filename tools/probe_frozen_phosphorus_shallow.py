"""the one-launch frozen year of the phosphorus module at one and two levels per lane (option "frozen_phosphorus_shallow", DESIGN.md
section 3.6.4) against the other ways to run the same frozen year.  One process per size (a child process each, started afresh),
the ways alternating inside it:

    launches   frozen_persistent 0: a launch per phase
    stream     stream_years 3: the host-fed command stream
    tape       frozen_tape 1: the command tape
    one        frozen_phosphorus 1 + frozen_phosphorus_shallow 1 on the lean cache: one launch, a workgroup per ypos column

Per size: REPS repetitions of every way in turn (a year that allocates and builds a cache or records a tape comes first and is not
timed), median and min - max of the year's wall time (host clock around a year that ends in a synchronise); which path every
setting actually took, from the counters; every result checked bit for bit against the launches; one launch / stream and one
launch / launches as ratios of medians of the same run.  For the one-launch year also the device time of the launch (HIP events
around it, counter "frozen_launch_us") and that time per phase -- a phase is one Newton iteration's sweep of every column, between
two hand-overs: sum of n_iter x m over the rows (stats "nsweeps"), the few estimate phases left out of the count.

No threshold was set before the measurement and none is applied: the option stays opt-in whatever comes out.

    python tools/probe_frozen_phosphorus_shallow.py [n | nzxny ...]     (default: 26 52 104 40x50 80x100 125x150)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_phosphorus_years", "frozen_phosphorus_shallow_years",
            "frozen_team_years", "frozen_two_waves_years", "tape_years_run", "stream_years_run", "frozen_cache_builds", "frozen_launch_us")
BASE = dict(stream_years=0, frozen_tape=0, frozen_persistent=1, frozen_cache_after=0, frozen_cache_lean=1, frozen_cache_pieces=0,
            frozen_phosphorus=0, frozen_phosphorus_shallow=0)
WAYS = [("launches", dict(frozen_persistent=0)), ("stream", dict(frozen_persistent=0, stream_years=3)),
        ("tape", dict(frozen_persistent=0, frozen_tape=1)), ("one", dict(frozen_phosphorus=1, frozen_phosphorus_shallow=1))]
SIZES = ["26", "52", "104", "40x50", "80x100", "125x150"]


def state(eng, rng):
    tc, nz, ny = eng.shape
    prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                 ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    return np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, ny)))


def year(eng, xp, sched):
    eng.sync()
    t0 = time.perf_counter()
    out, st = eng.comp_fcn_frozen(xp, sched)
    eng.sync()
    return time.perf_counter() - t0, eng.download(out), st


def fmt(ts):
    ts = 1.0e3 * np.asarray(ts)
    return f"median {np.median(ts):8.2f} ms  (min {ts.min():8.2f} - max {ts.max():8.2f})"


def probe(nz, ny):
    from nk_ooc_amd.engine import phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    rng = np.random.default_rng(12)
    eng = phosphorus_engine(Grid2d.default(nz, ny))
    eng.set_option("frozen_alloc_async", 0)
    x0 = state(eng, rng)
    x = eng.upload(x0)
    xp = eng.upload(x0 * (1.0 + 1.0e-5 * np.cos(np.linspace(0.0, 3.0, nz))[None, :, None]))
    _, st_free, sched = eng.comp_fcn(x, record=True)
    print(f"phosphorus {nz} x {ny} ({(nz + 63) // 64} levels per lane): free-running year {st_free['seconds']:.3f} s, {len(sched)} steps, "
          f"{st_free['nnewton']} Newton iterations", flush=True)
    times = {name: [] for name, _ in WAYS}
    took, outs, dev_us, phases = {}, {}, [], 0
    for rep in range(REPS):
        for name, opts in WAYS:
            for k, v in dict(BASE, **opts).items():
                eng.set_option(k, v)
            year(eng, xp, sched)                                   # (allocates and builds the cache; records a tape)
            before = {k: eng.counter(k) for k in COUNTERS}
            t, out, st = year(eng, xp, sched)
            times[name].append(t)
            outs[name] = out
            d = {k: eng.counter(k) - before[k] for k in COUNTERS}
            took[name] = (d, eng.counter("frozen_cache_bytes"), st["nlaunch"])
            if name == "one" and d["frozen_persistent_years"]:
                dev_us.append(d["frozen_launch_us"])
                phases = st["nsweeps"]
    ref = outs["launches"]
    med = {name: float(np.median(times[name])) for name, _ in WAYS}
    for name, _ in WAYS:
        d, nbytes, nlaunch = took[name]
        if d["frozen_persistent_years"]:
            path = (f"one launch ({d['frozen_phosphorus_shallow_years']} shallow, {d['frozen_team_years']} team, {d['frozen_two_waves_years']} "
                    f"two-waves years), lean cache of {nbytes / 1e6:.1f} MB")
        elif d["tape_years_run"]:
            path = "command tape"
        elif d["stream_years_run"]:
            path = "host-fed command stream"
        else:
            path = "a launch per phase"
        line = f"  {name:9s} {fmt(times[name])}  took: {path}, {nlaunch} launches; bit-identical to launches: {np.array_equal(outs[name], ref)}"
        if d["frozen_persistent_years"]:
            line += f"; one launch / stream {med[name] / med['stream']:.3f}, / launches {med[name] / med['launches']:.3f} (medians)"
        print(line, flush=True)
    if dev_us:
        dev = np.asarray(dev_us, dtype=float)
        print(f"  one       device time of the launch: median {np.median(dev) / 1e3:8.2f} ms  (min {dev.min() / 1e3:8.2f} - max {dev.max() / 1e3:8.2f}); "
              f"{phases} phases: {np.median(dev) / phases:.2f} us per phase", flush=True)
    else:
        print("  one       did not take the one-launch year at this size", flush=True)
    eng.close()


def size_of(a):
    return tuple(int(v) for v in a.split("x")) if "x" in a else (int(a), int(a))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        probe(*size_of(sys.argv[2]))
    else:
        for a in sys.argv[1:] or SIZES:
            # a process of its own per size: nothing of one size's caches, allocations or clocks in the next one's figures
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", a]).returncode
            if rc != 0:
                sys.exit(f"size {a}: exit status {rc}; stopping")
