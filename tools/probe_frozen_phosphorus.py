"""the one-launch frozen year of the phosphorus module (option "frozen_phosphorus") against the other ways
to run the same frozen year, one engine per size (208 x 208, 256 x 256, 416 x 416), the ways alternating in one process:

    launches   frozen_persistent 0: a launch per phase
    stream     stream_years 3: the host-fed command stream (with its two-waves flavour where option "stream_two_waves" 1, the
               default, takes it: the log says which kernel ran)
    tape       frozen_tape 1: the command tape
    one_1      frozen_phosphorus 1 on the lean cache: one launch at one wave per SIMD, where all its workgroups are resident
    one_2      frozen_phosphorus 2: as 1, and the 256-register flavour where that one is not resident
    one_3      frozen_phosphorus 3: the 256-register flavour wherever it exists

Per size: five repetitions of every way in turn (a year that allocates and builds a cache or records a tape comes first and is
not timed), median and min - max of the year's wall time; which path every setting actually took, from the counters; every
result checked bit for bit against the launches; each one-launch / stream ratio of medians from the same run.

The rule, fixed before the measurement: value 2 is worth recommending at a size only if its median lies below the host-fed
stream year's MINIMUM of the same run.  The default stays 0 whatever comes out.

    python tools/probe_frozen_phosphorus.py [n | nzxny ...]          (default: 208 256x256 416)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ooc_amd.engine import phosphorus_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

REPS = 5
COUNTERS = ("frozen_persistent_years", "frozen_lean_years", "frozen_phosphorus_years", "frozen_two_waves_years", "tape_years_run",
            "stream_years_run", "frozen_cache_builds")
BASE = dict(stream_years=0, frozen_tape=0, frozen_persistent=1, frozen_cache_after=0, frozen_cache_lean=1, frozen_cache_pieces=0,
            frozen_phosphorus=0)
WAYS = [("launches", dict(frozen_persistent=0)), ("stream", dict(frozen_persistent=0, stream_years=3)),
        ("tape", dict(frozen_persistent=0, frozen_tape=1)), ("one_1", dict(frozen_phosphorus=1)), ("one_2", dict(frozen_phosphorus=2)),
        ("one_3", dict(frozen_phosphorus=3))]


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
    took, outs = {}, {}
    for rep in range(REPS):
        for name, opts in WAYS:
            for k, v in dict(BASE, **opts).items():
                eng.set_option(k, v)
            year(eng, xp, sched)                                   # (allocates and builds the cache; records a tape)
            before = {k: eng.counter(k) for k in COUNTERS}
            t, out, st = year(eng, xp, sched)
            times[name].append(t)
            outs[name] = out
            took[name] = ({k: eng.counter(k) - before[k] for k in COUNTERS}, eng.counter("frozen_cache_bytes"), st["nlaunch"],
                          eng.counter("stream_two_waves_kernel"))
    ref = outs["launches"]
    med = {name: float(np.median(times[name])) for name, _ in WAYS}
    stream_min = float(np.min(times["stream"]))
    for name, _ in WAYS:
        d, nbytes, nlaunch, stream_w2 = took[name]
        if d["frozen_persistent_years"]:
            path = f"one launch, {'the 256-register flavour' if d['frozen_two_waves_years'] else 'one wave per SIMD'}, lean cache of {nbytes / 1e9:.2f} GB"
        elif d["tape_years_run"]:
            path = "command tape"
        elif d["stream_years_run"]:
            path = "host-fed command stream" + (", two waves to a SIMD" if stream_w2 else ", one wave per SIMD")
        else:
            path = "a launch per phase"
        line = f"  {name:9s} {fmt(times[name])}  took: {path}, {nlaunch} launches; bit-identical to launches: {np.array_equal(outs[name], ref)}"
        if d["frozen_persistent_years"]:
            line += f"; one launch / stream (medians): {med[name] / med['stream']:.3f}"
        print(line, flush=True)
    d2 = took["one_2"][0]
    if d2["frozen_persistent_years"]:
        verdict = "worth recommending" if med["one_2"] < stream_min else "NOT worth recommending"
        print(f"  rule: value 2 median {1e3 * med['one_2']:.2f} ms against the stream year's minimum {1e3 * stream_min:.2f} ms: {verdict} at this size "
              f"(the default stays 0)", flush=True)
    else:
        print("  rule: value 2 did not take the one-launch year at this size: nothing to recommend", flush=True)
    eng.close()


if __name__ == "__main__":
    for a in sys.argv[1:] or ["208", "256x256", "416"]:
        nz, ny = (int(v) for v in a.split("x")) if "x" in a else (int(a), int(a))
        probe(nz, ny)
