"""the year that produces F(x) in a Newton iteration -- a free-running year with the 61 samples of a history file -- at
416 x 416, as a command stream (stream_years 1), three ways (option "stream_hist"): samples by
launches (0: the kernel ends and starts again around every sampled step), samples as commands of the resident kernel (1),
and the same with a sample buffer of a single slot (stream_hist_mb 0: a drain per sample).  Against the plain year of the
same engine and state.  Median and min .. max of `reps` years each, kernel starts, samples by command, drains; every
way is checked bit for bit against the first.
    python tools/probe_stream_hist.py [n] [reps] [plain]
`plain`: the plain year only (what a build without the option can run: NK2D_LIB_PATH names its library)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ooc_amd.engine import iage_engine, phosphorus_engine  # noqa: E402
from nk_ooc_amd.grid import Grid2d  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 416
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
plain_only = len(sys.argv) > 3 and sys.argv[3] == "plain"
t_eval = np.linspace(0.0, 365.0 * 86400.0, 61)


def state(eng, kind):
    tc, nz, ny = eng.shape
    rng = np.random.default_rng(5)
    if kind == "iage":
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        return np.stack([np.broadcast_to(col[:, None], (nz, ny))] * tc) + 0.01 * rng.standard_normal(eng.shape)
    prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                 ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
    return np.stack([np.broadcast_to(p[:, None], (nz, ny)) for p in prof]) * (1.0 + 0.05 * rng.random((3, nz, ny)))


def timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    res = fn()
    eng.sync()
    return time.perf_counter() - t0, res


def row(name, times, extra):
    times = sorted(times)
    print(f"  {name:22s} median {times[len(times) // 2]:.4f} s  min {times[0]:.4f}  max {times[-1]:.4f}  "
          f"(spread {times[-1] - times[0]:.4f}){extra}", flush=True)
    return times[len(times) // 2]


for kind in ("iage", "phosphorus"):
    eng = (iage_engine if kind == "iage" else phosphorus_engine)(Grid2d.default(n, n))
    eng.set_option("stream_years", 1)
    x = eng.upload(state(eng, kind))
    _, (fx, st, _) = timed(eng, lambda: eng.comp_fcn(x))        # (warm-up: the resident kernel's buffers, its shape)
    want = eng.download(fx)
    print(f"{kind} {n}x{n}: {st['nsteps']} steps, {st['nnewton']} Newton iterations, {reps} years each", flush=True)
    times, l0 = [], eng.counter("stream_launches")
    for _ in range(reps):
        t, (fx, st, _) = timed(eng, lambda: eng.comp_fcn(x))
        times.append(t)
        assert np.array_equal(eng.download(fx), want)
    plain = row("plain year", times, f"  kernel starts {(eng.counter('stream_launches') - l0) // reps}")
    if plain_only:
        eng.close()
        continue
    ref, med = None, {}
    for name, opts, k in (("samples by launches", dict(stream_hist=0), reps), ("samples as commands", dict(stream_hist=1, stream_hist_mb=256), reps),
                          ("... one slot", dict(stream_hist=1, stream_hist_mb=0), 1)):
        for key, v in opts.items():
            eng.set_option(key, v)
        _, (fx, st, hist) = timed(eng, lambda: eng.comp_fcn_hist(x, t_eval))      # (warm-up: staging and sample buffers)
        if ref is None:
            ref = hist
        same = np.array_equal(hist, ref) and np.array_equal(eng.download(fx), want)
        times = []
        c0 = [eng.counter(c) for c in ("stream_launches", "stream_hist_samples", "stream_hist_drains")]
        for _ in range(k):
            t, (fx, st, hist) = timed(eng, lambda: eng.comp_fcn_hist(x, t_eval))
            times.append(t)
            same = same and np.array_equal(hist, ref)
        c1 = [eng.counter(c) for c in ("stream_launches", "stream_hist_samples", "stream_hist_drains")]
        per = [(b - a) // k for a, b in zip(c0, c1)]
        med[name] = row(name, times, f"  kernel starts {per[0]}  samples by command {per[1]}  drains {per[2]}  same bits: {same}")
    off, on = med["samples by launches"], med["samples as commands"]
    print(f"  sampled year: {off:.4f} s -> {on:.4f} s ({1e3 * (off - on):+.1f} ms saved); over the plain year {1e3 * (off - plain):.1f} ms -> "
          f"{1e3 * (on - plain):.1f} ms", flush=True)
    eng.close()
