"""the schedule cache of the one-launch frozen year as one slab against a list of pieces (option frozen_cache_pieces,
DESIGN.md section 3.6.1) at iage n x n.

    python tools/probe_cache_pieces.py steady [n] [lib ...]   slab and pieces alternating in one context, five years each: median and
                                                            min - max of the launch, and the time of the two build launches by cache
                                                            form; then the same slab years with every other library named (a
                                                            parent build: NK2D_LIB_PATH), each in a process of its own
    python tools/probe_cache_pieces.py solve [n]            what a solve gets: a fresh process per leg -- slab, pieces, pieces + early
                                                            at 256, 1024 and 4096 MiB --, each the work of one Newton iteration: the
                                                            recorded free-running year, the preconditioner set-up, five products
(the legs are child processes; this process never opens the device)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YEARS = 5


def _engine(n):
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    eng = iage_engine(Grid2d.default(n, n))
    col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
    x = eng.upload(np.stack([np.broadcast_to(col[:, None], (n, n))] * 2).copy())
    return eng, x


def _timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return time.perf_counter() - t0, out


def _fmt(xs, scale=1e3, unit="ms"):
    xs = np.asarray(xs) * scale
    return f"{np.median(xs):.2f} {unit} ({xs.min():.2f} - {xs.max():.2f})"


def leg_steady(n, forms):
    """one context; for each form in turn: the first year (build included), then YEARS years; the launch time from the counter"""
    eng, x = _engine(n)
    eng.set_option("frozen_alloc_async", 0)
    fx, _, sched = eng.comp_fcn(x, record=True)
    launch = {f: [] for f in forms}
    build = {f: [] for f in forms}
    for rep in range(2):
        for form in forms:
            eng.set_option("frozen_cache_pieces", 1 if form == "pieces" else 0)
            t_first, _ = _timed(eng, lambda: eng.comp_fcn_frozen(x, sched))      # (allocation + two build launches + the year)
            for k in range(YEARS):
                us = eng.counter("frozen_launch_us")
                t, _ = _timed(eng, lambda: eng.comp_fcn_frozen(x, sched))
                launch[form].append(1e-6 * (eng.counter("frozen_launch_us") - us))
                if k == 0:
                    build[form].append(t_first - t)
    lib = os.environ.get("NK2D_LIB_PATH", "this build")
    for form in forms:
        print(f"steady {n} x {n} [{lib}] {form}: launch {_fmt(launch[form])} over {len(launch[form])} years; first year minus a later "
              f"one (allocation + build) {_fmt(build[form])}; one-launch years {eng.counter('frozen_persistent_years')}", flush=True)
    eng.close()


def leg_solve(n, form, piece_mb):
    eng, x = _engine(n)
    if form != "slab":
        eng.set_option("frozen_cache_pieces", 1)
        eng.set_option("frozen_cache_piece_mb", piece_mb)
    if form == "early":
        eng.set_option("frozen_cache_early", 1)
    eng.set_region(np.ones((n, n), dtype=np.int32), np.outer(eng.grid.depth.delta, eng.grid.ypos.delta))
    t_all = time.perf_counter()
    t_year, (fx, _, sched) = _timed(eng, lambda: eng.comp_fcn(x, record=True))
    t_setup, _ = _timed(eng, eng.precond_setup)
    v = eng.precond_apply(fx)
    prods, one = [], 0
    for k in range(5):
        years = eng.counter("frozen_persistent_years")
        t, _ = _timed(eng, lambda: eng.jvp(x, fx, v, sched=sched))
        prods.append(t)
        one += eng.counter("frozen_persistent_years") - years
    total = time.perf_counter() - t_all
    print(f"solve {n} x {n} {form} piece_mb {piece_mb:g}: year {t_year:.3f} s, set-up {t_setup:.3f} s, products "
          + " ".join(f"{t:.3f}" for t in prods) + f" s, {one} of 5 in one launch, total {total:.3f} s; pieces "
          f"{eng.counter('frozen_cache_pieces')}, early requests {eng.counter('frozen_cache_early_requests')}", flush=True)
    eng.close()


def _child(args, env=None, limit=600):
    e = dict(os.environ)
    e.update(env or {})
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=e, timeout=limit)
    if res.returncode != 0:
        sys.exit(f"leg {args} ended with status {res.returncode}: nothing more is started")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "solve"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 416
    if mode == "steady":
        _child(["_steady", n, "slab,pieces"])
        for lib in sys.argv[3:]:
            _child(["_steady", n, "slab"], {"NK2D_LIB_PATH": lib})
    elif mode == "solve":
        for form, mb in (("slab", 1024), ("pieces", 1024), ("early", 256), ("early", 1024), ("early", 4096)):
            _child(["_solve", n, form, mb])
    elif mode == "_steady":
        leg_steady(n, sys.argv[3].split(","))
    elif mode == "_solve":
        leg_solve(n, sys.argv[3], float(sys.argv[4]))
