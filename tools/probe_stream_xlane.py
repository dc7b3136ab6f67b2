"""command-stream year: the resident kernel's cross-lane moves at distances 1 and 32 and its wave sums in the VALU (option
"stream_xlane" 1) against 0.  One process, one engine per case; the arms alternate, five free-running years each (a library without
the option: twice five of its one arm); per arm the median and the min - max of the year's wall time, the kernel's own clocks per
command (counters "stream_prof_*": microseconds a workgroup spends executing commands, and executing Newton commands, over their
counts), counter "stream_xlane_bits", and whether the arm's year is the first arm's bit for bit.  With --parent LIB the same cases
run first on that library (a build of the parent commit) in a process of its own, through NK2D_LIB_PATH: the parent's arm of the
comparison, and its checksum of the year to compare with this library's.

usage: probe_stream_xlane.py [--parent LIB] [case ...]      (default iage_26 iage_52 iage_104 iage_208 iage_416 phosphorus_416)"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = (0, 1)
ROUNDS = 5
CASES = ["iage_26", "iage_52", "iage_104", "iage_208", "iage_416", "phosphorus_416"]


def _set(eng, bits):
    try:
        eng.set_option("stream_xlane", bits)
        return True
    except Exception:       # (a library from before the option)
        return False


def _engine(case):
    from nk_ooc_amd.engine import iage_engine, phosphorus_engine
    from nk_ooc_amd.grid import Grid2d

    kind, n = case.split("_")[0], int(case.split("_")[1])
    if kind == "phosphorus":
        eng = phosphorus_engine(Grid2d.default(n, n))
        prof = [np.interp(eng.grid.depth.mid, zs, vs) for zs, vs in (([1.3e2, 2.6e2], [5.5e-3, 4.1e0]), ([9.5e1, 1.4e2], [7.1e-2, 1.5e-4]),
                                                                     ([1.7e2, 2.5e2], [1.8e-2, 7.9e-4]))]
        x0 = np.stack([np.broadcast_to(p[:, None], (n, n)) for p in prof]).copy()
    else:
        eng = iage_engine(Grid2d.default(n, n))
        col = np.interp(eng.grid.depth.mid, [55.0, 200.0], [0.0, 2.0])
        x0 = np.stack([np.broadcast_to(col[:, None], (n, n))] * eng.shape[0]).copy()
    eng.set_option("stream_years", 1)
    return eng, x0


def _prof(eng):
    return np.array([eng.counter(f"stream_prof_{i}") for i in range(12)], dtype=np.float64)


def main(cases):
    from nk_ooc_amd import _lib

    print(f"library {os.path.relpath(_lib.LIB_PATH, ROOT)}", flush=True)
    for case in cases:
        eng, x0 = _engine(case)
        x = eng.upload(x0)
        known = _set(eng, 0)
        arms = ARMS if known else (0,)
        ref, same, in_effect, st = None, {}, {}, None
        for bits in arms:       # (every arm's code is loaded and its occupancy asked for before anything is timed)
            _set(eng, bits)
            fx, st, _ = eng.comp_fcn(x)
            got = eng.download(fx)
            ref = got if ref is None else ref
            same[bits] = bool(np.array_equal(got, ref))
            in_effect[bits] = eng.counter("stream_xlane_bits") if known else -1
        wall = {b: [] for b in arms}
        clocks = {b: np.zeros(12) for b in arms}
        for _ in range(ROUNDS * (1 if known else len(ARMS))):
            for bits in arms:
                _set(eng, bits)
                p0 = _prof(eng)
                stats = eng.comp_fcn(x)[1]
                clocks[bits] += _prof(eng) - p0
                wall[bits].append(1.0e3 * stats["seconds"])
        base = float(np.median(wall[arms[0]]))
        spread = max(wall[arms[0]]) - min(wall[arms[0]])
        print(f"{case}: {st['nsteps']} steps, {st['nnewton']} Newton iterations, stream years {eng.counter('stream_years_run')}, timeouts "
              f"{eng.counter('stream_timeouts')}, columns per workgroup {eng.counter('stream_columns_per_workgroup')}, two waves "
              f"{eng.counter('stream_two_waves_kernel')}; spread of the {arms[0]} arm {spread:.3f} ms = {100.0 * spread / base:.2f} % (min - max over "
              f"the median); checksum of the year {float(np.sum(ref)):.17g}, sha1 {hashlib.sha1(ref.tobytes()).hexdigest()[:16]}", flush=True)
        for bits in arms:
            med, c = float(np.median(wall[bits])), clocks[bits]
            print(f"  stream_xlane {bits} (in effect {in_effect[bits]:2d}): year median {med:9.3f} ms  [{min(wall[bits]):9.3f} - {max(wall[bits]):9.3f}]  "
                  f"{100.0 * (base - med) / base:+.2f} % against {arms[0]}, {(base - med) / spread if spread > 0 else float('inf'):+.1f} spreads, "
                  f"median below the minimum of {arms[0]}: {med < min(wall[arms[0]])};  a command {c[1] / max(c[3], 1.0):7.3f} us, "
                  f"a Newton command {c[5] / max(c[9], 1.0):7.3f} us ({int(c[9] / len(wall[bits]))} a year);  same bits {same[bits]}", flush=True)
        eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--parent":
        # (before this process opens the device: the parent's library needs a process of its own)
        env = dict(os.environ, NK2D_LIB_PATH=os.path.abspath(args[1]))
        args = args[2:]
        subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, check=True)
    main(args or CASES)
