#!/usr/bin/env python
"""phosphorus_fcn_70x12.npz: the reference's forward year from the state of phosphorus_70x12.npz, which holds tendencies and
Jacobians but no year.  gen_golden.gen_phosphorus(..., with_fcn=True) with the fixture's own seed, written to a scratch
directory; `y0` must be the fixture's `y` to the bit, and only the year goes into the new file:

    python tests/golden/gen_phosphorus_fcn.py          (where gen_golden.py runs; a solve_ivp year, about a minute)

tests/test_gpu_frozen_phosphorus_shallow.py holds the recorded year of that state to `fcn` (two levels per lane)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402


def main():
    gen_golden._install_placeholders()
    sys.path.insert(0, gen_golden.REF)
    have = np.load(os.path.join(HERE, "phosphorus_70x12.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        gen_golden.HERE = tmp
        gen_golden.gen_phosphorus("70x12", 70, 12, 10, with_fcn=True)
        new = np.load(os.path.join(tmp, "phosphorus_70x12.npz"))
        assert np.array_equal(new["y0"], have["y"]) and np.array_equal(new["tend"], have["tend"])
        np.savez_compressed(os.path.join(HERE, "phosphorus_fcn_70x12.npz"), nz=70, ny=12, y0=new["y0"], fcn=new["fcn"],
                            nfev=new["nfev"], njev=new["njev"], nlu=new["nlu"])
    print("wrote phosphorus_fcn_70x12.npz")


if __name__ == "__main__":
    main()
