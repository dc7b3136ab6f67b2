"""The VALU cross-lane moves behind option "frozen_xlane" (xl_up / xl_down / xl_wave_sum, csrc/nk2d_common.h) against
__shfl_up / __shfl_down, through the library's self-test entry: one wave, every helper at every distance 1, 2, 4, 8, 16, 32, on
the caller's 64 doubles.  The contract is bits, in all 64 lanes: the partner's value where the lane has one and the lane's own
value where it has none -- the tridiagonal solves multiply that slot by a zero, and another value there could turn the sign
of a zero or make a NaN.  So the inputs are the lane index (which lane a value came from), random normals, and a vector of
signed zeros, infinities, denormals and NaNs with distinct payloads, compared as 64-bit integers.  Of the sum over the wave
only lane 0 is the total; there it is wave_sum's additions in wave_sum's order, the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIST = (1, 2, 4, 8, 16, 32)
# rows of the self-test's output (include/nk2d.h): six distances each
ROWS = {"up": 0, "down": 6, "cplx up re": 12, "cplx up im": 18, "cplx down re": 24, "cplx down im": 30}
SUM_ROW = 36


def _specials():
    pool = [0x0000000000000000, 0x8000000000000000,         # +0.0, -0.0
            0x7FF0000000000000, 0xFFF0000000000000,         # +inf, -inf
            0x0000000000000001, 0x800FFFFFFFFFFFFF,         # the smallest and the largest denormal, one of each sign
            0x0000000100000000, 0x00000000FFFFFFFF]         # denormals that live in one 32-bit half only
    bits = []
    for i in range(64):
        if i % 3 == 2:      # NaNs, quiet and signalling, each with a payload of its own in both halves
            bits.append((0x7FF8000000000000 if i % 2 else 0xFFF0000000000000) | ((i + 1) << 32) | (0xABC00 + i))
        else:
            bits.append(pool[(i // 3 + i) % len(pool)])
    bits = np.array(bits, dtype=np.uint64)
    return bits.view(np.float64)


INPUTS = {
    "lane_index": lambda: np.arange(64, dtype=np.float64),
    "normals": lambda: np.random.default_rng(5).standard_normal(64),
    "specials": _specials,
}


@pytest.fixture(scope="module")
def eng():
    from nk_ooc_amd.engine import iage_engine
    from nk_ooc_amd.grid import Grid2d

    e = iage_engine(Grid2d.default(20, 3, 0.0, 0.0))
    yield e
    e.close()


def _shfl(v, s, up):
    lanes = np.arange(64)
    src = np.where(lanes >= s, lanes - s, lanes) if up else np.where(lanes + s < 64, lanes + s, lanes)
    return v[src]


@pytest.mark.parametrize("name", list(INPUTS))
def test_moves_are_shfl_bit_for_bit(eng, name):
    v = INPUTS[name]()
    out = eng.xlane_selftest(v).view(np.uint64)
    ref, got = out[0], out[1]
    vb, wb = v.view(np.uint64), v[::-1].copy().view(np.uint64)
    for what, row0 in ROWS.items():
        src = wb if what.endswith("im") else vb
        for lv, s in enumerate(DIST):
            bad = np.flatnonzero(ref[row0 + lv] != got[row0 + lv])
            print(f"{name}: {what} by {s}: lanes that differ from __shfl {bad.tolist()}")
            # (the __shfl column itself is the move it is meant to be: a NaN's payload travels through ds_bpermute untouched)
            assert np.array_equal(ref[row0 + lv], _shfl(src, s, "up" in what)), (what, s)
            assert bad.size == 0, (what, s, bad.tolist())
    print(f"{name}: sum over the wave, lane 0: __shfl {ref[SUM_ROW, 0]:#x}, VALU {got[SUM_ROW, 0]:#x}")
    assert ref[SUM_ROW, 0] == got[SUM_ROW, 0]       # (the same operands in the same additions: the same NaN too)
