"""Option "pc_pivot_wave" (the pivot blocks of the preconditioner's Gauss-Jordan inversions inverted by one wave in
registers) adds an option and a counter, no entry point; the header, the README and the engine's environment knob name it,
and the library holds the wave flavours of the three kernels that invert a pivot block."""
import os

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pc_pivot_wave_is_an_option_with_a_counter_and_documented():
    assert len(_lib.SIGNATURES) == 56
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    for name in ('"pc_pivot_wave"', '"pc_pivot_wave_steps"'):
        assert name in header, name
    assert "NK2D_PC_PIVOT_WAVE" in open(os.path.join(ROOT, "README.md")).read()
    assert "NK2D_PC_PIVOT_WAVE" in open(os.path.join(os.path.dirname(_lib.__file__), "engine.py")).read()
    # the names are the library's, not only the header's: they are in its read-only data; the kernels by their mangled
    # names, template argument 1
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"pc_pivot_wave", b"pc_pivot_wave_steps", b"k_pc_pivot_invertILi1EE", b"k_pc_gj_stepILi1EE",
                 b"k_pc_gj_rowsILi1EE"):
        assert name in blob, name
