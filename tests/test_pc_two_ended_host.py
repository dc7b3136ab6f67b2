"""Option "pc_two_ended" (the preconditioner's block elimination from both ends of the ypos axis) adds an option and two
counters, no entry point; the header, the README and the engine's environment knob name it."""
import os

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pc_two_ended_is_an_option_with_counters_and_documented():
    assert len(_lib.SIGNATURES) == 56
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    for name in ('"pc_two_ended"', '"pc_setup_rounds"', '"pc_sub_launches"'):
        assert name in header, name
    assert "NK2D_PC_TWO_ENDED" in open(os.path.join(ROOT, "README.md")).read()
    assert "NK2D_PC_TWO_ENDED" in open(os.path.join(os.path.dirname(_lib.__file__), "engine.py")).read()
    # the names are the library's, not only the header's: they are in its read-only data
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"pc_two_ended", b"pc_setup_rounds", b"pc_sub_launches", b"k_pc_gemv2_ends", b"k_pc_schur_ends"):
        assert name in blob, name
