"""The phosphorus preconditioner behind the C ABI adds no entry point (the ABI keeps its 56; the declaration is the one-vector
form of nk2d_precond_setup_states on a phosphorus context), a counter and an environment knob of the Python layer; with the
knob unset PhosphorusPrecond.apply makes the five calls it made."""
import os
import re

import numpy as np

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_declaration_is_documented_and_bound_to_an_existing_entry_point():
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", header[header.index('extern "C"'):]))
    assert "nk2d_precond_setup_states" in declared
    assert declared == set(_lib.SIGNATURES) and len(declared) == 56
    # the header says at that entry point what it does on a phosphorus context
    doc = header[header.index("/* the same for a forced module"):header.index("int nk2d_precond_setup_states")]
    for text in ("module_kind 1", "states[0] = e_hat", "nk2d_shift_factor", "shift / 2", "removes the declaration"):
        assert text in doc, text
    engine_src = open(os.path.join(os.path.dirname(_lib.__file__), "engine.py")).read()
    assert "def precond_set_nullspace(self, e_hat)" in engine_src and "NK2D_PHOS_PC_FUSED" in engine_src
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (header, readme):
        for name in ("NK2D_PHOS_PC_FUSED", "pc_phos_applies", "nk2d_precond_setup_states"):
            assert name in text, name
    # the header says where the eigen-pair stays and how a binding gets it
    assert "OPinv" in header and "eigs" in header
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"nk2d_precond_setup_states", b"pc_phos_applies", b"k_pc_phos_combine", b"k_pc_phos_finish"):
        assert name in blob, name


class RecordingEngine:
    """stands in for ModuleEngine: records the calls a PhosphorusPrecond makes, computes nothing"""

    shape = (3, 4, 2)
    nz, ny = 4, 2

    def __init__(self):
        from nk_ooc_amd.engine import phos_pc_fused_from_env

        self.phos_pc_fused = phos_pc_fused_from_env()      # read at creation, as ModuleEngine does
        self.calls = []

    def _note(self, name, *args):
        self.calls.append((name,) + args)
        return f"vec{len(self.calls)}"

    def set_lin_state(self, y):
        self._note("set_lin_state")

    def upload(self, host, out=None):
        return self._note("upload")

    def shift_factor(self, t, scale, shifts):
        self._note("shift_factor", tuple(shifts))

    def scale(self, x, s, out=None):
        return self._note("scale")

    def dot(self, a, b):
        self._note("dot", a, b)
        return np.array([0.25])

    def shift_solve(self, i, v, out=None):
        return self._note("shift_solve", i, v)

    def axpby(self, a, x, b, y, out=None):
        self._note("axpby", float(np.asarray(a).reshape(-1)[0]), x, float(np.asarray(b).reshape(-1)[0]), y, out)
        return out if out is not None else f"vec{len(self.calls)}"

    def precond_set_nullspace(self, e_hat):
        self._note("precond_set_nullspace", e_hat)

    def precond_apply(self, v, out=None):
        return self._note("precond_apply", v)


def _precond(monkeypatch, eng):
    from nk_ooc_amd.phosphorus import PhosphorusPrecond

    def eigs(self, mu, tol, max_solves, start):
        self.clock = {"factor": 0.0, "solve": 0.0, "host": 0.0}
        self.restart = np.zeros(24)
        return np.array([0.0, 0.04 + 0.0j]), np.ones(24), 8

    monkeypatch.setattr(PhosphorusPrecond, "_smallest_eigs", eigs)
    return PhosphorusPrecond(eng, np.ones((4, 2)), (0.0, 1.0))


def test_with_the_knob_unset_apply_makes_the_five_calls(monkeypatch):
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("NK2D_PHOS_PC_FUSED", raising=False)
        else:
            monkeypatch.setenv("NK2D_PHOS_PC_FUSED", value)
        eng = RecordingEngine()
        pc = _precond(monkeypatch, eng)
        assert not pc.fused
        assert ("shift_factor", (0.02, 0.01)) in eng.calls
        assert not [c for c in eng.calls if c[0] == "precond_set_nullspace"]
        eng.calls.clear()
        res = pc.apply("v", out="out")
        names = [c[0] for c in eng.calls]
        assert names == ["shift_solve", "shift_solve", "axpby", "dot", "axpby", "axpby"], names
        full, half = "vec1", "vec2"
        assert eng.calls[0] == ("shift_solve", 0, "v") and eng.calls[1] == ("shift_solve", 1, "v")
        assert eng.calls[2] == ("axpby", 2.0, half, -1.0, full, half)
        assert eng.calls[3] == ("dot", half, pc.ones)
        assert eng.calls[4] == ("axpby", 1.0, half, -0.25, pc.e_hat, half)
        assert eng.calls[5] == ("axpby", 1.0, half, -1.0, "v", "out") and res == "out"


def test_with_the_knob_set_the_library_keeps_e_hat_and_apply_is_one_call(monkeypatch):
    monkeypatch.setenv("NK2D_PHOS_PC_FUSED", "1")
    eng = RecordingEngine()
    pc = _precond(monkeypatch, eng)
    assert pc.fused
    # declared after the factorisation of the two shifted systems, with the scaled null vector
    names = [c[0] for c in eng.calls]
    assert names.index("precond_set_nullspace") > len(names) - 1 - names[::-1].index("shift_factor")
    assert eng.calls[names.index("precond_set_nullspace")] == ("precond_set_nullspace", pc.e_hat)
    eng.calls.clear()
    pc.apply("v")
    assert eng.calls == [("precond_apply", "v")]
