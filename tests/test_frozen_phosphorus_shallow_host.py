"""Option "frozen_phosphorus_shallow" (the one-launch frozen year for the phosphorus module at one and two levels per lane, DESIGN.md
section 3.6.4) adds an option, a counter and an environment name, no entry point: the header still declares 56 and documents the
new names, the library holds them, README and engine name the environment variable, and the planner's rules for such a context
hold under AddressSanitizer on the CPU."""
import os
import re

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("frozen_phosphorus_shallow", "frozen_phosphorus_shallow_years")
ENV = "NK2D_FROZEN_PHOSPHORUS_SHALLOW"


def test_header_documents_the_option_and_the_counter_and_declares_56_entry_points():
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    body = header[header.index('extern "C"'):]
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", body))
    assert len(declared) == 56, len(declared)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in NAMES:
        assert f'"{name}"' in header, name
    assert re.search(r"\b%s\b" % ENV, header)
    # the new option's text stands behind "frozen_phosphorus"'s, which stays what it was
    old = header.index("three to eight levels per lane", header.index('"frozen_phosphorus"'))
    assert old < header.index('"frozen_phosphorus_shallow"')
    # the names are the library's own, not only the header's
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in NAMES:
        assert name.encode() in blob, name
    assert b"frozen_phosphorus_shallow is 0 or 1" in blob


def test_readme_and_engine_name_the_environment_variable():
    from nk_ooc_amd import engine

    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"`{ENV}`" in readme and "`frozen_phosphorus_shallow`" in readme and "`frozen_phosphorus_shallow_years`" in readme
    src = open(engine.__file__).read()
    pat = r'if "%s" in os\.environ:\s*\n\s*self\.set_option\("frozen_phosphorus_shallow", float\(os\.environ\["%s"\]\)\)' % (ENV, ENV)
    assert re.search(pat, src)
    # before the engine's first year: in the constructor, beside the option it extends
    assert src.index('"NK2D_FROZEN_PHOSPHORUS"') < src.index(f'"{ENV}"') < src.index("def set_option")


def test_design_names_the_option():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`frozen_phosphorus_shallow`" in design and ENV in design
    assert "frozen_phosphorus_shallow_years" in design


def test_frozen_plan_shallow_under_address_sanitizer():
    """csrc/nk2d_frozen_plan.h for a phosphorus context at one and two levels per lane (eligibility with the field 0 and 1, nothing in
    LDS and by column for every option value, the row size, the form key) against hand-derived answers, built with a plain g++
    under -fsanitize=address,undefined and run on the CPU: `make asan-host`, tests/host_asan/test_frozen_plan_shallow.cpp"""
    import shutil
    import subprocess

    import pytest

    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "newton-krylov_ooc_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "asan-host"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "frozen plan shallow ok" in res.stdout
    assert "frozen plan ok" in res.stdout and "hostmath ok" in res.stdout
