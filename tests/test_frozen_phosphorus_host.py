"""Option "frozen_phosphorus" (the one-launch frozen year for the phosphorus module) adds an option, two
counters and an environment name, no entry point: the header still declares 56 and documents the new names, and README and
engine name the environment variable."""
import os
import re

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("frozen_phosphorus", "frozen_phosphorus_years", "frozen_two_waves_years")
ENV = "NK2D_FROZEN_PHOSPHORUS"


def test_header_documents_the_option_and_the_counters_and_declares_56_entry_points():
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    body = header[header.index('extern "C"'):]
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", body))
    assert len(declared) == 56, len(declared)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in NAMES:
        assert f'"{name}"' in header, name
    assert ENV in header
    # one and two levels per lane stay out, and the header says so
    assert "three to eight levels per lane" in header[header.index('"frozen_phosphorus"'):]
    # the names are the library's own, not only the header's
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in NAMES:
        assert name.encode() in blob, name


def test_readme_and_engine_name_the_environment_variable():
    from nk_ooc_amd import engine

    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"`{ENV}`" in readme and "`frozen_phosphorus`" in readme
    src = open(engine.__file__).read()
    pat = r'if "%s" in os\.environ:\s*\n\s*self\.set_option\("frozen_phosphorus", float\(os\.environ\["%s"\]\)\)' % (ENV, ENV)
    assert re.search(pat, src)
    # before the engine's first year: in the constructor, beside the forced module's option
    assert src.index('"NK2D_FROZEN_FORCED"') < src.index(f'"{ENV}"') < src.index("def set_option")
