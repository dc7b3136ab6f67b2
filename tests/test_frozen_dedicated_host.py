"""Option "frozen_dedicated" without a GPU: the routing rule of csrc/nk2d_frozen_plan.h under AddressSanitizer, and that the option,
its environment variable and its counters are named where a user looks for them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "NK2D_FROZEN_DEDICATED"


def test_engine_reads_the_environment_variable():
    from nk_ooc_amd import engine

    src = open(engine.__file__).read()
    pat = r'if "%s" in os\.environ:\s*\n\s*self\.set_option\("frozen_dedicated", float\(os\.environ\["%s"\]\)\)' % (ENV, ENV)
    assert re.search(pat, src)
    assert src.index(f'"{ENV}"') < src.index("def set_option")      # (in the constructor: before the engine's first year)


def test_documents_name_the_option():
    for name in ("README.md", "DESIGN.md", os.path.join("include", "nk2d.h")):
        text = open(os.path.join(ROOT, name)).read()
        for word in ("frozen_dedicated", "frozen_dedicated_years", "frozen_dedicated_bits"):
            assert word in text, (name, word)
    assert ENV in open(os.path.join(ROOT, "README.md")).read()


def test_new_unit_is_a_source_of_the_library():
    """listed where the library's sources are listed: the Makefile's SRCS, from which the build id is formed too"""
    mk = open(os.path.join(ROOT, "newton-krylov_ooc_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "nk2d_frozen_d.hip" in srcs and "nk2d_frozen.hip" in srcs
    assert re.search(r"^nk2d_build_id\.h: \$\(SRCS\)", mk, re.M)


def test_frozen_plan_dedicated_under_address_sanitizer():
    """frozen_dedicated() and NK2D_FROZEN_DEDICATED against hand-derived answers, built with a plain g++ under
    -fsanitize=address,undefined and run on the CPU: `make asan-host`, tests/host_asan/test_frozen_plan_dedicated.cpp"""
    import shutil
    import subprocess

    import pytest

    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "newton-krylov_ooc_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "asan-host"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "frozen plan dedicated ok" in res.stdout
