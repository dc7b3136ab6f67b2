"""Option "stream_hist" (history samples as commands of the year's resident kernel) adds options and counters, no entry
point: the library exports exactly the symbols include/nk2d.h declares -- 56 -- and the header documents the new names."""
import os
import re
import shutil
import subprocess

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exported(path):
    """the dynamic symbols with C linkage that the library defines under the project's prefix"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm to list the library's symbols with"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("nk2d_")}


def test_stream_hist_adds_no_entry_point_and_is_documented():
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    body = header[header.index('extern "C"'):]
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", body))
    assert len(declared) == 56, len(declared)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    _lib.load()
    exported = _exported(_lib.LIB_PATH)
    assert exported == declared, exported ^ declared
    for name in ('"stream_hist"', '"stream_hist_mb"', '"stream_hist_samples"', '"stream_hist_drains"'):
        assert name in header, name
    # the option and its counters are the library's, not only the header's: their names are in its read-only data
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"stream_hist_mb", b"stream_hist_samples", b"stream_hist_drains"):
        assert name in blob, name
