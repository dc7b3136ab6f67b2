"""Option "frozen_cache_pieces" (the schedule cache of the one-launch frozen year as a list of pieces) adds options, counters
and environment names, no entry point: the header still declares 56 and documents the new names, and the engine hands the
three environment names to nk2d_set_option."""
import os
import re

from nk_ooc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTIONS = ("frozen_cache_pieces", "frozen_cache_piece_mb", "frozen_cache_piece_rows", "frozen_cache_early")
COUNTERS = ("frozen_cache_pieces", "frozen_cache_piece_allocs", "frozen_cache_early_requests", "frozen_cache_bytes",
            "frozen_cache_pending")
ENV = {"NK2D_FROZEN_CACHE_PIECES": "frozen_cache_pieces", "NK2D_FROZEN_CACHE_PIECE_MB": "frozen_cache_piece_mb",
       "NK2D_FROZEN_CACHE_EARLY": "frozen_cache_early"}


def test_header_names_the_options_and_counters_and_declares_56_entry_points():
    header = open(os.path.join(ROOT, "include", "nk2d.h")).read()
    body = header[header.index('extern "C"'):]
    declared = set(re.findall(r"\b(nk2d_[a-z0-9_]+)\s*\(", body))
    assert len(declared) == 56, len(declared)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in OPTIONS + COUNTERS:
        assert f'"{name}"' in header, name
    # the names are the library's own, not only the header's
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in OPTIONS + COUNTERS:
        assert name.encode() in blob, name


def test_environment_names_reach_set_option():
    """engine.py reads each name where it reads NK2D_STREAM_HIST: `if NAME in os.environ: set_option(option, float(...))`"""
    from nk_ooc_amd import engine

    src = open(engine.__file__).read()
    for env, option in ENV.items():
        pat = r'if "%s" in os\.environ:\s*\n\s*self\.set_option\("%s", float\(os\.environ\["%s"\]\)\)' % (env, option, env)
        assert re.search(pat, src), env
    # and before the engine's first year: in the constructor, beside the stream options
    assert src.index('"NK2D_STREAM_HIST"') < src.index('"NK2D_FROZEN_CACHE_PIECES"') < src.index("def set_option")
