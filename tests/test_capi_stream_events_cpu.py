"""Streams fed event lists (gvtm_stream_push_events, gvtm_stream_get_drift, gvtm_stream_set_drift): the exported names,
the refusal of a null stream, the Python methods and the header's declarations.  No GPU needed (a stream only exists on a
device plan: everything behind these checks is tests/test_gpu_stream_events.py's)."""
import os
import re
import subprocess

import gama_tts_amd as g
from gama_tts_amd import capi

INVALID_ARGUMENT = 1
NAMES = ("gvtm_stream_push_events", "gvtm_stream_get_drift", "gvtm_stream_set_drift")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gama_vtm.h")


def exported(diagnostics=False):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path(diagnostics)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_the_three_names_are_exported():
    assert set(NAMES) <= exported()
    assert set(NAMES) <= exported(diagnostics=True)


def test_the_two_kernel_hooks_are_the_diagnostics_library_s_alone():
    hooks = {"gvtm_debug_tracks_append", "gvtm_debug_carry_rows"}
    assert hooks <= exported(diagnostics=True)
    assert not hooks & exported()


def test_a_null_stream_is_refused():
    lib = g.load_library()
    assert lib.gvtm_stream_push_events(None, None, None, None, None, 0, None, None) == INVALID_ARGUMENT
    assert "null stream" in lib.gvtm_last_error().decode()
    assert lib.gvtm_stream_get_drift(None, None) == INVALID_ARGUMENT
    assert lib.gvtm_stream_set_drift(None, None) == INVALID_ARGUMENT


def test_the_python_stream_has_the_three_methods():
    for name in ("push_events", "get_drift", "set_drift"):
        assert callable(getattr(capi.Stream, name))


def test_the_header_declares_the_functions():
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    # the drift rule is the header's to state: resets leave the generators alone, set_drift(NULL) reseeds
    assert "gvtm_stream_set_drift(stream, NULL)" in text
