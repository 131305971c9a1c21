"""Streams that listen, without a GPU: the names of the section "Streams that listen" of include/gama_vtm.h in the header, the
export list and the binding, the rule's arithmetic (gvtm_listen_buffer_count) against integer arithmetic, and the refusals
of a null stream."""
import ctypes
import os
import re
import subprocess

import numpy as np

import gama_tts_amd as g
from gama_tts_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gvtm_listen_buffer_count", "gvtm_stream_listen", "gvtm_stream_unlisten", "gvtm_stream_listen_state", "gvtm_stream_take_spectra",
         "gvtm_stream_peek_spectra_device"]
RING = 65536
INVALID_ARGUMENT = 1


def test_names_are_in_the_header_the_export_list_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    lib = g.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout.split()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.PROTOTYPES and hasattr(lib, name) and name in exported, name
    for constant, value in [("GVTM_LISTEN_SPECTRA", 1), ("GVTM_LISTEN_SIGNAL", 2)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (constant, value), header), constant
    assert (capi.LISTEN_SPECTRA, capi.LISTEN_SIGNAL) == (1, 2)
    for method in ("listen", "unlisten", "listen_state", "take_spectra", "peek_spectra_device"):
        assert callable(getattr(g.Stream, method)), method
    # the section stands behind the analysis section
    assert header.index(" * Streams that listen:") > header.index("int gvtm_analyze_spectrum_device(")


def test_buffer_count_is_integer_arithmetic():
    cases = []
    for fill in (0, 1, 65535):
        for n_new in (0, 1, RING - fill - 1, RING - fill, RING - fill + 1, 2 * RING + 3):
            cases.append((fill, n_new))
    assert len(cases) == 18 and (65535, 0) in cases and (0, RING) in cases
    for fill, n_new in cases:
        got = capi.listen_buffer_count(fill, n_new)
        assert got == ((fill + n_new) // RING, (fill + n_new) % RING), (fill, n_new, got)
    assert capi.listen_buffer_count(0, RING - 1) == (0, RING - 1) and capi.listen_buffer_count(1, RING - 1) == (1, 0)
    assert capi.listen_buffer_count(65535, 2 * RING + 3) == (3, 2)
    # a null fill_after; a fill that is no ring's, a negative count: nothing completes, the fill stays
    lib = g.load_library()
    assert lib.gvtm_listen_buffer_count(65535, 1, None) == 1
    assert capi.listen_buffer_count(RING, 5) == (0, RING) and capi.listen_buffer_count(-1, RING) == (0, -1)
    assert capi.listen_buffer_count(7, -1) == (0, 7)


def test_every_stream_entry_refuses_a_null_stream():
    lib = g.load_library()
    analysis = g.Analysis(capi.WINDOW_BLACKMAN, 1024, device=capi.DEVICE_NONE)
    fill, queued = np.zeros(1, np.int64), np.zeros(1, np.int32)
    pointers = [ctypes.c_void_p() for _ in range(3)]
    calls = [lambda: lib.gvtm_stream_listen(None, analysis._h, 1, capi.LISTEN_SPECTRA),
             lambda: lib.gvtm_stream_unlisten(None),
             lambda: lib.gvtm_stream_listen_state(None, capi._ptr(fill), capi._ptr(queued)),
             lambda: lib.gvtm_stream_take_spectra(None, None, None, capi._ptr(queued)),
             lambda: lib.gvtm_stream_peek_spectra_device(None, *[ctypes.byref(p) for p in pointers])]
    assert len(calls) == len(NAMES) - 1
    for call in calls:
        assert call() == INVALID_ARGUMENT
        assert b"null stream" in lib.gvtm_last_error()
    assert not any(p.value for p in pointers)
