"""Utterances of several event lists (gvtm_tracks_chunks_frame_count, gvtm_generate_tracks_chunks_device,
gvtm_synthesize_events_chunks_device): the exported names, the host-side frame count and the device entries' argument
checks on design-only plans.  No GPU needed."""
import ctypes
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists

from chunk_cases import list_with_frames, offset_tables
from voice_cases import configs, configs5, track_configs

OK, INVALID_ARGUMENT, NO_DEVICE = 0, 1, 2
BAD_COUNT = ctypes.c_size_t(-1).value
NAMES = ("gvtm_tracks_chunks_frame_count", "gvtm_generate_tracks_chunks_device", "gvtm_synthesize_events_chunks_device")


def test_the_three_names_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NAMES) <= exported


def chunk_structures():
    L = lambda seed, n: event_lists.random_event_table(seed, n_events=n)
    e0, e1, e2 = L(50, 0), L(51, 1), L(52, 2)
    return {"none": [],
            "one": [L(1, 40)],
            "empty_only": [e0],
            "short_only": [e0, e1, e0],
            "two": [L(2, 17), L(3, 33)],
            "short_first": [e0, L(4, 9), e1, L(5, 25), e2],
            "short_middle": [e1, L(6, 9), e2, L(7, 3), e0],
            "short_last": [e2, L(8, 33), e0, L(9, 80), e1],
            "ring_edges": [list_with_frames(c) for c in (1, 31, 32, 33)],
            "long": [L(10, 240), L(11, 241)]}


@pytest.mark.parametrize("name", list(chunk_structures()))
def test_frame_count_is_the_sum_over_the_chunks(name):
    chunks = chunk_structures()[name]
    events, chunk_offsets, _ = offset_tables([chunks])
    assert chunk_offsets.shape[0] == len(chunks) + 1
    period2 = track_configs()[0]
    period2.control_period_ms = 2  # twice the frames
    for cfg in (track_configs()[0], period2):
        singles = [capi.tracks_frame_count(cfg, capi.events_from_table(t)) for t in chunks]
        assert all((s > 0) == (t.shape[0] >= 2) for s, t in zip(singles, chunks))
        assert capi.tracks_chunks_frame_count(cfg, events, chunk_offsets) == sum(singles)
        if name == "ring_edges":
            assert singles == [c * 4 // cfg.control_period_ms for c in (1, 31, 32, 33)]
    if name == "none":
        # n_chunks == 0: nothing is read but the configuration
        assert g.load_library().gvtm_tracks_chunks_frame_count(ctypes.byref(track_configs()[0]), None, None, 0) == 0


def test_frame_count_refusals():
    lib = g.load_library()
    events, chunk_offsets, _ = offset_tables([chunk_structures()["two"]])
    good = track_configs()[0]
    args = (events.ctypes.data, chunk_offsets.ctypes.data, 2)
    assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(good), *args) not in (0, BAD_COUNT)
    # what gvtm_tracks_frame_count refuses: a control period of 0, a cutoff above 0.48 of the drift rate, reserved_
    for key, value in (("control_period_ms", 0), ("drift_lowpass_cutoff", 0.48 * 250.0 + 1.0), ("reserved_", 1)):
        bad = track_configs()[0]
        setattr(bad, key, value)
        assert lib.gvtm_tracks_frame_count(ctypes.byref(bad), events.ctypes.data, 17) == BAD_COUNT, key
        assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(bad), *args) == BAD_COUNT, key
        assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(bad), None, None, 0) == BAD_COUNT, key
        with pytest.raises(capi.GvtmError):
            capi.tracks_chunks_frame_count(bad, events, chunk_offsets)
    # nulls with n_chunks > 0, a null configuration, offsets that decrease
    assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(good), None, chunk_offsets.ctypes.data, 2) == BAD_COUNT
    assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(good), events.ctypes.data, None, 2) == BAD_COUNT
    assert lib.gvtm_tracks_chunks_frame_count(None, *args) == BAD_COUNT
    backwards = np.array([0, 17, 10], dtype=np.int64)
    assert lib.gvtm_tracks_chunks_frame_count(ctypes.byref(good), events.ctypes.data, backwards.ctypes.data, 2) == BAD_COUNT


def device_entries(plan):
    """Status of the two device entries on a small (host-memory, never dereferenced) batch."""
    lib = plan._lib
    ev = np.zeros(4, dtype=capi.EVENT_DTYPE)
    chunk_offsets = np.array([0, 2, 4], dtype=np.int64)
    utt_chunks = np.array([0, 1, 2], dtype=np.int64)
    ids = np.zeros(2, dtype=np.int32)
    params = np.zeros((2, 8, 16), dtype=np.float32)
    audio = np.zeros((2, 65536), dtype=np.float32)
    gen = lib.gvtm_generate_tracks_chunks_device(plan._h, ev.ctypes.data, chunk_offsets.ctypes.data, utt_chunks.ctypes.data, ids.ctypes.data, 2, 8,
                                                 params.ctypes.data, None, None, None)
    syn = lib.gvtm_synthesize_events_chunks_device(plan._h, ev.ctypes.data, chunk_offsets.ctypes.data, utt_chunks.ctypes.data, ids.ctypes.data, 2, 8,
                                                   audio.ctypes.data, 65536, None, None, None, None, None)
    return gen, syn


@pytest.mark.parametrize("model5", [False, True], ids=["models0-4", "model5"])
def test_device_entries_want_the_table_first_and_then_a_device(model5):
    plan = g.VoicesPlan(configs5(48000.0) if model5 else configs(), 250.0, capi.DEVICE_NONE)
    assert device_entries(plan) == (INVALID_ARGUMENT, INVALID_ARGUMENT)
    assert "gvtm_plan_set_voice_tracks" in plan._lib.gvtm_last_error().decode()
    plan.set_voice_tracks(track_configs())
    assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)


def test_a_null_plan_is_refused():
    lib = g.load_library()
    assert lib.gvtm_generate_tracks_chunks_device(None, None, None, None, None, 0, 0, None, None, None, None) == INVALID_ARGUMENT
    assert lib.gvtm_synthesize_events_chunks_device(None, None, None, None, None, 0, 0, None, 0, None, None, None, None, None) == INVALID_ARGUMENT
