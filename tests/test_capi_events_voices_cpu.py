"""Per-voice track configurations of a plan (gvtm_plan_set_voice_tracks) and the events-voices entries' argument checks, on
design-only plans: five voices of the models 0-4 and of reference model 5.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi

from voice_cases import configs, configs5, track_configs

OK, INVALID_ARGUMENT, NO_DEVICE = 0, 1, 2
REFERENCE_GLOTTAL_PITCH = [-12.0, 0.0, 2.5, 5.0, 7.5]  # of the five variants, in VOICES' order


def plans():
    return [g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE),
            g.VoicesPlan(configs5(48000.0), 250.0, capi.DEVICE_NONE)]


@pytest.fixture(params=[0, 1], ids=["models0-4", "model5"])
def plan(request):
    return plans()[request.param]


def set_tracks(plan, cfgs, n=None, null=False):
    arr = (capi.TrackConfig * max(len(cfgs), 1))(*cfgs)
    rc = plan._lib.gvtm_plan_set_voice_tracks(plan._h, None if null else arr, len(cfgs) if n is None else n)
    return rc, plan._lib.gvtm_last_error().decode()


def device_entries(plan):
    """Status of the two device entries on a small (host-memory, never dereferenced) batch."""
    lib = plan._lib
    ev = np.zeros(4, dtype=capi.EVENT_DTYPE)
    off = np.array([0, 2, 4], dtype=np.int64)
    ids = np.zeros(2, dtype=np.int32)
    params = np.zeros((2, 8, 16), dtype=np.float32)
    audio = np.zeros((2, 65536), dtype=np.float32)
    gen = lib.gvtm_generate_tracks_voices_device(plan._h, ev.ctypes.data, off.ctypes.data, ids.ctypes.data, 2, 8, params.ctypes.data, None, None, None)
    syn = lib.gvtm_synthesize_events_voices_device(plan._h, ev.ctypes.data, off.ctypes.data, ids.ctypes.data, 2, 8, audio.ctypes.data, 65536,
                                                   None, None, None, None, None)
    return gen, syn


def test_mean_pitches_follow_the_variant_files():
    for model5 in (False, True):
        assert [c.mean_pitch for c in track_configs(model5=model5)] == [-4.0 + p for p in REFERENCE_GLOTTAL_PITCH] == [-16.0, -4.0, -1.5, 1.0, 3.5]


def test_five_configurations_are_accepted(plan):
    plan.set_voice_tracks(track_configs(model5=bool(plan.info.model5)))
    plan.set_voice_tracks(track_configs(model5=bool(plan.info.model5)))  # and again


def test_device_entries_want_the_table_first_and_then_a_device(plan):
    assert device_entries(plan) == (INVALID_ARGUMENT, INVALID_ARGUMENT)
    assert "gvtm_plan_set_voice_tracks" in plan._lib.gvtm_last_error().decode()
    plan.set_voice_tracks(track_configs())
    assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)
    lib = plan._lib
    assert lib.gvtm_generate_tracks_voices_device(None, None, None, None, 0, 0, None, None, None, None) == INVALID_ARGUMENT
    assert lib.gvtm_synthesize_events_voices_device(None, None, None, None, 0, 0, None, 0, None, None, None, None, None) == INVALID_ARGUMENT


def test_refusals_name_the_voice(plan):
    good = track_configs()
    rc, msg = set_tracks(plan, good[:4])
    assert rc == INVALID_ARGUMENT and "4" in msg and "5" in msg
    rc, msg = set_tracks(plan, good, n=6)
    assert rc == INVALID_ARGUMENT
    # control period 2 ms on a plan of 250 Hz (4 ms): voice 1
    cfgs = track_configs()
    cfgs[1].control_period_ms = 2
    rc, msg = set_tracks(plan, cfgs)
    assert rc == INVALID_ARGUMENT and msg.startswith("voice 1: ") and "control" in msg
    # a low-pass cutoff above 0.48 of the drift generator's rate: voice 3
    cfgs = track_configs()
    cfgs[3].drift_lowpass_cutoff = 0.48 * 250.0 + 1.0
    rc, msg = set_tracks(plan, cfgs)
    assert rc == INVALID_ARGUMENT and msg.startswith("voice 3: ") and "drift_lowpass_cutoff" in msg
    cfgs = track_configs()
    cfgs[4].reserved_ = 1
    rc, msg = set_tracks(plan, cfgs)
    assert rc == INVALID_ARGUMENT and msg.startswith("voice 4: ") and "reserved_" in msg
    # nulls
    assert set_tracks(plan, good, null=True)[0] == INVALID_ARGUMENT
    arr = (capi.TrackConfig * 5)(*good)
    assert plan._lib.gvtm_plan_set_voice_tracks(None, arr, 5) == INVALID_ARGUMENT
    # none of the refused calls set a table
    assert device_entries(plan) == (INVALID_ARGUMENT, INVALID_ARGUMENT)


def test_a_refused_call_leaves_the_previous_table(plan):
    plan.set_voice_tracks(track_configs())
    assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)
    cfgs = track_configs()
    cfgs[3].drift_lowpass_cutoff = 200.0
    rc, msg = set_tracks(plan, cfgs)
    assert rc == INVALID_ARGUMENT and msg.startswith("voice 3: ")
    assert set_tracks(plan, track_configs()[:2])[0] == INVALID_ARGUMENT
    # the plan still holds the first table: the device entries get as far as the missing device
    assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)


def test_one_voice_plan_takes_one_configuration():
    vp = g.VoicesPlan(configs(names=["female"]), 250.0, capi.DEVICE_NONE)
    assert set_tracks(vp, track_configs())[0] == INVALID_ARGUMENT
    vp.set_voice_tracks(track_configs(names=["female"]))
    assert device_entries(vp) == (NO_DEVICE, NO_DEVICE)


def test_binding_raises_with_the_librarys_message(plan):
    cfgs = track_configs()
    cfgs[2].control_period_ms = 1
    with pytest.raises(capi.GvtmError) as ei:
        plan.set_voice_tracks(cfgs)
    assert ei.value.status == INVALID_ARGUMENT and "voice 2" in str(ei.value)
