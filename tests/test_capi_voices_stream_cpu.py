"""Streams over plans of several voices (gvtm_stream_create_voices / gvtm_stream_reset_voices) on design-only plans of the
five 0_male voices (tests/golden/voice_*.txt) and the five 5_male voices (voice5_*.txt): the argument checks and their
order, the Python binding, and gvtm_stream_create still refused on those plans.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
from voice_cases import configs, configs5

INVALID, NO_DEVICE = 1, 2


def plan_v2():
    return g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)


def plan_m5():
    return g.VoicesPlan(configs5(), 250.0, capi.DEVICE_NONE)


PLANS = [plan_v2, plan_m5]


def create(lib, h, ids, batch):
    s = ctypes.c_void_p(12345)
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    rc = lib.gvtm_stream_create_voices(h, None if arr is None else arr.ctypes.data, batch, ctypes.byref(s))
    return rc, s


@pytest.mark.parametrize("make", PLANS)
def test_null_arguments_and_empty_batch(make):
    vp = make()
    lib = vp._lib
    ids = np.zeros(3, dtype=np.int32)
    s = ctypes.c_void_p()
    assert lib.gvtm_stream_create_voices(None, ids.ctypes.data, 3, ctypes.byref(s)) == INVALID
    assert lib.gvtm_stream_create_voices(vp._h, ids.ctypes.data, 3, None) == INVALID
    rc, s = create(lib, vp._h, None, 3)
    assert rc == INVALID and not s.value  # (stream_out cleared)
    rc, s = create(lib, vp._h, ids, 0)
    assert rc == INVALID and not s.value
    # a null argument comes before a bad id
    assert lib.gvtm_stream_create_voices(vp._h, None, 0, None) == INVALID
    assert b"null" in lib.gvtm_last_error()


@pytest.mark.parametrize("make", PLANS)
def test_bad_ids_are_refused_before_the_missing_device(make):
    vp = make()
    lib = vp._lib
    for ids, first in (([0, 1, 5, 2], 2), ([4, -1, 7], 1), ([-3], 0), ([0, 1, 2, 3, 4, 5], 5)):
        rc, s = create(lib, vp._h, ids, len(ids))
        assert rc == INVALID and not s.value, ids
        msg = lib.gvtm_last_error().decode()
        assert ("utterance %d" % first) in msg and str(ids[first]) in msg, msg
    # only the first `batch` ids are read
    rc, _ = create(lib, vp._h, [1, 2, 99], 2)
    assert rc == NO_DEVICE
    # every id in range: the design-only plan is what stops it
    rc, s = create(lib, vp._h, [4, 3, 2, 1, 0, 0], 6)
    assert rc == NO_DEVICE and not s.value


@pytest.mark.parametrize("make", PLANS)
def test_python_stream_with_voice_ids_on_a_design_only_plan(make):
    vp = make()
    with pytest.raises(capi.GvtmError) as e:
        capi.Stream(vp, 5, voice_ids=[0, 1, 2, 3, 4])
    assert e.value.status == NO_DEVICE
    with pytest.raises(capi.GvtmError) as e:
        capi.Stream(vp, 2, voice_ids=[0, 9])
    assert e.value.status == INVALID and "utterance 1" in str(e.value)
    with pytest.raises(ValueError):
        capi.Stream(vp, 3, voice_ids=[0, 1])


@pytest.mark.parametrize("make", PLANS)
def test_stream_create_still_refused_on_several_voices(make):
    vp = make()
    lib = vp._lib
    s = ctypes.c_void_p()
    assert lib.gvtm_stream_create(vp._h, 2, ctypes.byref(s)) == INVALID and not s.value
    assert b"gvtm_stream_create" in lib.gvtm_last_error() and b"5 voices" in lib.gvtm_last_error()
    with pytest.raises(capi.GvtmError) as e:
        capi.Stream(vp, 2)
    assert e.value.status == INVALID


def test_one_voice_plans_take_the_voices_entry_design_only():
    cfg = configs(names=["female"])[0]
    for plan in (g.Plan(cfg, 250.0, capi.DEVICE_NONE), g.VoicesPlan([cfg], 250.0, capi.DEVICE_NONE)):
        rc, _ = create(plan._lib, plan._h, [0, 0], 2)
        assert rc == NO_DEVICE
        rc, _ = create(plan._lib, plan._h, [0, 1], 2)
        assert rc == INVALID and b"utterance 1" in plan._lib.gvtm_last_error()


def test_reset_voices_null_arguments():
    vp = plan_v2()
    lib = vp._lib
    ids = np.zeros(2, dtype=np.int32)
    assert lib.gvtm_stream_reset_voices(None, ids.ctypes.data) == INVALID
