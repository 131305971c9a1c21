"""Parameter targets under a mix of voices, the host side (gvtm_targets_voice_output_count,
gvtm_targets_voices_output_capacity) and the refusals of gvtm_synthesize_targets_voices_device as far as a design-only plan
lets them go.  No GPU needed.

Pins: the counts by steps of every voice of a five-voice plan against the one-voice plan of that voice's configuration, at
step counts around each voice's own filter length, on an up-sampling and on a down-sampling plan; the capacity as the largest
of the voices'; (size_t)-1 for a null plan and a voice outside the plan; the order of the entry's refusals -- arguments, then
the plan's model, then the device -- on plans of one voice, of several, and of model 5 in both classes; the three names in
the header, the library and the binding."""
import ctypes
import functools
import os
import subprocess

import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import targets_io
from voice_cases import configs, configs5, male_plan, model5_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
NONE = ctypes.c_size_t(-1).value
ENTRIES = ("gvtm_targets_voice_output_count", "gvtm_targets_voices_output_capacity", "gvtm_synthesize_targets_voices_device")


def test_names_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ENTRIES:
        assert name + "(" in header and name in exported and name in capi.PROTOTYPES, name


# ---- 1. counts per voice ----

@pytest.mark.parametrize("rate", [44100.0, 16000.0], ids=["up", "down-16k"])
def test_counts_per_voice_are_the_one_voice_plans(rate):
    cfgs = configs(rate, 1, capi.PRECISION_F32)
    plan = g.VoicesPlan(cfgs, 250.0, capi.DEVICE_NONE)
    assert plan.n_voices == 5
    singles = [g.Plan(c, 250.0, capi.DEVICE_NONE) for c in cfgs]
    lengths = [plan.targets_filter_length(v) for v in range(5)]
    assert len(set(lengths)) >= 2  # voices whose windows differ
    sizes = set()
    for v, single in enumerate(singles):
        n = lengths[v]
        assert n == single.targets_filter_length()
        for s in (0, 1, n - 1, n, n + 1, 5000):
            sizes.add(s)
            assert plan.targets_voice_output_count(v, s) == single.targets_output_count(s), (v, s)
    for s in sorted(sizes):
        assert plan.targets_voices_output_capacity(s) == max(single.targets_output_capacity(s) for single in singles), s
    if rate == 16000.0:
        # a down-sampling plan keeps the reference's ring: the row is longer than any utterance of that many steps
        assert all(plan.voice_info(v).internal_rate_hz > rate for v in range(5))
        assert plan.targets_voices_output_capacity(5000) > max(plan.targets_voice_output_count(v, 5000) for v in range(5))
    # voice 0's are the plan's own (gvtm_targets_output_count looks at the first voice)
    assert plan.targets_voice_output_count(0, 777) == plan.targets_output_count(777)
    # a plan of one voice has the two as well
    assert singles[2].targets_voice_output_count(0, 777) == singles[2].targets_output_count(777)
    assert singles[2].targets_voices_output_capacity(777) == singles[2].targets_output_capacity(777)


def test_error_returns():
    lib = g.load_library()
    assert lib.gvtm_targets_voice_output_count(None, 0, 5) == NONE
    assert lib.gvtm_targets_voices_output_capacity(None, 5) == NONE
    plan = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
    assert plan.targets_voice_output_count(-1, 5) == NONE
    assert plan.targets_voice_output_count(plan.n_voices, 5) == NONE
    assert plan.targets_voice_output_count(plan.n_voices - 1, 5) != NONE
    single = male_plan(device=capi.DEVICE_NONE)
    assert single.targets_voice_output_count(1, 5) == NONE and single.targets_voice_output_count(0, 5) != NONE


# ---- 2. the device entry's refusals ----

device_entry = functools.partial(targets_io.device_entry, entry_name="gvtm_synthesize_targets_voices_device", voices=True)


def plan_of(kind):
    if kind == "one-voice":
        return male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    if kind == "one-voice-voices-plan":
        return g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["female"]), 250.0, capi.DEVICE_NONE)
    if kind == "five-voices":
        return g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
    if kind == "model5-voices":
        return g.VoicesPlan(configs5(names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    return model5_plan("male", float_class=kind == "model5-float", device=capi.DEVICE_NONE)


@pytest.mark.parametrize("kind", ["one-voice", "one-voice-voices-plan", "five-voices", "model5", "model5-float", "model5-voices"])
def test_entry_checks_its_arguments_then_the_model_then_wants_a_device(kind):
    plan = plan_of(kind)
    lib = plan._lib
    after_checks = UNSUPPORTED if kind.startswith("model5") else NO_DEVICE
    assert device_entry(plan) == after_checks
    for null in ("offsets", "steps", "values", "audio", "voices"):
        assert device_entry(plan, null=null) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error(), null
    assert device_entry(plan, n_lists=31) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=3, ids=True) == after_checks  # with ids lists may be shared
    assert device_entry(plan, max_steps=2 ** 31) == INVALID_ARGUMENT and b"step counter" in lib.gvtm_last_error()
    capacity = plan.targets_voices_output_capacity(8)
    assert device_entry(plan, stride=capacity - 1) == INVALID_ARGUMENT and b"gvtm_targets_voices_output_capacity" in lib.gvtm_last_error()
    assert device_entry(plan, stride=capacity) == after_checks
    # the order: a null table before the lists' number, that before the stride, the stride before the plan's kind
    assert device_entry(plan, null="voices", stride=1) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=31, stride=1) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    # batch == 0: nothing is looked at but the plan -- and a design-only plan has no device
    assert device_entry(plan, batch=0, null="voices", stride=0) == after_checks


def test_the_stride_is_held_against_the_longest_voice():
    # (the male voice's tube is the longest and its internal rate the lowest: it yields the most samples per step)
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["baby", "male"]), 250.0, capi.DEVICE_NONE)
    own = plan.targets_output_capacity(5000)  # voice 0's
    capacity = plan.targets_voices_output_capacity(5000)
    assert capacity > own
    assert device_entry(plan, stride=own, max_steps=5000) == INVALID_ARGUMENT
    assert device_entry(plan, stride=capacity, max_steps=5000) == NO_DEVICE


def test_a_null_plan_is_refused():
    lib = g.load_library()
    args = [None] * 16
    for i in (2, 8, 9, 11):
        args[i] = 0
    assert lib.gvtm_synthesize_targets_voices_device(*args) == INVALID_ARGUMENT
