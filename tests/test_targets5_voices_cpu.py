"""Model 5 parameter targets under a mix of voices, the host side: gvtm_synthesize_targets_model5_voices_device as far as a
design-only plan lets it go, and the fixture tests/golden/targets5_voices_golden.npz against the host rule.  No GPU needed.

Pins: the name in the header, the library and the binding, with the prototype of gvtm_synthesize_targets_voices_device; the
order of the entry's refusals -- arguments, then the plan's model family, then the one-voice float plan, then the device -- on
design-only plans of every kind; the filter lengths of a five-voice model 5 plan; per fixture case the sample count by steps
of its voice and the SHA-256 of the frames the reference was fed, so that the fixture's inputs cannot drift from the rule."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import targets5_voices_cases as cases
import targets_io
from voice_cases import configs, male_plan
from voice_files import VOICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
ENTRY = "gvtm_synthesize_targets_model5_voices_device"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_voices_golden.npz"))


def test_name_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert ENTRY + "(" in header and ENTRY in exported and ENTRY in capi.PROTOTYPES
    # argument for argument it is the models 0 to 4 entry
    assert capi.PROTOTYPES[ENTRY] == capi.PROTOTYPES["gvtm_synthesize_targets_voices_device"]
    assert hasattr(capi.Plan, "synthesize_targets_model5_voices_device")


# ---- the refusals ----

device_entry = functools.partial(targets_io.device_entry, entry_name=ENTRY, voices=True)


# kind -> (the plan, what the entry answers once its arguments are in order, a word of that refusal's message)
def plan_of(kind):
    if kind == "models-0-4-one-voice":
        return male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE), UNSUPPORTED, b"gvtm_synthesize_targets_voices_device"
    if kind == "models-0-4-voices":
        return g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE), UNSUPPORTED, b"gvtm_synthesize_targets_voices_device"
    if kind == "model5":
        return cases.single_plan(False, "female"), NO_DEVICE, b"design-only"
    if kind == "model5-voices":
        return cases.voices_plan(False), NO_DEVICE, b"design-only"
    if kind == "model5-float":
        return cases.single_plan(True, "female"), UNSUPPORTED, b"no launch of several voices"
    assert kind == "model5-float-voices"
    return cases.voices_plan(True), NO_DEVICE, b"design-only"


KINDS = ["models-0-4-one-voice", "models-0-4-voices", "model5", "model5-voices", "model5-float", "model5-float-voices"]


@pytest.mark.parametrize("kind", KINDS)
def test_entry_checks_its_arguments_then_the_plan_then_wants_a_device(kind):
    plan, after_checks, word = plan_of(kind)
    lib = plan._lib
    assert device_entry(plan) == after_checks and word in lib.gvtm_last_error(), lib.gvtm_last_error()
    for null in ("offsets", "steps", "values", "audio", "voices"):
        assert device_entry(plan, null=null) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error(), null
    assert device_entry(plan, n_lists=31) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=3, ids=True) == after_checks  # with ids lists may be shared
    assert device_entry(plan, max_steps=2 ** 31) == INVALID_ARGUMENT and b"step counter" in lib.gvtm_last_error()
    capacity = plan.targets_voices_output_capacity(8)
    assert device_entry(plan, stride=capacity - 1) == INVALID_ARGUMENT and b"gvtm_targets_voices_output_capacity" in lib.gvtm_last_error()
    assert device_entry(plan, stride=capacity) == after_checks
    # the order: what check_batch_arguments refuses before the voice ids, those before the stride, the stride before the plan
    assert device_entry(plan, null="offsets", n_lists=31, stride=1) == INVALID_ARGUMENT and b"null list offsets" in lib.gvtm_last_error()
    assert device_entry(plan, null="voices", n_lists=31, stride=1) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    assert device_entry(plan, null="voices", stride=1) == INVALID_ARGUMENT and b"null voice ids" in lib.gvtm_last_error()
    # batch == 0: nothing is looked at but the plan -- and a design-only plan has no device
    assert device_entry(plan, batch=0, null="voices", stride=0) == after_checks and word in lib.gvtm_last_error()


def test_a_null_plan_is_refused():
    lib = g.load_library()
    args = [None] * 16
    for i in (2, 8, 9, 11):
        args[i] = 0
    assert getattr(lib, ENTRY)(*args) == INVALID_ARGUMENT and b"null plan" in lib.gvtm_last_error()


def test_the_stride_is_held_against_the_longest_voice():
    # (the male voice's tube is the longest and its internal rate the lowest: it yields the most samples per step)
    plan = cases.voices_plan(False, names=["baby", "male"])
    own = plan.targets_output_capacity(5000)  # voice 0's
    capacity = plan.targets_voices_output_capacity(5000)
    assert capacity > own
    assert device_entry(plan, stride=own, max_steps=5000) == INVALID_ARGUMENT
    assert device_entry(plan, stride=capacity, max_steps=5000) == NO_DEVICE


# ---- the five voices' filters, and the fixture ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_five_voices_have_five_filter_lengths(float_class):
    plan = cases.voices_plan(float_class)
    lengths = [plan.targets_filter_length(v) for v in range(5)]
    assert plan.n_voices == 5 and len(set(lengths)) == 5 and lengths[0] == cases.MALE_N == 3021
    assert lengths == sorted(lengths)  # the shorter the tract, the higher the internal rate and the longer the window
    for v, voice in enumerate(VOICES):
        assert lengths[v] == cases.single_plan(float_class, voice).targets_filter_length()


@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_fixture_counts_and_frames_are_the_host_rules(fixture, float_class):
    plan = cases.voices_plan(float_class)
    all_cases = cases.all_cases(plan, float_class)
    assert len(all_cases) == 4 * (4 if float_class else 3)
    held = {k for k in fixture.files if k.startswith(cases.MODEL[float_class] + "__") and not k.endswith("__frames")}
    assert held == {cases.name(float_class, voice, s) for voice, s in all_cases}
    for voice, s in all_cases:
        key, v = cases.name(float_class, voice, s), VOICES.index(voice)
        assert fixture[key].size == plan.targets_voice_output_count(v, s), key
        assert fixture[key].size <= plan.targets_voices_output_capacity(s), key
        assert bytes(fixture[key + "__frames"]).decode() == cases.sha256_of_frames(cases.frames_of(plan, voice, s)), key
