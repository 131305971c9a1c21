"""Model 5 under the interactive window, the host side: gvtm_synthesize_targets_model5_device's name, prototype and refusals
as far as a design-only plan lets them go, and the fixture tests/golden/targets5_golden.npz.  No GPU needed.

Pins: the symbol in the header, the library and the binding, with the header's prototype in the binding's table; the order
of the entry's refusals -- arguments, the stride against gvtm_targets_output_capacity, the plan's kind (the models 0 to 4
and plans of several voices are UNSUPPORTED), then the device (a design-only model 5 plan is NO_DEVICE, with batch 0 too);
gvtm_targets_apply_host at model 5's filter length (3021) against the reference's MovingAverageFilter<float>, by the SHA-256
the fixture stores; the fixture's own sanity -- its frames are the host rule's of today, its interactive samples differ from
the batch protocol's model on the same frames and are as many -- and, where oracle/_ref is built, that ref_vtm gives the
fixture's bytes again."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import targets5_cases as cases
import targets_io
from test_capi_prototypes_cpu import HEADER, c_prototypes, problems, read
from voice_cases import configs, configs5, male_plan, model5_plan

OK, INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
ENTRY = "gvtm_synthesize_targets_model5_device"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_golden.npz"))


# ---- 1. the symbol ----

def test_the_symbol_is_exported_and_its_prototype_is_the_headers():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    assert ENTRY in {line.split()[-1] for line in out.splitlines() if line.split()}
    header = c_prototypes(read(HEADER))
    assert ENTRY in header and ENTRY in capi.PROTOTYPES
    assert problems({ENTRY: header[ENTRY]}, {ENTRY: capi.PROTOTYPES[ENTRY]}) == []
    # argument for argument gvtm_synthesize_targets_device's
    assert header[ENTRY] == header["gvtm_synthesize_targets_device"]
    assert hasattr(g.Plan, "synthesize_targets_model5_device")


# ---- 2. the refusals ----

device_entry = functools.partial(targets_io.device_entry, entry_name=ENTRY, voices=False)


def plan_of(kind):
    if kind == "models-0-4":
        return male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    if kind == "five-voices":
        return g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
    if kind == "model5-voices":
        return g.VoicesPlan(configs5(names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    return model5_plan("male", float_class=kind == "model5-float", device=capi.DEVICE_NONE)


@pytest.mark.parametrize("kind", ["model5", "model5-float", "models-0-4", "five-voices", "model5-voices"])
def test_entry_checks_its_arguments_then_the_plan_then_wants_a_device(kind):
    plan = plan_of(kind)
    lib = plan._lib
    after_checks = NO_DEVICE if kind in ("model5", "model5-float") else UNSUPPORTED
    assert device_entry(plan) == after_checks
    if kind == "models-0-4":
        assert b"gvtm_synthesize_targets_device" in lib.gvtm_last_error()  # (the message points to the other entry)
    for null in ("offsets", "steps", "values", "audio"):
        assert device_entry(plan, null=null) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error(), null
    assert device_entry(plan, n_lists=31) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=3, ids=True) == after_checks  # with ids lists may be shared
    assert device_entry(plan, max_steps=2 ** 31) == INVALID_ARGUMENT and b"step counter" in lib.gvtm_last_error()
    capacity = plan.targets_output_capacity(8)
    assert device_entry(plan, stride=capacity - 1) == INVALID_ARGUMENT and b"gvtm_targets_output_capacity" in lib.gvtm_last_error()
    assert device_entry(plan, stride=capacity) == after_checks
    # the order: a null table before the lists' number, that before the stride, the stride before the plan's kind
    assert device_entry(plan, null="audio", stride=1) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=31, stride=1) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    # batch == 0: nothing is looked at but the plan -- and a design-only plan has no device
    assert device_entry(plan, batch=0, null="audio", stride=0) == after_checks


def test_a_null_plan_is_refused():
    lib = g.load_library()
    args = [None] * 15
    for i in (2, 7, 8, 10):
        args[i] = 0
    assert getattr(lib, ENTRY)(*args) == INVALID_ARGUMENT


# ---- 3. the rule at model 5's filter length ----

@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_host_rule_at_the_model5_filter_length_is_the_references_filter(fixture, float_class):
    plan = model5_plan(device=capi.DEVICE_NONE, float_class=float_class)
    assert plan.targets_filter_length() == cases.N == 3021
    for key in sorted(cases.FILTER_CASES):
        n_steps, lists = cases.filter_case(key)
        frames, status = capi.targets_apply_host(plan, lists, n_steps)
        assert status == 0 and frames.shape == (n_steps, 16)
        assert cases.sha256_of_frames(frames) == bytes(fixture[key + "__sha256"]).decode(), key


# ---- 4. the fixture's own sanity ----

def test_step_counts_cover_every_chunk_of_the_variant():
    assert cases.CHUNKS == {True: (60, 52), False: (56, 24)}
    for float_class in (True, False):
        for chunk in cases.CHUNKS[float_class]:
            assert cases.step_counts(chunk) == [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 3020, 3021, 3022, 3021 + chunk, 6042 + chunk + 5]
            assert set(cases.step_counts(chunk)) <= set(cases.class_counts(float_class))


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_fixture_holds_every_case_made_from_todays_frames(fixture, float_class):
    plan = model5_plan(device=capi.DEVICE_NONE, float_class=float_class)
    for n_steps in cases.class_counts(float_class):
        key = cases.name(float_class, n_steps)
        assert fixture[key].dtype == np.float32 and fixture[key].size == plan.targets_output_count(n_steps), key
        frames = cases.frames_of(plan, n_steps)
        assert cases.sha256_of_frames(frames) == bytes(fixture[key + "__frames"]).decode(), key
        if n_steps > 1000:
            assert np.unique(frames[:, 0]).size > n_steps // 2  # the pitch moves: f0 differs from step to step
    wide = cases.lists_of(sorted(cases.WIDE)[0])
    assert all((np.asarray(wide[p][1]) > 0).all() for p in (5, 6))


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_interactive_samples_differ_from_the_batch_protocols(fixture, float_class):
    for n_steps in cases.PLAIN:
        interactive, plain = fixture[cases.name(float_class, n_steps)], fixture[cases.name(float_class, n_steps, plain=True)]
        assert interactive.size == plain.size > 0
        # (the first samples are the silence in front of the tube's delay: zero in both)
        assert (plain != 0).sum() > 10 and (interactive[plain != 0] != plain[plain != 0]).all()
        # divided by an f0 of a hundred hertz and more: much smaller
        assert np.abs(interactive).max() < 0.1 * np.abs(plain).max()


@pytest.mark.skipif(oracle.ref_binary() is None, reason="oracle/_ref is not built here")
@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_the_reference_gives_the_fixtures_bytes_again(fixture, float_class):
    plan = model5_plan(device=capi.DEVICE_NONE, float_class=float_class)
    rate = plan.info.internal_rate_hz
    for n_steps in (0, 5, cases.PLAIN[1], cases.N + 1):
        frames = cases.frames_of(plan, n_steps)
        got, _ = oracle.ref_synthesize(frames, cases.MODEL[float_class], cases.RATE, rate, oracle.VOICE5_MALE, poll=cases.POLL)
        assert got.tobytes() == fixture[cases.name(float_class, n_steps)].tobytes(), n_steps
    frames = cases.frames_of(plan, cases.PLAIN[1])
    got, _ = oracle.ref_synthesize(frames, cases.MODEL[float_class], cases.RATE, rate, oracle.VOICE5_MALE)
    assert got.tobytes() == fixture[cases.name(float_class, cases.PLAIN[1], plain=True)].tobytes()
