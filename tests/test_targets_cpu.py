"""Synthesis from parameter targets on the host (gvtm_targets_filter_length, gvtm_targets_output_count / _capacity,
gvtm_targets_apply_host) and the device entry's refusals on design-only plans.  No GPU needed.

Pins: the filter length against the float formula (a float product rounded half away from zero), on the plans of the
modification cases and at 20 050 Hz, where the product is 1002.5; the host entry bit for bit against the literal
restatement of tests/targets_cases.py (a real ring of N np.float32, Python floats for the sum) on the case table and on
seeded random cases, refused ones among them, and against tests/golden/targets_golden.npz (the reference's
MovingAverageFilter<float> under the loop of the rule as the header states it); the sample counts by steps against the
oracle's at one step per frame; where oracle/_ref is built, the oracle at one step per frame against the compiled reference
on the host rule's frames; every refusal of the device entry as far as a design-only plan lets it go."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import modification_cases
import oracle
import targets_cases as cases
import targets_io
from voice_cases import configs, male_plan, model5_plan

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
ENTRIES = ("gvtm_targets_filter_length", "gvtm_targets_output_count", "gvtm_targets_output_capacity", "gvtm_targets_apply_host",
           "gvtm_synthesize_targets_device")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "targets_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def plans():
    return {key: cases.make_plan(key, capi.DEVICE_NONE) for key in cases.PLANS}


@pytest.fixture(scope="module")
def restated():
    """The literal restatement on every case of the table, once."""
    out = {}
    for name in cases.CASES:
        key, n_steps, lists = cases.case(name)
        out[name] = cases.apply_rule(lists, n_steps, cases.filter_length(cases.PLANS[key].rate))
    return out


def test_names_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ENTRIES:
        assert name + "(" in header and name in exported and name in capi.PROTOTYPES, name


# ---- 1. the filter length ----

def test_filter_length_is_the_float_formula(plans):
    for key in modification_cases.PLANS:
        assert (plans[key].info.internal_rate_hz, plans[key].info.control_steps) == tuple(cases.PLANS[key]), key
        assert plans[key].targets_filter_length() == cases.filter_length(cases.PLANS[key].rate), key
    assert plans["male"].targets_filter_length() == 1002 and plans["male5"].targets_filter_length() == 3021
    # 20 050 Hz: the product is 1002.5 exactly; half away from zero, where numpy's and Python's round say 1002
    half = plans["half50"]
    assert half.info.internal_rate_hz == 20050.0 == cases.PLANS["half50"].rate
    assert np.float32(20050.0) * np.float32(50.0e-3) == np.float32(1002.5)
    assert half.targets_filter_length() == cases.filter_length(20050.0) == 1003
    assert int(np.round(np.float32(20050.0) * np.float32(50.0e-3))) == 1002 == round(1002.5)
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
    for v in range(plan.n_voices):
        assert plan.targets_filter_length(v) == cases.filter_length(plan.voice_info(v).internal_rate_hz), v


def test_filter_length_bad_calls(plans):
    lib = g.load_library()
    assert lib.gvtm_targets_filter_length(None, 0) == -1
    assert lib.gvtm_targets_filter_length(plans["male"]._h, 1) == -1 and lib.gvtm_targets_filter_length(plans["male"]._h, -1) == -1
    with pytest.raises(g.GvtmError):
        plans["male"].targets_filter_length(3)


# ---- 2. the host rule against the literal restatement ----

def test_cases_cover_what_they_claim(restated):
    assert {cases.CASES[n][0] for n in cases.CASES} == set(cases.RULE_PLANS)
    n = cases.filter_length(cases.PLANS["male"].rate)
    assert {cases.CASES[name][1] for name in cases.CASES if name.startswith("male__")} >= {0, 1, n - 1, n, n + 1, 2 * n + 7}
    _, n_steps, lists = cases.case("male__2n7")
    steps = [l[0] for l in lists]
    assert steps[0] == [] and steps[1][0] > 0 and steps[2] == [0]                              # empty, starts late, only step 0
    assert 0 < steps[3][1] - steps[3][0] < n and steps[4][1] - steps[4][0] == n                # less than N apart, exactly N apart
    assert len({s // 4 for s in steps[5][:3]}) == 1 and len(steps[5][:3]) == 3                 # three changes in one block of four
    assert steps[6] == [n_steps - 1, n_steps, n_steps + 1]
    assert len(steps[7]) > 64 and set(np.diff(steps[7])) == {2, 3}
    # the wide values: six decades apart in one window, and the sequential sum is not the exactly rounded window mean
    mags = np.abs(lists[cases.WIDE][1].astype(np.float64))
    assert mags.min() < 1e-5 and mags.max() > 1e3
    seq = restated["male__2n7"][0][:, cases.WIDE]
    exact = cases.exact_mean_column(*lists[cases.WIDE], n_steps, n)
    assert (seq.view(np.uint32) != exact.view(np.uint32)).any()
    # ... while a list of two tame values is the exactly rounded mean all the way (the restatement of the mean is right)
    tame = cases.exact_mean_column(*lists[9], n_steps, n)
    assert restated["male__2n7"][0][:, 9].tobytes() == tame.tobytes()
    # a parameter without a point at step 0 is held at 0 until its first point; a point at step S never acts
    assert not restated["male__2n7"][0][: steps[1][0], 1].any() and restated["male__2n7"][0][steps[1][0], 1] != 0
    assert not restated["male__2n7"][0][:, 12].any()


def test_host_entry_equals_the_restatement_on_every_case(plans, restated):
    for name in cases.CASES:
        key, n_steps, lists = cases.case(name)
        out, status = capi.targets_apply_host(plans[key], lists, n_steps)
        want, want_status = restated[name]
        assert status == want_status == 0, name
        assert out.shape == (n_steps, 16) and out.tobytes() == want.tobytes(), name


def call_host(plan, lists, n_steps, offsets=None, guard=7.0):
    """The host entry with a doctored offset table -> (frames_out that started out as `guard`, status)."""
    table, steps, values = capi.pack_targets(lists)
    if offsets is not None:
        table = np.asarray(offsets, dtype=np.int64)
    out = np.full((max(n_steps, 1) if n_steps < 10 ** 6 else 1, 16), guard, dtype=np.float32)
    status = ctypes.c_int32(-5)
    rc = plan._lib.gvtm_targets_apply_host(plan._h, 0, capi._ptr(table), capi._ptr(steps), capi._ptr(values), int(n_steps), capi._ptr(out), ctypes.byref(status))
    assert rc == OK
    return out, int(status.value)


def test_host_entry_equals_the_restatement_on_random_cases(plans):
    statuses = []
    for seed in range(200):
        key, n_steps, lists, offsets = cases.random_case(seed)
        want_status = cases.status_of(n_steps, lists, offsets)
        out, status = call_host(plans[key], lists, n_steps, offsets)
        assert status == want_status, seed
        if status == 0:
            want, _ = cases.apply_rule(lists, n_steps, cases.filter_length(cases.PLANS[key].rate))
            assert out[:n_steps].tobytes() == want.tobytes(), seed
        else:
            assert (out == 7.0).all(), seed  # a refused utterance leaves its output alone
        statuses.append(status)
    assert set(statuses) == {0, 1, 2, 3, 4}  # (random_case still makes every kind of refused utterance)
    assert 30 <= sum(1 for s in statuses if s) <= 70  # about one in four


def test_statuses_and_their_order(plans):
    plan = plans["male"]
    good = [([0, 3], np.float32([1.0, 2.0]))] + [([], np.float32([]))] * 15
    with_list = lambda p, steps, values: good[:p] + [(steps, np.float32(values))] + good[p + 1:]  # noqa: E731
    table = [0, 2] + [2] * 15
    for n_steps, lists, offsets, want in [
            (5, good, None, 0), (0, good, None, 0), (-1, good, None, 1), (cases.STEP_LIMIT, good, None, 1),
            (-1, good, [0, 2, 1] + [2] * 14, 1),                                    # 1 before 2
            (5, good, [0, 2, 1] + [2] * 14, 2), (5, good, [-1] + table[1:], 2),
            (5, with_list(3, [1], [np.nan]), [0, 2, 3, 2] + [3] * 13, 2),           # 2 before 3
            (5, with_list(3, [1], [np.nan]), None, 3), (5, with_list(15, [1], [np.inf]), None, 3), (5, with_list(1, [1], [-np.inf]), None, 3),
            (5, with_list(1, [4, 4], [1.0, 2.0])[:15] + [([2], np.float32([np.nan]))], None, 3),   # 3 before 4: a later list's value
            (5, with_list(1, [-1], [1.0]), None, 4), (5, with_list(1, [4, 4], [1.0, 2.0]), None, 4), (5, with_list(7, [4, 9, 8], [1.0, 2.0, 3.0]), None, 4),
            (5, with_list(7, [2 ** 31 - 1], [3.0e38]), None, 0)]:
        assert cases.status_of(n_steps, lists, offsets) == want
        out, status = call_host(plan, lists, n_steps, offsets, guard=-3.25)
        assert status == want, (n_steps, offsets)
        if want:
            assert (out == -3.25).all()


def test_host_entry_bad_calls(plans):
    lib, plan, p = g.load_library(), plans["male"], capi._ptr
    offsets, steps, values = capi.pack_targets([([0], [1.0])] + [([], [])] * 15)
    out = np.zeros((4, 16), np.float32)
    status = ctypes.c_int32(-5)

    def call(plan_h=plan._h, voice=0, offsets=offsets, steps=steps, values=values, n_steps=4, out=out, status=status):
        return lib.gvtm_targets_apply_host(plan_h, voice, p(offsets), p(steps), p(values), n_steps, p(out), ctypes.byref(status) if status is not None else None)

    assert call() == OK and status.value == 0
    for bad in (dict(plan_h=None), dict(status=None), dict(offsets=None), dict(out=None), dict(steps=None), dict(values=None), dict(voice=1), dict(voice=-1)):
        status.value = -5
        assert call(**bad) == INVALID_ARGUMENT and status.value == -5, bad
        assert lib.gvtm_last_error()
    # nothing to read or write: null tables are fine
    assert call(offsets=np.zeros(17, np.int64), steps=None, values=None) == OK and status.value == 0
    assert call(out=None, n_steps=0) == OK and status.value == 0


# ---- 3. the fixture from the reference's filter ----

def test_host_entry_equals_the_fixture_on_every_case(fixture, plans):
    assert len(cases.CASES) >= 15
    full = 0
    for name in cases.CASES:
        key, n_steps, lists = cases.case(name)
        out, status = capi.targets_apply_host(plans[key], lists, n_steps)
        assert status == 0 and cases.check_frames(fixture, name, out) is None, name
        full += (name + "__frames") in fixture
    assert full >= 5
    # the check can fail: one bit of one value
    _, n_steps, lists = cases.case("male__s200")
    out, _ = capi.targets_apply_host(plans["male"], lists, n_steps)
    out.view(np.uint32)[150, cases.WIDE] ^= 1
    assert cases.check_frames(fixture, "male__s200", out) is not None


# ---- 4. the output count ----

@pytest.mark.parametrize("rate,layout", [(44100.0, 0), (16000.0, 0), (22050.0, 1)], ids=["up", "down-16k", "down-layout1-22k"])
def test_output_count_by_steps_equals_the_oracle_at_one_step_per_frame(rate, layout):
    plan = male_plan(rate=rate, layout=layout, device=capi.DEVICE_NONE)
    cfg = oracle.male_config(rate, 1, layout=layout)
    internal = plan.info.internal_rate_hz
    assert oracle.derive(cfg, internal).control_steps == 1 and (internal > rate) == (rate != 44100.0)
    for n_steps in (0, 1, 100, 1002, 5000):
        assert plan.targets_output_count(n_steps) == oracle.output_count(cfg, n_steps, control_rate=internal), n_steps
    # by steps, whatever the plan's control rate: the frames' counts are the steps' counts
    assert plan.targets_output_count(7 * plan.info.control_steps) == plan.output_count(7)
    assert plan.targets_output_capacity(7 * plan.info.control_steps) == plan.output_capacity(7)
    other = male_plan(rate=rate, layout=layout, crate=500.0, device=capi.DEVICE_NONE)
    if other.info.internal_rate_hz == internal:
        assert other.targets_output_count(1002) == plan.targets_output_count(1002)
    assert max(plan.targets_output_count(s) for s in range(0, 300, 7)) <= plan.targets_output_capacity(300)
    lib = g.load_library()
    assert lib.gvtm_targets_output_count(None, 5) == lib.gvtm_targets_output_capacity(None, 5) == ctypes.c_size_t(-1).value


# ---- 5. the oracle at one step per frame against the compiled reference ----

@pytest.mark.parametrize("name", ["male__np1", "male__s200"])
def test_oracle_at_one_step_per_frame_equals_the_reference(plans, name, tmp_path):
    if oracle.ref_binary() is None:
        pytest.skip("oracle/_ref is not built here")
    # (spoken lists: the case table's values are no parameters a voice can have)
    n_steps = cases.CASES[name][1]
    frames, status = capi.targets_apply_host(plans["male"], cases.spoken_lists(n_steps, 5, wide=True), n_steps)
    assert status == 0
    rate = plans["male"].info.internal_rate_hz
    for model, float_model in (("0", 0), ("1", 1)):
        ref, _ = oracle.ref_synthesize(frames, model=model, control_rate=rate, tmpdir=str(tmp_path))
        got = oracle.synthesize(oracle.male_config(44100.0, 1, float_model=float_model), frames, control_rate=rate)
        assert got.size == ref.size and got.tobytes() == ref.tobytes(), (name, model)


# ---- 6. the device entry's refusals ----

device_entry = functools.partial(targets_io.device_entry, entry_name="gvtm_synthesize_targets_device", voices=False)


@pytest.mark.parametrize("kind", ["one-voice", "two-voices", "model5", "model5-float"])
def test_device_entry_checks_its_arguments_and_then_wants_a_device(kind):
    if kind == "two-voices":
        plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    elif kind == "one-voice":
        plan = male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    else:
        plan = model5_plan("male", float_class=kind == "model5-float", device=capi.DEVICE_NONE)
    lib = plan._lib
    after_checks = NO_DEVICE if kind == "one-voice" else UNSUPPORTED
    assert device_entry(plan) == after_checks
    for null in ("offsets", "steps", "values", "audio"):
        assert device_entry(plan, null=null) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error(), null
    # without list ids every utterance has 16 lists of its own
    assert device_entry(plan, n_lists=31) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=3, ids=True) == after_checks  # with ids lists may be shared
    assert device_entry(plan, max_steps=2 ** 31) == INVALID_ARGUMENT and b"step counter" in lib.gvtm_last_error()
    assert device_entry(plan, stride=plan.targets_output_capacity(8) - 1) == INVALID_ARGUMENT and b"audio_stride" in lib.gvtm_last_error()
    assert device_entry(plan, stride=plan.targets_output_capacity(8)) == after_checks
    # the order: a null table before the lists' number, that before the stride, the stride before the plan's kind
    assert device_entry(plan, null="values", n_lists=31) == INVALID_ARGUMENT and b"null" in lib.gvtm_last_error()
    assert device_entry(plan, n_lists=31, stride=1) == INVALID_ARGUMENT and b"n_lists" in lib.gvtm_last_error()
    # batch == 0: nothing is looked at but the plan -- and a design-only plan has no device
    assert device_entry(plan, batch=0, null="offsets", stride=0) == after_checks


def test_a_null_plan_is_refused():
    lib = g.load_library()
    args = [None] * 15
    for i in (2, 7, 8, 10):
        args[i] = 0
    assert lib.gvtm_synthesize_targets_device(*args) == INVALID_ARGUMENT
    assert lib.gvtm_targets_apply_host(None, 0, None, None, None, 0, None, None) == INVALID_ARGUMENT
