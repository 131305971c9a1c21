"""Parameter-modification gestures on the host (gvtm_modification_filter_length, gvtm_modification_apply_host) and the device
entries' argument checks on design-only plans.  No GPU needed.

Pins: the filter length against the float formula (a float product rounded half away from zero) on the five voices at
SectionDelay 1 to 3, the five model 5 voices in both classes and a sweep of tract lengths that crosses rates whose product
ends in .5; the host entry against tests/golden/modification_golden.npz (the reference's MovingAverageFilter<float> under
the loop of the rule as the header states it) on every case, and against the literal restatement of
tests/modification_cases.py on seeded random cases, refused ones among them; every status and their order; that a refused
utterance leaves its output alone; the bad calls; the device entries' refusals in the header's order as far as a design-only
plan lets them go; the names in the header, the library and the binding; and that examples/synthesize_modified.c compiles
as strict C99 and runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import modification_cases as cases
from voice_cases import configs, male_plan, model5_plan
from voice_files import VOICES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID_ARGUMENT, NO_DEVICE = 0, 1, 2
ENTRIES = ("gvtm_modification_filter_length", "gvtm_modification_apply_host", "gvtm_apply_modifications_device", "gvtm_synthesize_modified_device")
ADD, MULTIPLY, R3, VELUM = cases.ADD, cases.MULTIPLY, cases.R3, cases.VELUM


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "modification_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def plans():
    return {key: cases.make_plan(key, capi.DEVICE_NONE) for key in cases.PLANS}


def test_names_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ENTRIES:
        assert name + "(" in header and name in exported and name in capi.PROTOTYPES, name
    for text in ("#define GVTM_MODIFICATION_ADD 0", "#define GVTM_MODIFICATION_MULTIPLY 1", "#define GVTM_MAX_GESTURES 64"):
        assert text in header
    assert (capi.MODIFICATION_ADD, capi.MODIFICATION_MULTIPLY, capi.MAX_GESTURES) == (0, 1, 64) == (ADD, MULTIPLY, cases.MAX_GESTURES)


# ---- the case table ----

def test_cases_cover_what_they_claim(fixture):
    assert set(n.split("__")[0] for n in cases.CASES) == set(cases.PLANS)
    facts = {n: (cases.PLANS[c[0]].cs, cases.filter_length(cases.PLANS[c[0]].rate), c[1], c[3]) for n, c in cases.CASES.items()}
    steps_of = lambda n: [s for _, _, steps, _ in facts[n][3] for s in steps]  # noqa: E731
    assert {f[2] for f in facts.values()} >= {2, 3, 40}
    assert any(0 in steps_of(n) for n in facts)                                              # a point at step 0
    assert any(s % cs for n, (cs, _, _, _) in facts.items() for s in steps_of(n))            # ... in the middle of a frame
    assert any(sum(1 for s in steps if s // cs == steps[0] // cs) >= 3 for cs, _, _, gs in facts.values() for _, _, steps, _ in gs if steps)
    assert any((f - 1) * cs - 1 in steps for cs, _, f, gs in facts.values() for _, _, steps, _ in gs)   # the last step
    beyond = [(n, [all(s >= (f - 1) * cs for s in steps) for _, _, steps, _ in gs if steps]) for n, (cs, _, f, gs) in facts.items()]
    assert any(any(b) and not all(b) for _, b in beyond)                                      # a gesture all beyond the end, next to one that acts
    assert any(any(s >= (f - 1) * cs for s in steps) and steps[0] < (f - 1) * cs for cs, _, f, gs in facts.values() for _, _, steps, _ in gs if steps)
    assert any(not steps for _, _, _, gs in facts.values() for _, _, steps, _ in gs)           # a gesture without points
    # a value held for more than 3 N steps; values that change every N / 2 steps all the way
    assert any(len(steps) == 1 and (f - 1) * cs - steps[0] > 3 * n for cs, n, f, gs in facts.values() for _, _, steps, _ in gs)
    assert any(len(steps) > 4 and max(np.diff(steps)) <= n // 2 and (f - 1) * cs - steps[-1] <= n // 2
               for cs, n, f, gs in facts.values() for _, _, steps, _ in gs)
    values_of = lambda n, op: [float(v) for _, o, _, vs in facts[n][3] if o == op for v in vs]  # noqa: E731
    assert any(0.0 in values_of(n, MULTIPLY) and min(values_of(n, MULTIPLY)) < 0.0 for n in facts)
    assert any(np.signbit(v) and v == 0.0 for n in facts for v in values_of(n, MULTIPLY))
    # the sign of zero reaches the bytes
    columns = fixture["male__mul_zero_neg__columns"]
    assert (np.signbit(columns) & (columns == 0.0)).any() and (~np.signbit(columns) & (columns == 0.0)).any()
    # two gestures on one parameter, the later starting later: the frames in between keep the earlier one's values
    _, base, gs = cases.case("male__same_param")
    cs, n = facts["male__same_param"][:2]
    assert gs[0][0] == gs[2][0] == R3 and gs[2][2][0] > gs[0][2][0]
    alone, _ = cases.apply_rule(base, gs[:1], cs, n)
    both = fixture["male__same_param__columns"][:, cases.modified_parameters(gs).index(R3)]
    second = -(-gs[2][2][0] // cs) + 1
    assert both[:second].tobytes() == alone[:second, R3].tobytes() and (both[second:] != alone[second:, R3]).all()
    assert any(len({p for p, _, _, _ in gs}) >= 3 for _, _, _, gs in facts.values())          # gestures on different parameters
    assert any(len(gs) == 64 for _, _, _, gs in facts.values())
    # wide values: 1e-6 to 1e4 in magnitude, both signs, and in every such case frames where the sequential sum is not the
    # exactly rounded mean of the window
    wide = [n for n in facts if "wide" in n]
    assert len(wide) >= 5
    for name in wide:
        cs, n, _, gs = facts[name]
        _, base, _ = cases.case(name)
        mags = np.abs(np.concatenate([np.asarray(v, dtype=np.float64) for _, _, _, v in gs]))
        assert mags.min() < 1e-5 and mags.max() > 1e3 and mags.min() >= 1e-6 and mags.max() <= 1e4, name
        assert any(float(v) < 0 for _, _, _, vs in gs for v in vs) and any(float(v) > 0 for _, _, _, vs in gs for v in vs)
        differ = 0
        for gesture in gs:
            seq, _ = cases.apply_rule(base, [gesture], cs, n)
            exact = cases.exact_mean_column(base, gesture, cs, n)
            differ += sum(1 for k, v in exact.items() if np.float32(v).tobytes() != seq[k, gesture[0]].tobytes())
        assert differ > 0, name
    # the rate at which rounding half to even gives another N than the reference's std::round
    half = cases.PLANS["half"].rate
    assert half == 22125.0 and cases.filter_length(half) == 443 and int(np.round(half * 20.0e-3)) == 442 == round(half * 20.0e-3)


def test_restatement_equals_the_fixture_on_the_male_cases(fixture):
    """The numpy restatement is itself held against the reference (the cheaper plan's cases: it walks every step)."""
    for name in cases.CASES:
        key, base, gestures = cases.case(name)
        if key == "male":
            out, status = cases.apply_rule(base, gestures, cases.PLANS[key].cs, cases.filter_length(cases.PLANS[key].rate))
            assert status == 0 and cases.check_frames(fixture, name, out) is None, name


# ---- the filter length ----

def test_filter_length_is_the_float_formula(plans):
    for key, plan in plans.items():
        assert (plan.info.internal_rate_hz, plan.info.control_steps) == tuple(cases.PLANS[key]), key
        assert plan.modification_filter_length() == cases.filter_length(cases.PLANS[key].rate), key
    assert plans["half"].modification_filter_length() == 443 and plans["male5"].modification_filter_length() == 1208
    for delay in (1, 2, 3):
        plan = g.VoicesPlan(configs(delay=delay, precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
        for v in range(len(VOICES)):
            assert plan.modification_filter_length(v) == cases.filter_length(plan.voice_info(v).internal_rate_hz), (delay, v)
    for float_class in (False, True):
        for voice in VOICES:
            plan = model5_plan(voice, float_class=float_class, device=capi.DEVICE_NONE)
            assert plan.modification_filter_length() == cases.filter_length(plan.info.internal_rate_hz) > 1000, (voice, float_class)
    seen_half = 0
    for length in np.concatenate([np.linspace(12.0, 20.0, 81), [15.846, 15.6343, 17.53]]):
        plan = male_plan({"vocal_tract_length": float(length), "vocal_tract_length_offset": 0.0}, device=capi.DEVICE_NONE)
        rate = plan.info.internal_rate_hz
        assert plan.modification_filter_length() == cases.filter_length(rate), length
        seen_half += rate % 50 == 25
    assert seen_half >= 2  # (22 125 and 22 425 Hz)


def test_filter_length_bad_calls(plans):
    lib = g.load_library()
    assert lib.gvtm_modification_filter_length(None, 0) == -1
    assert lib.gvtm_modification_filter_length(plans["male"]._h, 1) == -1 and lib.gvtm_modification_filter_length(plans["male"]._h, -1) == -1
    with pytest.raises(g.GvtmError):
        plans["male"].modification_filter_length(3)


# ---- the host entry ----

def test_host_entry_equals_the_fixture_on_every_case(fixture, plans):
    assert len(cases.CASES) >= 30
    for name in cases.CASES:
        key, base, gestures = cases.case(name)
        assert tuple(fixture[name + "__plan"]) == (cases.PLANS[key].rate, float(cases.PLANS[key].cs)), name
        out, status = capi.modification_apply_host(plans[key], base, gestures)
        assert status == 0, name
        assert cases.check_frames(fixture, name, out) is None


def test_host_entry_on_a_voice_of_a_plan_of_several(fixture):
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    for voice, key in enumerate(("male", "female")):
        _, base, gestures = cases.case(key + "__half_n")
        out, status = capi.modification_apply_host(plan, base, gestures, voice=voice)
        assert status == 0 and cases.check_frames(fixture, key + "__half_n", out) is None


def test_host_entry_equals_the_restatement_on_random_cases(plans):
    statuses = set()
    for seed in range(60):
        key, base, gestures = cases.random_case(seed)
        want, want_status = cases.apply_rule(base, gestures, cases.PLANS[key].cs, cases.filter_length(cases.PLANS[key].rate))
        guard = np.full((max(base.shape[0], 1), 16), 7.0, dtype=np.float32)
        out, status = capi.modification_apply_host(plans[key], base, gestures, frames_out=guard)
        assert status == want_status, seed
        assert out[: base.shape[0]].tobytes() == (want if status == 0 else np.full_like(base, 7.0)).tobytes(), seed
        statuses.add(status)
    assert statuses == {0, 1, 2, 3, 4}  # (random_case still makes every kind of refused utterance)


def point(step, value=0.5):
    return ([step], np.float32([value]))


GOOD = (R3, ADD) + point(3)
STATUSES = [  # (frames, gestures, status)
    (2, [], 0),
    (2, [GOOD], 0),
    (1, [GOOD], 1),
    (0, [], 1),
    (1, [GOOD] * 65, 1),                                             # 1 before 2
    (5, [GOOD] * 64, 0),
    (5, [GOOD] * 65, 2),
    (5, [(16, ADD) + point(3)] * 65, 2),                             # 2 before 3
    (5, [(16, ADD) + point(3)], 3),
    (5, [(-1, ADD) + point(3)], 3),
    (5, [(R3, 2) + point(3)], 3),
    (5, [(R3, -1) + point(3)], 3),
    (5, [(R3, ADD) + point(3, np.inf)], 3),
    (5, [(R3, ADD) + point(3, -np.inf)], 3),
    (5, [(R3, MULTIPLY) + point(3, np.nan)], 3),
    (5, [(R3, ADD, [5, 4], np.float32([1, 2])), (VELUM, 7) + point(3)], 3),           # 3 before 4: a later gesture's operation
    (5, [(R3, ADD, [-1], np.float32([1])), GOOD, (VELUM, ADD, [1, 2], np.float32([1, np.nan]))], 3),  # ... and a later point's value
    (5, [(R3, ADD, [-1], np.float32([1]))], 4),
    (5, [GOOD, (R3, ADD, [4, 4], np.float32([1, 2]))], 4),
    (5, [GOOD, (R3, ADD, [4, 9, 8], np.float32([1, 2, 3]))], 4),
    (5, [(R3, ADD, [7], np.float32([1])), (R3, ADD, [3], np.float32([1]))], 0),      # steps increase within a gesture, not across
    (5, [(R3, ADD, [2 ** 31 - 1], np.float32([3.0e38]))], 0),
]


@pytest.mark.parametrize("n_frames,gestures,want", STATUSES, ids=[str(i) for i in range(len(STATUSES))])
def test_statuses_their_order_and_the_untouched_output(plans, n_frames, gestures, want):
    base = cases.base_frames(n_frames, 77)
    assert cases.status_of(n_frames, gestures) == want
    guard = np.full((max(n_frames, 1), 16), -3.25, dtype=np.float32)
    out, status = capi.modification_apply_host(plans["male"], base, gestures, frames_out=guard)
    assert status == want
    if want:
        assert (out == -3.25).all()
    else:
        assert out[:n_frames].tobytes() == cases.apply_rule(base, gestures, 80, 401)[0].tobytes()


def test_host_entry_bad_calls(plans):
    lib, plan = g.load_library(), plans["male"]
    frames, out = np.zeros((4, 16), np.float32), np.zeros((4, 16), np.float32)
    table, offsets = np.array([[R3, ADD]], np.int32), np.array([0, 1], np.int64)
    steps, values = np.array([3], np.int32), np.array([1.0], np.float32)
    status = ctypes.c_int32(-5)
    p = capi._ptr

    def call(plan_h=plan._h, voice=0, frames=frames, n_frames=4, table=table, offsets=offsets, n=1, steps=steps, values=values, out=out, status=status):
        return lib.gvtm_modification_apply_host(plan_h, voice, p(frames), n_frames, p(table), p(offsets), n, p(steps), p(values), p(out),
                                                ctypes.byref(status) if status is not None else None)

    assert call() == OK and status.value == 0
    for bad in (dict(plan_h=None), dict(status=None), dict(out=None), dict(frames=None), dict(table=None), dict(offsets=None), dict(steps=None),
                dict(values=None), dict(voice=1), dict(voice=-1), dict(offsets=np.array([1, 0], np.int64)), dict(offsets=np.array([-1, 0], np.int64))):
        status.value = -5
        assert call(**bad) == INVALID_ARGUMENT and status.value == -5, bad
        assert lib.gvtm_last_error()
    # nothing to read: null tables are fine
    assert call(table=None, offsets=None, n=0, steps=None, values=None) == OK and status.value == 0
    assert call(offsets=np.array([5, 5], np.int64), steps=None, values=None) == OK and status.value == 0
    assert call(frames=None, n_frames=0) == OK and status.value == 1


# ---- the device entries on design-only plans ----

def device_entries(plan, batch=2, null=None, n_bases=2, base_ids=True, voice_ids=True, misaligned=None, stride=65536):
    """Status of the two device entries on a small (host-memory, never dereferenced) batch; null: an argument to leave out."""
    lib = plan._lib
    a = dict(base=np.zeros((2, 8, 16), np.float32), base_counts=np.array([8, 8], np.int32), gestures=np.zeros((2, 2), np.int32),
             gesture_offsets=np.array([0, 1, 2], np.int64), utt_gestures=np.array([0, 1, 2], np.int64), steps=np.zeros(2, np.int32),
             values=np.zeros(2, np.float32), params_out=np.zeros((2, 8, 16), np.float32), counts_out=np.zeros(2, np.int32), audio=np.zeros((2, 65536), np.float32))
    ptr = {k: (None if k == null else v.ctypes.data + (4 if k == misaligned else 0)) for k, v in a.items()}
    ids = np.zeros(2, np.int32).ctypes.data if base_ids else None
    voices = np.zeros(2, np.int32).ctypes.data if voice_ids else None
    common = (plan._h, ptr["base"], ptr["base_counts"], n_bases, ids, ptr["gestures"], ptr["gesture_offsets"], ptr["utt_gestures"], ptr["steps"],
              ptr["values"], voices, batch, 8)
    apply = lib.gvtm_apply_modifications_device(*common, ptr["params_out"], ptr["counts_out"], None, None)
    synth = lib.gvtm_synthesize_modified_device(*common, ptr["audio"], stride, None, None, None, None, None)
    return apply, synth


@pytest.mark.parametrize("kind", ["one-voice", "two-voices", "model5", "model5-float"])
def test_device_entries_check_their_arguments_and_then_want_a_device(kind):
    if kind == "two-voices":
        plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    elif kind == "one-voice":
        plan = male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    else:
        plan = model5_plan("male", float_class=kind == "model5-float", device=capi.DEVICE_NONE)
    assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)
    for null in ("base", "base_counts", "gestures", "gesture_offsets", "utt_gestures", "steps", "values"):
        assert device_entries(plan, null=null) == (INVALID_ARGUMENT, INVALID_ARGUMENT), null
    assert device_entries(plan, null="params_out") == (INVALID_ARGUMENT, NO_DEVICE)  # (the one-call entry has its own)
    assert device_entries(plan, null="counts_out") == (INVALID_ARGUMENT, NO_DEVICE)
    # without base ids every utterance has its own base
    assert device_entries(plan, base_ids=False) == (NO_DEVICE, NO_DEVICE)
    assert device_entries(plan, base_ids=False, n_bases=1) == (INVALID_ARGUMENT, INVALID_ARGUMENT)
    assert device_entries(plan, n_bases=1) == (NO_DEVICE, NO_DEVICE)  # with ids bases may be shared
    # without voice ids the plan has one voice
    want = INVALID_ARGUMENT if kind == "two-voices" else NO_DEVICE
    assert device_entries(plan, voice_ids=False) == (want, want)
    assert device_entries(plan, misaligned="base") == (INVALID_ARGUMENT, INVALID_ARGUMENT)
    assert device_entries(plan, misaligned="params_out") == (INVALID_ARGUMENT, NO_DEVICE)
    # the order: a null table before the missing base ids, those before the missing voice ids, those before the alignment
    lib = plan._lib
    assert device_entries(plan, null="values", base_ids=False, n_bases=1) == (INVALID_ARGUMENT, INVALID_ARGUMENT) and b"null" in lib.gvtm_last_error()
    if kind == "two-voices":
        assert device_entries(plan, base_ids=False, n_bases=1, voice_ids=False) == (INVALID_ARGUMENT, INVALID_ARGUMENT) and b"n_bases" in lib.gvtm_last_error()
        assert device_entries(plan, voice_ids=False, misaligned="base") == (INVALID_ARGUMENT, INVALID_ARGUMENT) and b"voice id" in lib.gvtm_last_error()
    # the one-call entry: then the audio buffer, then its stride, then the device
    assert device_entries(plan, null="audio") == (NO_DEVICE, INVALID_ARGUMENT) and b"audio" in lib.gvtm_last_error()
    assert device_entries(plan, stride=16) == (NO_DEVICE, INVALID_ARGUMENT) and b"audio_stride" in lib.gvtm_last_error()
    assert device_entries(plan, null="audio", misaligned="base")[1] == INVALID_ARGUMENT and b"aligned" in lib.gvtm_last_error()
    # batch == 0: nothing is looked at but the plan -- and a design-only plan has no device (as the neighbouring entries)
    assert device_entries(plan, batch=0, null="base") == (NO_DEVICE, NO_DEVICE)


def test_a_null_plan_is_refused():
    lib = g.load_library()
    none17, none20 = [None] * 17, [None] * 20
    for i in (3, 11, 12):
        none17[i] = none20[i] = 0
    none20[14] = 0
    assert lib.gvtm_apply_modifications_device(*none17) == INVALID_ARGUMENT
    assert lib.gvtm_synthesize_modified_device(*none20) == INVALID_ARGUMENT


def test_pack_gestures_tables():
    table, offsets, utt, steps, values = capi.pack_gestures([[(R3, ADD, [1, 2], [0.5, 1.5])], [], [(VELUM, MULTIPLY, [], []), (0, ADD, [7], [2.0])]])
    assert table.tolist() == [[R3, ADD], [VELUM, MULTIPLY], [0, ADD]] and table.dtype == np.int32
    assert offsets.tolist() == [0, 2, 2, 3] and utt.tolist() == [0, 1, 1, 3] and offsets.dtype == utt.dtype == np.int64
    assert steps.tolist() == [1, 2, 7] and steps.dtype == np.int32 and values.tolist() == [0.5, 1.5, 2.0] and values.dtype == np.float32
    empty = capi.pack_gestures([])
    assert empty[0].shape == (0, 2) and empty[1].tolist() == [0] and empty[2].tolist() == [0]


def test_example_compiles_as_c99_and_runs(tmp_path):
    exe = tmp_path / "synthesize_modified"
    lib_dir = os.path.dirname(capi.library_path())
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O2", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "synthesize_modified.c"), "-L" + lib_dir, "-lgama_vtm", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "the 20 ms filter holds 401 samples" in run.stdout
    assert "parameter 9: first modified frame 21:" in run.stdout and "last 99:" in run.stdout  # r3: from 80 ms on, to the end
    assert "parameter 3: first modified frame" in run.stdout
    assert "samples, peak" in run.stdout or "synthesis: no HIP device" in run.stdout  # (without a device it says so and exits 0)
