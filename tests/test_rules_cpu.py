"""gvtm_rules_apply_host against the reference's generateEventList() (tests/golden/rules_golden.npz, made by
tests/golden/make_rules_golden.py from the cases of rules_cases.py): events as integers, rule data, onsets and statuses bit
for bit, the reference's two exceptions as statuses 1 and 2, the frame counts of the generated lists, and the two record
layouts of the new section of include/gama_vtm.h against a C compiler's."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rules_cases as cases
from gama_tts_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def rules(golden):
    made = {m: capi.Rules(cases.model_arrays(golden, m)) for m in cases.MODELS}
    yield made
    for r in made.values():
        r.close()


def golden_events(golden, name):
    """The reference's list as gvtm_event records (has_interp 0, interp 0: generateEventList() makes none)."""
    time, values = golden[name + "__time"], golden[name + "__values"]
    ev = np.zeros(time.shape[0], dtype=capi.EVENT_DTYPE)
    ev["time_ms"] = time
    ev["param"] = values[:, :16].view(np.float64)
    ev["special"] = values[:, 16:].view(np.float64)
    return ev


def golden_rule_data(golden, name):
    rows = golden[name + "__rule_data"]
    rd = np.zeros(rows.shape[0], dtype=capi.RULE_DATA_DTYPE)
    for i, field in enumerate(capi.RULE_DATA_DTYPE.names):
        rd[field] = rows[:, i]
    return rd


def as_bits(records):
    return np.ascontiguousarray(records).view(np.uint8)


ENTRIES = [str(n) for n in np.load(cases.GOLDEN)["names"]]


def test_the_case_table_reaches_every_status_and_every_model(golden):
    statuses = {int(golden[n + "__status"]) for n in ENTRIES}
    assert statuses == {0, 1, 2, 3, 4}
    assert {int(golden[n + "__model"]) for n in ENTRIES} == {0, 1}
    assert {int(golden[n + "__cp"]) for n in ENTRIES} == {1, 2, 3, 4}
    assert golden["sentence.0__time"].shape[0] > 240 and golden["sentence.0__postures"].shape[0] >= 50
    assert {e.split(".")[0] for e in ENTRIES} == set(cases.CASES)


@pytest.mark.parametrize("name", ENTRIES)
def test_host_rule_is_the_references_list(golden, rules, name):
    r = rules[cases.MODELS[int(golden[name + "__model"])]]
    postures = capi.postures_from_table(cases.posture_records(golden, name))
    cp = int(golden[name + "__cp"])
    events, rule_data, onsets, status = r.apply_host(cp, postures)
    assert status == cases.expected_status(golden, name)
    want = golden_events(golden, name)
    assert events.shape == want.shape and np.array_equal(as_bits(events), as_bits(want))
    want_rules = golden_rule_data(golden, name)
    assert rule_data.shape == want_rules.shape and np.array_equal(as_bits(rule_data), as_bits(want_rules))
    assert r.event_count(cp, postures) == (want.shape[0], status)
    if status == 0:
        assert np.array_equal(onsets.view(np.uint64), golden[name + "__onsets"].view(np.uint64))
        assert events.shape[0] >= 2 and (np.diff(events["time_ms"]) > 0).all() and (events["time_ms"] % cp == 0).all()
        # the debug flag marks the rule boundaries and marks: those events exist in our list at the same places
        assert np.array_equal(events["time_ms"][golden[name + "__flag"] != 0], golden[name + "__time"][golden[name + "__flag"] != 0])
        config = capi.TrackConfig(control_period_ms=cp, macro_intonation=0, micro_intonation=1, intonation_drift=0, smooth_intonation=1,
                                  initial_pitch=0.0, mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)
        assert capi.tracks_frame_count(config, events) == capi.tracks_frame_count(config, want) > 0


def test_capacities(golden, rules):
    r = rules["0_male"]
    postures = capi.postures_from_table(cases.posture_records(golden, "hello.0"))
    n, status = r.event_count(4, postures)
    assert status == 0 and n == golden["hello.0__time"].shape[0]
    with pytest.raises(capi.GvtmError) as e:
        r.apply_host(4, postures, capacity=n - 1)
    assert e.value.status == 1 and "does not fit capacity" in str(e.value)
    events, rule_data, _, status = r.apply_host(4, postures, capacity=n + 3, rule_capacity=2)
    assert status == 0 and events.shape[0] == n and rule_data.shape[0] == 2
    assert np.array_equal(as_bits(rule_data), as_bits(golden_rule_data(golden, "hello.0")[:2]))
    for cp in (0, 5):
        with pytest.raises(capi.GvtmError):
            r.event_count(cp, postures)


def test_device_entry_without_a_device_is_refused(golden, rules):
    lib = capi.load_library()
    rc = lib.gvtm_generate_events_device(rules["0_male"]._h, 4, 8, 8, 1, 8, 1, 8, None, 0, None, None, None, None)
    assert rc == 2 and b"GVTM_DEVICE_NONE" in lib.gvtm_last_error()


def test_record_layouts_are_the_c_structs(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = {"gvtm_posture": capi.POSTURE_DTYPE, "gvtm_rule_data": capi.RULE_DATA_DTYPE}
    lines = ["#include <stdio.h>", '#include "gama_vtm.h"', "int main(void) {"]
    for name, dtype in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f) for f in dtype.names]
    counts = capi.RulesModel._COUNTS + tuple(n for n, _ in capi.RulesModel._ARRAYS)
    lines.append('printf("gvtm_rules_model %zu\\n", sizeof(gvtm_rules_model));')
    lines += ['printf("gvtm_rules_model.%s %%zu %%zu\\n", offsetof(gvtm_rules_model, %s), sizeof(((gvtm_rules_model*)0)->%s));' % (f, f, f) for f in counts]
    lines += ["return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    seen = dict((line.split()[0], [int(x) for x in line.split()[1:]]) for line in
                subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, dtype in structs.items():
        assert seen[name] == [dtype.itemsize]
        for f in dtype.names:
            assert seen["%s.%s" % (name, f)] == [dtype.fields[f][1], dtype.fields[f][0].itemsize], (name, f)
    assert seen["gvtm_rules_model"] == [ctypes.sizeof(capi.RulesModel)]
    for f in counts:
        field = getattr(capi.RulesModel, f)
        assert seen["gvtm_rules_model." + f] == [field.offset, field.size], f
    assert [structs[n].itemsize for n in sorted(structs)] == [24, 48]
