"""Rhythm and intonation-point placement on the host (gvtm_prosody_rhythm_host, gvtm_prosody_points_host,
gvtm_prosody_point_count) against the reference's EventList (tests/golden/prosody_golden.npz, every case of
prosody_cases.py): the tempi after applyRhythm(), the IntonationPoints and, under gvtm_intonation_apply_host, the list
applyIntonation() leaves, all bit for bit; the refusals; the entries in the header, the export map and the binding; the
vocoid table of the 0_male database."""
import os
import re

import numpy as np
import pytest

import prosody_cases as cases
import rules_cases
from gama_tts_amd import capi, control_model
from test_rules_cpu import as_bits, golden_rule_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ARTIC = "/root/reference/data/voice/english/0_male/artic.xml"
ENTRIES = [str(n) for n in np.load(cases.GOLDEN)["names"]]
NEW_ENTRIES = ("gvtm_prosody_create", "gvtm_prosody_destroy", "gvtm_prosody_rhythm_host", "gvtm_prosody_point_count", "gvtm_prosody_points_host",
               "gvtm_apply_rhythm_device", "gvtm_place_intonation_device", "gvtm_synthesize_prosody_device")


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def rules():
    made = capi.Rules(dict(np.load(rules_cases.MODEL_0_MALE)))
    yield made
    made.close()


def track_config(cp, macro=1):
    return capi.TrackConfig(control_period_ms=cp, macro_intonation=macro, micro_intonation=1, intonation_drift=0, smooth_intonation=1, initial_pitch=0.0,
                            mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=1000.0 / cp, drift_lowpass_cutoff=4.0)


class Prosodies:
    """One gvtm_prosody per (intonation factor, global tempo) of the golden entries, made on first use."""

    def __init__(self, golden, device=capi.DEVICE_NONE):
        self.golden, self.device, self.made = golden, device, {}

    def of(self, name):
        key = (float(self.golden[name + "__intonation_factor"]), float(self.golden[name + "__global_tempo"]))
        if key not in self.made:
            config = capi.prosody_config(self.golden["intonation"], self.golden["rhythm"], key[0], key[1])
            self.made[key] = capi.Prosody(config, self.golden["vocoid"], self.device)
        return self.made[key]

    def close(self):
        for p in self.made.values():
            p.close()


@pytest.fixture(scope="module")
def prosodies(golden):
    made = Prosodies(golden)
    yield made
    made.close()


def tables(golden, name):
    """A golden entry -> (postures before rhythm, feet, groups, draws or None) as the entries take them."""
    draws = np.ascontiguousarray(golden[name + "__draws"]) if int(golden[name + "__random"]) else None
    return (capi.postures_from_table(golden[name + "__postures"]), capi.feet_from_table(golden[name + "__feet"]),
            capi.tone_groups_from_table(golden[name + "__groups"]), draws)


def own(golden, name):
    """A refusal of prosody_cases.OWN -> (entry, postures before rhythm, feet, groups, points status, rhythm status)"""
    entry, feet, groups, status, rhythm_status = cases.own_tables(name)
    return entry, capi.postures_from_table(golden[entry + "__postures"]), capi.feet_from_table(feet), capi.tone_groups_from_table(groups), status, rhythm_status


def host_chain(golden, rules, prosodies, name):
    """rhythm, the rule, the points, on the host -> (postures after rhythm, events, rule data, onsets, points, status)"""
    postures, feet, groups, draws = tables(golden, name)
    cp = int(golden[name + "__cp"])
    after, rhythm_status = prosodies.of(name).rhythm_host(postures, feet)
    assert rhythm_status == 0
    events, rule_data, onsets, rule_status = rules.apply_host(cp, after)
    points, status = prosodies.of(name).points_host(cp, after, feet, groups, draws, rule_data, onsets, rule_status)
    return after, events, rule_data, onsets, points, status


def test_the_case_table_covers_what_it_was_written_for(golden):
    assert {e.split(".")[0] for e in ENTRIES} == set(cases.CASES)
    assert {int(golden[n + "__cp"]) for n in ENTRIES} == {1, 2, 3, 4}
    assert len(golden["points_64__points"]) == capi.MAX_INTONATION_POINTS
    assert {int(t) for n in ENTRIES for t in golden[n + "__groups"][:, 2]} >= {0, 1, 2, 3, 4, 5}
    assert max(len(golden[n + "__groups"]) for n in ENTRIES) == 3
    assert sum(int(golden[n + "__random"]) for n in ENTRIES) >= 4 and golden["intonation"][0] == np.float32(-40.0)
    # the random cases: three seeds, three different contours on one utterance
    seeds = [golden["random_%d__points" % s] for s in (1, 20240229, 4294967295)]
    assert not np.array_equal(seeds[0], seeds[1]) and not np.array_equal(seeds[1], seeds[2])
    # a foot without a vocoid, a posture in no foot, two points at one beat
    vocoid = golden["vocoid"]
    feet, ids = golden["no_vocoid__feet"], golden["no_vocoid__postures"][:, 0].astype(int)
    assert any(not vocoid[ids[int(f[0]): int(f[1]) + 1]].any() for f in feet)
    assert golden["outside_feet__feet"][-1, 1] < len(golden["outside_feet__postures"]) - 1
    # a beat + offset below zero: the time stored behind the push is not minTime
    rows, points = golden["negative_time__rule_data"], golden["negative_time__points"]
    assert rows[0, 7] + golden["intonation"][0] < 0 and points[0, 0] < points[1, 0] < points[0, 0] + 2.0 * 4
    rows = golden["one_rule__rule_data"]
    assert int(golden["one_rule__feet"][1, 0]) == 2 and int(golden["one_rule__feet"][2, 0]) == 3 and rows[1, 1] <= 2 and rows[1, 2] >= 3


@pytest.mark.parametrize("name", ENTRIES)
def test_rhythm_is_the_references(golden, prosodies, name):
    postures, feet, _, _ = tables(golden, name)
    after, status = prosodies.of(name).rhythm_host(postures, feet)
    assert status == 0
    assert np.array_equal(after["tempo"].view(np.uint64), golden[name + "__tempo_after"].view(np.uint64))
    for field in ("posture", "marked", "rule_tempo"):
        assert np.array_equal(after[field], postures[field])
    in_place, status = prosodies.of(name).rhythm_host(postures, feet, in_place=True)
    assert status == 0 and np.array_equal(as_bits(in_place), as_bits(after))


@pytest.mark.parametrize("name", ENTRIES)
def test_points_are_the_references(golden, rules, prosodies, name):
    _, feet, groups, _ = tables(golden, name)
    after, events, rule_data, onsets, points, status = host_chain(golden, rules, prosodies, name)
    assert np.array_equal(as_bits(rule_data), as_bits(golden_rule_data(golden, name)))
    assert np.array_equal(onsets.view(np.uint64), golden[name + "__onsets"].view(np.uint64))
    want = capi.points_from_table(golden[name + "__points"])
    assert status == 0 and len(points) == len(want) == capi.prosody_point_count(len(after), feet, groups)
    assert np.array_equal(as_bits(points), as_bits(want)), (points, want)


@pytest.mark.parametrize("name", ENTRIES)
def test_points_under_the_intonation_rule_give_the_references_merged_list(golden, rules, prosodies, name):
    _, events, _, _, points, _ = host_chain(golden, rules, prosodies, name)
    merged, status = capi.intonation_apply_host(track_config(int(golden[name + "__cp"])), events, points)
    want = capi.events_from_table(golden[name + "__merged"])
    assert status == 0 and len(merged) == len(want) and want["has_interp"].sum() == len(points)
    assert np.array_equal(as_bits(merged), as_bits(want))


@pytest.mark.parametrize("name", sorted(cases.OWN))
def test_refusals(golden, rules, prosodies, name):
    entry, postures, feet, groups, want, want_rhythm = own(golden, name)
    after, rhythm_status = prosodies.of(entry).rhythm_host(postures, feet)
    assert rhythm_status == want_rhythm
    if rhythm_status:
        after = postures
    _, rule_data, onsets, rule_status = rules.apply_host(4, after)
    points, status = prosodies.of(entry).points_host(4, after, feet, groups, None, rule_data, onsets, rule_status)
    count = capi.prosody_point_count(len(postures), feet, groups)
    assert status == want and len(points) == (count if want == 0 else 0)
    if want == capi.PROSODY_BAD_STRUCTURE:
        assert count == -1
    elif want == capi.PROSODY_TOO_MANY:
        assert count == capi.MAX_INTONATION_POINTS + 1
    elif len(groups) == 0:
        assert count == 0


def test_refusals_that_need_no_table_of_their_own(golden, rules, prosodies):
    name = "two_groups"
    postures, feet, groups, _ = tables(golden, name)
    after, events, rule_data, onsets, points, status = host_chain(golden, rules, prosodies, name)
    p = prosodies.of(name)
    assert status == 0 and len(points) == 7
    # the rules entry refused the utterance; no rows; a row short, so that the last postures lie in none
    for args in ((rule_data, 2), (rule_data[:0], 0), (rule_data[:3], 0)):
        got, status = p.points_host(4, after, feet, groups, None, args[0], onsets, rule_status=args[1])
        assert status == capi.PROSODY_NO_RULES and len(got) == 0
    # a posture id outside the vocoid table
    bad = after.copy()
    bad["posture"][3] = len(golden["vocoid"])
    assert p.points_host(4, bad, feet, groups, None, rule_data, onsets)[1] == capi.PROSODY_BAD_STRUCTURE
    # draws, parameters and onsets that are not finite
    draws = np.full((len(feet), 2), 0.5)
    assert p.points_host(4, after, feet, groups, draws, rule_data, onsets)[1] == 0
    draws[1, 1] = np.inf
    assert p.points_host(4, after, feet, groups, draws, rule_data, onsets)[1] == capi.PROSODY_BAD_VALUE
    nan_groups = groups.copy()
    nan_groups["param"][1, 3] = np.nan
    assert p.points_host(4, after, feet, nan_groups, None, rule_data, onsets)[1] == capi.PROSODY_BAD_VALUE
    nan_rows = rule_data.copy()
    nan_rows["beat"][-1] = np.nan
    assert p.points_host(4, after, feet, groups, None, nan_rows, onsets)[1] == capi.PROSODY_BAD_VALUE
    # more points than the caller's room is a bad call, not a status
    with pytest.raises(capi.GvtmError):
        p.points_host(4, after, feet, groups, None, rule_data, onsets, capacity=6)
    with pytest.raises(capi.GvtmError):
        p.points_host(5, after, feet, groups, None, rule_data, onsets)


def test_create_refuses_a_model_without_the_category_and_numbers_that_are_not_finite(golden):
    config = capi.prosody_config(golden["intonation"], golden["rhythm"])
    with pytest.raises(capi.GvtmError):
        capi.Prosody(config, None)
    for key in ("time_offset", "intonation_factor", "marked_div", "global_tempo"):
        bad = config.copy()
        bad[key] = np.nan
        with pytest.raises(capi.GvtmError):
            capi.Prosody(bad, golden["vocoid"])
    p = capi.Prosody(config, golden["vocoid"])
    with pytest.raises(capi.GvtmError) as e:  # a host-only object has no device entry
        p.apply_rhythm_device(None, None, 0, None, None, 0, 0, None)
    assert e.value.args[0] == 2 or "GVTM_DEVICE_NONE" in str(e.value)
    p.close()


def test_entries_are_in_the_header_the_export_map_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    exports = open(os.path.join(ROOT, "gama_tts_amd", "csrc", "exports_vtm.map")).read()
    assert re.search(r"global:\s*gvtm_\*;", exports)
    lib = capi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.PROTOTYPES and hasattr(lib, name), name
    for struct in ("gvtm_foot", "gvtm_tone_group", "gvtm_prosody_config"):
        assert re.search(r"struct %s \{" % struct, header) and "typedef struct %s %s;" % (struct, struct) in header
    assert (capi.FOOT_DTYPE.itemsize, capi.TONE_GROUP_DTYPE.itemsize, capi.PROSODY_CONFIG_DTYPE.itemsize) == (24, 32, 112)


def test_the_vocoid_table_of_0_male(golden):
    names = [str(n) for n in np.load(rules_cases.MODEL_0_MALE)["posture_names"]]
    vocoid = golden["vocoid"]
    assert vocoid.dtype == np.uint8 and len(vocoid) == len(names)
    assert all(vocoid[names.index(n)] for n in ("a", "e", "i", "uh", "uu")) and not any(vocoid[names.index(n)] for n in ("#", "^", "s", "t", "m"))
    if os.path.exists(REF_ARTIC):  # a fresh compile of the reference's database gives the table the reference's Model gave
        fresh = control_model.compile_model(REF_ARTIC)["vocoid"]
        assert fresh.dtype == np.uint8 and np.array_equal(fresh, vocoid)
    assert "vocoid" not in control_model.ARRAYS
    assert control_model.compile_model(rules_cases.synthetic_xml())["vocoid"] is None  # a database without the category
