"""Pins the float instantiation of the VocalTractModel5 restatement (oracle/vtm_oracle_body.inc, v5_*, TFloat = float) bit
for bit against vectors of the real VocalTractModel5<float,1> for the four 5_male variants besides male, and both
instantiations at the limits of the sample-rate converter -- down-sampling pad 96, output rate = 3 x the internal rate --
(tests/golden/voices5f_golden.npz, made by tests/golden/make_model5_golden.py): the bar of test_oracle5f_vs_golden.py
(count, SHA-256, full / strided / tail samples), on internal rates of 70.5 to 141 kHz and at ratios of 0.136 and 3.0,
which the 5_male float vectors never reach.  The device tests of the float class on these voices
(test_gpu_model5_float_voices.py) lean on the oracle this file holds to the reference."""
import hashlib

import numpy as np
import pytest

import model5_cases as cases
import oracle

CASES = cases.CASES["voices5f"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle5_matches_reference_vector(case, golden):
    m, tr = cases.check_oracle_vector(case, golden)
    assert tr.shape[0] == m["frames"]
    assert m["steps"] == cases.STEPS_PER_FRAME[case["voice"]] * tr.shape[0]


@pytest.mark.parametrize("case", [c for c in CASES if c["store"] == "tail"], ids=lambda c: c["name"])
def test_overrun_vectors_sit_on_a_flush_overrun_of_the_float_converter(case):
    cfg = cases.voice_oracle_config(case["voice"], case["rate"], 1)
    f = cases.OVERRUN_FRAMES[case["voice"]]
    n = {k: oracle.synthesize5(cfg, np.zeros((k, 16), np.float32))[0].size for k in (f - 1, f, f + 1)}
    assert n[f] == cases.load("voices5f")["manifest"][case["name"]]["n"]
    assert n[f] > n[f + 1] > n[f - 1]
    assert n[f] - n[f + 1] < cases.OVERRUN_TAIL  # the stored tail covers the extra lap of the ring


def test_every_new_voice_and_every_limit_is_pinned():
    assert sorted({c["voice"] for c in cases.VOICE_CASES}) == sorted(cases.NEW_VOICES)
    for v in cases.NEW_VOICES:
        assert {c["store"] for c in cases.VOICE_CASES if c["voice"] == v} == {"digest", "full", "tail"}
    assert all(c["float_model"] for c in cases.VOICE_CASES)
    for voice, _, what in cases.LIMITS:
        assert {c["model"] for c in cases.LIMIT_CASES if c["voice"] == voice and what in c["name"]} == {"5", "5f"}
    assert set(cases.load("voices5f")["manifest"]) == {c["name"] for c in CASES}


# ---- the vectors discriminate: a float class that is subtly something else fails them ------------------------------------

@pytest.mark.parametrize("case", [c for c in cases.FLOAT_CASES if c["store"] == "full"], ids=lambda c: c["name"])
def test_the_double_class_narrowed_to_float_is_not_the_float_class(case, golden):
    data = cases.load("voices5f")
    tr = cases.track_for(case, golden)
    rate = cases.DOUBLE_RATIO3_RATE if "ratio3" in case["name"] else case["rate"]
    out, _ = oracle.synthesize5(cases.voice_oracle_config(case["voice"], rate, 0), tr, case["crate"])
    ref = data[case["name"] + "__out"]
    assert out.size != ref.size or not np.array_equal(out, ref)


@pytest.mark.parametrize("case", cases.VOICE_CASES, ids=lambda c: c["name"])
def test_the_male_voice_is_no_other_voice(case, golden):
    m = cases.load("voices5f")["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    out, _ = oracle.synthesize5(cases.voice_oracle_config("male", case["rate"], 1), tr, case["crate"])
    assert out.size != m["n"] or hashlib.sha256(out.tobytes()).hexdigest() != m["sha256"]
