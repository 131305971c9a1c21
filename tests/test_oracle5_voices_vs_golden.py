"""Pins the VocalTractModel5 restatement (oracle/vtm_oracle_body.inc, v5_*) bit for bit against vectors of the real
reference classes for the four 5_male variants besides male (tests/golden/voices5_golden.npz, made by
tests/golden/make_model5_golden.py): the bar of test_oracle5_vs_golden.py, on voices whose internal rates (70.5 to
141 kHz) the 5_male vectors never reach."""
import pytest

import model5_cases as cases

CASES = cases.CASES["voices5"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle5_matches_reference_vector(case, golden):
    m, tr = cases.check_oracle_vector(case, golden)
    assert round(m["fs"] / cases.CRATE) * tr.shape[0] == m["steps"]
    assert m["steps"] == cases.STEPS_PER_FRAME[case["voice"]] * tr.shape[0]


def test_every_new_voice_is_pinned():
    assert sorted({c["voice"] for c in CASES}) == sorted(cases.NEW_VOICES)
    for v in cases.NEW_VOICES:
        assert {c["store"] for c in CASES if c["voice"] == v} == {"digest", "full", "tail"}
