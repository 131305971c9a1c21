"""Pins the VocalTractModel5 restatement (oracle/vtm_oracle_body.inc, v5_*) bit for bit against vectors of the real
reference classes for the four 5_male variants besides male (tests/golden/voices5_golden.npz, made by
tests/golden/make_voices5_golden.py): the bar of test_oracle5_vs_golden.py, on voices whose internal rates (70.5 to
141 kHz) the 5_male vectors never reach."""
import hashlib

import numpy as np
import pytest

import golden5_voices_cases as cases
import oracle
import voice_files


@pytest.fixture(scope="module")
def golden5v():
    return voice_files.golden5v()


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_oracle5_matches_reference_vector(case, golden, golden5v):
    m = golden5v["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    out, rate = oracle.synthesize5(cases.oracle_config(case["voice"], case["rate"]), tr, cases.CRATE)
    assert abs(rate - m["fs"]) < 2e-3
    assert round(m["fs"] / cases.CRATE) * tr.shape[0] == m["steps"]
    assert m["steps"] == cases.STEPS_PER_FRAME[case["voice"]] * tr.shape[0]
    assert out.size == m["n"]
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"]
    if case["store"] == "full":
        assert np.array_equal(out, golden5v[case["name"] + "__out"])
    else:
        assert np.array_equal(out[:: cases.DIGEST_STRIDE], golden5v[case["name"] + "__strided"])
    if case["store"] == "tail":
        assert np.array_equal(out[-cases.OVERRUN_TAIL:], golden5v[case["name"] + "__tail"])


def test_every_new_voice_is_pinned():
    assert sorted({c["voice"] for c in cases.CASES}) == sorted(cases.NEW_VOICES)
    for v in cases.NEW_VOICES:
        assert {c["store"] for c in cases.CASES if c["voice"] == v} == {"digest", "full", "tail"}
