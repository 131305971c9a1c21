"""Pins the VocalTractModel5 restatement (oracle/vtm_oracle_body.inc, v5_*) bit for bit against vectors of
the real reference classes (tests/golden/vtm5_golden.npz, made by tests/golden/make_model5_golden.py): what the
device tests of model 5 (test_gpu_model5.py, test_gpu_model5_float.py) lean on.
"""
import numpy as np
import pytest

import golden_cases
import model5_cases as cases
import oracle


@pytest.mark.parametrize("case", cases.CASES["vtm5"], ids=lambda c: c["name"])
def test_oracle5_matches_reference_vector(case, golden):
    m, tr = cases.check_oracle_vector(case, golden)
    assert round(m["fs"] / case["crate"]) * tr.shape[0] == m["steps"]


def test_survey_known_answer_model5(golden5):
    # model 5, 5_male data, const track, 44.1 kHz
    m = golden5["manifest"]["const_m5_44k"]
    assert m["n"] == 88356
    assert m["sum"] == pytest.approx(7.932018498e+00, rel=1e-9)
    assert m["maxabs"] == pytest.approx(1.288747461e+04, rel=1e-9)


def test_model5_internal_rate():
    # speed of sound at 35 C x 30 sections x 100 / 17.5 cm (VocalTractModel5.h:462-465)
    _, rate = oracle.synthesize5(oracle.male5_config(), np.zeros((0, 16), np.float32))
    assert rate == pytest.approx((331.4 + 0.6 * 35.0) * 30 * 100 / 17.5, abs=2e-3)


@pytest.mark.parametrize("model,fm", [("5", 0), ("5f", 1)])
def test_oracle5_matches_reference_binary_on_fresh_tracks(model, fm):
    """Seeded random tracks against what the reference binary produced for them (tests/golden/random_golden.npz)."""
    import tracks
    for seed in (31, 32):
        tr = tracks.random_track(60, seed, seed % 2 == 0)
        out, rate = oracle.synthesize5(oracle.male5_config(48000.0, fm), tr)
        m = golden_cases.check_against_random_golden(out, model, seed)
        assert abs(rate - m["fs"]) < 2e-3
