"""Pins the float instantiation of the VocalTractModel5 restatement (oracle/vtm_oracle_body.inc, v5_*, TFloat = float) bit
for bit against vectors of the real VocalTractModel5<float,1> (tests/golden/vtm5f_golden.npz, made by
tests/golden/make_model5_golden.py): the sine waveform, a constant mouth impedance, no noise modulation, tn_min != tn_max,
22.05 kHz at a 500 Hz control rate, and 44.1 kHz at 106 frames (a flush-overrun length of the float converter)."""
import numpy as np
import pytest

import model5_cases as cases


@pytest.mark.parametrize("case", cases.CASES["vtm5f"], ids=lambda c: c["name"])
def test_float_oracle5_matches_reference_vector(case):
    m, tr = cases.check_oracle_vector(case, None)
    assert tr.shape[0] == m["frames"] <= 120
    assert round(m["fs"] / case["crate"]) * tr.shape[0] == m["steps"]


def test_the_106_frame_vector_sits_on_a_flush_overrun_of_the_float_converter():
    """44.1 kHz: 106 frames give 924 samples more than 105, and 107 give 571 fewer than 106."""
    import oracle
    case = cases.by_name("ovr_m5f_44k_106f")
    cfg = cases.oracle_config(case)
    n = {f: oracle.synthesize5(cfg, np.zeros((f, 16), np.float32))[0].size for f in (105, 106, 107)}
    assert n[106] == cases.load("vtm5f")["manifest"][case["name"]]["n"]
    assert n[106] - n[105] == 924 and n[107] - n[106] == -571
