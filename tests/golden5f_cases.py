"""Parity fixtures of VocalTractModel5<float,1> (the 5_male voice; oracle/ref_driver.cpp's model "5f"), beyond the three
float vectors of tests/golden5_cases.py: the source and impedance switches of the class, the 22.05 kHz / 500 Hz rate
class and a flush-overrun length of the float converter (44.1 kHz: 106 frames give 924 samples more than 105, 107 give
571 fewer than 106).

Shared by tests/golden/make_vtm5f_golden.py (runs the REAL reference, oracle/_ref/ref_vtm), tests/test_oracle5f_vs_golden.py
(the float oracle), tests/test_capi_model5_float_cpu.py (design-only plans) and tests/test_gpu_model5_float.py (the device).
Every case has at most 120 frames."""
import json
import os

import numpy as np

import golden5_cases
import oracle

C = golden5_cases.C

CASES = [
    C("sine_m5f", ("random", 120, 5, True), model="5f", store="digest", waveform=1),
    C("constant_mouth_m5f", ("random", 120, 5, True), model="5f", store="digest", constant_radius_mouth_impedance="true",
      mouth_impedance_radius=1.2),
    C("no_modulation_m5f", ("random", 120, 5, True), model="5f", store="digest", noise_modulation=0),
    C("tn_delta_m5f", ("random", 120, 5, True), model="5f", store="digest", glottal_pulse_tn_min=16.0, glottal_pulse_tn_max=32.0),
    C("rand7_m5f_22k_crate500", ("random", 120, 7, True), model="5f", rate=22050.0, crate=500.0),
    C("ovr_m5f_44k_106f", ("random", 120, 6, False, 106), model="5f", rate=44100.0),
]

DIGEST_STRIDE = golden5_cases.DIGEST_STRIDE
track_for = golden5_cases.track_for
GOLDEN = os.path.join(oracle.GOLDEN_DIR, "vtm5f_golden.npz")

_golden = None


def golden5f():
    """tests/golden/vtm5f_golden.npz: the reference's samples (full or strided) and the manifest, loaded once."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN, allow_pickle=False)
        data = {k: z[k] for k in z.files}
        data["manifest"] = json.loads(bytes(data.pop("manifest_json")).decode())
        _golden = data
    return _golden


def config_dict(case):
    """The merged 5_male configuration keys of a case."""
    d = oracle.read_config_file(oracle.VOICE5_MALE)
    d.update({k: str(v) for k, v in case["overrides"].items()})
    return d


def oracle_config(case):
    return oracle.config5_from_dict(config_dict(case), case["rate"], case["float_model"])
