"""The fixtures of reference model 5: one case table for its four vector files, their loader and what every reader of a
vector needs.  Needs the oracle binding and voice_files only, not the product.

Shared by tests/golden/make_model5_golden.py (runs the REAL reference, oracle/_ref/ref_vtm), the four
test_oracle5*_vs_golden.py (the oracles), the test_capi_model5*_cpu.py and test_capi_voices5_cpu.py (design-only plans) and
the test_gpu_model5*.py, test_gpu_voices5.py and test_gpu_voices_stream.py (the device); tests/test_model5_cases.py holds
the table to the files.

A case: name, fixture (CASES[fixture] lists it, tests/golden/<fixture>_golden.npz holds its vector), voice (one of the five
5_male variants, tests/golden/voice5_*.txt), overrides on the voice file, model ("5" = VocalTractModel5<double,1> from the
factory, vtm/VocalTractModel.cpp:47-48; "5f" = VocalTractModel5<float,1> instantiated by oracle/ref_driver.cpp) and
float_model (1 for "5f"), output rate, control rate, track recipe (golden_cases.track_for) and store: "full" stores the
output, "digest" every DIGEST_STRIDE-th sample, "tail" that and the last OVERRUN_TAIL samples; the manifest has the count
and the SHA-256 of all.

  vtm5      the male voice, both classes (17 double, 3 float): SURVEY.md section 0's const track, the switches of the class.
  vtm5f     the male voice in float beyond those three: the source and impedance switches, the 22.05 kHz / 500 Hz rate
            class and a flush-overrun length of the float converter (44.1 kHz: 106 frames give 924 samples more than 105,
            107 give 571 fewer than 106).  Every case has at most 120 frames.
  voices5   the double class on the four variants besides male: "hello", 120 consonant-heavy frames and the voice's
            flush-overrun length.
  voices5f  the float class on the same recipes (<voice>_hello_5f, _cons_5f, _ovr_5f: the float converter overruns at the
            lengths the double one does; make_model5_golden.py asserts count(f) > count(f + 1)), and both classes at the
            converter's limits, 12 frames, "full":
              male at 8 200 Hz and baby at 19 200 Hz: down-sampling pad 96, the largest the plans accept (vtm_design.hpp:
                kMaxPad; the kernel's ring is sized for it); baby has 564 steps per frame;
              female at 211 440 Hz: output rate / internal rate exactly 3.0 in float (70 480 Hz x 3), the largest ratio the
                plans accept.  In double the internal rate (331.4 + 0.6 * 35) * 3000 / 15 comes out as 70 480 Hz exactly as
                well, the ratio is exactly 3.0 and gvtm_plan_create_model5 accepts it: the double case uses the same rate
                (the next double above 211 440 Hz is refused)."""
import functools
import hashlib
import json
import os

import numpy as np

import golden_cases
import oracle
import voice_files

NEW_VOICES = voice_files.VOICES[1:]
RATE, CRATE = 48000.0, 250.0
DIGEST_STRIDE = golden_cases.DIGEST_STRIDE
OVERRUN_TAIL = golden_cases.OVERRUN_TAIL
track_for = golden_cases.track_for

# Internal rate (331.4 + 0.6 * 35) * 30 * 100 / L Hz (VocalTractModel5.h:462-465) and control steps per 250 Hz frame
TRACT_CM = {"male": 17.5, "female": 15.0, "large_child": 12.5, "small_child": 10.0, "baby": 7.5}
STEPS_PER_FRAME = {"male": 242, "female": 282, "large_child": 338, "small_child": 423, "baby": 564}

# a frame count of each voice whose converter runs into the flush overrun (an extra lap of the 1024-sample ring after the
# last automatic dataEmpty(); vtm_design.hpp: src_flush_overrun), and its output rate: the shortest at 48 kHz, except for
# female, which overruns at no length up to 6000 frames at 48 kHz (at 44.1 kHz: 167, 658, 2131, ...)
OVERRUN_FRAMES = {"female": 167, "large_child": 295, "small_child": 975, "baby": 337}
OVERRUN_RATE = {"female": 44100.0, "large_child": RATE, "small_child": RATE, "baby": RATE}

MAX_PAD = 96  # the largest down-sampling pad a model 5 plan accepts
LIMIT_TRACK = ("random", 12, 78, True)
# (voice, output rate, what the rate sits on)
LIMITS = [("male", 8200.0, "pad96"), ("baby", 19200.0, "pad96"), ("female", 211440.0, "ratio3")]
DOUBLE_RATIO3_RATE = 211440.0  # the highest rate the double class takes for female: 3.0 x, too (module docstring)

CASES = {"vtm5": [], "vtm5f": [], "voices5": [], "voices5f": []}


def C(fixture, name, track, voice="male", model="5", rate=RATE, crate=CRATE, store="full", **overrides):
    CASES[fixture].append(dict(name=name, fixture=fixture, voice=voice, overrides=overrides, model=model,
                               float_model=1 if model == "5f" else 0, rate=rate, crate=crate, track=track, store=store))


# const track, 44.1 kHz -> 88356 samples
C("vtm5", "const_m5_44k", ("const", 500), rate=44100.0, store="digest")
C("vtm5", "ramp_m5", ("ramp", 500), store="digest")
C("vtm5", "cons2000_m5", ("random", 500, 2000, True), store="digest")
C("vtm5", "hello_m5", ("hello",), store="digest")
C("vtm5", "rand5_m5", ("random", 120, 5, True))
C("vtm5", "rand6_m5_44k", ("random", 120, 6, False), rate=44100.0)
C("vtm5", "rand7_m5_22k_crate500", ("random", 120, 7, True), rate=22050.0, crate=500.0)
C("vtm5", "bypass_m5", ("random", 120, 5, True), bypass=1)
C("vtm5", "sine_m5", ("random", 120, 5, True), waveform=1)
C("vtm5", "tn_delta_m5", ("random", 120, 5, True), glottal_pulse_tn_min=16.0, glottal_pulse_tn_max=32.0)
C("vtm5", "no_modulation_m5", ("random", 120, 5, True), noise_modulation=0)
C("vtm5", "constant_mouth_m5", ("random", 120, 5, True), constant_radius_mouth_impedance="true", mouth_impedance_radius=1.2)
C("vtm5", "female_m5", ("random", 120, 6, False), vocal_tract_length=15.0, glottal_pulse_tn_min=32.0,
  glottal_pulse_tn_max=32.0, breathiness=1.5)
C("vtm5", "radius_coefs_m5", ("random", 120, 8, True), radius_3_coef=1.3, global_radius_coef=0.9,
  global_nasal_radius_coef=1.1, vocal_tract_length_offset=1.0, loss_factor=0.8, max_glottal_loss=5.0, min_glottal_loss=1.0)
C("vtm5", "silence_m5", ("silence", 40))
C("vtm5", "one_frame_m5", ("random", 120, 5, True, 1))
C("vtm5", "three_frames_m5", ("random", 120, 5, True, 3))
C("vtm5", "rand5_m5f", ("random", 120, 5, True), model="5f")
C("vtm5", "cons2000_m5f", ("random", 500, 2000, True), model="5f", store="digest")
C("vtm5", "bypass_m5f", ("random", 120, 5, True), model="5f", bypass=1)

C("vtm5f", "sine_m5f", ("random", 120, 5, True), model="5f", store="digest", waveform=1)
C("vtm5f", "constant_mouth_m5f", ("random", 120, 5, True), model="5f", store="digest",
  constant_radius_mouth_impedance="true", mouth_impedance_radius=1.2)
C("vtm5f", "no_modulation_m5f", ("random", 120, 5, True), model="5f", store="digest", noise_modulation=0)
C("vtm5f", "tn_delta_m5f", ("random", 120, 5, True), model="5f", store="digest", glottal_pulse_tn_min=16.0,
  glottal_pulse_tn_max=32.0)
C("vtm5f", "rand7_m5f_22k_crate500", ("random", 120, 7, True), model="5f", rate=22050.0, crate=500.0)
C("vtm5f", "ovr_m5f_44k_106f", ("random", 120, 6, False, 106), model="5f", rate=44100.0)

for _i, _v in enumerate(NEW_VOICES):
    _ovr = ("random", OVERRUN_FRAMES[_v], 60 + _i, True)
    C("voices5", "%s_hello" % _v, ("hello",), _v, store="digest")
    C("voices5", "%s_cons" % _v, ("random", 120, 50 + _i, True), _v)
    C("voices5", "%s_ovr_%df" % (_v, OVERRUN_FRAMES[_v]), _ovr, _v, store="tail", rate=OVERRUN_RATE[_v])
    C("voices5f", "%s_hello_5f" % _v, ("hello",), _v, "5f", store="digest")
    C("voices5f", "%s_cons_5f" % _v, ("random", 120, 50 + _i, True), _v, "5f")
    C("voices5f", "%s_ovr_5f" % _v, _ovr, _v, "5f", store="tail", rate=OVERRUN_RATE[_v])
VOICE_CASES = list(CASES["voices5f"])
for _v, _rate, _what in LIMITS:
    C("voices5f", "%s_%s_5f" % (_v, _what), LIMIT_TRACK, _v, "5f", rate=_rate)
    C("voices5f", "%s_%s_5" % (_v, _what), LIMIT_TRACK, _v, "5", rate=DOUBLE_RATIO3_RATE if _what == "ratio3" else _rate)
LIMIT_CASES = CASES["voices5f"][len(VOICE_CASES):]
FLOAT_CASES = [c for c in CASES["voices5f"] if c["float_model"]]
DOUBLE_CASES = [c for c in CASES["voices5f"] if not c["float_model"]]

# the male voice: every float vector (three of vtm5, all of vtm5f) and the double ones
MALE_FLOAT_CASES = [c for c in CASES["vtm5"] if c["float_model"]] + CASES["vtm5f"]
MALE_DOUBLE_CASES = [c for c in CASES["vtm5"] if not c["float_model"]]


def by_name(name):
    return next(c for cs in CASES.values() for c in cs if c["name"] == name)


def golden_path(fixture):
    return os.path.join(oracle.GOLDEN_DIR, fixture + "_golden.npz")


@functools.lru_cache(maxsize=None)
def load(fixture):
    """tests/golden/<fixture>_golden.npz: the reference's samples (full, strided, tail) by key and, as "manifest", what it
    reported per case; loaded once."""
    z = np.load(golden_path(fixture), allow_pickle=False)
    data = {k: z[k] for k in z.files}
    data["manifest"] = json.loads(bytes(data.pop("manifest_json")).decode())
    return data


def config_keys(case):
    """The configuration keys of a case: its voice file with its overrides."""
    d = oracle.read_config_file(voice_files.voice_path(case["voice"], model5=True))
    d.update({k: str(v) for k, v in case["overrides"].items()})
    return d


def oracle_config(case):
    return oracle.config5_from_dict(config_keys(case), case["rate"], case["float_model"])


def voice_oracle_config(voice, rate=RATE, float_model=0, overrides=None):
    """oracle_config by hand, for what is no case."""
    return oracle_config(dict(voice=voice, rate=rate, float_model=float_model, overrides=overrides or {}))


def stored(case, out):
    """[(what `out` has to equal, the array's key in the fixture)] of a case, as its store says."""
    name = case["name"]
    if case["store"] == "full":
        return [(out, name + "__out")]
    parts = [(out[::DIGEST_STRIDE], name + "__strided")]
    if case["store"] == "tail":
        parts.append((out[-OVERRUN_TAIL:], name + "__tail"))
    return parts


def check_oracle_vector(case, golden):
    """Asserts what every oracle-against-vector test asserts: the internal rate, the count, the SHA-256 and the stored
    samples bit for bit -> (the case's manifest entry, its track)."""
    data = load(case["fixture"])
    m = data["manifest"][case["name"]]
    tr = track_for(case, golden)
    out, rate = oracle.synthesize5(oracle_config(case), tr, case["crate"])
    assert abs(rate - m["fs"]) < 2e-3  # the internal rate is not an integer (VocalTractModel5.h:465; reported in mHz)
    assert out.size == m["n"]
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"]
    for got, key in stored(case, out):
        assert np.array_equal(got, data[key]), key
    return m, tr
